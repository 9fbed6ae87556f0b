"""Inverse skinning on the GPU (``include/ag_inverse_skinning.h``, ``WeightVolume.gradient_volume`` / ``root_find``,
``inverse_skinning.transform_live2cano`` / ``transform_cano2live``) against ``inverse_skinning_oracle.py``.

Bars, none derived from the kernel's output: 4 x the worst |float32 oracle - float64 oracle| on the same input plus 2^-22 x the largest
magnitude (of the gradient; of the bounds for points).  Root finding is compared where the float32 and the float64 oracle visited the
same node at every iteration (the weights are the NEAREST node's: a run that steps into another cell solves another equation); the
share left out is capped at 1 % per case and printed.  Ten iterations run on the smooth volumes of the oracle, uniform-random volumes
only for one.  The exact-grid case and the singular step are compared with the float32 oracle itself: the header states every
operation, and where the node choice is exact there is nothing left to differ.

The round trip (``transform_cano2live`` then ``transform_live2cano``) asks that the residual of the solver's own equation,
|sum_j w_j(node(xc)) (A_j xc) - xt|, is no larger after the refinement than before, for EVERY refined point.  That is a property of the
iteration inside one cell, where the equation is one affine map; from cell to cell the equation changes, so the canonical points are
taken near grid nodes (``points_near_nodes``: on generic points a few per cent end in a neighbouring cell with a larger residual, in
the float64 oracle as in the reference's algorithm).  A residual below 2^-22 x the largest |bound| is below what float32 coordinates
can express and counts as zero.

Known without a GPU: the kernels' source, compiled for the host and walked lane by lane under the address and undefined-behaviour
sanitizers (``profiles/ub/inverse_skinning_host_walk.hip``), equals the float32 oracle bit for bit in both gradient modes.
Measured on the MI355X: the gradient, the initial guess and the root finder equal the float32 oracle BIT FOR BIT on every case below; no
point is left out (0.0000 % on all ten cases); worst |xc - float64 oracle| 1.011e-7 / 8.93e-8 / 9.16e-8 / 8.17e-8 / 9.63e-8 on the
ten-iteration cases (bars 6.67e-7 / 6.19e-7 / 6.29e-7 / 5.89e-7 / 6.47e-7), worst gradient deviation 2.9e-7 (bar 1.6e-6, random volume),
initial guess 3.7e-7 (bar 1.8e-6); the round trip takes the mean residual of 585 refined points from 1.3e-3 to 2.4e-8 (max 1.4e-7), none
worse; the whole file runs in 4 s.  Every test prints its own figures.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_skinning_oracle as iso  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 0.01


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _volume(case):
    from animatablegaussians_amd.weight_volume import WeightVolume
    vol = WeightVolume(_t(case["volume"]), _t(case["volume"]), case["bounds"], np.zeros(3, np.float32), case["bounds"])
    assert np.array_equal(vol.voxel_size.cpu().numpy(), case["spacing"]), "the volume's node spacing is not the oracle's float32 (hi - lo) / (R - 1)"
    return vol


@functools.lru_cache(maxsize=None)
def _case(shape, B, n, kind):
    """Inputs of one case -- built once, never modified."""
    c = iso.smooth_case(shape, n=max(n, 1), B=B, offset=0.05 if shape[3] == 55 else 0.02)
    if kind == "random":
        c["volume"] = iso.random_volume(shape)
    if n == 0:
        c["xt"], c["xc_init"] = c["xt"][:, :0], c["xc_init"][:, :0]
    return c


@functools.lru_cache(maxsize=None)
def _oracles(shape, B, n, kind, iterations, masked):
    c = _case(shape, B, n, kind)
    active = _mask(B, n) if masked else None
    args = (c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], c["jnt_mats"], active, 0.1, iterations)
    return iso.root_find(*args, dtype=np.float64), iso.root_find(*args, dtype=np.float32)


def _mask(B, n):
    return (np.arange(B * n).reshape(B, n) % 5) != 2


GRADIENT_CASES = [((9, 7, 5, 6), "smooth"), ((9, 7, 5, 6), "random"), ((16, 16, 16, 55), "smooth"), ((5, 4, 3, 1), "random"), ((2, 3, 2, 128), "random")]


@pytest.mark.parametrize("shape,kind", GRADIENT_CASES)
def test_gradient_volume_against_the_float64_oracle(shape, kind):
    c = _case(shape, 1, 1, kind)
    got = _volume(c).gradient_volume().cpu().numpy()
    o64, o32 = iso.gradient(c["volume"], c["spacing"]), iso.gradient(c["volume"], c["spacing"], np.float32)
    limit, own = iso.bar(o32, o64, np.abs(o64).max())
    dev = np.abs(got.astype(np.float64) - o64)
    X, Y, Z = shape[:3]
    idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1)
    on_face = ((idx == 0) | (idx == np.array(shape[:3]) - 1)).sum(-1)                   # 1: face, 2: edge, 3: corner nodes (zero padding acts)
    worst = {k: float(dev[on_face == k].max()) for k in range(4) if (on_face == k).any()}
    print(f"{shape} {kind}: worst |gradient - float64 oracle| by nodes on 0 / 1 / 2 / 3 faces {worst}, bar {limit:.3e} (float32 oracle's own "
          f"{own:.3e}); equals the float32 oracle bit for bit: {np.array_equal(got, o32)}")
    assert got.shape == shape + (3,) and 3 in worst and dev.max() <= limit


@pytest.mark.parametrize("shape", [(9, 7, 5, 6), (5, 4, 3, 1)])
def test_exact_grid_pins_the_node_choice(shape):
    c, want = iso.exact_grid_case(shape)
    vol = _volume(c)
    got = vol.root_find(_t(c["xt"]), _t(c["xc_init"]), _t(c["jnt_mats"]), iterations=1).cpu().numpy()
    o32, n32 = iso.root_find(c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], c["jnt_mats"], iterations=1, dtype=np.float32)
    assert np.array_equal(n32[0], want)                                                 # halves round away from zero, both ends clamp
    bad = (got != o32).any(-1)
    print(f"{shape}: {want.shape[1]} points on nodes, halves and outside the bounds; points that differ from the float32 oracle: {int(bad.sum())}")
    assert np.array_equal(got, o32)


ROOT_CASES = [  # shape, B, N, volume, iterations, masked
    ((9, 7, 5, 6), 1, iso.N_POINTS, "smooth", 10, False),
    ((9, 7, 5, 6), 2, iso.N_POINTS, "smooth", 10, True),
    ((16, 16, 16, 55), 1, iso.N_POINTS, "smooth", 10, True),
    ((16, 16, 16, 55), 2, 67, "smooth", 10, False),
    ((5, 4, 3, 1), 1, iso.N_POINTS, "smooth", 10, False),
    ((16, 16, 16, 55), 1, iso.N_POINTS, "random", 1, False),
    ((9, 7, 5, 6), 2, 1, "random", 1, True),
    ((9, 7, 5, 6), 1, 1, "smooth", 10, False),
    ((5, 4, 3, 1), 2, iso.N_POINTS, "random", 0, True),
    ((9, 7, 5, 6), 1, 0, "smooth", 10, False),
]


@pytest.mark.parametrize("shape,B,n,kind,iterations,masked", ROOT_CASES)
def test_root_find_against_the_float64_oracle(shape, B, n, kind, iterations, masked):
    import torch
    c = _case(shape, B, n, kind)
    vol = _volume(c)
    active = _mask(B, n) if masked else None
    args = (_t(c["xt"]), _t(c["xc_init"]), _t(c["jnt_mats"]))
    kw = dict(active=_t(active) if masked else None, iterations=iterations)
    got_t = vol.root_find(*args, **kw)
    again = vol.root_find(*args, **kw)
    from_volume = vol.root_find(*args, grad_volume=vol.gradient_volume(), **kw)
    assert got_t.shape == (B, n, 3) and torch.equal(got_t, again), "two calls differ"
    assert torch.equal(got_t, from_volume), "grad_volume=None and grad_volume=gradient_volume() differ"
    got = got_t.cpu().numpy()
    if n == 0:
        return
    (o64, n64), (o32, n32) = _oracles(shape, B, n, kind, iterations, masked)
    keep = iso.kept(n32, n64)
    left_out = 1.0 - keep.mean()
    limit, own = iso.bar(o32[keep], o64[keep], np.abs(c["bounds"]).max())
    dev = np.abs(got.astype(np.float64) - o64).max(-1)
    print(f"{shape} B {B} N {n} {kind} iterations {iterations} masked {masked}: left out {left_out:.4%}; worst |xc - float64 oracle| over the kept "
          f"points {dev[keep].max():.3e}, bar {limit:.3e} (float32 oracle's own {own:.3e}); equals the float32 oracle bit for bit: "
          f"{np.array_equal(got, o32)}; moved by up to {np.abs(o64 - c['xc_init']).max():.3e}")
    assert left_out <= CAP and dev[keep].max() <= limit
    if masked:
        assert np.array_equal(got[~active], c["xc_init"][~active]) and (n == 1 or (active.any() and not active.all()))
    if iterations == 0:
        assert np.array_equal(got, c["xc_init"])
    elif n > 1:
        assert (got[keep] != c["xc_init"][keep]).any()
    if B == 2 and n > 1 and iterations:                                                 # each batch its own matrices: batch 1 with batch 0's differs
        swapped, _ = iso.root_find(c["volume"], c["bounds"], c["spacing"], c["xt"][1:], c["xc_init"][1:], c["jnt_mats"][:1], None, 0.1, iterations)
        assert np.abs(swapped[0] - o64[1]).max() > 100 * limit


def test_unbatched_points_are_one_batch():
    import torch
    c = _case((9, 7, 5, 6), 1, 300, "smooth")
    vol = _volume(c)
    xt, xc, mats = _t(c["xt"]), _t(c["xc_init"]), _t(c["jnt_mats"])
    want = vol.root_find(xt, xc, mats)
    got = vol.root_find(xt[0], xc[0], mats[0])
    assert tuple(got.shape) == (300, 3) and torch.equal(got, want[0]) and torch.equal(vol.root_find(xt[0], xc[0], mats), want[0])
    ori = vol.root_find(xt, xc, mats, volume_type="ori")                              # one tensor serves both types in this volume
    assert torch.equal(ori, want) and not torch.equal(vol.root_find(xt, xc, mats, lam=0.0), want)


def test_singular_step_is_plus_one_centimetre():
    c = _case((9, 7, 5, 6), 1, 1, "smooth")
    vol = _volume(c)
    mats = np.zeros_like(c["jnt_mats"])
    got = vol.root_find(_t(c["xt"]), _t(c["xc_init"]), _t(mats), iterations=1).cpu().numpy()
    o32, _ = iso.root_find(c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], mats, iterations=1, dtype=np.float32)
    print(f"zero matrices: xc_init {c['xc_init'][0, 0]}, after one step {got[0, 0]}")
    assert np.isfinite(got).all() and np.array_equal(got, o32) and np.array_equal(got, c["xc_init"] - iso.STEP)


@pytest.mark.parametrize("shape,B,n,with_normals", [((16, 16, 16, 55), 2, iso.N_POINTS, True), ((9, 7, 5, 6), 1, 300, False), ((5, 4, 3, 1), 1, 1, True)])
def test_initial_guess_against_numpy_inverse(shape, B, n, with_normals):
    from animatablegaussians_amd import inverse_skinning as inv
    c = _case(shape, B, n, "smooth")
    J = shape[3]
    rng = np.random.RandomState(9)
    w = rng.uniform(0, 1, (B, n, J)) ** 4 + 1e-3
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    normals = rng.normal(0, 1, (B, n, 3)).astype(np.float32) if with_normals else None
    got = inv.initial_guess(_t(c["xt"]), _t(w), _t(c["jnt_mats"]), _t(normals) if with_normals else None)
    M = np.einsum("bnj,bjrc->bnrc", w.astype(np.float64), c["jnt_mats"].astype(np.float64))
    M[..., 3, :] = [0, 0, 0, 1]                                                         # the blend as an affine map (the header)
    Mi = np.linalg.inv(M)
    want = [np.einsum("bnrc,bnc->bnr", Mi[..., :3, :3], c["xt"].astype(np.float64)) + Mi[..., :3, 3]]
    o32 = iso.init(c["xt"], w, c["jnt_mats"], normals, np.float32)
    if with_normals:
        want.append(np.einsum("bnrc,bnc->bnr", Mi[..., :3, :3], normals.astype(np.float64)))
    else:
        got, o32 = (got,), (o32,)
    for name, g, o, w64, scale in zip(("points", "normals"), got, o32, want, (np.abs(c["bounds"]).max(), 1.0)):
        limit, own = iso.bar(o, w64, max(scale, np.abs(w64).max()))
        dev = float(np.abs(g.cpu().numpy().astype(np.float64) - w64).max())
        print(f"{shape} B {B} N {n} {name}: worst |init - np.linalg.inv| {dev:.3e}, bar {limit:.3e} (float32 oracle's own {own:.3e}); equals the float32 "
              f"oracle bit for bit: {np.array_equal(g.cpu().numpy(), o)}")
        assert tuple(g.shape) == (B, n, 3) and dev <= limit


@functools.lru_cache(maxsize=None)
def _round_trip():
    """The mesh, its volume, canonical points near nodes, their posed positions and the posed mesh -- built once, never modified."""
    import torch
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd.weight_volume import WeightVolume, grid_axes
    v, f, w, mats = iso.round_trip_inputs()
    vol = WeightVolume.from_body_mesh(_t(v), _t(f), _t(w), res=32)
    bounds = vol.volume_bounds.cpu().numpy()
    nodes = np.stack(np.meshgrid(*grid_axes(bounds, (32, 32, 32)), indexing="ij"), -1)
    cano = iso.points_near_nodes(nodes, np.abs(vol.smpl_sdf_volume.cpu().numpy()), vol.voxel_size.cpu().numpy())
    mats_t = _t(mats)
    posed = inv.transform_cano2live(_t(cano), mats_t, vol)
    live_v = inv.transform_cano2live(_t(v[None]), mats_t, vol)
    mesh = (live_v, _t(f[None]), _t(w[None]))
    torch.cuda.synchronize()
    return vol, mats, mats_t, cano, posed, mesh


def test_round_trip_refinement_never_raises_the_residual():
    import torch
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd import mesh_query
    vol, mats, mats_t, cano, posed, mesh = _round_trip()
    normals = _t(np.random.RandomState(1).normal(0, 1, cano.shape).astype(np.float32))
    guess, near0 = inv.transform_live2cano(posed, mats_t, vol, *mesh, use_root_finding=False, near_thres=0.03)
    refined, refined_n, near = inv.transform_live2cano(posed, mats_t, vol, *mesh, normals=normals, near_thres=0.03)
    pts_w, near_want = mesh_query.calc_blending_weight(posed, *mesh, 0.03)
    assert torch.equal(near, near_want) and torch.equal(near0, near_want) and near.any() and not near.all()
    guess_n = inv.initial_guess(posed, pts_w, inv.rigid_hands(mats_t), normals)[1]
    assert torch.equal(refined_n, guess_n)                                              # normals are not refined
    nonopt = torch.isin(pts_w.argmax(-1), torch.tensor([7, 8, 10, 11], device=posed.device)).cpu().numpy()
    volume, bounds, rigid = vol.diff_weight_volume.cpu().numpy(), vol.volume_bounds.cpu().numpy(), inv.rigid_hands(mats_t).cpu().numpy()
    xt, g, r = posed.cpu().numpy(), guess.cpu().numpy(), refined.cpu().numpy()
    before = np.linalg.norm(iso.forward_nearest(volume, bounds, g, rigid) - xt, axis=-1)
    after = np.linalg.norm(iso.forward_nearest(volume, bounds, r, rigid) - xt, axis=-1)
    floor = 2.0 ** -22 * float(np.abs(bounds).max())
    worse = (after > np.maximum(before, floor)) & ~nonopt
    print(f"{cano.shape[1]} points, {int(nonopt.sum())} kept at the initial guess; residual before: mean {before[~nonopt].mean():.3e} max "
          f"{before[~nonopt].max():.3e}, after: mean {after[~nonopt].mean():.3e} max {after[~nonopt].max():.3e}; worse after: {int(worse.sum())}; "
          f"|refined - canonical| max {np.abs(r - cano).max():.3e}, |guess - canonical| max {np.abs(g - cano).max():.3e}; near: {int(near.sum())}")
    assert 0 < nonopt.sum() < nonopt.size and np.array_equal(r[nonopt], g[nonopt]) and (r[~nonopt] != g[~nonopt]).any()
    assert not worse.any() and after[~nonopt].mean() < 0.25 * before[~nonopt].mean()


def test_with_hand_false_is_the_call_with_the_matrices_overwritten():
    import torch
    from animatablegaussians_amd import inverse_skinning as inv
    vol, mats, mats_t, cano, posed, mesh = _round_trip()
    by_hand = mats_t.clone()
    by_hand[:, 25:40] = by_hand[:, 20:21]
    by_hand[:, 40:55] = by_hand[:, 21:22]
    assert not torch.equal(by_hand, mats_t)
    a, flag_a = inv.transform_live2cano(posed, mats_t, vol, *mesh, with_hand=False)
    b, flag_b = inv.transform_live2cano(posed, by_hand, vol, *mesh, with_hand=True)
    c, _ = inv.transform_live2cano(posed, mats_t, vol, *mesh, with_hand=True)
    assert torch.equal(a, b) and torch.equal(flag_a, flag_b) and not torch.equal(a, c)
    assert torch.equal(inv.transform_cano2live(_t(cano), by_hand, vol, with_hand=True), posed)
    p, n = inv.transform_cano2live(_t(cano), mats_t, vol, normals=_t(cano))
    assert torch.equal(p, posed) and tuple(n.shape) == cano.shape
    with pytest.raises(ValueError, match="55"):
        inv.transform_live2cano(posed, mats_t[:, :54], vol, *mesh)
    six = _case((9, 7, 5, 6), 1, 1, "smooth")
    with pytest.raises(ValueError, match="55 SMPL-X joints"):                           # rigid hands are defined for SMPL-X's joints only
        inv.transform_live2cano(posed, _t(six["jnt_mats"]), _volume(six), *mesh)


def test_refusals_launch_nothing():
    import torch
    c = _case((9, 7, 5, 6), 1, 1, "smooth")
    vol = _volume(c)
    xt, xc, mats = _t(c["xt"]), _t(c["xc_init"]), _t(c["jnt_mats"])
    wide = dict(c, volume=np.zeros((2, 2, 2, 129), np.float32), spacing=((c["bounds"][1] - c["bounds"][0]) / np.float32(1)).astype(np.float32))
    with pytest.raises(ValueError, match="129"):
        _volume(wide).root_find(xt, xc, torch.zeros(1, 129, 4, 4, device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        vol.root_find(xt.cpu(), xc, mats)
    with pytest.raises(ValueError, match="GPU"):
        vol.root_find(xt, xc, mats.cpu())
    with pytest.raises(ValueError, match="active"):
        vol.root_find(xt, xc, mats, active=torch.ones(1, 1, dtype=torch.bool))          # a mask on another device than the volume
    with pytest.raises(ValueError, match="grad_volume"):
        vol.root_find(xt, xc, mats, grad_volume=vol.gradient_volume().cpu())
    with pytest.raises(ValueError, match="jnt_mats"):
        vol.root_find(xt, xc, mats[:, :5])
    with pytest.raises(ValueError, match="iterations"):
        vol.root_find(xt, xc, mats, iterations=-1)
