"""The diffused blend-weight volume on the GPU (``include/ag_weight_diffuse.h``, ``weight_volume.diffuse_weights``,
``WeightVolume.diffuse``) against ``weight_diffuse_oracle.py``: the operator against its float64 restatement, the solve against the
dense direct solution of the same linear system.

Bars, none derived from the kernel's output:
* operator: 4 x the worst |float32 oracle - float64 oracle| on the same input (the rule of ``test_weight_volume_gpu.py``) plus
  2^-22 x the input's largest magnitude;
* solve: |u - direct| <= 4 x the larger of the float32 and float64 oracle CG's own distance from the direct solution at the same
  ``tol`` (the stopping tolerance, not the arithmetic, decides that distance); the float64 relative residual of the returned ``u``
  <= 4 x that of the float32 oracle CG's result; iterations <= 1.5 x the float64 oracle's count (a solver that merely creeps to
  the answer fails it); ``info['true_rel_residual']`` within a factor 2 of the float64 one;
* row sums after ``WeightVolume.diffuse``: ``row_sum_bar(J)``, worked out in the oracle.

Known without a GPU: the kernels' source, compiled for the host and run thread by thread (``profiles/ub/weight_diffuse_host_walk.hip``),
equals the float32 oracle's operator bit for bit on these shapes and takes the float64 oracle's iteration counts (51, 54, 41, 14).
Every test prints its own figures.  Measured on the MI355X: the operator equals the float32 oracle bit for bit on all four shapes;
the solves take 51 / 54 / 41 / 14 iterations, land 2.44e-5 / 2.35e-5 / 2.19e-5 / 5.19e-6 from the direct solution (bars 9.8e-5 / 9.4e-5 /
8.8e-5 / 2.1e-5) and leave float64 relative residuals of 1.008e-5 / 8.51e-6 / 6.54e-6 / 4.30e-6 (the float32 oracle's: 1.007e-5 / 8.50e-6 /
6.50e-6 / 4.31e-6); ``WeightVolume.diffuse`` at (12, 14, 10) x 55 is 4.0e-7 from the oracle with |row sum - 1| <= 1.5e-7.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_query_oracle as mqo  # noqa: E402
import weight_diffuse_oracle as wdo  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(target, fixed, w, spacing) of ``band_case`` -- built once, never modified."""
    target, fixed, w = wdo.band_case(shape)
    return target, fixed, w, wdo.SPACINGS[shape]


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """(direct, error of the float64 oracle CG, error of the float32 one, float64 iterations, true relative residual of the float32 one)"""
    target, fixed, w, _ = _case(shape)
    direct = wdo.direct_solve(target, fixed, w)
    u64, it64, _ = wdo.cg(target, fixed, w, dtype=np.float64)
    u32, _, _ = wdo.cg(target, fixed, w, dtype=np.float32)
    return (direct, float(np.abs(u64 - direct).max()), float(np.abs(u32.astype(np.float64) - direct).max()), it64,
            wdo.true_rel_residual(u32, target, fixed, w))


@functools.lru_cache(maxsize=None)
def _solve(shape):
    from animatablegaussians_amd.weight_volume import diffuse_weights
    target, fixed, w, spacing = _case(shape)
    u, info = diffuse_weights(_t(target), _t(fixed), spacing, tol=wdo.TOL, check_every=1)
    return u, info


@pytest.mark.parametrize("shape", wdo.SHAPES)
def test_operator_against_the_float64_oracle(shape):
    from animatablegaussians_amd.weight_volume import diffusion_operator
    _, fixed, w, spacing = _case(shape)
    probe = wdo.probe_input(shape)
    got = diffusion_operator(_t(probe), _t(fixed), spacing).cpu().numpy()
    o64, o32 = wdo.apply(probe, fixed, w), wdo.apply(probe, fixed, w, np.float32)
    own = float(np.abs(o32.astype(np.float64) - o64).max())
    dev = float(np.abs(got.astype(np.float64) - o64).max())
    bar = 4 * own + 2.0 ** -22 * float(np.abs(probe).max())
    print(f"{shape}: worst |GPU - float64| {dev:.3e}, float32 oracle {own:.3e}, bar {bar:.3e}, equals the float32 oracle bit for bit: "
          f"{np.array_equal(got, o32)}")
    assert got.dtype == np.float32 and got.shape == o64.shape and np.isfinite(got).all() and dev <= bar
    assert (got[fixed] == 0).all()


@pytest.mark.parametrize("shape", wdo.SHAPES)
def test_solve_against_the_direct_solution(shape):
    target, fixed, w, _ = _case(shape)
    direct, e64, e32, it64, t32 = _reference(shape)
    u, info = _solve(shape)
    got = u.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == target.shape and np.isfinite(got).all()
    assert np.array_equal(got[fixed], target[fixed]), "the fixed nodes must carry the target bit for bit"
    err = float(np.abs(got.astype(np.float64) - direct).max())
    true_rel = wdo.true_rel_residual(got, target, fixed, w)
    own = info["true_rel_residual"].numpy()
    print(f"{shape}: iterations {info['iterations']} (float64 oracle {it64}); |u - direct| {err:.3e}, oracle CG float64 {e64:.3e} float32 {e32:.3e}; "
          f"float64 relative residual of u {true_rel.max():.3e} (float32 oracle's {t32.max():.3e}), reported {own.max():.3e}, "
          f"recurrence {float(info['rel_residual'].max()):.3e}")
    assert info["converged"] and float(info["rel_residual"].max()) <= wdo.TOL
    assert err <= 4 * max(e64, e32)
    assert true_rel.max() <= 4 * t32.max()
    assert info["iterations"] <= 1.5 * it64
    assert own.shape == true_rel.shape and (own <= 2 * true_rel).all() and (true_rel <= 2 * own).all()
    if shape[3] >= 3:
        assert (got[..., 0] == 0).all(), "a channel whose fixed values are all zero must stay exactly zero"
        assert true_rel[0] == 0 and own[0] == 0 and float(info["rel_residual"][0]) == 0


def test_two_solves_are_bit_identical():
    import torch
    from animatablegaussians_amd.weight_volume import diffuse_weights
    shape = (12, 12, 12, 55)
    target, fixed, _, spacing = _case(shape)
    u, info = _solve(shape)
    again, info2 = diffuse_weights(_t(target), _t(fixed), spacing, tol=wdo.TOL, check_every=1)
    assert torch.equal(u, again) and info2["iterations"] == info["iterations"]
    assert torch.equal(info2["rel_residual"], info["rel_residual"]) and torch.equal(info2["true_rel_residual"], info["true_rel_residual"])
    # batches of 16 stop at the next multiple of 16 and land on the same solution within the bar of the solve
    batched, info3 = diffuse_weights(_t(target), _t(fixed), spacing, tol=wdo.TOL)
    direct, e64, e32, _, _ = _reference(shape)
    assert info3["converged"] and info3["iterations"] == -(-info["iterations"] // 16) * 16
    assert float(np.abs(batched.cpu().numpy().astype(np.float64) - direct).max()) <= 4 * max(e64, e32)


@functools.lru_cache(maxsize=None)
def _lattice_volume():
    from animatablegaussians_amd.weight_volume import WeightVolume
    v, f = mqo.lattice_mesh()
    vol = WeightVolume.from_body_mesh(_t(v), _t(f), _t(mqo.sparse_weights(v)), res=(12, 14, 10))
    return v, f, vol, vol.diffuse()


def test_weight_volume_diffuse(tmp_path):
    import torch
    from animatablegaussians_amd.weight_volume import WeightVolume
    v, f, vol, out = _lattice_volume()
    assert out is not vol and out.ori_weight_volume is vol.ori_weight_volume and out.smpl_sdf_volume is vol.smpl_sdf_volume
    assert vol.diffused is False and vol.diffusion is None and vol.diff_weight_volume is vol.ori_weight_volume
    assert out.diffused is True and out.diffusion["converged"] and torch.equal(out.volume_bounds, vol.volume_bounds)
    assert torch.equal(out.center, vol.center) and torch.equal(out.smpl_bounds, vol.smpl_bounds)
    got = out.diff_weight_volume.cpu().numpy()
    J = got.shape[3]
    assert got.shape == (12, 14, 10, 55) and got.dtype == np.float32 and got.min() >= 0 and got.max() <= 1
    rows = float(np.abs(got.astype(np.float64).sum(-1) - 1).max())
    # the oracle on the same ori, SDF and band
    ori = vol.ori_weight_volume.cpu().numpy()
    sdf = vol.smpl_sdf_volume.cpu().numpy()[..., 0]
    spacing = [float(h) for h in vol.voxel_size.cpu()]
    band = out.diffusion["band"]
    assert band == 1.5 * max(spacing)
    fixed = np.abs(sdf) <= np.float32(band)
    assert int(fixed.sum()) == out.diffusion["fixed_nodes"] and 0 < fixed.sum() < fixed.size
    w = wdo.weights(spacing)
    direct = wdo.direct_solve(ori, fixed, w)
    e64 = float(np.abs(wdo.cg(ori, fixed, w, dtype=np.float64)[0] - direct).max())
    e32 = float(np.abs(wdo.cg(ori, fixed, w, dtype=np.float32)[0].astype(np.float64) - direct).max())
    err = float(np.abs(got.astype(np.float64) - wdo.clip_renormalise(direct)).max())
    moved = float(np.abs(got - ori).max())
    print(f"diffuse (12, 14, 10) x {J}: {int(fixed.sum())} of {fixed.size} nodes fixed, band {band:.4f} m, iterations {out.diffusion['iterations']}; "
          f"|row sum - 1| {rows:.3e} (bar {wdo.row_sum_bar(J):.3e}); |diff - oracle| {err:.3e}, oracle CG float64 {e64:.3e} float32 {e32:.3e}; "
          f"largest |diff - ori| {moved:.3f}")
    assert rows <= wdo.row_sum_bar(J)
    assert err <= 4 * max(e64, e32)
    assert moved > 0.05, "diffusion must change the weights away from the surface"
    # save -> load, bit for bit, with a diff volume of its own
    p = str(tmp_path / "cano_weight_volume.npz")
    out.save(p)
    with np.load(p) as d:
        assert sorted(d.files) == ["center", "diff_weight_volume", "ori_weight_volume", "sdf_volume", "smpl_bounds", "volume_bounds"]
        assert np.array_equal(d["diff_weight_volume"], got) and np.array_equal(d["ori_weight_volume"], ori)
        assert not np.array_equal(d["diff_weight_volume"], d["ori_weight_volume"]) and d["sdf_volume"].shape == (12, 14, 10)
    back = WeightVolume.load(p)
    for a, b in ((back.diff_weight_volume, out.diff_weight_volume), (back.ori_weight_volume, out.ori_weight_volume),
                 (back.smpl_sdf_volume, out.smpl_sdf_volume), (back.volume_bounds, out.volume_bounds), (back.center, out.center),
                 (back.smpl_bounds, out.smpl_bounds)):
        assert torch.equal(a, b)
    assert back.diffused is True


def test_avatar_from_a_diffused_volume():
    import torch
    from animatablegaussians_amd.avatar import AvatarNet
    v, f, vol, out = _lattice_volume()
    net = AvatarNet.from_template({'with_viewdirs': True}, _t(v), _t(f), out)
    assert net.lbs.shape[1] == 55 and net.lbs.shape[0] == net.init_points.shape[0] > 1000
    assert torch.equal(net.lbs, out.forward_weight(net.init_points))
    assert not torch.equal(net.lbs, vol.forward_weight(net.init_points))


def test_argument_errors():
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.weight_volume import WeightVolume, diffuse_weights, diffusion_operator
    shape = (5, 4, 3, 65)
    target, fixed, _, spacing = _case(shape)
    t, m = _t(target), _t(fixed)
    with pytest.raises(ValueError, match="GPU"):
        diffuse_weights(t.cpu(), m, spacing)
    with pytest.raises(ValueError, match="GPU"):
        diffuse_weights(t, m.cpu(), spacing)
    for bad in (m[:, :, :2], m[..., None], m.to(torch.uint8)):
        with pytest.raises(ValueError, match="fixed must be"):
            diffuse_weights(t, bad.contiguous(), spacing)
        with pytest.raises(ValueError, match="fixed must be"):
            diffusion_operator(t, bad.contiguous(), spacing)
    with pytest.raises(ValueError, match="no fixed node"):
        diffuse_weights(t, torch.zeros_like(m), spacing)
    u, info = diffuse_weights(t, torch.ones_like(m), spacing)
    assert u is t and info["iterations"] == 0 and info["converged"] and float(info["true_rel_residual"].max()) == 0
    u, info = diffuse_weights(t, m, spacing, max_iter=1)
    assert info["iterations"] == 1 and info["converged"] is False and float(info["rel_residual"].max()) > wdo.TOL
    assert torch.equal(u[m], t[m]) and torch.isfinite(u).all()
    v, f, vol, _ = _lattice_volume()
    with pytest.raises(RuntimeError, match="did not reach"):
        vol.diffuse(max_iter=1)
    no_sdf = WeightVolume(vol.ori_weight_volume, vol.ori_weight_volume, vol.volume_bounds, vol.center, vol.smpl_bounds)
    with pytest.raises(ValueError, match="sdf_volume"):
        no_sdf.diffuse()
    # the C ABI's own refusals, by return code (the Python surface never lets these through)
    L = _lib.lib()
    z = torch.zeros(4096).cuda()
    w = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    n_ws = L.ag_weight_diffuse_workspace_bytes(4, 4, 4, 2)
    ws = torch.zeros(n_ws, dtype=torch.uint8).cuda()
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = L.ag_weight_diffuse_apply(P(z), P(z), 1, 4, 4, 2, w, P(z), None)
    assert rc != 0 and b"at least 2" in L.ag_last_error()
    rc = L.ag_weight_diffuse_apply(None, P(z), 4, 4, 4, 2, w, P(z), None)
    assert rc != 0 and b"null pointer" in L.ag_last_error()
    rc = L.ag_weight_diffuse_apply(P(z), P(z), 4, 4, 4, 2, None, P(z), None)
    assert rc != 0 and b"null pointer" in L.ag_last_error()
    rc = L.ag_weight_diffuse_apply(P(z), P(z), 4, 4, 4, 0, w, P(z), None)
    assert rc != 0 and b"channel count" in L.ag_last_error()
    rc = L.ag_weight_diffuse_init(P(z), P(z), 4, 1, 4, 2, w, P(z), P(z), P(z), P(z), P(ws), n_ws, P(z), P(z), None)
    assert rc != 0 and b"at least 2" in L.ag_last_error()
    rc = L.ag_weight_diffuse_init(P(z), P(z), 4, 4, 4, 2, w, P(z), None, P(z), P(z), P(ws), n_ws, P(z), P(z), None)
    assert rc != 0 and b"null pointer" in L.ag_last_error()
    rc = L.ag_weight_diffuse_init(P(z), P(z), 4, 4, 4, 2, w, P(z), P(z), P(z), P(z), P(ws), n_ws - 1, P(z), P(z), None)
    assert rc != 0 and b"workspace" in L.ag_last_error()
    rc = L.ag_weight_diffuse_iterate(P(z), 4, 4, 1, 2, w, 1, P(z), P(z), P(z), P(z), P(ws), n_ws, P(z), None)
    assert rc != 0 and b"at least 2" in L.ag_last_error()
    rc = L.ag_weight_diffuse_iterate(P(z), 4, 4, 4, 2, w, 1, P(z), P(z), P(z), P(z), None, n_ws, P(z), None)
    assert rc != 0 and b"null pointer" in L.ag_last_error()
    rc = L.ag_weight_diffuse_iterate(P(z), 4, 4, 4, 2, w, -1, P(z), P(z), P(z), P(z), P(ws), n_ws, P(z), None)
    assert rc != 0 and b"iterations" in L.ag_last_error()
    bad_w = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    rc = L.ag_weight_diffuse_apply(P(z), P(z), 4, 4, 4, 2, bad_w, P(z), None)
    assert rc != 0 and b"weight" in L.ag_last_error()
    torch.cuda.synchronize()


def test_elements_past_two_to_the_31_are_addressed():
    """One operator application on a [2, 2, Z, 55] volume of just over 2^31 elements (8.6 GB in, 8.6 GB out): an element index kept in
    32 bits wraps inside the last z-row, a byte offset kept in 32 bits from the first eighth on.  The last 64 z-slices of all four rows
    are compared with the oracle run on the last 65 slices (its first slice supplies the lower neighbour and is not compared)."""
    import torch
    from animatablegaussians_amd.weight_volume import diffusion_operator
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip(f"needs 24 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    J = 55
    Z = 2 ** 31 // (4 * J) + 1                                                      # 9 761 290: the first Z with 4 Z J > 2^31
    assert 4 * Z * J > 2 ** 31 > 4 * (Z - 1) * J
    spacing = (0.03, 0.02, 0.01)
    w = wdo.weights(spacing)
    probe = torch.empty(2, 2, Z, J, device="cuda")
    tail = wdo.probe_input((2, 2, 65, J), seed=11)
    probe[:, :, :Z - 65] = 0.25
    probe[:, :, Z - 65:] = _t(tail)
    fixed = torch.zeros(2, 2, Z, dtype=torch.bool, device="cuda")
    tail_fixed = np.zeros((2, 2, 65), bool)
    tail_fixed[:, :, 3::7] = True
    tail_fixed[1, 1, -1] = True
    fixed[:, :, Z - 65:] = _t(tail_fixed)
    out = diffusion_operator(probe, fixed, spacing)
    got = out[:, :, Z - 64:].cpu().numpy()
    body = out[:, :, 1000:2000].abs().max().item(), out[1, 0, Z // 2:Z // 2 + 1000].abs().max().item()
    del out, probe
    o64, o32 = wdo.apply(tail, tail_fixed, w)[:, :, 1:], wdo.apply(tail, tail_fixed, w, np.float32)[:, :, 1:]
    own = float(np.abs(o32.astype(np.float64) - o64).max())
    dev = float(np.abs(got.astype(np.float64) - o64).max())
    bar = 4 * own + 2.0 ** -22 * float(np.abs(tail).max())
    print(f"[2, 2, {Z}, {J}]: worst |GPU - float64| on the last 64 slices {dev:.3e}, float32 oracle {own:.3e}, bar {bar:.3e}")
    assert dev <= bar and (got[tail_fixed[:, :, 1:]] == 0).all()
    assert body == (0.0, 0.0), "a constant interior must give exact zeros"
