"""The hand fusion's kernels (``include/ag_hand_fusion.h``, ``hand_fusion.py``) and ``render(..., hands=)`` against
``hand_fusion_oracle.py``.

* The bar, per output and case, is the project's: |gpu - float64 oracle| <= 4 x max|float32 oracle - float64 oracle| + 2^-22 x max|float64
  oracle|, maxima over the case's compared points; ``density`` has its own bar, because it amplifies an SDF error by up to 1 / b^2.  The
  device's ``sinf`` / ``cosf`` / ``expf``, the MFMA's k order and the fold of the pose columns are different from, and as valid as, torch's.
* A point is left out of a comparison only where the float32 and the float64 oracle take different discrete decisions (the sign of
  ``n . (p - q)`` of a hand with weight, the centre-y test and, end to end, the closest face), at most 1 % of a case; every test prints
  the count, and ``test_hand_fusion_cpu.py`` asserts the cap on the oracle alone for every point set used here.
* The kernel alone is fed the float32 oracle's ``(dist2, face_id, bary)``, which the float64 oracle is fed too: its error is then its
  own and not the closest point's tie-breaking.  ``fuse_hands`` end to end searches the closest point on the device.
* Bit-for-bit statements: inactive points carry the body's values; ``compact=True`` equals ``compact=False``; two calls agree; ``render``
  with hands is the chain of the public calls and does not depend on ``chunk_size``; ``render`` without hands is what it was.
Every test prints the measured deviation and its bar.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hand_fusion_oracle as hfo  # noqa: E402
import template_field_oracle as tfo  # noqa: E402
import template_render_oracle as tro  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("sdf", "density", "color")
RENDER_MAPS = ("rgb_map", "acc_map", "depth_map", "weights")


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _fields(sc):
    from animatablegaussians_amd.hand_fusion import HandField
    sd = hfo.state_dict(sc["nets"]["left"], sc["nets"]["right"])
    return HandField.from_state_dict(sd, "left", sc["multires"]), HandField.from_state_dict(sd, "right", sc["multires"])


def _hands(sc):
    return {side: {k: _t(v) for k, v in sc["hands"][side].items()} for side in hfo.SIDES}


def _body(sc):
    body = {"sdf": _t(sc["sdf_b"]), "density": _t(sc["density_b_in"]), "cano_xyz": _t(sc["cano_xyz"])}
    if sc["color_b"] is not None:
        body["color"] = _t(sc["color_b"])
    return body


def _kernel(sc, cp):
    """The fused kernel alone on the oracle's closest points, in place on copies of the body's values."""
    from animatablegaussians_amd import hand_fusion as hf
    left, right = _fields(sc)
    body = _body(sc)
    queries = tuple((_t(cp[s]["dist2"].astype(np.float32)), _t(cp[s]["face"].astype(np.int32)), _t(cp[s]["bary"].astype(np.float32))) for s in hfo.SIDES)
    prepared = hf.PreparedHands(_hands(sc), body["sdf"].device)
    hf.fuse_kernel(_t(sc["p"]), body["cano_xyz"], body["sdf"].view(-1), body["density"].view(-1), body.get("color"), prepared, queries, left, right,
                   float(sc["centre"][1]), hfo.density_b(), sc["hand_pose"])
    return {k: body[k] for k in OUTPUTS if k in body}


def _fuse(sc, **kw):
    from animatablegaussians_amd import hand_fusion as hf
    left, right = _fields(sc)
    return hf.fuse_hands(_body(sc), _t(sc["p"]), _hands(sc), left, right, cano_smpl_center=sc["centre"], density_b=hfo.density_b(),
                         hand_pose=sc["hand_pose"], **kw)


def _compare(name, got, o32, o64, keep):
    n = len(keep)
    out = int((~keep).sum())
    print(f"{name}: {out} of {n} points left out")
    assert out <= hfo.EXCLUSION_CAP * n
    limits = hfo.bars(o32, o64, keep)
    for k in OUTPUTS:
        if o64.get(k) is None:
            assert k not in got
            continue
        g = got[k].detach().cpu().numpy().astype(np.float64).reshape(o64[k].shape)
        dev = float(np.abs(g - o64[k])[keep].max())
        own = float(np.abs(o32[k].astype(np.float64) - o64[k])[keep].max())
        print(f"{name} {k}: |gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {limits[k]:.3e}")
        assert np.isfinite(g).all() and dev <= limits[k], f"{name} {k}: {dev:.3e} > {limits[k]:.3e}"


def _body_bits_where(got, sc, where):
    """The outputs at the points ``where`` are the body's values bit for bit."""
    for k, src in (("sdf", "sdf_b"), ("density", "density_b_in"), ("color", "color_b")):
        if k in got:
            assert np.array_equal(_bits(got[k])[where], _bits(sc[src])[where]), f"{k}: an inactive point does not carry the body's value"


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hfo.SIZES)
def test_kernel_on_the_oracles_closest_points(n):
    """Tile tails (1, 31, 32, 33 points), several tiles (257) and several workgroups (1031); for n >= 6 the first six points are a vertex
    of each hand (dist = 0) and, by each hand, y exactly at the centre (kept) and one ulp below it (zeroed)."""
    sc, cp, o32, o64, keep = hfo.case("mixed", n)
    got = _kernel(sc, cp)
    _compare(f"kernel, mixed, n = {n}", got, o32, o64, keep)
    _body_bits_where(got, sc, o32["inactive"])
    if n >= 6:
        assert cp["left"]["dist2"][0] == 0 and cp["right"]["dist2"][1] == 0, "the points on the surface are gone"
        sdf = got["sdf"].cpu().numpy().reshape(-1)
        assert o32["inactive"][[3, 5]].all() and not np.array_equal(_bits(sdf[[2, 4]]), _bits(sc["sdf_b"].reshape(-1)[[2, 4]]))


@pytest.mark.parametrize("kind", ["inactive", "active", "left", "clasped"])
def test_kernel_point_sets(kind):
    """Every point inactive (the body's values, bit for bit), every point active, only the left hand active, and hands close enough for
    ``wl + wr > 1`` (the ``s`` normalisation)."""
    sc, cp, o32, o64, keep = hfo.case(kind, 1031)
    got = _kernel(sc, cp)
    _compare(f"kernel, {kind}", got, o32, o64, keep)
    _body_bits_where(got, sc, o32["inactive"])
    if kind == "inactive":
        assert o32["inactive"].all()
    else:
        assert not np.array_equal(_bits(got["sdf"]), _bits(sc["sdf_b"]))


def test_kernel_with_a_hand_pose():
    sc, cp, o32, o64, keep = hfo.case("mixed", 257, pose=True)
    got = _kernel(sc, cp)
    _compare("kernel, non-zero hand_pose", got, o32, o64, keep)
    rest, cp0, *_ = hfo.case("mixed", 257)
    zero = _kernel(rest, cp0)
    assert np.array_equal(_bits(got["sdf"]), _bits(zero["sdf"])) and np.array_equal(_bits(got["density"]), _bits(zero["density"]))
    moved = float((got["color"] - zero["color"]).abs().max())
    print(f"the pose moves the colour by up to {moved:.3e}")
    assert moved > 1e-3


def test_kernel_without_colour():
    sc, cp, o32, o64, keep = hfo.case("mixed", 257, color=False)
    got = _kernel(sc, cp)
    assert set(got) == {"sdf", "density"}
    _compare("kernel, no colour", got, o32, o64, keep)
    full, cpf, *_ = hfo.case("mixed", 257)
    with_colour = _kernel(full, cpf)
    assert np.array_equal(_bits(got["sdf"]), _bits(with_colour["sdf"])) and np.array_equal(_bits(got["density"]), _bits(with_colour["density"]))


def test_kernel_on_the_mano_topology():
    """778 vertices and 1552 faces, the reference's closed MANO topology, on synthetic vertices: the real counts run once."""
    sc, cp, o32, o64, keep = hfo.case("mixed", 257, mano=True)
    assert sc["hands"]["left"]["f"].shape == (1552, 3) and sc["hands"]["right"]["v"].shape == (778, 3)
    _compare("kernel, MANO topology", _kernel(sc, cp), o32, o64, keep)


def test_a_hand_without_a_closest_face_has_weight_zero():
    """The right hand's only face is skipped by the closest-point query: ``face_id = -1``, ``dist2 = inf`` at every point."""
    sc, cp, o32, o64, keep = hfo.case("mixed", 257, empty_right=True)
    assert (cp["right"]["face"] == -1).all() and np.isinf(cp["right"]["dist2"]).all()
    got = _kernel(sc, cp)
    _compare("kernel, right hand missing", got, o32, o64, keep)
    _body_bits_where(got, sc, o32["inactive"])
    assert o32["inactive"].sum() > (hfo.case("mixed", 257)[2]["inactive"]).sum()
    # end to end: the device's own query returns -1 for every point
    sc, _, o32, o64, keep = hfo.case("faces", 257, empty_right=True, own_closest=True)
    end_to_end = _fuse(sc)
    _compare("fuse_hands, right hand missing", end_to_end, o32, o64, keep)
    assert _same(end_to_end, _fuse(sc, compact=False))


# ---- fuse_hands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [1, 2])
def test_fuse_hands_end_to_end(subdiv):
    """Gate, compaction, the two closest-point queries on the device, the fused kernel, the scatter.  The points lie over the interior of
    a hand's face (80 and 320 faces) or between the hands, so that the float32 and the float64 search name the same face."""
    sc, _, o32, o64, keep = hfo.case("faces", 1031, own_closest=True, subdiv=subdiv)
    body = _body(sc)
    before = {k: v.clone() for k, v in body.items()}
    from animatablegaussians_amd import hand_fusion as hf
    left, right = _fields(sc)
    kw = dict(cano_smpl_center=sc["centre"], density_b=hfo.density_b())
    got = hf.fuse_hands(body, _t(sc["p"]), _hands(sc), left, right, **kw)
    assert set(got) == {"sdf", "density", "color", "cano_xyz"} and got["sdf"].shape == (1031, 1) and got["color"].shape == (1031, 3)
    assert _same(body, before), "fuse_hands changed body_ret"
    assert np.array_equal(_bits(got["cano_xyz"]), _bits(sc["cano_xyz"]))
    _compare(f"fuse_hands, {20 * 4 ** subdiv} faces", got, o32, o64, keep)
    _body_bits_where(got, sc, o32["inactive"])
    share = 1.0 - float(o32["inactive"].mean())
    print(f"active share {share:.3f}")
    assert 0.3 < share < 0.8
    # every point through the queries and the kernel: the same bits; and a second call: the same bits
    assert _same(got, hf.fuse_hands(body, _t(sc["p"]), _hands(sc), left, right, compact=False, **kw)), "compact=False differs from compact=True"
    assert _same(got, hf.fuse_hands(body, _t(sc["p"]), _hands(sc), left, right, **kw)), "two calls differ"
    # [1, N, 3] points and a centre on the device are accepted
    assert _same(got, hf.fuse_hands(body, _t(sc["p"])[None], _hands(sc), left, right, cano_smpl_center=_t(sc["centre"]), density_b=hfo.density_b()))


def test_fuse_hands_when_every_point_is_inactive_or_active():
    for kind in ("inactive", "active"):
        sc = hfo.case(kind, 1031)[0]
        got, everything = _fuse(sc), _fuse(sc, compact=False)
        assert _same(got, everything), f"{kind}: compact=False differs from compact=True"
        if kind == "inactive":
            _body_bits_where(got, sc, np.ones(1031, bool))
    empty = dict(sc, p=sc["p"][:0], cano_xyz=sc["cano_xyz"][:0], sdf_b=sc["sdf_b"][:0], density_b_in=sc["density_b_in"][:0], color_b=sc["color_b"][:0])
    none = _fuse(empty)
    assert none["sdf"].shape == (0, 1) and none["color"].shape == (0, 3)


def test_hand_meshes_on_the_device():
    """``hand_meshes`` picks the hands out of the body's vertices, reverses the left hand's faces and gives both hands outward unit
    normals (``subject_maps.vertex_normals``) that agree with the float64 angle-weighted normals of ``mesh_query_oracle``."""
    import mesh_query_oracle as mqo
    import torch
    from animatablegaussians_amd.hand_fusion import hand_meshes
    u, f = hfo.icosphere(2)
    V = len(u)
    rs = np.random.RandomState(9)
    li, ri = rs.permutation(400)[:V] + 100, rs.permutation(400)[:V] + 600
    body = rs.normal(size=(1100, 3))
    right = u * hfo.RADII + np.array([-0.75, 0.3, 0.0])
    body[ri], body[li] = right, right * np.array([-1.0, 1.0, 1.0])                 # the left hand is the right hand's mirror image
    body = body.astype(np.float32)
    m = hand_meshes(_t(body), li, ri, f)
    for side, ids, faces, centre in (("left", li, f[:, ::-1], (0.75, 0.3, 0.0)), ("right", ri, f, (-0.75, 0.3, 0.0))):
        v, n, ff = (m[side][k].cpu().numpy() for k in ("v", "n", "f"))
        assert ff.dtype == np.int32 and np.array_equal(ff, faces) and np.array_equal(_bits(v), _bits(body[ids]))
        want = mqo.pseudonormals(body[ids], faces)[2]
        dev = float(np.abs(n - want).max())
        print(f"{side}: |normals - float64 angle-weighted normals| {dev:.2e}")
        assert dev <= 2e-5 and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-6
        assert ((n * (v - np.float32(centre))).sum(1) > 0).all(), f"the {side} hand's normals point inward: the winding is wrong"
    with pytest.raises(ValueError, match="index vertex"):
        hand_meshes(_t(body[:500]), li, ri, f)
    assert m["left"]["n"].dtype == torch.float32


# ---- render ---------------------------------------------------------------------------------------------------------------------------------
def _sphere_field():
    from animatablegaussians_amd.template_field import TemplateField
    net = tfo.make_net(tfo.NARROW, 4, trained=False)                                 # geometric initialisation: an approximate sphere
    arch = net["arch"]
    return TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=False, multires_viewdir=arch["multires_viewdir"],
                                         geo_activation=net["geo_activation"])


def _render_hands(live):
    """Hands 0.45 either side of x = 0: samples with |x| < 0.06 are inactive, the rest see one hand."""
    sc = hfo.scene("mixed", 8)
    h = hfo.synthetic_hands(1, 0.45, live=live)
    left, right = _fields(sc)
    hands = {side: {k: _t(v) for k, v in h[side].items()} for side in hfo.SIDES}
    hands.update(left_field=left, right_field=right, cano_smpl_center=np.float32([0.0, -0.45, 0.0]))
    return hands


def _camera_33():
    o, d = tro.pinhole_rays(6, half_width=0.5)
    return _t(o[:33]), _t(d[:33]), _t(np.full(33, 1.3, np.float32)), _t(np.full(33, 3.7, np.float32))


def test_render_without_hands_is_the_chain_it_was():
    """No ``hands`` argument at all: sample, field, composite.  Nothing of the fusion runs."""
    from animatablegaussians_amd import template_render as tr
    field = _sphere_field()
    o, d, near, far = _camera_33()
    got = tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS)
    pts, z = tr.sample_pts_on_rays(o, d, near, far, 64)
    ret = field(pts.view(-1, 3), want=("sdf", "density", "color"))
    assert _same(got, tr.composite(ret["density"], ret["color"], z, want=RENDER_MAPS)), "render differs from the chain of its public calls"
    for chunk in (1, 7, 33):
        assert _same(got, tr.render(field, o, d, near, far, sampling="uniform", chunk_size=chunk, want=RENDER_MAPS))


def test_render_with_hands_is_the_chain_of_the_public_calls():
    """33 rays, 64 samples, canonical space: ``render(hands=)`` = sample -> field -> ``fuse_hands`` -> composite, bit for bit and for
    every ``chunk_size``; ``hands=None`` is the render without the argument."""
    from animatablegaussians_amd import hand_fusion as hf
    from animatablegaussians_amd import template_render as tr
    field = _sphere_field()
    o, d, near, far = _camera_33()
    hands = _render_hands(live=False)
    got = tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS, hands=hands)
    assert got["rgb_map"].shape == (33, 3) and got["weights"].shape == (33, 64)
    pts, z = tr.sample_pts_on_rays(o, d, near, far, 64)
    ret = field(pts.view(-1, 3), want=("sdf", "density", "color"))
    fused = hf.fuse_hands(ret, pts.view(-1, 3), {s: hands[s] for s in hfo.SIDES}, hands["left_field"], hands["right_field"],
                          cano_smpl_center=hands["cano_smpl_center"], density_b=field.density_b)
    by_hand = tr.composite(fused["density"], fused["color"], z, want=RENDER_MAPS)
    assert _same(got, by_hand), "render(hands=) differs from sample -> field -> fuse_hands -> composite"
    for chunk in (1, 7, 33):
        assert _same(got, tr.render(field, o, d, near, far, sampling="uniform", chunk_size=chunk, want=RENDER_MAPS, hands=hands)), f"chunk_size = {chunk}"
    assert _same(got, tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS, hands=dict(hands, compact=False)))
    plain = tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS)
    assert _same(plain, tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS, hands=None))
    assert not _same(plain, got), "the hands change nothing"
    box = [hands[s]["cano_v"][:, 0].min().item() for s in hfo.SIDES], [hands[s]["cano_v"][:, 0].max().item() for s in hfo.SIDES]
    share = float(hf.active_mask(pts.view(-1, 3), (box[0][0], box[1][0]), (box[0][1], box[1][1]), -0.45).float().mean())
    moved = int((fused["density"] != ret["density"]).sum())
    print(f"active share of the samples {share:.3f}; densities changed: {moved} of {ret['density'].numel()}")
    assert 0.05 < share < 0.95 and moved > 0
    # acc only: no colour is fused
    acc = tr.render(field, o, d, near, far, sampling="uniform", want=("acc_map",), hands=hands)
    assert np.array_equal(_bits(acc["acc_map"]), _bits(got["acc_map"]))
    with pytest.raises(ValueError, match="hands must be"):
        tr.render(field, o, d, near, far, sampling="uniform", hands={"left": hands["left"]})


def test_render_posed_space_with_hands_is_the_chain_by_hand():
    """``space='live'``: the hands' ``v`` / ``n`` and the closest-point queries are in the space of the samples, the gates in canonical
    space."""
    import inverse_skinning_oracle as iso
    import mesh_query_oracle as mqo
    from animatablegaussians_amd import hand_fusion as hf
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd import template_render as tr
    from animatablegaussians_amd.weight_volume import WeightVolume
    field = _sphere_field()
    case = iso.smooth_case((16, 16, 16, 55), n=1, B=1, offset=0.05)
    vol = WeightVolume(_t(case["volume"]), _t(case["volume"]), case["bounds"], np.zeros(3, np.float32), case["bounds"])
    v, f = mqo.lattice_mesh(8, 10)
    live = dict(cano2live_jnt_mats=_t(case["jnt_mats"]), volume=vol, live_mesh_v=_t(v[None]), live_mesh_f=_t(f[None]),
                live_mesh_lbs=_t(mqo.sparse_weights(v, 55)[None]), near_thres=0.05, use_root_finding=True, with_hand=False)
    o, d = tro.pinhole_rays(6, eye=(0.1, -0.2, -2.5), target=(0.0, -0.2, 0.0), half_width=0.3)
    o, d = _t(o[:33]), _t(d[:33])
    near, far = _t(np.full(33, 1.8, np.float32)), _t(np.full(33, 3.2, np.float32))
    h = hfo.synthetic_hands(1, 0.2, live=True)
    left, right = _fields(hfo.scene("mixed", 8))
    hands = {side: {k: _t(a) for k, a in h[side].items()} for side in hfo.SIDES}
    hands.update(left_field=left, right_field=right, cano_smpl_center=np.float32([0.0, -0.6, 0.0]))
    got = tr.render(field, o, d, near, far, space="live", sampling="uniform", live=live, chunk_size=12, want=RENDER_MAPS, hands=hands)
    pts, z = tr.sample_pts_on_rays(o, d, near, far, 64)
    cano, _ = inv.transform_live2cano(pts.view(1, -1, 3), **live)
    ret = field(cano[0], want=("sdf", "density", "color"))
    fused = hf.fuse_hands(ret, pts.view(-1, 3), {s: hands[s] for s in hfo.SIDES}, left, right, cano_smpl_center=hands["cano_smpl_center"],
                          density_b=field.density_b)
    assert _same(got, tr.composite(fused["density"], fused["color"], z, want=RENDER_MAPS)), "render(space='live', hands=) differs from the chain by hand"
    wrong = hf.fuse_hands(ret, cano[0], {s: hands[s] for s in hfo.SIDES}, left, right, cano_smpl_center=hands["cano_smpl_center"], density_b=field.density_b)
    assert not np.array_equal(_bits(wrong["sdf"]), _bits(fused["sdf"])), "the posed samples do not reach the closest-point queries"
    assert not np.array_equal(_bits(fused["sdf"]), _bits(ret["sdf"]))
