"""The closest-point-on-a-mesh kernels on the GPU (``include/ag_mesh_query.h``) against the float64 run of ``mesh_query_oracle.py``, and
what is built on them: the signed distance, ``WeightVolume.from_body_mesh`` / ``save``, ``canonical_maps(lbs_rule='nearest')`` and the
reference-named wrappers.

Every tolerance is 4 x the worst deviation of the oracle's float32 run from its float64 run ON THE SAME INPUTS, never anything the
kernel returned: ``tol_d`` for distances (|q - c|, sqrt(dist2) and their difference), ``eps_b`` for the barycentrics' sign and sum,
``tol_on`` for the distance of the reconstructed point from the returned face, and -- on non-fragile queries -- the tolerances of the
interpolated weights and of the closest point.  The factor 4 allows for a float32 evaluation that meets the faces in another order
than the oracle's scan; a wrong-region answer is off by a face's size (centimetres), four orders above.  Face ids are never compared
with the oracle's for equality: where two faces are equally near to within rounding either is a true minimiser.  A query is FRAGILE
when a face that shares no vertex with the oracle's face lies within ``tol_d`` of the minimum (the medial surface); at most 2 % may be,
and ``test_mesh_query_cpu.py`` shows the oracle alone stays below that on these inputs.

T = ``mesh_query.FACE_TILE`` = 256 is the LDS tile of the tiled walk; both walks run on every shape and must agree bit for bit.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_query_oracle as mqo  # noqa: E402

pytestmark = pytest.mark.gpu
T = 256


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(points, v, f, walk="default"):
    from animatablegaussians_amd import mesh_query
    d2, fid, bary, feat = mesh_query.closest_point(_t(points), _t(v), _t(f), walk=walk, return_feature=True)
    assert d2.dtype == bary.dtype == __import__("torch").float32 and fid.dtype == feat.dtype == __import__("torch").int32
    assert tuple(d2.shape) == tuple(fid.shape) == tuple(feat.shape) == (len(points),) and tuple(bary.shape) == (len(points), 3)
    return {"dist2": d2.cpu().numpy(), "face": fid.cpu().numpy().astype(np.int64), "bary": bary.cpu().numpy(), "feature": feat.cpu().numpy()}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("dist2", "face", "bary", "feature"))


def _validity(tag, res, o64, o32, dev, p, v, f):
    got = mqo.measure(res, o64, p, v, f)
    print(f"{tag}: float32 oracle d {dev['d']:.3e} b {dev['b']:.3e} on {dev['on']:.3e} | GPU d {got['d']:.3e} b {got['b']:.3e} on {got['on']:.3e}"
          f" | bars 4 x | equals the float32 oracle bit for bit: {_same(res, o32)}")
    assert np.isfinite(res["bary"]).all() and ((res["face"] >= 0) == (o64["face"] >= 0)).all()
    assert (res["face"] < len(f)).all() and (res["feature"] >= 0).all() and (res["feature"] <= 6).all()
    assert got["d"] <= 4 * dev["d"] and got["b"] <= 4 * dev["b"] and got["on"] <= 4 * dev["on"]


@functools.lru_cache(maxsize=None)
def _lattice():
    v, f = mqo.lattice_mesh()
    p = mqo.mixed_queries(v, f, np.random.default_rng(7), 2048)
    return (v, f, p) + mqo.deviations(p, v, f)


@functools.lru_cache(maxsize=None)
def _shape_queries():
    v, f = mqo.lattice_mesh()
    return v, f, mqo.mixed_queries(v, f, np.random.default_rng(13), 257)


@pytest.mark.parametrize("F", [1, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_shapes_about_the_tile_and_the_wave(F, N):
    from animatablegaussians_amd import mesh_query
    assert mesh_query.FACE_TILE == T
    v, faces, pts = _shape_queries()
    f, p = faces[:F], (pts[:N] if N > 1 else pts[200:201])
    o64, o32, dev = mqo.deviations(p, v, f, cull=False)
    res = _gpu(p, v, f)
    _validity(f"F={F} N={N}", res, o64, o32, dev, p, v, f)
    assert _same(res, _gpu(p, v, f, "uniform")) and _same(res, _gpu(p, v, f, "tiled"))


def test_lattice_validity_weights_and_closest_point():
    from animatablegaussians_amd import mesh_query
    v, f, p, o64, o32, dev = _lattice()
    res = _gpu(p, v, f)
    _validity("lattice N=2048", res, o64, o32, dev, p, v, f)
    assert _same(res, _gpu(p, v, f, "tiled")) and _same(res, _gpu(p, v, f, "uniform")) and _same(res, _gpu(p, v, f))
    tol_d = 4 * dev["d"]
    fragile = o64["d_other"] - np.sqrt(o64["dist2"]) <= tol_d
    assert fragile.mean() <= 0.02
    w = mqo.sparse_weights(v)
    w64, c64 = mqo.interpolate(o64, f, w), mqo.closest_points_of(o64, v, f)
    dev_w = float(np.abs(mqo.interpolate(o32, f, w, np.float32).astype(np.float64) - w64)[~fragile].max())
    dev_c = float(np.abs(mqo.closest_points_of(o32, v, f) - c64)[~fragile].max())
    got_w = mesh_query.interpolate_lbs(_t(p), _t(v), _t(f), _t(w))
    sdf, fid, got_c = mesh_query.signed_distance(_t(p), _t(v), _t(f))
    assert tuple(got_w.shape) == (len(p), 55) and tuple(got_c.shape) == (len(p), 3) and np.array_equal(fid.cpu().numpy(), res["face"])
    as_np = mesh_query.interpolate_lbs(p, v, f, w)                                 # the reference's calling convention: arrays in, array out
    assert isinstance(as_np, np.ndarray) and np.array_equal(as_np, got_w.cpu().numpy())
    ew = float(np.abs(got_w.cpu().numpy().astype(np.float64) - w64)[~fragile].max())
    ec = float(np.abs(got_c.cpu().numpy().astype(np.float64) - c64)[~fragile].max())
    print(f"non-fragile ({int(fragile.sum())} fragile): weights GPU {ew:.3e} float32 oracle {dev_w:.3e}; closest point GPU {ec:.3e} float32 oracle {dev_c:.3e}")
    assert ew <= 4 * dev_w and ec <= 4 * dev_c
    assert np.abs(np.abs(sdf.cpu().numpy().astype(np.float64)) - np.sqrt(o64["dist2"])).max() <= tol_d
    # sign: the queries of the random third are off the surface
    s64 = mqo.sign(p, o64, v, f) * np.sqrt(o64["dist2"])
    decided = np.abs(s64) > tol_d
    third = np.arange(len(p)) < len(p) // 3
    assert decided[third].mean() >= 0.99 and (s64[third] < 0).sum() > 20 and (s64[third] > 0).sum() > 20
    assert (np.sign(sdf.cpu().numpy()) == np.sign(s64))[decided].all()


@functools.lru_cache(maxsize=None)
def _small_grid():
    from animatablegaussians_amd.weight_volume import body_bounds, grid_axes
    v, f = mqo.lattice_mesh(12, 11)
    axes = grid_axes(body_bounds(v.min(0), v.max(0))[0], (24, 24, 24))
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return (v, f, axes, g) + mqo.deviations(g, v, f, cull=False)


def test_sign_on_a_grid_against_the_oracle():
    """The grid mode (three axes, no point array) on a 24^3 grid about a closed 264-face lattice: distance and sign."""
    from animatablegaussians_amd import mesh_query
    v, f, axes, g, o64, o32, dev = _small_grid()
    sdf, fid, bary = mesh_query.grid_signed_distance([_t(a) for a in axes], _t(v), _t(f))
    by_points = mesh_query.signed_distance(_t(g), _t(v), _t(f))
    assert np.array_equal(sdf.cpu().numpy(), by_points[0].cpu().numpy()) and np.array_equal(fid.cpu().numpy(), by_points[1].cpu().numpy())
    tol_d = 4 * dev["d"]
    s64 = mqo.sign(g, o64, v, f) * np.sqrt(o64["dist2"])
    decided = np.abs(s64) > tol_d
    area, _ = mqo.mesh_area_volume(v, f)
    expected = area * 2 * tol_d / float(np.prod(g.max(0).astype(np.float64) - g.min(0)))
    print(f"24^3 grid: tol_d {tol_d:.3e}, undecided {int((~decided).sum())} (expected share {expected:.1e}), inside {int((s64 < 0).sum())}")
    assert (~decided).mean() <= 0.01 and (s64 < 0).sum() > 100
    got = sdf.cpu().numpy().astype(np.float64)
    assert (np.sign(got) == np.sign(s64))[decided].all()
    assert np.abs(np.abs(got) - np.sqrt(o64["dist2"])).max() <= tol_d
    wn = mqo.winding_number(g[::7], v, f)
    assert ((got[::7] < 0) == (wn > 0.5))[decided[::7]].all()                     # and against the independent inside / outside test


def test_duplicate_and_zero_area_faces_and_the_tie_rule():
    import torch
    from animatablegaussians_amd import mesh_query
    v, f = mqo.special_mesh()
    p = mqo.mixed_queries(v, f[:160], np.random.default_rng(5), 300)
    tri7 = v[f[7]].astype(np.float64)
    p = np.concatenate([p, tri7.mean(0, keepdims=True).astype(np.float32), tri7.astype(np.float32)], 0)       # on face 7 = face 160
    o64, o32, dev = mqo.deviations(p, v, f, cull=False)
    res = _gpu(p, v, f)
    _validity("special mesh", res, o64, o32, dev, p, v, f)
    assert not (res["face"] == 160).any() and not (res["face"] == 163).any() and (res["face"][300:] <= 7).all()
    assert (res["bary"] >= 0).all()
    d2a, fa, ba = mesh_query.closest_point(_t(p), _t(v), _t(f))
    d2b, fb, bb = mesh_query.closest_point(_t(p), _t(v), _t(f))
    assert torch.equal(d2a, d2b) and torch.equal(fa, fb) and torch.equal(ba, bb)
    assert _same(res, _gpu(p, v, f, "tiled")) and _same(res, _gpu(p, v, f, "uniform"))
    # duplicate first, original second: still the lower INDEX
    g = np.concatenate([f[7:8], f], 0)
    assert not (_gpu(p, v, g)["face"] == 8).any()
    # the zero-area faces alone, and no usable face at all
    alone = _gpu(p, v, f[161:163])
    assert np.isfinite(alone["dist2"]).all() and (alone["bary"] >= 0).all() and np.abs(alone["bary"].astype(np.float64).sum(1) - 1).max() <= 2.0 ** -22
    for faces in (f[163:], f[:0]):
        none = _gpu(p, v, faces)
        assert (none["face"] == -1).all() and np.isinf(none["dist2"]).all() and (none["bary"] == 0).all() and (none["feature"] == 0).all()
        sdf, fid, c = mesh_query.signed_distance(_t(p), _t(v), _t(faces))
        assert torch.isinf(sdf).all() and (sdf > 0).all() and (c == 0).all()


def test_translated_mesh():
    v, f = mqo.lattice_mesh()
    vt = (v + np.float32([3, -2, 5])).astype(np.float32)
    p = mqo.mixed_queries(vt, f, np.random.default_rng(17), 513)
    o64, o32, dev = mqo.deviations(p, vt, f)
    _validity("translated by (+3, -2, +5) m", _gpu(p, vt, f), o64, o32, dev, p, vt, f)


def test_from_body_mesh_on_a_non_cubic_grid(tmp_path):
    import torch
    from animatablegaussians_amd.avatar import AvatarNet
    from animatablegaussians_amd.weight_volume import WeightVolume, body_bounds, grid_axes
    v, f = mqo.lattice_mesh()
    w = mqo.sparse_weights(v)
    res = (5, 6, 7)
    vol = WeightVolume.from_body_mesh(_t(v), _t(f), _t(w), res=res)
    assert (vol.res_x, vol.res_y, vol.res_z, vol.joint_num) == res + (55,) and vol.diffused is False
    assert vol.diff_weight_volume is vol.ori_weight_volume and tuple(vol.smpl_sdf_volume.shape) == res + (1,)
    bounds, center, smpl = body_bounds(v.min(0), v.max(0))
    assert np.array_equal(vol.volume_bounds.cpu().numpy(), bounds) and np.array_equal(vol.center.cpu().numpy(), center)
    assert np.array_equal(vol.smpl_bounds.cpu().numpy(), smpl)
    g = np.stack(np.meshgrid(*grid_axes(bounds, res), indexing="ij"), -1).reshape(-1, 3)            # node (i, j, k) = (x_i, y_j, z_k)
    o64, o32, dev = mqo.deviations(g, v, f)
    tol_d = 4 * dev["d"]
    fragile = o64["d_other"] - np.sqrt(o64["dist2"]) <= tol_d
    assert fragile.mean() <= 0.02
    w64 = mqo.interpolate(o64, f, w)
    dev_w = float(np.abs(mqo.interpolate(o32, f, w, np.float32).astype(np.float64) - w64)[~fragile].max())
    s64 = -mqo.sign(g, o64, v, f) * np.sqrt(o64["dist2"])                                           # positive inside
    ori = vol.ori_weight_volume.cpu().numpy().reshape(-1, 55).astype(np.float64)
    sdf = vol.smpl_sdf_volume.cpu().numpy().reshape(-1).astype(np.float64)
    ew = float(np.abs(ori - w64)[~fragile].max())
    print(f"from_body_mesh {res}: weights GPU {ew:.3e} float32 oracle {dev_w:.3e}; tol_d {tol_d:.3e}; inside nodes {int((s64 > 0).sum())}")
    assert ew <= 4 * dev_w and np.abs(np.abs(sdf) - np.abs(s64)).max() <= tol_d
    decided = np.abs(s64) > tol_d
    assert (~decided).mean() <= 0.01 and (np.sign(sdf) == np.sign(s64))[decided].all() and (s64 > 0).any()
    # sampling at the nodes returns the nodes: trilinear weights 1 and 0 up to the rounding of the node's own cell coordinate
    nodes = _t(g.astype(np.float32))
    # a node's cell coordinate carries four roundings of values <= 1 times R - 1 <= 6 (< 2^-19) on each of three axes, times a value <= max
    span = float(vol.ori_weight_volume.abs().max()) * 2.0 ** -17
    assert float((vol.forward_weight(nodes, volume_type="ori") - vol.ori_weight_volume.view(-1, 55)).abs().max()) <= span
    assert torch.equal(vol.forward_weight(nodes), vol.forward_weight(nodes, volume_type="ori"))
    assert float((vol.forward_sdf(nodes) - vol.smpl_sdf_volume.view(-1, 1)).abs().max()) <= float(vol.smpl_sdf_volume.abs().max()) * 2.0 ** -17
    # save / load round trip
    path = str(tmp_path / "cano_weight_volume.npz")
    vol.save(path)
    back = WeightVolume.load(path)
    for a, b in ((back.diff_weight_volume, vol.diff_weight_volume), (back.ori_weight_volume, vol.ori_weight_volume),
                 (back.smpl_sdf_volume, vol.smpl_sdf_volume), (back.volume_bounds, vol.volume_bounds), (back.center, vol.center),
                 (back.smpl_bounds, vol.smpl_bounds)):
        assert torch.equal(a, b)
    assert back.diffused is True                                                   # a file says nothing else
    # res as an int; and the avatar constructor takes the object as it is
    cube = WeightVolume.from_body_mesh(_t(v), _t(f), _t(w), res=4)
    assert tuple(cube.ori_weight_volume.shape) == (4, 4, 4, 55)
    net = AvatarNet.from_template({'with_viewdirs': True}, _t(v), _t(f), vol)
    assert net.lbs.shape[1] == 55 and net.lbs.shape[0] == net.init_points.shape[0] > 1000
    assert torch.equal(net.lbs, vol.forward_weight(net.init_points))


def test_canonical_maps_nearest_rule_against_the_rendered_rule():
    """Only the nearest-face search is new code: the rendered points lie on their faces, so both rules interpolate the same weights.
    The float64 oracle decides tolerance and fragility on every 11th point (the search over 21 096 faces costs it 1 ms per point)."""
    import torch
    from animatablegaussians_amd import subject_maps as sm, synth
    m = synth.body_mesh()
    v, f, w = _t(m["vertices"]), _t(m["faces"]), _t(m["lbs_weights"])
    n = sm.vertex_normals(v, f)
    rendered = sm.canonical_maps(v, f, n, w, size=256)
    nearest = sm.canonical_maps(v, f, n, w, size=256, lbs_rule="nearest")
    for k in ("cano_smpl_pos_map", "cano_smpl_nml_map", "mask", "face_id", "bary", "log_scale"):
        assert torch.equal(rendered[k], nearest[k]), k
    assert torch.equal(sm.canonical_maps(v, f, n, w, size=256, lbs_rule="rendered")["init_pts_lbs"], rendered["init_pts_lbs"])
    with pytest.raises(ValueError, match="lbs_rule"):
        sm.canonical_maps(v, f, n, w, size=256, lbs_rule="closest")
    pts = rendered["cano_smpl_pos_map"][rendered["mask"]].cpu().numpy()
    a, b = rendered["init_pts_lbs"].cpu().numpy().astype(np.float64), nearest["init_pts_lbs"].cpu().numpy().astype(np.float64)
    assert a.shape == b.shape and a.shape[0] == len(pts) > 20000
    idx = np.arange(0, len(pts), 11)[:2048]
    o64, o32, dev = mqo.deviations(pts[idx], m["vertices"], m["faces"])
    fragile = o64["d_other"] - np.sqrt(o64["dist2"]) <= 4 * dev["d"]
    w64 = mqo.interpolate(o64, m["faces"], m["lbs_weights"])
    dev_w = float(np.abs(mqo.interpolate(o32, m["faces"], m["lbs_weights"], np.float32).astype(np.float64) - w64)[~fragile].max())
    worst = float(np.abs(b[idx] - w64)[~fragile].max())
    both = float(np.abs(b[idx] - a[idx])[~fragile].max())
    print(f"{len(idx)} of {len(pts)} points, {int(fragile.sum())} fragile: nearest vs float64 oracle {worst:.3e}, nearest vs rendered {both:.3e}, "
          f"float32 oracle {dev_w:.3e}; all points: nearest vs rendered {float(np.abs(a - b).max()):.3e}")
    assert fragile.mean() <= 0.02 and worst <= 4 * dev_w and both <= 4 * dev_w
    assert np.isfinite(b).all() and np.abs(b.sum(1) - 1).max() < 1e-5


def test_reference_named_wrappers():
    import torch
    from animatablegaussians_amd import mesh_query
    v, f, p, o64, o32, dev = _lattice()
    vt = (v + np.float32([0.1, 0.0, -0.2])).astype(np.float32)
    P = torch.stack([_t(p[:300]), _t(p[300:600])])
    Vb = torch.stack([_t(v), _t(vt)])
    dists, indices, bc = mesh_query.nearest_face_pytorch3d(P, Vb, _t(f).long())
    assert tuple(dists.shape) == tuple(indices.shape) == (2, 300) and tuple(bc.shape) == (2, 300, 3)
    assert dists.dtype == bc.dtype == torch.float32 and indices.dtype == torch.int64
    for b, (pp, vv) in enumerate(((p[:300], v), (p[300:600], vt))):
        d2, fid, bary = mesh_query.closest_point(_t(pp), _t(vv), _t(f))
        assert torch.equal(dists[b], torch.sqrt(d2)) and torch.equal(indices[b], fid.long()) and torch.equal(bc[b], bary)
    w = _t(mqo.sparse_weights(v))
    Fb = torch.stack([_t(f), _t(f)]).long()
    pts_w, near = mesh_query.calc_blending_weight(P, Vb, Fb, torch.stack([w, w]), near_thres=0.08)
    assert tuple(pts_w.shape) == (2, 300, 55) and near.dtype == torch.bool and tuple(near.shape) == (2, 300)
    assert torch.equal(near, dists < 0.08) and near.any() and not near.all()
    assert torch.equal(pts_w[1], mesh_query.interpolate_lbs(P[1], Vb[1], _t(f), w))
    with pytest.raises(ValueError, match="GPU"):
        mesh_query.closest_point(torch.from_numpy(p), _t(v), _t(f))
    with pytest.raises(ValueError, match="walk"):
        mesh_query.closest_point(_t(p), _t(v), _t(f), walk="sorted")
    d2, fid, bary = mesh_query.closest_point(_t(p[:0]), _t(v), _t(f))
    assert d2.numel() == 0 and tuple(bary.shape) == (0, 3)
