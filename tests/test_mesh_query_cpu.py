"""The closest-point-on-a-mesh path, the part that needs no GPU: the numpy oracle (``mesh_query_oracle.py``) against closed forms on one
triangle, against random samples of every face and against the generalized winding number; the bounds and axes of
``WeightVolume.from_body_mesh`` against a literal transcription of ``gen_data/gen_weight_volume.py:136-153``; the file ``save`` writes;
the ABI surface; and the exclusion caps of ``test_mesh_query_gpu.py`` on the oracle alone."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_query_oracle as mqo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.sh recompiles a unit when ANY header under csrc/ or include/ is newer than its object
STALE_HEADERS = 'find "$HERE" "$HERE/../../include" -maxdepth 1 -name \'*.h\' -newer "$obj"'


def test_entry_points_declared_bound_and_exported():
    import inspect
    from animatablegaussians_amd import _lib, mesh_query, subject_maps, weight_volume
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_mesh_query.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_want in (("ag_mesh_closest_point_workspace_bytes", 1), ("ag_mesh_closest_point", 2), ("ag_mesh_pseudonormal_sign", 6)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_mesh_query.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(table[name][2]) == n_args == n_want, name
        assert hasattr(L, name), f"{name} is not exported"
    fields = re.search(r"typedef struct AgMeshQueryArgs \{(.*?)\} AgMeshQueryArgs;", hdr, flags=re.S).group(1)
    declared = [re.sub(r".*?(\w+)$", r"\1", part.strip()) for line in fields.split(";") for part in line.split(",") if part.strip()]
    assert declared == [n for n, _ in _lib.AgMeshQueryArgs._fields_]
    assert L.ag_abi_version() == 1
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_mesh_query\.hip" \$EXACT', build) and STALE_HEADERS in build
    assert int(re.search(r"#define AG_MESH_QUERY_FACE_TILE (\d+)", hdr).group(1)) == mesh_query.FACE_TILE
    for fn in ("closest_point", "signed_distance", "nearest_face_pytorch3d", "interpolate_lbs", "calc_blending_weight", "pseudonormals"):
        assert callable(getattr(mesh_query, fn))
    p = inspect.signature(mesh_query.calc_blending_weight).parameters
    assert list(p) == ["query_pts", "smpl_v", "smpl_f", "smpl_lbs", "near_thres", "method"]
    assert p["near_thres"].default == 0.08 and p["method"].default == "barycentric"
    with pytest.raises(NotImplementedError):
        mesh_query.calc_blending_weight(None, None, None, method="NN")
    p = inspect.signature(subject_maps.canonical_maps).parameters
    assert p["lbs_rule"].kind is inspect.Parameter.KEYWORD_ONLY and p["lbs_rule"].default == "rendered"
    p = inspect.signature(weight_volume.WeightVolume.from_body_mesh).parameters
    assert list(p) == ["vertices", "faces", "lbs_weights", "res"] and p["res"].default == 128
    p = inspect.signature(weight_volume.WeightVolume.save).parameters
    assert list(p) == ["self", "path", "alias_diff"] and p["alias_diff"].default is True
    assert weight_volume.WeightVolume.diffused is True


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_triangle_in_every_voronoi_region_and_on_the_boundaries(dtype):
    v, f = mqo.one_triangle()
    pts, feats, close = mqo.voronoi_queries()
    o = mqo.closest_point(pts, v, f, dtype)
    tol = 8 * np.finfo(dtype).eps * 3.0                                           # coordinates up to 2.5, a handful of roundings
    want_d = np.linalg.norm(pts - close, axis=1)
    assert (o["face"] == 0).all()
    assert np.abs(np.sqrt(o["dist2"].astype(np.float64)) - want_d).max() <= tol
    want_b = np.stack([1 - close[:, 0] / 2 - close[:, 1], close[:, 0] / 2, close[:, 1]], 1)
    assert np.abs(o["bary"].astype(np.float64) - want_b).max() <= tol
    assert (o["bary"] >= 0).all() and np.abs(o["bary"].astype(np.float64).sum(1) - 1).max() <= tol
    seen = set()
    for got, want, p in zip(o["feature"], feats, pts):
        if want is not None:
            assert got == want, (p, got, want)
            seen.add(int(got))
    assert seen == set(range(7))
    both = {(1.0, 0.0): {0, 1}, (0.0, 0.0): {0, 1, 3, 4}, (2.0, -0.5): {1, 5}, (-0.5, 0.0): {3, 4}, (-0.5, 1.0): {3, 6}, (0.0, -0.5): {1, 4}}
    for got, want, p in zip(o["feature"], feats, pts):
        if want is None and (p[0], p[1]) in both:
            assert int(got) in both[(p[0], p[1])], (p, got)


def test_zero_area_duplicate_and_skipped_faces():
    v, f = mqo.special_mesh()
    rng = np.random.default_rng(5)
    p = mqo.mixed_queries(v, f[:160], rng, 300)
    for dtype in (np.float64, np.float32):
        o = mqo.closest_point(p, v, f, dtype)
        assert np.isfinite(o["dist2"]).all() and np.isfinite(o["bary"]).all() and (o["bary"] >= 0).all()
        assert np.abs(o["bary"].astype(np.float64).sum(1) - 1).max() <= 4 * np.finfo(dtype).eps
        assert not (o["face"] == 160).any() and not (o["face"] == 163).any()     # the duplicate loses every tie, the skipped face never wins
        assert (o["face"] == 7).any()
        alone = mqo.closest_point(p, v, f[161:163], dtype)                        # the two zero-area faces alone
        assert np.isfinite(alone["dist2"]).all() and (alone["bary"] >= 0).all()
        assert (mqo.closest_point(p, v, f[161:162], dtype)["feature"] > 0).all()  # two equal corners: det = 0 exactly, the edges answer
        seg = np.sqrt(mqo.closest_point(p, v, np.array([[f[20, 0], f[20, 1], f[20, 0]]]), np.float64)["dist2"])
        d161 = np.sqrt(mqo.closest_point(p, v, f[161:162], dtype)["dist2"].astype(np.float64))
        assert np.abs(d161 - seg).max() <= 1e-6
        none = mqo.closest_point(p, v, f[163:], dtype)
        assert (none["face"] == -1).all() and np.isinf(none["dist2"]).all() and (none["bary"] == 0).all()
    assert (mqo.closest_point(p, v, f[:0])["face"] == -1).all()


@functools.lru_cache(maxsize=None)
def _lattice():
    v, f = mqo.lattice_mesh()
    p = mqo.mixed_queries(v, f, np.random.default_rng(7), 2048)
    return (v, f, p) + mqo.deviations(p, v, f)


def test_no_sample_of_any_face_is_closer_than_the_returned_distance():
    v, f, p, o64, o32, dev = _lattice()
    rng = np.random.default_rng(11)
    q = p[::16].astype(np.float64)                                                # 128 queries of all three kinds
    b = rng.dirichlet(np.ones(3) * 0.5, (len(f), 12))                             # 12 samples per face, corners and edges favoured
    s = (b[..., None] * v.astype(np.float64)[f][:, None]).sum(2)                  # [F, 12, 3]
    d = np.sqrt(o64["dist2"][::16])
    closest = np.sqrt(((q[:, None, None] - s[None]) ** 2).sum(-1)).min((1, 2))
    assert (closest >= d - 1e-12).all()
    c = mqo.closest_points_of(o64, v, f)[::16]
    assert np.abs(np.linalg.norm(q - c, axis=1) - d).max() <= 1e-12               # and the distance is attained on the returned face
    assert mqo.distance_to_face(c, o64["face"][::16], v, f).max() <= 1e-12


def test_the_culled_oracle_equals_the_full_scan():
    v, f, p, o64, o32, dev = _lattice()
    for dtype, culled in ((np.float64, o64), (np.float32, o32)):
        full = mqo.closest_point(p[:700], v, f, dtype)
        for k in ("dist2", "face", "bary", "feature"):
            assert np.array_equal(full[k], culled[k][:700]), k
    v, f = mqo.special_mesh()
    p = mqo.mixed_queries(v, f[:160], np.random.default_rng(5), 300)
    a, b = mqo.closest_point(p, v, f, np.float32), mqo.closest_point(p, v, f, np.float32, cull=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_fragile_share_of_the_gpu_test_inputs_stays_below_its_cap():
    """The caps test_mesh_query_gpu.py allows itself, shown on the oracle alone: at most 2 % of the queries fragile."""
    v, f, p, o64, o32, dev = _lattice()
    tol_d = 4 * dev["d"]
    fragile = o64["d_other"] - np.sqrt(o64["dist2"]) <= tol_d
    print(f"lattice: float32 oracle deviations {dev}, tol_d {tol_d:.3e}, fragile {int(fragile.sum())} of {len(p)}, "
          f"faces differing between the float32 and the float64 run {int((o64['face'] != o32['face']).sum())}")
    assert 0 < dev["d"] < 1e-5 and fragile.mean() <= 0.02
    w = mqo.sparse_weights(v)
    dw = np.abs(mqo.interpolate(o32, f, w, np.float32).astype(np.float64) - mqo.interpolate(o64, f, w))[~fragile].max()
    dc = np.abs(mqo.closest_points_of(o32, v, f) - mqo.closest_points_of(o64, v, f))[~fragile].max()
    print(f"float32 oracle, non-fragile queries: weights {dw:.3e}, closest point {dc:.3e}")
    assert dw < 1e-3 and dc < 1e-4                                                # three orders below a wrong-region answer (~ a face, 5 cm)


@functools.lru_cache(maxsize=None)
def _body_grid():
    m, g, total = mqo.body_grid_nodes()
    v, f = m["vertices"], m["faces"]
    o64, o32, dev = mqo.deviations(g, v, f)
    return v, f, g, total, o64, o32, dev


def test_pseudonormal_sign_equals_the_winding_number_classification():
    v, f, g, total, o64, o32, dev = _body_grid()
    tol_d = 4 * dev["d"]
    sdf = mqo.sign(g, o64, v, f) * np.sqrt(o64["dist2"])
    wn = mqo.winding_number(g, v, f)
    assert np.abs(wn - np.round(wn)).max() < 1e-9 and set(np.round(wn).astype(int)) == {0, 1}          # a closed, outward-wound mesh
    decided = np.abs(sdf) > tol_d
    area, volume = mqo.mesh_area_volume(v, f)
    cube = float(np.prod(g.max(0).astype(np.float64) - g.min(0)))
    expected = area * 2 * tol_d / cube
    print(f"{len(g)} of {total} nodes visited, {int((wn > 0.5).sum())} inside; tol_d {tol_d:.3e}; undecided {int((~decided).sum())}, "
          f"expected share area * 2 tol_d / volume of the cube = {expected:.2e}")
    assert ((sdf < 0) == (wn > 0.5))[decided].all() and (wn > 0.5).sum() > 100
    # every undecided node is among the visited ones (they are near the surface), so the share is of ALL nodes; a Poisson count with
    # mean total * expected (about 0.1) exceeds 1 + 10 x its mean with probability < 1e-3
    assert (~decided).sum() <= 1 + 10 * expected * total and (~decided).sum() <= 0.01 * total
    # the float32 run's sign, from its own closest points, agrees wherever the distance decides
    s32 = mqo.sign(g, o32, v, f, dtype=np.float32)
    assert (s32 == np.sign(sdf))[decided].all()


def test_bounds_and_axes_follow_the_reference_lines():
    """A literal transcription of gen_weight_volume.py:88-90,136-153 against ``weight_volume.body_bounds`` / ``grid_axes``."""
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.weight_volume import body_bounds, grid_axes
    vertices = synth.body_mesh()["vertices"].astype(np.float64)                   # a trimesh's vertices are float64
    res = (5, 6, 7)
    min_xyz = vertices.min(0).astype(np.float32)
    max_xyz = vertices.max(0).astype(np.float32)
    max_len = 1.1 * (max_xyz - min_xyz).max()
    center = 0.5 * (min_xyz + max_xyz)
    volume_bounds = np.stack(
        [center - 0.5 * max_len, center + 0.5 * max_len], 0
    )
    min_xyz[:2] -= 0.05
    max_xyz[:2] += 0.05
    min_xyz[2] -= 0.15
    max_xyz[2] += 0.15
    smpl_bounds = np.stack(
        [min_xyz, max_xyz], 0
    )
    x = np.linspace(volume_bounds[0, 0], volume_bounds[1, 0], res[0])
    y = np.linspace(volume_bounds[0, 1], volume_bounds[1, 1], res[1])
    z = np.linspace(volume_bounds[0, 2], volume_bounds[1, 2], res[2])
    pts = np.stack(np.meshgrid(x, y, z, indexing = 'ij'), axis = -1)
    got_bounds, got_center, got_smpl = body_bounds(vertices.min(0), vertices.max(0))
    assert got_bounds.dtype == got_center.dtype == got_smpl.dtype == np.float32
    assert np.array_equal(got_bounds, volume_bounds.astype(np.float32)) and np.array_equal(got_center, center.astype(np.float32))
    assert np.array_equal(got_smpl, smpl_bounds.astype(np.float32))
    axes = grid_axes(got_bounds, res)
    assert [a.dtype for a in axes] == [np.float32] * 3 and [len(a) for a in axes] == list(res)
    nodes = np.stack(np.meshgrid(*axes, indexing="ij"), -1)
    assert nodes.shape == pts.shape == (5, 6, 7, 3) and np.array_equal(nodes, pts.astype(np.float32))
    assert np.array_equal(nodes[2, 3, 4], np.float32([x[2], y[3], z[4]]))        # node (i, j, k) = (x_i, y_j, z_k)


def test_save_writes_the_reference_file(tmp_path):
    import torch
    from animatablegaussians_amd.weight_volume import WeightVolume
    rng = np.random.default_rng(3)
    ori = torch.from_numpy(rng.random((5, 6, 7, 4)).astype(np.float32))
    vol = WeightVolume.__new__(WeightVolume)                                      # the constructor refuses a host device; save reads attributes only
    vol.ori_weight_volume = vol.diff_weight_volume = ori
    vol.smpl_sdf_volume = torch.from_numpy(rng.standard_normal((5, 6, 7, 1)).astype(np.float32))
    vol.volume_bounds = torch.tensor([[-1., -1, -1], [1, 1, 1]])
    vol.smpl_bounds = torch.tensor([[-.5, -.9, -.2], [.5, .9, .2]])
    vol.center = torch.zeros(3)
    vol.diffused = False
    p = str(tmp_path / "cano_weight_volume.npz")
    vol.save(p)
    with np.load(p) as d:
        assert sorted(d.files) == ["center", "diff_weight_volume", "ori_weight_volume", "sdf_volume", "smpl_bounds", "volume_bounds"]
        assert all(d[k].dtype == np.float32 for k in d.files)
        assert d["diff_weight_volume"].shape == d["ori_weight_volume"].shape == (5, 6, 7, 4) and d["sdf_volume"].shape == (5, 6, 7)
        assert d["volume_bounds"].shape == d["smpl_bounds"].shape == (2, 3) and d["center"].shape == (3,)
        assert np.array_equal(d["diff_weight_volume"], d["ori_weight_volume"]) and np.array_equal(d["ori_weight_volume"], ori.numpy())
        assert np.array_equal(d["sdf_volume"], vol.smpl_sdf_volume.numpy()[..., 0])
    vol.save(p, alias_diff=False)
    with np.load(p) as d:
        assert "diff_weight_volume" not in d.files and "ori_weight_volume" in d.files
    vol.diffused = True                                                           # a diffused volume always writes its own
    vol.diff_weight_volume = ori * 0.5
    vol.save(p, alias_diff=False)
    with np.load(p) as d:
        assert np.array_equal(d["diff_weight_volume"], ori.numpy() * 0.5)
