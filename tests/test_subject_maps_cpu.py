"""Canonical maps from a mesh, the part that needs no GPU: the ABI surface, the float64 oracle against itself, the cap on the
share of pixels the GPU comparison may set aside, and the rendered-face shortcut of the skinning-weight interpolation."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_maps_oracle as smo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGILE_CAP = 0.005


def test_entry_points_declared_bound_and_exported():
    import ctypes
    from animatablegaussians_amd import _lib, subject_maps
    from animatablegaussians_amd.avatar import AvatarNet
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_subject_maps.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ag_mesh_rasterize_ortho_workspace_bytes", "ag_mesh_rasterize_ortho", "ag_mesh_resolve_attribute_workspace_bytes",
                 "ag_mesh_resolve_attribute", "ag_knn_mean_dist2_workspace_bytes", "ag_knn_mean_dist2"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_subject_maps.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in table and len(table[name][2]) == n_args, f"{name}: header declares {n_args} arguments"
        assert hasattr(L, name), f"{name} is not exported"
    # the by-value matrix and the struct the binding mirrors
    fields = re.search(r"typedef struct AgMeshRasterArgs \{(.*?)\} AgMeshRasterArgs;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*;", fields)
    assert names == [f[0] for f in _lib.AgMeshRasterArgs._fields_]
    assert ctypes.sizeof(_lib.AgMeshRasterArgs) == 10 * 4 + 12 * 4 + 5 * 8 + 8
    for fn in ("rasterize_ortho", "resolve", "vertex_normals", "knn_log_scale", "canonical_maps", "write_subject_dir"):
        assert callable(getattr(subject_maps, fn))
    assert callable(AvatarNet.from_mesh) and callable(AvatarNet.from_smplx)
    p = inspect.signature(AvatarNet.__init__).parameters["log_scale"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "NOT pinned" in subject_maps.vertex_normals.__doc__


def test_host_tensors_raise():
    import torch
    from animatablegaussians_amd import subject_maps as sm
    v, f = smo.lattice_mesh()
    with pytest.raises(ValueError, match="GPU"):
        sm.rasterize_ortho(torch.from_numpy(v), torch.from_numpy(f), smo.lattice_view(32), 32)
    with pytest.raises(ValueError, match="GPU"):
        sm.knn_log_scale(torch.zeros(10, 3))


def test_body_mesh_is_a_closed_consistently_wound_surface():
    from animatablegaussians_amd import synth
    m = synth.body_mesh(second_component=False)
    v, f = m["vertices"].astype(np.float64), m["faces"].astype(np.int64)
    assert v.shape == (10442, 3) and f.shape == (20880, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    directed = set(map(tuple, e))
    assert len(directed) == len(e) and all((b, a) in directed for a, b in directed)       # every edge once in each direction
    vol = (np.cross(v[f[:, 0]], v[f[:, 1]]) * v[f[:, 2]]).sum() / 6.0
    assert vol > 0.1                                                                          # counter-clockwise from outside
    assert (np.abs(v[:, :2] - 0.5 * (v.min(0) + v.max(0))[:2]) < 1.0).all()                  # inside the 2 m window
    full = synth.body_mesh()
    assert full["vertices"].shape[0] == 10442 + 110 and full["faces"].shape[0] == 20880 + 216
    w = full["lbs_weights"]
    assert w.shape[1] == 55 and ((w > 0).sum(1) <= 4).all() and np.abs(w.astype(np.float64).sum(1) - 1).max() < 4 * 2.0 ** -24
    # smooth: the weights are cubic B-splines of s = (y - ymin) / (ymax - ymin) * (J - 3), whose slope is at most 2/3 per unit of s
    ff, y = full["faces"].astype(np.int64), full["vertices"][:, 1].astype(np.float64)
    ds = np.abs(y[ff[:, 0]] - y[ff[:, 1]]) / (y.max() - y.min()) * 52
    assert (np.abs(w[ff[:, 0]] - w[ff[:, 1]]).max(1) <= 2.0 / 3.0 * ds + 1e-6).all()


def test_lattice_on_pixel_centres_is_covered_exactly_once_and_float32_agrees():
    S = 32
    v, f = smo.lattice_mesh(S)
    view = smo.lattice_view(S)
    wx, wy, _ = smo.window_vertices(v, view, S, S)
    assert np.array_equal(wx - 0.5, np.round(wx - 0.5)) and np.array_equal(wy - 0.5, np.round(wy - 0.5))    # ON pixel centres
    count = np.zeros((S, S), np.int64)
    for k in range(len(f)):
        count += smo.rasterize(v, f[k:k + 1], view, S, S, cull=False, flip_rows=False, fragile=False)["face_id"] >= 0
    gx0, gx1, gy0, gy1 = int(wx.min() - 0.5), int(wx.max() - 0.5), int(wy.min() - 0.5), int(wy.max() - 0.5)
    interior = np.zeros((S, S), bool)
    interior[gy0 + 1:gy1, gx0 + 1:gx1] = True               # centres strictly inside the outline: on shared edges / vertices or inside faces
    assert (count[interior] == 1).all(), "a pixel centre on a shared edge or vertex must belong to exactly one face"
    assert (count[~interior] <= 1).all() and count[:gy0].sum() == 0 and count[:, :gx0].sum() == 0
    # the ORIENTATION of the rule, on the outline (rows of `count` are window rows, y up): the left column and the top row own their
    # centres, the bottom row and the right column do not; of the four corners only the top-left one is owned
    assert (count[gy0 + 1:gy1 + 1, gx0] == 1).all() and (count[gy1, gx0:gx1] == 1).all()
    assert (count[gy0, gx0:gx1 + 1] == 0).all() and (count[gy0:gy1 + 1, gx1] == 0).all()
    a = smo.rasterize(v, f, view, S, S, dtype=np.float64)
    b = smo.rasterize(v, f, view, S, S, dtype=np.float32)
    assert np.array_equal(a["face_id"], b["face_id"])
    assert np.array_equal((a["face_id"] >= 0)[::-1], count == 1)
    assert np.abs(a["bary"] - b["bary"]).max() <= 4 * 2.0 ** -24


def _meshes():
    from animatablegaussians_amd import synth
    body = synth.body_mesh()
    soup = synth.smplx_model_arrays()
    return {"body": (body["vertices"], body["faces"]), "soup": (soup["v_template"].astype(np.float32), soup["f"].astype(np.int32))}


@pytest.mark.parametrize("name,S", [("body", 1024), ("body", 256), ("soup", 256)])
def test_fragile_share_is_capped(name, S):
    """A condition, not a measurement: the GPU comparison excludes exactly the flagged pixels, so their share must stay small."""
    v, f = _meshes()[name]
    r = smo.canonical_raster(v, f, S)
    covered = int((r["face_id"] >= 0).sum())
    flagged = int(r["fragile"].sum())
    print(f"{name} S={S}: covered {covered}, fragile {flagged} ({100.0 * flagged / covered:.3f} %)")
    assert covered > 0.05 * S * S
    assert flagged <= FRAGILE_CAP * covered


def test_rendered_face_interpolates_the_skinning_weights_like_the_nearest_face():
    """The shortcut of the attribute resolve: on non-fragile pixels of the two-component mesh the brute-force nearest face of the
    rendered point gives the rendered face's interpolated weights.  Tolerance: the rendered point carries ~4 roundings of 2^-53 relative
    to max|v|; recovering barycentrics from it divides by the face's height h, and the weights are <= 1: 64 * 2^-53 * max|v| / min h
    (64 for the handful of operations on either side)."""
    from animatablegaussians_amd import synth
    m = synth.body_mesh()
    v, f, w = m["vertices"], m["faces"], m["lbs_weights"].astype(np.float64)
    S = 96
    r = smo.canonical_raster(v, f, S)
    keep = (r["face_id"] >= 0) & ~r["fragile"]
    assert keep.sum() > 1000 and (r["face_id"][keep] >= 20880).any(), "the second component must be visible"
    pos = smo.resolve(r["face_id"], r["bary"], f, v)[keep]
    want = smo.resolve(r["face_id"], r["bary"], f, w)[keep]
    ids, bar = smo.nearest_face_barycentric(pos, v, f)
    tri = f.astype(np.int64)[ids]
    got = bar[:, 0:1] * w[tri[:, 0]] + bar[:, 1:2] * w[tri[:, 1]] + bar[:, 2:3] * w[tri[:, 2]]
    v64, t = v.astype(np.float64), f.astype(np.int64)
    e = [np.linalg.norm(v64[t[:, i]] - v64[t[:, (i + 1) % 3]], axis=1) for i in range(3)]
    height = np.linalg.norm(np.cross(v64[t[:, 1]] - v64[t[:, 0]], v64[t[:, 2]] - v64[t[:, 0]]), axis=1) / np.maximum.reduce(e)
    tol = 64 * 2.0 ** -53 * np.abs(v64).max() / height.min()
    err = np.abs(got - want).max()
    print(f"nearest-face vs rendered-face weights: max |diff| {err:.3e}, tolerance {tol:.3e}, same face on {(ids == r['face_id'][keep]).mean():.4f}")
    assert err <= tol
