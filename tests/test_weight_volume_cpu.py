"""The blend-weight volume path, the part that needs no GPU: the float64 oracle against outputs of the reference's own
``CanoBlendWeightVolume`` (``golden/weight_volume_ref.npz``, written by ``golden/make_golden_weight_volume.py``), the mesh PLY reader on
files assembled here from the format's definition, the ABI surface, and the refusal of a host device."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_volume_oracle as wvo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.sh recompiles a unit when ANY header under csrc/ or include/ is newer than its object
STALE_HEADERS = 'find "$HERE" "$HERE/../../include" -maxdepth 1 -name \'*.h\' -newer "$obj"'
GOLDEN, FIXTURE_CASES, fixture_case = wvo.GOLDEN, wvo.FIXTURE_CASES, wvo.fixture_case

@pytest.mark.parametrize("out,vol,pts,scaled", FIXTURE_CASES)
def test_float64_oracle_agrees_with_the_reference_fixture(out, vol, pts, scaled):
    d = np.load(GOLDEN)
    v, p, b = fixture_case(d, vol, pts, scaled)
    o64, o32 = wvo.sample(v, p, b, np.float64), wvo.sample(v, p, b, np.float32)
    assert o32.dtype == np.float32 and o64.shape == (len(p), v.shape[3]) == d[out + "_f32"].shape
    own = float(np.abs(o32.astype(np.float64) - o64).max())
    dev32 = float(np.abs(d[out + "_f32"].astype(np.float64) - o64).max())
    dev64 = float(np.abs(d[out + "_f64"] - o64).max())
    print(f"{out}: |reference fp32 - oracle| {dev32:.3e}, |reference fp64 - oracle| {dev64:.3e}, |float32 oracle - oracle| {own:.3e}")
    assert own > 0 and dev32 <= 4 * own
    assert dev64 <= 64 * 2.0 ** -53                      # the same formula in the same precision: a few roundings of values <= 1


def test_fixture_covers_the_special_points():
    d = np.load(GOLDEN)
    p, (lo, hi) = d["points"].astype(np.float64), d["volume_bounds"].astype(np.float64)
    for k in range(3):
        assert (p[:, k] < lo[k]).any() and (p[:, k] > hi[k]).any()
    assert (p == lo).all(1).any() and (p == hi).all(1).any()
    res = d["diff_weight_volume"].shape[:3]
    nodes = (p - lo) / (hi - lo) * (np.array(res) - 1)
    assert (np.abs(nodes - np.round(nodes)).max(1) < 1e-5).sum() >= int(np.prod(res))
    assert d["sdf_volume"].ndim == 3 and os.path.getsize(GOLDEN) < 512 * 1024


def _mesh():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, 0.5, -2.5]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [4, 2, 1]], np.int32)
    n = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, -1], [0.6, 0.8, 0]], np.float32)
    return v, f, n


def test_mesh_ply_round_trips_through_the_writer(tmp_path):
    from animatablegaussians_amd import obj_io, synth
    v, f, n = _mesh()
    for normals in (n, None):
        p = str(tmp_path / "sub" / "m.ply")
        obj_io.save_mesh_ply(p, v, f, normals)
        assert open(p, "rb").read(40).startswith(b"ply\nformat binary_little_endian 1.0\n")
        v2, f2, n2 = obj_io.load_mesh_ply(p)
        assert v2.dtype == np.float32 and f2.dtype == np.int32 and np.array_equal(v2, v) and np.array_equal(f2, f)
        assert (n2 is None) if normals is None else (n2.dtype == np.float32 and np.array_equal(n2, n))
    m = synth.body_mesh()
    p = str(tmp_path / "body.ply")
    obj_io.save_mesh_ply(p, m["vertices"], m["faces"])
    v2, f2, n2 = obj_io.load_mesh_ply(p)
    assert np.array_equal(v2, m["vertices"]) and np.array_equal(f2, m["faces"]) and n2 is None


def test_mesh_ply_ascii_assembled_by_hand(tmp_path):
    from animatablegaussians_amd import obj_io
    v, f, n = _mesh()
    # properties in another order, normals present, an extra scalar, the face list named vertex_index, an extra element in front
    lines = ["ply", "format ascii 1.0", "comment made by hand", "element thing 2", "property int a", "element vertex 5",
             "property float nz", "property float y", "property float x", "property uchar red", "property float z", "property float nx",
             "property float ny", "element face 3", "property uchar flag", "property list uchar int vertex_index", "end_header",
             "7", "8"]
    r = lambda x: repr(float(x))  # noqa: E731
    for i in range(5):
        lines.append(" ".join([r(n[i, 2]), r(v[i, 1]), r(v[i, 0]), str(10 * i), r(v[i, 2]), r(n[i, 0]), r(n[i, 1])]))
    for i in range(3):
        lines.append(f"1 3 {f[i, 0]} {f[i, 1]} {f[i, 2]}")
    p = str(tmp_path / "a.ply")
    open(p, "w").write("\n".join(lines) + "\n")
    v2, f2, n2 = obj_io.load_mesh_ply(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(n2, n)


def _big_endian_ply(v, faces, n_vertices=None, n_faces=None):
    head = ("ply\nformat binary_big_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty uchar red\nproperty double z\n"
            "element face %d\nproperty list uchar uint vertex_indices\nend_header\n") % (len(v) if n_vertices is None else n_vertices,
                                                                                         len(faces) if n_faces is None else n_faces)
    body = b"".join(struct.pack(">ddBd", float(x), float(y), 200 + i, float(z)) for i, (x, y, z) in enumerate(v))
    body += b"".join(struct.pack(">B%dI" % len(face), len(face), *[int(i) for i in face]) for face in faces)
    return head.encode("ascii") + body


def test_mesh_ply_big_endian_doubles_assembled_by_hand(tmp_path):
    from animatablegaussians_amd import obj_io
    v, f, _ = _mesh()
    p = str(tmp_path / "b.ply")
    open(p, "wb").write(_big_endian_ply(v, f))
    v2, f2, n2 = obj_io.load_mesh_ply(p)
    assert v2.dtype == np.float32 and np.array_equal(v2, v) and f2.dtype == np.int32 and np.array_equal(f2, f) and n2 is None


def test_mesh_ply_argument_errors(tmp_path):
    from animatablegaussians_amd import obj_io
    v, f, _ = _mesh()
    p = str(tmp_path / "e.ply")
    open(p, "wb").write(_big_endian_ply(v, [[0, 1, 2], [0, 1, 2, 3]]))
    with pytest.raises(ValueError, match="triangle"):
        obj_io.load_mesh_ply(p)
    whole = _big_endian_ply(v, f)
    for cut in (len(whole) - 5, len(whole) - 13 * len(f) - 7, 40):                    # inside the faces, the vertices, the header
        open(p, "wb").write(whole[:cut])
        with pytest.raises(ValueError, match="truncated"):
            obj_io.load_mesh_ply(p)
    open(p, "w").write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n1 1\n")
    with pytest.raises(ValueError, match="truncated"):
        obj_io.load_mesh_ply(p)
    open(p, "wb").write(b"solid not a ply\n")
    with pytest.raises(ValueError, match="not a PLY"):
        obj_io.load_mesh_ply(p)
    with pytest.raises(ValueError, match="one row per vertex"):
        obj_io.save_mesh_ply(p, v, f, normals=v[:2])


def test_synthetic_volume_follows_the_reference_bounds_rule():
    from animatablegaussians_amd import synth
    m = synth.body_mesh()
    a = synth.weight_volume_arrays(m, (9, 7, 5), 7)
    v = m["vertices"]
    assert a["diff_weight_volume"].shape == a["ori_weight_volume"].shape == (9, 7, 5, 7) and a["sdf_volume"].shape == (9, 7, 5)
    assert all(x.dtype == np.float32 for x in a.values())
    lo, hi = a["volume_bounds"]
    assert np.allclose(hi - lo, 1.1 * (v.max(0) - v.min(0)).max(), rtol=1e-6) and np.allclose(0.5 * (lo + hi), a["center"], atol=1e-6)
    assert np.allclose(a["center"], 0.5 * (v.min(0) + v.max(0)), atol=1e-7)
    assert np.allclose(a["smpl_bounds"], [v.min(0) - [0.05, 0.05, 0.15], v.max(0) + [0.05, 0.05, 0.15]], atol=1e-6)
    for k in ("diff_weight_volume", "ori_weight_volume"):
        assert (a[k] >= 0).all() and np.abs(a[k].astype(np.float64).sum(-1) - 1).max() < 1e-6
    assert (a["diff_weight_volume"] > 0).all()                                        # dense rows, as a diffused volume has
    assert a["sdf_volume"].max() > 0 > a["sdf_volume"].min()


def test_weight_volume_on_a_host_device_raises(tmp_path):
    import torch
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.weight_volume import WeightVolume
    a = synth.weight_volume_arrays(synth.body_mesh(), (4, 4, 4), 3)
    p = str(tmp_path / "cano_weight_volume.npz")
    np.savez(p, **a)
    with pytest.raises(ValueError, match="GPU"):
        WeightVolume.load(p, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        WeightVolume(*[torch.from_numpy(a[k]) for k in ("diff_weight_volume", "ori_weight_volume", "volume_bounds", "center", "smpl_bounds")])


def test_entry_points_declared_bound_and_exported():
    import inspect
    from animatablegaussians_amd import _lib, obj_io, subject_maps, weight_volume
    from animatablegaussians_amd.avatar import AvatarNet
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_weight_volume.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bag_weight_volume_sample\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "ag_weight_volume_sample is not declared in include/ag_weight_volume.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert len(table["ag_weight_volume_sample"][2]) == n_args == 10
    assert hasattr(L, "ag_weight_volume_sample"), "ag_weight_volume_sample is not exported"
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_weight_volume\.hip" \$EXACT', build) and STALE_HEADERS in build
    for fn in ("forward_weight", "forward_sdf", "load"):
        assert callable(getattr(weight_volume.WeightVolume, fn))
    assert not hasattr(weight_volume.WeightVolume, "forward_weight_grad")
    assert callable(obj_io.load_mesh_ply) and callable(obj_io.save_mesh_ply)
    assert callable(AvatarNet.from_template) and callable(AvatarNet.from_template_dir)
    p = inspect.signature(subject_maps.canonical_maps).parameters
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("weight_volume", "center"))
    assert list(p)[:5] == ["vertices", "faces", "normals", "lbs_weights", "size"] and p["size"].default == 1024
