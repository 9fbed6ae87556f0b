"""Iso-surface extraction on the GPU (``include/ag_isosurface.h``, ``isosurface.marching_cubes`` / ``recon_mesh``,
``WeightVolume.isosurface``) against ``isosurface_oracle.py``.

Bars, none derived from the kernel's output: faces EQUAL the oracle's as arrays; vertices equal the float32 oracle BIT FOR BIT and lie
within 4 x the worst |float32 oracle - float64 oracle| plus 2^-22 x the largest |coordinate| of the float64 oracle.  Both oracles
classify the same float32 values, so no case is left out.  Every test prints its own figures.

Known without a GPU: the kernels' source, compiled for the host and walked thread by thread under the address and
undefined-behaviour sanitizers (``profiles/ub/isosurface_host_walk.hip``), equals the float32 oracle bit for bit on the small shapes.
Measured on the MI355X: faces equal and vertices bit-identical to the float32 oracle on every case (so the deviation from float64 IS the
float32 oracle's own: e.g. 1.2e-7 against a bar of 9.1e-7 at (33, 34, 35)); sphere + torus: Euler [0, 2], signed volume 3415.175750 against
3415.175765 (bar 4.3e-2); 82 of 905 triangles degenerate and kept on the integer volume; mask case 1165 faces and 1072 vertices, both equal to
the cell-by-cell count; scan depth V 524 501, F 419 643; recon_mesh normals within 1.8e-7 of the float64 restatement (bar 1.0e-6), face normal .
mean vertex normal >= 0.986; closed chain: 648 vertices, 1292 faces, |forward_sdf| <= 2.2e-7 (bar 8.4e-7), the sign agrees at all 11 812 far
nodes, 676 268 template points; the whole file runs in 5 s.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isosurface_oracle as io  # noqa: E402
import mesh_query_oracle as mqo  # noqa: E402
import weight_volume_oracle as wvo  # noqa: E402

pytestmark = pytest.mark.gpu
SPACING, ORIGIN = (0.03, 0.02, 0.01), (-0.4, 1.1, 0.05)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()            # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(vol, iso=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), mask=None):
    from animatablegaussians_amd.isosurface import marching_cubes
    v, f = marching_cubes(_t(vol), iso, spacing, origin, None if mask is None else _t(mask))
    assert v.is_cuda and f.is_cuda and v.dtype.is_floating_point and str(f.dtype) == "torch.int32"
    return v.cpu().numpy(), f.cpu().numpy()


def _check(name, vol, iso=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), mask=None, finite=True):
    """The three bars of the module docstring; returns the GPU's (vertices, faces) and the vertex bar."""
    v32, f32 = io.extract(vol, iso, spacing, origin, mask, np.float32)
    v64, f64 = io.extract(vol, iso, spacing, origin, mask, np.float64)
    assert np.array_equal(f32, f64)
    v, f = _run(vol, iso, spacing, origin, mask)
    assert v.shape == v32.shape and f.shape == f32.shape, f"{name}: V, F = {len(v)}, {len(f)}; the oracle's {len(v32)}, {len(f32)}"
    with np.errstate(all="ignore"):
        own = float(np.nanmax(np.abs(v32.astype(np.float64) - v64), initial=0.0))
        bar = 4 * own + 2.0 ** -22 * float(np.nanmax(np.abs(v64), initial=0.0))
        dev = float(np.nanmax(np.abs(v.astype(np.float64) - v64), initial=0.0))
    differ = int((_bits(v) != _bits(v32)).sum())
    print(f"{name}: V {len(v)}, F {len(f)}; faces that differ {int((f != f32).any(1).sum())}; vertex words that differ from the float32 oracle {differ}; "
          f"|gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
    assert np.array_equal(f, f32), f"{name}: faces differ from the oracle's"
    assert differ == 0, f"{name}: {differ} vertex words differ from the float32 oracle"
    assert dev <= bar
    if finite:
        assert np.isfinite(v).all()
    return v, f, bar


def test_every_case_in_isolation():
    vol, mask = io.every_case_volume()
    v, f, _ = _check("all 256 cases, one per third cell", vol, 0.0, mask=mask)
    assert len(f) == 820 == int(io.TRI_COUNT.sum())
    # spacing 1, origin 0: the faces of carrier c use vertices with z in [3 c, 3 c + 1] only
    first = np.concatenate([[0], np.cumsum(io.TRI_COUNT)])
    for c in range(256):
        used = f[first[c]:first[c + 1]].reshape(-1)
        assert ((v[used, 2] >= 3 * c) & (v[used, 2] <= 3 * c + 1)).all(), f"case {c} uses a vertex outside its cell"


@pytest.mark.parametrize("case", [0, 255, 1, 0x69])
def test_single_cell(case):
    rng = np.random.default_rng(case)
    vol = np.empty((2, 2, 2), np.float32)
    for corner in range(8):
        vol[corner & 1, (corner >> 1) & 1, corner >> 2] = (0.25 + 0.75 * rng.random()) * (1 if (case >> corner) & 1 else -1)
    v, f, _ = _check(f"case {case:#04x} alone", vol)
    assert len(f) == io.TRI_COUNT[case] and v.shape == (len(v), 3) and f.shape == (len(f), 3)


@pytest.mark.parametrize("iso", [0.0, 0.137])
@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 7, 2), (5, 4, 3), (17, 9, 33), (33, 34, 35)])
def test_noise_touching_the_border(shape, iso):
    _check(f"noise {shape}, iso {iso}", io.noise_field(shape, 11), iso, SPACING, ORIGIN)


@functools.lru_cache(maxsize=None)
def _two_bodies():
    shape = (40, 36, 44)
    vol = np.maximum(io.sphere_field(shape, (11.3, 17.6, 12.4), 7.7), io.torus_field(shape, (26.4, 18.3, 29.6), 8.2, 3.1))
    vol.setflags(write=False)
    return vol


def _volume_gradient_l1(v, f):
    """sum_i |dVol / dv_i|_1 of Vol = sum_faces det(v0, v1, v2) / 6: what one unit of per-coordinate vertex error can move the volume."""
    v = np.asarray(v, np.float64)
    g = np.zeros_like(v)
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        np.add.at(g, f[:, a], np.cross(v[f[:, b]], v[f[:, c]]) / 6.0)
    return float(np.abs(g).sum())


def test_sphere_and_disjoint_torus():
    vol = _two_bodies()
    v, f, bar = _check("sphere + torus (40, 36, 44)", vol)
    _, counts, closed = io.directed_edge_census(f)
    chi = io.euler_characteristics(f, len(v))
    v64, _ = io.extract(vol, dtype=np.float64)
    got, want = io.signed_volume(v, f), io.signed_volume(v64, f)
    # first order in the vertex error, from the float64 oracle's mesh; the higher orders are smaller by bar / cell size (< 1e-4): 1 %
    vol_bar = 1.01 * bar * _volume_gradient_l1(v64, f)
    print(f"closed and oriented {closed} (a directed edge at most {int(counts.max())} times), Euler {chi}, signed volume {got:.6f} / {want:.6f}, "
          f"difference {abs(got - want):.3e}, bar {vol_bar:.3e}")
    assert closed and chi == [0, 2]
    assert got > 0 and abs(got - want) <= vol_bar


def test_values_exactly_on_the_level():
    rng = np.random.default_rng(5)
    vol = rng.integers(-1, 2, (9, 8, 7)).astype(np.float32)
    v, f, _ = _check("integers from {-1, 0, 1} at (9, 8, 7)", vol, 0.0, SPACING, ORIGIN)
    tri = v[f].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    print(f"degenerate triangles kept: {int((area == 0).sum())} of {len(f)}")
    assert (area == 0).any() and np.isfinite(v).all()


def test_mask_and_non_finite_nodes():
    rng = np.random.default_rng(5)
    vol = io.noise_field((12, 11, 10), 6)
    mask = rng.random(vol.shape) >= 0.1
    bad = [17, 400, 901, 555]
    vol.reshape(-1)[bad[:3]] = np.nan
    vol.reshape(-1)[bad[3]] = np.inf
    v, f, _ = _check("(12, 11, 10), 10 % masked, 3 NaN, 1 inf", vol, 0.0, SPACING, ORIGIN, mask)
    # counted independently, cell by cell
    ok = np.isfinite(vol) & mask
    want_f, touched = 0, set()
    X, Y, Z = vol.shape
    for i in range(X - 1):
        for j in range(Y - 1):
            for k in range(Z - 1):
                if not ok[i:i + 2, j:j + 2, k:k + 2].all():
                    continue
                case = sum(int(vol[i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)] >= 0) << c for c in range(8))
                want_f += int(io.TRI_COUNT[case])
                for e in set(io.TRI_TABLE[case][io.TRI_TABLE[case] >= 0].tolist()):
                    lo, _ = io._edge_corners(e)
                    touched.add((((i + lo[0]) * Y + j + lo[1]) * Z + k + lo[2]) * 3 + e // 4)
    full_v, full_f = io.extract(np.where(np.isfinite(vol), vol, 1.0).astype(np.float32), 0.0, SPACING, ORIGIN)
    print(f"faces {len(f)} (cell by cell {want_f}), vertices {len(v)} (edges of processed cells {len(touched)}); unmasked finite volume: {len(full_v)}, {len(full_f)}")
    assert len(f) == want_f and len(v) == len(touched) and len(v) < len(full_v) and np.isfinite(v).all()


def test_empty_results():
    vol = io.noise_field((6, 5, 4), 1)
    for name, iso in (("all below", 100.0), ("all at or above", -100.0)):
        v, f = _run(vol, iso)
        print(f"{name}: {v.shape}, {f.shape}")
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32
    v, f = _run(np.zeros((3, 3, 3), np.float32), 0.0)                    # every node exactly on the level is inside
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_scan_depth():
    """The scans work on blocks of 1024 items (256 threads x 4) and recurse on the block sums.  [2, 2, L] has 12 L + 1 edge items: more
    than 1024^2 of them, L > 87 381, puts more than one block on level 0 (1537 blocks) AND on level 1 (2 blocks), with the single top
    block above them; the 4 L + 1 cell items (513 blocks, then the top) take the two-level path in the same call.  A further level needs
    more than 2^30 items, a volume of 3.6e8 nodes; it is the same code (the levels are one loop).  L = 2^17 + 3 is not a multiple of any
    block size, so every level ends in a partial block."""
    L = 2 ** 17 + 3
    assert 12 * L + 1 > 1024 ** 2 and 4 * L + 1 > 1024
    _check(f"[2, 2, {L}]", io.noise_field((2, 2, L), 3), 0.0, SPACING, ORIGIN)


def test_repeatability():
    vol = io.noise_field((33, 34, 35), 12)
    a, b = _run(vol, 0.05, SPACING, ORIGIN), _run(vol, 0.05, SPACING, ORIGIN)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and len(a[1]) > 10000
    print(f"two calls: V {len(a[0])}, F {len(a[1])}, identical bits")


def test_recon_mesh_on_a_sphere():
    from animatablegaussians_amd.isosurface import recon_mesh
    res = (20, 18, 16)
    bounds = np.array([[-0.9, 0.2, 1.1], [1.1, 2.0, 2.7]], np.float32)
    voxel = (bounds[1] - bounds[0]) / np.array(res, np.float32)
    centres = [bounds[0][d] + (np.arange(res[d], dtype=np.float32) + 0.5) * voxel[d] for d in range(3)]
    g = np.stack(np.meshgrid(*centres, indexing="ij"), -1).astype(np.float64)
    centre = np.array([0.13, 1.07, 1.93])
    sdf = (0.5 - np.linalg.norm(g - centre, axis=-1)).astype(np.float32)
    v, f, n = recon_mesh(_t(sdf).reshape(-1), res, _t(bounds), iso_value=0.0)
    assert v.is_cuda and f.is_cuda and n.is_cuda
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    # the reference's formula: skimage's vertices are idx * voxel_size; + bounds[0] + 0.5 * voxel_size
    i32, f32 = io.extract(sdf, 0.0, voxel, (0, 0, 0), None, np.float32)
    i64, _ = io.extract(sdf, 0.0, voxel, (0, 0, 0), None, np.float64)
    w32 = i32 + bounds[0] + np.float32(0.5) * voxel
    w64 = i64 + bounds[0].astype(np.float64) + 0.5 * voxel.astype(np.float64)
    own = float(np.abs(w32.astype(np.float64) - w64).max())
    bar = 4 * own + 2.0 ** -22 * float(np.abs(w64).max())
    dev = float(np.abs(v.astype(np.float64) - w64).max())
    print(f"V {len(v)}, F {len(f)}: vertex words that differ from the float32 restatement {int((_bits(v) != _bits(w32)).sum())}, |gpu - float64| {dev:.3e}, "
          f"own {own:.3e}, bar {bar:.3e}; distance of the vertices from the sphere {float(np.abs(np.linalg.norm(v - centre, axis=1) - 0.5).max()):.3e}")
    assert np.array_equal(f, f32) and np.array_equal(_bits(v), _bits(w32)) and dev <= bar
    assert np.abs(np.linalg.norm(v - centre, axis=1) - 0.5).max() < 0.1 * voxel.min()       # half-voxel convention: off by 0.5 voxel otherwise
    # normals: the torch-CPU restatement at the SAME sample points, in float32 and float64
    pts = (v - bounds[0]) / (bounds[1] - bounds[0])
    import torch
    n32 = io.reference_normals(sdf, voxel, pts, torch.float32)
    n64 = io.reference_normals(sdf, voxel, pts, torch.float64)
    n_own = float(np.abs(n32.astype(np.float64) - n64).max())
    n_bar = 4 * n_own + 2.0 ** -22
    n_dev = float(np.abs(-n.astype(np.float64) - n64).max())
    tri = v[f].astype(np.float64)
    geo = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    dots = np.einsum("ij,ij->i", geo / np.linalg.norm(geo, axis=1, keepdims=True), n[f].astype(np.float64).mean(1))
    radial = np.einsum("ij,ij->i", n, (v - centre) / np.linalg.norm(v - centre, axis=1, keepdims=True))
    print(f"normals: |gpu - float64 restatement| {n_dev:.3e}, the float32 restatement's own {n_own:.3e}, bar {n_bar:.3e}; face normal . mean vertex normal "
          f">= {float(dots.min()):.3f}; normal . radial direction >= {float(radial.min()):.3f}")
    assert n_dev <= n_bar
    assert (dots > 0).all() and (radial > 0.9).all()


@functools.lru_cache(maxsize=None)
def _chain():
    from animatablegaussians_amd.weight_volume import WeightVolume
    mv, mf = mqo.lattice_mesh()
    vol = WeightVolume.from_body_mesh(_t(mv), _t(mf), _t(mqo.sparse_weights(mv)), res=(24, 28, 20))
    v, f = vol.isosurface()
    return vol, v, f


def test_closed_chain_surface_and_sdf():
    import torch
    from animatablegaussians_amd import mesh_query
    vol, v, f = _chain()
    sdf = vol.smpl_sdf_volume[..., 0].cpu().numpy()
    lo, vs = vol.volume_bounds[0].cpu().numpy(), vol.voxel_size.cpu().numpy()
    v32, f32 = io.extract(sdf, 0.0, vs, lo, None, np.float32)
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    _, counts, closed = io.directed_edge_census(fh)
    print(f"V {len(vh)}, F {len(fh)}, closed and oriented {closed}, Euler {io.euler_characteristics(fh, len(vh))}")
    assert np.array_equal(fh, f32) and np.array_equal(_bits(vh), _bits(v32)) and closed
    # forward_sdf at the vertices: trilinear interpolation is the linear one on a grid edge, so the sampled SDF is 0 up to rounding
    got = vol.forward_sdf(v)[:, 0].cpu().numpy().astype(np.float64)
    bounds = vol.volume_bounds.cpu().numpy()
    own = np.abs(wvo.sample(sdf[..., None], vh, bounds, np.float64)[:, 0])
    bar = 4 * float(own.max()) + 2.0 ** -22 * float(np.abs(sdf).max())
    print(f"|forward_sdf| at the vertices {float(np.abs(got).max()):.3e}; the float64 sampler at the same float32 vertices {float(own.max()):.3e}; bar {bar:.3e}")
    assert np.abs(got).max() <= bar
    # the sign of mesh_query.signed_distance against the EXTRACTED mesh (negative inside) where |sdf| exceeds one voxel diagonal
    far = np.abs(sdf) > float(np.linalg.norm(vs))
    axes = np.meshgrid(*[lo[d] + np.arange(sdf.shape[d], dtype=np.float32) * vs[d] for d in range(3)], indexing="ij")
    nodes = np.stack(axes, -1)[far].astype(np.float32)
    d, _, _ = mesh_query.signed_distance(_t(nodes), v, f)
    agree = np.sign(-d.cpu().numpy()) == np.sign(sdf[far])
    print(f"nodes farther than a voxel diagonal {int(far.sum())} of {far.size}, sign agrees on {int(agree.sum())}")
    assert far.sum() > 1000 and agree.all()
    assert torch.equal(*(vol.isosurface()[1], f))


def test_closed_chain_file_and_template(tmp_path):
    from animatablegaussians_amd.avatar import AvatarNet
    from animatablegaussians_amd.obj_io import load_mesh_ply, save_mesh_ply
    vol, v, f = _chain()
    path = str(tmp_path / "template.ply")
    save_mesh_ply(path, v.cpu(), f.cpu())
    lv, lf, ln = load_mesh_ply(path)
    assert np.array_equal(_bits(lv), _bits(v.cpu().numpy())) and np.array_equal(lf, f.cpu().numpy()) and ln is None
    net = AvatarNet.from_template({'with_viewdirs': True}, _t(lv), _t(lf), vol)
    print(f"template of {len(lv)} vertices, {len(lf)} faces -> {net.init_points.shape[0]} points")
    assert net.init_points.shape[0] > 1000 and net.lbs.shape[0] == net.init_points.shape[0]


def test_python_argument_errors():
    import torch
    from animatablegaussians_amd.isosurface import marching_cubes, recon_mesh
    from animatablegaussians_amd.weight_volume import WeightVolume
    vol = _t(io.noise_field((4, 5, 6), 0))
    for bad in (lambda: marching_cubes(vol.cpu()), lambda: marching_cubes(vol[0]), lambda: marching_cubes(vol.double()),
                lambda: marching_cubes(np.zeros((4, 5, 6), np.float32)),
                lambda: marching_cubes(vol, mask=torch.ones((4, 5, 5), dtype=torch.bool, device="cuda")),
                lambda: marching_cubes(vol, mask=torch.ones((4, 5, 6), dtype=torch.float32, device="cuda")),
                lambda: marching_cubes(vol, mask=torch.ones((4, 5, 6), dtype=torch.bool)),
                lambda: marching_cubes(vol[:1]), lambda: marching_cubes(vol, spacing=(1.0, 0.0, 1.0)), lambda: marching_cubes(vol, spacing=(1.0, 1.0)),
                lambda: marching_cubes(vol, iso=float("nan")), lambda: marching_cubes(vol, origin=(0.0, float("inf"), 0.0)),
                lambda: recon_mesh(vol.cpu(), (4, 5, 6), np.zeros((2, 3))), lambda: recon_mesh(vol, (4, 5, 7), np.zeros((2, 3))),
                lambda: recon_mesh(vol, (4, 5, 6), np.zeros((3, 2)))):
        with pytest.raises(ValueError):
            bad()
    w = torch.rand(3, 3, 3, 2, device="cuda")
    b = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    with pytest.raises(ValueError):
        WeightVolume(w, w, b, np.zeros(3, np.float32), b).isosurface()
    # a non-contiguous view and a uint8 mask are taken
    v, f = marching_cubes(vol.permute(2, 1, 0), mask=torch.ones((6, 5, 4), dtype=torch.uint8, device="cuda"))
    want_v, want_f = io.extract(vol.cpu().numpy().transpose(2, 1, 0))
    assert np.array_equal(f.cpu().numpy(), want_f) and np.array_equal(_bits(v.cpu().numpy()), _bits(want_v))


def test_abi_refusals():
    import torch
    from animatablegaussians_amd import _lib
    L = _lib.lib()
    X, Y, Z = 5, 4, 3
    vol = _t(io.noise_field((X, Y, Z), 0))
    n_ws = int(L.ag_isosurface_workspace_bytes(X, Y, Z))
    assert n_ws > 17 * X * Y * Z
    ws = torch.zeros(n_ws, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    one, zero3 = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0)

    def refused(rc, code, *words):
        msg = L.ag_last_error().decode()
        print(f"  {rc}: {msg}")
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def count(vp=p(vol), x=X, y=Y, z=Z, iso=0.0, wp=p(ws), nb=n_ws, cp=p(counts)):
        return L.ag_isosurface_count(vp, None, x, y, z, iso, wp, nb, cp, None)

    def emit(v, V, f, F, x=X, y=Y, z=Z, iso=0.0, sp=one, org=zero3, vp=p(vol), wp=p(ws), nb=n_ws):
        return L.ag_isosurface_emit(vp, x, y, z, iso, sp, org, wp, nb, None if v is None else p(v), V, None if f is None else p(f), F, None)

    INV = -1
    refused(count(x=1), INV, "at least 2")
    refused(count(z=1), INV, "at least 2")
    refused(count(vp=None), INV, "null")
    refused(count(wp=None), INV, "null")
    refused(count(cp=None), INV, "null")
    refused(count(iso=float("inf")), INV, "iso")
    refused(count(iso=float("nan")), INV, "iso")
    refused(count(nb=n_ws - 1), _lib.AG_ERR_SCRATCH_TOO_SMALL, "workspace")
    # sizes only: nothing of that size is allocated, the refusal comes before any pointer is read
    assert L.ag_isosurface_workspace_bytes(1024, 1024, 683) == 0 and L.ag_isosurface_workspace_bytes(1024, 1024, 682) > 0
    refused(count(x=1024, y=1024, z=683), INV, "2^31")
    assert count() == 0
    torch.cuda.synchronize()
    V, F = (int(c) for c in counts.cpu())
    want_v, want_f = io.extract(vol.cpu().numpy())
    assert (V, F) == (len(want_v), len(want_f)) and V > 0 and F > 0
    v = torch.zeros((V + 1, 3), device="cuda")
    f = torch.full((F + 1, 3), -7, dtype=torch.int32, device="cuda")
    refused(emit(v, V, f, F, x=1), INV, "at least 2")
    refused(emit(v, V, f, F, vp=None), INV, "null")
    refused(emit(None, V, f, F), INV, "null")
    refused(emit(v, V, None, F), INV, "null")
    refused(emit(v, V, f, F, sp=(ctypes.c_float * 3)(1, 0, 1)), INV, "spacing")
    refused(emit(v, V, f, F, sp=(ctypes.c_float * 3)(1, -1, 1)), INV, "spacing")
    refused(emit(v, V, f, F, sp=(ctypes.c_float * 3)(1, float("inf"), 1)), INV, "spacing")
    refused(emit(v, V, f, F, sp=None), INV, "NULL")
    refused(emit(v, V, f, F, iso=float("nan")), INV, "iso")
    refused(emit(v, V, f, F, nb=n_ws - 1), _lib.AG_ERR_SCRATCH_TOO_SMALL, "workspace")
    refused(emit(v, V + 1, f, F), INV, f"V = {V}")
    refused(emit(v, V, f, F + 1), INV, f"F = {F}")
    refused(emit(v, V - 1, f, F - 1), INV, "count")
    refused(emit(v, V, f, F, x=Y, y=X), INV, "workspace does not hold")
    torch.cuda.synchronize()
    assert (v == 0).all() and (f == -7).all(), "a refused call wrote its outputs"
    assert emit(v, V, f, F) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(v[:V].cpu().numpy()), _bits(want_v)) and np.array_equal(f[:F].cpu().numpy(), want_f)
    assert (v[V] == 0).all() and (f[F] == -7).all(), "emit wrote past V or F"
