"""A subject's canonical assets from its mesh, on the GPU (``include/ag_subject_maps.h``).

What the reference's ``gen_data/gen_pos_maps.py:93-134`` produces with an OpenGL context, trimesh, OpenCV and pytorch3d -- the
front|back canonical position and normal maps and the per-point skinning weights -- and the k-NN scale initialiser of
``GaussianModel.create_from_pcd`` (``gaussians/gaussian_model.py:170-171``):

    rasterize_ortho  ->  resolve (positions, normals: dense; skinning weights: compacted)  ->  knn_log_scale

The two views (derived from ``gen_pos_maps.py:93-102`` and ``renderer_gl.py:363-375``; c = ``cano_center``, S px span 2 m):
pixel (r, c) of BOTH halves samples world x = cx + (2c+1)/S - 1, y = cy + 1 - (2r+1)/S; the front half keeps the surface with the
largest z and culls by the winding seen from +z, the back half keeps the smallest z and culls by the winding seen from -z.  The
reference's depth row (near 0.1, far 100, camera 10 m away) is replaced by depth = -+(z - cz): the same order in real numbers,
without the offset of ~0.8 that would cost fp32 eight bits of depth resolution; nothing is clipped in depth.

NOT pinned: no image written by an OpenGL implementation exists for this package to compare with, so parity with a vendor's
fixed-point vertex snapping and 24-bit depth buffer is not claimed.  The contract is the float64 restatement of the rasterization
rules in ``tests/subject_maps_oracle.py``.

Every tensor must be on the GPU; there is no host path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import stream as _stream
from .avatar_ops import mask_to_pix


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(t: torch.Tensor, name: str, dtype, cols: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (there is no host path)")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError(f"{name} must be [n, {cols}], got {tuple(t.shape)}")
    return t.to(dtype).contiguous()


def view_matrices(cano_center) -> Tuple[np.ndarray, np.ndarray]:
    """(front, back) world -> NDC, 3 x 4 float32.  The back matrix is the un-mirrored render (``mirror_cols`` undoes it)."""
    cx, cy, cz = (np.float32(v) for v in cano_center)
    front = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, -1, cz]], np.float32)
    back = np.array([[-1, 0, 0, cx], [0, 1, 0, -cy], [0, 0, 1, -cz]], np.float32)
    return front, back


def rasterize_ortho(vertices: torch.Tensor, faces: torch.Tensor, view, size, *, cull: bool = True, flip_rows: bool = True,
                    mirror_cols: bool = False, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, col0: int = 0):
    """-> (face_id [H, W] int32, -1 = empty; bary [H, W, 3]).  ``view``: 3 x 4 world -> NDC; ``size``: S or (W, H).
    ``out`` = (face_id, bary) of a wider canvas and ``col0`` place the view at canvas columns [col0, col0 + W).
    Semantics, tie rules and the fp32 operation order: ``include/ag_subject_maps.h``."""
    v = _dev(vertices, "vertices", torch.float32, 3)
    f = _dev(faces, "faces", torch.int32, 3)
    W, H = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    view = np.ascontiguousarray(np.asarray(view, np.float32).reshape(-1))
    if view.size != 12:
        raise ValueError("view must be a 3 x 4 world -> NDC matrix")
    dev = v.device
    if out is None:
        face_id = torch.empty(H, W, dtype=torch.int32, device=dev)
        bary = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    else:
        face_id, bary = out
        if (not isinstance(face_id, torch.Tensor) or not isinstance(bary, torch.Tensor) or face_id.device != dev or bary.device != dev
                or face_id.dim() != 2 or face_id.dtype != torch.int32 or not face_id.is_contiguous() or face_id.shape[0] != H
                or bary.dtype != torch.float32 or not bary.is_contiguous() or tuple(bary.shape) != tuple(face_id.shape) + (3,)):
            raise ValueError("out must be contiguous (int32 [H, stride], float32 [H, stride, 3]) on the vertices' GPU")
        if col0 < 0 or col0 + W > face_id.shape[1]:
            raise ValueError(f"columns [{col0}, {col0 + W}) do not fit a canvas of {face_id.shape[1]} columns")
    L = _lib.lib()
    ws = torch.empty(L.ag_mesh_rasterize_ortho_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    a = _lib.AgMeshRasterArgs()
    a.V, a.F, a.W, a.H = v.shape[0], f.shape[0], W, H
    a.cull, a.flip_rows, a.mirror_cols = int(cull), int(flip_rows), int(mirror_cols)
    a.out_col0, a.out_stride = int(col0), int(face_id.shape[1])
    a.view[:] = view.tolist()
    a.vertices, a.faces, a.face_id, a.bary = _p(v), _p(f), _p(face_id), _p(bary)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    with _lib.on_device(dev):
        _lib.check(L.ag_mesh_rasterize_ortho(ctypes.byref(a), _stream(dev)), "ag_mesh_rasterize_ortho")
    return face_id, bary


def resolve(face_id: torch.Tensor, bary: torch.Tensor, faces: torch.Tensor, attribute: torch.Tensor,
            pix: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Barycentric interpolation of a per-vertex attribute [V, C]: dense -> face_id.shape + (C,), exactly 0 on empty pixels; with a
    pixel list ``pix`` [N] (flat indices into the canvas) -> [N, C]."""
    fid = _dev(face_id, "face_id", torch.int32)
    b = _dev(bary, "bary", torch.float32)
    f = _dev(faces, "faces", torch.int32, 3)
    a = _dev(attribute, "attribute", torch.float32)
    if a.dim() != 2 or tuple(b.shape) != tuple(fid.shape) + (3,):
        raise ValueError("attribute must be [V, C] and bary face_id.shape + (3,)")
    C, n_pix = a.shape[1], fid.numel()
    if pix is not None:
        pix = _dev(pix, "pix", torch.int32)
        out = torch.empty(pix.numel(), C, dtype=torch.float32, device=a.device)
    else:
        out = torch.empty(tuple(fid.shape) + (C,), dtype=torch.float32, device=a.device)
    with _lib.on_device(a.device):
        _lib.check(_lib.lib().ag_mesh_resolve_attribute(_p(fid), _p(b), _p(f), _p(a), a.shape[0], f.shape[0], C, n_pix, _p(pix),
                                                        0 if pix is None else pix.numel(), _p(out), _stream(a.device)),
                   "ag_mesh_resolve_attribute")
    return out


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Unit per-vertex normals [V, 3]: the sum over a vertex's corners of the unit face normal weighted by the corner angle,
    normalised (zero where a vertex has no non-degenerate face).

    This is NOT pinned to trimesh's ``vertex_normals`` (what ``gen_pos_maps.py:91`` uses): trimesh is not available to this package
    and its weighting is a sparse-matrix detail of its own.  The normal map feeds only the cosine between surface normal and view
    direction (``AvatarNet.get_viewdir_feat``).  The per-vertex sum is a dense [V, valence] reduction, not an atomic scatter, so the
    result is the same on every run."""
    v = _dev(vertices, "vertices", torch.float32, 3)
    f = _dev(faces, "faces", torch.int64, 3)
    p = v[f]                                                                   # [F, 3 corners, 3]
    e1, e2 = torch.roll(p, -1, 1) - p, torch.roll(p, 1, 1) - p                 # the two edges leaving each corner
    fn = torch.nn.functional.normalize(torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), dim=-1)
    cosang = (torch.nn.functional.normalize(e1, dim=-1) * torch.nn.functional.normalize(e2, dim=-1)).sum(-1).clamp(-1, 1)
    contrib = (torch.acos(cosang)[..., None] * fn[:, None, :]).reshape(-1, 3)  # [3F, 3]
    owner = f.reshape(-1)
    order = torch.sort(owner, stable=True)[1]
    so = owner[order]
    V = v.shape[0]
    first = torch.searchsorted(so, torch.arange(V, device=v.device))
    slot = torch.arange(so.numel(), device=v.device) - first[so]
    dense = torch.zeros(V, int(slot.max().item()) + 1 if so.numel() else 1, 3, device=v.device)
    dense[so, slot] = contrib[order]
    return torch.nn.functional.normalize(dense.sum(1), dim=-1)


def knn_grid(points: torch.Tensor, cell: Optional[float] = None):
    """The search grid of ``knn_dist2``: (origin [3] float32, cell size, dims [3]).  It decides the time, never the result."""
    pts = _dev(points, "points", torch.float32, 3)
    N = pts.shape[0]
    lo, hi = pts.amin(0), pts.amax(0)
    ext = (hi - lo).double().cpu().numpy()
    lo = lo.cpu().numpy()
    if cell is None:
        # ~8 points per OCCUPIED cell.  First guess: 8 per cell of the bounding box; the points lie on a surface, where most of those
        # cells are empty and the occupancy of the others goes with cell^2: one correction from the counted occupancy.
        nz = np.maximum(ext, max(1e-3 * float(ext.max()), 1e-9))
        cell = float(np.cbrt(nz.prod() * 8.0 / N))
        d0 = [int(e / cell) + 1 for e in ext]                                  # d0[0] * d0[1] * d0[2] <~ 1e6 * N / 8: fits int64
        ids = ((pts - pts.amin(0)) / cell).floor().long()
        occ = torch.unique((ids[:, 0] * d0[1] + ids[:, 1]) * d0[2] + ids[:, 2]).numel()
        cell *= float(np.sqrt(min(1.0, 8.0 * occ / N)))
    cell = max(float(cell), float(ext.max()) * 1e-6, 1e-12)
    dims = np.floor(ext / cell).astype(np.int64) + 1
    while dims.prod() > (1 << 22):                                             # bounds the workspace; coarser cells stay exact
        cell *= 1.26
        dims = np.floor(ext / cell).astype(np.int64) + 1
    return lo, cell, dims


def knn_dist2(points: torch.Tensor, cell: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (mean [N], sorted [N, 3]) squared distances to the 3 nearest other points (``knn_points(K = 4)[..., 1:]``), exact over all
    N points.  ``cell``: grid cell size (time only, never the result); default: from the point density (``knn_grid``)."""
    pts = _dev(points, "points", torch.float32, 3)
    N = pts.shape[0]
    if N < 4:
        raise ValueError(f"k-NN with K = 4 (the point itself and 3 neighbours) needs at least 4 points, got {N}")
    lo, cell, dims = knn_grid(pts, cell)
    L = _lib.lib()
    ws = torch.empty(L.ag_knn_mean_dist2_workspace_bytes(N, int(dims.prod())), dtype=torch.uint8, device=pts.device)
    mean = torch.empty(N, dtype=torch.float32, device=pts.device)
    d3 = torch.empty(N, 3, dtype=torch.float32, device=pts.device)
    with _lib.on_device(pts.device):
        _lib.check(L.ag_knn_mean_dist2(_p(pts), N, (ctypes.c_float * 3)(*[float(x) for x in lo]), cell,
                                       (ctypes.c_int32 * 3)(*[int(d) for d in dims]), _p(mean), _p(d3), _p(ws), ws.numel(),
                                       _stream(pts.device)), "ag_knn_mean_dist2")
    return mean, d3


def knn_log_scale(points: torch.Tensor) -> torch.Tensor:
    """``log sqrt(clamp_min(mean squared distance to the 3 nearest neighbours, 1e-7))`` [N]  (gaussian_model.py:170-171)."""
    return torch.log(torch.sqrt(torch.clamp_min(knn_dist2(points)[0], 1e-7)))


def canonical_maps(vertices: torch.Tensor, faces: torch.Tensor, normals: torch.Tensor, lbs_weights: Optional[torch.Tensor] = None,
                   size: int = 1024, *, weight_volume=None, center: Optional[torch.Tensor] = None,
                   lbs_rule: str = "rendered") -> Dict[str, torch.Tensor]:
    """The canonical part of ``gen_pos_maps.py`` (:75, :93-134) plus the scale initialiser.  Without the keywords: the
    SMPL-X-as-template branch, the mesh IS the body and ``lbs_weights`` [V, J] are interpolated.  With ``weight_volume`` (a
    ``weight_volume.WeightVolume``): the ``using_template`` branch (:79-82, :128-130), the mesh is the clothed template,
    ``lbs_weights`` may be ``None`` and ``init_pts_lbs = weight_volume.forward_weight(cano_pos_map[mask])``, not renormalised, as in
    the reference.  ``center`` [3] (on the GPU) is the centre of the two views; default: the centre of the mesh's bounding box, or with
    a volume its ``center`` -- the reference takes the centre of the SMPL-X body also when it renders a template (:75 runs before
    :88), and that is the ``center`` ``gen_weight_volume.py:139`` stores.  Returns

    ``cano_smpl_pos_map`` / ``cano_smpl_nml_map`` [S, 2S, 3] (front | back, zeros where empty), ``mask`` [S, 2S] (``|pos| > 0``),
    ``init_pts_lbs`` [N, J] in ``map[mask]`` order, ``log_scale`` [N], ``cano_center`` [3], and ``face_id`` / ``bary``.
    ``lbs_rule`` (the per-vertex branch only): ``'rendered'`` interpolates the weights with the RENDERED face and its barycentrics;
    ``'nearest'`` is the reference's rule (:132), the nearest face of the rendered point (``mesh_query.interpolate_lbs``): the same
    weights up to rounding, at the cost of a search over all faces per point."""
    v = _dev(vertices, "vertices", torch.float32, 3)
    f = _dev(faces, "faces", torch.int32, 3)
    n = _dev(normals, "normals", torch.float32, 3)
    if weight_volume is None or lbs_weights is not None:
        w = _dev(lbs_weights, "lbs_weights", torch.float32)
        if w.dim() != 2 or w.shape[0] != v.shape[0]:
            raise ValueError("normals [V, 3] and lbs_weights [V, J] must have one row per vertex")
    if n.shape[0] != v.shape[0]:
        raise ValueError("normals [V, 3] and lbs_weights [V, J] must have one row per vertex")
    if lbs_rule not in ("rendered", "nearest"):
        raise ValueError(f"lbs_rule must be 'rendered' or 'nearest', got {lbs_rule!r}")
    S = int(size)
    if center is None:
        center = 0.5 * (v.amin(0) + v.amax(0)) if weight_volume is None else weight_volume.center       # gen_pos_maps.py:75
    center = _dev(center, "center", torch.float32).reshape(-1)
    if center.numel() != 3:
        raise ValueError(f"center must have 3 components, got {tuple(center.shape)}")
    front, back = view_matrices(center.cpu().numpy())
    face_id = torch.empty(S, 2 * S, dtype=torch.int32, device=v.device)
    bary = torch.empty(S, 2 * S, 3, dtype=torch.float32, device=v.device)
    rasterize_ortho(v, f, front, S, out=(face_id, bary), col0=0)
    rasterize_ortho(v, f, back, S, mirror_cols=True, out=(face_id, bary), col0=S)
    pos = resolve(face_id, bary, f, v)
    nml = resolve(face_id, bary, f, n)
    mask = torch.linalg.norm(pos, dim=-1) > 0.                                 # :126
    pix = mask_to_pix(mask)
    init_points = pos.reshape(-1, 3)[pix.long()]
    if weight_volume is not None:
        lbs = weight_volume.forward_weight(init_points)                         # :129-130
    elif lbs_rule == "nearest":
        from .mesh_query import interpolate_lbs
        lbs = interpolate_lbs(init_points, v, f, w)                             # :132
    else:
        lbs = resolve(face_id, bary, f, w, pix=pix)
    return {"cano_smpl_pos_map": pos, "cano_smpl_nml_map": nml, "mask": mask, "init_pts_lbs": lbs,
            "log_scale": knn_log_scale(init_points), "cano_center": center, "face_id": face_id, "bary": bary}


def write_subject_dir(data_dir: str, maps: Dict[str, torch.Tensor]) -> None:
    """``<data_dir>/smpl_pos_map/{cano_smpl_pos_map.exr, cano_smpl_nml_map.exr, init_pts_lbs.npy}`` as ``gen_pos_maps.py:113,124,134``
    writes them: what ``AvatarNet.from_data_dir`` and the reference's own constructor read."""
    from . import exr
    d = os.path.join(data_dir, "smpl_pos_map")
    os.makedirs(d, exist_ok=True)
    exr.imwrite(os.path.join(d, "cano_smpl_pos_map.exr"), maps["cano_smpl_pos_map"].detach().cpu().numpy().astype(np.float32))
    exr.imwrite(os.path.join(d, "cano_smpl_nml_map.exr"), maps["cano_smpl_nml_map"].detach().cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "init_pts_lbs.npy"), maps["init_pts_lbs"].detach().cpu().numpy().astype(np.float32))
