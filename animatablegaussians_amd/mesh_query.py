"""Closest point on a triangle mesh and the signed distance to it, on the GPU (``include/ag_mesh_query.h``).

The nearest-face search the reference takes from pytorch3d (``utils/posevocab_custom_ops/nearest_face.py:30-61``, behind
``interpolate_lbs`` of ``gen_data/gen_pos_maps.py:24-39`` and ``calc_blending_weight(method='barycentric')`` of
``utils/smpl_util.py:46-53``) and the signed distance it takes from libigl (``gen_data/gen_weight_volume.py:155``): for points that do not
come out of this package's rasterizer -- scan points, a template's vertices, Gaussians read from a PLY, the nodes of a weight volume.

    closest_point  ->  (dist2, face_id, bary)  ->  subject_maps.resolve(face_id, bary, faces, attribute)   (interpolated attributes)
                                               ->  pseudonormal sign                                         (signed_distance)

Exact brute force over all faces; ties between faces go to the lower face index, so the result is a pure function of the inputs.
The sign is the angle-weighted pseudonormal test (Baerentzen & Aanaes 2005): exact for closed, consistently wound manifold meshes;
with several intersecting components (SMPL-X's eyeballs) it is the sign with respect to the closest face's component, where libigl's
default is the same test on the same closest face.  NOT pinned: neither pytorch3d nor libigl is available to this package, so parity
with their tie-breaking and roundings is not claimed; the contract is ``tests/mesh_query_oracle.py`` in float64.

Every tensor must be on the GPU; there is no host path and no autograd (outputs never require grad).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .subject_maps import _dev, _p, _stream, resolve, vertex_normals

FACE_TILE = 256                    # AG_MESH_QUERY_FACE_TILE: faces per LDS tile of the tiled walk
WALKS = {"default": 0, "uniform": 1, "tiled": 2}


def _run(points: Optional[torch.Tensor], axes, vertices: torch.Tensor, faces: torch.Tensor, walk: str = "default"):
    """-> (dist2 [N], face_id [N] int32, bary [N, 3], feature [N] int32, the filled argument struct and what it points to)."""
    v = _dev(vertices, "vertices", torch.float32, 3)
    f = _dev(faces, "faces", torch.int32, 3)
    if walk not in WALKS:
        raise ValueError(f"walk must be one of {sorted(WALKS)}, got {walk!r}")
    a = _lib.AgMeshQueryArgs()
    if axes is None:
        p = _dev(points, "points", torch.float32, 3).detach()
        if p.device != v.device:
            raise ValueError(f"points are on {p.device}, the mesh on {v.device}")
        N = p.shape[0]
        a.points = _p(p)
        keep = (p,)
    else:
        keep = tuple(_dev(x, "axis", torch.float32).reshape(-1) for x in axes)
        if len(keep) != 3 or any(x.device != v.device or x.numel() < 1 for x in keep):
            raise ValueError("axes must be three non-empty 1-D tensors on the mesh's GPU")
        a.gx, a.gy, a.gz = (int(x.numel()) for x in keep)
        N = a.gx * a.gy * a.gz
        a.axis_x, a.axis_y, a.axis_z = (_p(x) for x in keep)
    if N >= 2 ** 31:
        raise ValueError(f"{N} queries exceed one call")
    dev = v.device
    L = _lib.lib()
    dist2 = torch.empty(N, dtype=torch.float32, device=dev)
    face_id = torch.empty(N, dtype=torch.int32, device=dev)
    bary = torch.empty(N, 3, dtype=torch.float32, device=dev)
    feature = torch.empty(N, dtype=torch.int32, device=dev)
    ws = torch.empty(L.ag_mesh_closest_point_workspace_bytes(f.shape[0]), dtype=torch.uint8, device=dev)
    a.N, a.V, a.F, a.walk = N, v.shape[0], f.shape[0], WALKS[walk]
    a.vertices, a.faces = _p(v), _p(f)
    a.dist2, a.face_id, a.bary, a.feature = _p(dist2), _p(face_id), _p(bary), _p(feature)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    with _lib.on_device(dev):
        _lib.check(L.ag_mesh_closest_point(ctypes.byref(a), _stream(dev)), "ag_mesh_closest_point")
    return dist2, face_id, bary, feature, a, (v, f, ws) + keep


def closest_point(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, *, walk: str = "default",
                  return_feature: bool = False):
    """``points`` [N, 3], ``vertices`` [V, 3], ``faces`` [F, 3] -> (dist2 [N], face_id [N] int32, bary [N, 3]): the exact closest point
    of the closed triangles, ``b0 v0 + b1 v1 + b2 v2`` in the face's own corner order.  A face with an index outside [0, V) is
    skipped; without any face ``face_id = -1``, ``dist2 = inf``, ``bary = 0``.  ``return_feature`` adds the feature code [N] int32
    (0 face interior, 1-3 edge v0v1 / v1v2 / v2v0, 4-6 vertex).  ``walk``: how the kernel reads the face records (``'uniform'`` /
    ``'tiled'``; time only, the results are bit-identical).  Definition and fp32 operation order: ``include/ag_mesh_query.h``."""
    dist2, face_id, bary, feature = _run(points, None, vertices, faces, walk)[:4]
    return (dist2, face_id, bary, feature) if return_feature else (dist2, face_id, bary)


def pseudonormals(vertices: torch.Tensor, faces: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The three normal tables of the sign test, once per mesh: unit face normals [F, 3] (zero for a zero-area or skipped face), per
    edge the sum of the unit normals of all faces that share it [F, 3, 3] (edges v0v1, v1v2, v2v0; a border edge: its own face's
    normal), angle-weighted vertex normals [V, 3] (``subject_maps.vertex_normals``).  Sorted segment sums, no atomic scatter: the
    same on every run."""
    v = _dev(vertices, "vertices", torch.float32, 3)
    f = _dev(faces, "faces", torch.int64, 3)
    V, F = v.shape[0], f.shape[0]
    if F == 0 or V == 0:
        return v.new_zeros(F, 3), v.new_zeros(F, 3, 3), v.new_zeros(V, 3)
    valid = ((f >= 0) & (f < V)).all(1)
    fc = f.clamp(0, V - 1)
    p = v[fc]
    fn = torch.nn.functional.normalize(torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), dim=-1) * valid[:, None]
    a, b = fc, torch.roll(fc, -1, 1)                                            # edge k runs from corner k to corner k + 1
    key = (torch.minimum(a, b) * V + torch.maximum(a, b)).reshape(-1)          # [3F], undirected
    key = torch.where(valid[:, None].expand(-1, 3).reshape(-1), key, torch.full_like(key, V * V) + torch.arange(3 * F, device=v.device))
    order = torch.sort(key, stable=True)[1]
    sk = key[order]
    uniq, inverse = torch.unique_consecutive(sk, return_inverse=True)
    first = torch.searchsorted(sk, uniq)
    slot = torch.arange(sk.numel(), device=v.device) - first[inverse]
    dense = torch.zeros(uniq.numel(), int(slot.max().item()) + 1, 3, device=v.device)
    dense[inverse, slot] = fn[:, None, :].expand(-1, 3, -1).reshape(-1, 3)[order]
    sums = dense.sum(1)
    en = torch.empty(3 * F, 3, device=v.device)
    en[order] = sums[inverse]
    vn = vertex_normals(v, f[valid].to(torch.int32)) if bool(valid.any()) else v.new_zeros(V, 3)
    return fn.contiguous(), en.reshape(F, 3, 3).contiguous(), vn.contiguous()


def _interpolate(face_id, bary, faces, attribute):
    """``subject_maps.resolve`` in dense mode; a mesh without faces (every ``face_id`` is -1) gives zeros, as empty pixels do."""
    if faces.shape[0] == 0:
        return attribute.new_zeros(tuple(face_id.shape) + (attribute.shape[1],), dtype=torch.float32)
    return resolve(face_id, bary, faces, attribute)


def _signed(points, axes, vertices, faces, walk="default"):
    """-> (sdf [N] negative inside, dist2, face_id, bary)."""
    dist2, face_id, bary, feature, a, keep = _run(points, axes, vertices, faces, walk)
    v, f = keep[0], keep[1]
    fn, en, vn = pseudonormals(v, f)
    sign = torch.empty_like(dist2)
    if dist2.numel():
        with _lib.on_device(v.device):
            _lib.check(_lib.lib().ag_mesh_pseudonormal_sign(ctypes.byref(a), _p(fn), _p(en), _p(vn), _p(sign), _stream(v.device)),
                       "ag_mesh_pseudonormal_sign")
    # sign 0 (a query on the surface, or a feature without a normal) counts as outside: sdf = +dist
    return torch.where(sign < 0, -torch.sqrt(dist2), torch.sqrt(dist2)), dist2, face_id, bary


def signed_distance(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor):
    """-> (sdf [N], face_id [N] int32, closest_pts [N, 3]) as ``igl.signed_distance(points, vertices, faces)`` returns them
    (``gen_weight_volume.py:155``): NEGATIVE inside a closed mesh wound counter-clockwise seen from outside.  The caveats of the
    pseudonormal sign are in the module docstring."""
    sdf, _, face_id, bary = _signed(points, None, vertices, faces)
    return sdf, face_id, _interpolate(face_id, bary, _dev(faces, "faces", torch.int32, 3), _dev(vertices, "vertices", torch.float32, 3))


def grid_signed_distance(axes, vertices: torch.Tensor, faces: torch.Tensor):
    """``signed_distance`` at the nodes (x_i, y_j, z_k) of a grid given by three 1-D axes, node ``(i * Y + j) * Z + k``; the
    coordinates are read from the axes as they are.  -> (sdf [X*Y*Z], face_id, bary [X*Y*Z, 3])."""
    sdf, _, face_id, bary = _signed(None, axes, vertices, faces)
    return sdf, face_id, bary


def nearest_face_pytorch3d(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor):
    """``points`` [B, N, 3], ``vertices`` [B, M, 3], ``faces`` [F, 3] -> (dists = sqrt(dist2) [B, N], indices int64 [B, N],
    bc_coords [B, N, 3]): signature and returns of ``utils/posevocab_custom_ops/nearest_face.py:30-61``."""
    if not isinstance(points, torch.Tensor) or not isinstance(vertices, torch.Tensor) or points.dim() != 3 or vertices.dim() != 3 \
            or points.shape[0] != vertices.shape[0]:
        raise ValueError("points must be [B, N, 3] and vertices [B, M, 3]")
    dists, indices, bc = [], [], []
    for b in range(points.shape[0]):
        d2, fid, bary = closest_point(points[b], vertices[b], faces)
        dists.append(torch.sqrt(d2))
        indices.append(fid.to(torch.int64))
        bc.append(bary)
    return torch.stack(dists, 0), torch.stack(indices, 0), torch.stack(bc, 0)


def _gpu(x, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=t.device if t.is_cuda else "cuda", dtype=dtype)


def interpolate_lbs(pts, vertices, faces, vertex_lbs):
    """The skinning weights [N, J] of ``pts`` [N, 3]: those of the nearest point of the mesh, interpolated on its face
    (``gen_pos_maps.py:24-39``).  Arrays are uploaded (the reference's call takes numpy arrays); the search and the interpolation
    run on the GPU.  Returns a numpy array when ``pts`` is one, as the reference does, else a tensor on the GPU."""
    p, v = _gpu(pts, torch.float32), _gpu(vertices, torch.float32)
    f, w = _gpu(faces, torch.int32), _gpu(vertex_lbs, torch.float32)
    _, fid, bary = closest_point(p, v, f)
    lbs = _interpolate(fid, bary, f, w)
    return lbs if isinstance(pts, torch.Tensor) else lbs.cpu().numpy()


def calc_blending_weight(query_pts, smpl_v, smpl_f, smpl_lbs=None, near_thres: float = 0.08, method: str = "barycentric"):
    """``query_pts`` [B, N, 3], ``smpl_v`` [B, M, 3], ``smpl_f`` [B, F, 3], ``smpl_lbs`` [B, M, J] -> (pts_w [B, N, J], near_flag
    [B, N] bool = distance < ``near_thres``): ``utils/smpl_util.py:46-53``.  As there, the faces of batch 0 serve every batch.  The
    reference's ``'NN'`` method is pytorch3d's k-NN and not built; its global default for ``smpl_lbs`` does not exist here."""
    if method != "barycentric":
        raise NotImplementedError(f"calc_blending_weight: method {method!r} is not built (only 'barycentric')")
    if smpl_lbs is None:
        raise ValueError("calc_blending_weight: smpl_lbs [B, M, J] is required")
    if not (query_pts.shape[0] == smpl_v.shape[0] == smpl_f.shape[0] == smpl_lbs.shape[0]):
        raise ValueError("query_pts, smpl_v, smpl_f and smpl_lbs must have one batch size")
    dists, indices, bc = nearest_face_pytorch3d(query_pts, smpl_v, smpl_f[0])
    f = _dev(smpl_f[0], "smpl_f", torch.int32, 3)
    pts_w = torch.stack([_interpolate(indices[b].to(torch.int32), bc[b], f, _dev(smpl_lbs[b], "smpl_lbs", torch.float32))
                         for b in range(query_pts.shape[0])], 0)
    return pts_w, dists < near_thres
