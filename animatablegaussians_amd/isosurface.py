"""Iso-surface extraction on the GPU: a scalar volume on a regular grid -> triangle mesh (``include/ag_isosurface.h``).

Re-host of what the reference's ``utils/recon_util.recon_mesh`` (``recon_util.py:51-75``) asks of ``skimage.measure.marching_cubes`` on
the host: the step that turns the template stage's SDF grid into ``template.ply`` (``main_template.py:103-133``).  The mesh is defined
by this project (``include/ag_isosurface.h``), not by skimage, which is installed nowhere this project is built:

* a node is inside iff ``value >= iso`` (the reference's SDFs and occupancies are larger inside);
* the case table is generated from a rule that reads each cube face on its own (``csrc/gen_isosurface_table.py``), so the mesh is
  watertight, and an ambiguous face joins its inside corners (thin inside parts stay connected);
* a cell is processed iff its eight values are finite and, with a ``mask``, its eight mask entries are non-zero;
* faces are wound counter-clockwise seen from outside (the side of lower values), this package's convention
  (``synth._lattice_surface``, ``mesh_query.signed_distance``): the signed volume of a sphere SDF's surface is positive;
* vertices and faces come in a fixed order (grid edge key, cell index), bit-identical between calls; triangles of zero area, which
  appear where a node's value equals ``iso``, are kept.

Every tensor must be on the GPU; there is no host path.  The host waits for the device twice per call, both times for a few bytes:
the read of the two counts, and ``ag_isosurface_emit``'s own check that the buffers it is given were allocated for them.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _three(x, name: str):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    vals = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
    if len(vals) != 3:
        raise ValueError(f"{name} must have three components, got {x}")
    return vals


def marching_cubes(volume: torch.Tensor, iso: float = 0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
                   mask: Optional[torch.Tensor] = None):
    """``volume`` [X, Y, Z] float32 on the GPU -> ``(vertices [V, 3] float32, faces [F, 3] int32)`` on the same device: the surface
    ``volume == iso`` as defined in ``include/ag_isosurface.h``.  Node (i, j, k) sits at ``origin + (i, j, k) * spacing``.  ``mask``
    [X, Y, Z] bool or uint8: cells that touch a zero entry are skipped.  An empty surface returns shapes ``(0, 3)``."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise ValueError("volume must be a tensor on the GPU (there is no host path)")
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise ValueError(f"volume must be a float32 tensor [X, Y, Z], got {volume.dtype} {tuple(volume.shape)}")
    X, Y, Z = (int(s) for s in volume.shape)
    if min(X, Y, Z) < 2 or 3 * X * Y * Z >= 2 ** 31:
        raise ValueError(f"volume must have X, Y, Z >= 2 and 3 * X * Y * Z < 2^31, got {(X, Y, Z)}")
    vol = volume.detach().contiguous()
    m = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != vol.device:
            raise ValueError("mask must be a tensor on the volume's device")
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (X, Y, Z):
            raise ValueError(f"mask must be bool or uint8 of shape {(X, Y, Z)}, got {mask.dtype} {tuple(mask.shape)}")
        m = mask.contiguous()
    iso = float(iso)
    sp, org = _three(spacing, "spacing"), _three(origin, "origin")
    if not (np.isfinite(iso) and np.isfinite(sp).all() and np.isfinite(org).all() and min(sp) > 0):
        raise ValueError(f"iso and origin must be finite and spacing finite and positive, got {iso}, {sp}, {org}")
    L = _lib.lib()
    dev = vol.device
    n_ws = int(L.ag_isosurface_workspace_bytes(X, Y, Z))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    c_sp, c_org = (ctypes.c_float * 3)(*sp), (ctypes.c_float * 3)(*org)
    with _lib.on_device(dev):
        stream = _lib.stream(dev)
        _lib.check(L.ag_isosurface_count(_ptr(vol), _ptr(m), X, Y, Z, iso, _ptr(ws), n_ws, _ptr(counts), stream), "ag_isosurface_count")
        V, F = (int(c) for c in counts.cpu())
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        _lib.check(L.ag_isosurface_emit(_ptr(vol), X, Y, Z, iso, c_sp, c_org, _ptr(ws), n_ws, _ptr(vertices) if V else None, V,
                                        _ptr(faces) if F else None, F, stream), "ag_isosurface_emit")
    return vertices, faces


def volume_normals(volume: torch.Tensor, voxel_size, grid_pts: torch.Tensor) -> torch.Tensor:
    """The reference's ``extract_normal_from_volume`` (``recon_util.py:9-48``): the 3x3x3 Sobel gradient of ``volume`` [X, Y, Z] with
    zero padding (``ag_weight_volume_gradient`` with one channel), sampled trilinearly with border clamp at ``grid_pts`` [N, 3] in
    [0, 1]^3 (``ag_weight_volume_sample``; 0 and 1 are the first and last NODE) and divided by its norm.  Not negated."""
    X, Y, Z = (int(s) for s in volume.shape)
    L = _lib.lib()
    dev = volume.device
    grad = torch.empty((X, Y, Z, 3), dtype=torch.float32, device=dev)
    pts = grid_pts.to(torch.float32).contiguous()
    out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        stream = _lib.stream(dev)
        _lib.check(L.ag_weight_volume_gradient(_ptr(volume), X, Y, Z, 1, (ctypes.c_float * 3)(*_three(voxel_size, "voxel_size")), _ptr(grad), stream),
                   "ag_weight_volume_gradient")
        if pts.shape[0]:
            _lib.check(L.ag_weight_volume_sample(_ptr(grad), X, Y, Z, 3, _ptr(pts), pts.shape[0], None, _ptr(out), stream), "ag_weight_volume_sample")
    return out / out.norm(dim=1, keepdim=True)


def recon_mesh(occ_volume: torch.Tensor, volume_res, bounds, volume_mask: Optional[torch.Tensor] = None, iso_value: float = 0.5):
    """The reference's ``recon_mesh`` (``recon_util.py:51-75``) on the device: ``occ_volume`` (any shape with ``prod(volume_res)``
    float32 elements, on the GPU), ``bounds`` [2, 3] -> ``(vertices [V, 3], faces [F, 3] int32, normals [V, 3])``, tensors on the device
    (``obj_io.save_mesh_ply`` takes their ``.cpu()``).  ``iso_value``: 0.5 for an occupancy, 0 for an SDF.

    Conventions, the reference's:

    * ``voxel_size = (bounds[1] - bounds[0]) / volume_res`` -- divided by ``res``, not ``res - 1``;
    * HALF-VOXEL convention: node (i, j, k) sits at the CENTRE of voxel (i, j, k), ``bounds[0] + ((i, j, k) + 0.5) * voxel_size``; a vertex is
      ``idx * voxel_size + bounds[0] + 0.5 * voxel_size`` in that order of operations, ``idx`` its fractional grid index;
    * normals: the Sobel gradient of the volume (zero padding), sampled trilinearly with border clamp at ``(v - bounds[0]) / len``
      taken as [0, 1] between the first and last node (the reference's ``grid_sample`` with ``align_corners``; the half voxel is NOT
      undone there either), divided by its norm and negated: they point towards lower values, out of the surface.

    WINDING: the reference reverses skimage's faces (``faces[:, [2, 1, 0]]``).  skimage's own winding could not be checked, so the
    contract here is the outcome: faces wound counter-clockwise seen from outside, agreeing with the returned normals (every face's
    geometric normal has a positive dot product with its vertices' normals).  ``marching_cubes`` already winds them so; nothing is
    reversed."""
    res = tuple(int(r) for r in volume_res)
    if len(res) != 3:
        raise ValueError(f"volume_res must be (X, Y, Z), got {volume_res}")
    if not isinstance(occ_volume, torch.Tensor) or not occ_volume.is_cuda:
        raise ValueError("occ_volume must be a tensor on the GPU (there is no host path)")
    if occ_volume.dtype != torch.float32 or occ_volume.numel() != res[0] * res[1] * res[2]:
        raise ValueError(f"occ_volume must hold {res[0]} * {res[1]} * {res[2]} float32 values, got {occ_volume.dtype} {tuple(occ_volume.shape)}")
    vol = occ_volume.detach().reshape(res).contiguous()
    if volume_mask is not None:
        if not isinstance(volume_mask, torch.Tensor) or volume_mask.numel() != vol.numel():
            raise ValueError(f"volume_mask must be a tensor of {vol.numel()} elements")
        volume_mask = volume_mask.reshape(res)
    b = bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else np.asarray(bounds)
    b = b.astype(np.float32)
    if b.shape != (2, 3):
        raise ValueError(f"bounds must be [2, 3], got {b.shape}")
    volume_len = b[1] - b[0]
    voxel_size = volume_len / np.array(res, dtype=np.float32)
    idx, faces = marching_cubes(vol, iso_value, spacing=voxel_size, origin=(0.0, 0.0, 0.0), mask=volume_mask)       # idx * voxel_size, as skimage's spacing
    lo, vs, ln = (torch.from_numpy(a).to(vol.device) for a in (b[0], voxel_size, volume_len))
    vertices = idx + lo + 0.5 * vs
    normals = -volume_normals(vol, voxel_size, (vertices - lo) / ln)
    return vertices, faces, normals
