"""The canonical blend-weight volume of a clothed-template subject, sampled on the GPU (``include/ag_weight_volume.h``).

Re-host of the reference's ``CanoBlendWeightVolume`` (``network/volume.py:42-93,116-130``): ``<data_dir>/cano_weight_volume.npz`` holds the
SMPL-X skinning weights diffused into a [X, Y, Z, J] grid around the body (``gen_data/gen_weight_volume.py``), and the per-point
weights of a template's canonical points are trilinear samples of it (``gen_pos_maps.py:128-130``).  The reference transposes the
arrays to [1, J, X, Y, Z] for ``F.grid_sample``; here they stay channel-last as the file stores them, which is the layout the kernel
reads (one grid node = one contiguous row) and needs no second copy of a 461 MB volume.

The Poisson-DIFFUSED volume is an input: it needs the reference's external solver and is out of scope.  What a closest-point query
gives is built here (``WeightVolume.from_body_mesh``, ``include/ag_mesh_query.h``): the bounds, ``center``, the nearest-surface
``ori_weight_volume`` and ``sdf_volume`` of ``gen_data/gen_weight_volume.py:136-170``, with the nearest-surface weights standing in for
the diffused ones; ``WeightVolume.save`` writes the reference's file.
No gradient with respect to ``pts`` (nor the volume): the outputs never require grad.  The reference differentiates ``forward_weight``
only when it trains a template network, which this package does not do.  ``forward_weight_grad`` is omitted: the reference's own
``base_gradient_volume`` it reads is commented out (``volume.py:70``).

Every tensor must be on the GPU; there is no host path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib


def _volume(t, name: str, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.to(device=device, dtype=torch.float32)
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (there is no host path)")
    if t.dim() == 3:
        t = t[..., None]                                                           # volume.py:59-60 (a 3-D sdf_volume)
    if t.dim() != 4 or min(t.shape[:3]) < 2 or t.shape[3] < 1:
        raise ValueError(f"{name} must be [X, Y, Z, C] with X, Y, Z >= 2 and C >= 1, got {tuple(t.shape)}")
    return t.contiguous()


def body_bounds(min_xyz: np.ndarray, max_xyz: np.ndarray):
    """(volume_bounds [2, 3], center [3], smpl_bounds [2, 3]) from the body's bounding box, the expressions of
    ``gen_weight_volume.py:136-150``: a cube of 1.1 x the longest extent about the box's centre, and the box grown by 5 / 5 / 15 cm."""
    min_xyz = np.array(min_xyz).astype(np.float32)
    max_xyz = np.array(max_xyz).astype(np.float32)
    max_len = 1.1 * (max_xyz - min_xyz).max()
    center = 0.5 * (min_xyz + max_xyz)
    volume_bounds = np.stack([center - 0.5 * max_len, center + 0.5 * max_len], 0)
    min_xyz[:2] -= 0.05
    max_xyz[:2] += 0.05
    min_xyz[2] -= 0.15
    max_xyz[2] += 0.15
    smpl_bounds = np.stack([min_xyz, max_xyz], 0)
    return volume_bounds.astype(np.float32), center.astype(np.float32), smpl_bounds.astype(np.float32)


def grid_axes(volume_bounds: np.ndarray, res):
    """The three node axes ``float32(np.linspace(lo_k, hi_k, res_k))`` (``gen_weight_volume.py:88-90``, rounded to the float32 the
    device computes in)."""
    return [np.float32(np.linspace(volume_bounds[0, k], volume_bounds[1, k], res[k])) for k in range(3)]


class WeightVolume:
    """``diff_weight_volume`` / ``ori_weight_volume`` [X, Y, Z, J], optional ``sdf_volume`` [X, Y, Z] or [X, Y, Z, 1], ``volume_bounds``
    [2, 3] (lo, hi), ``center`` [3] (of the SMPL-X body: ``gen_weight_volume.py:139``), ``smpl_bounds`` [2, 3]; arrays or tensors.
    ``device`` defaults to the device of ``diff_weight_volume``.  ``diffused``: whether ``diff_weight_volume`` holds Poisson-diffused
    weights (a loaded file) or is the nearest-surface ``ori_weight_volume`` itself (``from_body_mesh``)."""

    diffused = True

    def __init__(self, diff_weight_volume, ori_weight_volume, volume_bounds, center, smpl_bounds, sdf_volume=None, device=None):
        if device is None:
            device = diff_weight_volume.device if isinstance(diff_weight_volume, torch.Tensor) else "cuda"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"a WeightVolume must be on the GPU (there is no host path), got device {dev}")
        self.diff_weight_volume = _volume(diff_weight_volume, "diff_weight_volume", dev)
        self.ori_weight_volume = _volume(ori_weight_volume, "ori_weight_volume", dev)
        if self.ori_weight_volume.shape != self.diff_weight_volume.shape:
            raise ValueError("ori_weight_volume and diff_weight_volume must have one shape")
        self.res_x, self.res_y, self.res_z, self.joint_num = (int(s) for s in self.diff_weight_volume.shape)
        self.smpl_sdf_volume = None
        if sdf_volume is not None:
            self.smpl_sdf_volume = _volume(sdf_volume, "sdf_volume", dev)
        small = lambda a, shape, name: self._small(a, shape, name, dev)  # noqa: E731
        self.volume_bounds = small(volume_bounds, (2, 3), "volume_bounds")
        self.center = small(center, (3,), "center")
        self.smpl_bounds = small(smpl_bounds, (2, 3), "smpl_bounds")
        self._bounds_host = (ctypes.c_float * 6)(*self.volume_bounds.reshape(-1).cpu().tolist())
        volume_len = self.volume_bounds[1] - self.volume_bounds[0]
        self.voxel_size = volume_len / torch.tensor([self.res_x - 1, self.res_y - 1, self.res_z - 1]).to(volume_len)      # volume.py:68-69

    @staticmethod
    def _small(a, shape, name, dev):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        return t.to(device=dev, dtype=torch.float32).contiguous()

    @classmethod
    def load(cls, path: str, device="cuda") -> "WeightVolume":
        """Read ``cano_weight_volume.npz`` as ``gen_weight_volume.py:164-170`` writes it (``volume.py:43-69``)."""
        if torch.device(device).type != "cuda":
            raise ValueError(f"a WeightVolume must be on the GPU (there is no host path), got device {device}")
        with np.load(path) as data:
            return cls(data["diff_weight_volume"], data["ori_weight_volume"], data["volume_bounds"], data["center"], data["smpl_bounds"],
                       sdf_volume=data["sdf_volume"] if "sdf_volume" in data else None, device=device)

    @classmethod
    def from_body_mesh(cls, vertices: torch.Tensor, faces: torch.Tensor, lbs_weights: torch.Tensor, res=128) -> "WeightVolume":
        """The volume of a body mesh (the canonical SMPL-X: ``vertices`` [V, 3], ``faces`` [F, 3], ``lbs_weights`` [V, J], on the GPU)
        without the Poisson solver: ``gen_weight_volume.py:136-170`` minus ``diff_weights``.  Bounds, ``center`` and ``smpl_bounds``
        are the reference's numpy expressions on the host; the grid axes are ``float32(np.linspace(lo_k, hi_k, res_k))``, uploaded as
        they are and read by the kernel (node (i, j, k) = (x_i, y_j, z_k), arrays [X, Y, Z, ...]); ``ori_weight_volume`` holds the
        weights interpolated at each node's closest point of the mesh, ``sdf_volume`` the signed distance, positive inside (:167;
        ``mesh_query``: pseudonormal sign, exact for a closed, consistently wound mesh).  ``res``: an int or (X, Y, Z).

        ``diff_weight_volume`` IS ``ori_weight_volume`` (one tensor, 461 MB at 128^3 x 55, not two) and ``diffused`` is ``False``:
        these are NEAREST-SURFACE weights, discontinuous across the body's medial surface (between the legs, under the arms), where
        the reference's are Poisson-diffused and smooth.  Near the body surface, where a tight template lies, the two agree."""
        from . import mesh_query
        from .subject_maps import _dev, resolve
        v = _dev(vertices, "vertices", torch.float32, 3)
        f = _dev(faces, "faces", torch.int32, 3)
        w = _dev(lbs_weights, "lbs_weights", torch.float32)
        if w.dim() != 2 or w.shape[0] != v.shape[0] or v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError("from_body_mesh needs a non-empty mesh and lbs_weights [V, J] with one row per vertex")
        res = (int(res),) * 3 if np.isscalar(res) else tuple(int(r) for r in res)
        if len(res) != 3 or min(res) < 2:
            raise ValueError(f"res must be an int or (X, Y, Z), each >= 2, got {res}")
        volume_bounds, center, smpl_bounds = body_bounds(v.amin(0).cpu().numpy(), v.amax(0).cpu().numpy())
        axes = grid_axes(volume_bounds, res)
        sdf, face_id, bary = mesh_query.grid_signed_distance([torch.from_numpy(a).to(v.device) for a in axes], v, f)
        ori = resolve(face_id, bary, f, w).view(res + (w.shape[1],))
        vol = cls(ori, ori, volume_bounds, center, smpl_bounds, sdf_volume=(-sdf).view(res), device=v.device)
        vol.diffused = False
        return vol

    def save(self, path: str, alias_diff: bool = True) -> None:
        """Write ``cano_weight_volume.npz`` with the key names, shapes and dtypes of ``gen_weight_volume.py:164-170`` (float32;
        ``sdf_volume`` [X, Y, Z]): what ``load`` and the reference's ``CanoBlendWeightVolume`` read.  ``alias_diff=False`` leaves
        ``diff_weight_volume`` out of the file of a volume that is not ``diffused``, for users who will add their own (the file
        cannot be loaded until they have)."""
        host = lambda t: t.detach().cpu().numpy().astype(np.float32)  # noqa: E731
        arrays = {"ori_weight_volume": host(self.ori_weight_volume), "volume_bounds": host(self.volume_bounds),
                  "smpl_bounds": host(self.smpl_bounds), "center": host(self.center)}
        if self.diffused or alias_diff:
            arrays["diff_weight_volume"] = arrays["ori_weight_volume"] if self.diff_weight_volume is self.ori_weight_volume \
                else host(self.diff_weight_volume)
        if self.smpl_sdf_volume is not None:
            arrays["sdf_volume"] = host(self.smpl_sdf_volume)[..., 0]
        np.savez(path, **arrays)

    def _sample(self, volume: torch.Tensor, pts: torch.Tensor, requires_scale: bool) -> torch.Tensor:
        if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
            raise ValueError("pts must be a tensor on the GPU (there is no host path)")
        if pts.device != volume.device:
            raise ValueError(f"pts is on {pts.device}, the volume on {volume.device}")
        if pts.dim() not in (2, 3) or pts.shape[-1] != 3:
            raise ValueError(f"pts must be [B, N, 3] or [N, 3], got {tuple(pts.shape)}")
        p = pts.detach().to(torch.float32).contiguous()
        X, Y, Z, C = volume.shape
        n = p.numel() // 3
        out = torch.empty(tuple(p.shape[:-1]) + (C,), dtype=torch.float32, device=p.device)
        with _lib.on_device(p.device):
            _lib.check(_lib.lib().ag_weight_volume_sample(ctypes.c_void_p(volume.data_ptr()), X, Y, Z, C, ctypes.c_void_p(p.data_ptr()), n,
                                                          self._bounds_host if requires_scale else None, ctypes.c_void_p(out.data_ptr()),
                                                          ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)),
                       "ag_weight_volume_sample")
        return out

    def forward_weight(self, pts: torch.Tensor, requires_scale: bool = True, volume_type: str = "diff") -> torch.Tensor:
        """``pts`` [B, N, 3] (or [N, 3]) -> [B, N, J] (or [N, J]).  ``requires_scale``: ``pts`` are world coordinates, scaled to [0, 1]
        by ``volume_bounds``; without, they already are in [0, 1].  ``volume_type``: ``'diff'`` (diffused) or anything else for the
        nearest-surface ``ori_weight_volume``, as in the reference.  Points outside the volume take the border's value."""
        return self._sample(self.diff_weight_volume if volume_type == "diff" else self.ori_weight_volume, pts, requires_scale)

    def forward_sdf(self, pts: torch.Tensor, requires_scale: bool = True) -> torch.Tensor:
        """``pts`` [B, N, 3] (or [N, 3]) -> the SMPL-X signed distance [B, N, 1] (or [N, 1]); positive inside (``gen_weight_volume.py:167``)."""
        if self.smpl_sdf_volume is None:
            raise ValueError("this WeightVolume was built without an sdf_volume")
        return self._sample(self.smpl_sdf_volume, pts, requires_scale)
