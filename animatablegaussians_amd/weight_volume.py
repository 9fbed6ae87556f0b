"""The canonical blend-weight volume of a clothed-template subject, sampled on the GPU (``include/ag_weight_volume.h``).

Re-host of the reference's ``CanoBlendWeightVolume`` (``network/volume.py:42-93,116-130``): ``<data_dir>/cano_weight_volume.npz`` holds the
SMPL-X skinning weights diffused into a [X, Y, Z, J] grid around the body (``gen_data/gen_weight_volume.py``), and the per-point
weights of a template's canonical points are trilinear samples of it (``gen_pos_maps.py:128-130``).  The reference transposes the
arrays to [1, J, X, Y, Z] for ``F.grid_sample``; here they stay channel-last as the file stores them, which is the layout the kernel
reads (one grid node = one contiguous row) and needs no second copy of a 461 MB volume.

Everything in the file can be built here.  ``WeightVolume.from_body_mesh`` (``include/ag_mesh_query.h``) gives what a closest-point
query gives: the bounds, ``center``, the nearest-surface ``ori_weight_volume`` and ``sdf_volume`` of
``gen_data/gen_weight_volume.py:136-170``.  ``WeightVolume.diffuse`` (``include/ag_weight_diffuse.h``) then extends the weights near the
body surface smoothly into the whole grid, which is what ``diff_weight_volume`` is for; ``WeightVolume.save`` writes the reference's
file: ``WeightVolume.from_body_mesh(v, f, w).diffuse().save(path)``.  The reference produces its ``diff_weight_volume`` with an external
program (PointInterpolant: values and gradients fitted with B-splines on an adaptive octree).  ``diffuse`` is NOT that program and
claims no equality with its output: it is the discrete harmonic extension defined by ``diffuse_weights`` below.
The way back, posed point -> canonical point, reads the volume at its NEAREST node together with its Sobel gradient
(``WeightVolume.gradient_volume``, ``WeightVolume.root_find``; ``include/ag_inverse_skinning.h``, ``inverse_skinning.py``).
``WeightVolume.isosurface`` turns the SDF back into a mesh (``isosurface.py``, ``include/ag_isosurface.h``).
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


def stencil_weights(spacing) -> np.ndarray:
    """``w_k = (h_min / h_k)^2`` as float32 [3]: 1 on a cubic grid, so the problem does not depend on the grid's scale."""
    h = np.asarray([float(x) for x in spacing], np.float64)
    if h.shape != (3,) or not (np.isfinite(h).all() and (h > 0).all()):
        raise ValueError(f"spacing must be three positive node spacings, got {spacing}")
    return ((h.min() / h) ** 2).astype(np.float32)


def _diffuse_args(target, fixed):
    if not (isinstance(target, torch.Tensor) and isinstance(fixed, torch.Tensor) and target.is_cuda and fixed.is_cuda):
        raise ValueError("target and fixed must be tensors on the GPU (there is no host path)")
    if target.device != fixed.device:
        raise ValueError(f"target is on {target.device}, fixed on {fixed.device}")
    if target.dim() != 4 or min(target.shape[:3]) < 2 or target.shape[3] < 1:
        raise ValueError(f"target must be [X, Y, Z, J] with X, Y, Z >= 2 and J >= 1, got {tuple(target.shape)}")
    if fixed.dtype != torch.bool or tuple(fixed.shape) != tuple(target.shape[:3]):
        raise ValueError(f"fixed must be a bool mask of shape {tuple(target.shape[:3])}, got {fixed.dtype} {tuple(fixed.shape)}")
    return target.detach().to(torch.float32).contiguous(), fixed.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def diffusion_operator(values: torch.Tensor, fixed: torch.Tensor, spacing) -> torch.Tensor:
    """``A values`` of ``include/ag_weight_diffuse.h``: at every node that is not ``fixed`` the weighted sum over the three axes of
    ``(u - u_lower) + (u - u_upper)`` (neighbours read as given, one outside the grid dropped), 0 on fixed nodes."""
    v, m = _diffuse_args(values, fixed)
    w = (ctypes.c_float * 3)(*stencil_weights(spacing).tolist())
    X, Y, Z, J = v.shape
    out = torch.empty_like(v)
    with _lib.on_device(v.device):
        _lib.check(_lib.lib().ag_weight_diffuse_apply(_ptr(v), _ptr(m), X, Y, Z, J, w, _ptr(out),
                                                      _lib.stream(v.device)), "ag_weight_diffuse_apply")
    return out


def diffuse_weights(target: torch.Tensor, fixed: torch.Tensor, spacing, *, tol: float = 1e-5, max_iter: Optional[int] = None,
                    check_every: int = 16):
    """The discrete harmonic extension of ``target`` [X, Y, Z, J] from the nodes of the bool mask ``fixed`` [X, Y, Z] into all the
    others (``include/ag_weight_diffuse.h``); ``spacing``: the three node spacings.  Returns ``(u, info)``:

    * ``u = target`` on fixed nodes, bit for bit;
    * at every other node, for every channel, ``sum_k w_k [(u - u_lower_k) + (u - u_upper_k)] = 0`` with ``w_k = (h_min / h_k)^2``
      and a neighbour outside the grid dropped (no flux through the cube's faces).

    So ``u`` stays within the range of the fixed values of its channel (maximum principle), rows that sum to 1 on the fixed nodes sum
    to 1 everywhere, and ``u`` is continuous where nearest-surface weights jump.  ``u`` is the raw solution: not clipped, not
    renormalised.  This is this project's definition; it is not the reference's external PointInterpolant fit and claims no
    equality with it.

    Solver: conjugate gradients on the free nodes, all channels in lockstep, each with its own scalars, so each is an exact CG of
    its own system; ``check_every`` iterations are enqueued at a time and the [J] residuals read in between.  It stops when every
    channel has ``|r_j| <= tol |b_j|``.  A channel whose fixed values are all zero stays exactly zero.
    ``max_iter`` defaults to ``20 * max(X, Y, Z)``: plain CG needed about 5.6 iterations per node along the longest edge on CPU
    trials of this problem at 16^3 to 64^3 (the count grows with the distance, in nodes, that the fixed values must travel), and 3.5 x
    that leaves room for an anisotropic grid or a thin band without letting a stalled solve run on.

    ``info``: ``iterations``, ``rel_residual`` [J] (the recurrence's ``|r_j| / |b_j|``, 0 where ``b_j = 0``), ``true_rel_residual`` [J]
    (``|A u|_j / |b_j|`` from one more application of the operator to the returned ``u``), ``converged``.
    No fixed node: ``ValueError`` (the extension is undefined).  All nodes fixed: ``target`` itself, 0 iterations."""
    t, m = _diffuse_args(target, fixed)
    w_host = stencil_weights(spacing)
    if not (tol > 0) or int(check_every) < 1:
        raise ValueError(f"tol must be positive and check_every at least 1, got {tol}, {check_every}")
    X, Y, Z, J = t.shape
    n_fixed = int(m.sum())
    if n_fixed == 0:
        raise ValueError("no fixed node: the harmonic extension is undefined")
    zeros = torch.zeros(J, dtype=torch.float64)
    if n_fixed == m.numel():
        return target, {"iterations": 0, "rel_residual": zeros, "true_rel_residual": zeros.clone(), "converged": True}
    if max_iter is None:
        max_iter = 20 * max(X, Y, Z)
    max_iter, check_every = int(max_iter), int(check_every)
    L = _lib.lib()
    w = (ctypes.c_float * 3)(*w_host.tolist())
    dev = t.device
    x, r, p, ap = (torch.empty_like(t) for _ in range(4))
    n_ws = int(L.ag_weight_diffuse_workspace_bytes(X, Y, Z, J))
    if n_ws == 0:
        raise ValueError(f"a grid of {X} x {Y} x {Z} nodes is outside what ag_weight_diffuse takes (fewer than 2^31 nodes)")
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    bb = torch.empty(J, dtype=torch.float32, device=dev)
    rr = torch.empty(J, dtype=torch.float32, device=dev)

    def rel(num, den):
        num, den = num.double().cpu(), den.double().cpu()
        return torch.where(den > 0, (num / den.clamp_min(1e-300)).sqrt(), num.sqrt())

    with _lib.on_device(dev):
        stream = _lib.stream(dev)
        _lib.check(L.ag_weight_diffuse_init(_ptr(t), _ptr(m), X, Y, Z, J, w, _ptr(x), _ptr(r), _ptr(p), _ptr(ap), _ptr(ws), n_ws, _ptr(bb), _ptr(rr),
                                            stream), "ag_weight_diffuse_init")
        bb_host = bb.double().cpu()
        iterations = 0
        while True:
            rr_host = rr.double().cpu()
            converged = bool((rr_host <= (tol * tol) * bb_host).all())
            if converged or iterations >= max_iter:
                break
            n = min(check_every, max_iter - iterations)
            _lib.check(L.ag_weight_diffuse_iterate(_ptr(m), X, Y, Z, J, w, n, _ptr(x), _ptr(r), _ptr(p), _ptr(ap), _ptr(ws), n_ws, _ptr(rr), stream),
                       "ag_weight_diffuse_iterate")
            iterations += n
        u = torch.where(m[..., None], t, x)
        _lib.check(L.ag_weight_diffuse_apply(_ptr(u), _ptr(m), X, Y, Z, J, w, _ptr(ap), stream), "ag_weight_diffuse_apply")
        true_sq = ap.double().square().sum((0, 1, 2))
    info = {"iterations": iterations, "rel_residual": rel(rr, bb), "true_rel_residual": rel(true_sq, bb), "converged": converged}
    return u, info


class WeightVolume:
    """``diff_weight_volume`` / ``ori_weight_volume`` [X, Y, Z, J], optional ``sdf_volume`` [X, Y, Z] or [X, Y, Z, 1], ``volume_bounds``
    [2, 3] (lo, hi), ``center`` [3] (of the SMPL-X body: ``gen_weight_volume.py:139``), ``smpl_bounds`` [2, 3]; arrays or tensors.
    ``device`` defaults to the device of ``diff_weight_volume``.  ``diffused``: whether ``diff_weight_volume`` holds diffused weights
    (a loaded file, or the result of ``diffuse``) or is the nearest-surface ``ori_weight_volume`` itself (``from_body_mesh``).
    ``diffusion``: what ``diffuse`` recorded of its solve (``None`` otherwise)."""

    diffused = True
    diffusion = None

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
        before diffusion: ``gen_weight_volume.py:136-170`` minus ``diff_weights``.  Bounds, ``center`` and ``smpl_bounds``
        are the reference's numpy expressions on the host; the grid axes are ``float32(np.linspace(lo_k, hi_k, res_k))``, uploaded as
        they are and read by the kernel (node (i, j, k) = (x_i, y_j, z_k), arrays [X, Y, Z, ...]); ``ori_weight_volume`` holds the
        weights interpolated at each node's closest point of the mesh, ``sdf_volume`` the signed distance, positive inside (:167;
        ``mesh_query``: pseudonormal sign, exact for a closed, consistently wound mesh).  ``res``: an int or (X, Y, Z).

        ``diff_weight_volume`` IS ``ori_weight_volume`` (one tensor, 461 MB at 128^3 x 55, not two) and ``diffused`` is ``False``:
        these are NEAREST-SURFACE weights, discontinuous across the body's medial surface (between the legs, under the arms), where
        diffused ones are smooth.  Near the body surface, where a tight template lies, the two agree; for a skirt, a coat hem or a
        loose sleeve call ``diffuse()`` on the result."""
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

    def diffuse(self, band: Optional[float] = None, *, tol: float = 1e-5, max_iter: Optional[int] = None) -> "WeightVolume":
        """A NEW volume whose ``diff_weight_volume`` is ``ori_weight_volume`` diffused from the body surface into the whole grid
        (``diffuse_weights``); ``ori_weight_volume``, the SDF and the bounds are shared with this one, ``diffused`` is ``True`` and
        ``diffusion`` holds the solve's ``info`` and the ``band`` used.

        Fixed nodes: ``|sdf_volume| <= band``, where the nearest-surface weights are the right ones.  ``band`` is in the units of the
        bounds (metres) and defaults to 1.5 x the largest node spacing, which keeps at least one layer of nodes on either side of the
        surface wherever it passes -- a choice of this project, not a value of the reference.  The solution is clipped to [0, 1] and
        each row divided by its sum (``gen_weight_volume.py:131-132``); a row that sums to 0 stays 0.
        ``RuntimeError`` if the solve does not reach ``tol`` within ``max_iter`` iterations."""
        if self.smpl_sdf_volume is None:
            raise ValueError("diffuse needs the sdf_volume: it says which nodes lie near the body surface")
        spacing = [float(h) for h in self.voxel_size.cpu()]
        if band is None:
            band = 1.5 * max(spacing)
        band = float(band)
        fixed = (self.smpl_sdf_volume[..., 0].abs() <= band).contiguous()
        u, info = diffuse_weights(self.ori_weight_volume, fixed, spacing, tol=tol, max_iter=max_iter)
        if not info["converged"]:
            raise RuntimeError(f"the diffusion did not reach tol = {tol} in {info['iterations']} iterations "
                               f"(worst relative residual {float(info['rel_residual'].max()):.3e}); raise max_iter")
        u = u.clamp(0.0, 1.0)
        total = u.sum(-1, keepdim=True)
        u = torch.where(total > 0, u / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(u))
        vol = WeightVolume(u, self.ori_weight_volume, self.volume_bounds, self.center, self.smpl_bounds, sdf_volume=self.smpl_sdf_volume,
                           device=u.device)
        vol.diffused = True
        vol.diffusion = dict(info, band=band, fixed_nodes=int(fixed.sum()))
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
                                                          _lib.stream(p.device)),
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

    def isosurface(self, level: float = 0.0):
        """``(vertices [V, 3], faces [F, 3] int32)`` of the surface ``smpl_sdf_volume == level`` in world coordinates
        (``isosurface.marching_cubes``): node (i, j, k) sits at ``volume_bounds[0] + (i, j, k) * voxel_size``, at the grid NODES (no half
        voxel, unlike ``isosurface.recon_mesh``).  Faces are wound counter-clockwise seen from outside the body."""
        if self.smpl_sdf_volume is None:
            raise ValueError("this WeightVolume was built without an sdf_volume")
        from . import isosurface
        return isosurface.marching_cubes(self.smpl_sdf_volume[..., 0], level, spacing=self.voxel_size, origin=self.volume_bounds[0])

    def _which(self, volume_type: str) -> torch.Tensor:
        return self.diff_weight_volume if volume_type == "diff" else self.ori_weight_volume

    def _spacing_host(self):
        return (ctypes.c_float * 3)(*self.voxel_size.cpu().tolist())

    def gradient_volume(self, volume_type: str = "diff") -> torch.Tensor:
        """The Sobel gradient [X, Y, Z, J, 3] of the weight volume (``include/ag_inverse_skinning.h``; the reference's
        ``compute_gradient_volume``, ``network/volume.py:9-39``, in its [X, Y, Z, J * 3] layout): 1.38 GB at 128^3 x 55.  ``root_find``
        does not need it; pass it as ``grad_volume`` to read the rows instead of forming them on the fly (identical bits)."""
        vol = self._which(volume_type)
        X, Y, Z, J = vol.shape
        out = torch.empty((X, Y, Z, J, 3), dtype=torch.float32, device=vol.device)
        with _lib.on_device(vol.device):
            _lib.check(_lib.lib().ag_weight_volume_gradient(_ptr(vol), X, Y, Z, J, self._spacing_host(), _ptr(out),
                                                            _lib.stream(vol.device)),
                       "ag_weight_volume_gradient")
        return out

    def root_find(self, posed_pts: torch.Tensor, cano_init: torch.Tensor, jnt_mats: torch.Tensor, *, active: Optional[torch.Tensor] = None,
                  lam: float = 0.1, iterations: int = 10, volume_type: str = "diff", grad_volume: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Canonical points ``xc`` with ``sum_j w_j(xc) (A_j xc) = posed_pts``: ``iterations`` damped Newton steps from ``cano_init``
        through the weights at the NEAREST node of the volume and their Sobel gradient (``include/ag_inverse_skinning.h``; the
        reference's ``root_finding.cu``).  ``posed_pts``, ``cano_init`` [B, N, 3] (or [N, 3] with ``jnt_mats`` [J, 4, 4] or [1, J, 4, 4]),
        ``jnt_mats`` [B, J, 4, 4] canonical -> posed, each batch its own; ``active`` [B, N] bool: points with ``False`` come back as
        ``cano_init``.  Each step is clamped to 1 cm per axis, so the result lies within ``iterations`` cm of ``cano_init``.
        No gradient: the reference runs this step under ``no_grad``."""
        from . import inverse_skinning
        return inverse_skinning._root_find(self, posed_pts, cano_init, jnt_mats, active, lam, iterations, volume_type, grad_volume)
