"""Posed point -> canonical point through a subject's blend-weight volume (``include/ag_inverse_skinning.h``).

Re-host of the reference's ``TemplateNet.transform_live2cano`` / ``transform_cano2live`` (``network/template.py:209-286``) and of its
CUDA extension ``utils/root_finding``: the initial guess is the inverse of the joint matrices blended with the skinning weights at the
nearest point of the posed body mesh (``mesh_query.calc_blending_weight``), the refinement is ``iterations`` damped Newton steps on
``sum_j w_j(xc) (A_j xc) = xt`` through the nearest node of the ``WeightVolume`` and its Sobel gradient.  The template network that
calls these in the reference is not built; the functions take what it would have taken from its batch.

Differences from the reference, all stated in the header: nothing is compacted (the mask of points to refine goes to the kernel), each
batch uses its own joint matrices (the reference's compaction reads batch 0's for every point; the two agree for one batch), and
``iterations`` is honoured (the reference always runs 10).  No gradients: the reference runs the whole step under ``no_grad``.
Every tensor must be on the GPU; there is no host path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import stream as _stream
from .weight_volume import WeightVolume

HAND_JOINTS = ((25, 40, 20), (40, 55, 21))        # joints [first, last) take the matrix of the wrist (template.py:213-214)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _points(t, name: str, dev=None, last: int = 3) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (there is no host path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dim() not in (2, 3) or t.shape[-1] != last:
        raise ValueError(f"{name} must be [B, N, {last}] or [N, {last}], got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _matrices(jnt_mats, B: int, J: Optional[int], dev) -> torch.Tensor:
    if not isinstance(jnt_mats, torch.Tensor) or not jnt_mats.is_cuda:
        raise ValueError("jnt_mats must be a tensor on the GPU (there is no host path)")
    if jnt_mats.device != dev:
        raise ValueError(f"jnt_mats is on {jnt_mats.device}, the points on {dev}")
    m = jnt_mats.detach().to(torch.float32)
    if m.dim() == 3:
        m = m[None]
    if m.dim() != 4 or tuple(m.shape[2:]) != (4, 4) or m.shape[0] != B or (J is not None and m.shape[1] != J):
        raise ValueError(f"jnt_mats must be [{B}, {'J' if J is None else J}, 4, 4], got {tuple(jnt_mats.shape)}")
    if not 1 <= m.shape[1] <= 128:
        raise ValueError(f"J = {m.shape[1]} is outside 1 .. 128")
    return m.contiguous()


def rigid_hands(jnt_mats: torch.Tensor) -> torch.Tensor:
    """A copy of ``jnt_mats`` [B, 55, 4, 4] in which the fingers move rigidly with their wrist: joints 25-39 take joint 20's matrix and
    40-54 joint 21's (``template.py:211-214``, the reference's ``with_hand = False``)."""
    if jnt_mats.dim() != 4 or jnt_mats.shape[1] != 55:
        raise ValueError(f"with_hand=False needs the 55 SMPL-X joints, got jnt_mats {tuple(jnt_mats.shape)}")
    m = jnt_mats.clone()
    for first, last, wrist in HAND_JOINTS:
        m[:, first:last] = m[:, wrist:wrist + 1]
    return m


def initial_guess(posed_pts: torch.Tensor, pts_w: torch.Tensor, jnt_mats: torch.Tensor, normals: Optional[torch.Tensor] = None):
    """``template.py:247-253``: the inverse of the blend ``sum_j w_j A_j`` (as an affine map) applied to ``posed_pts`` [B, N, 3], and its
    rotation part to ``normals``.  ``pts_w`` [B, N, J], ``jnt_mats`` [B, J, 4, 4].  Returns the points, or (points, normals)."""
    p = _points(posed_pts, "posed_pts")
    squeeze = p.dim() == 2
    if not isinstance(pts_w, torch.Tensor) or pts_w.dim() != p.dim():
        raise ValueError("pts_w must be a tensor [B, N, J] (or [N, J]) beside posed_pts")
    w = _points(pts_w, "pts_w", p.device, last=int(pts_w.shape[-1]))
    n = _points(normals, "normals", p.device) if normals is not None else None
    if w.shape[:-1] != p.shape[:-1] or (n is not None and n.shape != p.shape):
        raise ValueError(f"posed_pts {tuple(p.shape)}, pts_w {tuple(w.shape)} and normals must agree in [B, N]")
    B, N = (1, p.shape[0]) if squeeze else (p.shape[0], p.shape[1])
    m = _matrices(jnt_mats, B, int(w.shape[-1]), p.device)
    out_p = torch.empty_like(p)
    out_n = torch.empty_like(n) if n is not None else None
    with _lib.on_device(p.device):
        _lib.check(_lib.lib().ag_inverse_skinning_init(_ptr(p), _ptr(w), _ptr(m), _ptr(n), _ptr(out_p), _ptr(out_n), B, N, int(w.shape[-1]),
                                                       _stream(p.device)), "ag_inverse_skinning_init")
    return out_p if n is None else (out_p, out_n)


def _root_find(volume: WeightVolume, posed_pts, cano_init, jnt_mats, active, lam, iterations, volume_type, grad_volume):
    vol = volume._which(volume_type)
    xt = _points(posed_pts, "posed_pts", vol.device)
    xc = _points(cano_init, "cano_init", vol.device)
    if xt.shape != xc.shape:
        raise ValueError(f"posed_pts {tuple(xt.shape)} and cano_init {tuple(xc.shape)} must have one shape")
    B, N = (1, xt.shape[0]) if xt.dim() == 2 else (xt.shape[0], xt.shape[1])
    X, Y, Z, J = (int(s) for s in vol.shape)
    if not 1 <= J <= 128:
        raise ValueError(f"J = {J} is outside 1 .. 128")
    m = _matrices(jnt_mats, B, J, vol.device)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations must not be negative, got {iterations}")
    mask = None
    if active is not None:
        if not isinstance(active, torch.Tensor) or active.device != vol.device or active.dtype != torch.bool or active.shape != xt.shape[:-1]:
            raise ValueError(f"active must be a bool tensor of shape {tuple(xt.shape[:-1])} on {vol.device}")
        mask = active.to(torch.uint8).contiguous()
    grad = None
    if grad_volume is not None:
        if not isinstance(grad_volume, torch.Tensor) or grad_volume.device != vol.device or grad_volume.dtype != torch.float32 \
                or tuple(grad_volume.shape) != (X, Y, Z, J, 3):
            raise ValueError(f"grad_volume must be float32 [{X}, {Y}, {Z}, {J}, 3] on {vol.device} (WeightVolume.gradient_volume)")
        grad = grad_volume.contiguous()
    out = torch.empty_like(xc)
    with _lib.on_device(vol.device):
        _lib.check(_lib.lib().ag_inverse_skinning_root_find(_ptr(vol), _ptr(grad), X, Y, Z, J, volume._bounds_host, volume._spacing_host(), _ptr(xt),
                                                            _ptr(xc), _ptr(m), _ptr(mask), _ptr(out), B, N, float(lam), iterations,
                                                            _stream(vol.device)), "ag_inverse_skinning_root_find")
    return out


def transform_cano2live(cano_pts: torch.Tensor, cano2live_jnt_mats: torch.Tensor, volume: WeightVolume, *, normals: Optional[torch.Tensor] = None,
                        with_hand: bool = False, volume_type: str = "diff"):
    """``template.py:209-224``: ``cano_pts`` [B, N, 3] blended forward with the volume's trilinear weights
    (``WeightVolume.forward_weight``) and ``cano2live_jnt_mats`` [B, J, 4, 4]; ``normals`` are rotated by the blend's 3 x 3 part.
    ``with_hand=False`` makes the hands rigid (``rigid_hands``).  Returns the posed points, or (points, normals)."""
    from .avatar_ops import lbs_transform
    p = _points(cano_pts, "cano_pts", volume.diff_weight_volume.device)
    if p.dim() != 3:
        raise ValueError(f"cano_pts must be [B, N, 3], got {tuple(p.shape)}")
    n = _points(normals, "normals", p.device) if normals is not None else None
    if n is not None and n.shape != p.shape:
        raise ValueError("normals must have the shape of cano_pts")
    m = _matrices(cano2live_jnt_mats, p.shape[0], volume.joint_num, p.device)
    if not with_hand:
        m = rigid_hands(m)
    w = volume.forward_weight(p, volume_type=volume_type)
    unit = torch.zeros((p.shape[1], 4), dtype=torch.float32, device=p.device)
    unit[:, 0] = 1.0
    posed = torch.stack([lbs_transform(p[b], unit, w[b], m[b])[0] for b in range(p.shape[0])], 0) if p.shape[1] else torch.empty_like(p)
    if n is None:
        return posed
    rot = m.clone()
    rot[:, :, :3, 3] = 0.0                                    # the blend's rotation part alone (template.py:223)
    posed_n = torch.stack([lbs_transform(n[b], unit, w[b], rot[b])[0] for b in range(p.shape[0])], 0) if p.shape[1] else torch.empty_like(n)
    return posed, posed_n


def transform_live2cano(posed_pts: torch.Tensor, cano2live_jnt_mats: torch.Tensor, volume: WeightVolume, live_mesh_v: torch.Tensor,
                        live_mesh_f: torch.Tensor, live_mesh_lbs: torch.Tensor, *, normals: Optional[torch.Tensor] = None, near_thres: float = 0.08,
                        use_root_finding: bool = True, with_hand: bool = False, nonopt_bone_ids: Sequence[int] = (7, 8, 10, 11), lam: float = 0.1,
                        iterations: int = 10, volume_type: str = "diff"):
    """``template.py:226-286`` with barycentric weights: ``posed_pts`` [B, N, 3] -> ``(cano_pts[, cano_normals], near_flag)``.

    The weights of each point are those at its nearest point of the posed mesh (``live_mesh_v`` [B, M, 3], ``live_mesh_f`` [B, F, 3],
    ``live_mesh_lbs`` [B, M, J]; ``mesh_query.calc_blending_weight``), ``near_flag`` [B, N] says whether that point is closer than
    ``near_thres``.  The initial guess is ``initial_guess``; with ``use_root_finding`` every point whose largest weight is not one of
    ``nonopt_bone_ids`` (the knees and ankles' children in the reference: bones the iteration is not trusted on) is then refined with
    ``WeightVolume.root_find``; the others keep the initial guess.  Normals are not refined, as in the reference."""
    from . import mesh_query
    p = _points(posed_pts, "posed_pts", volume.diff_weight_volume.device)
    if p.dim() != 3:
        raise ValueError(f"posed_pts must be [B, N, 3], got {tuple(p.shape)}")
    m = _matrices(cano2live_jnt_mats, p.shape[0], volume.joint_num, p.device)
    if not with_hand:
        m = rigid_hands(m)
    pts_w, near_flag = mesh_query.calc_blending_weight(p, live_mesh_v, live_mesh_f, live_mesh_lbs, near_thres, method="barycentric")
    guess = initial_guess(p, pts_w, m, normals)
    cano, cano_n = guess if normals is not None else (guess, None)
    if use_root_finding and p.shape[1]:
        argmax = pts_w.argmax(-1)
        active = torch.ones_like(argmax, dtype=torch.bool)
        for i in nonopt_bone_ids:
            active &= argmax != int(i)
        cano = volume.root_find(p, cano, m, active=active, lam=lam, iterations=iterations, volume_type=volume_type)
    return (cano, near_flag) if normals is None else (cano, cano_n, near_flag)
