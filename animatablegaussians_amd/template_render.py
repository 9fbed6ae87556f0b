"""Render the template field along camera rays on the GPU (``include/ag_ray_march.h``): ``rgb_map`` / ``acc_map`` of a template checkpoint.

Re-host of the reference's ``TemplateNet.render`` (``network/template.py:288-405``) in eval mode for one batch element, from three HIP
kernels and the two that existed: near / far of every ray against balls around the posed SMPL-X vertices (the reference's CUDA extension
``utils/posevocab_custom_ops/near_far_smpl_kernel.cu``), sample placement (``nerf_util.sample_pts_on_rays``), ``transform_live2cano`` for
posed space (``inverse_skinning``), the fused field (``template_field.TemplateField``) and alpha compositing (``template.py:372-374``,
``nerf_util.raw2outputs``).  The random numbers of a perturbed sampling are the caller's (``u``), never a kernel's.

``render_normals`` is the same march with ``compute_grad``: the raw SDF gradient at every sample (``render_output['normal']``,
``template.py:380-383``) from ``TemplateField.sdf_normal``, and a composited normal image.

``render(..., hands=)`` fuses the hand fields into the body field at every sample (``template.py:365-366``, ``hand_fusion.fuse_hands``) between
the field and the compositing: what a checkpoint trained with ``with_hand: true`` needs.

Training (``include/ag_ray_march_grad.h``): ``composite`` is differentiable in ``density`` and ``color`` (``composite_backward``: one
reverse scan per ray, no division by ``1 - alpha + 1e-10``), ``laplace_density`` is ``LaplaceDensity`` with a learned ``beta``,
differentiable in both arguments, ``render_train`` is ``TemplateNet.render`` in training mode (the caller's noise on the view
directions, the scattering through ``mask_within_patch``) around any differentiable field callable, and ``training_loss`` the colour
and mask L1 terms of ``main_template.py:37-51``.

NOT here: the reverse pass of the fused MLP (``render_train`` takes a torch callable as the field until it exists), the eikonal
term's second-order pass, the hand fusion's backward and gradients to ``z_vals``.  The rays and the box near / far are the caller's, as
in the reference's batch; ``ray_select`` builds them on the device (``image_rays`` / ``render_image`` for a camera, ``sample_randomly`` /
``sample_patches`` for a training batch from a frame).  Near / far of the SMPL-X balls is pinned to the header's
formulas: the reference's kernel is CUDA and was never run beside this one.  Every tensor must be on the GPU; there is no host path
and no PyTorch fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .mlp_blob import ptr as _ptr, stream as _stream

MIN_SAMPLES, MAX_SAMPLES = 2, 1024          # include/ag_ray_march.h
OUTPUTS = ("rgb_map", "acc_map", "depth_map", "disp_map", "weights")
SAMPLINGS = ("smpl", "uniform", "depth")


def _f32(t, name: str, shape, dev=None) -> torch.Tensor:
    """``t`` as a contiguous float32 device tensor of ``shape`` (None entries are free)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (there is no host path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and int(s) != w for s, w in zip(t.shape, shape)):
        raise ValueError(f"{name} must be [{', '.join('N' if w is None else str(w) for w in shape)}], got {tuple(t.shape)}")
    return t.detach().contiguous()


def _rays(ray_o, ray_d):
    o = _f32(ray_o, "ray_o", (None, 3))
    d = _f32(ray_d, "ray_d", (o.shape[0], 3), o.device)
    return o, d


def _samples(n_samples) -> int:
    s = int(n_samples)
    if not MIN_SAMPLES <= s <= MAX_SAMPLES:
        raise ValueError(f"n_samples must be {MIN_SAMPLES} .. {MAX_SAMPLES}, got {n_samples}")
    return s


def _want(want, allowed=OUTPUTS):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not set(want) <= set(allowed):
        raise ValueError(f"want names {', '.join(repr(k) for k in allowed)}, got {want}")
    return want


def near_far_smpl(vertices: torch.Tensor, ray_o: torch.Tensor, ray_d: torch.Tensor, radius: float = 0.1, fallback=None):
    """``near [R], far [R], hit [R] (bool)`` of the rays against a ball of ``radius`` around each of ``vertices`` [V, 3]
    (``posevocab_custom_ops.near_far_smpl``).  A ray that hits no ball takes ``fallback = (near [R], far [R])`` (``template.py:308-309``),
    or 0 / 0 without one, which is what the reference's kernel writes."""
    o, d = _rays(ray_o, ray_d)
    v = _f32(vertices, "vertices", (None, 3), o.device)
    if v.shape[0] < 1:
        raise ValueError("vertices must hold at least one vertex")
    radius = float(radius)
    if not (radius > 0 and radius < float("inf")):
        raise ValueError(f"radius must be finite and positive, got {radius}")
    fb_n = fb_f = None
    if fallback is not None:
        if not isinstance(fallback, (tuple, list)) or len(fallback) != 2:
            raise ValueError("fallback must be (near [R], far [R])")
        fb_n, fb_f = _f32(fallback[0], "fallback near", (o.shape[0],), o.device), _f32(fallback[1], "fallback far", (o.shape[0],), o.device)
    R = o.shape[0]
    near, far = torch.empty(R, dtype=torch.float32, device=o.device), torch.empty(R, dtype=torch.float32, device=o.device)
    hit = torch.empty(R, dtype=torch.uint8, device=o.device)
    if R:
        with _lib.on_device(o.device):
            _lib.check(_lib.lib().ag_ray_near_far(_ptr(v), v.shape[0], _ptr(o), _ptr(d), R, radius, _ptr(fb_n), _ptr(fb_f), _ptr(near), _ptr(far), _ptr(hit),
                                                  _stream(o.device)), "ag_ray_near_far")
    return near, far, hit.to(torch.bool)


def _t_vals(S: int, dev) -> torch.Tensor:
    """``torch.linspace(0, 1, S)`` in float32, computed on the host (as ``volume_axes`` does for the grid): torch's values bit for bit."""
    return torch.linspace(0.0, 1.0, steps=S, dtype=torch.float32).to(dev)


def _sample(o, d, near, far, t, u, mask, want_dirs):
    R, S = o.shape[0], t.shape[0]
    z = torch.empty((R, S), dtype=torch.float32, device=o.device)
    pts = torch.empty((R, S, 3), dtype=torch.float32, device=o.device)
    dirs = torch.empty((R, S, 3), dtype=torch.float32, device=o.device) if want_dirs else None
    if R:
        with _lib.on_device(o.device):
            _lib.check(_lib.lib().ag_ray_sample(_ptr(o), _ptr(d), _ptr(near), _ptr(far), R, _ptr(t), S, _ptr(u), _ptr(mask), _ptr(z), _ptr(pts), _ptr(dirs),
                                                _stream(o.device)), "ag_ray_sample")
    return pts, z, dirs


def _perturbation(u, mask, R, S, dev):
    if u is None:
        if mask is not None:
            raise ValueError("a mask without u: the mask says which rays u perturbs")
        return None, None
    u = _f32(u, "u", (R, S), dev)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype != torch.bool or tuple(mask.shape) != (R,):
            raise ValueError(f"mask must be a bool tensor [{R}] on {dev}")
        mask = mask.to(torch.uint8).contiguous()
    return u, mask


def sample_pts_on_rays(ray_o: torch.Tensor, ray_d: torch.Tensor, near: torch.Tensor, far: torch.Tensor, n_samples: int = 64,
                       u: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, return_viewdirs: bool = False):
    """``nerf_util.sample_pts_on_rays``: ``pts [R, S, 3], z_vals [R, S]`` with ``z = near * (1 - t) + far * t``, ``t = linspace(0, 1, S)``.
    ``u`` [R, S] (the caller's ``torch.rand``) perturbs the samples inside their strata, for the rays of the bool ``mask`` [R] or for all
    rays without one (the reference's ``perturb`` / ``depth_guided_mask``); a given ``u`` always gives the same samples.
    ``return_viewdirs`` adds ``ray_d / |ray_d|`` repeated for each ray's samples, [R, S, 3] (``template.py:355-356``)."""
    o, d = _rays(ray_o, ray_d)
    R = o.shape[0]
    near, far = _f32(near, "near", (R,), o.device), _f32(far, "far", (R,), o.device)
    S = _samples(n_samples)
    u, mask = _perturbation(u, mask, R, S, o.device)
    pts, z, dirs = _sample(o, d, near, far, _t_vals(S, o.device), u, mask, bool(return_viewdirs))
    return (pts, z, dirs) if return_viewdirs else (pts, z)


def _composite_into(density, color, z, white_bkgd, out):
    """``out``: name -> preallocated tensor (or a slice of one along the rays) for ``acc_map`` and whatever else is wanted."""
    R, S = z.shape
    if R:
        with _lib.on_device(z.device):
            _lib.check(_lib.lib().ag_ray_composite(_ptr(density), _ptr(color), _ptr(z), R, S, 1 if white_bkgd else 0, _ptr(out.get("rgb_map")),
                                                   _ptr(out["acc_map"]), _ptr(out.get("depth_map")), _ptr(out.get("disp_map")), _ptr(out.get("weights")),
                                                   _stream(z.device)), "ag_ray_composite")


def _outputs(want, R, S, dev):
    shapes = {"rgb_map": (R, 3), "acc_map": (R,), "depth_map": (R,), "disp_map": (R,), "weights": (R, S)}
    return {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in OUTPUTS if k in want or k == "acc_map"}


def composite(density: torch.Tensor, color: Optional[torch.Tensor], z_vals: torch.Tensor, white_bkgd: bool = False, want=("rgb_map", "acc_map")):
    """``template.py:345-346, 372-374`` + ``nerf_util.raw2outputs``: ``density`` [R, S] (or [R * S, 1], the field's shape), ``color``
    [R, S, 3] (or [R * S, 3]; None for a field without colour), ``z_vals`` [R, S] -> dict with ``rgb_map`` [R, 3], ``acc_map`` [R] and, when
    named in ``want``, ``depth_map`` [R], ``disp_map`` [R], ``weights`` [R, S].  alpha is formed inside the kernel.

    Differentiable in ``density`` and ``color``: when grad mode is on and either requires grad, the same launch is recorded for autograd
    and its backward is ``composite_backward``; ``disp_map`` is not differentiable, and a ``z_vals`` that requires grad is refused.  In
    every other case nothing but the forward launch runs; the maps' bits are the same either way."""
    want = _want(want)
    grad_mode = torch.is_grad_enabled()
    if grad_mode and isinstance(z_vals, torch.Tensor) and z_vals.requires_grad:
        raise ValueError("z_vals requires grad: there is no gradient to the sample positions (they carry no parameters in the reference); detach z_vals")
    tracked = grad_mode and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (density, color))
    density_in, color_in, z = _composite_inputs(density, color, z_vals)
    R, S = z.shape
    if color_in is None and "rgb_map" in want:
        raise ValueError("rgb_map needs color")
    if "rgb_map" not in want:
        color_in = None
    if tracked:
        # the same launch and the same bits, recorded for autograd (composite_backward)
        maps = _Composite.apply(density_in, color_in, z, bool(white_bkgd), want)
        return {k: v for k, v in zip([k for k in OUTPUTS if k in want or k == "acc_map"], maps) if k in want}
    out = _outputs(want, R, S, z.device)
    _composite_into(density_in.detach().contiguous(), None if color_in is None else color_in.detach().contiguous(), z, white_bkgd, out)
    return {k: v for k, v in out.items() if k in want}


def _composite_inputs(density, color, z_vals):
    """The checks of ``composite`` -> ``density`` [R, S] and ``color`` [R, S, 3] (or None) still attached to their graphs, ``z`` detached."""
    z = _f32(z_vals, "z_vals", (None, None))
    R, S = z.shape
    _samples(S)
    if not isinstance(density, torch.Tensor) or density.numel() != R * S:
        raise ValueError(f"density must hold {R} x {S} values, got {tuple(density.shape) if isinstance(density, torch.Tensor) else type(density)}")
    density = density.reshape(R, S)
    _f32(density, "density", (R, S), z.device)
    if color is not None:
        if not isinstance(color, torch.Tensor) or color.numel() != R * S * 3 or color.shape[-1] != 3:
            raise ValueError(f"color must hold {R} x {S} x 3 values, got {tuple(color.shape) if isinstance(color, torch.Tensor) else type(color)}")
        color = color.reshape(R, S, 3)
        _f32(color, "color", (R, S, 3), z.device)
    return density, color, z


GRADS = ("rgb_map", "acc_map", "depth_map", "weights")


def _composite_backward(density, color, z, white_bkgd, g, need_density, need_color):
    """One ``ag_ray_composite_backward`` launch on detached contiguous inputs; ``g``: name -> contiguous float32 gradient."""
    R, S = z.shape
    gd = torch.empty((R, S), dtype=torch.float32, device=z.device) if need_density else None
    gc = torch.empty((R, S, 3), dtype=torch.float32, device=z.device) if need_color else None
    if R:
        with _lib.on_device(z.device):
            _lib.check(_lib.lib().ag_ray_composite_backward(_ptr(density), _ptr(color), _ptr(z), R, S, 1 if white_bkgd else 0, _ptr(g.get("rgb_map")),
                                                            _ptr(g.get("acc_map")), _ptr(g.get("depth_map")), _ptr(g.get("weights")), _ptr(gd), _ptr(gc),
                                                            _stream(z.device)), "ag_ray_composite_backward")
    return gd, gc


def composite_backward(density: torch.Tensor, color: Optional[torch.Tensor], z_vals: torch.Tensor, grads: dict, white_bkgd: bool = False):
    """The gradient of ``composite`` (``include/ag_ray_march_grad.h``): ``grads`` holds the upstream gradients of any of ``rgb_map`` [R, 3],
    ``acc_map`` [R], ``depth_map`` [R], ``weights`` [R, S] (a missing one is zero; none at all gives zeros) -> ``{"density": [R, S],
    "color": [R, S, 3]}``.  ``color`` is None in the result when ``grads`` has no ``rgb_map`` (the colour then receives no gradient) or
    no ``color`` was given.  There is no gradient to ``z_vals`` and none through ``disp_map``."""
    if not isinstance(grads, dict) or not set(grads) <= set(GRADS):
        raise ValueError(f"grads names {', '.join(repr(k) for k in GRADS)}, got {sorted(grads) if isinstance(grads, dict) else type(grads)}")
    density, color, z = _composite_inputs(density, color, z_vals)
    R, S = z.shape
    shapes = {"rgb_map": (R, 3), "acc_map": (R,), "depth_map": (R,), "weights": (R, S)}
    g = {k: _f32(v, f"grads[{k!r}]", shapes[k], z.device) for k, v in grads.items() if v is not None}
    if "rgb_map" in g and color is None:
        raise ValueError("grads['rgb_map'] needs color")
    color = color.detach().contiguous() if "rgb_map" in g else None
    gd, gc = _composite_backward(density.detach().contiguous(), color, z, white_bkgd, g, True, color is not None)
    return {"density": gd, "color": gc}


class _Composite(torch.autograd.Function):
    """``composite`` for autograd: the forward is ``_composite_into``, the backward ``ag_ray_composite_backward``."""

    @staticmethod
    def forward(ctx, density, color, z, white_bkgd, want):
        density = density.detach().contiguous()
        color = None if color is None else color.detach().contiguous()
        R, S = z.shape
        out = _outputs(want, R, S, z.device)
        _composite_into(density, color, z, white_bkgd, out)
        ctx.save_for_backward(density, color, z)
        ctx.white_bkgd, ctx.names = white_bkgd, tuple(out)
        ctx.set_materialize_grads(False)
        if "disp_map" in out:
            ctx.mark_non_differentiable(out["disp_map"])
        return tuple(out.values())

    @staticmethod
    def backward(ctx, *upstream):
        density, color, z = ctx.saved_tensors
        g = {k: v.contiguous() for k, v in zip(ctx.names, upstream) if v is not None and k in GRADS}
        need_density, need_color = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and "rgb_map" in g
        if not need_density and not need_color:
            return None, None, None, None, None
        gd, gc = _composite_backward(density, color if "rgb_map" in g else None, z, ctx.white_bkgd, g, need_density, need_color)
        return gd, gc, None, None, None


class _LaplaceDensity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, beta):
        s = sdf.detach().contiguous()
        b = beta.detach().contiguous()
        out = torch.empty_like(s)
        if s.numel():
            with _lib.on_device(s.device):
                _lib.check(_lib.lib().ag_laplace_density(_ptr(s), s.numel(), _ptr(b), _ptr(out), _stream(s.device)), "ag_laplace_density")
        ctx.save_for_backward(s, b)
        return out

    @staticmethod
    def backward(ctx, g):
        s, b = ctx.saved_tensors
        need_sdf, need_beta = ctx.needs_input_grad
        if not need_sdf and not need_beta:
            return None, None
        g = g.contiguous()
        N, L = s.numel(), _lib.lib()
        gs = torch.empty_like(s) if need_sdf else None
        gb = torch.empty_like(b) if need_beta else None
        ws = torch.empty(int(L.ag_laplace_density_backward_workspace_bytes(N)) // 8, dtype=torch.float64, device=s.device) if need_beta else None
        if N or need_beta:
            with _lib.on_device(s.device):
                _lib.check(L.ag_laplace_density_backward(_ptr(s), _ptr(g), N, _ptr(b), _ptr(gs), _ptr(gb), _ptr(ws), _stream(s.device)),
                           "ag_laplace_density_backward")
        return gs, gb


def laplace_density(sdf: torch.Tensor, beta) -> torch.Tensor:
    """``LaplaceDensity`` (``network/density.py:22-36``) of the field's ``sdf`` (positive inside; any shape) -> the density, same shape:
    ``(1 / b) * (0.5 + 0.5 * sign(-sdf) * expm1(-|sdf| / b))`` with ``b = |beta| + 1e-4`` formed on the device from ``beta``, a one-element
    float32 device tensor (the learned parameter: no host read) or a float.  For the same ``sdf`` it equals ``TemplateField``'s density
    bit for bit.  Differentiable in ``sdf`` and in a tensor ``beta`` (``ag_laplace_density_backward``; the gradient of ``beta`` is
    bit-identical between calls)."""
    if not isinstance(sdf, torch.Tensor) or not sdf.is_cuda or sdf.dtype != torch.float32:
        raise ValueError("sdf must be a float32 tensor on the GPU (there is no host path)")
    if isinstance(beta, torch.Tensor):
        if beta.device != sdf.device or beta.dtype != torch.float32 or beta.numel() != 1:
            raise ValueError(f"beta must be a one-element float32 tensor on {sdf.device} or a float")
    else:
        beta = torch.tensor([float(beta)], dtype=torch.float32, device=sdf.device)
    return _LaplaceDensity.apply(sdf, beta)


def _march_setup(ray_o, ray_d, near, far, space, sampling, live_smpl_v, radius, dist, near_sur_dist, n_samples, u, chunk_size, live):
    """The checks and the sampling set-up that ``render`` and ``render_normals`` share, after their own checks of ``want``: ->
    ``(o, d, near, far, t, u, mask, chunk_size, batched)`` with near / far already those of the sampling.  A refusal launches nothing."""
    if space not in ("cano", "live"):
        raise ValueError(f"space must be 'cano' or 'live', got {space!r}")
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling must be one of {SAMPLINGS}, got {sampling!r}")
    batched = isinstance(ray_o, torch.Tensor) and ray_o.dim() == 3
    if batched:
        if ray_o.shape[0] != 1:
            raise ValueError(f"render takes one batch element, got ray_o {tuple(ray_o.shape)}")
        squeeze = lambda t: t[0] if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == 1 else t  # noqa: E731
        ray_o, ray_d, near, far, dist, u = (squeeze(t) for t in (ray_o, ray_d, near, far, dist, u))
    o, d = _rays(ray_o, ray_d)
    R, dev = o.shape[0], o.device
    near, far = _f32(near, "near", (R,), dev), _f32(far, "far", (R,), dev)
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise ValueError(f"chunk_size must be positive, got {chunk_size}")
    if space == "live":
        if not isinstance(live, dict) or not {"cano2live_jnt_mats", "volume", "live_mesh_v", "live_mesh_f", "live_mesh_lbs"} <= set(live):
            raise ValueError("space='live' needs live = dict(cano2live_jnt_mats=, volume=, live_mesh_v=, live_mesh_f=, live_mesh_lbs=, ...), the "
                             "arguments of inverse_skinning.transform_live2cano")
        if "normals" in live:
            raise ValueError("live must not carry normals: compute_grad / normals are not rendered")
    mask = None
    if sampling == "smpl":
        if live_smpl_v is None:
            raise ValueError("sampling='smpl' needs live_smpl_v, the posed SMPL-X vertices [V, 3]")
        v = live_smpl_v[0] if isinstance(live_smpl_v, torch.Tensor) and live_smpl_v.dim() == 3 and live_smpl_v.shape[0] == 1 else live_smpl_v
        v = _f32(v, "live_smpl_v", (None, 3), dev)
        S = 64
    elif sampling == "uniform":
        S = 64
    else:
        if dist is None or near_sur_dist is None:
            raise ValueError("sampling='depth' needs dist [R] and near_sur_dist")
        dist = _f32(dist, "dist", (R,), dev)
        S = _samples(n_samples)
        mask = dist > 1e-6
        near_sur_dist = float(near_sur_dist)
        near, far = torch.where(mask, dist - near_sur_dist, near), torch.where(mask, dist + near_sur_dist, far)
    u, mask = _perturbation(u, mask if u is not None else None, R, S, dev)
    if sampling == "smpl":                          # after every check: a refusal launches nothing
        near, far, _ = near_far_smpl(v, o, d, radius, fallback=(near, far))
    return o, d, near, far, _t_vals(S, dev), u, mask, chunk_size, batched


def _chunks(setup, space, live, want_dirs):
    """``(r0, r1, canonical points [(r1 - r0) * S, 3], z [r1 - r0, S], dirs or None, the points as sampled)`` of every chunk of rays:
    sample, then (live) map."""
    o, d, near, far, t, u, mask, chunk_size, _ = setup
    if space == "live":
        from .inverse_skinning import transform_live2cano
    for r0 in range(0, o.shape[0], chunk_size):
        r1 = min(o.shape[0], r0 + chunk_size)
        pts, z, dirs = _sample(o[r0:r1], d[r0:r1], near[r0:r1], far[r0:r1], t, None if u is None else u[r0:r1], None if mask is None else mask[r0:r1],
                               want_dirs)
        pts = sampled = pts.view(-1, 3)
        if space == "live":
            pts = transform_live2cano(pts[None], **live)[0][0]
        yield r0, r1, pts, z, dirs, sampled


def render(field, ray_o: torch.Tensor, ray_d: torch.Tensor, near: torch.Tensor, far: torch.Tensor, *, space: str = "cano", sampling: str = "smpl",
           live_smpl_v: Optional[torch.Tensor] = None, radius: float = 0.1, dist: Optional[torch.Tensor] = None,
           near_sur_dist: Optional[float] = None, n_samples: int = 64, u: Optional[torch.Tensor] = None, chunk_size: int = 4096,
           white_bkgd: bool = False, live: Optional[dict] = None, want=("rgb_map", "acc_map"), hands: Optional[dict] = None):
    """``TemplateNet.render`` in eval mode for one batch element: rays ``ray_o`` / ``ray_d`` [R, 3] (or [1, R, 3]) with the box ``near`` /
    ``far`` [R] (or [1, R]) through ``field`` (a ``TemplateField``) -> dict of ``rgb_map`` [R, 3], ``acc_map`` [R] and, when named in
    ``want``, ``depth_map``, ``disp_map``, ``weights`` [R, S]; a leading 1 of the rays is kept in the outputs.

    ``sampling`` (the reference's ``depth_guided_sampling``): ``"smpl"`` takes near / far from ``near_far_smpl(live_smpl_v, ..)`` with
    the given ones for the rays that hit nothing, 64 samples; ``"uniform"`` the given ones, 64 samples; ``"depth"`` ``dist -+
    near_sur_dist`` where ``dist`` [R] ``> 1e-6`` and the given ones elsewhere, ``n_samples`` samples.  ``u`` [R, S] perturbs the samples
    (the reference's training mode; with ``"depth"`` only the rays with a valid ``dist``, ``template.py:334``).

    ``space="live"`` maps every sample to canonical space first: ``live`` holds the arguments of
    ``inverse_skinning.transform_live2cano`` by name (``cano2live_jnt_mats``, ``volume``, ``live_mesh_v``, ``live_mesh_f``,
    ``live_mesh_lbs`` and optionally ``near_thres``, ``use_root_finding``, ``with_hand`` ..).  The rays are processed ``chunk_size`` at
    a time: sample, map, field, composite straight into the outputs; nothing depends on ``chunk_size``, bit for bit.  A field without
    a colour MLP renders everything but ``rgb_map``.

    ``hands`` (the reference's ``with_hand``): ``dict(left=dict(v=, n=, f=, cano_v=), right=dict(...), left_field=, right_field=,
    cano_smpl_center=)`` and optionally ``hand_pose`` [45] and ``compact``: the two hand meshes with ``v`` / ``n`` in the space the rays
    are in (``hand_fusion.hand_meshes`` of the posed vertices for ``space="live"``, of the canonical ones for ``"cano"``) and ``cano_v``
    in canonical space, the two ``HandField`` and the centre.  Every chunk then goes through ``hand_fusion.fuse_hands`` between the
    field and the composite.  Without ``hands`` nothing of it runs and the outputs are what they were, bit for bit."""
    from .template_field import TemplateField
    if not isinstance(field, TemplateField):
        raise ValueError("field must be a TemplateField")
    want = _want(want)
    if "rgb_map" in want and not field.color:
        raise ValueError("this field has no colour MLP: rgb_map cannot be rendered")
    if hands is not None:
        required = {"left", "right", "left_field", "right_field", "cano_smpl_center"}
        if not isinstance(hands, dict) or not required <= set(hands) or not set(hands) <= required | {"hand_pose", "compact"}:
            raise ValueError("hands must be dict(left=, right=, left_field=, right_field=, cano_smpl_center=[, hand_pose=, compact=])")
        from . import hand_fusion
        hand_pose = hand_fusion.check_fields(hands["left_field"], hands["right_field"], hands.get("hand_pose"))      # no launch: a refusal here leaves nothing behind
    setup = _march_setup(ray_o, ray_d, near, far, space, sampling, live_smpl_v, radius, dist, near_sur_dist, n_samples, u, chunk_size, live)
    o, t, batched = setup[0], setup[4], setup[8]
    if hands is not None:                           # the meshes: checked and their boxes reduced on the device, once, after near / far
        prepared = hand_fusion.PreparedHands(hands, o.device)
    out = _outputs(want, o.shape[0], t.shape[0], o.device)
    field_want = ("sdf", "density", "color") if "rgb_map" in want else ("sdf", "density")
    use_dirs = bool(field.use_viewdir) and "rgb_map" in want
    for r0, r1, pts, z, dirs, sampled in _chunks(setup, space, live, use_dirs):
        ret = field(pts, dirs.view(-1, 3) if use_dirs else None, want=field_want)
        if hands is not None:
            ret = hand_fusion.fuse_hands(ret, sampled, prepared, hands["left_field"], hands["right_field"], cano_smpl_center=hands["cano_smpl_center"],
                                         density_b=field.density_b, hand_pose=hand_pose, compact=hands.get("compact", True))
        _composite_into(ret["density"], ret.get("color"), z, white_bkgd, {k: v[r0:r1] for k, v in out.items()})
    out = {k: v for k, v in out.items() if k in want}
    return {k: v[None] for k, v in out.items()} if batched else out


NORMAL_OUTPUTS = ("normal", "normal_map", "acc_map", "depth_map", "weights")


def render_normals(field, ray_o: torch.Tensor, ray_d: torch.Tensor, near: torch.Tensor, far: torch.Tensor, *, space: str = "cano", sampling: str = "smpl",
                   live_smpl_v: Optional[torch.Tensor] = None, radius: float = 0.1, dist: Optional[torch.Tensor] = None,
                   near_sur_dist: Optional[float] = None, n_samples: int = 64, u: Optional[torch.Tensor] = None, chunk_size: int = 4096,
                   live: Optional[dict] = None, want=("normal_map", "acc_map")):
    """``render``'s rays, samplings, spaces and checks with ``compute_grad`` (``template.py:380-383``) -> dict of

    ``normal`` [R, S, 3] (only when named in ``want``): the reference's ``render_output['normal']``, the raw gradient of the SDF at
    every sample (``TemplateField.sdf_normal``), in CANONICAL coordinates also for ``space="live"``: the reference differentiates with
    respect to the canonical points;
    ``normal_map`` [R, 3] ``= sum_s weights_s * n_s / max(||n_s||, 1e-12)``: the unit normals composited as ``render`` composites the
    colour, without a background.  This is this project's definition; the reference has no normal image;
    ``acc_map`` [R] (``render``'s bit for bit) and, when named, ``depth_map`` [R], ``weights`` [R, S].

    Per chunk: sample, map, one ``ag_template_field_sdf_grad`` launch, composite; nothing depends on ``chunk_size``, bit for bit."""
    from .template_field import TemplateField
    if not isinstance(field, TemplateField):
        raise ValueError("field must be a TemplateField")
    want = _want(want, NORMAL_OUTPUTS)
    setup = _march_setup(ray_o, ray_d, near, far, space, sampling, live_smpl_v, radius, dist, near_sur_dist, n_samples, u, chunk_size, live)
    o, t, batched = setup[0], setup[4], setup[8]
    R, S, dev = o.shape[0], t.shape[0], o.device
    out = _outputs(tuple(k for k in want if k in OUTPUTS) + (("rgb_map",) if "normal_map" in want else ()), R, S, dev)
    normal = torch.empty((R, S, 3), dtype=torch.float32, device=dev) if "normal" in want else None
    for r0, r1, pts, z, _, _ in _chunks(setup, space, live, False):
        ret = field.sdf_normal(pts, want=("sdf", "normal", "density"))
        n = ret["normal"]
        if normal is not None:
            normal[r0:r1] = n.view(r1 - r0, S, 3)
        unit = n / torch.linalg.norm(n, dim=-1, keepdim=True).clamp_min(1e-12) if "normal_map" in want else None
        _composite_into(ret["density"], unit, z, False, {k: v[r0:r1] for k, v in out.items()})
    if "normal_map" in want:
        out["normal_map"] = out.pop("rgb_map")
    if normal is not None:
        out["normal"] = normal
    out = {k: v for k, v in out.items() if k in want}
    return {k: v[None] for k, v in out.items()} if batched else out


def render_train(field_fn, beta, ray_o: torch.Tensor, ray_d: torch.Tensor, near: torch.Tensor, far: torch.Tensor, *, space: str = "cano",
                 sampling: str = "smpl", live_smpl_v: Optional[torch.Tensor] = None, radius: float = 0.1, dist: Optional[torch.Tensor] = None,
                 near_sur_dist: Optional[float] = None, n_samples: int = 64, u: Optional[torch.Tensor] = None, chunk_size: Optional[int] = None,
                 dir_noise: Optional[torch.Tensor] = None, mask_within_patch: Optional[torch.Tensor] = None, white_bkgd: bool = False,
                 live: Optional[dict] = None, want=("rgb_map", "acc_map"), hands: Optional[dict] = None):
    """``TemplateNet.render`` in training mode for one batch element, differentiable with respect to whatever ``field_fn`` and ``beta``
    hold: ``render``'s rays, samplings, spaces and checks, then per chunk

    ``field_fn(cano_pts [N, 3], viewdirs [N, 3]) -> (sdf [N, 1] or [N], color [N, 3])``, any differentiable callable
    (``template_train.TemplateFieldModule``, whose forward and reverse pass are this project's kernels, or any torch module), ``laplace_density(sdf, beta)`` and ``composite``.

    ``u`` [R, S] perturbs the samples (``perturb = self.training``) and ``dir_noise`` [R * S, 3] (the reference's ``randn * 0.1``) is added
    to the unit view directions, which are normalised again (``template.py:358-362``); both are the caller's random numbers, and
    without them nothing is perturbed.  ``chunk_size`` None takes all rays in one chunk, as the reference does in training.  Posed
    space maps the samples without a graph (the reference's ``transform_live2cano`` is under ``no_grad`` for the points it returns).
    ``mask_within_patch`` [P] (bool, R of them set): ``rgb_map`` / ``acc_map`` are scattered into zeros of length P
    (``template.py:394-403``); the other maps stay per ray.

    -> dict of the maps of ``want`` plus ``cano_pts`` [R * S, 3] (detached: a caller forms its own eikonal term there), ``z_vals`` [R, S]
    and ``mask_within_patch`` as given.  ``hands=`` is refused: the hand fusion has no backward."""
    if hands is not None:
        raise ValueError("hands: the hand fusion's backward is not built; render_train renders the body field alone")
    if not callable(field_fn):
        raise ValueError("field_fn must be callable: (cano_pts [N, 3], viewdirs [N, 3]) -> (sdf [N, 1], color [N, 3])")
    want = _want(want)
    n_rays = ray_o.shape[-2] if isinstance(ray_o, torch.Tensor) and ray_o.dim() >= 2 else 1
    setup = _march_setup(ray_o, ray_d, near, far, space, sampling, live_smpl_v, radius, dist, near_sur_dist, n_samples, u,
                         max(1, n_rays) if chunk_size is None else chunk_size, live)
    o, t, batched = setup[0], setup[4], setup[8]
    R, S, dev = o.shape[0], t.shape[0], o.device
    if dir_noise is not None:
        dir_noise = _f32(dir_noise[0] if batched and dir_noise.dim() == 3 else dir_noise, "dir_noise", (R * S, 3), dev)
    if mask_within_patch is not None:
        m = mask_within_patch
        if not isinstance(m, torch.Tensor) or m.device != dev or m.dtype != torch.bool or m.dim() not in (1, 2) or (m.dim() == 2 and m.shape[0] != 1):
            raise ValueError(f"mask_within_patch must be a bool tensor [P] (or [1, P]) on {dev}")
        m = m.reshape(-1)
        if int(m.sum()) != R:
            raise ValueError(f"mask_within_patch marks {int(m.sum())} rays, the batch has {R}")
    parts, pts_all, z_all = [], [], []
    for r0, r1, pts, z, dirs, _ in _chunks(setup, space, live, True):
        dirs = dirs.view(-1, 3)
        if dir_noise is not None:
            dirs = dirs + dir_noise[r0 * S:r1 * S]
            dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
        pts = pts.detach()
        sdf, color = field_fn(pts, dirs)
        parts.append(composite(laplace_density(sdf, beta), color, z, white_bkgd, want))
        pts_all.append(pts)
        z_all.append(z)
    if not parts:                                   # R = 0
        parts, pts_all, z_all = [_outputs(want, 0, S, dev)], [torch.empty((0, 3), device=dev)], [torch.empty((0, S), device=dev)]
    out = {k: torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in want}
    if mask_within_patch is not None:
        for k in ("rgb_map", "acc_map"):
            if k in out:
                full = torch.zeros((m.shape[0],) + tuple(out[k].shape[1:]), dtype=torch.float32, device=dev)
                out[k] = full.index_put((m,), out[k])
    out["cano_pts"] = torch.cat(pts_all) if len(pts_all) > 1 else pts_all[0]
    out["z_vals"] = torch.cat(z_all) if len(z_all) > 1 else z_all[0]
    if batched:
        out = {k: v[None] for k, v in out.items()}
    out["mask_within_patch"] = mask_within_patch
    return out


def training_loss(out: dict, color_gt: torch.Tensor, mask_gt: torch.Tensor, weights: dict):
    """The colour and mask terms of ``main_template.py:37-51`` on ``render_train``'s output: ``total = weights["color"] * L1(rgb_map,
    color_gt) + weights["mask"] * L1(acc_map, mask_gt)``, means over every element -> ``(total, {"color_loss": .., "mask_loss": ..})``
    (tensors: no host read).  With ``out["mask_within_patch"]`` the targets outside the patch count as 0 (``template.py:400-401``), without
    being modified.  A term whose map is missing from ``out`` is left out, as in the reference.  Plain torch."""
    total, terms = None, {}
    m = out.get("mask_within_patch")
    for name, key, gt, w in (("color_loss", "rgb_map", color_gt, "color"), ("mask_loss", "acc_map", mask_gt, "mask")):
        if key not in out:
            continue
        pred = out[key]
        gt = gt.reshape(pred.shape)
        if m is not None:
            keep = m.reshape(pred.shape[:-1] if key == "rgb_map" else pred.shape)
            gt = torch.where(keep[..., None] if key == "rgb_map" else keep, gt, torch.zeros_like(gt))
        terms[name] = torch.nn.functional.l1_loss(pred, gt)
        total = float(weights[w]) * terms[name] if total is None else total + float(weights[w]) * terms[name]
    if total is None:
        raise ValueError("out holds neither rgb_map nor acc_map")
    return total, terms
