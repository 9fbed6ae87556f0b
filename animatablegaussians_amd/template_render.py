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

NOT here: any backward, the training-mode noise on the view directions, the
scattering through ``mask_within_patch`` and the dataset-side ray selection of ``nerf_util`` (``get_rays``, ``get_near_far``, patch
sampling): the caller brings the rays and the box near / far, as the reference's batch does.  Near / far is pinned to the header's
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
    named in ``want``, ``depth_map`` [R], ``disp_map`` [R], ``weights`` [R, S].  alpha is formed inside the kernel."""
    want = _want(want)
    z = _f32(z_vals, "z_vals", (None, None))
    R, S = z.shape
    _samples(S)
    if not isinstance(density, torch.Tensor) or density.numel() != R * S:
        raise ValueError(f"density must hold {R} x {S} values, got {tuple(density.shape) if isinstance(density, torch.Tensor) else type(density)}")
    density = _f32(density.reshape(R, S), "density", (R, S), z.device)
    if color is None:
        if "rgb_map" in want:
            raise ValueError("rgb_map needs color")
    else:
        if not isinstance(color, torch.Tensor) or color.numel() != R * S * 3 or color.shape[-1] != 3:
            raise ValueError(f"color must hold {R} x {S} x 3 values, got {tuple(color.shape) if isinstance(color, torch.Tensor) else type(color)}")
        color = _f32(color.reshape(R, S, 3), "color", (R, S, 3), z.device) if "rgb_map" in want else None
    out = _outputs(want, R, S, z.device)
    _composite_into(density, color, z, white_bkgd, out)
    return {k: v for k, v in out.items() if k in want}


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
