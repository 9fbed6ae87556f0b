"""Camera rays and ray batches of the template stage, on the GPU (``include/ag_ray_select.h``): from a decoded frame on the device, a
camera and the posed bounding box to what ``template_render.render`` / ``render_train`` / ``training_loss`` take.

Re-host of the dataset side of the reference's ``utils/nerf_util.py``, which runs in numpy inside loader workers: ``get_rays``,
``get_near_far``, ``get_bound_2d_mask``, ``sample_randomly_for_nerf_rendering`` (``dataset/dataset_mv_rgb.py:199-211``),
``sample_patch_for_nerf_rendering`` and the whole-image rays of ``dataset/dataset_pose.py:338-357``.  Four kernels: classify every pixel
(outside the box's image-space mask / on the matte / off it), compact a class or flag array into ascending pixel lists (the order
``uv_img[mask]`` enumerates), and build ray, box near / far, hit flag and targets for a list of pixels; ``get_near_far`` alone for rays
the caller holds.  The float32 operations are stated one by one in the header and ``tests/ray_select_oracle.py`` restates them in numpy:
the results are equal bit for bit.

Host cost: the camera (3 x 3, 3 x 3, position: inverted in float64 on the host, rounded once to float32) and the eight projected box
corners go to the kernels by value.  ``candidates`` reads the two list lengths once; every sampling round, ``sample_patches``,
``image_rays`` and ``get_near_far`` read one hit count (the size of their result).  Nothing else leaves the device.  The random draws
are never a kernel's: they are ``picks`` or ``torch.randperm`` / ``torch.rand`` with the caller's ``generator``.

The box's mask is the closed union of the six projected faces by integer edge functions on the rounded corners (header): the project's
own definition of what the reference draws with ``cv2.fillPoly``; parity with OpenCV's scan conversion is not pinned.

NOT built: ``sample_randomly_for_nerf_rendering_wSideViewMask``, ``resize_factor != 1`` of the patch sampler, several views per launch.
Every image and ray tensor must be on the GPU; there is no host path and no PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .mlp_blob import ptr as _ptr, stream as _stream

MAX_CORNER = 1 << 29                                                                           # include/ag_ray_select.h
BATCH_KEYS = ("uv", "ray_o", "ray_d", "near", "far", "color_gt", "mask_gt", "depth_gt", "dist")


# ---- host side: the camera and the corners --------------------------------------------------------------------------------------------
def _host(x, shape, name: str) -> np.ndarray:
    """A camera matrix or the bounds as float64 on the host (a device tensor is read back: they are passed to the kernels by value)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} must be {list(shape)}, got {list(a.shape)}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds a value that is not finite")
    return a


def _matrices(extr, intr):
    extr, intr = _host(extr, (4, 4), "extr"), _host(intr, (3, 3), "intr")
    try:
        return extr, intr, np.linalg.inv(extr), np.linalg.inv(intr)
    except np.linalg.LinAlgError:
        raise ValueError("extr and intr must be invertible") from None


def _bounds(bounds) -> np.ndarray:
    b = _host(bounds, (2, 3), "bounds")
    if (b[1] < b[0]).any():
        raise ValueError("bounds must be [[min x, y, z], [max x, y, z]]")
    return b


def _frame(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise ValueError(f"bad frame size H = {H}, W = {W}")
    return H, W


def _camera(extr, intr, bounds, H: int = 0, W: int = 0) -> _lib.AgRayCamera:
    extr, intr, inv_extr, inv_intr = _matrices(extr, intr)
    c = _lib.AgRayCamera()
    c.inv_intr[:] = np.float32(inv_intr).reshape(-1).tolist()
    c.inv_rot[:] = np.float32(inv_extr[:3, :3]).reshape(-1).tolist()
    c.cam[:] = np.float32(inv_extr[:3, 3]).tolist()
    c.fx, c.fy, c.cx, c.cy = (float(np.float32(v)) for v in (intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]))
    c.bounds[:] = np.float32(np.zeros(6) if bounds is None else _bounds(bounds).reshape(-1)).tolist()
    c.W, c.H = W, H
    return c


def project_corners(bounds, intr, extr) -> np.ndarray:
    """The box's eight corners (``get_bound_corners``' order) as ``nerf_util.project`` places them, in float64, rounded with ``np.round``
    -> int64 [8, 2].  ``ValueError`` when a corner has camera-space ``z <= 0``: the reference divides by ``z`` there and draws nonsense."""
    b, K, RT = _bounds(bounds), _host(intr, (3, 3), "intr"), _host(extr, (4, 4), "extr")
    corners = np.array([[b[(i >> 2) & 1, 0], b[(i >> 1) & 1, 1], b[i & 1, 2]] for i in range(8)])
    xyz = corners @ RT[:3, :3].T + RT[:3, 3:].T
    if (xyz[:, 2] <= 0).any():
        raise ValueError("a corner of the box lies behind the camera (camera-space z <= 0): its projection means nothing")
    xyz = xyz @ K.T
    xy = np.round(xyz[:, :2] / xyz[:, 2:])
    if not (np.abs(xy) <= MAX_CORNER).all():
        raise ValueError("a projected corner lies beyond 2^29 pixels")
    return xy.astype(np.int64)


# ---- checks of device tensors ---------------------------------------------------------------------------------------------------------
def _gpu(t, name: str, dtypes, shape, dev=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (there is no host path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and int(s) != w for s, w in zip(t.shape, shape)):
        raise ValueError(f"{name} must be [{', '.join('N' if w is None else str(w) for w in shape)}], got {tuple(t.shape)}")
    return t.detach().contiguous()


def _bytes(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else (t.view(torch.uint8) if t.dtype == torch.bool else t)


_FLAG = (torch.bool, torch.uint8)


def _mask_pair(mask_img, unsample):
    mask = _gpu(mask_img, "mask_img", _FLAG, (None, None))
    H, W = _frame(*mask.shape)
    if unsample is not None:
        unsample = _gpu(unsample, "unsample_region_mask", _FLAG, (H, W), mask.device)
    return mask, unsample, H, W


def _images(color_img, mask_img, depth_img, unsample):
    mask, unsample, H, W = _mask_pair(mask_img, unsample)
    color = _gpu(color_img, "color_img", (torch.float32,), (H, W, 3), mask.device)
    depth = None if depth_img is None else _gpu(depth_img, "depth_img", (torch.float32,), (H, W), mask.device)
    return color, mask, depth, unsample, H, W


def _ratio(r) -> float:
    r = float(r)
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"inside_ratio must be in [0, 1], got {r}")
    return r


# ---- the launches ---------------------------------------------------------------------------------------------------------------------
def _classify(corners: np.ndarray, H: int, W: int, mask, unsample, dev) -> torch.Tensor:
    cls = torch.empty((H, W), dtype=torch.uint8, device=dev)
    xy = (_lib.c_i32 * 16)(*[int(v) for v in corners.reshape(-1)])
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ag_ray_classify(xy, H, W, _ptr(_bytes(mask)), _ptr(_bytes(unsample)), _ptr(cls), _stream(dev)), "ag_ray_classify")
    return cls


def _compact(flags: torch.Tensor, two: bool):
    """uint8 flags [n] -> (list of the 1s, list of the 2s or None, counts int32 [2] on the device); the lists hold n entries, of which the
    first ``counts`` are written."""
    n, dev = flags.numel(), flags.device
    L = _lib.lib()
    one = torch.empty(n, dtype=torch.int32, device=dev)
    other = torch.empty(n, dtype=torch.int32, device=dev) if two else None
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws_bytes = int(L.ag_ray_compact_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.ag_ray_compact(_ptr(flags), n, _ptr(one), _ptr(other), _ptr(counts), _ptr(ws), ws_bytes, _stream(dev)), "ag_ray_compact")
    return one, other, counts


def _build(cam: _lib.AgRayCamera, n: int, dev, pix=None, uv_in=None, images=None, box: bool = True, want_uv: bool = True) -> dict:
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"ray_o": f(n, 3), "ray_d": f(n, 3)}
    if want_uv:
        out["uv"] = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if box:
        out.update(near=f(n), far=f(n), hit=torch.empty(n, dtype=torch.uint8, device=dev))
    color = mask = depth = None
    if images is not None:
        color, mask, depth = images
        out.update(color_gt=f(n, 3), mask_gt=f(n), depth_gt=f(n), dist=f(n))
    if n:
        g = out.get
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ag_ray_build(ctypes.byref(cam), _ptr(pix), _ptr(uv_in), n, _ptr(color), _ptr(_bytes(mask)), _ptr(depth), _ptr(g("uv")),
                                               _ptr(out["ray_o"]), _ptr(out["ray_d"]), _ptr(g("near")), _ptr(g("far")), _ptr(g("hit")), _ptr(g("color_gt")),
                                               _ptr(g("mask_gt")), _ptr(g("depth_gt")), _ptr(g("dist")), _stream(dev)), "ag_ray_build")
    return out


def _kept(flags: torch.Tensor):
    """Ascending entries of the set flags as int64 indices: one compaction and ONE host read (their number)."""
    one, _, counts = _compact(flags, False)
    return one[:int(counts[0])].to(torch.int64)


# ---- public -----------------------------------------------------------------------------------------------------------------------------
def get_rays(uv: torch.Tensor, extr, intr):
    """``nerf_util.get_rays``: integer pixels ``uv`` [n, 2] = (x, y) on the GPU (int32 or int64; they enter WITHOUT + 0.5) and the host
    matrices ``extr`` [4, 4], ``intr`` [3, 3] -> ``(ray_d [n, 3], ray_o [n, 3])`` float32."""
    uv = _gpu(uv, "uv", (torch.int32, torch.int64), (None, 2))
    cam = _camera(extr, intr, None)
    out = _build(cam, uv.shape[0], uv.device, uv_in=uv.to(torch.int32).contiguous(), box=False, want_uv=False)
    return out["ray_d"], out["ray_o"]


def get_near_far(bounds, ray_o: torch.Tensor, ray_d: torch.Tensor):
    """``nerf_util.get_near_far``: the rays against ``bounds`` [2, 3] padded by 1 cm -> ``(near [K], far [K], mask_at_box [n] bool)``; near
    and far cover the K rays that cross exactly two faces, as the reference returns them.  One host read (K)."""
    o = _gpu(ray_o, "ray_o", (torch.float32,), (None, 3))
    d = _gpu(ray_d, "ray_d", (torch.float32,), (o.shape[0], 3), o.device)
    b = (_lib.c_f * 6)(*np.float32(_bounds(bounds).reshape(-1)).tolist())
    n, dev = o.shape[0], o.device
    near, far = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    hit = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ag_ray_box_near_far(b, _ptr(o), _ptr(d), n, _ptr(near), _ptr(far), _ptr(hit), _stream(dev)), "ag_ray_box_near_far")
    keep = _kept(hit)
    return near[keep], far[keep], hit.view(torch.bool)


def bound_mask(bounds, intr, extr, H: int, W: int, device="cuda") -> torch.Tensor:
    """``get_bound_2d_mask(bounds, K, pose, H, W) > 0`` -> bool [H, W] on ``device`` (argument order as in the reference)."""
    H, W = _frame(H, W)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the mask is drawn on the GPU (there is no host path), got device {dev}")
    corners = project_corners(bounds, intr, extr)
    return _classify(corners, H, W, None, None, dev).view(torch.bool)


@dataclass
class Candidates:
    """``inside`` / ``outside``: ascending flat pixels (``y * W + x``, int32) inside the box's mask, outside the unsample region, on / off
    the matte: the reference's ``inside_uv`` / ``outside_uv`` in their order.  ``bound_mask`` [H, W] bool: the reference's ``bound_mask``
    AFTER the unsample region was taken out of it.  ``counts``: the two lengths, int32 [2] on the device."""
    inside: torch.Tensor
    outside: torch.Tensor
    bound_mask: torch.Tensor
    counts: torch.Tensor
    H: int
    W: int


def _candidates(mask, unsample, H, W, corners) -> Candidates:
    cls = _classify(corners, H, W, mask, unsample, mask.device)
    inside, outside, counts = _compact(cls.view(-1), True)
    n_in, n_out = counts.tolist()                                   # the one host read
    return Candidates(inside[:n_in].clone(), outside[:n_out].clone(), cls != 0, counts, H, W)


def candidates(mask_img: torch.Tensor, bounds, extr, intr, unsample_region_mask: Optional[torch.Tensor] = None) -> Candidates:
    """The two pixel lists a batch is drawn from.  ``mask_img`` [H, W] (bool or uint8, non-zero = subject), ``unsample_region_mask``
    likewise (non-zero = never sampled).  Reads the two counts to the host once."""
    mask, unsample, H, W = _mask_pair(mask_img, unsample_region_mask)
    return _candidates(mask, unsample, H, W, project_corners(bounds, intr, extr))


def _index_list(p, k: int, n: int, what: str, dev) -> torch.Tensor:
    """A pick list on the host -> int64 device indices; ``ValueError`` unless it holds ``k`` distinct values of 0 .. n - 1."""
    a = np.asarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what} must be a flat list of integers")
    a = a.astype(np.int64)
    if a.size != k:
        raise ValueError(f"{what} holds {a.size} indices, the round draws {k}")
    if a.size and (a.min() < 0 or a.max() >= n or np.unique(a).size != a.size):
        raise ValueError(f"{what} must hold distinct indices of 0 .. {n - 1} (a draw without replacement)")
    return torch.from_numpy(a).to(dev)


def _draw(n: int, k: int, generator, dev) -> torch.Tensor:
    if generator is None:
        return torch.randperm(n, device=dev)[:k]
    return torch.randperm(n, generator=generator, device=generator.device)[:k].to(dev)


def sample_randomly(color_img, mask_img, depth_img, extr, intr, live_bounds, sample_num: int = 1024, inside_ratio: float = 0.5,
                    unsample_region_mask=None, generator: Optional[torch.Generator] = None, picks=None) -> dict:
    """``sample_randomly_for_nerf_rendering``: ``color_img`` [H, W, 3] float32, ``mask_img`` [H, W] bool / uint8, ``depth_img`` [H, W] float32
    or None (zeros), all on the GPU -> the reference's dict on the device: ``uv`` int32 [S, 2], ``ray_o``, ``ray_d`` [S, 3], ``near``, ``far``,
    ``mask_gt``, ``depth_gt``, ``dist`` [S], ``color_gt`` [S, 3] (zero off the matte), with S = ``sample_num`` (a round draws what is missing and keeps no more than it drew).

    The reference's rounds, ``while count < sample_num``: draw ``int(rest * inside_ratio)`` inside pixels and the remaining outside
    pixels WITHOUT replacement, keep the rays that hit the box.  A round costs one host read (its hit count).  The draws are ``picks``,
    a list with one ``(inside indices, outside indices)`` pair of host integer lists per round (indices into the candidate lists), or
    ``torch.randperm(n, generator=generator)[:k]`` (on the generator's device; without one, the GPU's default generator).  Asking for
    more than a list holds raises ``ValueError``, as ``np.random.choice`` does; so do picks that run out, and a round in which no ray hits
    (the reference would draw for ever)."""
    color, mask, depth, unsample, H, W = _images(color_img, mask_img, depth_img, unsample_region_mask)
    sample_num, ratio = int(sample_num), _ratio(inside_ratio)
    if sample_num < 1:
        raise ValueError(f"sample_num must be positive, got {sample_num}")
    corners = project_corners(live_bounds, intr, extr)
    cam = _camera(extr, intr, live_bounds, H, W)
    dev = mask.device
    cand = _candidates(mask, unsample, H, W, corners)
    n_in, n_out = cand.inside.numel(), cand.outside.numel()
    kept, count, rnd = [], 0, 0
    while count < sample_num:
        rest = sample_num - count
        k_in = int(rest * ratio)
        k_out = rest - k_in
        if k_in > n_in or k_out > n_out:
            raise ValueError(f"round {rnd} draws {k_in} inside and {k_out} outside pixels without replacement, the lists hold {n_in} and {n_out}")
        if picks is not None:
            if rnd >= len(picks):
                raise ValueError(f"picks holds {len(picks)} rounds, round {rnd} is needed ({count} of {sample_num} rays so far)")
            ii = _index_list(picks[rnd][0], k_in, n_in, f"picks[{rnd}][0]", dev)
            oi = _index_list(picks[rnd][1], k_out, n_out, f"picks[{rnd}][1]", dev)
        else:
            ii, oi = _draw(n_in, k_in, generator, dev), _draw(n_out, k_out, generator, dev)
        pix = torch.cat([cand.inside[ii], cand.outside[oi]])
        hit = _build(cam, rest, dev, pix=pix, want_uv=False)["hit"]
        keep = _kept(hit)
        if keep.numel() == 0:
            raise ValueError(f"round {rnd}: none of the {rest} drawn rays hits the box")
        kept.append(pix[keep])
        count += keep.numel()
        rnd += 1
    pix = torch.cat(kept) if len(kept) > 1 else kept[0]
    out = _build(cam, pix.numel(), dev, pix=pix.contiguous(), images=(color, mask, depth))
    return {k: out[k] for k in BATCH_KEYS}


def sample_patches(color_img, mask_img, depth_img, extr, intr, live_bounds, patch_num: int = 2, patch_size: int = 32, inside_ratio: float = 0.5,
                   unsample_region_mask=None, resize_factor: float = 1.0, generator: Optional[torch.Generator] = None, picks=None) -> dict:
    """``sample_patch_for_nerf_rendering`` with ``resize_factor = 1`` (any other value is refused).  Per patch: with probability
    ``inside_ratio`` a centre from the inside list, else from the outside list; the patch starts at ``clip(centre - patch_size // 2, 0, size
    - patch_size)`` on both axes.  -> dict on the device with ``uv`` [P, 2], ``color_gt`` [P, 3], ``mask_gt``, ``depth_gt`` [P] over all
    ``P = patch_num * patch_size ** 2`` pixels, ``mask_within_patch`` [P] bool = inside the box's mask (unsample region taken out) and
    hit, and ``ray_o``, ``ray_d``, ``near``, ``far``, ``dist`` over the marked pixels only.  The dict feeds
    ``render_train(mask_within_patch=...)`` and ``training_loss`` as it is.

    ``picks``: one ``(use_inside, index)`` pair per patch; otherwise ``torch.rand`` / ``torch.randint`` with ``generator`` (host draws; a GPU
    generator's draws are read back once).  The centres and patch origins are computed on the device; the call's host reads are the
    candidate counts and the number of marked pixels."""
    if float(resize_factor) != 1.0:
        raise ValueError(f"resize_factor = {resize_factor}: only 1 is built")
    color, mask, depth, unsample, H, W = _images(color_img, mask_img, depth_img, unsample_region_mask)
    patch_num, ps, ratio = int(patch_num), int(patch_size), _ratio(inside_ratio)
    if patch_num < 1 or ps < 1:
        raise ValueError(f"patch_num and patch_size must be positive, got {patch_num} and {patch_size}")
    if ps > H or ps > W:
        raise ValueError(f"patch_size {ps} is larger than the frame {H} x {W}")
    if picks is not None and len(picks) < patch_num:
        raise ValueError(f"picks holds {len(picks)} patches, {patch_num} are drawn")
    corners = project_corners(live_bounds, intr, extr)
    cam = _camera(extr, intr, live_bounds, H, W)
    dev = mask.device
    cand = _candidates(mask, unsample, H, W, corners)
    if picks is None:
        gdev = generator.device if generator is not None else "cpu"
        r = torch.rand(2 * patch_num, generator=generator, device=gdev).cpu().tolist()
    centres = []
    for i in range(patch_num):
        use_inside = bool(picks[i][0]) if picks is not None else r[2 * i] < ratio
        lst = cand.inside if use_inside else cand.outside
        n = lst.numel()
        if n == 0:
            raise ValueError(f"patch {i} takes its centre from the {'inside' if use_inside else 'outside'} list, which is empty")
        index = int(picks[i][1]) if picks is not None else min(int(r[2 * i + 1] * n), n - 1)
        if not 0 <= index < n:
            raise ValueError(f"patch {i}: index {index} is outside the list's 0 .. {n - 1}")
        centres.append(lst[index])
    c = torch.stack(centres).to(torch.int64)                                                   # [patch_num], on the device
    half = ps // 2
    u0 = (c % W - half).clamp(0, W - ps)
    v0 = (torch.div(c, W, rounding_mode="floor") - half).clamp(0, H - ps)
    step = torch.arange(ps, device=dev)
    pix = ((v0[:, None, None] + step[None, :, None]) * W + (u0[:, None, None] + step[None, None, :])).reshape(-1)
    out = _build(cam, pix.numel(), dev, pix=pix.to(torch.int32).contiguous(), images=(color, mask, depth))
    within = cand.bound_mask.view(-1)[pix] & out["hit"].view(torch.bool)
    keep = _kept(within.view(torch.uint8))
    ret = {k: out[k] for k in ("uv", "color_gt", "mask_gt", "depth_gt")}
    ret.update({k: out[k][keep] for k in ("ray_o", "ray_d", "near", "far", "dist")})
    ret["mask_within_patch"] = within
    return ret


def image_rays(extr, intr, img_w: int, img_h: int, live_bounds, device="cuda") -> dict:
    """``dataset_pose.py:338-357``: a ray for every pixel of an ``img_w`` x ``img_h`` image, those that hit the box kept in row-major order ->
    ``uv`` int32 [R, 2], ``ray_o``, ``ray_d`` [R, 3], ``near``, ``far`` [R], ``dist`` [R] zeros, ``img_w``, ``img_h``.  One host read (R)."""
    H, W = _frame(img_h, img_w)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the rays are built on the GPU (there is no host path), got device {dev}")
    cam = _camera(extr, intr, live_bounds, H, W)
    out = _build(cam, H * W, dev)
    keep = _kept(out["hit"])
    ret = {k: out[k][keep] for k in ("uv", "ray_o", "ray_d", "near", "far")}
    ret["dist"] = torch.zeros_like(ret["near"])
    ret["img_w"], ret["img_h"] = W, H
    return ret


def render_image(field, extr, intr, img_w: int, img_h: int, bounds, **render_kwargs) -> dict:
    """An image of the template field from a camera: ``image_rays`` -> ``template_render.render(field, ..., **render_kwargs)`` -> ``rgb``
    [H, W, 3] and ``acc`` [H, W], scattered back through ``uv``.  Pixels without a ray take the background: 0, or 1 with
    ``white_bkgd=True``; their ``acc`` is 0.  The values are those of ``render`` on the same rays, bit for bit.  ``render_kwargs``: everything
    of ``render`` but the rays and ``want`` (``sampling="smpl"`` needs ``live_smpl_v``, as there)."""
    from .template_render import render
    from .template_field import TemplateField
    if not isinstance(field, TemplateField):
        raise ValueError("field must be a TemplateField")
    if "want" in render_kwargs:
        raise ValueError("render_image renders rgb_map and acc_map; want is not the caller's")
    dev = next((t.device for t in render_kwargs.values() if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))
    rays = image_rays(extr, intr, img_w, img_h, bounds, device=dev)
    H, W = rays["img_h"], rays["img_w"]
    rgb = torch.full((H * W, 3), 1.0 if render_kwargs.get("white_bkgd") else 0.0, dtype=torch.float32, device=dev)
    acc = torch.zeros(H * W, dtype=torch.float32, device=dev)
    if rays["uv"].shape[0]:
        out = render(field, rays["ray_o"], rays["ray_d"], rays["near"], rays["far"], want=("rgb_map", "acc_map"), **render_kwargs)
        at = rays["uv"][:, 1].to(torch.int64) * W + rays["uv"][:, 0].to(torch.int64)
        rgb[at] = out["rgb_map"]
        acc[at] = out["acc_map"]
    return {"rgb": rgb.view(H, W, 3), "acc": acc.view(H, W), "uv": rays["uv"]}
