"""Training targets from decoded frames, on the GPU (``include/ag_targets.h``): the float colour, the subject mask and the boundary band
that ``losses.training_loss`` reads, plus the mask's bounding box.

Re-host of what the reference's loader computes on host arrays for every view of every step (``dataset/dataset_mv_rgb.py:182-198``):
``color_img = (color_img / 255.).astype(np.float32)`` and ``get_boundary_mask`` (``:263-285``: threshold the matte at 128, ``cv.erode``
and ``cv.dilate`` with a ``kernel_size`` box, the band where the two differ, plus the soft-matte pixels ``5 < matte < 250``).  Here the
frame goes to the device as the 4 bytes per pixel the files hold and one kernel launch writes all three images for all views; the
results equal the reference's bit for bit (``tests/targets_oracle.py``).  Channel order is kept (BGR in, BGR out, as ``cv.imread``
leaves it; ``losses.lpips_loss`` flips it).

Arguments are checked before anything touches the GPU.  The kernel has no host path: ``device`` must be a GPU.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .losses import bbox_from_profiles

MAX_KERNEL_SIZE = 15


def _uint8_tensor(x, name: str) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise TypeError(f"{name} must be uint8, got {x.dtype}")
        return torch.from_numpy(np.ascontiguousarray(x))
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.uint8:
            raise TypeError(f"{name} must be uint8, got {x.dtype}")
        return x
    raise TypeError(f"{name} must be a numpy array or a tensor, got {type(x).__name__}")


def _check(color, matte, kernel_size, device):
    """-> (color or None, matte, batched, device); every TypeError / ValueError of the public functions comes from here."""
    matte = _uint8_tensor(matte, "matte_img")
    if color is not None:
        color = _uint8_tensor(color, "color_img")
        if color.dim() not in (3, 4) or color.shape[-1] != 3:
            raise ValueError(f"color_img must be [H, W, 3] or [V, H, W, 3], got {tuple(color.shape)}")
        if matte.dim() == color.dim() and matte.shape[-1] == 3:
            raise ValueError(f"matte_img must have one channel ([H, W] or [V, H, W]), got the 3-channel {tuple(matte.shape)}")
        if tuple(matte.shape) != tuple(color.shape[:-1]):
            raise ValueError(f"matte_img {tuple(matte.shape)} does not match color_img {tuple(color.shape)}")
    elif matte.dim() not in (2, 3):
        raise ValueError(f"matte_img must be [H, W] or [V, H, W], got {tuple(matte.shape)}")
    if matte.numel() == 0:
        raise ValueError(f"empty image: matte_img is {tuple(matte.shape)}")
    if isinstance(kernel_size, bool) or int(kernel_size) != kernel_size or kernel_size % 2 == 0 or not 1 <= kernel_size <= MAX_KERNEL_SIZE:
        raise ValueError(f"kernel_size must be odd and in 1..{MAX_KERNEL_SIZE}, got {kernel_size}")
    on_gpu = [t.device for t in (color, matte) if t is not None and t.is_cuda]
    dev = on_gpu[0] if on_gpu else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"targets are prepared on the GPU (there is no host path), got device {dev}")
    if any(d != dev for d in on_gpu):
        raise ValueError(f"color_img is on {color.device}, matte_img on {matte.device}")
    return color, matte, matte.dim() == 3, dev


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    t = t.contiguous()
    return t if t.is_cuda else t.to(dev, non_blocking=t.is_pinned())


def _run(color, matte, kernel_size: int, profiles: bool, dev):
    """[V, H, W(, 3)] uint8 on ``dev`` -> (color float32 or None, mask uint8, boundary uint8, profiles uint8 [V (H + W)] or None)."""
    V, H, W = (int(s) for s in matte.shape)
    color_f = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev) if color is not None else None
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    boundary = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    prof = torch.empty(V * (H + W), dtype=torch.uint8, device=dev) if profiles else None
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None  # noqa: E731
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ag_prepare_targets(p(color), p(matte), V, H, W, int(kernel_size), p(color_f), p(mask), p(boundary),
                                                 p(prof), p(prof, V * H), _lib.stream(dev)),
                   "ag_prepare_targets")
    return color_f, mask, boundary, prof


def prepare_targets(color_img, matte_img, *, kernel_size: int = 5, bbox: bool = True, device="cuda") -> dict:
    """One view ``color_img`` [H, W, 3], ``matte_img`` [H, W], or a stack [V, H, W, 3], [V, H, W]; uint8 numpy arrays, CPU tensors
    (uploaded as uint8, without blocking when pinned) or tensors on the GPU -> the items of ``losses.training_loss``:

        ``color_img`` float32 [.., H, W, 3] = colour / 255     ``mask_img`` bool [.., H, W] = matte > 128
        ``boundary_mask_img`` bool [.., H, W]: the reference's ``get_boundary_mask(matte, kernel_size)``
        ``mask_bbox`` (with ``bbox``): ``losses.mask_bbox`` of the mask, a tuple, or a list of tuples for a stack

    Runs on the current stream of the inputs' device (``device`` when both are on the host).  ``bbox=True`` reads back the mask's row
    and column profiles, H + W bytes per view: the call's one synchronisation; a view with an empty mask raises ``ValueError``.  With
    ``bbox=False`` nothing is read back and there is no ``mask_bbox`` key.  ``TypeError`` for anything but uint8, ``ValueError`` for
    shapes that do not match, a 3-channel matte, or a ``kernel_size`` that is even or outside 1..15."""
    color, matte, batched, dev = _check(color_img, matte_img, kernel_size, device)
    if color is None:
        raise TypeError("color_img must be a numpy array or a tensor, got NoneType")
    color, matte = _upload(color, dev), _upload(matte, dev)
    if not batched:
        color, matte = color[None], matte[None]
    color_f, mask, boundary, prof = _run(color, matte, kernel_size, bool(bbox), dev)
    out = {"color_img": color_f, "mask_img": mask.view(torch.bool), "boundary_mask_img": boundary.view(torch.bool)}
    if not batched:
        out = {k: t[0] for k, t in out.items()}
    if bbox:
        V, H, W = matte.shape
        host = prof.cpu().numpy()
        rows, cols = host[:V * H].reshape(V, H), host[V * H:].reshape(V, W)
        boxes = []
        for v in range(V):
            if not rows[v].any():
                raise ValueError(f"view {v}: the mask is empty (no matte value above 128), it has no bounding box")
            boxes.append(bbox_from_profiles(rows[v], cols[v]))
        out["mask_bbox"] = boxes if batched else boxes[0]
    return out


def boundary_mask(matte_img, kernel_size: int = 5, device="cuda"):
    """The reference's static ``get_boundary_mask`` alone -> ``(boundary_mask, mask)``, bool, in the shape of ``matte_img`` ([H, W] or
    [V, H, W], uint8): for callers that already hold float colour.  No read-back."""
    _, matte, batched, dev = _check(None, matte_img, kernel_size, device)
    matte = _upload(matte, dev)
    _, mask, boundary, _ = _run(None, matte if batched else matte[None], kernel_size, False, dev)
    mask, boundary = mask.view(torch.bool), boundary.view(torch.bool)
    return (boundary, mask) if batched else (boundary[0], mask[0])
