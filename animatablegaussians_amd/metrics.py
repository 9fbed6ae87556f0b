"""Scores of rendered views, on the GPU (``include/ag_metrics.h``): PSNR, SSIM and LPIPS on the evaluation crop.

What the reference's ``eval/score.py`` computes on host arrays with scikit-image, OpenCV and its LPIPS module, and what
``eval/comparison_body_only_avatars.py:45-71`` accumulates per frame:

    psnr_ssim (one kernel pass over both images)  |  eval_crop -> lpips_score  |  Metrics.update / result

SSIM is ``skimage.metrics.structural_similarity`` restated (the formulas are in the header): a uniform window of ``win_size`` taps
or, with ``gaussian_weights``, scipy's 11-tap Gaussian of sigma 1.5; the mean over the centres whose whole window lies inside the
image, over all channels.  PSNR is ``10 log10(R^2 / mse)`` with the float64 mean over all elements.

NOT pinned: neither scikit-image nor OpenCV is available to this package, so parity with the two libraries themselves is not
claimed.  The contract is the float64 restatement in ``tests/metrics_oracle.py`` (``scipy.ndimage`` filters and a bilinear resize
written out); where scikit-image can be imported, ``tests/test_metrics_cpu.py`` compares the oracle with it.

``psnr_ssim`` needs its images on the GPU; there is no host path.  ``eval_crop`` is plain torch and runs wherever its images are.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .losses import bbox_from_profiles

TILE_H, TILE_W = 16, 32      # AG_METRICS_TILE_H / _W of include/ag_metrics.h: the block of window centres one workgroup owns
MAX_TAPS = 11
EVAL_PAD = 50                # eval/score.py:32


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def gaussian_taps(sigma: float = 1.5, truncate: float = 3.5) -> np.ndarray:
    """scipy's ``_gaussian_kernel1d``: radius ``int(truncate * sigma + 0.5)``, ``exp(-i^2 / 2 sigma^2)`` normalised to sum 1."""
    radius = int(truncate * sigma + 0.5)
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-0.5 / (sigma * sigma) * i * i)
    return k / k.sum()


def window_taps(win_size: int = 7, gaussian_weights: bool = False) -> np.ndarray:
    """The 1-D taps of the separable window (float64): ``1 / win_size`` each, or the Gaussian (``win_size`` is then ignored, as
    scikit-image ignores it)."""
    if gaussian_weights:
        return gaussian_taps()
    if int(win_size) != win_size or win_size % 2 == 0 or not 3 <= win_size <= MAX_TAPS:
        raise ValueError(f"win_size must be odd and in 3..{MAX_TAPS}, got {win_size}")
    return np.full(int(win_size), 1.0 / int(win_size), np.float64)


def _check_pair(pred, gt, n_taps) -> Tuple[torch.Tensor, torch.Tensor]:
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if pred.shape != gt.shape:
        raise ValueError(f"pred and gt must have the same shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.dim() not in (3, 4):
        raise ValueError(f"images must be [H, W, C] or [B, H, W, C], got {tuple(pred.shape)}")
    H, W, C = pred.shape[-3:]
    if not 1 <= C <= 4:
        raise ValueError(f"1 to 4 channels (last axis), got {C}")
    if H < n_taps or W < n_taps:
        raise ValueError(f"images of {H} x {W} are smaller than the window of {n_taps}")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("pred and gt must be contiguous")
    if not (pred.is_cuda and gt.is_cuda) or pred.device != gt.device:
        raise ValueError("pred and gt must be on the same GPU (there is no host path)")
    return (pred[None], gt[None]) if pred.dim() == 3 else (pred, gt)


def psnr_ssim_sums(pred: torch.Tensor, gt: torch.Tensor, *, data_range: float = 1.0, win_size: int = 7, gaussian_weights: bool = False,
                   use_sample_covariance: bool = True, K1: float = 0.01, K2: float = 0.03, return_map: bool = False):
    """The kernel's own outputs -> (sq_err_sum [B], ssim_sum [B], n_elements, n_centres, map or None): the float64 sum of squared
    errors over the H W C elements of each image and the float64 sum of S over its (H-2p)(W-2p) C window centres."""
    taps = window_taps(win_size, gaussian_weights)
    n = int(taps.size)
    x, y = _check_pair(pred, gt, n)
    B, H, W, C = x.shape
    p = (n - 1) // 2
    dev = x.device
    cov_norm = n * n / (n * n - 1.0) if use_sample_covariance else 1.0
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    sq = torch.empty(B, dtype=torch.float64, device=dev)
    ss = torch.empty(B, dtype=torch.float64, device=dev)
    smap = torch.empty(B, H - 2 * p, W - 2 * p, C, dtype=torch.float32, device=dev) if return_map else None
    if B > 0:
        L = _lib.lib()
        ws = torch.empty(L.ag_psnr_ssim_workspace_bytes(B, H, W, n), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.ag_psnr_ssim(_p(x), _p(y), B, H, W, C, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, cov_norm, C1, C2,
                                      _p(sq), _p(ss), _p(smap), _p(ws), ws.numel(),
                                      _lib.stream(dev)), "ag_psnr_ssim")
    return sq, ss, H * W * C, (H - 2 * p) * (W - 2 * p) * C, smap


def psnr_ssim(pred: torch.Tensor, gt: torch.Tensor, *, data_range: float = 1.0, win_size: int = 7, gaussian_weights: bool = False,
              use_sample_covariance: bool = True, K1: float = 0.01, K2: float = 0.03, return_map: bool = False):
    """-> (psnr [B], ssim [B]) float64 on the images' device, plus the SSIM map [B, H-2p, W-2p, C] float32 with ``return_map``.
    ``pred``, ``gt``: [B, H, W, C] or [H, W, C] (B = 1), float32, contiguous, C in 1..4.  One pass over both batches; nothing is
    read back, so the call does not wait for the device.  Identical images give ``psnr = inf``.  ``ValueError`` for anything else."""
    sq, ss, n_el, n_centres, smap = psnr_ssim_sums(pred, gt, data_range=data_range, win_size=win_size, gaussian_weights=gaussian_weights,
                                                   use_sample_covariance=use_sample_covariance, K1=K1, K2=K2, return_map=return_map)
    psnr_v = 10.0 * torch.log10(float(data_range) ** 2 / (sq / float(n_el)))
    ssim_v = ss / float(n_centres)
    return (psnr_v, ssim_v, smap) if return_map else (psnr_v, ssim_v)


def psnr(pred, gt, *, data_range: float = 1.0) -> torch.Tensor:
    """``skimage.metrics.peak_signal_noise_ratio`` per image -> [B] float64 (eval/score.py:101-103)."""
    return psnr_ssim(pred, gt, data_range=data_range)[0]


def ssim(pred, gt, **kwargs) -> torch.Tensor:
    """``skimage.metrics.structural_similarity`` per image over all channels -> [B] float64 (eval/score.py:106-108)."""
    return psnr_ssim(pred, gt, **kwargs)[1]


def eval_crop(mask, patch_size: int, *images, bbox=None):
    """The evaluation crop of eval/score.py:23-60 on [H, W, 3] images: the bounding box of ``mask > 0`` grown by 50 px and clipped
    to the image (end-exclusive, exactly as the reference slices it), pasted on a square canvas of ones centred on the short axis,
    then a bilinear resize to ``patch_size`` with half-pixel centres and no antialiasing -> [patch_size, patch_size, 3] each
    (``None`` passes through).  ``bbox`` = ``losses.mask_bbox(host mask)`` spares a device mask the read-back of its row and column
    profiles (the one host synchronisation of this function).

    The resize is ``F.interpolate(mode='bilinear', align_corners=False)``, which is also what OpenCV's ``INTER_LINEAR`` computes on
    float images; parity with OpenCV itself is NOT pinned, because OpenCV is not available to this package."""
    if bbox is None:
        m = torch.as_tensor(mask) > 0
        prof = torch.cat([m.any(1), m.any(0)]).cpu().numpy()
        bbox = bbox_from_profiles(prof[:m.shape[0]], prof[m.shape[0]:])
    Hm, Wm = (int(s) for s in mask.shape[:2])
    min_v, min_u, max_v, max_u = bbox
    clip = lambda v, hi: min(max(v, 0), hi)  # noqa: E731
    min_v, max_v = clip(min_v - EVAL_PAD, Hm), clip(max_v + EVAL_PAD, Hm)
    min_u, max_u = clip(min_u - EVAL_PAD, Wm), clip(max_u + EVAL_PAD, Wm)
    len_v, len_u = max_v - min_v, max_u - min_u
    max_size = max(len_v, len_u)
    out = []
    for image in images:
        if image is None:
            out.append(None)
            continue
        canvas = torch.ones((max_size, max_size, 3), dtype=image.dtype, device=image.device)
        if len_v > len_u:
            s = (max_size - len_u) // 2
            canvas[:, s:s + len_u] = image[min_v:max_v, min_u:max_u]
        else:
            s = (max_size - len_v) // 2
            canvas[s:s + len_v, :] = image[min_v:max_v, min_u:max_u]
        canvas = F.interpolate(canvas.permute(2, 0, 1)[None], size=(patch_size, patch_size), mode='bilinear', align_corners=False)
        out.append(canvas[0].permute(1, 2, 0).contiguous())
    return out if len(out) > 1 else out[0]


def cut_rect(img: torch.Tensor) -> torch.Tensor:
    """eval/score.py:73-81: pad a [H, W, C] image with ones at the bottom or the right to a square."""
    h, w = img.shape[:2]
    if h == w:
        return img
    size = max(h, w)
    out = torch.ones((size, size, img.shape[2]), dtype=img.dtype, device=img.device)
    out[:h, :w] = img
    return out


def lpips_score(lpips, src: torch.Tensor, tar: torch.Tensor, flip_rgb: bool = True) -> torch.Tensor:
    """eval/score.py:87-98 -> 0-d tensor on the images' device: [H, W, 3] images in [0, 1], squared with ``cut_rect``, LPIPS with
    ``normalize=True`` under ``no_grad``.  The reference feeds what ``cv.imread`` returned, BGR; ``flip_rgb`` reorders RGB renders to
    that order, as ``losses.lpips_loss`` does."""
    src, tar = cut_rect(src), cut_rect(tar)
    order = [2, 1, 0] if flip_rgb else [0, 1, 2]
    with torch.no_grad():
        return lpips(src.permute(2, 0, 1)[None, order].contiguous(), tar.permute(2, 0, 1)[None, order].contiguous(), normalize=True).mean()


class Metrics:
    """The accumulator of eval/score.py:9-20 (fields ``psnr``, ``ssim``, ``lpips``, ``count``; the same ``__repr__``) with the sums
    kept as float64 tensors on the device: ``update`` enqueues, ``result`` (and ``repr``, which calls it) is the only point that
    waits for the device -- given a host mask; a device mask costs ``eval_crop`` one small read-back per frame."""

    def __init__(self):
        self.psnr = 0.
        self.ssim = 0.
        self.lpips = 0.
        self.count = 0

    def update(self, pred: torch.Tensor, gt: torch.Tensor, mask=None, lpips=None, patch_size: int = 512) -> None:
        """One frame, or a batch of frames, of one method (comparison_body_only_avatars.py:45-71).  ``pred``, ``gt``: [H, W, 3] or
        [B, H, W, 3] float32 in [0, 1] on the GPU; ``mask``: [H, W] / [B, H, W] bool (device tensor, host tensor or numpy array), True on
        the subject: ``gt`` is set to 1 outside it (on a copy).  PSNR and SSIM are taken on the full images; with an ``lpips`` module,
        LPIPS on the 50-px-padded crop around the mask resized to ``patch_size`` (on the full frame squared with ones when there is
        no mask)."""
        if pred.dim() == 3:
            pred, gt = pred[None], gt[None]
            mask = None if mask is None else mask[None]
        if mask is not None:
            dev_mask = torch.as_tensor(mask).to(device=gt.device, dtype=torch.bool, non_blocking=True)
            gt = gt.clone()
            gt[~dev_mask] = 1.
        p, s = psnr_ssim(pred, gt)
        self.psnr = self.psnr + p.sum()
        self.ssim = self.ssim + s.sum()
        if lpips is not None:
            for b in range(pred.shape[0]):
                if mask is None:
                    pc, gc = pred[b], gt[b]
                else:
                    host = not (isinstance(mask, torch.Tensor) and mask.is_cuda)
                    pc, gc = eval_crop(np.asarray(mask[b]) if host else mask[b], patch_size, pred[b], gt[b])
                self.lpips = self.lpips + lpips_score(lpips, pc, gc).to(torch.float64)
        self.count += int(pred.shape[0])

    def result(self) -> dict:
        """{'count', 'psnr', 'ssim', 'lpips'}: the means as Python floats (waits for the device)."""
        if self.count == 0:
            return {"count": 0, "psnr": math.nan, "ssim": math.nan, "lpips": math.nan}
        return {"count": self.count, **{k: float(getattr(self, k)) / self.count for k in ("psnr", "ssim", "lpips")}}

    def __repr__(self):
        if self.count > 0:
            r = self.result()
            return f"Count: {r['count']}, PSNR: {r['psnr']}, SSIM: {r['ssim']}, LPIPS: {r['lpips']}"
        return 'count is 0!'
