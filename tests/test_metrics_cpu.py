"""Image scores, the part that needs no GPU: the ABI surface, the float64 oracle against closed forms, against the definition
written without a filter library and (where it can be imported) against scikit-image, the evaluation crop against its numpy
restatement, and the argument errors that are raised before anything touches a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_oracle as mo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from animatablegaussians_amd import _lib, metrics
    raw = open(os.path.join(ROOT, "include", "ag_metrics.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ag_psnr_ssim_workspace_bytes", "ag_psnr_ssim"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_metrics.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in table and len(table[name][2]) == n_args, f"{name}: header declares {n_args} arguments"
        assert hasattr(L, name), f"{name} is not exported"
    defines = dict(re.findall(r"#define (AG_METRICS_\w+) (\d+)", hdr))
    assert (metrics.TILE_H, metrics.TILE_W, metrics.MAX_TAPS) == tuple(
        int(defines[k]) for k in ("AG_METRICS_TILE_H", "AG_METRICS_TILE_W", "AG_METRICS_MAX_TAPS"))
    for fn in ("psnr_ssim", "psnr", "ssim", "eval_crop", "lpips_score", "Metrics"):
        assert callable(getattr(metrics, fn))
    assert "NOT pinned" in metrics.eval_crop.__doc__
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert "ag_metrics.hip" in build and "include/ag_metrics.h" in build       # compiled, and the header is in the staleness test


def test_entry_point_rejects_bad_sizes_without_launching():
    """The size rules of the C entry points need no device: they return before any pointer is used."""
    from animatablegaussians_amd import _lib
    L = _lib.lib()
    taps = (ctypes.c_double * 12)(*([1.0 / 7] * 12))
    call = lambda B, H, W, C, n: L.ag_psnr_ssim(None, None, B, H, W, C, taps, n, 1.0, 1e-4, 9e-4, None, None, None, None, 0, None)  # noqa: E731
    assert call(1, 6, 32, 3, 7) != 0 and call(1, 32, 6, 3, 7) != 0          # H < w, W < w
    assert call(1, 32, 32, 5, 7) != 0 and call(1, 32, 32, 0, 7) != 0        # C outside 1..4
    assert call(1, 32, 32, 3, 8) != 0 and call(1, 32, 32, 3, 13) != 0       # even tap count, more than 11
    assert call(0, 32, 32, 3, 7) == 0                                       # B = 0: nothing to do, nothing launched
    assert L.ag_psnr_ssim_workspace_bytes(1, 6, 32, 7) == 0
    th, tw = 16, 32
    assert L.ag_psnr_ssim_workspace_bytes(3, th + 6 + 1, 2 * tw + 6, 7) == 3 * 2 * 2 * 16 + 256


def test_gaussian_taps():
    from animatablegaussians_amd import metrics
    k = mo.gaussian_taps()
    assert k.size == 11 and abs(k.sum() - 1.0) <= 2.0 ** -52 and np.array_equal(k, k[::-1]) and k.argmax() == 5
    assert np.array_equal(metrics.window_taps(7, True), k)
    assert np.array_equal(metrics.window_taps(7), np.full(7, 1.0 / 7))
    from scipy.ndimage import _filters
    if hasattr(_filters, "_gaussian_kernel1d"):
        np.testing.assert_allclose(k, _filters._gaussian_kernel1d(1.5, 0, 5), rtol=0, atol=2.0 ** -52)


@pytest.mark.parametrize("gaussian", [False, True])
def test_oracle_closed_forms(gaussian):
    x = mo.smooth_image(40, 37, 3, seed=3)
    s, smap = mo.ssim(x, x, gaussian_weights=gaussian)
    assert s == 1.0 and (smap == 1.0).all()
    p = 5 if gaussian else 3
    assert smap.shape == (40 - 2 * p, 37 - 2 * p, 3)
    # constant images a, b: every variance vanishes (to float64 rounding of the window means), S = (2ab + C1) / (a^2 + b^2 + C1)
    a, b, C1 = 0.75, 0.5, 1e-4
    s, smap = mo.ssim(np.full((20, 24, 2), a), np.full((20, 24, 2), b), gaussian_weights=gaussian)
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    # the variances are differences of O(1) window means, each off by a few 2^-53, against C2 = 9e-4
    assert abs(s - want) <= 64 * 2.0 ** -53 / 9e-4 and np.abs(smap - want).max() <= 64 * 2.0 ** -53 / 9e-4
    # PSNR of a constant offset d: mse = d^2
    for d in (0.25, 0.125, 1e-2):
        y = np.full((9, 11, 3), 0.5)
        assert abs(mo.psnr(y + d, y) - (-20 * np.log10(d))) <= 1e-12 * 20
    assert mo.psnr(x, x) == float("inf")


@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("cov", [True, False])
def test_oracle_equals_the_definition_on_whole_windows(gaussian, cov):
    """scipy's reflected border is cropped away entirely: the oracle equals the plain separable window sums of the header."""
    from animatablegaussians_amd import metrics
    for name, (pred, gt) in mo.image_pairs(33, 41, 3, seed=5).items():
        s, smap = mo.ssim(pred, gt, gaussian_weights=gaussian, use_sample_covariance=cov)
        direct = mo.ssim_direct(pred, gt, metrics.window_taps(7, gaussian), use_sample_covariance=cov)
        err = np.abs(smap - direct).max()
        print(f"{name} gaussian={gaussian} cov={cov}: max |scipy - direct| = {err:.3e}")
        # both are float64 evaluations of the same real function; the variances lose 2^-53 / C2 ~ 1e-13 relative at worst
        assert err <= 1e-11 and abs(s - direct.mean()) <= 1e-12


@pytest.mark.parametrize("gaussian", [False, True])
def test_oracle_equals_scikit_image(gaussian):
    sk = pytest.importorskip("skimage.metrics")
    for pred, gt in mo.image_pairs(48, 56, 3, seed=7).values():
        for dt in (np.float64, np.float32):
            want, want_map = sk.structural_similarity(pred.astype(dt), gt.astype(dt), channel_axis=-1, data_range=1.0,
                                                      gaussian_weights=gaussian, full=True)
            got, got_map = mo.ssim(pred, gt, gaussian_weights=gaussian, dtype=dt)
            p = (got_map.shape[0] - 48) // -2
            if dt is np.float64:
                assert abs(got - want) <= 1e-12 and np.abs(got_map - want_map[p:-p, p:-p]).max() <= 1e-12
            else:
                assert np.array_equal(got_map, want_map[p:-p, p:-p])
        assert abs(mo.psnr(pred, gt) - sk.peak_signal_noise_ratio(gt, pred, data_range=1)) <= 1e-12
        assert abs(mo.mse(pred, gt) - sk.mean_squared_error(gt, pred)) <= 1e-15


def _crop_case(kind):
    H, W = 150, 170
    mask = np.zeros((H, W), bool)
    if kind == "tall":
        mask[60:95, 75:90] = True          # 50-px growth stays inside: 135 x 115 -> canvas 135, centred in u
    elif kind == "wide":
        mask[70:80, 55:110] = True         # 109 x 155 -> centred in v
    else:
        mask[0:40, 120:170] = True         # touches the top and the right border: the growth clips on both
    mask[mask.nonzero()[0][0] + 3, mask.nonzero()[1][0] + 2] = False     # a hole changes nothing
    rng = np.random.default_rng(11)
    imgs = [rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2)]
    return mask, imgs


@pytest.mark.parametrize("kind", ["tall", "wide", "clipped"])
def test_eval_crop_equals_the_numpy_restatement(kind):
    import torch
    from animatablegaussians_amd import losses, metrics
    mask, imgs = _crop_case(kind)
    patch = 64
    min_v, max_v, min_u, max_u = mo.eval_box(mask)
    size = max(max_v - min_v, max_u - min_u)
    if kind == "clipped":
        assert min_v == 0 and max_u == mask.shape[1] and max_v == 39 + 50 and min_u == 120 - 50
    else:
        assert (max_v - min_v > max_u - min_u) == (kind == "tall")
    want = mo.eval_crop(mask, patch, *imgs)
    # float64 tensors: torch interpolates in float64, only rounding separates the two
    got = metrics.eval_crop(torch.from_numpy(mask), patch, *[torch.from_numpy(i.astype(np.float64)) for i in imgs])
    for g, w_ in zip(got, want):
        assert tuple(g.shape) == (patch, patch, 3) and g.dtype == torch.float64
        assert np.abs(g.numpy() - w_).max() <= 1e-12
    # float32 tensors: the source coordinate (d + 0.5) * scale - 0.5 < size carries ~3 roundings of 2^-24 * size, values lie in [0, 1]
    tol = (3 * size + 4) * 2.0 ** -24
    got32 = metrics.eval_crop(torch.from_numpy(mask), patch, *[torch.from_numpy(i) for i in imgs], bbox=losses.mask_bbox(mask))
    for g, w_ in zip(got32, want):
        err = np.abs(g.numpy().astype(np.float64) - w_).max()
        print(f"{kind}: canvas {size}, float32 crop vs float64 oracle {err:.3e} (tolerance {tol:.3e})")
        assert g.dtype == torch.float32 and err <= tol
    assert metrics.eval_crop(torch.from_numpy(mask), patch, None, torch.from_numpy(imgs[0]))[0] is None


def test_training_crop_is_unchanged_by_the_shared_bbox():
    import torch
    from animatablegaussians_amd import losses
    mask, imgs = _crop_case("tall")
    assert losses.mask_bbox(mask) == (60, 75, 94, 89)
    assert losses.mask_bbox(mask) == losses.bbox_from_profiles(mask.any(1), mask.any(0))
    img = torch.from_numpy(imgs[0]).permute(2, 0, 1)
    a = losses.crop_image(torch.from_numpy(mask).float(), 32, False, torch.ones(3), img)
    b = losses.crop_image(torch.from_numpy(mask).float(), 32, False, torch.ones(3), img, bbox=losses.mask_bbox(mask))
    assert torch.equal(a, b) and tuple(a.shape) == (3, 32, 32)


def test_argument_errors_without_a_gpu():
    import torch
    from animatablegaussians_amd import metrics
    x = torch.zeros(16, 16, 3)
    with pytest.raises(ValueError, match="GPU"):
        metrics.psnr_ssim(x, x)
    with pytest.raises(ValueError, match="GPU"):
        metrics.ssim(x[None], x[None])
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.psnr_ssim(torch.zeros(6, 16, 3), torch.zeros(6, 16, 3))
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.psnr_ssim(torch.zeros(16, 10, 3), torch.zeros(16, 10, 3), gaussian_weights=True)
    with pytest.raises(ValueError, match="float32"):
        metrics.psnr_ssim(x.double(), x.double())
    with pytest.raises(ValueError, match="same shape"):
        metrics.psnr_ssim(x, torch.zeros(16, 17, 3))
    with pytest.raises(ValueError, match="odd"):
        metrics.psnr_ssim(x, x, win_size=8)
    with pytest.raises(ValueError, match="channels"):
        metrics.psnr_ssim(torch.zeros(16, 16, 5), torch.zeros(16, 16, 5))
    with pytest.raises(ValueError, match="contiguous"):
        metrics.psnr_ssim(x.transpose(0, 1), x.transpose(0, 1))


def test_metrics_repr_and_cut_rect():
    import torch
    from animatablegaussians_amd import metrics
    m = metrics.Metrics()
    assert repr(m) == "count is 0!" and m.result()["count"] == 0
    m.psnr, m.ssim, m.lpips, m.count = torch.tensor(60.0, dtype=torch.float64), torch.tensor(1.5, dtype=torch.float64), 0.25, 2
    assert repr(m) == f"Count: 2, PSNR: {60.0 / 2}, SSIM: {1.5 / 2}, LPIPS: {0.25 / 2}"
    assert m.result() == {"count": 2, "psnr": 30.0, "ssim": 0.75, "lpips": 0.125}
    img = torch.rand(5, 8, 3)
    sq = metrics.cut_rect(img)
    assert tuple(sq.shape) == (8, 8, 3) and torch.equal(sq[:5], img) and (sq[5:] == 1).all()
    sq = metrics.cut_rect(img.transpose(0, 1))
    assert tuple(sq.shape) == (8, 8, 3) and torch.equal(sq[:, :5], img.transpose(0, 1)) and (sq[:, 5:] == 1).all()
