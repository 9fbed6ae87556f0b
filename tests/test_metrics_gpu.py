"""PSNR / SSIM on the GPU (``include/ag_metrics.h``) against the float64 restatement in ``metrics_oracle.py``, and the ``Metrics``
accumulator against the oracle composition.

Bars (set by the definition's own float32 behaviour, not by the kernel):
  * SSIM map, per pixel:  |S_gpu - S_f64| <= 4 max|S_f32 - S_f64| + 8 * 2^-23, with S_f32 the same oracle run in float32 -- what
    scikit-image computes for float32 images -- on the same inputs.  The factor 4 allows a different order of the additions, the
    floor covers inputs on which the float32 oracle happens to be exact.
  * SSIM score: the same bar (the map's worst float32 deviation stands in for the scalar's own, which is too noisy to scale).
  * mse: within n * 2^-53 relative of the oracle, n = H W C: the any-order summation bound for non-negative float64 terms.

Shapes come from the kernel's tile (``metrics.TILE_H`` x ``TILE_W`` window centres per workgroup): a single centre, a partial tile,
exactly one tile, one more in each axis (four workgroups, three of them slivers), two tiles minus one.

Measured on the MI355X (worst over the shapes, channels and image pairs below; the kernel sums in float64): SSIM map 2.98e-8 = 2^-25,
its own rounding to float32, against bars of 1.5e-6 to 5.9e-4; SSIM score 7.1e-14; mse 2.7e-16 relative.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 8 * 2.0 ** -23


def _shapes(w):
    from animatablegaussians_amd.metrics import TILE_H as TH, TILE_W as TW
    return [(w, w), (w + 1, w + 16), (TH + w - 1, TW + w - 1), (TH + w, TW + w), (2 * TH + w - 2, 2 * TW + w - 2)]


def _cases():
    out = []
    for gaussian, w in ((False, 7), (True, 11)):
        for hw in _shapes(w):
            for C in (1, 3):
                out.append((gaussian, w, hw[0], hw[1], C))
    out.append((True, 11, _shapes(11)[3][0], _shapes(11)[3][1], 4))       # the largest LDS footprint: 11 taps, 4 channels
    out.append((False, 3, _shapes(3)[3][0], _shapes(3)[3][1], 2))         # the smallest window, two channels
    return out


def _pairs(H, W, C):
    pairs = mo.image_pairs(H, W, C, seed=H * 1000 + W * 10 + C)
    # the issue's literal fourth pair as well: the mostly-white image against the smooth ground truth
    pairs["white_vs_smooth"] = (pairs["white_box"][0], pairs["noise5"][1])
    return pairs


@functools.lru_cache(maxsize=None)
def _oracle(gaussian, w, H, W, C):
    out = {}
    for name, (pred, gt) in _pairs(H, W, C).items():
        kw = dict(win_size=w, gaussian_weights=gaussian)
        s64, m64 = mo.ssim(pred, gt, **kw)
        _, m32 = mo.ssim(pred, gt, dtype=np.float32, **kw)
        out[name] = dict(pred=pred, gt=gt, ssim=s64, map=m64, dev32=float(np.abs(m32.astype(np.float64) - m64).max()),
                         mse=mo.mse(pred, gt), psnr=mo.psnr(pred, gt))
    return out


@pytest.mark.parametrize("gaussian,w,H,W,C", _cases())
def test_ssim_map_score_and_mse_against_the_float64_oracle(gaussian, w, H, W, C):
    import torch
    from animatablegaussians_amd import metrics
    ref = _oracle(gaussian, w, H, W, C)
    names = list(ref)
    pred = torch.from_numpy(np.stack([ref[n]["pred"] for n in names])).cuda()
    gt = torch.from_numpy(np.stack([ref[n]["gt"] for n in names])).cuda()
    kw = dict(win_size=w, gaussian_weights=gaussian)
    sq, ss, n_el, n_centres, smap = metrics.psnr_ssim_sums(pred, gt, return_map=True, **kw)
    psnr, ssim, smap2 = metrics.psnr_ssim(pred, gt, return_map=True, **kw)
    assert n_el == H * W * C and n_centres == (H - w + 1) * (W - w + 1) * C and tuple(smap.shape) == (len(names), H - w + 1, W - w + 1, C)
    assert psnr.dtype == ssim.dtype == sq.dtype == torch.float64 and smap.dtype == torch.float32 and psnr.is_cuda and torch.equal(smap, smap2)
    assert torch.equal(ssim, ss / n_centres)
    sq, ssim, psnr, smap = sq.cpu().numpy(), ssim.cpu().numpy(), psnr.cpu().numpy(), smap.cpu().numpy().astype(np.float64)
    failures = []
    for i, n in enumerate(names):
        r = ref[n]
        bar = 4 * r["dev32"] + FLOOR
        e_map = float(np.abs(smap[i] - r["map"]).max())
        e_s = abs(float(ssim[i]) - r["ssim"])
        e_mse = abs(sq[i] / n_el - r["mse"]) / r["mse"]
        print(f"w={w} {H}x{W}x{C} {n:16s} ssim {r['ssim']:.6f}: map err {e_map:.3e} score err {e_s:.3e} (bar {bar:.3e}, float32 oracle "
              f"{r['dev32']:.3e}); mse rel err {e_mse:.3e} (bar {n_el * 2.0 ** -53:.3e}); psnr {psnr[i]:.6f} vs {r['psnr']:.6f}")
        if not e_map <= bar:
            failures.append(f"{n}: map {e_map:.3e} > {bar:.3e}")
        if not e_s <= bar:
            failures.append(f"{n}: score {e_s:.3e} > {bar:.3e}")
        if not e_mse <= n_el * 2.0 ** -53:
            failures.append(f"{n}: mse {e_mse:.3e}")
        # 10 log10: the relative error of mse, n 2^-53, moves the PSNR by 10 / ln 10 times as much, plus the rounding of log10 and the scale
        if not abs(psnr[i] - r["psnr"]) <= 10 / np.log(10) * n_el * 2.0 ** -53 + 4 * 2.0 ** -53 * abs(r["psnr"]):
            failures.append(f"{n}: psnr {psnr[i]} vs {r['psnr']}")
    assert not failures, failures


def test_other_parameters_reach_the_kernel():
    """data_range, K1 / K2 and the population covariance change C1, C2 and cn: each against the oracle with the same bars."""
    import torch
    from animatablegaussians_amd import metrics
    pred, gt = mo.image_pairs(30, 45, 3, seed=2)["noise5"]
    a, b = torch.from_numpy(pred * 255).cuda(), torch.from_numpy(gt * 255).cuda()
    for kw in (dict(data_range=255.0), dict(data_range=255.0, use_sample_covariance=False), dict(data_range=255.0, K1=0.02, K2=0.05, win_size=5)):
        s64, m64 = mo.ssim(pred * 255, gt * 255, **kw)
        _, m32 = mo.ssim(pred * 255, gt * 255, dtype=np.float32, **kw)
        bar = 4 * float(np.abs(m32.astype(np.float64) - m64).max()) + FLOOR
        p, s, m = metrics.psnr_ssim(a, b, return_map=True, **kw)
        e_map, e_s = float(np.abs(m[0].cpu().numpy().astype(np.float64) - m64).max()), abs(float(s) - s64)
        print(f"{kw}: map err {e_map:.3e}, score err {e_s:.3e}, bar {bar:.3e}")
        assert e_map <= bar and e_s <= bar
        assert abs(float(p) - mo.psnr(pred * 255, gt * 255, 255.0)) <= 1e-9
        assert torch.equal(metrics.ssim(a, b, **kw), s) and torch.equal(metrics.psnr(a, b, data_range=255.0), p)


def test_identical_images_and_single_image_input():
    import torch
    from animatablegaussians_amd import metrics
    x = torch.from_numpy(mo.smooth_image(40, 50, 3, seed=1)).cuda()
    p, s = metrics.psnr_ssim(x, x.clone())
    assert tuple(p.shape) == (1,) and torch.isinf(p).all() and (p > 0).all()
    assert abs(float(s) - 1.0) <= FLOOR
    e = torch.empty(0, 40, 50, 3, device="cuda")
    p, s = metrics.psnr_ssim(e, e)
    assert tuple(p.shape) == (0,) and tuple(s.shape) == (0,)


def test_deterministic_and_batch_invariant():
    import torch
    from animatablegaussians_amd import metrics
    from animatablegaussians_amd.metrics import TILE_H as TH, TILE_W as TW
    H, W = 3 * TH + 9, 5 * TW + 3
    pairs = list(mo.image_pairs(H, W, 3, seed=9).values())[:3]
    pred = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
    gt = torch.from_numpy(np.stack([g for _, g in pairs])).cuda()
    for kw in (dict(), dict(gaussian_weights=True)):
        first = metrics.psnr_ssim(pred, gt, return_map=True, **kw)
        again = metrics.psnr_ssim(pred, gt, return_map=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        for i in range(3):
            one = metrics.psnr_ssim(pred[i], gt[i], return_map=True, **kw)
            assert torch.equal(one[0], first[0][i:i + 1]) and torch.equal(one[1], first[1][i:i + 1]) and torch.equal(one[2][0], first[2][i])


def test_argument_errors_raise_before_any_launch():
    import torch
    from animatablegaussians_amd import metrics
    x = torch.zeros(2, 16, 20, 3, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        metrics.psnr_ssim(x.half(), x.half())
    with pytest.raises(ValueError, match="float32"):
        metrics.psnr_ssim(x.double(), x.double())
    with pytest.raises(ValueError, match="contiguous"):
        metrics.psnr_ssim(x.transpose(1, 2), x.transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        metrics.psnr_ssim(x[:, :, ::2], x[:, :, ::2])
    with pytest.raises(ValueError, match="same shape"):
        metrics.psnr_ssim(x, x[:, :, :19])
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.psnr_ssim(x[:, :6].contiguous(), x[:, :6].contiguous())
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.psnr_ssim(x[:, :10].contiguous(), x[:, :10].contiguous(), gaussian_weights=True)
    with pytest.raises(ValueError, match="odd"):
        metrics.psnr_ssim(x, x, win_size=8)
    with pytest.raises(ValueError, match="channels"):
        metrics.psnr_ssim(torch.zeros(16, 20, 5, device="cuda"), torch.zeros(16, 20, 5, device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        metrics.psnr_ssim(x, x.cpu())


def test_metrics_accumulator_equals_the_oracle_composition():
    """Two 96 x 80 frames with masks: gt is whitened outside the mask, PSNR / SSIM on the full frames against the oracle with the bars
    above, LPIPS (name-seeded weights) on the 50-px crop against this package's LPIPS fed the ORACLE's crop, to the 1e-4 relative
    ``test_lpips.py`` holds the module to."""
    import torch
    from animatablegaussians_amd import metrics
    from animatablegaussians_amd.lpips import LPIPS, lpips_named_fill
    net = LPIPS(net='vgg')
    sd = net.reference_state_dict()
    net.load_reference_state_dict({**lpips_named_fill({k: v for k, v in sd.items() if not k.startswith("scaling_layer")}),
                                   "scaling_layer.shift": net.scaling_layer__shift, "scaling_layer.scale": net.scaling_layer__scale})
    net = net.cuda()
    H, W, patch = 96, 80, 64
    rng = np.random.default_rng(4)
    gt = np.stack([mo.smooth_image(H, W, 3, seed=s) for s in (20, 21)])
    pred = np.clip(gt + 0.05 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    mask = np.zeros((2, H, W), bool)
    mask[0, 60:90, 30:45] = True        # the growth clips at the bottom
    mask[1, 52:58, 10:70] = True        # wide; clips left and right
    want = dict(psnr=0.0, ssim=0.0, lpips=0.0)
    bar = 0.0
    for i in range(2):
        g = gt[i].copy()
        g[~mask[i]] = 1.0
        s64, m64 = mo.ssim(pred[i], g)
        _, m32 = mo.ssim(pred[i], g, dtype=np.float32)
        bar += 4 * float(np.abs(m32.astype(np.float64) - m64).max()) + FLOOR
        want["psnr"] += mo.psnr(pred[i], g)
        want["ssim"] += s64
        pc, gc = (torch.from_numpy(c.astype(np.float32)).cuda() for c in mo.eval_crop(mask[i], patch, pred[i], g))
        with torch.no_grad():
            want["lpips"] += float(net(pc.permute(2, 0, 1)[None, [2, 1, 0]].contiguous(), gc.permute(2, 0, 1)[None, [2, 1, 0]].contiguous(),
                                       normalize=True).mean())
    gt_dev = torch.from_numpy(gt).cuda()
    keep = gt_dev.clone()
    results = []
    for m in (torch.from_numpy(mask).cuda(), mask):                  # a device mask and a host mask
        acc = metrics.Metrics()
        acc.update(torch.from_numpy(pred).cuda(), gt_dev, m, lpips=net, patch_size=patch)
        assert acc.count == 2 and all(isinstance(getattr(acc, k), torch.Tensor) and getattr(acc, k).dtype == torch.float64
                                      and getattr(acc, k).is_cuda for k in ("psnr", "ssim", "lpips"))
        r = acc.result()
        print(f"Metrics: {acc!r}; oracle psnr {want['psnr'] / 2}, ssim {want['ssim'] / 2} (bar {bar / 2:.3e}), lpips {want['lpips'] / 2}")
        assert abs(r["ssim"] - want["ssim"] / 2) <= bar / 2
        assert abs(r["psnr"] - want["psnr"] / 2) <= 1e-9
        np.testing.assert_allclose(r["lpips"], want["lpips"] / 2, rtol=1e-4)
        assert repr(acc) == f"Count: 2, PSNR: {r['psnr']}, SSIM: {r['ssim']}, LPIPS: {r['lpips']}"
        results.append(r)
    # a host mask and a device mask give the same kernel inputs: PSNR / SSIM bit for bit (LPIPS is only repeatable to its own tolerance)
    assert all(results[0][k] == results[1][k] for k in ("count", "psnr", "ssim"))
    assert torch.equal(gt_dev, keep)                                   # the caller's ground truth is not written to
    # one frame at a time accumulates to the same counts; without a mask and without LPIPS the frames are scored as they are
    acc = metrics.Metrics()
    for i in range(2):
        acc.update(torch.from_numpy(pred[i]).cuda(), gt_dev[i])
    r = acc.result()
    assert r["count"] == 2 and r["lpips"] == 0.0 and abs(r["psnr"] - (mo.psnr(pred[0], gt[0]) + mo.psnr(pred[1], gt[1])) / 2) <= 1e-9
