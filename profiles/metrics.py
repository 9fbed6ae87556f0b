"""Time ``metrics.psnr_ssim`` at 1024 x 1024 x 3 for B = 1 and 8 and, beside it, the same SSIM composed from torch operators
(``avg_pool2d`` on the five stacked moments, float32) on the same device.

Call times (device events around 20 calls, warmed up):      python profiles/metrics.py
Per-kernel times, a run of its own per batch size (the kernels are psnr_ssim_tile_kernel<3> and psnr_ssim_sum_kernel; everything
else in the trace belongs to the torch composition):
    rocprofv3 --kernel-trace --stats -d <out> -- python profiles/metrics.py --once --batch 8
Prints one JSON line; ``algorithmic_bytes`` = 2 B H W C 4, both images read once."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import metrics  # noqa: E402

H = W = 1024
C = 3


def torch_ssim(x, y, win=7, C1=1e-4, C2=9e-4):
    """[B, H, W, C] float32 -> [B] float32: the definition of include/ag_metrics.h from full-image torch passes."""
    a, b = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    u = F.avg_pool2d(torch.cat([a, b, a * a, b * b, a * b], 1), win, stride=1)
    ux, uy, uxx, uyy, uxy = u.chunk(5, 1)
    cn = win * win / (win * win - 1.0)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    s = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return s.mean((1, 2, 3))


def images(B):
    g = torch.Generator(device="cuda").manual_seed(B)
    gt = torch.rand(B, H, W, C, device="cuda", generator=g)
    return (gt + 0.05 * torch.randn(B, H, W, C, device="cuda", generator=g)).clamp_(0, 1), gt


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    once = "--once" in sys.argv
    batches = [int(sys.argv[sys.argv.index("--batch") + 1])] if "--batch" in sys.argv else [1, 8]
    out = {"H": H, "W": W, "C": C}
    for B in batches:
        pred, gt = images(B)
        ours = lambda: metrics.psnr_ssim(pred, gt)  # noqa: E731
        composed = lambda: torch_ssim(pred, gt)  # noqa: E731
        diff = float((ours()[1] - composed().double()).abs().max())
        row = {"algorithmic_bytes": 2 * B * H * W * C * 4, "max_abs_ssim_difference_to_torch_float32": diff}
        if once:
            for fn in (ours, composed):
                for _ in range(3 + 20):
                    fn()
            torch.cuda.synchronize()
        else:
            row["psnr_ssim_call_us"] = round(timed(ours), 1)
            row["torch_composed_ssim_call_us"] = round(timed(composed), 1)
        out[f"B{B}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
