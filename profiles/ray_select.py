"""Time the ray selection (``ray_select``) at a dataset-sized frame, 1500 x 2048, with 1024 rays and with 2 patches of 32 x 32, and beside
it the numpy oracle (``tests/ray_select_oracle.py``, the reference's loader arithmetic) on the same box.  A probe, not a test.

    python profiles/ray_select.py            # prints one JSON line

* ``kernel_us``: each native call alone (classify; the three launches of the compaction over all 3 M classes; build of 1024 listed
  pixels with targets; build of all pixels without), device events around 20 back-to-back calls, warmed up, the median of 9 such
  blocks.  A call of a few microseconds is launch-sized: the figure is then the rate at which launches issue, not the kernel's work.
* ``wall_ms``: the public functions with everything they do -- the host projection, the allocations, the torch indexing and the host
  reads (``candidates``: the two counts; a sampling round / ``sample_patches`` / ``image_rays``: one count) -- host clock around a call
  that ends in a synchronise, warmed up, the median of 15 calls; ``min`` beside it.
* ``numpy_ms``: the oracle's float32 path for the same batch (best of 2).
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ray_select_oracle as ro  # noqa: E402
from animatablegaussians_amd import ray_select as rs  # noqa: E402

H, W = 1500, 2048
RAYS, PATCHES, PATCH = 1024, 2, 32


def scene():
    extr, intr = ro.scene_camera("tilted", H, W)
    y, x = np.mgrid[:H, :W]
    mask = np.hypot((y - H / 2) / 1.6, x - W / 2) < 0.16 * W                          # an upright ellipse inside the box's mask
    rng = np.random.RandomState(0)
    color = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    depth = rng.uniform(1.5, 3.5, (H, W)).astype(np.float32)
    return extr, intr, color, mask, depth


def kernel_us(fn, calls=20, blocks=9):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return round(statistics.median(out), 2)


def wall_ms(fn, n=15):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3)}


def best_ms(fn, n=2):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(min(out), 1)


def main():
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    extr, intr, color, mask, depth = scene()
    dc, dm, dd = torch.from_numpy(color).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(depth).cuda()
    dev = dm.device
    corners = rs.project_corners(ro.BOX, intr, extr)
    cam = rs._camera(extr, intr, ro.BOX, H, W)
    cls = rs._classify(corners, H, W, dm, None, dev)
    cand = rs.candidates(dm, ro.BOX, extr, intr)
    pix = cand.inside[torch.randperm(cand.inside.numel(), device=dev)[:RAYS]].contiguous()
    res = {"frame": [H, W], "inside": cand.inside.numel(), "outside": cand.outside.numel()}
    res["kernel_us"] = {
        "classify": kernel_us(lambda: rs._classify(corners, H, W, dm, None, dev)),
        "compact_3_launches": kernel_us(lambda: rs._compact(cls.view(-1), True)),
        "build_1024_with_targets": kernel_us(lambda: rs._build(cam, RAYS, dev, pix=pix, images=(dc, dm, dd))),
        "build_all_pixels": kernel_us(lambda: rs._build(cam, H * W, dev)),
    }
    g = torch.Generator(device="cuda").manual_seed(0)
    res["wall_ms"] = {
        "candidates": wall_ms(lambda: rs.candidates(dm, ro.BOX, extr, intr)),
        "sample_randomly_1024": wall_ms(lambda: rs.sample_randomly(dc, dm, dd, extr, intr, ro.BOX, RAYS, generator=g)),
        "sample_patches_2x32x32": wall_ms(lambda: rs.sample_patches(dc, dm, dd, extr, intr, ro.BOX, PATCHES, PATCH)),
        "image_rays": wall_ms(lambda: rs.image_rays(extr, intr, W, H, ro.BOX)),
    }

    def numpy_sample_randomly():
        """The oracle's rounds with numpy's own draws (``np.random.choice`` without replacement, as the reference)."""
        inside, outside, _ = ro.candidates(mask, ro.BOX, extr, intr)
        rng, kept, count = np.random.RandomState(1), [], 0
        while count < RAYS:
            rest = RAYS - count
            k_in = int(rest * 0.5)
            drawn = np.concatenate([inside[rng.choice(len(inside), k_in, replace=False)], outside[rng.choice(len(outside), rest - k_in, replace=False)]])
            hit = ro.build(drawn, extr, intr, ro.BOX, H, W)["hit"]
            kept.append(drawn[hit])
            count += int(hit.sum())
        return ro.build(np.concatenate(kept), extr, intr, ro.BOX, H, W, color, mask, depth)

    res["numpy_ms"] = {
        "candidates": best_ms(lambda: ro.candidates(mask, ro.BOX, extr, intr)),
        "sample_randomly_1024": best_ms(numpy_sample_randomly),
        "sample_patches_2x32x32": best_ms(lambda: ro.sample_patches(color, mask, depth, extr, intr, ro.BOX, PATCHES, PATCH, None, [(True, 5), (False, 7)])),
        "image_rays": best_ms(lambda: ro.image_rays(extr, intr, W, H, ro.BOX)),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
