#!/usr/bin/env python
"""Time the blend-weight volume sampler at product size against the reference's own path on the same GPU.

    python profiles/weight_volume.py [--res 128] [--iters 200]

N = the canonical points of ``synth.body_mesh()`` at S = 1024 (268 k), C = 55, a res^3 volume (``synth.weight_volume_arrays``).
(a) ``WeightVolume.forward_weight``: the channel-last kernel (``include/ag_weight_volume.h``).
(b) ``F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True)`` on the transposed [1, C, X, Y, Z] copy with the grid
    ``(2 u - 1)[..., [2, 1, 0]]``, exactly as ``network/volume.py:79-92`` calls it (the scaling of the points included in both).
One process, device events around ``iters`` back-to-back calls after a warm-up of 20, the two paths alternating in 5 rounds; prints one
JSON line: the median round of each, the kernel's share of the 8 TB/s HBM peak against its algorithmic bytes 12 N + 4 C N, the
device memory each path holds for the volume, and the largest difference between the two outputs.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import subject_maps as sm, synth  # noqa: E402
from animatablegaussians_amd.weight_volume import WeightVolume  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = synth.body_mesh()
    v, f = t(m["vertices"]), t(m["faces"])
    maps = sm.canonical_maps(v, f, sm.vertex_normals(v, f), t(m["lbs_weights"]), size=1024)
    pts = maps["cano_smpl_pos_map"][maps["mask"]].contiguous()
    del maps
    a = synth.weight_volume_arrays(m, (args.res,) * 3, 55)
    vol = WeightVolume(*[t(a[k]) for k in ("diff_weight_volume", "ori_weight_volume", "volume_bounds", "center", "smpl_bounds")])
    N, C = pts.shape[0], vol.joint_num
    transposed = vol.diff_weight_volume.permute(3, 0, 1, 2)[None].contiguous()      # volume.py:49-51
    lo, ext = vol.volume_bounds[0], vol.volume_bounds[1] - vol.volume_bounds[0]

    def ours():
        return vol.forward_weight(pts)

    def reference():
        p = (pts[None] - lo[None, None]) / ext[None, None]
        grid = (2 * p - 1)[..., [2, 1, 0]][:, :, None, None]
        w = F.grid_sample(transposed, grid, mode='bilinear', padding_mode='border', align_corners=True)
        return w[:, :, :, 0, 0].permute(0, 2, 1)

    diff = float((ours() - reference()[0]).abs().max())

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters                               # microseconds per call

    rounds = [(timed(ours), timed(reference)) for _ in range(5)]
    us_ours, us_ref = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
    algorithmic = 12 * N + 4 * C * N
    print(json.dumps({
        "N": N, "C": C, "res": args.res, "iters": args.iters,
        "kernel_us": round(us_ours, 2), "kernel_us_rounds": [round(r[0], 2) for r in rounds],
        "grid_sample_us": round(us_ref, 2), "grid_sample_us_rounds": [round(r[1], 2) for r in rounds],
        "algorithmic_bytes": algorithmic, "kernel_share_of_8TBs_peak": round(algorithmic / (us_ours * 1e-6) / 8e12, 4),
        "volume_bytes": vol.diff_weight_volume.numel() * 4, "transposed_copy_bytes": transposed.numel() * 4,
        "max_abs_difference": diff}))


if __name__ == "__main__":
    main()
