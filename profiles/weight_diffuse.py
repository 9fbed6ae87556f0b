#!/usr/bin/env python
"""Time the blend-weight diffusion at product size (``include/ag_weight_diffuse.h``, ``WeightVolume.diffuse``).

    python profiles/weight_diffuse.py [--res 128] [--iters 50]

The volume is ``WeightVolume.from_body_mesh`` of ``synth.body_mesh(second_component=False)`` at res^3 x 55.  One process, device events:
(a) the HBM rate this device gives a plain copy of one volume (``Tensor.copy_``: one pass read, one written), the median of 5 rounds of
    20 copies -- the yardstick the iteration is held against, measured here and now, not taken from a data sheet;
(b) the time of one conjugate-gradient iteration: ``iters`` iterations enqueued by ONE ``ag_weight_diffuse_iterate`` call between two
    events, after a warm-up call, the median of 5 rounds, and its share of (a) against the algorithmic bytes of the three-pass form,
    11 volume passes per iteration (2 + 6 + 3: csrc/ag_weight_diffuse.hip);
(c) the whole ``diffuse()`` at ``tol = 1e-5``: wall time with a synchronise either side, the iteration count, the residuals it reports,
    the number of fixed nodes and the band.
Prints one JSON line.  There is nothing to compare against: the reference's solver is an external program for another platform.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import _lib, synth  # noqa: E402
from animatablegaussians_amd.weight_volume import WeightVolume, stencil_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = synth.body_mesh(second_component=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = WeightVolume.from_body_mesh(t(m["vertices"]), t(m["faces"]), t(m["lbs_weights"]), res=args.res)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    X, Y, Z, J = vol.ori_weight_volume.shape
    volume_bytes = vol.ori_weight_volume.numel() * 4

    def events(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n                                        # seconds per call

    # (a) the copy rate
    dst = torch.empty_like(vol.ori_weight_volume)
    copy = lambda: dst.copy_(vol.ori_weight_volume)  # noqa: E731
    events(copy, 5)
    copy_s = float(np.median([events(copy, 20) for _ in range(5)]))
    copy_rate = 2 * volume_bytes / copy_s
    del dst

    # (b) one iteration
    spacing = [float(h) for h in vol.voxel_size.cpu()]
    band = 1.5 * max(spacing)
    fixed = (vol.smpl_sdf_volume[..., 0].abs() <= band).contiguous()
    L = _lib.lib()
    w = (ctypes.c_float * 3)(*stencil_weights(spacing).tolist())
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    x, r, p, q = (torch.empty_like(vol.ori_weight_volume) for _ in range(4))
    n_ws = int(L.ag_weight_diffuse_workspace_bytes(X, Y, Z, J))
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    bb, rr = torch.empty(J, device="cuda"), torch.empty(J, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.ag_weight_diffuse_init(P(vol.ori_weight_volume), P(fixed), X, Y, Z, J, w, P(x), P(r), P(p), P(q), P(ws), n_ws, P(bb), P(rr), stream),
               "ag_weight_diffuse_init")

    def iterate():
        _lib.check(L.ag_weight_diffuse_iterate(P(fixed), X, Y, Z, J, w, args.iters, P(x), P(r), P(p), P(q), P(ws), n_ws, P(rr), stream),
                   "ag_weight_diffuse_iterate")

    events(iterate, 1)
    rounds = [events(iterate, 1) / args.iters for _ in range(5)]
    iter_s = float(np.median(rounds))
    del x, r, p, q

    # (c) the whole thing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = vol.diffuse()
    torch.cuda.synchronize()
    diffuse_s = time.perf_counter() - t0
    d = out.diffusion
    algorithmic = 11 * volume_bytes
    print(json.dumps({
        "res": [X, Y, Z], "J": J, "volume_bytes": volume_bytes, "from_body_mesh_s": round(build_s, 3),
        "copy_rate_TBs": round(copy_rate / 1e12, 3),
        "iteration_us": round(iter_s * 1e6, 1), "iteration_us_rounds": [round(s * 1e6, 1) for s in rounds],
        "algorithmic_bytes_per_iteration": algorithmic, "iteration_rate_TBs": round(algorithmic / iter_s / 1e12, 3),
        "share_of_copy_rate": round(algorithmic / iter_s / copy_rate, 3),
        "diffuse_s": round(diffuse_s, 3), "iterations": d["iterations"], "band_m": round(d["band"], 5), "fixed_nodes": d["fixed_nodes"],
        "rel_residual_max": float(d["rel_residual"].max()), "true_rel_residual_max": float(d["true_rel_residual"].max()),
        "row_sum_error_max": float((out.diff_weight_volume.double().sum(-1) - 1).abs().max()),
        "diff_minus_ori_max": float((out.diff_weight_volume - out.ori_weight_volume).abs().max())}))


if __name__ == "__main__":
    main()
