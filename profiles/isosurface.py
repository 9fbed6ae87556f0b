#!/usr/bin/env python
"""Time iso-surface extraction at the workload's own shape.

    python profiles/isosurface.py [--res 256 256 128] [--iters 3] [--runs 2]

An analytic body-like field (a lobed ellipsoid of half-axes 0.5 / 0.9 / 0.2 m, the radial function of ``synth.body_mesh``; positive
inside) is evaluated on the device at the nodes of the reference's ``testing_res`` grid (256, 256, 128) over a 1.2 x 2.0 x 0.6 m box.
``ag_isosurface_count`` and ``ag_isosurface_emit`` are timed separately with device events around ``iters`` back-to-back calls after one
warm-up call, ``runs`` times (each run listed, the median reported).  emit's own 20-byte read of the counts waits for the stream, so its
time includes that host round trip.  Also timed: ``isosurface.marching_cubes`` as a whole (allocation of the workspace and outputs and
the caller's read of the counts included, wall clock) and a device copy of 256 MB, whose rate (read + write bytes per second) is the HBM
rate the traffic floor is taken at.  The floor: two reads of the volume (count and emit each read it once) plus one write of the
outputs.  Prints one JSON line.  No time here is a pass / fail condition.
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
from animatablegaussians_amd import _lib, isosurface  # noqa: E402


def body_field(res, device):
    lo = torch.tensor([-0.6, -1.0, -0.3], device=device)
    hi = -lo
    spacing = (hi - lo) / (torch.tensor(res, device=device, dtype=torch.float32) - 1)
    ax = [lo[d] + torch.arange(res[d], device=device, dtype=torch.float32) * spacing[d] for d in range(3)]
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z).clamp_min(1e-6)
    T = torch.acos((y / r).clamp(-1, 1))
    P = torch.atan2(z, x)
    base = 1.0 / torch.sqrt((torch.sin(T) * torch.cos(P) / 0.5) ** 2 + (torch.cos(T) / 0.9) ** 2 + (torch.sin(T) * torch.sin(P) / 0.2) ** 2)
    surf = base * (1.0 + 0.18 * torch.sin(T) ** 2 * torch.cos(4.0 * T) * torch.cos(2.0 * P) + 0.10 * torch.sin(T) ** 2 * torch.sin(3.0 * P + 2.0 * T))
    return (surf - r).contiguous(), spacing.cpu().tolist(), lo.cpu().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    X, Y, Z = args.res
    vol, spacing, origin = body_field(args.res, dev)
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n_ws = int(L.ag_isosurface_workspace_bytes(X, Y, Z))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sp, org = (ctypes.c_float * 3)(*spacing), (ctypes.c_float * 3)(*origin)

    def count():
        _lib.check(L.ag_isosurface_count(p(vol), None, X, Y, Z, 0.0, p(ws), n_ws, p(counts), stream), "ag_isosurface_count")

    count()
    V, F = (int(c) for c in counts.cpu())
    vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)

    def emit():
        _lib.check(L.ag_isosurface_emit(p(vol), X, Y, Z, 0.0, sp, org, p(ws), n_ws, p(vertices), V, p(faces), F, stream), "ag_isosurface_emit")

    big = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    dst = torch.empty_like(big)

    def timed(fn, iters=args.iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters                                          # milliseconds per call

    def wall(fn, iters=args.iters):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    runs = [{"count": timed(count), "emit": timed(emit), "copy_256MB": timed(lambda: dst.copy_(big)),
             "marching_cubes_wall": wall(lambda: isosurface.marching_cubes(vol, 0.0, spacing, origin))} for _ in range(args.runs)]
    ms = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    hbm_rate = 2.0 * big.numel() * 4 / (ms["copy_256MB"] * 1e-3)
    v2, f2 = isosurface.marching_cubes(vol, 0.0, spacing, origin)
    floor_bytes = 2.0 * vol.numel() * 4 + 12.0 * V + 12.0 * F
    floor_ms = floor_bytes / hbm_rate * 1e3
    out = {"res": [X, Y, Z], "V": V, "F": F, "iters": args.iters, "workspace_bytes": n_ws,
           "same_as_marching_cubes": bool(torch.equal(v2, vertices) and torch.equal(f2, faces)),
           "ms": {k: round(v, 4) for k, v in ms.items()}, "ms_runs": [{k: round(v, 4) for k, v in r.items()} for r in runs],
           "hbm_copy_bytes_per_s": hbm_rate, "floor_bytes": floor_bytes, "floor_ms": round(floor_ms, 4),
           "count_plus_emit_over_floor": round((ms["count"] + ms["emit"]) / floor_ms, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
