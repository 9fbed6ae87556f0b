"""Time ``targets.prepare_targets`` at 1024 x 1024 and 1500 x 2048 for V = 1 and 16 views and, beside it, the host path it replaces on
the same box: the reference loader's arithmetic in numpy (``tests/targets_oracle.py``: threshold, 5 x 5 erosion and dilation, colour / 255
as float32) plus the upload of the float colour and the two bool planes (14 B/pixel, pageable memory as a loader's arrays are).

Call times (device events around 50 calls, warmed up, inputs already on the device, ``bbox=False`` so nothing waits):
    python profiles/targets.py
Kernel time alone, a run of its own (the kernel is prepare_targets_kernel<2>):
    rocprofv3 --kernel-trace --stats -d <out> -- python profiles/targets.py --once --views 16
Prints one JSON line.  ``contract_bytes`` = 18 V H W: 4 B/pixel read, 14 B/pixel written; ``contract_tb_per_s`` is that over the call
time (a call is one launch; with V = 1 it is launch-sized), to set against the 4.7-5.7 TB/s the package's other streaming kernels reach
(smplx_posedirs_t_kernel, mesh_resolve_ids_kernel, resolve_attribute_kernel)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import targets_oracle as to  # noqa: E402
from animatablegaussians_amd import targets  # noqa: E402

SIZES = [(1024, 1024), (1500, 2048)]


def frames(V, H, W):
    """A disc with a soft edge per view (a plausible matte: two classes, a thin band) and random colour."""
    y, x = np.mgrid[:H, :W].astype(np.float32)
    d = np.hypot(y - H / 2, x - W / 2)
    matte = np.round(255 * np.clip((0.3 * min(H, W) + 1.5 - d) / 3.0, 0, 1)).astype(np.uint8)
    color = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    return np.broadcast_to(color, (V, H, W, 3)).copy(), np.broadcast_to(matte, (V, H, W)).copy()


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def host_path_ms(color, matte, n=3):
    """One view through the loader's arithmetic and the float upload, host clock around work that ends in a synchronise."""
    best = {"numpy_ms": 1e30, "upload_ms": 1e30}
    for _ in range(n):
        t0 = time.perf_counter()
        items = to.prepare(color, matte)
        t1 = time.perf_counter()
        dev = [torch.from_numpy(v).cuda() for v in items.values()]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del dev
        best["numpy_ms"] = min(best["numpy_ms"], (t1 - t0) * 1e3)
        best["upload_ms"] = min(best["upload_ms"], (t2 - t1) * 1e3)
    return best


def main():
    once = "--once" in sys.argv
    views = [int(sys.argv[sys.argv.index("--views") + 1])] if "--views" in sys.argv else [1, 16]
    out = {}
    for H, W in SIZES:
        for V in views:
            color, matte = frames(V, H, W)
            dc, dm = torch.from_numpy(color).cuda(), torch.from_numpy(matte).cuda()
            call = lambda: targets.prepare_targets(dc, dm, bbox=False)  # noqa: E731
            row = {"contract_bytes": 18 * V * H * W}
            if once:
                for _ in range(5 + 50):
                    call()
                torch.cuda.synchronize()
            else:
                us = timed(call)
                row["call_us"] = round(us, 1)
                row["contract_tb_per_s"] = round(row["contract_bytes"] / us * 1e-6, 3)
                row["call_with_bbox_us"] = round(timed(lambda: targets.prepare_targets(dc, dm, bbox=True), n=20), 1)
                pc, pm = torch.from_numpy(color).pin_memory(), torch.from_numpy(matte).pin_memory()
                row["call_from_pinned_uint8_us"] = round(timed(lambda: targets.prepare_targets(pc, pm, bbox=False), n=20), 1)
                if V == 1:
                    host = host_path_ms(color[0], matte[0])
                    row["host_path_per_view_ms"] = {k: round(v, 2) for k, v in host.items()}
            out[f"{H}x{W}_V{V}"] = row
            del dc, dm
    print(json.dumps(out))


if __name__ == "__main__":
    main()
