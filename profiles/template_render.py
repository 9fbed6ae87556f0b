#!/usr/bin/env python
"""Time the template renderer: the four legs of one chunk of rays, and a whole 256 x 256 canonical render.

    python profiles/template_render.py [--rays 16384] [--vertices 10475] [--image 256] [--iters 20] [--runs 3]

The reference architecture (``profiles/template_field.py``'s recipe: multires 6, 39 -> 512 -> 256 x 5 -> 257, colour 256 x 3 -> 3), S = 64 samples
per ray, V vertices on a body-sized ellipsoid, pinhole rays at it.

* Legs of a chunk (R rays): ``near_far`` (``ag_ray_near_far``), ``sample`` (``ag_ray_sample``, no view directions: the reference
  configuration has ``use_viewdir`` off), ``field`` (``ag_template_field_forward``: sdf, density, colour) and ``composite``
  (``ag_ray_composite``: rgb and acc), each through its raw binding into preallocated buffers, so that the time between the two device
  events is launches back to back and nothing else.  One warm-up call, then ``iters`` calls between two events, ``runs`` times; every
  run is listed and the median reported.  A leg of a few microseconds is bounded below by the launch rate, not by the kernel.
* Bytes the memory-bound legs must move (computed here from the shapes): sample reads 32 R + 4 S and writes 16 R S; composite reads
  20 R S and writes 16 R.  Their rate is set against the 8 TB/s HBM peak (a streaming copy reaches 6.3 TB/s); at these sizes the
  buffers of a chunk (tens of MB) fit the 256 MiB Infinity Cache, so the figure is a bandwidth, not proof of HBM traffic.
* near_far: ball tests per second = R V / time.
* ``render_256``: ``template_render.render`` of image x image rays, canonical space, ``"smpl"`` sampling, chunks of 4096 and of 16 384
  rays, host clock around calls that end in a synchronise (allocations, launches and the near / far pass included).

Prints one JSON line.  No time here is a pass / fail condition.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from animatablegaussians_amd import _lib  # noqa: E402
from animatablegaussians_amd import template_field as tf  # noqa: E402
from animatablegaussians_amd import template_render as tr  # noqa: E402
from template_field import recipe  # noqa: E402  (profiles/template_field.py)

PEAK_HBM = 8e12
S = 64


def scene(n_rays, n_vertices, dev, seed=0):
    rs = np.random.RandomState(seed)
    p = rs.normal(size=(n_vertices, 3))
    body = (p / np.linalg.norm(p, axis=1, keepdims=True) * np.array([0.45, 0.9, 0.25])).astype(np.float32)
    eye = np.array([0.0, 0.0, -3.0])
    side = int(np.ceil(np.sqrt(n_rays)))
    g = ((np.arange(side) + 0.5) / side * 2 - 1)
    xx, yy = np.meshgrid(g * 0.25, g * 0.4)
    d = np.stack([xx.reshape(-1), yy.reshape(-1), np.ones(side * side)], 1)[:n_rays]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.repeat(eye[None], n_rays, 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    return t(body), t(o), t(d), torch.full((n_rays,), 2.0, device=dev), torch.full((n_rays,), 4.0, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--vertices", type=int, default=10475)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    R, V = args.rays, args.vertices
    geo, color = recipe()
    field = tf.TemplateField(geo, color, multires=6)
    body, o, d, box_near, box_far = scene(R, V, dev)
    L = _lib.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    near, far, hit = f32(R), f32(R), torch.empty(R, dtype=torch.uint8, device=dev)
    t_vals = tr._t_vals(S, dev)
    z, pts = f32(R, S), f32(R * S, 3)
    sdf, density, rgb = f32(R * S), f32(R * S), f32(R * S, 3)
    rgb_map, acc_map = f32(R, 3), f32(R)
    desc, blob = field.desc(), field._blob_on(dev)

    legs = {
        "near_far": lambda: _lib.check(L.ag_ray_near_far(p(body), V, p(o), p(d), R, 0.1, p(box_near), p(box_far), p(near), p(far), p(hit), stream), "near_far"),
        "sample": lambda: _lib.check(L.ag_ray_sample(p(o), p(d), p(near), p(far), R, p(t_vals), S, null, null, p(z), p(pts), null, stream), "sample"),
        "field": lambda: _lib.check(L.ag_template_field_forward(ctypes.byref(desc), p(blob), blob.numel(), p(pts), null, R * S, p(sdf), p(density), p(rgb),
                                                                stream), "field"),
        "composite": lambda: _lib.check(L.ag_ray_composite(p(density), p(rgb), p(z), R, S, 0, p(rgb_map), p(acc_map), null, null, null, stream), "composite"),
    }

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters          # microseconds

    for fn in legs.values():                             # the chain once, in order: every leg then runs on real inputs
        fn()
    torch.cuda.synchronize()
    runs = [{k: timed(fn, max(2, args.iters // 10) if k == "field" else args.iters) for k, fn in legs.items()} for _ in range(args.runs)]
    us = {k: float(np.median([r[k] for r in runs])) for k in legs}
    chunk = sum(us.values())
    bytes_moved = {"sample": 32 * R + 4 * S + 16 * R * S, "composite": 20 * R * S + 16 * R}

    def whole(chunk_size):
        n = args.image * args.image
        b, oo, dd, bn, bf = scene(n, V, dev)
        out = tr.render(field, oo, dd, bn, bf, sampling="smpl", live_smpl_v=b, chunk_size=chunk_size)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            out = tr.render(field, oo, dd, bn, bf, sampling="smpl", live_smpl_v=b, chunk_size=chunk_size)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return times, float(out["acc_map"].mean()), float((out["acc_map"] > 0.5).float().mean())

    r4096, acc_mean, covered = whole(4096)
    r16384, _, _ = whole(16384)
    out = {
        "rays": R, "samples": S, "vertices": V, "iters": args.iters,
        "leg_us": {k: round(v, 2) for k, v in us.items()}, "leg_us_runs": [{k: round(v, 2) for k, v in r.items()} for r in runs],
        "chunk_us": round(chunk, 1), "leg_share_of_chunk": {k: round(v / chunk, 5) for k, v in us.items()},
        "new_kernels_share_of_chunk": round((chunk - us["field"]) / chunk, 5),
        "bytes": bytes_moved,
        "TB_per_s": {k: round(b / (us[k] * 1e-6) / 1e12, 3) for k, b in bytes_moved.items()},
        "fraction_of_8TBs_peak": {k: round(b / (us[k] * 1e-6) / PEAK_HBM, 4) for k, b in bytes_moved.items()},
        "near_far_G_ball_tests_per_s": round(R * V / (us["near_far"] * 1e-6) / 1e9, 1),
        "rays_hit": int(hit.sum()), "acc_mean_of_chunk": round(float(acc_map.mean()), 4),
        "render_image": args.image, "render_ms_chunk_4096": [round(v, 2) for v in r4096], "render_ms_chunk_16384": [round(v, 2) for v in r16384],
        "render_acc_mean": round(acc_mean, 4), "render_fraction_covered": round(covered, 4),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
