#!/usr/bin/env python
"""Time the template renderer's reverse pass (``include/ag_ray_march_grad.h``) beside its forward and beside torch autograd.

    python profiles/template_render_grad.py [--rays 1024 262144] [--iters 20] [--runs 2]

Per ray count R (a training step's 1024 rays; 262 144 rays, enough samples to leave the caches), S = 64 samples per ray, the gradients
of a training step (``rgb_map`` and ``acc_map``), each leg through its raw binding into preallocated buffers between two device events:
one warm-up call, ``iters`` calls, ``runs`` times; every run is listed.  A leg of a few microseconds is bounded below by the launch
rate, not by the kernel.

* ``composite``: ``ag_ray_composite`` (rgb, acc): 20 bytes read per sample.
* ``composite_backward``: ``ag_ray_composite_backward`` (G_rgb, G_acc -> grad_density, grad_color): 20 read + 16 written per sample.
* ``density``: ``ag_laplace_density``: 4 + 4.  ``density_backward``: ``ag_laplace_density_backward`` (grad_sdf and grad_beta, both
  launches): 8 + 4.
* ``torch_forward`` / ``torch_forward_backward``: the same float32 chain (LaplaceDensity, alpha, cumprod, the sums) as torch ops on the
  device, and the same with ``torch.autograd.grad`` to sdf, colour and beta; their difference is torch's backward.

Prints one JSON line.  No time here is a pass / fail condition.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import _lib  # noqa: E402

S = 64


def scene(R, dev, seed=0):
    """Rays through a sphere of radius 0.5: signed distances, a smooth colour, jittered samples, random upstream gradients."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    off = torch.rand(R, generator=g) * 0.7                          # distance of the ray from the centre
    t = (torch.arange(S)[None] + 0.8 * torch.rand(R, S, generator=g)) / S
    z = 1.7 + 1.6 * t
    sdf = 0.5 - torch.sqrt(off[:, None] ** 2 + (z - 2.5) ** 2)
    color = 0.5 + 0.5 * torch.sin(3.0 * z[..., None] + torch.tensor([0.0, 1.0, 2.0]))
    to = lambda a: a.to(torch.float32).contiguous().to(dev)  # noqa: E731
    return to(sdf), to(color), to(z), to(torch.randn(R, 3, generator=g)), to(torch.randn(R, generator=g))


def torch_chain(sdf, beta, color, z):
    b = beta.abs() + 1e-4
    raw = -sdf
    density = (1 / b) * (0.5 + 0.5 * raw.sign() * torch.expm1(-raw.abs() / b))
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, dists[..., -1:]], -1)
    alpha = 1. - torch.exp(-density * dists)
    weights = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1. - alpha + 1e-10], -1), -1)[..., :-1]
    return torch.sum(weights[..., None] * color, -2), torch.sum(weights, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 262144])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731

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

    results = []
    for R in args.rays:
        N = R * S
        iters = args.iters if N <= 1 << 20 else max(3, args.iters // 4)
        sdf, color, z, g_rgb, g_acc = scene(R, dev)
        beta = torch.tensor([0.01], device=dev)
        density, rgb_map, acc_map = f32(R, S), f32(R, 3), f32(R)
        gd, gc, gs, gb = f32(R, S), f32(R, S, 3), f32(R, S), f32(1)
        ws = torch.empty(int(L.ag_laplace_density_backward_workspace_bytes(N)) // 8, dtype=torch.float64, device=dev)
        legs = {
            "density": lambda: _lib.check(L.ag_laplace_density(p(sdf), N, p(beta), p(density), stream), "density"),
            "composite": lambda: _lib.check(L.ag_ray_composite(p(density), p(color), p(z), R, S, 0, p(rgb_map), p(acc_map), null, null, null, stream), "composite"),
            "composite_backward": lambda: _lib.check(L.ag_ray_composite_backward(p(density), p(color), p(z), R, S, 0, p(g_rgb), p(g_acc), null, null, p(gd), p(gc),
                                                                                 stream), "composite_backward"),
            "density_backward": lambda: _lib.check(L.ag_laplace_density_backward(p(sdf), p(gd), N, p(beta), p(gs), p(gb), p(ws), stream), "density_backward"),
        }
        s_t, c_t, b_t = sdf.clone().requires_grad_(True), color.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def torch_forward():
            with torch.no_grad():
                torch_chain(s_t, b_t, c_t, z)

        def torch_both():
            rgb, acc = torch_chain(s_t, b_t, c_t, z)
            return torch.autograd.grad((rgb * g_rgb).sum() + (acc * g_acc).sum(), (s_t, c_t, b_t))

        legs["torch_forward"], legs["torch_forward_backward"] = torch_forward, torch_both
        for fn in legs.values():                         # the chain once, in order: every leg then runs on real inputs
            fn()
        torch.cuda.synchronize()
        t_gs, t_gc, t_gb = torch_both()
        agree = {"grad_sdf": float((gs - t_gs).abs().max() / t_gs.abs().max()), "grad_color": float((gc - t_gc).abs().max() / t_gc.abs().max()),
                 "grad_beta": float((gb - t_gb).abs().max() / t_gb.abs().max())}
        runs = [{k: timed(fn, iters) for k, fn in legs.items()} for _ in range(args.runs)]
        us = {k: float(np.median([r[k] for r in runs])) for k in legs}
        bytes_per_sample = {"density": 8, "composite": 20, "composite_backward": 36, "density_backward": 12}
        results.append({
            "rays": R, "samples": S, "iters": iters, "leg_us": {k: round(v, 2) for k, v in us.items()},
            "leg_us_runs": [{k: round(v, 2) for k, v in r.items()} for r in runs],
            "torch_backward_us": round(us["torch_forward_backward"] - us["torch_forward"], 2),
            "bytes_per_sample": bytes_per_sample,
            "TB_per_s": {k: round(b * N / (us[k] * 1e-6) / 1e12, 3) for k, b in bytes_per_sample.items()},
            "kernels_vs_torch_autograd_max_rel_difference": {k: float(f"{v:.2e}") for k, v in agree.items()},
            "acc_mean": round(float(acc_map.mean()), 4),
        })
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
