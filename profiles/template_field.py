#!/usr/bin/env python
"""Time the template field's SDF grid at the workload's own shape, against the same layers as a plain torch chain.

    python profiles/template_field.py [--res 256 256 128] [--iters 2] [--runs 2] [--grad]

The reference architecture (multires 6; 39 -> 512 -> 256 -> 256 -> 256 -> (256 + 39) -> 256 -> 257, Softplus(beta = 100); weights of a
deterministic recipe with the shapes of the geometric initialisation, every weight perturbed) is evaluated at the nodes of the
reference's ``testing_res`` grid (256, 256, 128) over a 1.2 x 2.0 x 0.6 m box:

* ``sdf_grid``: ``TemplateField.sdf_grid`` (the fused kernel, slab by slab; point assembly and launches included), device events around
  ``iters`` back-to-back calls after one warm-up call, ``runs`` times (each run listed, the median reported);
* ``torch_chain``: the same folded float32 weights as ``F.linear`` + ``F.softplus`` in float32 on the same GPU, the embedding with
  ``torch.sin`` / ``torch.cos``, in chunks of 256 * 256 * 4 points as ``test_geometry`` does, all 257 columns of the last layer as the
  reference computes them; timed the same way.  ``torch.backends.cuda.matmul.allow_tf32`` is left at its default (off: fp32 products).

``--grad`` adds three legs over the same points in the same chunks, timed the same way and reported under ``"grad"``:

* ``sdf_normal``: ``TemplateField.sdf_normal`` (the fused gradient kernel: value and three tangents, 8 points per weight pass);
* ``sdf_only``: ``TemplateField.__call__`` on the same chunks (the forward kernel, 32 points per weight pass);
* ``torch_autograd``: the torch chain above with ``requires_grad_()`` points and ``torch.autograd.grad`` of column 0, TF32 off.

FLOPs: 2 * multiply-adds of the layers the fused kernel runs for an SDF-only request (the last layer counted as ONE column: 256 MACs),
against the 155 TFLOP/s fp32-matrix peak; the torch chain's rate counts its 257 columns.  Also printed: the largest difference between
the two grids (two fp32 summation orders; not a pass / fail condition).  Prints one JSON line.  No time here is a pass / fail condition.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import template_field as tf  # noqa: E402

PEAK_F32_MATRIX = 155e12
WIDTHS = (512, 256, 256, 256, 256, 256)


def recipe(seed=0, multires=6):
    """Folded weights with the reference's shapes: normal(0, sqrt(2 / out)) rows, the last layer sqrt(pi / in) with bias -1.1."""
    rs = np.random.RandomState(seed)
    e = 3 + 6 * multires
    chans = [e] + list(WIDTHS) + [257]
    geo = []
    for l in range(len(chans) - 1):
        k = chans[l] + (e if l == 4 else 0)
        if l == len(chans) - 2:
            w, b = rs.normal(np.sqrt(np.pi / k), 1e-3, (chans[l + 1], k)), np.full(chans[l + 1], -1.1)
        else:
            w, b = rs.normal(0.0, np.sqrt(2.0 / chans[l + 1]), (chans[l + 1], k)), rs.normal(0.0, 0.02, chans[l + 1])
            if l == 0:
                w[:, 3:] *= 0.05
            if l == 4:
                w[:, -(e - 3):] *= 0.05
        geo.append((w.astype(np.float32), b.astype(np.float32)))
    cch = [256, 256, 256, 256, 3]
    color = [(rs.uniform(-1, 1, (cch[i + 1], cch[i])).astype(np.float32) / np.sqrt(cch[i]), np.zeros(cch[i + 1], np.float32)) for i in range(4)]
    return geo, color


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--grad", action="store_true", help="also time sdf_normal against the SDF-only forward and a torch autograd chain")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = tuple(args.res)
    bounds = np.array([[-0.6, -1.0, -0.3], [0.6, 1.0, 0.3]], np.float32)
    geo, color = recipe()
    field = tf.TemplateField(geo, color, multires=6)
    n = res[0] * res[1] * res[2]
    macs_fused = sum(w.size for w, _ in geo[:-1]) + geo[-1][0].shape[1]
    macs_chain = sum(w.size for w, _ in geo)

    weights = [(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)) for w, b in geo]
    axes = [a.to(dev) for a in tf.volume_axes(bounds, res)]
    step = max(1, tf.GRID_CHUNK // (res[1] * res[2]))

    def chain(x):
        e = torch.cat([x] + [fn(x * float(2 ** k)) for k in range(6) for fn in (torch.sin, torch.cos)], -1)
        h = e
        for l, (w, b) in enumerate(weights):
            if l == 4:
                h = torch.cat([h, e], -1)
            h = F.linear(h, w, b)
            if l < len(weights) - 1:
                h = F.softplus(h, beta=100)
        return h

    def slabs():
        for x0 in range(0, res[0], step):
            x1 = min(res[0], x0 + step)
            yield x0 * res[1] * res[2], x1 * res[1] * res[2], tf.volume_points(axes, x0, x1)

    def torch_chain():
        out = torch.empty(n, dtype=torch.float32, device=dev)
        for p0, p1, x in slabs():
            out[p0:p1] = -chain(x)[:, 0]
        return out.view(res)

    def sdf_normal():
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        for p0, p1, x in slabs():
            out[p0:p1] = field.sdf_normal(x)["normal"]
        return out

    def sdf_only():
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
        for p0, p1, x in slabs():
            out[p0:p1] = field(x)["sdf"]
        return out

    def torch_autograd():
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        for p0, p1, x in slabs():
            x.requires_grad_()
            s = chain(x)[:, :1]
            out[p0:p1] = torch.autograd.grad(s, x, torch.ones_like(s))[0]
        return out

    def timed(fn, iters=args.iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    runs = [{"sdf_grid": timed(lambda: field.sdf_grid(bounds, res, dev)), "torch_chain": timed(torch_chain)} for _ in range(args.runs)]
    ms = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    a, b = field.sdf_grid(bounds, res, dev), torch_chain()
    out = {"res": list(res), "points": n, "iters": args.iters, "blob_bytes": int(field.blob.nbytes),
           "macs_per_point": {"fused_sdf_only": int(macs_fused), "torch_chain": int(macs_chain)},
           "ms": {k: round(v, 3) for k, v in ms.items()}, "ms_runs": [{k: round(v, 3) for k, v in r.items()} for r in runs],
           "tflops": {"sdf_grid": round(2.0 * macs_fused * n / (ms["sdf_grid"] * 1e-3) / 1e12, 2),
                      "torch_chain": round(2.0 * macs_chain * n / (ms["torch_chain"] * 1e-3) / 1e12, 2)},
           "fraction_of_155TF": round(2.0 * macs_fused * n / (ms["sdf_grid"] * 1e-3) / PEAK_F32_MATRIX, 3),
           "fused_over_torch": round(ms["sdf_grid"] / ms["torch_chain"], 3),
           "lds_bytes_per_workgroup": 144896, "workgroups_per_cu": 1, "waves_per_simd": 2,
           "max_abs_difference": float((a - b).abs().max()), "sdf_range": [float(a.min()), float(a.max())],
           "allow_tf32": bool(torch.backends.cuda.matmul.allow_tf32)}
    if args.grad:
        legs = {"sdf_normal": sdf_normal, "sdf_only": sdf_only, "torch_autograd": torch_autograd}
        gruns = [{k: timed(fn) for k, fn in legs.items()} for _ in range(args.runs)]
        gms = {k: float(np.median([r[k] for r in gruns])) for k in legs}
        ga, gb = sdf_normal(), torch_autograd()
        out["grad"] = {"ms": {k: round(v, 3) for k, v in gms.items()}, "ms_runs": [{k: round(v, 3) for k, v in r.items()} for r in gruns],
                       "sdf_normal_over_sdf_only": round(gms["sdf_normal"] / gms["sdf_only"], 3),
                       "sdf_normal_over_torch_autograd": round(gms["sdf_normal"] / gms["torch_autograd"], 3),
                       "tflops_sdf_normal": round(2.0 * 4 * macs_fused * n / (gms["sdf_normal"] * 1e-3) / 1e12, 2),
                       "max_abs_difference": float((ga - gb).abs().max()), "largest_component": float(gb.abs().max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
