#!/usr/bin/env python
"""Time inverse skinning at the workload's own shape.

    python profiles/inverse_skinning.py [--res 128] [--points 1048576] [--iterations 10] [--iters 3]

The 128^3 x 55 nearest-surface volume of ``synth.body_mesh()`` (461 MB), 2^20 canonical points within 3 cm of its surface posed with
``transform_cano2live`` under joint rotations of up to 0.3 rad, initial guesses off by up to 2 cm per axis.  Timed with device events
around ``iters`` back-to-back calls after one warm-up call, the two gradient modes of ``WeightVolume.root_find`` alternating in 3 rounds
(median reported, rounds listed): on the fly (27 rows of 4 J bytes around the node per point and iteration) and from a precomputed
``gradient_volume`` (one row of 4 J and one of 12 J bytes), then ``gradient_volume`` itself (reads the volume, writes 3 x its size) and
``initial_guess``.  Prints one JSON line: times, the bytes each REQUESTS (neighbouring points share nodes and neighbouring nodes share
rows, so most requests are served by the caches: the figure bounds cache traffic, not HBM traffic) and that rate against the HBM
rate reached by a copy (6.3 TB/s) and the aggregate L2 rate (34.5 TB/s).  The two modes are also compared bit for bit.  No time here
is a pass / fail condition.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from animatablegaussians_amd import inverse_skinning as inv, synth  # noqa: E402
from animatablegaussians_amd.weight_volume import WeightVolume  # noqa: E402

HBM_RATE, L2_RATE = 6.3e12, 34.5e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import inverse_skinning_oracle as iso
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = synth.body_mesh()
    vol = WeightVolume.from_body_mesh(t(m["vertices"]), t(m["faces"]), t(m["lbs_weights"]), res=args.res)
    J, N = vol.joint_num, args.points
    rng = np.random.RandomState(0)
    v = m["vertices"].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    centres = np.tile(0.5 * (lo + hi), (J, 1))
    centres[:, 1] = np.linspace(lo[1], hi[1], J)
    mats = t(iso.joint_matrices(rng, 1, J, centres, max_angle=0.3))
    cano = t((v[rng.randint(0, len(v), N)] + rng.uniform(-0.03, 0.03, (N, 3))).astype(np.float32)[None])
    posed = inv.transform_cano2live(cano, mats, vol, with_hand=True)
    guess = cano + t(rng.uniform(-0.02, 0.02, (1, N, 3)).astype(np.float32))
    weights = vol.forward_weight(cano)

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

    ms_grad = timed(vol.gradient_volume)
    grad = vol.gradient_volume()
    modes = {"on_the_fly": lambda: vol.root_find(posed, guess, mats, iterations=args.iterations),
             "gradient_volume": lambda: vol.root_find(posed, guess, mats, iterations=args.iterations, grad_volume=grad)}
    rounds = [{k: timed(fn) for k, fn in modes.items()} for _ in range(3)]
    ms = {k: float(np.median([r[k] for r in rounds])) for k in modes}
    a, b = modes["on_the_fly"](), modes["gradient_volume"]()
    ms_init = timed(lambda: inv.initial_guess(posed, weights, mats), 10)
    nodes = float(args.res) ** 3
    requested = {"on_the_fly": 27.0 * 4 * J * N * args.iterations, "gradient_volume": 16.0 * J * N * args.iterations}
    out = {"res": args.res, "J": J, "points": N, "iterations": args.iterations, "iters": args.iters, "modes_bit_identical": bool(torch.equal(a, b)),
           "refined_minus_canonical_max": float((a - cano).abs().max()), "guess_minus_canonical_max": float((guess - cano).abs().max()),
           "gradient_volume_build": {"ms": round(ms_grad, 3), "bytes": 16.0 * J * nodes, "share_of_hbm_rate": round(16.0 * J * nodes / (ms_grad * 1e-3) / HBM_RATE, 4)},
           "initial_guess": {"ms": round(ms_init, 3), "bytes": (4.0 * J + 24) * N,
                             "share_of_hbm_rate": round((4.0 * J + 24) * N / (ms_init * 1e-3) / HBM_RATE, 4)}}
    for k in modes:
        rate = requested[k] / (ms[k] * 1e-3)
        out[k] = {"ms": round(ms[k], 3), "ms_rounds": [round(r[k], 3) for r in rounds], "ns_per_point_iteration": round(ms[k] * 1e6 / (N * max(args.iterations, 1)), 3),
                  "requested_bytes": requested[k], "requested_bytes_per_s": rate, "over_hbm_rate": round(rate / HBM_RATE, 4),
                  "over_l2_rate": round(rate / L2_RATE, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
