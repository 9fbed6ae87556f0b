#!/usr/bin/env python
"""Time the closest-point kernels at the size of a blend-weight volume.

    python profiles/mesh_query.py [--res 128] [--iters 3]

N = res^3 grid nodes about ``synth.body_mesh()`` (F = 21 096 faces, J = 55): the closest-point kernel with each walk (``'uniform'``:
records through the scalar cache; ``'tiled'``: records through LDS; the face-record kernel is included, 21 k threads), the dense
resolve of the J = 55 weights on its result, the pseudonormal sign, and the whole ``WeightVolume.from_body_mesh``.  One process,
device events around ``iters`` back-to-back calls after one warm-up call, the walks alternating in 3 rounds.  Prints one JSON line:
times, pair tests per second, and their share of the fp32 vector peak given the VALU instructions per pair counted in the compiled
loop body (``--valu-per-pair``; 106 for the uniform walk, 102 + 4 LDS reads for the tiled one at the time of writing) against
256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz = 78.6e12 lane-operations per second (the 157.3 TFLOPS of the data sheet count an FMA twice; nothing here contracts).  No time here is a pass / fail condition.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from animatablegaussians_amd import mesh_query, subject_maps as sm, synth  # noqa: E402
from animatablegaussians_amd.weight_volume import WeightVolume, body_bounds, grid_axes  # noqa: E402

PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--valu-per-pair", type=float, default=106.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = synth.body_mesh()
    v, f, w = t(m["vertices"]), t(m["faces"]), t(m["lbs_weights"])
    axes = [t(a) for a in grid_axes(body_bounds(m["vertices"].min(0), m["vertices"].max(0))[0], (args.res,) * 3)]
    N, F = args.res ** 3, f.shape[0]

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

    walk = {k: (lambda k=k: mesh_query._run(None, axes, v, f, k)) for k in ("uniform", "tiled")}
    rounds = [{k: timed(fn) for k, fn in walk.items()} for _ in range(3)]
    ms = {k: float(np.median([r[k] for r in rounds])) for k in walk}
    a, b = walk["uniform"](), walk["tiled"]()
    same = all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    dist2, face_id, bary, feature = a[:4]
    ms_resolve = timed(lambda: sm.resolve(face_id, bary, f, w), 10)
    ms_signed = timed(lambda: mesh_query.grid_signed_distance(axes, v, f), 1)
    ms_whole = timed(lambda: WeightVolume.from_body_mesh(v, f, w, res=args.res), 1)
    pairs = float(N) * F
    out = {"N": N, "F": F, "J": int(w.shape[1]), "iters": args.iters, "pair_tests": pairs, "walks_bit_identical": same,
           "valu_per_pair": args.valu_per_pair, "resolve_ms": round(ms_resolve, 3), "grid_signed_distance_ms": round(ms_signed, 2),
           "from_body_mesh_ms": round(ms_whole, 2), "cull": "not built (the optional second step of the issue)"}
    for k in walk:
        rate = pairs / (ms[k] * 1e-3)
        out[k] = {"ms": round(ms[k], 2), "ms_rounds": [round(r[k], 2) for r in rounds], "pair_tests_per_s": rate,
                  "share_of_fp32_vector_peak": round(rate * args.valu_per_pair / PEAK_LANE_OPS, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
