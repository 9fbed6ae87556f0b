"""numpy restatement of the weight-volume sampler's contract (``include/ag_weight_volume.h``): trilinear samples of a channel-last
[X, Y, Z, C] volume with ``F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True)`` semantics, as
``network/volume.py:72-93`` calls it.  ``dtype=np.float64`` is the oracle; ``dtype=np.float32`` evaluates the header's operation order
with every operation rounded to fp32 (numpy has no FMA) and gives the error scale of one legitimate fp32 evaluation."""
import os

import numpy as np

# outputs of the reference's own class (golden/make_golden_weight_volume.py): (stored output, volume, points, with bounds)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_volume_ref.npz")
FIXTURE_CASES = [("w_diff", "diff_weight_volume", "points", True), ("w_ori", "ori_weight_volume", "points", True),
                 ("w_unit", "diff_weight_volume", "points_unit", False), ("sdf", "sdf_volume", "points", True)]


def fixture_case(d, vol, pts, scaled):
    """(volume [X, Y, Z, C], points, bounds or None) of one stored output of the fixture ``d``."""
    v = d[vol]
    return (v[..., None] if v.ndim == 3 else v), d[pts], (d["volume_bounds"] if scaled else None)


def sample(volume, points, bounds=None, dtype=np.float64):
    """volume [X, Y, Z, C], points [N, 3] (point x -> first volume axis), bounds [2, 3] (lo, hi) or None (``requires_scale=False``)
    -> [N, C] in ``dtype``."""
    T = dtype
    vol = np.asarray(volume).astype(T)
    p = np.asarray(points).astype(T).reshape(-1, 3)
    R = vol.shape[:3]
    idx, fr, er = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(3):
            u = p[:, d]
            if bounds is not None:
                lo, hi = T(np.asarray(bounds)[0][d]), T(np.asarray(bounds)[1][d])
                u = (u - lo) / (hi - lo)
            g = T(2) * u - T(1)
            x = ((g + T(1)) / T(2)) * T(R[d] - 1)
            x = np.where(np.isnan(x), T(0), x)                                  # fmaxf(NaN, 0) = 0
            x = np.minimum(np.maximum(x, T(0)), T(R[d] - 1)).astype(T)
            fl = np.floor(x)
            idx.append(fl.astype(np.int64))
            fr.append((x - fl).astype(T))
            er.append(((fl + T(1)) - x).astype(T))
    acc = np.zeros((p.shape[0], vol.shape[3]), T)
    for k in range(8):
        a, b, c = k >> 2, (k >> 1) & 1, k & 1
        w = ((fr[2] if c else er[2]) * (fr[1] if b else er[1])) * (fr[0] if a else er[0])
        j0, j1, j2 = idx[0] + a, idx[1] + b, idx[2] + c
        ok = (j0 < R[0]) & (j1 < R[1]) & (j2 < R[2])
        rows = vol[np.minimum(j0, R[0] - 1), np.minimum(j1, R[1] - 1), np.minimum(j2, R[2] - 1)]
        acc = np.where(ok[:, None], (acc + w[:, None] * rows).astype(T), acc)
    return acc


def special_points(bounds, res, rng, n_random):
    """[n, 3] float32 points in world space: random ones inside and up to 15 % outside the bounds on every side, every grid node when
    there are few (else a random subset), ``lo`` and ``hi`` themselves, and the six points one extent outside a face."""
    lo, hi = np.asarray(bounds, np.float64)
    ext = hi - lo
    pts = [lo + ext * rng.uniform(-0.15, 1.15, (n_random, 3))]
    axes = [lo[d] + ext[d] * np.arange(res[d]) / (res[d] - 1) for d in range(3)]
    nodes = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    if len(nodes) > 512:
        nodes = nodes[rng.choice(len(nodes), 512, replace=False)]
    pts.append(nodes)
    pts.append(np.stack([lo, hi, 0.5 * (lo + hi)]))
    for d in range(3):
        for s in (-1.0, 2.0):
            q = 0.5 * (lo + hi)
            q[d] = lo[d] + s * ext[d]
            pts.append(q[None])
    return np.concatenate(pts, 0).astype(np.float32)
