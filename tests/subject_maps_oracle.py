"""Float64 restatement of the canonical-map pipeline (``include/ag_subject_maps.h``), the contract the device kernels are tested
against.  numpy only; no file of the reference is read.

What is restated (reference lines for orientation; none of its text is used):
  * the orthographic ``vertex_attribute`` render: pixel centres as sample points, back-face culling with counter-clockwise = front in
    window space, depth test "less", equal depth -> lower face index, top-left fill rule, rows flipped, back view mirrored
    (utils/renderer/renderer_gl.py:363-375,465-475,525-549; gen_data/gen_pos_maps.py:93-124);
  * barycentric interpolation of per-vertex attributes; the brute-force nearest face of a point (gen_pos_maps.py:24-39);
  * brute-force k-NN squared distances (gaussians/gaussian_model.py:170-171).

Vertex stage: the window coordinates and the depth are computed in FLOAT32 in the header's operand order (numpy rounds every
operation, as the kernel compiled without contraction does) and are then THE vertices: like a hardware rasterizer's snapping to its
sub-pixel grid, this is part of the contract, so that coverage is a property of exactly representable vertices.  Everything after it
runs in ``dtype``: float64 is the oracle, float32 (same operation order as the kernel) measures what fp32 evaluation costs.

Fragile pixels (float64 run only): a decision that an fp32 evaluation may legitimately take the other way.
  (1) edge: the centre is within EDGE_TOL = 1e-3 px of an edge of the winning face; and, the same criterion seen from the other side, a
      front face that misses the centre by less than 1e-3 px takes part in (2) as a runner-up;
  (2) depth: the runner-up's depth is closer to the winner's than the two depth error bounds together.  Bound for one face at one
      sample, u = 2^-24, from the kernel's operation sequence:
        E_i = sgn (dx (py - ay) - dy (px - ax)):  4 roundings feed each product (two differences, the product itself, and the final
              difference is bounded by the products)             dE_i <= 4 u M_i,   M_i = |dx (py - ay)| + |dy (px - ax)|
        A = (E_0 + E_1) + E_2                                    dA   <= sum dE_i + 2 u |A|
        b_i = E_i / A                                            db_i <= (dE_i + |b_i| dA) / |A| + u |b_i|
        b_2 = (1 - b_0) - b_1, depth = (b_0 d_0 + b_1 d_1) + b_2 d_2 = d_2 + b_0 (d_0 - d_2) + b_1 (d_1 - d_2) + roundings
                                                                 dz   <= db_0 |d_0 - d_2| + db_1 |d_1 - d_2| + 2 u |d_2| + 3 u max|d|
"""
from __future__ import annotations

import numpy as np

EDGE_TOL = 1e-3
U32 = 2.0 ** -24


def canonical_views(vertices: np.ndarray):
    """(cano_center, front 3x4, back 3x4) as float32: see animatablegaussians_amd/subject_maps.py for the derivation.  Front: window x
    = x - cx, depth = -(z - cz).  Back (before its mirror): window x = -(x - cx), depth = z - cz."""
    v = np.asarray(vertices, np.float32)
    c = (np.float32(0.5) * (v.min(0) + v.max(0))).astype(np.float32)
    front = np.array([[1, 0, 0, -c[0]], [0, 1, 0, -c[1]], [0, 0, -1, c[2]]], np.float32)
    back = np.array([[-1, 0, 0, c[0]], [0, 1, 0, -c[1]], [0, 0, 1, -c[2]]], np.float32)
    return c, front, back


def window_vertices(vertices, view, W, H):
    """fp32, the header's order: n_k = ((m0 x + m1 y) + m2 z) + m3;  wx = (n_0 + 1)(0.5 W), wy = (n_1 + 1)(0.5 H), depth = n_2."""
    v = np.asarray(vertices, np.float32)
    m = np.asarray(view, np.float32).reshape(3, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    n = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
    one = np.float32(1)
    return ((n[0] + one) * (np.float32(0.5) * np.float32(W))).astype(np.float32), \
           ((n[1] + one) * (np.float32(0.5) * np.float32(H))).astype(np.float32), n[2].astype(np.float32)


class _Edge:
    """Edge walked (x0, y0) -> (x1, y1): canonical end-point order (lexicographic), sign, top-left ownership."""

    def __init__(self, x0, y0, x1, y1):
        self.tl = (y1 < y0) or (y1 == y0 and x1 < x0)
        swap = (x1 < x0) or (x1 == x0 and y1 < y0)
        ax, ay, bx, by = (x1, y1, x0, y0) if swap else (x0, y0, x1, y1)
        self.ax, self.ay, self.dx, self.dy = ax, ay, bx - ax, by - ay
        self.neg = swap

    def value(self, px, py):
        e = self.dx * (py - self.ay) - self.dy * (px - self.ax)
        return -e if self.neg else e

    def magnitude(self, px, py):
        return np.abs(self.dx * (py - self.ay)) + np.abs(self.dy * (px - self.ax))

    def length(self):
        return float(np.hypot(float(self.dx), float(self.dy)))


def rasterize(vertices, faces, view, W, H, cull=True, flip_rows=True, mirror_cols=False, dtype=np.float64, fragile=None):
    """-> dict(face_id [H, W] int32, bary [H, W, 3] dtype, fragile [H, W] bool or None).  ``fragile`` defaults to dtype == float64."""
    T = np.dtype(dtype).type
    if fragile is None:
        fragile = T is np.float64
    wx32, wy32, d32 = window_vertices(vertices, view, W, H)
    wx, wy, dd = wx32.astype(T), wy32.astype(T), d32.astype(T)
    faces = np.asarray(faces).astype(np.int64)
    best_z = np.full((H, W), np.inf, T)
    best_id = np.full((H, W), -1, np.int32)
    bary = np.zeros((H, W, 3), T)
    if fragile:
        best_err = np.zeros((H, W))
        best_near = np.zeros((H, W), bool)
        other_lo = np.full((H, W), np.inf)
    half, onev = T(0.5), T(1)
    pad = 1 if fragile else 0
    V = wx.shape[0]
    for f in range(faces.shape[0]):
        i0, i1, i2 = faces[f]
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V:
            continue
        x0, y0, x1, y1, x2, y2 = wx[i0], wy[i0], wx[i1], wy[i1], wx[i2], wy[i2]
        z0, z1, z2 = dd[i0], dd[i1], dd[i2]
        e01 = _Edge(x0, y0, x1, y1)
        area = e01.value(x2, y2)
        if not (area > 0 or area < 0):
            continue
        swapped = False
        if area < 0:
            if cull:
                continue
            x1, y1, z1, x2, y2, z2 = x2, y2, z2, x1, y1, z1
            swapped = True
            e01 = _Edge(x0, y0, x1, y1)
        e12, e20 = _Edge(x1, y1, x2, y2), _Edge(x2, y2, x0, y0)
        mnx, mxx, mny, mxy = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
        gx0, gx1 = max(int(np.ceil(float(mnx) - 0.5)) - pad, 0), min(int(np.floor(float(mxx) - 0.5)) + pad, W - 1)
        gy0, gy1 = max(int(np.ceil(float(mny) - 0.5)) - pad, 0), min(int(np.floor(float(mxy) - 0.5)) + pad, H - 1)
        if gx1 < gx0 or gy1 < gy0:
            continue
        px = (np.arange(gx0, gx1 + 1).astype(T) + half)[None, :]
        py = (np.arange(gy0, gy1 + 1).astype(T) + half)[:, None]
        w0, w1, w2 = e12.value(px, py), e20.value(px, py), e01.value(px, py)
        cov = ((w0 > 0) | ((w0 == 0) & e12.tl)) & ((w1 > 0) | ((w1 == 0) & e20.tl)) & ((w2 > 0) | ((w2 == 0) & e01.tl))
        A = (w0 + w1) + w2
        cov &= A > 0
        cand = cov
        if fragile:
            l0, l1, l2 = max(e12.length(), 1e-300), max(e20.length(), 1e-300), max(e01.length(), 1e-300)
            s0, s1, s2 = w0 / l0, w1 / l1, w2 / l2                                    # signed distances to the three edge lines, px
            near_edge = (s0 < EDGE_TOL) | (s1 < EDGE_TOL) | (s2 < EDGE_TOL)
            cand = cov | ((s0 > -EDGE_TOL) & (s1 > -EDGE_TOL) & (s2 > -EDGE_TOL) & (A > 0))
        if not cand.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            b0 = w0 / A
            b1 = w1 / A
        b2 = (onev - b0) - b1
        z = ((b0 * z0 + b1 * z1) + b2 * z2) + T(0)
        sl = (slice(gy0, gy1 + 1), slice(gx0, gx1 + 1))
        bz = best_z[sl]
        better = cov & (z < bz)
        if fragile:
            aA = np.abs(A)
            dE0, dE1, dE2 = 4 * U32 * e12.magnitude(px, py), 4 * U32 * e20.magnitude(px, py), 4 * U32 * e01.magnitude(px, py)
            dA = dE0 + dE1 + dE2 + 2 * U32 * aA
            with np.errstate(divide="ignore", invalid="ignore"):
                db0 = (dE0 + np.abs(b0) * dA) / aA + U32 * np.abs(b0)
                db1 = (dE1 + np.abs(b1) * dA) / aA + U32 * np.abs(b1)
            err = db0 * abs(float(z0 - z2)) + db1 * abs(float(z1 - z2)) + 2 * U32 * abs(float(z2)) \
                + 3 * U32 * max(abs(float(z0)), abs(float(z1)), abs(float(z2)))
            ol, be, bn = other_lo[sl], best_err[sl], best_near[sl]
            had = better & np.isfinite(bz)
            ol[had] = np.minimum(ol[had], (bz - be)[had])                           # the dethroned winner becomes a runner-up
            lose = cand & ~better
            ol[lose] = np.minimum(ol[lose], (z - err)[lose])
            be[better] = err[better]
            bn[better] = near_edge[better]
        if better.any():
            bz[better] = z[better]
            best_id[sl][better] = f
            bb = bary[sl]
            bb[..., 0][better] = b0[better]
            bb[..., 1][better] = (b2 if swapped else b1)[better]
            bb[..., 2][better] = (b1 if swapped else b2)[better]
    frag = None
    if fragile:
        frag = (best_id >= 0) & (best_near | (other_lo <= best_z + best_err))
    out = {"face_id": best_id, "bary": bary, "fragile": frag}
    for k, a in out.items():
        if a is None:
            continue
        if flip_rows:
            a = a[::-1]
        if mirror_cols:
            a = a[:, ::-1]
        out[k] = np.ascontiguousarray(a)
    return out


def canonical_raster(vertices, faces, S, dtype=np.float64):
    """Front | back canvas [S, 2S]: dict(face_id, bary, fragile, cano_center)."""
    c, front, back = canonical_views(vertices)
    a = rasterize(vertices, faces, front, S, S, dtype=dtype)
    b = rasterize(vertices, faces, back, S, S, mirror_cols=True, dtype=dtype)
    out = {k: (None if a[k] is None else np.concatenate([a[k], b[k]], 1)) for k in a}
    out["cano_center"] = c
    return out


def resolve(face_id, bary, faces, attribute, dtype=np.float64):
    """(b0 a[f0] + b1 a[f1]) + b2 a[f2] in ``dtype``; zeros on empty pixels."""
    T = np.dtype(dtype).type
    faces = np.asarray(faces).astype(np.int64)
    a = np.asarray(attribute).astype(T)
    b = np.asarray(bary).astype(T)
    m = face_id >= 0
    out = np.zeros(face_id.shape + (a.shape[1],), T)
    tri = faces[face_id[m]]
    bm = b[m]
    out[m] = (bm[:, 0:1] * a[tri[:, 0]] + bm[:, 1:2] * a[tri[:, 1]]) + bm[:, 2:3] * a[tri[:, 2]]
    return out


def pixel_centre_xy(S, cano_center):
    """World (x, y) every covered pixel of the [S, 2S] canvas must carry: x = cx + (2c+1)/S - 1, y = cy + 1 - (2r+1)/S, both halves."""
    c = np.arange(S, dtype=np.float64)
    x = float(cano_center[0]) + (2 * c + 1) / S - 1
    y = float(cano_center[1]) + 1 - (2 * c + 1) / S
    X = np.broadcast_to(np.concatenate([x, x])[None, :], (S, 2 * S))
    Y = np.broadcast_to(y[:, None], (S, 2 * S))
    return X, Y


def nearest_face_barycentric(points, vertices, faces, chunk=64):
    """Brute force, float64: for every point the face with the smallest distance (lowest index on ties) and the barycentrics of the
    closest point on it."""
    v = np.asarray(vertices, np.float64)
    faces = np.asarray(faces).astype(np.int64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    ab, ac, bc = b - a, c - a, c - b
    n = np.cross(ab, ac)
    nn = (n * n).sum(1)
    ok = nn > 0
    nn_safe = np.where(ok, nn, 1.0)
    P = np.asarray(points, np.float64)
    ids = np.zeros(len(P), np.int64)
    bar = np.zeros((len(P), 3))

    def seg(p, s0, d):                                                     # closest point of segment s0 + t d
        t = np.clip(((p - s0) * d).sum(-1) / np.maximum((d * d).sum(-1), 1e-300), 0.0, 1.0)
        q = s0 + t[..., None] * d
        return t, ((p - q) ** 2).sum(-1)

    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        ap = p - a[None]
        wv = (np.cross(ab[None], ap) * n[None]).sum(-1) / nn_safe              # weight of c
        vv = (np.cross(ap, ac[None]) * n[None]).sum(-1) / nn_safe              # weight of b
        uu = 1.0 - vv - wv
        inside = ok[None] & (uu >= 0) & (vv >= 0) & (wv >= 0)
        dplane = (ap * n[None]).sum(-1) ** 2 / nn_safe
        t0, d0 = seg(p, a[None], ab[None])
        t1, d1 = seg(p, a[None], ac[None])
        t2, d2 = seg(p, b[None], bc[None])
        de = np.stack([d0, d1, d2], -1)
        ke = de.argmin(-1)
        dmin = np.where(inside, dplane, de.min(-1))
        dmin = np.where(ok[None], dmin, np.inf)
        j = dmin.argmin(1)
        r = np.arange(len(j))
        eb = np.stack([np.stack([1 - t0, t0, np.zeros_like(t0)], -1), np.stack([1 - t1, np.zeros_like(t1), t1], -1),
                       np.stack([np.zeros_like(t2), 1 - t2, t2], -1)], -2)[r, j]            # [chunk, 3 edges, 3]
        bj = np.where(inside[r, j][:, None], np.stack([uu[r, j], vv[r, j], wv[r, j]], -1), eb[r, ke[r, j]])
        ids[s:s + chunk], bar[s:s + chunk] = j, bj
    return ids, bar


def knn3_dist2(points, chunk=512):
    """Brute force, float64: ascending squared distances [N, 3] to the 3 nearest OTHER entries (K = 4 including the point itself,
    smallest dropped: with exact duplicates ONE zero is dropped)."""
    p = np.asarray(points, np.float64)
    out = np.zeros((len(p), 3))
    for s in range(0, len(p), chunk):
        d = ((p[s:s + chunk, None, :] - p[None]) ** 2).sum(-1)
        out[s:s + chunk] = np.sort(np.partition(d, 3, axis=1)[:, :4], axis=1)[:, 1:]
    return out


def lattice_mesh(S=32, n=6, step=3):
    """(vertices, faces): an n x n quad lattice, two triangles per quad with alternating diagonals, whose window-space vertices sit
    exactly ON pixel centres of an S x S target (S a power of two, centre of the bounding box at the origin): every product in the edge
    functions is exact in fp32 and fp64, and many pixel centres lie exactly on shared edges and vertices."""
    k = np.arange(n + 1) * step
    k = k - k.max() // 2                                                   # symmetric up to parity: handled by the centre below
    gx, gy = np.meshgrid(k, k, indexing="xy")
    v = np.stack([gx.reshape(-1) * 2.0 / S, gy.reshape(-1) * 2.0 / S, 0.01 * ((gx + 2 * gy) % 3).reshape(-1)], 1)
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            faces += [[a, b, d], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, c], [b, d, c]]
    return v.astype(np.float32), np.asarray(faces, np.int32)


def lattice_view(S):
    """World -> NDC for ``lattice_mesh``: window x = x * S/2 + S/2 + 0.5 px, i.e. lattice vertices land on pixel centres."""
    o = np.float32(1.0 / S)
    return np.array([[1, 0, 0, o], [0, 1, 0, o], [0, 0, -1, 0]], np.float32)
