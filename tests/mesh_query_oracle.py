"""numpy restatement of ``include/ag_mesh_query.h``: the closest point of a triangle mesh by brute force over all faces, the pseudonormal
sign, and -- independent of both -- the generalized winding number as an inside / outside test of closed meshes.

``closest_point(..., dtype)`` runs ONE code in float64 (the contract) and in float32: numpy rounds every array operation on its own
and has no FMA, so the float32 run performs the header's operations in the header's order, which is what the kernel (compiled
without contraction) performs.  The minimum over faces takes the lowest face index on equal d2 (``np.argmin`` returns the first), the
header's tie rule.
"""
import numpy as np


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _recip_or_zero(x):
    pos = x > 0
    return np.where(pos, 1 / np.where(pos, x, 1), 0).astype(x.dtype)


def face_records(vertices, faces, dtype):
    """The per-face record of the header (arrays over F) and ``valid`` (every index inside [0, V))."""
    v = np.asarray(vertices).astype(dtype)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    V = len(v)
    valid = ((f >= 0) & (f < V)).all(1) if V else np.zeros(len(f), bool)
    fc = np.clip(f, 0, max(V - 1, 0))
    if V == 0:
        v = np.zeros((1, 3), dtype)
    v0, v1, v2 = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    e0, e1 = v1 - v0, v2 - v0
    e2 = e1 - e0
    a, b, c, h = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e2)
    return {"v0": v0, "e0": e0, "e1": e1, "a": a, "b": b, "c": c, "ia": _recip_or_zero(a), "ic": _recip_or_zero(c), "ih": _recip_or_zero(h),
            "idet": _recip_or_zero(a * c - b * b), "valid": valid, "faces": f}


def _clamp01(x):
    return np.minimum(np.maximum(x, 0), 1)


def pair_tests(rec, q):
    """Every (query, face) pair: q [n, 3] -> (d2, b0, b1, b2, feature), each [n, F]; the header's four candidates and their order."""
    dt = rec["a"].dtype
    one, zero = dt.type(1), dt.type(0)
    rec = {k: (x[None] if rec["a"].ndim == 1 else x) for k, x in rec.items()}     # [F] records for all queries, or [n, K] per query
    D = rec["v0"] - q[:, None, :]
    e0, e1 = rec["e0"], rec["e1"]
    a, b, c = rec["a"], rec["b"], rec["c"]
    d, e = _dot(e0, D), _dot(e1, D)
    det = a * c - b * b
    sn, tn = b * e - c * d, b * d - a * e
    inside = (sn >= 0) & (tn >= 0) & (sn + tn <= det) & (det > 0)

    def dist2(s, t):
        r = (D + s[..., None] * e0) + t[..., None] * e1
        return _dot(r, r)

    s0, t0 = sn * rec["idet"], tn * rec["idet"]
    s1 = _clamp01(zero - d * rec["ia"])
    u2 = _clamp01(((a - b) + (d - e)) * rec["ih"])
    t3 = _clamp01(zero - e * rec["ic"])
    z = np.zeros_like(s1)
    with np.errstate(invalid="ignore"):
        d2 = np.where(inside, dist2(s0, t0), np.inf).astype(dt)
        b0, b1, b2 = np.maximum((one - s0) - t0, 0), s0, t0
        feat = np.zeros(d2.shape, np.int32)
        for k, (dk, c0, c1, c2, par, codes) in enumerate((
                (dist2(s1, z), one - s1, s1, z, s1, (1, 4, 5)),
                (dist2(one - u2, u2), z, one - u2, u2, u2, (2, 5, 6)),
                (dist2(z, t3), one - t3, z, t3, t3, (3, 4, 6)))):
            take = dk < d2
            d2 = np.where(take, dk, d2)
            b0, b1, b2 = np.where(take, c0, b0), np.where(take, c1, b1), np.where(take, c2, b2)
            feat = np.where(take, np.where(par <= 0, codes[1], np.where(par >= 1, codes[2], codes[0])), feat).astype(np.int32)
    d2 = np.where(rec["valid"], d2, np.inf).astype(dt)
    return d2, b0, b1, b2, feat


def closest_point(points, vertices, faces, dtype=np.float64, chunk=None, other=False, cull=False):
    """-> dict: ``dist2`` [N], ``face`` [N] (-1 without a face), ``bary`` [N, 3], ``feature`` [N]; with ``other``: also ``d_other`` [N],
    the distance (not squared) to the nearest face that shares NO vertex with the returned one (inf if there is none or, with
    ``cull``, none in the band).

    ``cull=False`` is the contract: every pair is tested.  ``cull=True`` tests, per query, only the faces whose bounding sphere
    (centroid c_f, radius R_f) reaches the band  |q - c_f| - R_f <= min_f (|q - c_f| + R_f)  (+ 1e-6 of the mesh size): a face
    outside it cannot hold the closest point, and the band is centimetres wide where roundings are 1e-7, so both runs return what
    the full scan returns (a CPU test checks it); the kept faces stay in ascending index order, so the tie rule is unchanged."""
    rec = face_records(vertices, faces, dtype)
    q = np.asarray(points).astype(dtype).reshape(-1, 3)
    N, F = len(q), len(rec["a"])
    out = {"dist2": np.full(N, np.inf, dtype), "face": np.full(N, -1, np.int64), "bary": np.zeros((N, 3), dtype),
           "feature": np.zeros(N, np.int32)}
    if other:
        out["d_other"] = np.full(N, np.inf)
    if F == 0 or N == 0:
        return out
    chunk = chunk or max(1, int((2e7 if cull else 2e6) // F))
    fidx = rec["faces"]
    if cull:
        v64 = np.asarray(vertices, np.float64)
        tri = v64[np.clip(fidx, 0, max(len(v64) - 1, 0))] if len(v64) else np.zeros((F, 3, 3))
        cen = tri.mean(1)
        rad = np.linalg.norm(tri - cen[:, None], axis=2).max(1)
        slack = 1e-6 * (1.0 + np.abs(v64).max() if len(v64) else 1.0)
    for s in range(0, N, chunk):
        qs = q[s:s + chunk]
        if cull:
            dc = np.linalg.norm(qs.astype(np.float64)[:, None] - cen[None], axis=2)
            dc = np.where(rec["valid"][None], dc, np.inf)
            keep = dc - rad[None] <= (dc + rad[None]).min(1, keepdims=True) + slack
            K = max(int(keep.sum(1).max()), 1)
            ids = np.sort(np.where(keep, np.arange(F)[None], F), 1)[:, :K]                    # ascending face index, F = padding
            pad = ids >= F
            ids = np.where(pad, 0, ids)
            sub = {k: x[ids] for k, x in rec.items()}
            sub["valid"] = sub["valid"] & ~pad
            d2, b0, b1, b2, feat = pair_tests(sub, qs)
        else:
            ids = np.broadcast_to(np.arange(F)[None], (len(qs), F))
            d2, b0, b1, b2, feat = pair_tests(rec, qs)
        col = np.argmin(d2, 1)
        rows = np.arange(len(col))
        best = ids[rows, col]
        m = d2[rows, col]
        hit = np.isfinite(m)
        out["dist2"][s:s + chunk] = np.where(hit, m, np.inf)
        out["face"][s:s + chunk] = np.where(hit, best, -1)
        out["bary"][s:s + chunk] = np.where(hit[:, None], np.stack([b0[rows, col], b1[rows, col], b2[rows, col]], 1), 0)
        out["feature"][s:s + chunk] = np.where(hit, feat[rows, col], 0)
        if other:
            mine = fidx[best]                                                   # [n, 3]
            shares = (fidx[ids][:, :, :, None] == mine[:, None, None, :]).any((2, 3))
            out["d_other"][s:s + chunk] = np.sqrt(np.where(shares, np.inf, d2).min(1).astype(np.float64))
    return out


def closest_points_of(result, vertices, faces):
    """float64 ``b0 v0 + b1 v1 + b2 v2`` of a result (the oracle's or the kernel's): [N, 3]; rows without a face are 0."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    face = np.asarray(result["face"], np.int64)
    ok = face >= 0
    tri = v[f[np.where(ok, face, 0)]]                                           # [N, 3, 3]
    return (np.asarray(result["bary"], np.float64)[:, :, None] * tri).sum(1) * ok[:, None]


def distance_to_face(points, face, vertices, faces):
    """float64 distance of point n to the ONE face ``face[n]``: [N]."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(points, np.float64)
    face = np.asarray(face, np.int64)
    out = np.empty(len(p))
    for s in range(0, len(p), 64):                                             # 64 x 64 pairs per step, the diagonal kept
        d2 = pair_tests(face_records(v, f[face[s:s + 64]], np.float64), p[s:s + 64])[0]
        out[s:s + 64] = np.sqrt(np.diagonal(d2))
    return out


def pseudonormals(vertices, faces):
    """float64 (face normals [F, 3], edge normals [F, 3, 3], vertex normals [V, 3]) as the header defines them: the oracle's own
    construction in numpy (``np.unique`` over undirected edge keys, ``np.add.at``), not the package's sorted dense sums on the device."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    V = len(v)
    valid = ((f >= 0) & (f < V)).all(1)
    fc = np.clip(f, 0, V - 1)
    p = v[fc]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    fn = np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0) * valid[:, None]
    vn = np.zeros((V, 3))
    for k in range(3):
        e1 = p[:, (k + 1) % 3] - p[:, k]
        e2 = p[:, (k + 2) % 3] - p[:, k]
        l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        ok = (l1 > 0) & (l2 > 0) & valid
        cosang = np.clip((e1 * e2).sum(1) / np.where(ok, l1 * l2, 1), -1, 1)
        np.add.at(vn, fc[ok, k], np.arccos(cosang[ok])[:, None] * fn[ok])
    lv = np.linalg.norm(vn, axis=1, keepdims=True)
    vn = np.where(lv > 0, vn / np.where(lv > 0, lv, 1), 0)
    key = np.minimum(fc, np.roll(fc, -1, 1)) * V + np.maximum(fc, np.roll(fc, -1, 1))       # [F, 3]
    key = np.where(valid[:, None], key, -1 - np.arange(3 * len(f)).reshape(-1, 3))
    uniq, inverse = np.unique(key.reshape(-1), return_inverse=True)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inverse.reshape(-1), np.repeat(fn, 3, 0))
    return fn, sums[inverse.reshape(-1)].reshape(-1, 3, 3), vn


def sign(points, result, vertices, faces, normals=None, dtype=np.float64):
    """Pseudonormal sign of each query with respect to ``result`` (+1 outside, -1 inside, 0 undecided / no face), the header's
    operations in ``dtype``: c = (b0 v0 + b1 v1) + b2 v2, w = q - c, (w . n)."""
    fn, en, vn = (np.asarray(x).astype(dtype) for x in (normals if normals is not None else pseudonormals(vertices, faces)))
    f = np.asarray(faces, np.int64)
    v = np.asarray(vertices).astype(dtype)
    face, feat = np.asarray(result["face"], np.int64), np.asarray(result["feature"], np.int64)
    ok = face >= 0
    fs = np.where(ok, face, 0)
    tri = v[np.clip(f[fs], 0, len(v) - 1)]
    b = np.asarray(result["bary"]).astype(dtype)
    c = (b[:, 0:1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:3] * tri[:, 2]
    w = np.asarray(points).astype(dtype) - c
    n = fn[fs]
    edge = (feat >= 1) & (feat <= 3)
    n = np.where(edge[:, None], en[fs, np.clip(feat - 1, 0, 2)], n)
    vert = feat >= 4
    n = np.where(vert[:, None], vn[np.clip(f[fs, np.clip(feat - 4, 0, 2)], 0, len(vn) - 1)], n)
    return np.sign(_dot(w, n)).astype(np.float64) * ok


def winding_number(points, vertices, faces, chunk=None):
    """Generalized winding number (sum of signed solid angles / 4 pi, van Oosterom & Strackee): 1 inside a closed mesh wound
    counter-clockwise seen from outside, 0 outside.  float64, independent of the closest-point code."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(points, np.float64)
    out = np.empty(len(p))
    chunk = chunk or max(1, int(2e6 // max(len(f), 1)))
    for s in range(0, len(p), chunk):
        a = v[f[:, 0]][None] - p[s:s + chunk, None]
        b = v[f[:, 1]][None] - p[s:s + chunk, None]
        c = v[f[:, 2]][None] - p[s:s + chunk, None]
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[s:s + chunk] = np.arctan2(num, den).sum(1) / (2 * np.pi)
    return out


def surface_samples(vertices, faces, rng, n):
    """n points on the surface: random faces, random barycentrics (float64)."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    b = rng.dirichlet(np.ones(3), n)
    return (b[:, :, None] * v[f[rng.integers(0, len(f), n)]]).sum(1)


def deviations(points, vertices, faces, chunk=None, cull=True):
    """What every tolerance of the GPU tests is made of: the float32 run against the float64 run on the same inputs.
    -> (o64, o32, dict of worst deviations): ``d`` distance, ``b`` barycentric validity (negative part, |sum - 1|), ``on`` distance of
    the reconstructed point to its face, ``c`` closest point and ``fragile`` mask of the float64 run (tolerance-free part)."""
    o64 = closest_point(points, vertices, faces, np.float64, chunk, other=True, cull=cull)
    o32 = closest_point(points, vertices, faces, np.float32, chunk, cull=cull)
    dev = measure(o32, o64, points, vertices, faces)
    return o64, o32, dev


def measure(res, o64, points, vertices, faces):
    """The figures the GPU tests bound, of any result ``res`` (dist2, face, bary) against the float64 run ``o64``."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    hit = o64["face"] >= 0
    dmin = np.sqrt(o64["dist2"].astype(np.float64))
    c = closest_points_of(res, vertices, faces)
    bary = np.asarray(res["bary"], np.float64)
    out = {"d": 0.0, "b": 0.0, "on": 0.0}
    if hit.any():
        qc = np.linalg.norm(p - c, axis=1)
        out["d"] = float(max(np.abs(qc - dmin)[hit].max(), np.abs(np.sqrt(np.asarray(res["dist2"], np.float64)) - dmin)[hit].max(),
                             np.abs(np.sqrt(np.asarray(res["dist2"], np.float64)) - qc)[hit].max()))
        out["b"] = float(max(np.maximum(-bary[hit], 0).max(), np.abs(bary[hit].sum(1) - 1).max()))
        out["on"] = float(distance_to_face(c[hit], np.asarray(res["face"], np.int64)[hit], vertices, faces).max())
    return out


# ------------------------------------------------------------ shared inputs ------------------------------------------------------------
def lattice_mesh(n_lat=36, n_lon=36, centre=(0.013, -0.21, 0.017)):
    """A coarse closed lobed surface (``synth._lattice_surface``; 2 n_lat n_lon faces: 2 592), float32 vertices, int32 faces, wound
    counter-clockwise seen from outside."""
    from animatablegaussians_amd import synth

    def lobed(T, P):
        base = 1.0 / np.sqrt((np.sin(T) * np.cos(P) / 0.5) ** 2 + (np.cos(T) / 0.9) ** 2 + (np.sin(T) * np.sin(P) / 0.2) ** 2)
        return base * (1.0 + 0.18 * np.sin(T) ** 2 * np.cos(4.0 * T) * np.cos(2.0 * P) + 0.10 * np.sin(T) ** 2 * np.sin(3.0 * P + 2.0 * T))

    v, f = synth._lattice_surface(lobed, centre, n_lat, n_lon)
    return v.astype(np.float32), f.astype(np.int32)


def mixed_queries(vertices, faces, rng, n):
    """A third random in the 1.1 x bounding cube, a third on the surface, a third the mesh's own vertices and edge midpoints (exact
    ties between the faces around them): [n, 3] float32."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    lo, hi = v.min(0), v.max(0)
    c, half = 0.5 * (lo + hi), 0.55 * (hi - lo).max()
    n1 = n // 3
    n2 = n // 3
    n3 = n - n1 - n2
    cube = c + rng.uniform(-half, half, (n1, 3))
    surf = surface_samples(v, f, rng, n2)
    vi = rng.integers(0, len(v), n3 - n3 // 2)
    fi, k = rng.integers(0, len(f), n3 // 2), rng.integers(0, 3, n3 // 2)
    mids = 0.5 * (v[f[fi, k]].astype(np.float32) + v[f[fi, (k + 1) % 3]].astype(np.float32))
    return np.concatenate([cube, surf, v[vi], mids], 0).astype(np.float32)


def special_mesh():
    """A small closed lattice (8 x 10: 160 faces) plus a DUPLICATE of face 7 (index 160), a ZERO-AREA face (161: two equal corners),
    a collinear zero-area face (162) and a face with an index outside [0, V) (163: skipped)."""
    v, f = lattice_mesh(8, 10)
    V = len(v)
    mid = (0.5 * (v[f[3, 0]] + v[f[3, 1]])).astype(np.float32)
    v = np.concatenate([v, mid[None]], 0)                                        # vertex V: on edge 0 of face 3
    extra = np.array([f[7], [f[20, 0], f[20, 1], f[20, 1]], [f[3, 0], V, f[3, 1]], [0, 1, V + 5]], np.int32)
    return v, np.concatenate([f, extra], 0)


def sparse_weights(vertices, J=55):
    """4-sparse skinning weights [V, J] that vary smoothly along y (the cubic B-spline rows of ``synth.body_mesh``), float32."""
    y = np.asarray(vertices, np.float64)[:, 1]
    s = (y - y.min()) / max(y.max() - y.min(), 1e-12) * (J - 3) * (1.0 - 1e-9)
    k = np.floor(s).astype(np.int64)
    t = s - k
    basis = np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], 1) / 6.0
    w = np.zeros((len(y), J))
    np.put_along_axis(w, k[:, None] + np.arange(4)[None], basis, 1)
    return w.astype(np.float32)


def interpolate(result, faces, attribute, dtype=np.float64):
    """(b0 a[f0] + b1 a[f1]) + b2 a[f2] of a result, the resolve's order, in ``dtype``; rows without a face are 0."""
    f = np.asarray(faces, np.int64)
    a = np.asarray(attribute).astype(dtype)
    face = np.asarray(result["face"], np.int64)
    ok = face >= 0
    idx = f[np.where(ok, face, 0)]
    b = np.asarray(result["bary"]).astype(dtype)
    return ((b[:, 0:1] * a[idx[:, 0]] + b[:, 1:2] * a[idx[:, 1]]) + b[:, 2:3] * a[idx[:, 2]]) * ok[:, None]


def mesh_area_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    t = v[np.asarray(faces, np.int64)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return 0.5 * np.linalg.norm(n, axis=1).sum(), abs((t[:, 0] * n).sum()) / 6.0


def body_grid_nodes(res=24, near=0.045, stride=61):
    """The nodes of the res^3 grid of ``from_body_mesh`` about ``synth.body_mesh(second_component=False)`` that the sign checks
    visit: every node within ``near`` of the body's bounding box and every ``stride``-th of the others (far nodes are all outside and
    all alike; the solid-angle sum costs 1e-5 s per node).  -> (mesh dict, nodes [n, 3] float32, total node count)."""
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.weight_volume import body_bounds, grid_axes
    m = synth.body_mesh(second_component=False)
    v = m["vertices"]
    bounds = body_bounds(v.min(0), v.max(0))[0]
    g = np.stack(np.meshgrid(*grid_axes(bounds, (res,) * 3), indexing="ij"), -1).reshape(-1, 3)
    box = np.maximum(np.maximum(v.min(0) - g, g - v.max(0)), 0)
    close = np.linalg.norm(box, axis=1) < near
    pick = close | (np.arange(len(g)) % stride == 0)
    return m, g[pick].astype(np.float32), len(g)


def one_triangle():
    return np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def voronoi_queries():
    """Queries about ``one_triangle()`` (right angle at v0, legs 2 and 1, in z = 0) placed analytically: (point, expected feature,
    closest point).  Region interiors, each at height z = 0.5 as well, and points exactly on region boundaries, where two codes are
    legitimate and the expected value is ``None``."""
    n = np.array([1.0, 2.0]) / np.sqrt(5.0)                                       # outward normal of the hypotenuse v1v2
    m = np.array([1.0, 0.5])                                                      # its midpoint
    rows = [((0.5, 0.25), 0, (0.5, 0.25)),                                        # face
            ((1.0, -0.5), 1, (1.0, 0.0)),                                         # edge v0v1
            (tuple(m + 0.5 * n), 2, tuple(m)),                                    # edge v1v2
            ((-0.5, 0.5), 3, (0.0, 0.5)),                                         # edge v2v0
            ((-0.5, -0.25), 4, (0.0, 0.0)),                                       # vertex v0
            ((2.5, -0.125), 5, (2.0, 0.0)),                                       # vertex v1
            ((-0.125, 1.5), 6, (0.0, 1.0)),                                       # vertex v2
            ((1.0, 0.0), None, (1.0, 0.0)),                                       # ON edge v0v1: face | edge
            ((0.0, 0.0), None, (0.0, 0.0)),                                       # ON v0
            ((2.0, -0.5), None, (2.0, 0.0)),                                      # boundary of edge v0v1 | vertex v1
            ((-0.5, 0.0), None, (0.0, 0.0)),                                      # boundary of edge v2v0 | vertex v0
            ((-0.5, 1.0), None, (0.0, 1.0)),                                      # boundary of edge v2v0 | vertex v2
            (tuple(np.array([2.0, 0.0]) + 0.5 * n), None, (2.0, 0.0)),            # boundary of edge v1v2 | vertex v1
            ((0.0, -0.5), None, (0.0, 0.0))]                                      # boundary of edge v0v1 | vertex v0
    pts, feats, close = [], [], []
    for (x, y), feat, (cx, cy) in rows:
        for z in (0.0, 0.5):
            pts.append((x, y, z)); feats.append(feat); close.append((cx, cy, 0.0))
    return np.array(pts, np.float64), feats, np.array(close, np.float64)


def host_walk_cases():
    """The CPU test shapes, as (name, vertices, faces, points): what ``profiles/ub/mesh_query_host_walk.hip`` walks."""
    rng = np.random.default_rng(20241)
    cases = []
    v, f = one_triangle()
    cases.append(("one triangle", v, f, voronoi_queries()[0].astype(np.float32)))
    v, f = special_mesh()
    cases.append(("duplicate, zero-area and skipped faces", v, f, mixed_queries(v, f[:160], rng, 257)))
    cases.append(("no valid face", v, f[163:], mixed_queries(v, f[:160], rng, 5)))
    v, f = lattice_mesh(12, 11)
    cases.append(("lattice 12 x 11", v, f, mixed_queries(v, f, rng, 300)))
    vt = (v + np.float32([3, -2, 5])).astype(np.float32)
    cases.append(("translated", vt, f, mixed_queries(vt, f, rng, 129)))
    cases.append(("one face of many", v, f[:1], mixed_queries(v, f, rng, 65)))
    return cases


def export_host_walk(path):
    """Write the cases and the float32 run's results for the host walk: little-endian int32 case count, then per case int32 (V, F,
    N), vertices, faces, points, the float32 normal tables (face [F, 3], edge [F, 3, 3], vertex [V, 3]), and the expected dist2
    [N], face [N] int32, bary [N, 3], feature [N] int32, sign [N] float32."""
    with open(path, "wb") as fh:
        cases = host_walk_cases()
        fh.write(np.int32(len(cases)).tobytes())
        for _, v, f, p in cases:
            o = closest_point(p, v, f, np.float32)
            nrm = [x.astype(np.float32) for x in pseudonormals(v, f)]
            sg = sign(p, o, v, f, nrm, np.float32).astype(np.float32)
            fh.write(np.array([len(v), len(f), len(p)], np.int32).tobytes())
            for a, dt in ((v, np.float32), (f, np.int32), (p, np.float32), (nrm[0], np.float32), (nrm[1], np.float32), (nrm[2], np.float32),
                          (o["dist2"], np.float32), (o["face"], np.int32), (o["bary"], np.float32), (o["feature"], np.int32), (sg, np.float32)):
                fh.write(np.ascontiguousarray(a, dt).tobytes())


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    export_host_walk(sys.argv[1])
