"""numpy restatement of ``include/ag_inverse_skinning.h``: the Sobel gradient volume, the initial guess and the damped Newton iteration,
each ONE code run in float64 (the contract) and in float32.  numpy rounds every array operation on its own and has no FMA, so the
float32 run performs the header's operations in the header's order, lane sums and their tree included.  ``root_find`` returns the grid
node of every iteration beside the points: two runs can only be compared where they visited the same nodes (the weights are those of
the NEAREST node, so the iteration is discontinuous across cell boundaries).  Also the inputs of the tests.
"""
import numpy as np

GROUP = 16
STEP = np.float32(0.01)
SHAPES = [(9, 7, 5, 6), (16, 16, 16, 55)]
N_POINTS = 4099


def _f(dtype, x):
    return np.asarray(x).astype(dtype)


def gradient(volume, spacing, dtype=np.float64):
    """[X, Y, Z, J, 3]: the header's expression, in its order, in ``dtype``; ``spacing``: the three float32 node spacings."""
    v = _f(dtype, volume)
    X, Y, Z, J = v.shape
    P = np.pad(v, ((1, 1), (1, 1), (1, 1), (0, 0)))
    two = dtype(2)
    k = [dtype(1) / (dtype(32) * dtype(np.float32(h))) for h in spacing]

    def val(a, b, c):
        return P[a:a + X, b:b + Y, c:c + Z]

    t = [[(val(a, b, 0) + two * val(a, b, 1)) + val(a, b, 2) for b in range(3)] for a in range(3)]
    q = [[val(a, b, 2) - val(a, b, 0) for b in range(3)] for a in range(3)]
    s = [(t[a][0] + two * t[a][1]) + t[a][2] for a in range(3)]
    e = [t[a][2] - t[a][0] for a in range(3)]
    r = [(q[a][0] + two * q[a][1]) + q[a][2] for a in range(3)]
    out = np.stack([(s[2] - s[0]) * k[0], ((e[0] + two * e[1]) + e[2]) * k[1], ((r[0] + two * r[1]) + r[2]) * k[2]], -1)
    assert out.dtype == dtype
    return out


def sobel_plain(volume, spacing):
    """The reference's filter written out as a 27-term float64 sum (no separable shortcut): what ``gradient`` must equal."""
    v = np.asarray(volume, np.float64)
    X, Y, Z, J = v.shape
    P = np.pad(v, ((1, 1), (1, 1), (1, 1), (0, 0)))
    smooth = np.array([1.0, 2.0, 1.0])
    diff = np.array([-1.0, 0.0, 1.0])
    out = np.zeros((X, Y, Z, J, 3))
    for d in range(3):
        f = [smooth, smooth, smooth]
        f[d] = diff
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    out[..., d] += f[0][a] * f[1][b] * f[2][c] * P[a:a + X, b:b + Y, c:c + Z]
        out[..., d] /= 32.0 * float(np.float32(spacing[d]))
    return out


def _inverse3(m):
    """m[r][c] arrays -> inv[r][c]: d left to right, the adjugate, times one reciprocal."""
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = m
    d = m00 * m11 * m22 - m00 * m12 * m21 - m01 * m10 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20
    rd = d.dtype.type(1) / d
    return [[(m11 * m22 - m12 * m21) * rd, -(m01 * m22 - m02 * m21) * rd, (m01 * m12 - m02 * m11) * rd],
            [-(m10 * m22 - m12 * m20) * rd, (m00 * m22 - m02 * m20) * rd, -(m00 * m12 - m02 * m10) * rd],
            [(m10 * m21 - m11 * m20) * rd, -(m00 * m21 - m01 * m20) * rd, (m00 * m11 - m01 * m10) * rd]]


def init(points, weights, jnt_mats, normals=None, dtype=np.float64):
    """The header's initial guess: points [B, N, 3], weights [B, N, J], jnt_mats [B, J, 4, 4] -> points (and normals) in ``dtype``."""
    p, w, A = _f(dtype, points), _f(dtype, weights), _f(dtype, jnt_mats)
    B, N, J = w.shape
    with np.errstate(all="ignore"):
        m = [[np.zeros((B, N), dtype) for _ in range(4)] for _ in range(3)]
        for j in range(J):
            for r in range(3):
                for c in range(4):
                    m[r][c] = m[r][c] + w[:, :, j] * A[:, j, r, c][:, None]
        inv = _inverse3([row[:3] for row in m])
        out, out_n = [], []
        for r in range(3):
            s = -((inv[r][0] * m[0][3] + inv[r][1] * m[1][3]) + inv[r][2] * m[2][3])
            out.append(((inv[r][0] * p[..., 0] + inv[r][1] * p[..., 1]) + inv[r][2] * p[..., 2]) + s)
            if normals is not None:
                n = _f(dtype, normals)
                out_n.append((inv[r][0] * n[..., 0] + inv[r][1] * n[..., 1]) + inv[r][2] * n[..., 2])
    out = np.stack(out, -1)
    assert out.dtype == dtype
    return out if normals is None else (out, np.stack(out_n, -1))


def round_half_away(x):
    """roundf for x >= 0, without forming x + 0.5 (which rounds): the integer part plus one where the exact remainder reaches a half."""
    r = np.trunc(x)
    return r + ((x - r) >= x.dtype.type(0.5))


def nodes_of(xc, bounds, res, dtype):
    lo, hi = _f(dtype, bounds[0]), _f(dtype, bounds[1])
    out = []
    with np.errstate(all="ignore"):
        for d in range(3):
            u = (xc[..., d] - lo[d]) / (hi[d] - lo[d])
            u = np.fmax(np.fmin(u, dtype(1)), dtype(0))
            out.append(round_half_away(dtype(res[d] - 1) * u).astype(np.int64))
    return np.stack(out, -1)


def root_find(volume, bounds, spacing, xt, xc_init, jnt_mats, active=None, lam=0.1, iterations=10, dtype=np.float64, grad=None):
    """-> (xc [B, N, 3] in ``dtype``, nodes [iterations, B, N, 3] int64).  ``grad``: a gradient volume to read instead of ``gradient``'s."""
    vol = _f(dtype, volume)
    X, Y, Z, J = vol.shape
    G = gradient(volume, spacing, dtype) if grad is None else _f(dtype, grad)
    xt_, A = _f(dtype, xt), _f(dtype, jnt_mats)
    xc = _f(dtype, xc_init).copy()
    B, N, _ = xc.shape
    lam = dtype(np.float32(lam))
    step = dtype(STEP)
    act = np.ones((B, N), bool) if active is None else np.asarray(active, bool)
    visited = np.zeros((iterations, B, N, 3), np.int64)
    with np.errstate(all="ignore"):
        for it in range(iterations):
            node = nodes_of(xc, bounds, (X, Y, Z), dtype)
            visited[it] = node
            new = xc.copy()
            for b in range(B):
                nb = node[b]
                W = vol[nb[:, 0], nb[:, 1], nb[:, 2]]                    # [N, J]
                Gn = G[nb[:, 0], nb[:, 1], nb[:, 2]]                     # [N, J, 3]
                x = xc[b]
                part = np.zeros((GROUP, N, 24), dtype)                   # lane sums: m 12, j2 9, f 3
                for j in range(J):
                    ln = part[j % GROUP]
                    w = W[:, j]
                    for r in range(3):
                        for c in range(4):
                            ln[:, 4 * r + c] = ln[:, 4 * r + c] + w * A[b, j, r, c]
                        s = ((A[b, j, r, 0] * x[:, 0] + A[b, j, r, 1] * x[:, 1]) + A[b, j, r, 2] * x[:, 2]) + A[b, j, r, 3]
                        for c in range(3):
                            ln[:, 12 + 3 * r + c] = ln[:, 12 + 3 * r + c] + s * Gn[:, j, c]
                        ln[:, 21 + r] = ln[:, 21 + r] + w * s
                part = part[:8] + part[8:]
                part = part[:4] + part[4:]
                part = part[:2] + part[2:]
                acc = part[0] + part[1]
                jac = [[acc[:, 4 * r + c] + acc[:, 12 + 3 * r + c] * lam for c in range(3)] for r in range(3)]
                inv = _inverse3(jac)
                delta = [acc[:, 21 + r] - xt_[b, :, r] for r in range(3)]
                for r in range(3):
                    up = (inv[r][0] * delta[0] + inv[r][1] * delta[1]) + inv[r][2] * delta[2]
                    up = np.fmax(np.fmin(up, step), -step)
                    new[b, :, r] = x[:, r] - up
            xc = np.where(act[..., None], new, xc)
    assert xc.dtype == dtype
    return xc, visited


def forward_nearest(volume, bounds, xc, jnt_mats):
    """The solver's own forward map in float64: sum_j w_j(node(xc)) (A_j xc), [B, N, 3]."""
    vol, A, x = np.asarray(volume, np.float64), np.asarray(jnt_mats, np.float64), np.asarray(xc, np.float64)
    node = nodes_of(x, bounds, vol.shape[:3], np.float64)
    W = vol[node[..., 0], node[..., 1], node[..., 2]]                    # [B, N, J]
    M = np.einsum("bnj,bjrc->bnrc", W, A[:, :, :3, :])
    return np.einsum("bnrc,bnc->bnr", M[..., :3], x) + M[..., 3]


def kept(nodes_a, nodes_b):
    """[B, N] bool: the two runs visited the same node at every iteration."""
    return (nodes_a == nodes_b).all((0, 3)) if nodes_a.shape[0] else np.ones(nodes_a.shape[1:3], bool)


def bar(o32, o64, floor_scale):
    """The bar of the tests: 4 x the worst |float32 oracle - float64 oracle| plus 2^-22 x ``floor_scale``."""
    own = float(np.abs(np.asarray(o32, np.float64) - o64).max()) if np.size(o64) else 0.0
    return 4.0 * own + 2.0 ** -22 * float(floor_scale), own


# ------------------------------------------------------------------- inputs -------------------------------------------------------------------
def rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def joint_matrices(rng, B, J, centres, max_angle=0.5):
    """[B, J, 4, 4] float32: joint j turns by up to ``max_angle`` rad about its centre and moves by up to 2 cm."""
    A = np.zeros((B, J, 4, 4))
    for b in range(B):
        for j in range(J):
            R = rotation(rng.normal(0, 1, 3), rng.uniform(-max_angle, max_angle))
            A[b, j, :3, :3] = R
            A[b, j, :3, 3] = centres[j] - R @ centres[j] + rng.uniform(-0.02, 0.02, 3)
            A[b, j, 3, 3] = 1
    return A.astype(np.float32)


def smooth_case(shape, n=N_POINTS, B=1, offset=0.02, seed=0):
    """A smooth volume (softmax of the distance to J joint centres, rounded to multiples of 2^-16), joint rotations up to 0.5 rad, and
    ``n`` points per batch whose posed positions have a root of the solver's own equation: xt = forward_nearest(x_true), float32; the
    initial guess is x_true moved by up to ``offset`` per axis.  All float32; ``spacing`` is (hi - lo) / (R - 1) in float32."""
    X, Y, Z, J = shape
    rng = np.random.RandomState(1000 * seed + 7 * J + X)
    lo, hi = np.array([-0.8, -1.1, -0.45], np.float32), np.array([0.75, 0.9, 0.5], np.float32)
    bounds = np.stack([lo, hi], 0)
    spacing = ((hi - lo) / np.array([X - 1, Y - 1, Z - 1], np.float32)).astype(np.float32)
    centres = rng.uniform(lo * 0.8, hi * 0.8, (J, 3))
    axes = [np.linspace(lo[d], hi[d], shape[d]) for d in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1)
    dist = np.sqrt(((g[..., None, :] - centres) ** 2).sum(-1))
    logits = -dist / 0.25
    w = np.exp(logits - logits.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    volume = (np.round(w * 65536.0) / 65536.0).astype(np.float32)
    mats = joint_matrices(rng, B, J, centres)
    x_true = rng.uniform(lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo), (B, n, 3)).astype(np.float32)
    xt = forward_nearest(volume, bounds, x_true, mats).astype(np.float32)
    xc_init = (x_true + rng.uniform(-offset, offset, (B, n, 3))).astype(np.float32)
    return {"volume": volume, "bounds": bounds, "spacing": spacing, "jnt_mats": mats, "xt": xt, "xc_init": xc_init, "x_true": x_true}


def random_volume(shape, seed=3):
    """Uniform-random weights: for the gradient, and for ONE iteration only (ten on such a volume wander between cells)."""
    return np.random.RandomState(seed + shape[3]).uniform(0, 1, shape).astype(np.float32)


def exact_grid_case(shape, seed=2):
    """lo = 0 and hi = R - 1, so that (R - 1) u is the coordinate itself wherever the division is exact: points on nodes, on exact
    half-way coordinates (which round away from zero: up), and outside the bounds at both ends (clamped).  Returns the case and the
    nodes every point must choose."""
    X, Y, Z, J = shape
    rng = np.random.RandomState(seed)
    res = np.array([X, Y, Z])
    bounds = np.stack([np.zeros(3), res - 1.0], 0).astype(np.float32)
    spacing = np.ones(3, np.float32)
    n = 256
    base = np.stack([rng.randint(0, r, n) for r in res], -1).astype(np.float64)
    kind = rng.randint(0, 4, (n, 3))
    pts = base + np.where(kind == 1, 0.5, 0.0)
    pts = np.where(kind == 2, -1.75, pts)
    pts = np.where(kind == 3, res + 2.25, pts)
    want = np.where(kind == 1, np.minimum(base + 1, res - 1), base)
    want = np.where(kind == 2, 0, want)
    want = np.where(kind == 3, res - 1, want).astype(np.int64)
    # the division by R - 1 must be exact for a half to stay a half: keep the points whose u * (R - 1) reproduces the coordinate
    u = np.clip(pts.astype(np.float32) / (res - 1).astype(np.float32), 0, 1).astype(np.float32)
    back = (res - 1).astype(np.float32) * u
    ok = ((back == np.clip(pts, 0, res - 1)) | (kind != 1)).all(-1)
    pts, want = pts[ok], want[ok]
    volume = random_volume(shape, seed)
    mats = joint_matrices(rng, 1, J, rng.uniform(0, 1, (J, 3)) * (res - 1), max_angle=0.3)
    xc_init = pts[None].astype(np.float32)
    xt = (xc_init + rng.uniform(-0.3, 0.3, xc_init.shape)).astype(np.float32)
    return {"volume": volume, "bounds": bounds, "spacing": spacing, "jnt_mats": mats, "xt": xt, "xc_init": xc_init}, want[None]


def round_trip_inputs(seed=4):
    """The small closed mesh of ``mesh_query_oracle.lattice_mesh(8, 10)`` with its smooth 4-sparse weights over J = 55 joints and joint
    matrices that turn by up to 0.2 rad about centres strung along the mesh's y axis: (vertices [V, 3], faces [F, 3], weights [V, 55],
    jnt_mats [1, 55, 4, 4]), float32 / int32."""
    import mesh_query_oracle as mqo
    rng = np.random.RandomState(seed)
    v, f = mqo.lattice_mesh(8, 10)
    w = mqo.sparse_weights(v, 55)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    centres = np.tile(0.5 * (lo + hi), (55, 1))
    centres[:, 1] = np.linspace(lo[1], hi[1], 55)
    return v, f, w, joint_matrices(rng, 1, 55, centres, max_angle=0.2)


def points_near_nodes(node_xyz, distance, spacing, band=0.06, n=600, jitter=0.1, seed=4):
    """``n`` of the grid nodes closer than ``band`` to the surface, each moved by up to ``jitter`` of a cell per axis: [1, n, 3] float32.
    A point that starts near a node stays in that node's cell through the whole iteration, where the solver's equation is ONE affine
    map; from cell to cell the equation itself changes (nearest-node weights), and with it the residual."""
    rng = np.random.RandomState(seed)
    near = np.where(np.asarray(distance).reshape(-1) < band)[0]
    pick = near[rng.permutation(len(near))[:n]]
    pts = np.asarray(node_xyz, np.float64).reshape(-1, 3)[pick] + rng.uniform(-jitter, jitter, (len(pick), 3)) * np.asarray(spacing, np.float64)
    return pts[None].astype(np.float32)


HOST_WALK_CASES = [((9, 7, 5, 6), 257, 2, 10), ((16, 16, 16, 55), 130, 1, 10), ((5, 4, 3, 1), 65, 1, 3), ((4, 3, 5, 17), 33, 2, 1)]


def export_host_walk(path):
    """The cases of profiles/ub/inverse_skinning_host_walk.hip.  Per case: dims [X, Y, Z, J, B, N, iterations] int32, lambda float32,
    bounds [2, 3], spacing [3], volume, jnt_mats [B, J, 4, 4], xt, xc_init [B, N, 3], active [B, N] uint8, weights [B, N, J], normals
    [B, N, 3] float32; then the float32 oracle's gradient [X, Y, Z, J, 3], root_find [B, N, 3], init points and normals [B, N, 3]."""
    with open(path, "wb") as fh:
        fh.write(np.int32(len(HOST_WALK_CASES)).tobytes())
        for k, (shape, n, B, iterations) in enumerate(HOST_WALK_CASES):
            c = smooth_case(shape, n=n, B=B, offset=0.05, seed=k)
            if shape[3] == 17:
                c["volume"] = random_volume(shape)
            rng = np.random.RandomState(40 + k)
            active = (rng.uniform(0, 1, (B, n)) < 0.8).astype(np.uint8)
            weights = rng.uniform(0, 1, (B, n, shape[3])).astype(np.float32) ** 4
            weights = (weights / weights.sum(-1, keepdims=True)).astype(np.float32)
            normals = rng.normal(0, 1, (B, n, 3)).astype(np.float32)
            lam = np.float32(0.1)
            g = gradient(c["volume"], c["spacing"], np.float32)
            xc, _ = root_find(c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], c["jnt_mats"], active, lam, iterations, np.float32)
            ip, inn = init(c["xt"], weights, c["jnt_mats"], normals, np.float32)
            fh.write(np.int32(list(shape) + [B, n, iterations]).tobytes())
            for a in (lam, c["bounds"], c["spacing"], c["volume"], c["jnt_mats"], c["xt"], c["xc_init"], active, weights, normals, g, xc, ip, inn):
                fh.write(np.ascontiguousarray(a).tobytes())


if __name__ == "__main__":
    import sys
    export_host_walk(sys.argv[1])
