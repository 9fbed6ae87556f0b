"""numpy restatement of ``include/ag_weight_diffuse.h``: the 7-point operator as a matrix-free function, the same operator as a dense
matrix with a direct solve on the free nodes (the answer every solver is measured against; fine up to about 2 000 nodes), the lockstep
conjugate gradients restated for a given dtype, and the cases of the tests.

``apply(..., dtype)`` and ``cg(..., dtype)`` run ONE code in float64 (the contract) and in float32: numpy rounds every array operation
on its own and has no FMA, so the float32 run of ``apply`` performs the header's operations in the header's order.  The sums of
``cg`` are numpy's (pairwise), not the kernel's: conjugate gradients correct themselves and the tests bound the solution, not the
trajectory.
"""
import numpy as np

TOL = 1e-5
SHAPES = [(9, 12, 14, 5), (12, 12, 12, 55), (2, 7, 33, 1), (5, 4, 3, 65)]
SPACINGS = {(9, 12, 14, 5): (0.031, 0.02, 0.0173), (12, 12, 12, 55): (0.02, 0.02, 0.02), (2, 7, 33, 1): (0.05, 0.04, 0.01),
            (5, 4, 3, 65): (0.01, 0.013, 0.021)}


def weights(spacing):
    """w_k = (h_min / h_k)^2, rounded to the float32 the device is handed."""
    h = np.asarray(spacing, np.float64)
    return ((h.min() / h) ** 2).astype(np.float32)


def _shift(u, axis, step):
    """u at the neighbour `step` along `axis`; at the grid's face the node itself (its difference is an exact zero: dropped)."""
    n = u.shape[axis]
    idx = np.clip(np.arange(n) + step, 0, n - 1)
    return np.take(u, idx, axis=axis)


def apply(u, fixed, w, dtype=np.float64):
    """(A u) [X, Y, Z, J]: d_k = (u - u_lower) + (u - u_upper), ((w_x d_x + w_y d_y) + w_z d_z), 0 on fixed nodes."""
    u = np.asarray(u).astype(dtype)
    w = np.asarray(w).astype(dtype)
    d = [(u - _shift(u, k, -1)) + (u - _shift(u, k, +1)) for k in range(3)]
    out = (w[0] * d[0] + w[1] * d[1]) + w[2] * d[2]
    return np.where(np.asarray(fixed, bool)[..., None], dtype(0), out).astype(dtype)


def dense_matrix(shape, w):
    """The operator over ALL nodes (no node fixed) as a dense float64 [N, N] matrix: the graph Laplacian of the grid with edge
    weights w_k.  Row n restricted to the free columns is A_ff, to the fixed columns A_fc."""
    X, Y, Z = shape
    N = X * Y * Z
    idx = np.arange(N).reshape(X, Y, Z)
    A = np.zeros((N, N))
    w = np.asarray(w, np.float64)
    for k in range(3):
        lo = np.take(idx, np.arange(shape[k] - 1), axis=k).reshape(-1)
        hi = np.take(idx, np.arange(1, shape[k]), axis=k).reshape(-1)
        A[lo, lo] += w[k]
        A[hi, hi] += w[k]
        A[lo, hi] -= w[k]
        A[hi, lo] -= w[k]
    return A


def free_matrix(fixed, w):
    """(A_ff [n_free, n_free], A_fc [n_free, n_fixed]) in float64."""
    fixed = np.asarray(fixed, bool)
    A = dense_matrix(fixed.shape, w)
    fr = ~fixed.reshape(-1)
    return A[np.ix_(fr, fr)], A[np.ix_(fr, ~fr)]


def direct_solve(target, fixed, w):
    """u [X, Y, Z, J] in float64: target on the fixed nodes, A_ff^-1 (-A_fc t) elsewhere, by LU."""
    fixed = np.asarray(fixed, bool)
    t = np.asarray(target, np.float64)
    J = t.shape[3]
    assert fixed.any() and fixed.size <= 2200, "the dense solve is for small grids"
    u = t.reshape(-1, J).copy()
    fr = ~fixed.reshape(-1)
    if fr.any():
        Aff, Afc = free_matrix(fixed, w)
        u[fr] = np.linalg.solve(Aff, -Afc @ u[~fr])
    return u.reshape(t.shape)


def cg(target, fixed, w, tol=TOL, max_iter=10000, dtype=np.float64):
    """The header's lockstep conjugate gradients in `dtype`: (u, iterations, rel_residual [J] of the recurrence)."""
    fixed = np.asarray(fixed, bool)
    t = np.asarray(target).astype(dtype)
    w = np.asarray(w).astype(dtype)
    zero = dtype(0)
    u0 = np.where(fixed[..., None], t, zero).astype(dtype)
    b = (zero - apply(u0, fixed, w, dtype)).astype(dtype)
    x = np.zeros_like(b)
    r, p = b.copy(), b.copy()
    axes = (0, 1, 2)
    bb = (b * b).sum(axes, dtype=dtype)
    rr = bb.copy()
    it = 0

    def safe_div(num, den):
        pos = den > 0
        return np.where(pos, num / np.where(pos, den, 1), zero).astype(dtype)

    limit = dtype(tol) * dtype(tol)
    while not (rr <= limit * bb).all() and it < max_iter:
        ap = apply(p, fixed, w, dtype)
        alpha = safe_div(rr, (p * ap).sum(axes, dtype=dtype))
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * ap).astype(dtype)
        rr_new = (r * r).sum(axes, dtype=dtype)
        beta = safe_div(rr_new, rr)
        p = (r + beta * p).astype(dtype)
        rr = rr_new
        it += 1
    u = np.where(fixed[..., None], t, x).astype(dtype)
    return u, it, rel(rr, bb)


def rel(num_sq, den_sq):
    num_sq, den_sq = np.asarray(num_sq, np.float64), np.asarray(den_sq, np.float64)
    pos = den_sq > 0
    return np.where(pos, np.sqrt(num_sq / np.where(pos, den_sq, 1)), np.sqrt(num_sq))


def true_rel_residual(u, target, fixed, w):
    """|A u|_j / |b_j| in float64 [J] (|A u|_j itself where b_j = 0): how far u is from satisfying the 7-point relation."""
    fixed = np.asarray(fixed, bool)
    u0 = np.where(fixed[..., None], np.asarray(target, np.float64), 0.0)
    b = apply(u0, fixed, w)
    r = apply(np.asarray(u, np.float64), fixed, w)
    return rel((r * r).sum((0, 1, 2)), (b * b).sum((0, 1, 2)))


def node_coordinates(shape, spacing):
    """[X, Y, Z, 3] float64, the grid centred on the origin."""
    axes = [(np.arange(n) - 0.5 * (n - 1)) * h for n, h in zip(shape[:3], spacing)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1)


def band_case(shape, spacing=None, seed=0):
    """(target [X, Y, Z, J] float32, fixed [X, Y, Z] bool, w float32 [3]) of a test: the nodes within 0.75 of the largest spacing of a
    sphere's surface (an analytic SDF band; the sphere's radius is 0.3 of the longest extent), plus two corners of the cube and a patch of one face; random non-negative values,
    with channel 0 all zero and channel 1 constant 1 on the fixed nodes where J >= 3."""
    shape = tuple(shape)
    spacing = SPACINGS[shape] if spacing is None else spacing
    X, Y, Z, J = shape
    rng = np.random.RandomState(100 * seed + J)
    g = node_coordinates(shape, spacing)
    radius = 0.3 * max((n - 1) * h for n, h in zip(shape[:3], spacing))
    sdf = np.sqrt((g ** 2).sum(-1)) - radius
    fixed = np.abs(sdf) <= 0.75 * max(spacing)
    fixed[0, 0, 0] = fixed[-1, -1, -1] = True
    fixed[0, Y // 3:Y // 3 + 2, Z // 2:Z // 2 + 3] = True
    target = rng.uniform(0, 1, shape).astype(np.float32)
    if J >= 3:
        target[..., 0] = 0
        target[..., 1] = 1
    assert fixed.any() and not fixed.all()
    return target, fixed, weights(spacing)


def two_lobe_case(shape=(11, 16, 9), J=2):
    """Two parallel capsules along x, at y = -/+ a quarter of the extent; the nodes within a radius of either axis are fixed and carry
    the nearest capsule's weights (1, 0) / (0, 1), which is what a nearest-surface volume stores EVERYWHERE: the target jumps across
    the mid-plane between them, which is free.  Returns (target, fixed, w)."""
    X, Y, Z = shape
    spacing = (0.02, 0.02, 0.02)
    g = node_coordinates(shape + (J,), spacing)
    ya = 0.25 * (Y - 1) * spacing[1]
    xs = np.clip(g[..., 0], -0.3 * (X - 1) * spacing[0], 0.3 * (X - 1) * spacing[0])
    d = [np.sqrt((g[..., 0] - xs) ** 2 + (g[..., 1] - s * ya) ** 2 + g[..., 2] ** 2) for s in (-1, 1)]
    fixed = np.minimum(d[0], d[1]) <= 0.05
    target = np.zeros(shape + (J,), np.float32)
    target[..., 0] = d[0] <= d[1]
    target[..., 1] = d[0] > d[1]
    assert Y % 2 == 0 and not fixed[:, Y // 2 - 1:Y // 2 + 1].any(), "the two layers either side of the mid-plane must be free"
    return target, fixed, weights(spacing)


def midplane_jump(u):
    """The largest difference between the two layers of nodes either side of the mid-plane y = 0."""
    Y = u.shape[1]
    return float(np.abs(np.asarray(u, np.float64)[:, Y // 2] - np.asarray(u, np.float64)[:, Y // 2 - 1]).max())


def clip_renormalise(u):
    """gen_weight_volume.py:131-132 in float64: clip to [0, 1], divide each row by its sum; a row that sums to 0 stays 0."""
    u = np.clip(np.asarray(u, np.float64), 0, 1)
    s = u.sum(-1, keepdims=True)
    return np.where(s > 0, u / np.where(s > 0, s, 1), 0.0)


def row_sum_bar(J):
    """|row sum - 1| of a float32 row of J non-negative quotients u_j / s, s the float32 sum of the u_j: in any order of summation s is
    off from the exact sum by at most (J - 1) 2^-24 of it, so the exact quotients sum to 1 within that; each rounded quotient is off
    by at most 2^-24 of itself, together 2^-24 of their sum.  (J + 1) 2^-24 with the second-order terms' share."""
    return (J + 1) * 2.0 ** -24


def probe_input(shape, seed=5):
    """A random float32 [X, Y, Z, J] for the operator alone: NOT zero on the fixed nodes (the operator reads neighbours as given)."""
    return np.random.RandomState(seed + shape[3]).normal(0, 1, shape).astype(np.float32)


HOST_WALK_SHAPES = SHAPES + [(3, 2, 70, 3), (2, 2, 130, 64)]


def export_host_walk(path):
    """The cases of profiles/ub/weight_diffuse_host_walk.hip: per case dims [X, Y, Z, J, float64 CG iterations] int32, w [3] float32,
    fixed [N] uint8, target [N, J] float32, probe [N, J] float32, float32 oracle's A probe [N, J] float32, direct solution [N, J]
    float64."""
    with open(path, "wb") as fh:
        fh.write(np.int32(len(HOST_WALK_SHAPES)).tobytes())
        for shape in HOST_WALK_SHAPES:
            spacing = SPACINGS.get(shape, (0.02, 0.03, 0.01))
            target, fixed, w = band_case(shape, spacing)
            probe = probe_input(shape)
            _, iterations, _ = cg(target, fixed, w)
            fh.write(np.int32(list(shape) + [iterations]).tobytes())
            for a in (w, fixed.astype(np.uint8), target, probe, apply(probe, fixed, w, np.float32), direct_solve(target, fixed, w)):
                fh.write(np.ascontiguousarray(a).tobytes())


if __name__ == "__main__":
    import sys
    export_host_walk(sys.argv[1])
