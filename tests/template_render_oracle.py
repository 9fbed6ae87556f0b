"""Host restatement of the template renderer's three definitions (``include/ag_ray_march.h``, ``template_render.py``) and small
deterministic scenes for them.

* near / far: the header's formulas in float32 operation by operation (numpy has no FMA: every ``*``, ``+``, ``-``, ``/`` and ``sqrt`` is one
  rounded float32 operation, sums left to right) and in float64.  Minimum and maximum are exact, so the float32 version is what the
  kernel must give bit for bit.
* sampling: ``nerf_util.sample_pts_on_rays`` in float32 operation by operation, with the random numbers handed in.
* compositing: ``template.py:345-346, 372-374`` + ``nerf_util.raw2outputs`` as the reference writes them (``torch.cumprod``,
  ``torch.sum``), in float32 and float64.

Scene builders use ``numpy.random.RandomState`` only.  Nothing here touches a GPU.
"""
import numpy as np
import torch

F32 = np.float32
BETA = 0.0101                       # LaplaceDensity's b of the reference configuration: |0.01| + 1e-4


# ---- near / far ---------------------------------------------------------------------------------------------------------------------------
def _ball_terms(vertices, ray_o, ray_d, radius, dtype):
    v, o, d = (np.asarray(x, F32).astype(dtype) for x in (vertices, ray_o, ray_d))
    radius = dtype(F32(radius))
    two, four = dtype(2), dtype(4)
    d0, d1, d2 = (d[:, None, k] for k in range(3))
    x0, x1, x2 = (o[:, None, k] - v[None, :, k] for k in range(3))
    a = d0 * d0 + d1 * d1 + d2 * d2                                          # [R, 1]
    b = two * (d0 * x0 + d1 * x1 + d2 * x2)                                  # [R, V]
    c = x0 * x0 + x1 * x1 + x2 * x2 - radius * radius
    disc = b * b - four * a * c
    assert a.dtype == dtype and disc.dtype == dtype
    return a, b, disc


def near_far(vertices, ray_o, ray_d, radius=0.1, fallback=None, dtype=F32, rows=4096):
    """``near [R], far [R], hit [R] (bool), disc [R, V]`` in ``dtype`` (``np.float32``: operation by operation; ``np.float64``)."""
    R = len(ray_o)
    near, far, hit = np.zeros(R, dtype), np.zeros(R, dtype), np.zeros(R, bool)
    disc_all = np.empty((R, len(vertices)), dtype)
    for r0 in range(0, R, rows):
        sl = slice(r0, min(R, r0 + rows))
        a, b, disc = _ball_terms(vertices, ray_o[sl], ray_d[sl], radius, dtype)
        ok = ~(disc.astype(np.float64) < 1e-8)
        with np.errstate(invalid="ignore", divide="ignore"):
            root = np.sqrt(np.where(ok, disc, dtype(0)))
            nv = (-b - root) / (dtype(2) * a)
            fv = (-b + root) / (dtype(2) * a)
        assert nv.dtype == dtype
        hit[sl] = ok.any(1)
        near[sl] = np.where(ok, nv, dtype(np.inf)).min(1)
        far[sl] = np.where(ok, fv, dtype(-np.inf)).max(1)
        disc_all[sl] = disc
    miss = ~hit
    near[miss] = 0 if fallback is None else np.asarray(fallback[0], F32).astype(dtype)[miss]
    far[miss] = 0 if fallback is None else np.asarray(fallback[1], F32).astype(dtype)[miss]
    return near, far, hit, disc_all


def sphere_points(n, radius=0.5, seed=0, centre=(0.0, 0.0, 0.0)):
    """``n`` points on a sphere: the stand-in for the posed body's vertices."""
    p = np.random.RandomState(seed).normal(size=(n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * radius + np.asarray(centre)).astype(F32)


def pinhole_rays(n, eye=(0.15, -0.1, -2.5), target=(0.0, 0.0, 0.0), half_width=0.35, normalise=True):
    """``n x n`` rays of a pinhole camera at ``eye`` looking at ``target``: ``(ray_o [n*n, 3], ray_d [n*n, 3])`` float32, row-major pixels."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    g = (np.arange(n) + 0.5) / n * 2 - 1
    xx, yy = np.meshgrid(g * half_width, g * half_width)
    d = fwd[None] + xx.reshape(-1, 1) * right[None] + yy.reshape(-1, 1) * up[None]
    if normalise:
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(eye[None], n * n, 0).astype(F32), d.astype(F32)


KINDS = ("camera", "camera", "camera", "miss", "inside", "behind", "graze_hit", "graze_miss")


def near_far_scene(V, R, seed=0, radius=0.1):
    """``vertices [V, 3], ray_o [R, 3], ray_d [R, 3], fallback (near [R], far [R])``.  Ray r is of kind ``KINDS[r % 8]``: a camera ray
    towards the cloud (directions not normalised); a ray that points away from it; an origin inside a vertex's ball; an origin past
    the cloud, looking away from vertex k (every ball it meets is behind it); and two rays that graze one vertex's ball with its float32 ``disc`` just at or above /
    just below the 1e-8 of the comparison (searched over origin offsets of a few 1e-7 for one whose float64 ``disc`` is on the same side)."""
    rs = np.random.RandomState(seed)
    vertices = sphere_points(V, 0.5, seed + 1)
    o = np.zeros((R, 3), np.float64)
    d = np.zeros((R, 3), np.float64)
    eye = np.array([0.15, -0.1, -2.5])
    for r in range(R):
        kind = KINDS[r % 8]
        k = (r // 8) % V
        c = vertices[k].astype(np.float64)
        aim = rs.normal(0, 0.35, 3)
        if kind == "camera":
            o[r], d[r] = eye, (aim - eye) * rs.uniform(0.5, 2.0)
        elif kind == "miss":
            o[r], d[r] = eye, eye - aim
        elif kind == "inside":
            o[r], d[r] = c + rs.normal(0, 0.02, 3), rs.normal(size=3)
        elif kind == "behind":
            o[r], d[r] = -eye, -eye - (c + rs.normal(0, 0.03, 3))                 # away from vertex k: its ball is behind the origin
        else:
            dd = rs.normal(size=3)
            dd /= np.linalg.norm(dd)
            n = np.cross(dd, rs.normal(size=3))
            n /= np.linalg.norm(n)
            want_hit = kind == "graze_hit"
            cand = c[None] + (radius * (1 + np.arange(-40, 41) * 3e-7))[:, None] * n[None] - 0.3 * dd[None]
            pair = (vertices[k:k + 1], cand.astype(F32), np.repeat(dd[None], len(cand), 0).astype(F32), radius)
            disc, disc64 = _ball_terms(*pair, F32)[2][:, 0].astype(np.float64), _ball_terms(*pair, np.float64)[2][:, 0]
            good = ((disc >= 1e-8) & (disc < 1e-5)) if want_hit else ((disc < 1e-8) & (disc > -1e-5))
            good &= (disc64 >= 1e-8) == want_hit                                  # the side is the same in exact arithmetic
            j = int(np.flatnonzero(good)[0]) if good.any() else 40
            o[r], d[r] = cand[j], dd
    fallback = (rs.uniform(1.0, 2.0, R).astype(F32), rs.uniform(3.0, 4.0, R).astype(F32))
    return vertices, o.astype(F32), d.astype(F32), fallback


def near_far_census(near, far, hit, disc):
    """How many rays / pairs of each kind the float32 oracle sees: misses, negative near, both negative, grazing pairs on either side."""
    tiny = np.abs(disc.astype(np.float64)) < 1e-5
    return dict(miss=int((~hit).sum()), hit=int(hit.sum()), negative_near=int((hit & (near < 0) & (far > 0)).sum()),
                behind=int((hit & (far < 0)).sum()), graze_hit=int((tiny & (disc.astype(np.float64) >= 1e-8)).sum()),
                graze_miss=int((tiny & (disc.astype(np.float64) < 1e-8)).sum()))


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------
def t_vals(S):
    return torch.linspace(0.0, 1.0, steps=S).numpy()


def sample(ray_o, ray_d, near, far, S, u=None, mask=None):
    """``z_vals [R, S], pts [R, S, 3]`` in float32, operation by operation (``nerf_util.py:102-131``)."""
    o, d, near, far = (np.asarray(x, F32) for x in (ray_o, ray_d, near, far))
    t = t_vals(S)
    assert t.dtype == F32
    z = near[:, None] * (F32(1) - t)[None] + far[:, None] * t[None]
    if u is not None:
        m = np.ones(len(o), bool) if mask is None else np.asarray(mask, bool)
        mids = F32(0.5) * (z[:, 1:] + z[:, :-1])
        upper = np.concatenate([mids, z[:, -1:]], 1)
        lower = np.concatenate([z[:, :1], mids], 1)
        z = np.where(m[:, None], lower + (upper - lower) * np.asarray(u, F32), z)
    pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
    assert z.dtype == F32 and pts.dtype == F32
    return z, pts


def viewdirs64(ray_d):
    d = np.asarray(ray_d, F32).astype(np.float64)
    return d / np.sqrt((d * d).sum(1, keepdims=True))


def ray_scene(R, seed=0):
    """``ray_o, ray_d [R, 3], near, far [R]``: camera rays at the unit scene with an interval around it; a few rays not normalised."""
    rs = np.random.RandomState(seed)
    n = int(np.ceil(np.sqrt(R)))
    o, d = pinhole_rays(n)
    o, d = o[:R].copy(), d[:R].copy()
    d[::5] *= rs.uniform(0.5, 2.0, (len(d[::5]), 1)).astype(F32)
    near = (2.5 - rs.uniform(0.6, 1.0, R)).astype(F32)
    far = (2.5 + rs.uniform(0.6, 1.0, R)).astype(F32)
    return o, d, near, far


# ---- compositing ------------------------------------------------------------------------------------------------------------------------
def composite(density, color, z_vals, white_bkgd=False, dtype=torch.float64):
    """The reference's integration of the inputs as given (float32 for a kernel's inputs, float64 inside a float64 chain), computed in
    ``dtype``: dict of numpy arrays ``rgb_map [R, 3], acc_map, depth_map,
    disp_map [R], weights [R, S]`` and ``alpha [R, S]``."""
    R, S = np.shape(z_vals)
    dn = torch.from_numpy(np.ascontiguousarray(density).reshape(R, S, 1)).to(dtype)
    rgb = torch.from_numpy(np.ascontiguousarray(color).reshape(R, S, 3)).to(dtype)
    z = torch.from_numpy(np.ascontiguousarray(z_vals)).to(dtype)
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, dists[..., -1:]], -1)
    alpha = (1. - torch.exp(-dn * dists[..., None]))[..., 0]
    weights = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1. - alpha + 1e-10], -1), -1)[..., :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z, -1)
    disp_map = 1. / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / torch.sum(weights, -1))
    acc_map = torch.sum(weights, -1)
    if white_bkgd:
        rgb_map = rgb_map + (1. - acc_map[..., None])
    return {k: v.numpy() for k, v in dict(rgb_map=rgb_map, acc_map=acc_map, depth_map=depth_map, disp_map=disp_map, weights=weights, alpha=alpha).items()}


def laplace_density(raw, b=BETA):
    """``LaplaceDensity`` of the raw network output (negative inside), float64."""
    raw = np.asarray(raw, np.float64)
    return (1.0 / b) * (0.5 + 0.5 * np.sign(raw) * np.expm1(-np.abs(raw) / b))


def composite_case(R, S, seed=0):
    """``density [R, S], color [R, S, 3], z_vals [R, S]`` float32: rays of ``pinhole_rays`` through a sphere of radius 0.5 (they enter and
    leave its surface, or pass beside it), Laplace densities (b = 0.0101) of its signed distance, a smooth colour, jittered samples.
    Ray 0 goes through the centre; every third ray has an interval of 0.25 S, whose steps are long enough inside the sphere for
    alpha = 1 exactly in float32 (density * dist > 17.4)."""
    rs = np.random.RandomState(seed)
    n = max(2, int(np.ceil(np.sqrt(R))))
    o, d = pinhole_rays(n, eye=(0.0, 0.0, -2.5), half_width=0.3)
    order = np.argsort(np.abs(d[:, :2]).sum(1), kind="stable")                 # ray 0: the one nearest to the axis; the last ones pass beside
    pick = np.round(np.linspace(0, len(order) - 1, R)).astype(int) if R > 1 else np.array([0])
    o, d = o[order[pick]].astype(np.float64), d[order[pick]].astype(np.float64)
    o[0], d[0] = (0.0, 0.0, -2.5), (0.0, 0.0, 1.0)
    near = np.full(R, 1.7)
    far = np.where(np.arange(R) % 3 == 2, 1.7 + max(1.6, 0.25 * S), 3.3)
    t = (np.arange(S)[None] + 0.8 * rs.uniform(0, 1, (R, S))) / S
    z = near[:, None] + (far - near)[:, None] * t
    p = o[:, None] + d[:, None] * z[..., None]
    raw = np.linalg.norm(p, axis=-1) - 0.5
    color = 0.5 + 0.5 * np.sin(3.0 * p + np.array([0.0, 1.0, 2.0]))
    return laplace_density(raw).astype(F32), color.astype(F32), z.astype(F32)
