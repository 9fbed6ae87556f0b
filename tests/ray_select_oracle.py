"""Numpy restatement of the template stage's ray selection (``include/ag_ray_select.h``; the reference's ``utils/nerf_util.py``:
``get_bound_2d_mask``, ``get_rays``, ``get_near_far``, ``sample_randomly_for_nerf_rendering``, ``sample_patch_for_nerf_rendering`` and
the whole-image rays of ``dataset/dataset_pose.py``), written for two precisions:

* ``np.float32``: operation by operation as the header states them, one rounding per operation, sums left to right.  The kernels are
  compared with this bit for bit.
* ``np.float64``: the same sequence in double precision with the unrounded inverses: what the reference computes (its ``einsum`` /
  ``norm`` may sum in another order, which moves the last bits of a double).

The integer quad fill is the header's rule, this project's own definition of ``cv2.fillPoly`` on integer vertices (OpenCV was never run
beside it).  The random draws are never made here: every sampler takes ``picks``.  Scenes at the bottom.
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
QUADS = ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5))


# ---- the box's image-space mask ---------------------------------------------------------------------------------------------------------
def bound_corners(bounds):
    b = np.asarray(bounds, F64)
    return np.array([[b[(i >> 2) & 1, 0], b[(i >> 1) & 1, 1], b[i & 1, 2]] for i in range(8)], F64)


def project_corners(bounds, intr, extr):
    """The eight corners as ``project`` places them, float64, rounded half to even -> int64 [8, 2]; ``ValueError`` for a corner with
    camera-space z <= 0."""
    K, RT = np.asarray(intr, F64), np.asarray(extr, F64)
    xyz = bound_corners(bounds) @ RT[:3, :3].T + RT[:3, 3:].T
    if (xyz[:, 2] <= 0).any():
        raise ValueError("a corner of the box lies behind the camera (z <= 0)")
    xyz = xyz @ K[:3, :3].T
    return np.round(xyz[:, :2] / xyz[:, 2:]).astype(np.int64)


def quad_mask(quad, H, W):
    """The closed quad in either winding (bool [H, W]): all four int64 edge functions >= 0 or all <= 0, inside the quad's bounding box."""
    q = np.asarray(quad, np.int64).reshape(4, 2)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    ge, le = np.ones((H, W), bool), np.ones((H, W), bool)
    for i in range(4):
        (ax, ay), (bx, by) = q[i], q[(i + 1) % 4]
        e = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        ge &= e >= 0
        le &= e <= 0
    box = (x >= q[:, 0].min()) & (x <= q[:, 0].max()) & (y >= q[:, 1].min()) & (y <= q[:, 1].max())
    return (ge | le) & box


def bound_mask(bounds, intr, extr, H, W):
    c = project_corners(bounds, intr, extr)
    m = np.zeros((H, W), bool)
    for quad in QUADS:
        m |= quad_mask(c[list(quad)], H, W)
    return m


def classify(mask_img, bounds, extr, intr, unsample=None):
    """uint8 [H, W]: 0 outside the box's mask or inside the unsample region, 1 on the matte, 2 off it."""
    H, W = mask_img.shape
    bound = bound_mask(bounds, intr, extr, H, W)
    if unsample is not None:
        bound &= ~(np.asarray(unsample) != 0)
    return np.where(bound, np.where(np.asarray(mask_img) != 0, 1, 2), 0).astype(np.uint8)


def candidates(mask_img, bounds, extr, intr, unsample=None):
    cls = classify(mask_img, bounds, extr, intr, unsample).reshape(-1)
    return np.flatnonzero(cls == 1).astype(np.int32), np.flatnonzero(cls == 2).astype(np.int32), cls.reshape(mask_img.shape) != 0


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------
def camera(extr, intr, dt):
    """(inv(intr), inv(extr)[:3, :3], inv(extr)[:3, 3]) formed in float64 and rounded once to ``dt``."""
    ie, ii = np.linalg.inv(np.asarray(extr, F64)), np.linalg.inv(np.asarray(intr, F64))
    return ii.astype(dt), ie[:3, :3].astype(dt), ie[:3, 3].astype(dt)


def get_rays(uv, extr, intr, dt=F32):
    """``(ray_d [n, 3], ray_o [n, 3])`` of integer pixels ``uv`` [n, 2] = (x, y), WITHOUT + 0.5."""
    K, R, c = camera(extr, intr, dt)
    uv = np.asarray(uv).reshape(-1, 2)
    X, Y = uv[:, 0].astype(dt), uv[:, 1].astype(dt)
    p = [(K[i, 0] * X + K[i, 1] * Y) + K[i, 2] for i in range(3)]
    g = []
    for i in range(3):
        w = ((R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2]) + c[i]
        g.append(w - c[i])
    ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    den = ln + dt(1e-8)
    d = np.stack([g[i] / den for i in range(3)], -1).astype(dt)
    return d, np.broadcast_to(c, d.shape).copy()


def get_near_far(bounds, ray_o, ray_d, dt=F32):
    """``(near [n], far [n], hit [n])`` against the box padded by 0.01: near = far = 0 where ``hit`` is false (the reference returns the
    hit rays only: ``near[hit]``)."""
    b = np.asarray(bounds).astype(dt)
    lo, hi = b[0] - dt(0.01), b[1] + dt(0.01)
    o, d = np.asarray(ray_o, dt), np.asarray(ray_d, dt)
    n = o.shape[0]
    passed = np.zeros(n, np.int64)
    s = np.zeros((2, n), dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(6):
            a = j % 3
            plane = lo[a] if j < 3 else hi[a]
            t = (plane - o[:, a]) / (d[:, a] + dt(1e-9))
            q = [t * d[:, i] + o[:, i] for i in range(3)]
            ok = np.ones(n, bool)
            for i in range(3):
                ok &= (q[i] >= lo[i] - dt(1e-6)) & (q[i] <= hi[i] + dt(1e-6))
            e = [q[i] - o[:, i] for i in range(3)]
            dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            for m in range(2):
                take = ok & (passed == m)
                s[m][take] = dist[take]
            passed += ok
        hit = passed == 2
        nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        s0, s1 = s[0] / nrm, s[1] / nrm
    near = np.where(hit, np.minimum(s0, s1), dt(0)).astype(dt)
    far = np.where(hit, np.maximum(s0, s1), dt(0)).astype(dt)
    return near, far, hit


def build(pix, extr, intr, bounds, H, W, color=None, mask=None, depth=None, dt=F32):
    """Every output of the build kernel for the flat pixels ``pix`` (None: all, row-major)."""
    pix = np.arange(H * W, dtype=np.int64) if pix is None else np.asarray(pix, np.int64)
    uv = np.stack([pix % W, pix // W], -1).astype(np.int32)
    d, o = get_rays(uv, extr, intr, dt)
    near, far, hit = get_near_far(bounds, o, d, dt)
    out = dict(uv=uv, ray_o=o, ray_d=d, near=near, far=far, hit=hit)
    if color is not None:
        m = np.asarray(mask).reshape(-1)[pix] != 0
        dep = (np.asarray(depth, dt).reshape(-1)[pix] if depth is not None else np.zeros(len(pix), dt)).astype(dt)
        col = np.asarray(color, dt).reshape(-1, 3)[pix].copy()
        col[~m] = 0
        K = np.asarray(intr)
        fx, fy, cx, cy = dt(K[0, 0]), dt(K[1, 1]), dt(K[0, 2]), dt(K[1, 2])
        ex = ((uv[:, 0].astype(dt) + dt(0.5)) - cx) * dep / fx
        ey = ((uv[:, 1].astype(dt) + dt(0.5)) - cy) * dep / fy
        out.update(color_gt=col, mask_gt=m.astype(F32), depth_gt=dep, dist=np.sqrt((ex * ex + ey * ey) + dep * dep).astype(dt))
    return out


RAY_KEYS = ("ray_o", "ray_d", "near", "far")


def sample_randomly(color, mask, depth, extr, intr, bounds, sample_num, ratio, unsample, picks, dt=F32):
    """``sample_randomly_for_nerf_rendering`` with the draws of ``picks`` = [(inside indices, outside indices)] per round."""
    H, W = mask.shape
    inside, outside, _ = candidates(mask, bounds, extr, intr, unsample)
    kept, count, rnd = [], 0, 0
    while count < sample_num:
        rest = sample_num - count
        n_in = int(rest * ratio)
        ii, oi = (np.asarray(p, np.int64) for p in picks[rnd])
        assert len(ii) == n_in and len(oi) == rest - n_in, (rnd, len(ii), len(oi), n_in, rest - n_in)
        pix = np.concatenate([inside[ii], outside[oi]])
        b = build(pix, extr, intr, bounds, H, W, dt=dt)
        kept.append(pix[b["hit"]])
        count += int(b["hit"].sum())
        rnd += 1
    out = build(np.concatenate(kept), extr, intr, bounds, H, W, color, mask, depth, dt)
    assert out.pop("hit").all()
    out["rounds"] = rnd
    return out


def patch_origin(center, size, ps):
    return int(np.clip(center - ps // 2, 0, size - ps))


def sample_patches(color, mask, depth, extr, intr, bounds, patch_num, ps, unsample, picks, dt=F32):
    """``sample_patch_for_nerf_rendering`` (``resize_factor = 1``) with ``picks`` = [(use_inside, index)] per patch."""
    H, W = mask.shape
    inside, outside, bound = candidates(mask, bounds, extr, intr, unsample)
    pix = []
    for use_inside, index in picks[:patch_num]:
        c = int((inside if use_inside else outside)[index])
        u0, v0 = patch_origin(c % W, W, ps), patch_origin(c // W, H, ps)
        yy, xx = np.mgrid[v0:v0 + ps, u0:u0 + ps]
        pix.append((yy * W + xx).reshape(-1))
    pix = np.concatenate(pix)
    b = build(pix, extr, intr, bounds, H, W, color, mask, depth, dt)
    within = bound.reshape(-1)[pix] & b["hit"]
    out = {k: b[k] for k in ("uv", "color_gt", "mask_gt", "depth_gt")}
    out.update({k: b[k][within] for k in RAY_KEYS + ("dist",)})
    out["mask_within_patch"] = within
    return out


def image_rays(extr, intr, W, H, bounds, dt=F32):
    b = build(None, extr, intr, bounds, H, W, dt=dt)
    hit = b["hit"]
    out = {k: b[k][hit] for k in ("uv",) + RAY_KEYS}
    out["dist"] = np.zeros(int(hit.sum()), dt)
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
FRAMES = ((1, 1), (5, 3), (37, 70), (48, 64), (64, 65), (130, 257))          # (H, W)
BOX = np.array([[-0.45, -0.9, -0.3], [0.5, 0.95, 0.25]], F32)
CAMERAS = ("axis", "tilted", "close")
FOCAL = {"axis": 0.55, "tilted": 0.8, "close": 1.1, "cover": 1.1}             # in units of W; "cover": the box fills the frame (patch clipping)
MATTES = ("blob", "all_true", "all_false", "band")

# the cases of tests/golden/ray_select_ref.npz (tests/golden/make_golden_ray_select.py)
GOLDEN_RAY_FRAME = (37, 70)
# (camera, H, W, matte, sample_num, inside_ratio, force a second round)
GOLDEN_RANDOM_CASES = (("tilted", 37, 70, "blob", 128, 0.5, True), ("axis", 64, 65, "band", 96, 0.3, False), ("close", 48, 64, "blob", 64, 0.5, False))
# (camera, H, W, matte, patch_num, patch_size, inside_ratio)
GOLDEN_PATCH_CASES = (("tilted", 48, 64, "blob", 2, 8, 0.5), ("close", 37, 70, "band", 3, 16, 0.5))


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]]}[axis], F64)


def scene_camera(name, H, W):
    """``(extr [4, 4], intr [3, 3])`` float64: world -> camera, principal point (W / 2, H / 2)."""
    extr = np.eye(4)
    if name == "axis":
        extr[:3, 3] = [0.0, 0.0, 2.5]
    elif name == "cover":
        extr[:3, 3] = [0.0, 0.0, 1.0]
    elif name == "tilted":
        extr[:3, :3], extr[:3, 3] = _rot("x", 0.2) @ _rot("y", 0.4), [0.1, -0.05, 2.5]
    else:
        extr[:3, :3], extr[:3, 3] = _rot("y", 0.7), [0.3, 0.2, 1.4]
    f = FOCAL[name] * W
    return extr, np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], F64)


@functools.lru_cache(maxsize=None)
def scene_images(H, W, matte="blob"):
    """``(color float32 [H, W, 3], mask bool [H, W], depth float32 [H, W], unsample bool [H, W] or None)``; built once, read-only."""
    rs = np.random.RandomState(1000 * H + W)
    color = rs.uniform(0, 1, (H, W, 3)).astype(F32)
    depth = rs.uniform(1.5, 3.5, (H, W)).astype(F32)
    depth[rs.uniform(size=(H, W)) < 0.2] = 0                                    # no depth there: dist = 0
    if matte == "all_true":
        mask = np.ones((H, W), bool)
    elif matte == "all_false":
        mask = np.zeros((H, W), bool)
    else:
        y, x = np.mgrid[0:H, 0:W]
        field = np.zeros((H, W))
        for _ in range(4):
            cy, cx, r = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W, rs.uniform(0.15, 0.3) * max(H, W, 4)
            field += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (r * r))
        mask = field > 0.9
    unsample = None
    if matte == "band":
        unsample = np.zeros((H, W), bool)
        unsample[H // 3:max(H // 2, H // 3 + 1)] = True
    for a in (color, mask, depth) + (() if unsample is None else (unsample,)):
        a.setflags(write=False)
    return color, mask, depth, unsample


def missing_bound_pixels(name, H, W, dt=F64):
    """Flat pixels inside the box's mask whose ray does not hit the box (the mask is drawn from rounded corners; the box is padded by 1 cm)."""
    extr, intr = scene_camera(name, H, W)
    bound = bound_mask(BOX, intr, extr, H, W).reshape(-1)
    hit = build(None, extr, intr, BOX, H, W, dt=dt)["hit"]
    return np.flatnonzero(bound & ~hit)


def make_picks(name, H, W, matte, sample_num, ratio, seed, force=()):
    """Draws for ``sample_randomly``: per round ``RandomState.choice`` without replacement, as many rounds as the hits ask for.  The flat
    pixels of ``force`` are swapped into the first round's picks where they are candidates."""
    extr, intr = scene_camera(name, H, W)
    _, mask, _, unsample = scene_images(H, W, matte)
    inside, outside, _ = candidates(mask, BOX, extr, intr, unsample)
    rs = np.random.RandomState(seed)
    picks, count = [], 0
    while count < sample_num:
        rest = sample_num - count
        n_in = int(rest * ratio)
        ii, oi = rs.choice(len(inside), n_in, replace=False), rs.choice(len(outside), rest - n_in, replace=False)
        if not picks:
            for idx, cand in ((ii, inside), (oi, outside)):
                slot = 0
                for p in force:
                    where = np.flatnonzero(cand == p)
                    if len(where) and slot < len(idx):
                        if where[0] in idx:
                            continue
                        idx[slot] = where[0]
                        slot += 1
        picks.append((ii.astype(np.int64), oi.astype(np.int64)))
        pix = np.concatenate([inside[ii], outside[oi]])
        count += int(build(pix, extr, intr, BOX, H, W, dt=F64)["hit"].sum())
    return picks
