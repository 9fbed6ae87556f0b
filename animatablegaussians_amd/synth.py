"""Seeded synthetic inputs for the render hot path (no dataset or checkpoint can be fetched here).

Two scene families, both from ``numpy.random.RandomState(31359)`` (the reference's seed,
``main_avatar.py:817``; numpy's legacy generator is bit-stable across versions and machines):

* ``random_gaussians``  - BASELINE.json configs[0]: P random Gaussians in a body-sized box, one 512x512 front
  camera (f = 550, c = 256: the dataset default, ``dataset/dataset_mv_rgb.py:216-218``).
* ``avatar_map_gaussians`` - configs[1]/[4]: Gaussians laid out like the reference's canonical front|back position
  map (``gen_data/gen_pos_maps.py:42,61,112-113``): one Gaussian per set pixel of a (S x 2S) silhouette mask,
  S = 1024 -> ~234 k Gaussians on a 2 mm grid; free-view cameras at f = 1100, 1024x1024, subject 2.5 m away
  (``main_avatar.py:601-615``).
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np

from . import camera as cam

f32 = np.float32
SEED = 31359


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def random_gaussians(P: int = 10000, seed: int = SEED, img: int = 512, focal: float = 550.0) -> Dict[str, object]:
    rs = np.random.RandomState(seed)
    means3D = np.stack([rs.uniform(-0.5, 0.5, P), rs.uniform(-0.9, 0.9, P), rs.uniform(-0.2, 0.2, P)], 1).astype(f32)
    scales = np.exp(rs.normal(math.log(0.01), 0.3, (P, 3))).astype(f32)
    q = rs.normal(0, 1, (P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= rs.uniform(0.8, 1.2, (P, 1))          # deliberately NOT unit: the rasterizer uses raw quaternions
    rotations = q.astype(f32)
    opacities = _sigmoid(rs.normal(0, 1.5, (P, 1))).astype(f32)
    colors = rs.uniform(0, 1, (P, 3)).astype(f32)
    bg = rs.uniform(0, 1, 3).astype(f32)
    extr = cam.calc_front_mv(np.zeros(3, f32), tar_pos=(0.0, 0.0, 2.5))
    intr = np.array([[focal, 0, img / 2], [0, focal, img / 2], [0, 0, 1]], f32)
    scene = {
        "means3D": means3D, "scales": scales, "rotations": rotations, "opacities": opacities, "colors": colors,
        "bg": bg, "extr": extr, "intr": intr, "img_w": img, "img_h": img,
    }
    scene.update(upstream_grads(img, img, seed + 1))
    return scene


def upstream_grads(W: int, H: int, seed: int) -> Dict[str, np.ndarray]:
    rs = np.random.RandomState(seed)
    return {
        "dL_dcolor": rs.normal(0, 1, (3, H, W)).astype(f32),
        "dL_ddepth": rs.normal(0, 1, (1, H, W)).astype(f32),
        "dL_dalpha": rs.normal(0, 1, (1, H, W)).astype(f32),
    }


def body_mask(S: int = 1024) -> np.ndarray:
    """(S, S) bool silhouette: union of ellipses (head, torso, two arms in A-pose, two legs)."""
    v, u = np.mgrid[0:S, 0:S].astype(np.float64)
    x = (u + 0.5) / S * 2.0 - 1.0       # [-1, 1] across the map
    y = (v + 0.5) / S * 2.0 - 1.0       # top (-1) -> bottom (+1)

    def ell(cx, cy, rx, ry, ang=0.0):
        c, s = math.cos(ang), math.sin(ang)
        xr = (x - cx) * c + (y - cy) * s
        yr = -(x - cx) * s + (y - cy) * c
        return (xr / rx) ** 2 + (yr / ry) ** 2 <= 1.0

    m = ell(0.0, -0.78, 0.085, 0.11)                     # head
    m |= ell(0.0, -0.36, 0.17, 0.30)                     # torso
    m |= ell(-0.33, -0.36, 0.056, 0.30, math.radians(-38))   # arms
    m |= ell(0.33, -0.36, 0.056, 0.30, math.radians(38))
    m |= ell(-0.10, 0.42, 0.075, 0.46, math.radians(4))   # legs
    m |= ell(0.10, 0.42, 0.075, 0.46, math.radians(-4))
    return m


def avatar_map_gaussians(S: int = 1024, seed: int = SEED) -> Dict[str, object]:
    """Canonical Gaussians on an (S x 2S) front|back map.  Pixel pitch = 2.048 m / S."""
    rs = np.random.RandomState(seed)
    m = body_mask(S)
    mask = np.concatenate([m, m[:, ::-1]], axis=1)            # back half is the mirrored silhouette
    pitch = 2.048 / S
    vv, uu = np.nonzero(mask)                                  # row-major == the reference's boolean-mask order
    front = uu < S
    ul = np.where(front, uu, 2 * S - 1 - uu).astype(np.float64)
    x = (ul + 0.5 - S / 2) * pitch
    y = (S / 2 - (vv + 0.5)) * pitch
    bump = 0.10 * np.cos(np.clip(x / 0.45, -1, 1) * math.pi / 2)       # thickness profile
    z = np.where(front, bump, -bump)
    means3D = np.stack([x, y, z], 1).astype(f32)
    P = means3D.shape[0]
    base = math.log(pitch)                                     # ~mean 3-NN distance (create_from_pcd)
    scales = np.exp(base + rs.normal(0, 0.2, (P, 3))).astype(f32)
    q = rs.normal(0, 1, (P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rotations = q.astype(f32)
    opacities = _sigmoid(rs.normal(2.0, 1.0, (P, 1))).astype(f32)
    colors = rs.uniform(0, 1, (P, 3)).astype(f32)
    bg = np.array([1.0, 1.0, 1.0], f32)
    return {
        "mask": mask, "means3D": means3D, "scales": scales, "rotations": rotations,
        "opacities": opacities, "colors": colors, "bg": bg,
    }


def _lattice_surface(radius, centre, n_lat: int, n_lon: int):
    """Closed surface x = centre + radius(theta, phi) * direction on an n_lat x n_lon latitude / longitude lattice with two pole fans,
    wound counter-clockwise seen from outside.  -> (vertices [n_lat * n_lon + 2, 3] float64, faces [2 * n_lon * n_lat, 3] int64)."""
    theta = math.pi * (np.arange(n_lat) + 1.0) / (n_lat + 1.0)                # polar angle from +y, poles excluded
    phi = 2.0 * math.pi * np.arange(n_lon) / n_lon
    T, P = np.meshgrid(theta, phi, indexing="ij")
    T = np.concatenate([T.reshape(-1), [0.0, math.pi]])
    P = np.concatenate([P.reshape(-1), [0.0, 0.0]])
    d = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], 1)
    v = np.asarray(centre, np.float64) + radius(T, P)[:, None] * d
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    a, b = (i * n_lon + j).reshape(-1), (i * n_lon + (j + 1) % n_lon).reshape(-1)
    c, e = a + n_lon, b + n_lon                                                # the ring below
    jj = np.arange(n_lon)
    north, south = n_lat * n_lon, n_lat * n_lon + 1
    last = (n_lat - 1) * n_lon
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([b, e, c], 1),
                            np.stack([np.full(n_lon, north), (jj + 1) % n_lon, jj], 1),
                            np.stack([np.full(n_lon, south), last + jj, last + (jj + 1) % n_lon], 1)], 0)
    return v, faces.astype(np.int64)


def body_mesh(J: int = 55, second_component: bool = True) -> Dict[str, np.ndarray]:
    """A synthetic SURFACE of SMPL-X's size for the canonical-map path (``subject_maps.canonical_maps``): the random vertices and
    faces of ``smplx_model_arrays`` are a triangle soup, a stress input and no surface.

    First component: a closed, consistently wound (counter-clockwise from outside), star-shaped lobed surface -- an ellipsoid of
    half-axes (0.5, 0.9, 0.2) m whose radius is modulated by smooth lobes -- on a 145 x 72 latitude / longitude lattice with two
    pole fans: 10 442 vertices and 20 880 faces (SMPL-X: 10 475 and 20 908), inside the 2 m window of the canonical maps (1.19 x 1.8 m:
    wide enough that a face still projects to about a pixel on a 256^2 map).
    ``second_component``: a small closed sphere-like surface (110 vertices, 216 faces) that INTERSECTS the first, as the SMPL-X
    eyeballs intersect the head.  ``lbs_weights`` [V, J]: 4-sparse rows that vary smoothly over the surface (cubic B-spline weights of
    four consecutive joints along the body's long axis; rows sum to 1).  Deterministic, no random numbers."""
    def lobed(T, P):
        base = 1.0 / np.sqrt((np.sin(T) * np.cos(P) / 0.5) ** 2 + (np.cos(T) / 0.9) ** 2 + (np.sin(T) * np.sin(P) / 0.2) ** 2)
        return base * (1.0 + 0.18 * np.sin(T) ** 2 * np.cos(4.0 * T) * np.cos(2.0 * P) + 0.10 * np.sin(T) ** 2 * np.sin(3.0 * P + 2.0 * T))

    v, f = _lattice_surface(lobed, (0.013, -0.21, 0.017), 145, 72)
    if second_component:
        rim = v[(np.abs(v[:, 1] - (v[:, 1].max() - 0.12)).argmin())]         # a surface point near the top: the small sphere straddles it
        v2, f2 = _lattice_surface(lambda T, P: 0.03 * (1.0 + 0.1 * np.cos(3.0 * P) * np.sin(T)), rim, 9, 12)
        f = np.concatenate([f, f2 + v.shape[0]], 0)
        v = np.concatenate([v, v2], 0)
    y = v[:, 1]
    s = (y - y.min()) / (y.max() - y.min()) * (J - 3) * (1.0 - 1e-9)          # joints k .. k+3, k = floor(s) in [0, J-4]
    k = np.floor(s).astype(np.int64)
    t = s - k
    basis = np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], 1) / 6.0
    w = np.zeros((v.shape[0], J))
    np.put_along_axis(w, k[:, None] + np.arange(4)[None], basis, 1)
    return {"vertices": v.astype(f32), "faces": f.astype(np.int32), "lbs_weights": w.astype(f32)}


def free_view_cameras(n_views: int = 8, img: int = 1024, focal: float = 1100.0, dist: float = 2.5) -> List[Dict[str, object]]:
    cams = []
    for i in range(n_views):
        rot_Y = i / float(n_views) * 2.0 * math.pi
        extr = cam.calc_free_mv(np.zeros(3, f32), tar_pos=(0.0, 0.0, dist), rot_Y=rot_Y)
        intr = np.array([[focal, 0, img / 2], [0, focal, img / 2], [0, 0, 1]], f32)
        cams.append({"extr": extr, "intr": intr, "img_w": img, "img_h": img})
    return cams


def named_fill(state: Dict[str, object], seed: int = SEED) -> Dict[str, object]:
    """Deterministic synthetic values for a network's tensors, a pure function of (name, shape, seed): the same
    numbers can be produced wherever the names are known (the reference module in the build container, this package
    on the GPU box), which is how the StyleUNet parity fixture pins a 74M-parameter network without shipping weights.

    Scales follow the reference's initialisers (randn weights, randn/lr_mul mapping weights come out of the shapes
    alone), with small non-zero biases / noise strengths so that every path contributes."""
    import zlib

    import torch

    out = {}
    for name, t in state.items():
        if name.endswith((".kernel", ".ll", ".lh", ".hl", ".hh")):
            continue
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
        v = torch.randn(tuple(t.shape), generator=g, dtype=torch.float32)
        if name.startswith("style.") and name.endswith(".weight"):
            v = v * 100.0                                  # randn / lr_mlp
        elif name.endswith("modulation.bias"):
            v = 1.0 + 0.1 * v
        elif name.endswith(".bias") or name.endswith("noise.weight"):
            v = 0.1 * v
        out[name] = v
    return out


def pose_map(S: int = 512, seed: int = SEED):
    """Smooth synthetic position map [1, 3, S, S] inside a body-shaped mask (stand-in for smpl_pos_map)."""
    import torch

    rng = np.random.default_rng(seed + 77)
    yy, xx = np.meshgrid(np.linspace(-1, 1, S, dtype=np.float32), np.linspace(-1, 1, S, dtype=np.float32), indexing="ij")
    chans = []
    for c in range(3):
        a = rng.uniform(0.5, 3.0, 4).astype(np.float32)
        chans.append(0.5 * np.sin(a[0] * xx + a[1]) * np.cos(a[2] * yy + a[3]) + 0.1 * xx * (c - 1))
    m = (np.abs(xx) < 0.8) & (np.abs(yy) < 0.9)
    return torch.from_numpy((np.stack(chans) * m[None]).astype(np.float32))[None]


# SMPL-X kinematic tree (55 joints: pelvis, 21 body, jaw, 2 eyes, 15 + 15 finger joints) as the model files' kintree_table[0]
# holds it; any tree with parents[j] < j exercises the same code.
SMPLX_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53)


def smplx_model_arrays(seed: int = SEED, V: int = 10475, shape_dims: int = 400, n_faces: int = 20908) -> Dict[str, np.ndarray]:
    """A synthetic body model with the ARRAY NAMES, SHAPES AND DTYPES of `SMPLX_NEUTRAL.npz` (the licensed model files are
    not redistributable and not in this image): what smplx/body_models.py:237-260,604-625,995-1073 read from the file.
    Random but body-sized: vertices in a 0.6 x 1.7 x 0.3 m box, 1-cm shape / 2-mm pose-corrective bases, each joint a convex
    combination of 32 vertices, 4 skinning weights per vertex."""
    rng = np.random.default_rng(seed)
    J = len(SMPLX_PARENTS)
    m: Dict[str, np.ndarray] = {}
    m['v_template'] = ((rng.random((V, 3)) - 0.5) * np.array([0.6, 1.7, 0.3])).astype(np.float64)
    m['shapedirs'] = (rng.standard_normal((V, 3, shape_dims)) * 0.01).astype(np.float64)
    m['posedirs'] = (rng.standard_normal((V, 3, 9 * (J - 1))) * 0.002).astype(np.float64)
    Jr = np.zeros((J, V))
    for j in range(J):
        idx = rng.choice(V, 32, replace=False)
        w = rng.random(32)
        Jr[j, idx] = w / w.sum()
    m['J_regressor'] = Jr
    kin = np.zeros((2, J), np.int64)
    kin[0] = SMPLX_PARENTS
    kin[0, 0] = 2 ** 32 - 1                      # the files store the root's parent as uint32(-1); smplx overwrites it
    kin[1] = np.arange(J)
    m['kintree_table'] = kin
    W = np.zeros((V, J))
    for k, idx in enumerate(rng.integers(0, J, (4, V))):
        W[np.arange(V), idx] += rng.random(V) + (1.0 if k == 0 else 0.0)
    m['weights'] = W / W.sum(1, keepdims=True)
    m['f'] = rng.integers(0, V, (n_faces, 3)).astype(np.uint32)
    m['hands_componentsl'] = rng.standard_normal((45, 45)) * 0.3
    m['hands_componentsr'] = rng.standard_normal((45, 45)) * 0.3
    m['hands_meanl'] = rng.standard_normal(45) * 0.2
    m['hands_meanr'] = rng.standard_normal(45) * 0.2
    m['lmk_faces_idx'] = rng.integers(0, n_faces, 51).astype(np.int64)
    b = rng.random((51, 3))
    m['lmk_bary_coords'] = b / b.sum(1, keepdims=True)
    return m


def smplx_pose_params(seed: int = SEED, n: int = 1) -> Dict[str, np.ndarray]:
    """`n` frames of the parameter arrays a dataset's smpl_params.npz holds (dataset_mv_rgb.py:44-45)."""
    rng = np.random.default_rng(seed + 17)
    f32 = np.float32
    return {
        'betas': (rng.standard_normal((1, 10)) * 0.8).astype(f32),
        'global_orient': (rng.standard_normal((n, 3)) * 0.6).astype(f32),
        'transl': (rng.standard_normal((n, 3)) * 0.5).astype(f32),
        'body_pose': (rng.standard_normal((n, 63)) * 0.35).astype(f32),
        'jaw_pose': (rng.standard_normal((n, 3)) * 0.1).astype(f32),
        'expression': (rng.standard_normal((n, 10)) * 0.7).astype(f32),
        'left_hand_pose': (rng.standard_normal((n, 45)) * 0.3).astype(f32),
        'right_hand_pose': (rng.standard_normal((n, 45)) * 0.3).astype(f32),
    }


def weight_volume_arrays(mesh: Dict[str, np.ndarray], res=(32, 32, 32), J: int = 55) -> Dict[str, np.ndarray]:
    """A synthetic ``cano_weight_volume.npz`` around ``mesh`` (the stand-in for the SMPL-X body; ``body_mesh()``), with the array names,
    shapes and dtypes ``gen_data/gen_weight_volume.py:164-170`` writes and its bounds rule (:136-150): a cube of 1.1 x the body's
    longest extent about the centre of its bounding box.  The reference's volumes come out of a Poisson solver and libigl, neither of
    which is available here; these are smooth analytic stand-ins with the same post-processing (:131-132: clipped to [0, 1], rows
    normalised to sum 1): ``diff_weight_volume`` [X, Y, Z, J] from Gaussians of 12 cm about J centres along the body's long axis
    over a floor of 1e-3 (every joint non-zero everywhere, as in a diffused volume: the dense skinning path), ``ori_weight_volume``
    from sharper ones (4 cm) without a floor (far joints underflow to exact zeros), ``sdf_volume``
    [X, Y, Z], positive inside, of the bounding ellipsoid.  Deterministic, no random numbers."""
    v = np.asarray(mesh["vertices"], f32)
    min_xyz, max_xyz = v.min(0).astype(f32), v.max(0).astype(f32)
    max_len = f32(1.1) * (max_xyz - min_xyz).max()
    center = (f32(0.5) * (min_xyz + max_xyz)).astype(f32)
    bounds = np.stack([center - f32(0.5) * max_len, center + f32(0.5) * max_len], 0).astype(f32)
    smpl_min, smpl_max = min_xyz.copy(), max_xyz.copy()
    smpl_min[:2] -= 0.05
    smpl_max[:2] += 0.05
    smpl_min[2] -= 0.15
    smpl_max[2] += 0.15
    X, Y, Z = (int(r) for r in res)
    axes = [np.linspace(bounds[0, d], bounds[1, d], r, dtype=np.float64) for d, r in enumerate((X, Y, Z))]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    cy = np.linspace(min_xyz[1], max_xyz[1], J, dtype=np.float64)
    cx = center[0] + 0.25 * (max_xyz[0] - min_xyz[0]) * np.sin(np.arange(J) * 2.4)      # off the axis: the weights vary along x and z too
    cz = center[2] + 0.25 * (max_xyz[2] - min_xyz[2]) * np.cos(np.arange(J) * 1.7)
    d2 = (gx[..., None] - cx) ** 2 + (gy[..., None] - cy) ** 2 + (gz[..., None] - cz) ** 2

    def weights(sigma, floor):
        g = np.exp(-(d2 - d2.min(-1, keepdims=True)) / (2.0 * sigma * sigma)) + floor   # the nearest centre has weight 1 before normalising
        g = np.clip(g, 0.0, 1.0)
        return (g / g.sum(-1, keepdims=True)).astype(f32)

    half = 0.5 * (max_xyz - min_xyz).astype(np.float64)
    r = np.sqrt(((gx - center[0]) / half[0]) ** 2 + ((gy - center[1]) / half[1]) ** 2 + ((gz - center[2]) / half[2]) ** 2)
    return {"diff_weight_volume": weights(0.12, 1e-3), "ori_weight_volume": weights(0.04, 0.0), "sdf_volume": ((1.0 - r) * half.min()).astype(f32),
            "volume_bounds": bounds, "center": center, "smpl_bounds": np.stack([smpl_min, smpl_max], 0).astype(f32)}
