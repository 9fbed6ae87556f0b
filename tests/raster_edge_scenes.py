"""Seeded scenes that drive the tile rasterizer down the paths its generator-made scenes never take (tests only; numpy and the CPU
oracle, no GPU).  Every builder returns ``(scene, cam, ref, reach)``:

  * ``scene`` / ``cam``: what ``helpers.cam_of`` / ``helpers.oracle_forward`` / ``helpers.gpu_native_forward`` take (``scene`` carries the
    upstream image gradients too);
  * ``ref``: the oracle's forward state of the scene (at the scene's ``scale_modifier``), computed once -- callers must not modify it;
  * ``reach``: the facts that prove the scene takes its path, computed in numpy from the inputs and ``ref`` alone.
    tests/test_raster_edges_cpu.py asserts them, which is what keeps the GPU comparisons of tests/test_raster_edges_gpu.py from passing
    on a scene that no longer reaches the branch it is named after.

The cameras look down +z of view space from ``calc_front_mv``: view = (x, -y, dist - z) of world, so a scene is laid out in VIEW space
(ratio to the depth, depth) and mapped back.  All of them have ``fx != fy``: ``tanfovx / tanfovy`` differs from ``W / H``, so exchanging the
two focal lengths (or the two half-extents of the backward) changes every conic.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import helpers as h
from animatablegaussians_amd import camera

f32 = np.float32
TILE = 16
WIN_BINS = 2048            # csrc/ag_preprocess.hip, csrc/ag_binning.hip: kWinBins, the workgroup's tile-window histogram
SCAN_PASS = 4096           # csrc/ag_binning.hip tile_scan_kernel: tiles per pass (1024 threads x 4)
LAMBDA_HUGE = 1.0e4        # csrc/ag_preprocess.hip: splats with lambda1 >= 1e4 are never culled by r2cut / qcut
OP_MIN = f32(1.0) / f32(255.0)   # the blend's alpha threshold, as the kernels write it (1.0f / 255.0f)


# ---------------------------------------------------------------------------------------------------------------------------------
# construction helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _camera(W, H, fx, fy, dist):
    extr = camera.calc_front_mv(np.zeros(3, f32), tar_pos=(0.0, 0.0, dist))
    intr = np.array([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]], f32)
    return {"extr": extr, "intr": intr, "img_w": W, "img_h": H}


def _from_view(rx, ry, depth, dist):
    """World positions of the view-space points (rx * depth, ry * depth, depth)."""
    return np.stack([rx * depth, -(ry * depth), dist - depth], 1).astype(f32)


def _appearance(rs, P):
    q = rs.normal(0, 1, (P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= rs.uniform(0.8, 1.2, (P, 1))                    # raw quaternions: the rasterizer does not normalise them
    return {"rotations": q.astype(f32), "colors": rs.uniform(0, 1, (P, 3)).astype(f32), "bg": rs.uniform(0, 1, 3).astype(f32)}


def _upstream(rs, W, H):
    return {"dL_dcolor": rs.normal(0, 1, (3, H, W)).astype(f32), "dL_ddepth": rs.normal(0, 1, (1, H, W)).astype(f32),
            "dL_dalpha": rs.normal(0, 1, (1, H, W)).astype(f32)}


def _finish(scene, scale_modifier=1.0):
    scene["scale_modifier"] = float(scale_modifier)
    cam = h.cam_of(scene)
    ref = h.oracle_forward(scene, cam, scale_modifier=float(scale_modifier))
    return scene, cam, ref


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 / exact restatements used by the reach facts
# ---------------------------------------------------------------------------------------------------------------------------------
def view_space(scene, cam):
    """View-space positions in float64 (auxiliary.h transformPoint4x3 on the row-major memory of the matrix)."""
    V = cam["viewmatrix"].astype(np.float64).reshape(-1)
    m = scene["means3D"].astype(np.float64)
    return np.stack([V[0 + k] * m[:, 0] + V[4 + k] * m[:, 1] + V[8 + k] * m[:, 2] + V[12 + k] for k in range(3)], 1)


def clamp_sets(scene, cam, margin=1e-5):
    """Which Gaussians the frustum clamp of computeCov2D moves, per axis and sign: |t / tz| against 1.3 tanfov in float64, rows within
    ``margin`` (relative) of the limit in neither set -- fp32 may decide those either way.  -> dict of boolean arrays."""
    t = view_space(scene, cam)
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    lx, ly = 1.3 * cam["tanfovx"], 1.3 * cam["tanfovy"]
    hi, lo = 1.0 + margin, 1.0 - margin
    out = {"x_pos": rx > lx * hi, "x_neg": rx < -lx * hi, "y_pos": ry > ly * hi, "y_neg": ry < -ly * hi,
           "x_in": np.abs(rx) < lx * lo, "y_in": np.abs(ry) < ly * lo}
    out["x"] = out["x_pos"] | out["x_neg"]
    out["y"] = out["y_pos"] | out["y_neg"]
    out["x_only"] = out["x"] & out["y_in"]
    out["y_only"] = out["y"] & out["x_in"]
    out["both"] = out["x"] & out["y"]
    out["none"] = out["x_in"] & out["y_in"]
    return out


def lambda1_f64(scene, cam, ref):
    """The larger eigenvalue of the dilated 2D covariance (forward.cu computeCov2D + the radius of preprocessCUDA), evaluated in float64 from
    the inputs and the oracle's fp32 cov3D.  fp32 evaluation moves it by ~1e-6 relative: callers keep a 1e-4 band around a threshold."""
    t = view_space(scene, cam)
    lx, ly = 1.3 * cam["tanfovx"], 1.3 * cam["tanfovy"]
    tz = t[:, 2]
    tx = np.clip(t[:, 0] / tz, -lx, lx) * tz
    ty = np.clip(t[:, 1] / tz, -ly, ly) * tz
    fx = cam["img_w"] / (2.0 * cam["tanfovx"])
    fy = cam["img_h"] / (2.0 * cam["tanfovy"])
    P = len(tz)
    J = np.zeros((P, 2, 3))
    J[:, 0, 0], J[:, 0, 2] = fx / tz, -fx * tx / (tz * tz)
    J[:, 1, 1], J[:, 1, 2] = fy / tz, -fy * ty / (tz * tz)
    V = cam["viewmatrix"].astype(np.float64)
    Rv = V[:3, :3].T                                       # view = Rv world + tv
    c = (ref["cov3D"] if scene.get("cov3D_precomp") is None else scene["cov3D_precomp"]).astype(np.float64)
    S = np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(P, 3, 3)
    A = J @ Rv
    cov = A @ S @ A.transpose(0, 2, 1)
    a, b, d = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    mid = 0.5 * (a + d)
    return mid + np.sqrt(np.maximum(0.1, mid * mid - (a * d - b * b)))


def tile_rects(ref, W, H):
    """auxiliary.h getRect on the oracle's projected means and radii, in its fp32 operations -> (x0, y0, x1, y1) int arrays [P]."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    r = ref["radii"].astype(f32)
    px, py = ref["means2D"][:, 0].astype(f32), ref["means2D"][:, 1].astype(f32)
    t = f32(TILE)
    with np.errstate(invalid="ignore"):
        x0 = np.trunc((px - r) / t).astype(np.int64)
        y0 = np.trunc((py - r) / t).astype(np.int64)
        x1 = np.trunc((px + r + t - f32(1)) / t).astype(np.int64)
        y1 = np.trunc((py + r + t - f32(1)) / t).astype(np.int64)
    x0, x1 = np.clip(x0, 0, gx), np.clip(x1, 0, gx)
    y0, y1 = np.clip(y0, 0, gy), np.clip(y1, 0, gy)
    drawn = ref["radii"] > 0
    return tuple(np.where(drawn, v, 0) for v in (x0, y0, x1, y1))


def _common(scene, cam, ref):
    x0, y0, x1, y1 = tile_rects(ref, cam["img_w"], cam["img_h"])
    drawn = ref["radii"] > 0
    return {"P": int(len(drawn)), "drawn": int(drawn.sum()), "num_rendered": int(ref["num_rendered"]),
            "fragile_frac": float(ref["fragile"].astype(bool).mean()),
            "rects_match_tiles_touched": bool(np.array_equal(((x1 - x0) * (y1 - y0)).astype(np.uint32), ref["tiles_touched"])),
            "fx_ne_fy": bool(abs(cam["tanfovx"] / cam["tanfovy"] - cam["img_w"] / cam["img_h"]) > 0.02 * cam["img_w"] / cam["img_h"])}


def _tile_lengths(ref):
    return (ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. scale modifier
# ---------------------------------------------------------------------------------------------------------------------------------
def _scale_modifier_inputs():
    W, H, fx, fy, dist, P = 160, 112, 180.0, 150.0, 2.5, 1500
    rs = np.random.RandomState(41001)
    scene = _camera(W, H, fx, fy, dist)
    rx = rs.uniform(-1.0, 1.0, P) * (W / 2) / fx
    ry = rs.uniform(-1.0, 1.0, P) * (H / 2) / fy
    depth = dist + rs.uniform(-0.2, 0.2, P)
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scene["scales"] = np.exp(rs.normal(math.log(0.02), 0.35, (P, 3))).astype(f32)
    scene["opacities"] = (1.0 / (1.0 + np.exp(-rs.normal(-1.5, 1.2, (P, 1))))).astype(f32)
    scene.update(_appearance(rs, P))
    scene.update(_upstream(rs, W, H))
    return scene


@functools.lru_cache(maxsize=None)
def scale_modifier_scene(scale_modifier=2.0, precomp=False):
    """P = 1500 at 160x112, splats of ~1.4 px at modifier 1: 0.5 leaves most of them at the 0.3 px^2 dilation floor, 2.0 doubles them.
    ``precomp``: the same scene with ``cov3D_precomp`` = the oracle's covariances at modifier 1 and no scales / rotations -- the modifier must
    then be ignored."""
    scene = _scale_modifier_inputs()
    one = h.oracle_forward(scene, h.cam_of(scene))
    if precomp:
        scene = dict(scene, cov3D_precomp=one["cov3D"].copy(), scales=None, rotations=None)
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    both = (ref["radii"] > 0) & (one["radii"] > 0)
    reach["radii_changed_frac"] = float((ref["radii"][both] != one["radii"][both]).mean())
    reach["state_equals_modifier_1"] = bool(all(np.array_equal(ref[k], one[k]) for k in ("radii", "conic_opacity", "means2D", "point_list", "color")))
    return scene, cam, ref, reach


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. frustum clamp
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frustum_clamp_scene(scale_modifier=1.0):
    """144x112 with fx = 80, fy = 128 (tanfovx / tanfovy = 2.06 against W / H = 1.29); 1200 wide splats (sigma 8-11 px) whose view-space
    ratios x / z, y / z reach 1.8x the half-field, so that a good part of the drawn ones lies beyond the 1.3 tanfov clamp of computeCov2D, in x,
    in y, in both and on either side.  (Every splat with opacity above 1 / 255 has a ring of 2 pi sigma^2 1e-4 px^2 on which the oracle calls a
    pixel fragile, whatever its opacity: count and size are chosen to stay below the 5e-3 cap of the image comparison.)"""
    W, H, fx, fy, dist, P = 144, 112, 80.0, 128.0, 2.5, 1200
    rs = np.random.RandomState(41002)
    scene = _camera(W, H, fx, fy, dist)
    rx = rs.uniform(-1.8, 1.8, P) * (W / 2) / fx
    ry = rs.uniform(-1.8, 1.8, P) * (H / 2) / fy
    depth = dist + rs.uniform(-0.3, 0.3, P)
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scene.update(_appearance(rs, P))
    sigma_px = rs.uniform(8.0, 11.0, (P, 1)) * rs.uniform(0.92, 1.08, (P, 3))
    qq = (scene["rotations"].astype(np.float64) ** 2).sum(1, keepdims=True)          # a raw quaternion's matrix is |q|^2 times a rotation
    scene["scales"] = (sigma_px * depth[:, None] / math.sqrt(fx * fy) / qq).astype(f32)
    # many layers deep: low opacities inside the field; a clamped splat's centre lies 0.3+ half-fields outside the image and only its tail
    # is seen, so those are nearly opaque -- otherwise no pixel reaches alpha >= 1 / 255 and their gradients are all zero
    outside = (np.abs(rx) * fx / (W / 2) > 1.3) | (np.abs(ry) * fy / (H / 2) > 1.3)
    scene["opacities"] = np.where(outside, rs.uniform(0.5, 0.95, P), rs.uniform(0.006, 0.03, P)).astype(f32)[:, None]
    scene.update(_upstream(rs, W, H))
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    drawn = ref["radii"] > 0
    cs = clamp_sets(scene, cam)
    n = max(int(drawn.sum()), 1)
    for k in ("x_only", "y_only", "both", "none"):
        reach[k + "_frac"] = float((cs[k] & drawn).sum() / n)
    for k in ("x_pos", "x_neg", "y_pos", "y_neg"):
        reach[k] = int((cs[k] & drawn).sum())
    reach["undecided"] = int((drawn & ~(cs["x"] | cs["x_in"]) | drawn & ~(cs["y"] | cs["y_in"])).sum())
    return scene, cam, ref, reach


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. near plane
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def near_plane_scene(scale_modifier=1.0):
    """96x80 (30 tiles: a ragged scan tail), 600 Gaussians with view depths uniform over 0.05 .. 0.8 -- a fifth behind the 0.2 near-plane cull
    -- and small world scales (~0.008: tens of pixels right beyond the plane, rectangles clamped to the whole tile grid); 24 of those within 0.1
    of the plane are given scales of ~0.12, hundreds of pixels: lambda1 >= 1e4, the side of r2cut / qcut that is never culled.  Opacities stay
    <= 0.05 so that the image does not saturate under the full-screen splats; the large ones take the upper end, which puts the ring where
    their alpha crosses 1 / 255 (the oracle's fragile pixels) outside the image."""
    W, H, fx, fy, P, n_big = 96, 80, 300.0, 260.0, 600, 24
    dist = 1.0
    rs = np.random.RandomState(41003)
    scene = _camera(W, H, fx, fy, dist)
    depth = rs.uniform(0.05, 0.8, P)
    big = np.arange(P) % (P // n_big) == 7
    depth[big] = rs.uniform(0.2005, 0.3, int(big.sum()))
    rx = rs.uniform(-1.6, 1.6, P) * (W / 2) / fx
    ry = rs.uniform(-1.6, 1.6, P) * (H / 2) / fy
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scales = np.exp(rs.normal(math.log(0.008), 0.5, (P, 3)))
    scales[big] = np.exp(rs.normal(math.log(0.12), 0.25, (int(big.sum()), 3)))
    scene["scales"] = scales.astype(f32)
    op = rs.uniform(0.0045, 0.05, (P, 1))
    op[big] = rs.uniform(0.03, 0.05, (int(big.sum()), 1))
    scene["opacities"] = op.astype(f32)
    scene.update(_appearance(rs, P))
    scene.update(_upstream(rs, W, H))
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    drawn = ref["radii"] > 0
    vz = view_space(scene, cam)[:, 2]
    lam = lambda1_f64(scene, cam, ref)
    x0, y0, x1, y1 = tile_rects(ref, W, H)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    reach.update(tiles=gx * gy, tiles_mod_4=(gx * gy) % 4,
                 behind_near_plane=int((vz < 0.2 - 1e-6).sum()), beyond_near_plane=int((vz > 0.2 + 1e-6).sum()),
                 culled_are_exactly_the_near_ones=bool(np.array_equal(drawn | (vz > 0.2 - 1e-6), vz > 0.2 - 1e-6)
                                                       and not (drawn & (vz < 0.2 - 1e-6)).any()),
                 drawn_within_0p05_of_plane=int((drawn & (vz < 0.25)).sum()),
                 drawn_lambda_huge=int((drawn & (lam >= 1.0001 * LAMBDA_HUGE)).sum()),
                 drawn_lambda_ordinary=int((drawn & (lam <= 0.9999 * LAMBDA_HUGE)).sum()),
                 drawn_whole_grid=int((drawn & (x0 == 0) & (y0 == 0) & (x1 == gx) & (y1 == gy)).sum()),
                 max_opacity=float(scene["opacities"].max()), min_transmittance=float(1.0 - ref["alpha"].max()))
    return scene, cam, ref, reach


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. opacity edges
# ---------------------------------------------------------------------------------------------------------------------------------
def opacity_edge_values():
    """name -> float32 opacity: the edges of the wave-level cull (ag_preprocess.hip: r2cut / qcut from log(255 op)) and of the blend's
    min(0.99, .) / alpha < 1 / 255 tests."""
    return {"zero": f32(0.0), "1e-3": f32(1e-3), "below_1_255": np.nextafter(OP_MIN, f32(0)), "above_1_255": np.nextafter(OP_MIN, f32(1)),
            "0.99": f32(0.99), "one": f32(1.0)}


@functools.lru_cache(maxsize=None)
def opacity_edge_scene(scale_modifier=1.0):
    """An ordinary 128x128 scene (P = 1500, splats of ~2 px) with six slices of 100 opacities overwritten by the edge values."""
    W, H, fx, fy, dist, P = 128, 128, 150.0, 135.0, 2.5, 1500
    rs = np.random.RandomState(41004)
    scene = _camera(W, H, fx, fy, dist)
    rx = rs.uniform(-1.0, 1.0, P) * (W / 2) / fx
    ry = rs.uniform(-1.0, 1.0, P) * (H / 2) / fy
    depth = dist + rs.uniform(-0.2, 0.2, P)
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scene["scales"] = np.exp(rs.normal(math.log(0.03), 0.3, (P, 3))).astype(f32)
    op = (1.0 / (1.0 + np.exp(-rs.normal(-1.5, 1.2, (P, 1))))).astype(f32)
    for i, v in enumerate(opacity_edge_values().values()):
        op[100 * i:100 * (i + 1), 0] = v
    scene["opacities"] = op
    scene.update(_appearance(rs, P))
    scene.update(_upstream(rs, W, H))
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    drawn = ref["radii"] > 0
    for name, v in opacity_edge_values().items():
        reach["drawn_" + name] = int((drawn & (scene["opacities"][:, 0] == v)).sum())
    reach["drawn_lambda_huge"] = int((drawn & (lambda1_f64(scene, cam, ref) >= 0.9999 * LAMBDA_HUGE)).sum())
    return scene, cam, ref, reach


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. spatially incoherent workgroups
# ---------------------------------------------------------------------------------------------------------------------------------
def block_windows(ref, W, H, block=256):
    """Per block of ``block`` consecutive Gaussians (one workgroup of the preprocess and of the scatter): the bounding window of the drawn
    rectangles in tiles -> list of (x0, y0, x1, y1) or None for a block that draws nothing."""
    x0, y0, x1, y1 = tile_rects(ref, W, H)
    drawn = ref["radii"] > 0
    out = []
    for s in range(0, len(drawn), block):
        m = drawn[s:s + block]
        if not m.any():
            out.append(None)
            continue
        sl = slice(s, s + block)
        out.append((int(x0[sl][m].min()), int(y0[sl][m].min()), int(x1[sl][m].max()), int(y1[sl][m].max())))
    return out


@functools.lru_cache(maxsize=None)
def incoherent_window_scene(scale_modifier=1.0):
    """780x750 = 49 x 47 = 2303 tiles (T % 4 = 3, one scan pass), P = 2048 splats of ~3 px.  The first 1024 are ordered by the tile of their
    centre, so each of their four workgroups sees a window of a few hundred tiles (the LDS-histogram path); the last 1024 are in random order
    over the whole image, so their workgroups' windows exceed the 2048 bins (the per-instance fallback).  Both kinds land in the same tiles."""
    W, H, fx, fy, dist, P = 780, 750, 800.0, 740.0, 2.5, 2048
    rs = np.random.RandomState(41005)
    scene = _camera(W, H, fx, fy, dist)
    rx = rs.uniform(-1.02, 1.02, P) * (W / 2) / fx
    ry = rs.uniform(-1.02, 1.02, P) * (H / 2) / fy
    # the first half in tile order of the centre (row-major tiles, as the canonical map of an avatar roughly is)
    px, py = (rx[:1024] * fx + W / 2), (ry[:1024] * fy + H / 2)
    order = np.lexsort((px, np.floor(px / TILE), np.floor(py / TILE)))
    rx[:1024], ry[:1024] = rx[:1024][order], ry[:1024][order]
    depth = dist + rs.uniform(-0.2, 0.2, P)
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scene["scales"] = np.exp(rs.normal(math.log(0.01), 0.3, (P, 3))).astype(f32)
    scene["opacities"] = (1.0 / (1.0 + np.exp(-rs.normal(0.0, 1.5, (P, 1))))).astype(f32)
    scene.update(_appearance(rs, P))
    scene.update(_upstream(rs, W, H))
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    wins = block_windows(ref, W, H)
    area = [0 if w is None else (w[2] - w[0]) * (w[3] - w[1]) for w in wins]
    cover = {True: np.zeros((gy, gx), bool), False: np.zeros((gy, gx), bool)}
    x0, y0, x1, y1 = tile_rects(ref, W, H)
    for b, a in enumerate(area):
        for i in range(256 * b, min(256 * (b + 1), P)):
            cover[a <= WIN_BINS][y0[i]:y1[i], x0[i]:x1[i]] = True
    reach.update(tiles=gx * gy, tiles_mod_4=(gx * gy) % 4, window_areas=area,
                 window_blocks=int(sum(0 < a <= WIN_BINS for a in area)), fallback_blocks=int(sum(a > WIN_BINS for a in area)),
                 common_tiles=int((cover[True] & cover[False]).sum()))
    return scene, cam, ref, reach


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. multi-pass tile scan
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multipass_scan_scene(scale_modifier=1.0):
    """1040x1040 = 65 x 65 = 4225 tiles: two passes of the 4096-tile scan, the second one 129 tiles long (T % 4 = 1: a ragged tail inside a
    second pass).  3000 small splats in random order, 60 of them placed in the last tile row and column, the last tile included."""
    W, H, fx, fy, dist, P = 1040, 1040, 1100.0, 1000.0, 2.5, 3000
    rs = np.random.RandomState(41006)
    scene = _camera(W, H, fx, fy, dist)
    px = rs.uniform(0, W, P)
    py = rs.uniform(0, H, P)
    n_edge = 60
    px[:n_edge // 2] = rs.uniform(1026, 1038, n_edge // 2)                 # last tile column
    py[n_edge // 2:n_edge] = rs.uniform(1026, 1038, n_edge // 2)           # last tile row
    px[0], py[0] = 1033.0, 1034.0                                          # the very last tile
    perm = rs.permutation(P)
    px, py = px[perm], py[perm]
    rx, ry = (px - W / 2) / fx, (py - H / 2) / fy
    depth = dist + rs.uniform(-0.2, 0.2, P)
    scene["means3D"] = _from_view(rx, ry, depth, dist)
    scene["scales"] = np.exp(rs.normal(math.log(0.004), 0.3, (P, 3))).astype(f32)
    scene["opacities"] = (1.0 / (1.0 + np.exp(-rs.normal(0.0, 1.5, (P, 1))))).astype(f32)
    scene.update(_appearance(rs, P))
    scene.update(_upstream(rs, W, H))
    scene, cam, ref = _finish(scene, scale_modifier)
    reach = _common(scene, cam, ref)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    n = _tile_lengths(ref)
    T = gx * gy
    reach.update(tiles=T, tiles_mod_4=T % 4, tiles_in_last_pass=T % SCAN_PASS,
                 nonempty_in_second_pass=int((n[SCAN_PASS:] > 0).sum()), last_tile_len=int(n[T - 1]),
                 empty_in_first_pass=int((n[:SCAN_PASS] == 0).sum()), empty_in_second_pass=int((n[SCAN_PASS:] == 0).sum()),
                 nonempty_in_first_pass=int((n[:SCAN_PASS] > 0).sum()))
    return scene, cam, ref, reach
