"""The ray selection, the part that needs no GPU: the ABI surface and its argument errors (raised before any launch), the module's
``ValueError`` cases (raised before anything touches the GPU), and the numpy oracle of ``tests/ray_select_oracle.py``:

* its float64 version against the reference's own ``get_rays`` / ``get_near_far`` / ``sample_randomly_for_nerf_rendering`` /
  ``sample_patch_for_nerf_rendering`` (``tests/golden/ray_select_ref.npz``, written by ``tests/golden/make_golden_ray_select.py``; the
  box's mask in that file is this project's integer fill, OpenCV's was never run).  Integers, flags and gathered values are equal;
  float64 values agree to 1e-12 (the reference's ``einsum`` / ``norm`` may sum in another order than the oracle's left-to-right sums);
* its float32 version, the one the kernels are compared with bit for bit, against the float64 one: the hit flag of every ray of every
  scene is equal (no ray is left out), and ``near`` / ``far`` / ``ray_d`` deviate by at most TWICE the largest deviation measured over
  the scenes (``MEASURED``; DESIGN.md "Ray selection" has the figures).  Both sides are deterministic: the factor only absorbs another
  numpy build's summation order inside the reference's float64 values.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_select_oracle as ro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ray_select_ref.npz")
AG_ERR_INVALID_ARGUMENT = -1
F64_TOL = 1e-12
# max |float32 oracle - float64| over every pixel of every frame x camera of the oracle (hit rays for near / far), measured on the CPU
MEASURED = {"near_far": 2.07e-6, "ray_d": 1.56e-7}
NAMES = ("ag_ray_classify", "ag_ray_compact_workspace_bytes", "ag_ray_compact", "ag_ray_camera_bytes", "ag_ray_build", "ag_ray_box_near_far")


@pytest.fixture(scope="module")
def ref():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    import animatablegaussians_amd as pkg
    from animatablegaussians_amd import _lib, ray_select
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_ray_select.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_ray_select.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(table[name][2]) == n_args, name
        assert hasattr(L, name), f"{name} is not exported"
    assert _lib.lib().ag_ray_camera_bytes() == ctypes.sizeof(_lib.AgRayCamera) == 4 * (9 + 9 + 3 + 4 + 6 + 2)
    assert _lib.lib().ag_ray_compact_workspace_bytes(0) >= 256 and _lib.lib().ag_ray_compact_workspace_bytes(-1) == 0
    assert _lib.lib().ag_ray_compact_workspace_bytes(1500 * 2048) >= 6000 * 8
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_ray_select\.hip" \$EXACT', build), "the float32 contract needs -ffp-contract=off"
    for name in ("get_rays", "get_near_far", "bound_mask", "candidates", "sample_randomly", "sample_patches", "image_rays", "render_image"):
        assert getattr(pkg, name) is getattr(ray_select, name) and name in pkg.__all__
    src = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "ag_ray_select.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code, "plain HIP C++ without inline assembly and without atomics"


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _classify(**over):
    from animatablegaussians_amd import _lib
    a = dict(corners=[0, 0, 4, 0, 0, 4, 4, 4] * 2, H=8, W=8, cls=0x3000)
    a.update(over)
    xy = (ctypes.c_int32 * 16)(*a["corners"]) if a["corners"] is not None else None
    L = _lib.lib()
    return L.ag_ray_classify(xy, a["H"], a["W"], None, None, _p(a["cls"]), None), L.ag_last_error().decode()


def _compact(**over):
    from animatablegaussians_amd import _lib
    a = dict(flags=0x1000, n=100, list1=0x2000, list2=0x3000, counts=0x4000, ws=0x5000, ws_bytes=1 << 20)
    a.update(over)
    L = _lib.lib()
    return L.ag_ray_compact(_p(a["flags"]), a["n"], _p(a["list1"]), _p(a["list2"]), _p(a["counts"]), _p(a["ws"]), a["ws_bytes"], None), L.ag_last_error().decode()


def _build(**over):
    """Every case handed in here fails validation (or has n = 0): the placeholder pointers are never dereferenced."""
    from animatablegaussians_amd import _lib
    a = dict(cam=True, W=8, H=8, pix=0x1000, uv_in=0, n=10, color=0, mask=0, depth=0, uv=0x2000, ray_o=0x3000, ray_d=0x4000, near=0x5000, far=0x6000,
             hit=0x7000, color_gt=0, mask_gt=0, depth_gt=0, dist=0)
    a.update(over)
    cam = _lib.AgRayCamera()
    cam.W, cam.H = a["W"], a["H"]
    L = _lib.lib()
    rc = L.ag_ray_build(ctypes.byref(cam) if a["cam"] else None, _p(a["pix"]), _p(a["uv_in"]), a["n"], _p(a["color"]), _p(a["mask"]), _p(a["depth"]),
                        _p(a["uv"]), _p(a["ray_o"]), _p(a["ray_d"]), _p(a["near"]), _p(a["far"]), _p(a["hit"]), _p(a["color_gt"]), _p(a["mask_gt"]),
                        _p(a["depth_gt"]), _p(a["dist"]), None)
    return rc, L.ag_last_error().decode()


@pytest.mark.parametrize("call,over,word", [
    (_classify, dict(corners=None), "null"), (_classify, dict(cls=0), "null"), (_classify, dict(H=0), "frame"), (_classify, dict(W=-2), "frame"),
    (_classify, dict(H=65536, W=32768), "frame"), (_classify, dict(corners=[0] * 15 + [(1 << 29) + 1]), "2^29"),
    (_classify, dict(corners=[-(1 << 29) - 1] + [0] * 15), "2^29"),
    (_compact, dict(n=-1), "outside"), (_compact, dict(n=1 << 31), "outside"), (_compact, dict(flags=0), "null"), (_compact, dict(list1=0), "null"),
    (_compact, dict(counts=0), "null"), (_compact, dict(ws=0), "null"), (_compact, dict(ws_bytes=16), "workspace"),
    (_build, dict(cam=False), "null camera"), (_build, dict(n=-1), "outside"), (_build, dict(n=1 << 31), "outside"),
    (_build, dict(uv_in=0x8000), "alternatives"), (_build, dict(color=0x8000), "go together"), (_build, dict(mask=0x8000), "go together"),
    (_build, dict(depth=0x8000), "go together"), (_build, dict(pix=0, uv_in=0x8000, color=0x8100, mask=0x8200), "take no images"),
    (_build, dict(W=0), "frame"), (_build, dict(H=-1), "frame"), (_build, dict(pix=0, n=63), "W H"),
    (_build, dict(color_gt=0x8000), "all given with images"), (_build, dict(color=0x8000, mask=0x8100, color_gt=0x8200, mask_gt=0x8300, depth_gt=0x8400), "all given with images"),
    (_build, dict(near=0), "go together"), (_build, dict(hit=0), "go together"),
])
def test_invalid_arguments_are_refused_before_any_launch(call, over, word):
    rc, msg = call(**over)
    assert rc == AG_ERR_INVALID_ARGUMENT and word in msg, (rc, msg)


def test_empty_calls_succeed_without_a_launch():
    from animatablegaussians_amd import _lib
    assert _build(n=0)[0] == 0
    L = _lib.lib()
    b = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert L.ag_ray_box_near_far(b, None, None, 0, None, None, None, None) == 0
    assert L.ag_ray_box_near_far(None, None, None, 0, None, None, None, None) == AG_ERR_INVALID_ARGUMENT
    assert L.ag_ray_box_near_far(b, None, _p(0x1000), 5, _p(0x2000), _p(0x3000), _p(0x4000), None) == AG_ERR_INVALID_ARGUMENT


# ---- the module's refusals that need no GPU -------------------------------------------------------------------------------------------------
def test_value_errors_before_anything_touches_the_gpu():
    import torch
    from animatablegaussians_amd import ray_select as rs
    H, W = 37, 70
    extr, intr = ro.scene_camera("tilted", H, W)
    color, mask, depth, _ = (None if a is None else torch.from_numpy(np.array(a)) for a in ro.scene_images(H, W))
    behind = extr.copy()
    behind[2, 3] = 0.2                                                              # the box's near corners end up behind the camera
    with pytest.raises(ValueError, match="behind the camera"):
        rs.project_corners(ro.BOX, intr, behind)
    with pytest.raises(ValueError, match="behind the camera"):
        rs.bound_mask(ro.BOX, intr, behind, H, W)
    with pytest.raises(ValueError, match="behind the camera"):
        ro.project_corners(ro.BOX, intr, behind)
    for bad in (lambda: rs.candidates(mask, ro.BOX, extr, intr),                     # host tensors
                lambda: rs.sample_randomly(color, mask, depth, extr, intr, ro.BOX),
                lambda: rs.sample_patches(color, mask, depth, extr, intr, ro.BOX),
                lambda: rs.get_rays(torch.zeros(4, 2, dtype=torch.int32), extr, intr),
                lambda: rs.get_near_far(ro.BOX, torch.zeros(4, 3), torch.zeros(4, 3)),
                lambda: rs.candidates(mask.numpy(), ro.BOX, extr, intr),
                lambda: rs.bound_mask(ro.BOX, intr, extr, H, W, device="cpu"),
                lambda: rs.image_rays(extr, intr, W, H, ro.BOX, device="cpu"),
                lambda: rs.bound_mask(ro.BOX, intr, extr, 0, W),
                lambda: rs.bound_mask(ro.BOX[0], intr, extr, H, W),
                lambda: rs.bound_mask(ro.BOX[::-1], intr, extr, H, W),
                lambda: rs.bound_mask(ro.BOX, intr[:2], extr, H, W),
                lambda: rs.bound_mask(ro.BOX, intr, np.full((4, 4), np.nan), H, W),
                lambda: rs.render_image(object(), extr, intr, W, H, ro.BOX)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="resize_factor"):
        rs.sample_patches(color, mask, depth, extr, intr, ro.BOX, resize_factor=0.5)
    assert np.array_equal(rs.project_corners(ro.BOX, intr, extr), ro.project_corners(ro.BOX, intr, extr))


def test_patch_origin_clips_at_all_four_borders():
    patch_origin = ro.patch_origin
    for size, ps in ((70, 32), (37, 32), (64, 8), (48, 7), (9, 9)):
        for c in range(size):
            lo = c - ps // 2
            assert patch_origin(c, size, ps) == (0 if lo < 0 else size - ps if lo > size - ps else lo)
    assert patch_origin(0, 70, 32) == 0 and patch_origin(69, 70, 32) == 38 and patch_origin(35, 70, 32) == 19       # left / top, right / bottom, free
    assert patch_origin(3, 37, 32) == 0 and patch_origin(36, 37, 32) == 5


# ---- the integer quad fill --------------------------------------------------------------------------------------------------------------
def test_quad_fill_on_hand_made_quads():
    sq = [(1, 1), (4, 1), (4, 3), (1, 3)]
    want = np.zeros((6, 7), bool)
    want[1:4, 1:5] = True                                                           # closed: the boundary pixels belong to it
    assert np.array_equal(ro.quad_mask(sq, 6, 7), want)
    assert np.array_equal(ro.quad_mask(sq[::-1], 6, 7), want), "the other winding"
    assert np.array_equal(ro.quad_mask(sq[2:] + sq[:2], 6, 7), want), "another first vertex"
    diamond = ro.quad_mask([(3, 0), (6, 3), (3, 6), (0, 3)], 7, 7)
    y, x = np.mgrid[0:7, 0:7]
    assert np.array_equal(diamond, np.abs(x - 3) + np.abs(y - 3) <= 3)
    seg = ro.quad_mask([(1, 1), (4, 4), (4, 4), (1, 1)], 7, 7)                      # degenerate: a segment, not its whole line
    assert np.array_equal(np.argwhere(seg), [[1, 1], [2, 2], [3, 3], [4, 4]])
    flat = ro.quad_mask([(0, 2), (3, 2), (5, 2), (2, 2)], 5, 8)                     # four collinear vertices
    assert np.array_equal(np.argwhere(flat), [[2, k] for k in range(6)])
    point = ro.quad_mask([(2, 3)] * 4, 5, 5)
    assert np.array_equal(np.argwhere(point), [[3, 2]])
    assert not ro.quad_mask([(10, 10), (14, 10), (14, 13), (10, 13)], 6, 7).any(), "off the frame"
    assert not ro.quad_mask([(-9, -9), (-5, -9), (-5, -6), (-9, -6)], 6, 7).any()
    part = ro.quad_mask([(-3, -2), (2, -2), (2, 1), (-3, 1)], 6, 7)                 # half off the frame
    assert np.array_equal(part, (x[:6, :7] <= 2) & (y[:6, :7] <= 1))
    assert ro.quad_mask([(-100, -100), (100, -100), (100, 100), (-100, 100)], 5, 3).all(), "a quad larger than the frame"
    big = 1 << 29
    assert ro.quad_mask([(-big, -big), (big, -big), (big, big), (-big, big)], 3, 3).all(), "int64 edge functions at the coordinate limit"


def test_scenes_hold_what_the_tests_rely_on():
    for H, W in ((37, 70), (48, 64)):
        missing = ro.missing_bound_pixels("tilted", H, W)
        assert len(missing) >= 2, "tilted needs pixels of the mask whose ray misses the box (a second sampling round)"
        assert np.array_equal(missing, ro.missing_bound_pixels("tilted", H, W, ro.F32))
    extr, intr = ro.scene_camera("axis", 48, 64)
    d, _ = ro.get_rays(np.array([[32, 24]]), extr, intr, ro.F32)
    assert d[0, 0] == 0 and d[0, 1] == 0 and d[0, 2] == 1, "the centre ray of the axis camera has exact zeros (the + 1e-9f path)"
    for H, W in ro.FRAMES[2:]:
        for cam in ro.CAMERAS:
            extr, intr = ro.scene_camera(cam, H, W)
            _, mask, _, _ = ro.scene_images(H, W)
            inside, outside, bound = ro.candidates(mask, ro.BOX, extr, intr)
            assert len(inside) and len(outside) and not bound.all(), (H, W, cam)
    moved = ro.BOX + np.float32([40, 0, 0])
    extr, intr = ro.scene_camera("axis", 37, 70)
    assert not ro.bound_mask(moved, intr, extr, 37, 70).any(), "a box moved off the frame has an empty mask"


# ---- float64 oracle = the reference ---------------------------------------------------------------------------------------------------------
def _close64(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= F64_TOL, f"{name}: {err:.3e}"
    return err


def test_float64_oracle_equals_the_references_rays(ref):
    H, W = ro.GOLDEN_RAY_FRAME
    for cam in ro.CAMERAS:
        extr, intr = ro.scene_camera(cam, H, W)
        b = ro.build(ref[f"rays_{cam}_pix"], extr, intr, ro.BOX, H, W, dt=ro.F64)
        assert np.array_equal(b["hit"], ref[f"rays_{cam}_hit"]), cam
        hit = b["hit"]
        errs = [_close64(f"{cam} ray_d", b["ray_d"], ref[f"rays_{cam}_ray_d"]), _close64(f"{cam} ray_o", b["ray_o"][0], ref[f"rays_{cam}_ray_o"]),
                _close64(f"{cam} near", b["near"][hit], ref[f"rays_{cam}_near"]), _close64(f"{cam} far", b["far"][hit], ref[f"rays_{cam}_far"])]
        print(f"{cam}: {len(hit)} rays, {int(hit.sum())} hit; |float64 oracle - reference| ray_d {errs[0]:.1e}, ray_o {errs[1]:.1e}, near {errs[2]:.1e}, far {errs[3]:.1e}")
        assert hit.any() and not hit.all()


def _batch_equals(name, got, want, keys):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("uv", "mask_within_patch", "color_gt", "mask_gt", "depth_gt"):
            assert g.shape == w.shape and np.array_equal(g, w), f"{name} {k}"
        elif k == "dist":                                                        # the reference rounds its float64 value to float32
            assert g.shape == w.shape and (np.abs(g - w) <= 2.0 ** -23 * np.abs(g)).all(), f"{name} {k}"
        else:
            _close64(f"{name} {k}", g, w)


def _random_picks(ref, i):
    return [(ref[f"random_{i}_pick_{r}_in"], ref[f"random_{i}_pick_{r}_out"]) for r in range(int(ref[f"random_{i}_rounds"]))]


def test_float64_oracle_equals_the_references_random_batches(ref):
    for i, (cam, H, W, matte, num, ratio, force) in enumerate(ro.GOLDEN_RANDOM_CASES):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, unsample = ro.scene_images(H, W, matte)
        picks = _random_picks(ref, i)
        got = ro.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, unsample, picks, ro.F64)
        want = {k: ref[f"random_{i}_{k}"] for k in ("uv", "ray_o", "ray_d", "near", "far", "color_gt", "mask_gt", "depth_gt", "dist")}
        assert got["rounds"] == len(picks) and len(want["uv"]) == num and (not force or len(picks) >= 2)
        _batch_equals(f"random {i}", got, want, want.keys())
        assert (want["color_gt"][want["mask_gt"] == 0] == 0).all() and want["mask_gt"].dtype == np.float32


def test_float64_oracle_equals_the_references_patches(ref):
    for i, (cam, H, W, matte, patch_num, ps, ratio) in enumerate(ro.GOLDEN_PATCH_CASES):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, unsample = ro.scene_images(H, W, matte)
        picks = list(zip(ref[f"patch_{i}_use_inside"].tolist(), ref[f"patch_{i}_index"].tolist()))
        got = ro.sample_patches(color, mask, depth, extr, intr, ro.BOX, patch_num, ps, unsample, picks, ro.F64)
        keys = ("uv", "mask_within_patch", "ray_o", "ray_d", "near", "far", "color_gt", "mask_gt", "depth_gt", "dist")
        want = {k: ref[f"patch_{i}_{k}"] for k in keys}
        assert len(want["uv"]) == patch_num * ps * ps and want["mask_within_patch"].sum() == len(want["ray_o"]) == len(want["dist"])
        _batch_equals(f"patch {i}", got, want, keys)


# ---- float32 oracle against float64 ---------------------------------------------------------------------------------------------------------
def test_float32_oracle_against_float64_on_every_scene():
    worst = {"near_far": 0.0, "ray_d": 0.0, "dist": 0.0}
    for H, W in ro.FRAMES:
        color, mask, depth, _ = ro.scene_images(H, W)
        for cam in ro.CAMERAS:
            extr, intr = ro.scene_camera(cam, H, W)
            b32 = ro.build(None, extr, intr, ro.BOX, H, W, color, mask, depth, ro.F32)
            b64 = ro.build(None, extr, intr, ro.BOX, H, W, color, mask, depth, ro.F64)
            assert all(b32[k].dtype == np.float32 for k in ("ray_o", "ray_d", "near", "far", "dist", "color_gt", "depth_gt"))
            assert np.array_equal(b32["hit"], b64["hit"]), f"{H} x {W} {cam}: the hit flag of {int((b32['hit'] != b64['hit']).sum())} rays differs"
            hit = b64["hit"]
            nf = max(float(np.abs(b32[k][hit] - b64[k][hit]).max()) for k in ("near", "far")) if hit.any() else 0.0
            rd = float(np.abs(b32["ray_d"] - b64["ray_d"]).max())
            worst = {"near_far": max(worst["near_far"], nf), "ray_d": max(worst["ray_d"], rd),
                     "dist": max(worst["dist"], float(np.abs(b32["dist"] - b64["dist"]).max()))}
            assert not b32["near"][~hit].any() and not b32["far"][~hit].any() and (b32["near"][hit] < b32["far"][hit]).all()
            assert np.array_equal(b32["uv"], b64["uv"]) and np.array_equal(b32["color_gt"], b64["color_gt"].astype(np.float32))
    print(f"max |float32 oracle - float64| over {len(ro.FRAMES) * len(ro.CAMERAS)} scenes: near / far {worst['near_far']:.3e}, ray_d {worst['ray_d']:.3e}, "
          f"dist {worst['dist']:.3e}; asserted at twice {MEASURED}")
    assert worst["near_far"] <= 2 * MEASURED["near_far"] and worst["ray_d"] <= 2 * MEASURED["ray_d"]
    assert worst["near_far"] >= 0.5 * MEASURED["near_far"] and worst["ray_d"] >= 0.5 * MEASURED["ray_d"], "MEASURED no longer describes these scenes"


def test_float32_oracle_against_the_references_values(ref):
    H, W = ro.GOLDEN_RAY_FRAME
    for cam in ro.CAMERAS:
        extr, intr = ro.scene_camera(cam, H, W)
        b = ro.build(ref[f"rays_{cam}_pix"], extr, intr, ro.BOX, H, W, dt=ro.F32)
        assert np.array_equal(b["hit"], ref[f"rays_{cam}_hit"]), f"{cam}: hit flags differ from the reference's"
        hit = b["hit"]
        nf = max(float(np.abs(b["near"][hit] - ref[f"rays_{cam}_near"]).max()), float(np.abs(b["far"][hit] - ref[f"rays_{cam}_far"]).max()))
        rd = float(np.abs(b["ray_d"] - ref[f"rays_{cam}_ray_d"]).max())
        print(f"{cam}: |float32 oracle - reference| near / far {nf:.3e}, ray_d {rd:.3e}")
        assert nf <= 2 * MEASURED["near_far"] and rd <= 2 * MEASURED["ray_d"]
    for i, (cam, H, W, matte, num, ratio, _) in enumerate(ro.GOLDEN_RANDOM_CASES):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, unsample = ro.scene_images(H, W, matte)
        got = ro.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, unsample, _random_picks(ref, i), ro.F32)
        assert np.array_equal(got["uv"], ref[f"random_{i}_uv"]) and np.array_equal(got["color_gt"], ref[f"random_{i}_color_gt"])
        for k, bar in (("near", "near_far"), ("far", "near_far"), ("ray_d", "ray_d")):
            assert float(np.abs(got[k] - ref[f"random_{i}_{k}"]).max()) <= 2 * MEASURED[bar], (i, k)
