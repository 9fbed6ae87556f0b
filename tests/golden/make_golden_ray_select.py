#!/usr/bin/env python
"""Writes ``tests/golden/ray_select_ref.npz``: what the reference's OWN ``utils/nerf_util.py`` returns on scenes of
``tests/ray_select_oracle.py``, with the random draws it made.

    python tests/golden/make_golden_ray_select.py /path/to/AnimatableGaussians

* ``get_rays`` / ``get_near_far`` on the 37 x 70 frame of the three cameras (every pixel for ``tilted``, every fourth for the others);
* ``sample_randomly_for_nerf_rendering`` and ``sample_patch_for_nerf_rendering`` on the cases of ``RANDOM_CASES`` / ``PATCH_CASES``.

``nerf_util`` imports ``cv2`` at its top and OpenCV is not among this project's dependencies, so a stub module stands in for it whose
``fillPoly`` is the oracle's integer quad fill: THE BOX'S MASK IN THE FIXTURE IS THEREFORE THIS PROJECT'S, not OpenCV's; everything after
the mask (the candidate order, the rays, the box test, the rounds, the gathers) is the reference's own code.  ``np.int`` (removed from
numpy, used by ``gen_uv``) is set to ``int``.  ``np.random.choice`` / ``np.random.rand`` are wrapped: every draw is recorded and becomes
the ``picks`` of the tests; for the ``tilted`` 37 x 70 case the first round's draws are preset (``ray_select_oracle.make_picks`` with two
pixels of the mask whose ray misses the box), so that the reference runs a second round.  Only data goes into the file.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ray_select_oracle as ro  # noqa: E402

RAY_FRAME, RANDOM_CASES, PATCH_CASES = ro.GOLDEN_RAY_FRAME, ro.GOLDEN_RANDOM_CASES, ro.GOLDEN_PATCH_CASES


def load_reference(ref_root):
    cv2 = types.ModuleType("cv2")

    def fill_poly(mask, polygons, value):
        for pts in polygons:
            pts = np.asarray(pts)
            assert pts.shape == (5, 2) and (pts[0] == pts[4]).all()
            mask[ro.quad_mask(pts[:4], *mask.shape)] = value
    cv2.fillPoly = fill_poly
    sys.modules["cv2"] = cv2
    np.int = int
    spec = importlib.util.spec_from_file_location("nerf_util_ref", os.path.join(ref_root, "utils", "nerf_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Draws:
    """Stands in for ``np.random.choice`` / ``np.random.rand``: replays ``preset`` draws first, then draws from its own seeded state."""

    def __init__(self, seed, preset=()):
        self.rs, self.preset, self.choices, self.rands = np.random.RandomState(seed), list(preset), [], []

    def choice(self, n, size, replace=True):
        assert replace is False
        got = np.asarray(self.preset.pop(0)) if self.preset else self.rs.choice(n, size, replace=False)
        assert len(got) == size and (got < n).all()
        self.choices.append(got.astype(np.int64))
        return got

    def rand(self):
        self.rands.append(self.rs.rand())
        return self.rands[-1]

    def __enter__(self):
        self.saved = (np.random.choice, np.random.rand)
        np.random.choice, np.random.rand = self.choice, self.rand
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.rand = self.saved
        return False


def main() -> int:
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AG_REFERENCE_ROOT", "")
    try:
        nu = load_reference(ref_root)
    except Exception as e:                                     # noqa: BLE001 -- any failure means "not on this machine"
        print(f"the reference checkout is not usable here ({e!r}): nothing written")
        return 3
    arrays = {}
    H, W = RAY_FRAME
    for cam in ro.CAMERAS:
        extr, intr = ro.scene_camera(cam, H, W)
        pix = np.arange(0, H * W, 1 if cam == "tilted" else 4)
        uv = np.stack([pix % W, pix // W], -1)
        ray_d, ray_o = nu.get_rays(uv, extr, intr)
        near, far, hit = nu.get_near_far(ro.BOX, ray_o, ray_d)
        arrays.update({f"rays_{cam}_pix": pix, f"rays_{cam}_ray_d": ray_d, f"rays_{cam}_ray_o": ray_o[0], f"rays_{cam}_near": near,
                       f"rays_{cam}_far": far, f"rays_{cam}_hit": hit})
    for i, (cam, H, W, matte, num, ratio, force) in enumerate(RANDOM_CASES):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, unsample = ro.scene_images(H, W, matte)
        preset = []
        if force:
            missing = ro.missing_bound_pixels(cam, H, W)
            assert len(missing) >= 2
            preset = list(ro.make_picks(cam, H, W, matte, num, ratio, seed=i, force=missing[:2])[0])
        with Draws(100 + i, preset) as draws:
            ret = nu.sample_randomly_for_nerf_rendering(color.copy(), mask.copy(), depth.copy(), extr, intr, ro.BOX, num, ratio, unsample)
        assert len(draws.choices) % 2 == 0 and (not force or len(draws.choices) >= 4)
        arrays[f"random_{i}_rounds"] = np.array(len(draws.choices) // 2)
        for r, c in enumerate(draws.choices):
            arrays[f"random_{i}_pick_{r // 2}_{'in' if r % 2 == 0 else 'out'}"] = c
        arrays.update({f"random_{i}_{k}": np.asarray(v) for k, v in ret.items()})
    for i, (cam, H, W, matte, patch_num, ps, ratio) in enumerate(PATCH_CASES):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, unsample = ro.scene_images(H, W, matte)
        with Draws(200 + i) as draws:
            ret = nu.sample_patch_for_nerf_rendering(color.copy(), mask.copy(), depth.copy(), extr, intr, ro.BOX, patch_num, ps, ratio, unsample)
        arrays[f"patch_{i}_use_inside"] = np.array([p < ratio for p in draws.rands])
        arrays[f"patch_{i}_index"] = np.array([c[0] for c in draws.choices], np.int64)
        arrays.update({f"patch_{i}_{k}": np.asarray(v) for k, v in ret.items()})
    path = os.path.join(HERE, "ray_select_ref.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes; random rounds "
          f"{[int(arrays[f'random_{i}_rounds']) for i in range(len(RANDOM_CASES))]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
