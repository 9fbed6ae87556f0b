#!/usr/bin/env python
"""The OpenCV pin of the training targets' boundary band -- runs the moment ``cv2`` and the reference checkout are importable.

`dataset/dataset_mv_rgb.py:263-285` (`MvRgbDatasetBase.get_boundary_mask`) calls `cv.erode` / `cv.dilate` with a k x k box and OpenCV's default
border.  OpenCV is not in this image and cannot be installed (no network), so `tests/targets_oracle.py` restates the function in numpy (erosion
padded with 255, dilation with 0) and `tests/test_targets_cpu.py` checks the two moving extrema against `scipy.ndimage`; parity with OpenCV
itself stays unpinned.  This script closes the gap on any machine that HAS OpenCV and the reference:

    python tests/golden/make_golden_targets.py /path/to/AnimatableGaussians

runs the reference's OWN static method on the scenes the tests use (the random class scenes, the structured scenes, kernel sizes 1 to 7) and
writes `tests/golden/targets_ref.npz` (matte_i, kernel_size_i, boundary_i, mask_i, count, cv2.__version__; well under 1 MiB compressed) and
prints how the numpy restatement compares.  `tests/test_targets_cpu.py::test_which_source_pins_the_boundary_mask` reports which of the two
sources pinned the oracle in a run: with the file present the oracle is asserted against the reference's own outputs.  Without OpenCV or the
reference the script exits 3 and changes nothing."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import targets_oracle as to  # noqa: E402


def reference_function(ref_root):
    """`MvRgbDatasetBase.get_boundary_mask` itself.  The module imports the reference's whole loader stack (smplx, trimesh, ...); where that
    fails, the method's source lines are executed alone with `cv` and `np` bound, which is still the reference's text, not a restatement."""
    import cv2 as cv
    path = os.path.join(ref_root, "dataset", "dataset_mv_rgb.py")
    try:
        sys.path.insert(0, ref_root)
        spec = importlib.util.spec_from_file_location("dataset_mv_rgb_ref", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.MvRgbDatasetBase.get_boundary_mask
    except Exception as e:                                     # noqa: BLE001 -- a missing dependency of the loader, not of the method
        print(f"importing the reference loader failed ({e!r}); executing get_boundary_mask's own lines")
        import textwrap
        lines = open(path).read().splitlines()
        start = next(i for i, l in enumerate(lines) if "def get_boundary_mask" in l)
        end = next(i for i in range(start + 1, len(lines)) if lines[i].strip().startswith("return "))
        ns = {"cv": cv, "np": np}
        exec(textwrap.dedent("\n".join(lines[start:end + 1])), ns)
        return ns["get_boundary_mask"]


def scenes():
    out = [(to.class_scene(shape, 0), 5) for shape in to.SCENE_SHAPES]
    out += [(to.class_scene((37, 70), 0), k) for k in (1, 3, 7)]
    out += [(m, 5) for _, m in sorted(to.structured_scenes().items())]
    return out


def main() -> int:
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AG_REFERENCE_ROOT", "")
    try:
        import cv2
        fn = reference_function(ref_root)
    except Exception as e:                                     # noqa: BLE001 -- any failure means "not on this machine"
        print(f"OpenCV or the reference checkout is not usable here ({e!r}): nothing written; the band stays pinned to the numpy restatement only")
        return 3
    arrays, differing = {}, 0
    cases = scenes()
    for i, (matte, k) in enumerate(cases):
        boundary, mask = fn(matte.copy(), k)
        arrays[f"matte_{i}"], arrays[f"kernel_size_{i}"] = matte, np.array(k)
        arrays[f"boundary_{i}"], arrays[f"mask_{i}"] = np.asarray(boundary, bool), np.asarray(mask, bool)
        ob, om = to.get_boundary_mask(matte, k)
        differing += int((ob != arrays[f"boundary_{i}"]).sum() + (om != arrays[f"mask_{i}"]).sum())
    np.savez_compressed(os.path.join(HERE, "targets_ref.npz"), count=np.array(len(cases)), version=np.array(cv2.__version__), **arrays)
    print(f"OpenCV {cv2.__version__}: get_boundary_mask on {len(cases)} scenes, {differing} pixels differ from the numpy restatement; "
          "wrote tests/golden/targets_ref.npz")
    return 0


if __name__ == "__main__":
    sys.exit(main())
