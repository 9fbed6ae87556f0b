"""The training-target path, the part that needs no GPU: the ABI surface and its argument errors (raised before any launch), the host
module's ``TypeError`` / ``ValueError`` cases (raised before anything touches the GPU), and the numpy oracle of
``tests/targets_oracle.py`` against ``scipy.ndimage`` and, where the fixture exists, against the reference's own ``get_boundary_mask``."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_oracle as to  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.sh recompiles a unit when ANY header under csrc/ or include/ is newer than its object
STALE_HEADERS = 'find "$HERE" "$HERE/../../include" -maxdepth 1 -name \'*.h\' -newer "$obj"'
AG_ERR_INVALID_ARGUMENT = -1


def test_entry_point_declared_bound_and_exported():
    import animatablegaussians_amd as pkg
    from animatablegaussians_amd import _lib, targets
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_targets.h")).read(), flags=re.S)
    m = re.search(r"\bag_prepare_targets\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "ag_prepare_targets is not declared in include/ag_targets.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert len(table["ag_prepare_targets"][2]) == n_args == 12
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ag_prepare_targets"), "ag_prepare_targets is not exported"
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_targets\.hip" \$(EXACT|FAST)', build) and STALE_HEADERS in build
    assert pkg.prepare_targets is targets.prepare_targets and pkg.boundary_mask is targets.boundary_mask
    src = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "ag_targets.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src), "the kernel is plain HIP C++: no inline assembly"


def _call(**over):
    """ag_prepare_targets with plausible non-null pointers (never dereferenced: every case here fails validation) -> (code, message)."""
    from animatablegaussians_amd import _lib
    L = _lib.lib()
    a = dict(color=0x1000, matte=0x2000, V=1, H=8, W=8, k=5, color_f=0x3000, mask=0x4000, boundary=0x5000, rows=0x6000, cols=0x7000)
    a.update(over)
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    rc = L.ag_prepare_targets(p(a["color"]), p(a["matte"]), a["V"], a["H"], a["W"], a["k"], p(a["color_f"]), p(a["mask"]), p(a["boundary"]),
                              p(a["rows"]), p(a["cols"]), None)
    return rc, L.ag_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(matte=0), "null"), (dict(mask=0), "null"), (dict(boundary=0), "null"),
    (dict(color=0), "color_u8 and color_f32"), (dict(color_f=0), "color_u8 and color_f32"),
    (dict(V=0), "sizes"), (dict(H=0), "sizes"), (dict(W=-3), "sizes"), (dict(V=-1), "sizes"),
    (dict(k=4), "kernel_size"), (dict(k=0), "kernel_size"), (dict(k=17), "kernel_size"), (dict(k=-5), "kernel_size"), (dict(k=16), "kernel_size"),
    (dict(rows=0), "row_any_u8 and col_any_u8"), (dict(cols=0), "row_any_u8 and col_any_u8"),
    (dict(color_f=0x3002), "aligned"),
])
def test_invalid_arguments_are_refused_before_any_launch(over, word):
    rc, msg = _call(**over)
    assert rc == AG_ERR_INVALID_ARGUMENT and word in msg, (rc, msg)


def test_host_module_type_and_value_errors():
    import torch
    from animatablegaussians_amd.targets import boundary_mask, prepare_targets
    c, m = np.zeros((6, 5, 3), np.uint8), np.zeros((6, 5), np.uint8)
    for bad_c, bad_m in ((c.astype(np.float32), m), (c, m.astype(bool)), (c, m.astype(np.int32)), (torch.zeros(6, 5, 3), torch.from_numpy(m)),
                         (torch.from_numpy(c), torch.zeros(6, 5, dtype=torch.bool)), (c.tolist(), m), (c, None), (None, m)):
        with pytest.raises(TypeError):
            prepare_targets(bad_c, bad_m)
    with pytest.raises(TypeError):
        boundary_mask(m.astype(np.float64))
    with pytest.raises(ValueError, match="3-channel"):
        prepare_targets(c, c)
    with pytest.raises(ValueError, match="3-channel"):
        prepare_targets(np.zeros((2, 6, 5, 3), np.uint8), torch.zeros(2, 6, 5, 3, dtype=torch.uint8))
    for bad_c, bad_m in ((c, np.zeros((5, 6), np.uint8)), (c, np.zeros((1, 6, 5), np.uint8)), (np.zeros((2, 6, 5, 3), np.uint8), m),
                         (np.zeros((6, 5, 4), np.uint8), m), (np.zeros((6, 5), np.uint8), m), (np.zeros((0, 5, 3), np.uint8), np.zeros((0, 5), np.uint8))):
        with pytest.raises(ValueError):
            prepare_targets(bad_c, bad_m)
    for k in (0, 2, 4, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="kernel_size"):
            prepare_targets(c, m, kernel_size=k)
        with pytest.raises(ValueError, match="kernel_size"):
            boundary_mask(m, kernel_size=k)
    with pytest.raises(ValueError, match="GPU"):
        prepare_targets(c, m, device="cpu")
    with pytest.raises(ValueError):
        boundary_mask(np.zeros((2, 2, 6, 5), np.uint8))


@pytest.mark.parametrize("shape", to.SCENE_SHAPES)
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_oracle_extrema_agree_with_scipy(shape, k):
    from scipy import ndimage
    m = to.class_scene(shape, seed=0)
    c = np.where(m < 128, 0, np.where(m > 128, 1, 128)).astype(np.uint8)
    for img in (c, m):
        assert np.array_equal(to.erode(img, k), ndimage.grey_erosion(img, size=(k, k), mode="constant", cval=255))
        assert np.array_equal(to.dilate(img, k), ndimage.grey_dilation(img, size=(k, k), mode="constant", cval=0))


def test_oracle_on_cases_worked_by_hand():
    for fill in (0, 255):                                                  # outside pixels take no part: a constant matte has no band
        b, mk = to.get_boundary_mask(np.full((7, 9), fill, np.uint8))
        assert not b.any() and mk.all() == (fill == 255)
    m = np.zeros((9, 9), np.uint8)
    m[0, 0] = 255
    b, mk = to.get_boundary_mask(m)                                        # 5 x 5 windows that see the corner pixel: rows and columns 0 .. 2
    want = np.zeros((9, 9), bool)
    want[:3, :3] = True
    assert np.array_equal(b, want) and mk.sum() == 1 and mk[0, 0]
    m = np.zeros((9, 9), np.uint8)
    m[4, 3], m[4, 5] = 255, 128                                            # a window that holds a 128 has emax - emin = 128 or 127, never 1
    b, mk = to.get_boundary_mask(m, 3)
    want = np.zeros((9, 9), bool)
    want[3:6, 2:4] = True                                                  # windows with the 255 and without the 128: columns 2 and 3
    want[4, 5] = True                                                      # and 128 itself lies in the soft band 5 < m < 250
    assert np.array_equal(b, want) and not mk[4, 5] and mk[4, 3]
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    b, mk = to.get_boundary_mask(v, 1)
    assert np.array_equal(b, (v > 5) & (v < 250)) and np.array_equal(mk, v > 128)
    src = v.copy()
    to.get_boundary_mask(src)
    assert np.array_equal(src, v)                                          # the caller's matte is not modified


def test_colour_division_is_the_reference_rounding_and_a_reciprocal_is_not():
    v = np.arange(256, dtype=np.uint8)
    want = to.color_float(v)
    assert want.dtype == np.float32
    assert np.array_equal(want.view(np.int32), (v.astype(np.float32) / np.float32(255)).view(np.int32))       # one fp32 division
    assert int((want != v.astype(np.float32) * (np.float32(1) / np.float32(255))).sum()) == 126               # not a multiplication


def test_random_scenes_are_balanced():
    """What keeps an all-true or an all-false output from passing the GPU test: on the larger shapes band, mask and their complements
    each cover at least a tenth of the pixels."""
    for shape in to.SCENE_SHAPES:
        if shape[0] * shape[1] < 37 * 70:
            continue
        b, mk = to.get_boundary_mask(to.class_scene(shape, 0))
        for frac in (b.mean(), 1 - b.mean(), mk.mean(), 1 - mk.mean()):
            assert frac >= 0.10, (shape, b.mean(), mk.mean())


def test_which_source_pins_the_boundary_mask():
    """The pin, stated by the run itself.  ``tests/golden/targets_ref.npz`` exists only where ``make_golden_targets.py`` ran with OpenCV
    importable (not in the build image): then the oracle is asserted against the outputs of the reference's own ``get_boundary_mask``.
    Otherwise the pin is this file's scipy comparison and hand-worked cases, and the test says so."""
    if not os.path.exists(to.GOLDEN):
        print("\n[parity] get_boundary_mask pinned by: the numpy restatement (tests/targets_oracle.py) checked against scipy.ndimage's "
              "grey_erosion / grey_dilation; OpenCV itself: NOT available in this image (tests/golden/make_golden_targets.py writes the pin where it is)")
        return
    g = np.load(to.GOLDEN)
    n = int(g["count"])
    for i in range(n):
        b, mk = to.get_boundary_mask(g[f"matte_{i}"], int(g[f"kernel_size_{i}"]))
        assert np.array_equal(b, g[f"boundary_{i}"]) and np.array_equal(mk, g[f"mask_{i}"]), i
    print(f"\n[parity] get_boundary_mask pinned by: the reference's own function on OpenCV {g['version']} ({n} scenes, tests/golden/targets_ref.npz)")
