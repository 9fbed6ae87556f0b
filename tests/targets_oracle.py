"""Numpy restatement of the reference loader's training targets (``dataset/dataset_mv_rgb.py:185`` and ``:263-285``), the oracle of
``animatablegaussians_amd.targets``, and the scenes its tests share.

``cv.erode`` / ``cv.dilate`` with a k x k box and OpenCV's default border are a moving minimum / maximum in which pixels outside the
image take part in neither: the erosion is padded with 255 and the dilation with 0 here.  The subtraction stays in uint8, as the
reference's is.  ``tests/test_targets_cpu.py`` checks the two moving extrema against ``scipy.ndimage.grey_erosion`` / ``grey_dilation``;
where ``golden/targets_ref.npz`` exists (``golden/make_golden_targets.py`` on a machine with OpenCV) it checks the whole function against
the reference's own ``get_boundary_mask``."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targets_ref.npz")

SCENE_VALUES = np.array([0, 3, 5, 6, 127, 128, 129, 249, 250, 255], np.uint8)
SCENE_WEIGHTS = np.array([.30, .02, .02, .02, .02, .05, .02, .02, .02, .51])
SCENE_SHAPES = [(1, 3), (4, 4), (37, 70), (19, 131), (70, 203)]


def _moving(img: np.ndarray, k: int, pad_value: int, reduce) -> np.ndarray:
    r = k // 2
    H, W = img.shape
    p = np.pad(img, r, mode="constant", constant_values=pad_value)
    out = p[r:r + H, r:r + W].copy()
    for dy in range(k):
        for dx in range(k):
            out = reduce(out, p[dy:dy + H, dx:dx + W])
    return out


def erode(img: np.ndarray, k: int) -> np.ndarray:
    return _moving(img, k, 255, np.minimum)


def dilate(img: np.ndarray, k: int) -> np.ndarray:
    return _moving(img, k, 0, np.maximum)


def get_boundary_mask(mask: np.ndarray, kernel_size: int = 5):
    """dataset_mv_rgb.py:263-285 line by line on a [H, W] uint8 matte (not modified) -> (boundary_mask bool, mask bool)."""
    assert mask.dtype == np.uint8 and mask.ndim == 2
    mask_bk = mask.copy()
    mask = mask.copy()
    thres = 128
    mask[mask < thres] = 0
    mask[mask > thres] = 1
    mask_erode = erode(mask, kernel_size)
    mask_dilate = dilate(mask, kernel_size)
    boundary_mask = (mask_dilate - mask_erode) == 1                       # uint8 - uint8
    boundary_mask = np.logical_or(boundary_mask, np.logical_and(mask_bk > 5, mask_bk < 250))
    return boundary_mask, mask == 1


def color_float(color: np.ndarray) -> np.ndarray:
    """dataset_mv_rgb.py:185."""
    assert color.dtype == np.uint8
    return (color / 255.).astype(np.float32)


def prepare(color: np.ndarray, matte: np.ndarray, kernel_size: int = 5) -> dict:
    """The three images of one view, or of a stack of views, as the reference's loader makes them."""
    if matte.ndim == 3:
        per = [get_boundary_mask(m, kernel_size) for m in matte]
        boundary, mask = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    else:
        boundary, mask = get_boundary_mask(matte, kernel_size)
    return {"color_img": color_float(color), "mask_img": mask, "boundary_mask_img": boundary}


def class_scene(shape, seed: int = 0) -> np.ndarray:
    """A matte of independent draws from the values around the reference's thresholds (0 | 5, 6 | 127, 128, 129 | 249, 250 | 255)."""
    rs = np.random.RandomState(seed)
    return rs.choice(SCENE_VALUES, size=shape, p=SCENE_WEIGHTS).astype(np.uint8)


def color_scene(shape, seed: int = 0) -> np.ndarray:
    return np.random.RandomState(1000 + seed).randint(0, 256, size=tuple(shape) + (3,)).astype(np.uint8)


def disc_scene(size: int = 41, radius: float = 12.0, soft: float = 3.0) -> np.ndarray:
    """A disc whose matte falls from 255 to 0 over ``soft`` pixels."""
    y, x = np.mgrid[:size, :size].astype(np.float64)
    d = np.hypot(y - size // 2, x - size // 2)
    return np.round(255 * np.clip((radius + soft / 2 - d) / soft, 0, 1)).astype(np.uint8)


def stripe_scene(shape, period: int = 14, axis: int = 1) -> np.ndarray:
    i = np.arange(shape[axis])
    line = np.where((i % period) < period // 2, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(line[None, :] if axis == 1 else line[:, None], shape))


def structured_scenes() -> dict:
    s = {"all_255": np.full((23, 37), 255, np.uint8), "all_0": np.zeros((23, 37), np.uint8), "disc": disc_scene(),
         "stripes_x": stripe_scene((67, 523), 14, 1), "stripes_y": stripe_scene((523, 67), 14, 0)}
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, 8), "corner_bl": (8, 0), "corner_br": (8, 8), "centre": (4, 4)}.items():
        m = np.zeros((9, 9), np.uint8)
        m[y, x] = 255
        s["pixel_" + name] = m
    return s
