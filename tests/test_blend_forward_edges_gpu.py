"""GPU parity of the blend forward on the paths around its item loop (pytest -m gpu): the background of empty tiles (one per workgroup,
several per workgroup, the whole image), the background read from device memory on every launch, and several items per workgroup with the
next item's header fetched ahead.

Every test renders through tests/helpers.py and compares against ``h.oracle_forward``: the forward state with ``h._bitexact``, the images with
``h.assert_image_parity`` at its defaults (1e-4 off the oracle's fragile pixels, ``n_contrib`` included).  On top of that every pixel of every
tile whose oracle range is empty must hold the background bit for bit, alpha 0, depth 0 and ``n_contrib`` 0.  No tolerance is introduced
here.  The scenes are small and seeded; what each has to reach (empty tiles, partial tiles, more active tiles than the one-item-per-workgroup
limit) is asserted on the oracle's ranges."""
import functools

import numpy as np
import pytest

import helpers as h
from animatablegaussians_amd import synth

pytestmark = pytest.mark.gpu

TILE = 16
BLEND_GRID = 6144          # workgroups of the blend forward (kBlendGrid, csrc/ag_common.h); 8 region items per active tile
BG = np.array([0.25, 0.5, 0.75], np.float32)      # three different components: a mix-up of two of them shows


def _corner_scene(W, H, P, focal, cx, cy, seed):
    """``P`` Gaussians of synth.random_gaussians seen through a short focal length, so that they gather around pixel (cx, cy)."""
    sc = synth.random_gaussians(P=P, seed=seed, img=max(W, H), focal=focal)
    sc["img_w"], sc["img_h"] = W, H
    sc["intr"] = np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1]], np.float32)
    sc["bg"] = BG.copy()
    sc.update(synth.upstream_grads(W, H, seed + 1))
    return sc


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, camera, oracle forward) of a named scene, computed once and shared; nobody writes to them."""
    if name == "corner":            # 40 x 24: 3 x 2 tiles, the last column 8 wide and the last row 8 high
        sc = _corner_scene(40, 24, 40, 30.0, 6.0, 7.0, 11)
    elif name == "culled":          # 100 x 60, every Gaussian behind the camera
        sc = _corner_scene(100, 60, 300, 60.0, 50.0, 30.0, 12)
        sc["means3D"] = sc["means3D"] + np.array([0, 0, 10.0], np.float32)
    elif name == "sparse_2048":     # 16 384 tiles for 6 144 workgroups: two or three empty tiles each
        sc = synth.random_gaussians(P=200, seed=13, img=2048, focal=2200.0)
        sc["bg"] = BG.copy()
    elif name == "dense_512":       # more than 768 active tiles of 1 024: 8 x active tiles exceeds the grid
        sc = synth.random_gaussians(P=4000, seed=14, img=512, focal=1500.0)
        sc["bg"] = BG.copy()
    else:
        raise KeyError(name)
    cam = h.cam_of(sc)
    return sc, cam, h.oracle_forward(sc, cam)


def _empty_tile_mask(ref, W, H):
    """[H, W] boolean: the pixels of the tiles whose oracle range is empty; also the number of such tiles."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    empty = (ref["ranges"][:, 1] == ref["ranges"][:, 0]).reshape(gy, gx)
    return np.repeat(np.repeat(empty, TILE, 0), TILE, 1)[:H, :W], int(empty.sum())


def _assert_background(color, depth, alpha, n_contrib, mask, bg):
    bg = np.asarray(bg, np.float32)
    for c in range(3):
        got = color[c][mask]
        assert np.array_equal(got.view(np.uint32), np.full(got.shape, bg[c], np.float32).view(np.uint32)), \
            f"colour channel {c} of an empty tile is not bg[{c}] = {bg[c]}: {np.unique(got)[:8]}"
    assert not alpha[0][mask].any(), "alpha of an empty tile is not 0"
    assert not depth[0][mask].any(), "depth of an empty tile is not 0"
    if n_contrib is not None:
        assert not n_contrib[mask].any(), "n_contrib of an empty tile is not 0"


def _render_and_check(name):
    sc, cam, ref = _case(name)
    fw = h.gpu_native_forward(sc, cam)
    h._bitexact(fw, ref)
    h.assert_image_parity(fw, ref)
    mask, n_empty = _empty_tile_mask(ref, cam["img_w"], cam["img_h"])
    _assert_background(fw["color"], fw["depth"], fw["alpha"], fw["n_contrib"], mask, sc["bg"])
    return ref, n_empty


def test_partial_tiles_and_empty_tiles():
    """40 x 24, a few dozen Gaussians in one corner: covered tiles match the oracle, the empty ones (partial tiles among them) hold bg."""
    ref, n_empty = _render_and_check("corner")
    n_tiles = ref["ranges"].shape[0]
    assert n_tiles == 6 and 2 <= n_empty < n_tiles and ref["num_rendered"] > 0
    empty = (ref["ranges"][:, 1] == ref["ranges"][:, 0]).reshape(2, 3)
    assert empty[:, 2].any() and empty[1, :].any(), "the scene must leave a partial tile of either direction empty"


def test_background_is_read_on_every_launch():
    """One prepared FusedRasterStep handle run twice, the bg tensor rewritten in place in between: the second image follows the new bg."""
    import torch
    from animatablegaussians_amd.rasterizer import FusedRasterStep
    sc, cam, ref = _case("corner")
    W, H, P = cam["img_w"], cam["img_h"], sc["means3D"].shape[0]
    bg2 = np.array([0.875, 0.125, 0.375], np.float32)
    sc2 = dict(sc, bg=bg2)
    ref2 = h.oracle_forward(sc2, cam)
    rs = h.gpu_settings(sc, cam)
    inp = h.gpu_inputs(sc)
    ins = [inp[k] for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    gs = [torch.from_numpy(sc[k]).cuda() for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha")]
    step = FusedRasterStep(P, W, H, "cuda", n_streams=1)
    hd = step.prepare(rs, *gs, 0)
    mask, n_empty = _empty_tile_mask(ref, W, H)
    assert n_empty >= 2
    for want, bg in ((ref, sc["bg"]), (ref2, bg2)):
        rs.bg.copy_(torch.from_numpy(bg).cuda())            # in place: the handle keeps the pointer it was prepared with
        color, depth, alpha, radii, _ = step.run(hd, *ins, inputs_outlive_join=True)
        step.join()
        torch.cuda.synchronize()
        got = {"color": color.cpu().numpy(), "depth": depth.cpu().numpy(), "alpha": alpha.cpu().numpy()}
        assert np.array_equal(radii.cpu().numpy(), want["radii"])
        frag = want["fragile"].astype(bool)
        for k in ("color", "depth", "alpha"):
            d = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
            assert d[:, ~frag].max() <= 1e-4, f"{k} with bg {bg}: off the oracle by {d[:, ~frag].max()}"
        _assert_background(got["color"], got["depth"], got["alpha"], None, mask, bg)
    assert np.abs(ref2["color"] - ref["color"]).max() > 0.3        # the two backgrounds are far apart in the oracle too


def test_every_gaussian_culled():
    """P > 0 and nothing in front of the camera: no instance, no active tile, the whole image is bg."""
    sc, cam, ref = _case("culled")
    assert sc["means3D"].shape[0] > 0 and ref["num_rendered"] == 0 and not ref["radii"].any()
    _, n_empty = _render_and_check("culled")
    assert n_empty == ref["ranges"].shape[0] == 7 * 4


def test_several_empty_tiles_per_workgroup():
    """2048 x 2048 with about 200 Gaussians: more than two empty tiles for each workgroup of the grid."""
    ref, n_empty = _render_and_check("sparse_2048")
    assert ref["ranges"].shape[0] == 16384 and n_empty > 2 * BLEND_GRID and ref["num_rendered"] > 0


def test_several_items_per_workgroup():
    """512 x 512 with more than 768 active tiles: the workgroups take several region items each, the next one's header fetched ahead."""
    ref, n_empty = _render_and_check("dense_512")
    n_active = ref["ranges"].shape[0] - n_empty
    assert ref["ranges"].shape[0] == 1024 and n_active > 768 and 8 * n_active > BLEND_GRID
