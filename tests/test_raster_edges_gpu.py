"""GPU parity of the HIP rasterizer against the CPU oracle on the edge scenes of tests/raster_edge_scenes.py (pytest -m gpu): the scale
modifier, the frustum clamp of computeCov2D under an asymmetric camera, splats right beyond the near plane, the opacity edges of the wave-
level cull, workgroups on either side of the tile-window limit, and a tile scan of two passes with a ragged tail.

Every test: (a) forward state bit-exact + images at ``assert_image_parity``'s defaults; (b) the backward at levels 1 and 2 of
test_raster_gpu.py::_check_backward -- blend-backward accumulators on the oracle's alpha map (``assert_accum_parity`` at its defaults), then
the streaming preprocess backward on the GPU's own accumulators against ``backward_preprocess`` (``assert_rows_close``: default, 3e-5 for
rotations) -- both with the scene's ``scale_modifier``; gradients of culled Gaussians exactly zero.  No tolerance is introduced here.
That each scene reaches its path is asserted on the CPU (tests/test_raster_edges_cpu.py)."""
import numpy as np
import pytest

import helpers as h
import raster_edge_scenes as es
from test_raster_gpu import _masked_grads, _run_autograd

pytestmark = pytest.mark.gpu

ROW_RTOL = {"dL_dmeans3D": 1e-5, "dL_dcov3D": 1e-5, "dL_dscales": 1e-5, "dL_drotations": 3e-5}      # _check_backward's: default, 3e-5 for rotations
GRADS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


def _forward(scene, cam, ref, tag):
    s = scene["scale_modifier"]
    fw = h.gpu_native_forward(scene, cam, scale_modifier=s)
    print(f"\n[parity] {tag}: scale_modifier {s:g}, P {ref['radii'].shape[0]}, drawn {int((ref['radii'] > 0).sum())}, instances {ref['num_rendered']}")
    h._bitexact(fw, ref)
    h.assert_image_parity(fw, ref)
    return fw


def _backward(scene, cam, ref, fw, tag, level2=True, row_sets=None):
    """Levels 1 and 2 of _check_backward with the scene's scale modifier.  ``row_sets``: {name: boolean rows} -- level 2 is asserted on each
    set separately (and then on all rows), so that a failure names the set.  Returns (GPU gradients, oracle preprocess backward or None)."""
    from oracle import raster_oracle as ro
    s = scene["scale_modifier"]
    grads = _masked_grads(scene, ref)
    nc = fw["n_contrib"] != ref["n_contrib"]
    assert not (nc & ~ref["fragile"].astype(bool)).any()
    # (1)
    acc_ref = ro.backward_blend(ref, scene["colors"], scene["bg"], grads["dL_dcolor"], grads["dL_ddepth"], grads["dL_dalpha"])
    got = h.gpu_native_backward(fw, grads, alphas=ref["alpha"], scale_modifier=s)
    worst = h.assert_accum_parity(got, acc_ref)
    print(f"[parity] {tag}: level 1, blend-backward accumulators: worst ratio to 1e-4 |ref| + 64 eps sum|term| = {worst:.2f} (bar 1)")
    for k in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity"):
        assert got[k].shape == acc_ref[k].shape
    vis = ref["radii"] > 0
    for k in GRADS:
        assert not got[k][~vis].any(), f"{k} must be zero for culled Gaussians"
    if not level2:
        return got, None
    # (2)
    pre = ro.backward_preprocess(ref, got, scene["means3D"], scene.get("scales"), scene.get("rotations"), cam["viewmatrix"],
                                 cam["projmatrix"], cam["tanfovx"], cam["tanfovy"], scale_modifier=s,
                                 cov3D_precomp=scene.get("cov3D_precomp"))
    names = ("dL_dmeans3D", "dL_dcov3D") + (("dL_dscales", "dL_drotations") if scene.get("scales") is not None else ())
    sets = dict(row_sets or {}, all=np.ones(len(vis), bool))
    for set_name, rows in sets.items():
        rows = rows & vis
        for k in names:        # not 0 == 0: the set has rows that receive a gradient (counted on the CPU too, test_raster_edges_cpu.py)
            assert (np.abs(pre[k][rows]).max(axis=1) > 0).sum() >= 20, (set_name, k)
            h.assert_rows_close(got[k][rows], pre[k][rows], f"{k} [{set_name} rows]", row_rtol=ROW_RTOL[k])
    print(f"[parity] {tag}: level 2, streaming backward within 1e-4 |ref| + row_rtol max|row| on {', '.join(f'{n} ({int((r & vis).sum())} rows)' for n, r in sets.items())}")
    return got, pre


@pytest.mark.parametrize("s", [0.5, 2.0])
def test_scale_modifier(s):
    scene, cam, ref, _ = es.scale_modifier_scene(s)
    fw = _forward(scene, cam, ref, f"scale modifier {s:g}")
    _backward(scene, cam, ref, fw, f"scale modifier {s:g}")
    # level 3's routing check: through GaussianRasterizer + autograd the modifier of the settings reaches both native calls
    grads = _masked_grads(scene, ref)
    own = h.gpu_native_backward(fw, grads, scale_modifier=s)
    e2e = _run_autograd(scene, cam, grads, scale_modifier=s)
    assert "dL_dscales" in e2e and np.abs(own["dL_dscales"]).max() > 0
    for k, v in e2e.items():   # a mis-wired gradient or a modifier left at 1 is off by O(1), atomic-order noise by ~1e-6
        np.testing.assert_allclose(v.reshape(own[k].shape), own[k], rtol=1e-3, atol=1e-4 * max(1.0, np.abs(own[k]).max()),
                                   err_msg="autograd " + k)


def test_scale_modifier_is_ignored_with_cov3d_precomp():
    """The modifier only ever multiplies scales: next to a precomputed covariance the whole forward state at modifier 2 is bit-identical to the
    one at modifier 1 (every sub-array of the scratch the forward writes, byte for byte), and the backward at either modifier meets levels 1 and 2 against the oracle.
    Gradient against gradient, bit for bit: the blend backward sums with float atomics, whose order is the waves' arrival order, so two
    backward calls are bit-identical only when no sum was reordered -- the same modifier is therefore run twice, the outcome is printed, and
    whenever that pair is bit-identical the pair of the two modifiers must be bit-identical too."""
    import torch
    scene, cam, ref, _ = es.scale_modifier_scene(2.0, True)
    fw2 = _forward(scene, cam, ref, "scale modifier 2 with cov3D_precomp")
    g2, _ = _backward(scene, cam, ref, fw2, "scale modifier 2 with cov3D_precomp")
    scene1 = dict(scene, scale_modifier=1.0)
    fw1 = h.gpu_native_forward(scene1, cam, scale_modifier=1.0)
    t1, t2 = fw1["_torch"], fw2["_torch"]
    assert fw1["num_rendered"] == fw2["num_rendered"]
    for k in ("radii", "alpha"):
        assert torch.equal(t1[k], t2[k]), f"forward {k} depends on the scale modifier next to cov3D_precomp"
    for k in ("color", "depth", "means2D", "conic_opacity", "depths", "r2cut", "cov3D", "tiles_touched", "ranges", "n_contrib", "tile_count",
              "point_list"):   # every sub-array the forward leaves defined (padding is uninitialised, the key scratch keeps the scatter's arrival order)
        assert fw1[k].tobytes() == fw2[k].tobytes(), f"forward {k} depends on the scale modifier next to cov3D_precomp"
    g1, _ = _backward(scene1, cam, ref, fw1, "scale modifier 1 with cov3D_precomp")
    g1b = h.gpu_native_backward(fw1, _masked_grads(scene, ref), alphas=ref["alpha"], scale_modifier=1.0)
    assert not g2["dL_dscales"].any() and not g2["dL_drotations"].any()
    repeatable = all(np.array_equal(g1[k], g1b[k]) for k in GRADS)
    identical = all(np.array_equal(g1[k], g2[k]) for k in GRADS)
    print(f"[parity] cov3D_precomp: gradients at modifier 1, two calls, bit-identical: {repeatable}; modifier 2 against modifier 1 bit-identical: {identical}")
    assert identical or not repeatable


def test_frustum_clamp():
    scene, cam, ref, _ = es.frustum_clamp_scene()
    fw = _forward(scene, cam, ref, "frustum clamp")
    cs = es.clamp_sets(scene, cam)
    sets = {"clamped in x only": cs["x_only"], "clamped in y only": cs["y_only"], "clamped in both": cs["both"], "unclamped": cs["none"]}
    got, pre = _backward(scene, cam, ref, fw, "frustum clamp", row_sets=sets)
    # Rows clamped in both axes: the J02 / J12 path into tx, ty is cut (x_grad_mul = y_grad_mul = 0), so what the conic gradient adds to
    # dL_dmeans3D is V^T (0, 0, dL_dtz): parallel to the view rotation's third row.  First on the oracle, with the conic gradient alone; then
    # on the GPU's dL_dmeans3D minus the oracle's mean2D and depth terms, at the row tolerance of level 2.
    from oracle import raster_oracle as ro
    vis = ref["radii"] > 0
    zero2, zero1 = np.zeros_like(got["dL_dmeans2D"]), np.zeros_like(got["dL_ddepths"])
    args = (scene["means3D"], scene["scales"], scene["rotations"], cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"], cam["tanfovy"])
    alone = ro.backward_preprocess(ref, {"dL_dmeans2D": zero2, "dL_dconic": got["dL_dconic"], "dL_ddepths": zero1}, *args,
                                   scale_modifier=scene["scale_modifier"])["dL_dmeans3D"].astype(np.float64)
    rest = ro.backward_preprocess(ref, {"dL_dmeans2D": got["dL_dmeans2D"], "dL_dconic": np.zeros_like(got["dL_dconic"]),
                                        "dL_ddepths": got["dL_ddepths"]}, *args,
                                  scale_modifier=scene["scale_modifier"])["dL_dmeans3D"].astype(np.float64)
    V = cam["viewmatrix"].astype(np.float64)
    axis = {"x": V[:3, 0], "y": V[:3, 1]}                     # d tx / d mean, d ty / d mean
    total = pre["dL_dmeans3D"].astype(np.float64)
    lim = (1e-4 * np.abs(total) + ROW_RTOL["dL_dmeans3D"] * np.abs(total).max(axis=1, keepdims=True) + 1e-9).sum(1)
    gpu_conic_part = got["dL_dmeans3D"].astype(np.float64) - rest
    big = np.abs(alone).max(axis=1)
    for ax, rows in (("x", cs["x"] & vis & (big > 0)), ("y", cs["y"] & vis & (big > 0))):     # (a drawn splat may reach no pixel with alpha >= 1/255)
        assert rows.sum() >= 50
        assert (np.abs(alone[rows] @ axis[ax]) <= 1e-6 * big[rows]).all(), f"oracle: conic gradient reaches t{ax} of a clamped row"
        worst = float((np.abs(gpu_conic_part[rows] @ axis[ax]) / lim[rows]).max())
        print(f"[parity] frustum clamp: rows clamped in {ax}, conic path into t{ax}: worst ratio to the level-2 row limit {worst:.2f} (bar 1)")
        assert worst <= 1.0, f"the conic gradient reaches t{ax} of rows clamped in {ax}"
    none = cs["none"] & vis
    for ax in ("x", "y"):         # ... and the path carries weight where nothing is clamped: it is far above that limit there
        assert (np.abs(alone[none] @ axis[ax]) > 10 * lim[none]).mean() > 0.5, ax


def test_near_plane():
    scene, cam, ref, _ = es.near_plane_scene()
    fw = _forward(scene, cam, ref, "near plane")                       # radii equality inside _bitexact is the cull test
    _backward(scene, cam, ref, fw, "near plane")
    drawn = ref["radii"] > 0
    lam = es.lambda1_f64(scene, cam, ref)
    op = scene["opacities"][:, 0]
    huge = drawn & (lam >= 1.0001 * es.LAMBDA_HUGE)
    ordinary = drawn & (lam <= 0.9999 * es.LAMBDA_HUGE) & (op > es.OP_MIN)
    assert huge.sum() >= 10 and ordinary.sum() >= 10
    assert (fw["r2cut"][huge] >= 3.0e38).all(), "a splat with lambda1 >= 1e4 must never be culled"
    assert np.isfinite(fw["r2cut"][ordinary]).all() and (fw["r2cut"][ordinary] < 3.0e38).all(), \
        "a splat with lambda1 < 1e4 and opacity above 1/255 carries a finite cull radius, not the never-culled mark"


def test_opacity_edges():
    scene, cam, ref, _ = es.opacity_edge_scene()
    fw = _forward(scene, cam, ref, "opacity edges")                    # n_contrib on all non-fragile pixels is part of the image parity
    got, _ = _backward(scene, cam, ref, fw, "opacity edges")
    drawn = ref["radii"] > 0
    op = scene["opacities"][:, 0]
    vals = es.opacity_edge_values()
    never = drawn & (op <= vals["below_1_255"])
    seen = drawn & (op >= np.float32(0.0041))
    assert never.sum() >= 150 and seen.sum() >= 150
    print(f"[parity] opacity edges: r2cut of the rows with op = 0 / 1e-3 / just below 1/255: "
          + " / ".join(f"{fw['r2cut'][drawn & (op == vals[k])].min():g} .. {fw['r2cut'][drawn & (op == vals[k])].max():g}" for k in ("zero", "1e-3", "below_1_255")))
    assert (fw["r2cut"][never] < 0).all(), "op < 1/255 never reaches alpha >= 1/255: culled everywhere"
    assert (fw["r2cut"][seen] > 0).all()
    zero = drawn & (op == 0)
    assert zero.sum() >= 50 and np.isfinite(got["dL_dopacity"][zero]).all()
    for k in GRADS:
        assert np.isfinite(got[k]).all(), k


def _check_tile_state(scene, cam, ref, fw):
    n = ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0].astype(np.int64)
    assert np.array_equal(fw["tile_count"].astype(np.int64), n), "per-tile instance counts differ from the oracle's range lengths"
    again = h.gpu_native_forward(scene, cam, scale_modifier=scene["scale_modifier"])
    assert np.array_equal(again["point_list"], fw["point_list"]) and np.array_equal(again["ranges"], fw["ranges"])
    assert np.array_equal(again["tile_count"], fw["tile_count"])


def test_incoherent_window():
    scene, cam, ref, _ = es.incoherent_window_scene()
    fw = _forward(scene, cam, ref, "incoherent window")
    _check_tile_state(scene, cam, ref, fw)
    _backward(scene, cam, ref, fw, "incoherent window")


def test_multipass_scan():
    scene, cam, ref, _ = es.multipass_scan_scene()
    fw = _forward(scene, cam, ref, "multi-pass scan")
    _check_tile_state(scene, cam, ref, fw)
    _backward(scene, cam, ref, fw, "multi-pass scan", level2=False)
