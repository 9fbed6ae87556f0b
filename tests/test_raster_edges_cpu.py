"""CPU checks of the edge scenes of tests/raster_edge_scenes.py (no GPU): every scene REACHES the path it is named after -- asserted on
the oracle's forward state, so that the GPU comparisons of tests/test_raster_edges_gpu.py cannot pass on a scene that has drifted off its
branch -- and stays within the fragile-pixel cap of ``helpers.assert_image_parity`` at its default.  Then the oracle itself on the paths
the scenes add: the ``scale_modifier`` identities, and the reference's own results at ``scale_modifier = 2`` on the clamp scene
(tests/golden/raster_edge_clamp_sm2.npz, made by tests/golden/make_golden.py from the reference's sources)."""
import inspect
import os

import numpy as np
import pytest

import helpers as h
import raster_edge_scenes as es
from oracle import raster_oracle as ro

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FRAGILE = inspect.signature(h.assert_image_parity).parameters["max_fragile_frac"].default


def _check_common(reach):
    print(f"\n[reach] {reach}")
    assert MAX_FRAGILE == 5e-3
    assert reach["fragile_frac"] <= MAX_FRAGILE, reach["fragile_frac"]
    assert reach["rects_match_tiles_touched"]            # the numpy getRect of the reach facts is the oracle's
    assert reach["fx_ne_fy"]
    assert reach["drawn"] > 0 and reach["num_rendered"] > 0


@pytest.mark.parametrize("s", [0.5, 2.0])
def test_scale_modifier_scene_reach(s):
    scene, cam, ref, reach = es.scale_modifier_scene(s)
    _check_common(reach)
    assert reach["P"] == 1500 and (cam["img_w"], cam["img_h"]) == (160, 112)
    assert reach["drawn"] >= 1400
    assert reach["radii_changed_frac"] >= 0.9 and not reach["state_equals_modifier_1"]     # the modifier is visible in nearly every radius


def test_scale_modifier_precomp_scene_reach():
    scene, cam, ref, reach = es.scale_modifier_scene(2.0, True)
    _check_common(reach)
    assert scene["scales"] is None and scene["rotations"] is None and scene["cov3D_precomp"].shape == (1500, 6)
    assert reach["state_equals_modifier_1"]              # the reference ignores the modifier next to a precomputed covariance


def test_frustum_clamp_scene_reach():
    scene, cam, ref, reach = es.frustum_clamp_scene()
    _check_common(reach)
    assert 1100 <= reach["P"] <= 1300
    assert reach["x_only_frac"] >= 0.05 and reach["y_only_frac"] >= 0.05 and reach["both_frac"] > 0.0
    assert reach["none_frac"] >= 0.30
    assert min(reach["x_pos"], reach["x_neg"], reach["y_pos"], reach["y_neg"]) >= 10     # both signs, on both axes
    assert reach["undecided"] == 0                       # no drawn Gaussian within 1e-5 of the limit: the row sets are unambiguous
    # wide splats: a nominal sigma (scale x |q|^2 x focal / depth) of 8-12 px; perspective (J's third column, up to 1.3 tanfov) stretches the
    # larger eigenvalue of the 2D covariance on top of that
    qq = (scene["rotations"].astype(np.float64) ** 2).sum(1, keepdims=True)
    focal = np.sqrt(float(scene["intr"][0, 0]) * float(scene["intr"][1, 1]))
    nominal = scene["scales"] * qq * focal / es.view_space(scene, cam)[:, 2:3]
    assert 7.0 <= nominal.min() and nominal.max() <= 12.5
    lam = es.lambda1_f64(scene, cam, ref)[ref["radii"] > 0]
    assert 6.0 <= np.sqrt(lam.min()) and np.sqrt(lam.max()) <= 25.0      # fx = 0.79, fy = 1.26 of the geometric-mean focal


def test_frustum_clamp_scene_clamped_rows_receive_gradients():
    """A clamped splat's centre is outside the image; the row sets of the GPU test compare gradients, so they must not be zero against zero."""
    from test_raster_gpu import _masked_grads
    scene, cam, ref, _ = es.frustum_clamp_scene()
    g = _masked_grads(scene, ref)
    acc = ro.backward_blend(ref, scene["colors"], scene["bg"], g["dL_dcolor"], g["dL_ddepth"], g["dL_dalpha"])
    cs, drawn = es.clamp_sets(scene, cam), ref["radii"] > 0
    live = {k: int((np.abs(acc["dL_dconic"][cs[k] & drawn]).max(axis=1) > 0).sum()) for k in ("x_only", "y_only", "both", "none")}
    print(f"\n[reach] rows with a conic gradient: {live}")
    assert live["x_only"] >= 50 and live["y_only"] >= 50 and live["both"] >= 20 and live["none"] >= 300


def test_near_plane_scene_reach():
    scene, cam, ref, reach = es.near_plane_scene()
    _check_common(reach)
    assert reach["tiles"] == 30 and reach["tiles_mod_4"] == 2
    assert reach["behind_near_plane"] >= 50 and reach["beyond_near_plane"] >= 50 and reach["culled_are_exactly_the_near_ones"]
    assert reach["drawn_within_0p05_of_plane"] >= 10
    assert reach["drawn_lambda_huge"] >= 10 and reach["drawn_lambda_ordinary"] >= 10
    assert reach["drawn_whole_grid"] >= 10
    assert reach["max_opacity"] <= 0.05 and reach["min_transmittance"] >= 0.05


def test_opacity_edge_scene_reach():
    scene, cam, ref, reach = es.opacity_edge_scene()
    _check_common(reach)
    vals = es.opacity_edge_values()
    assert vals["below_1_255"] < es.OP_MIN < vals["above_1_255"] and vals["zero"] == 0.0 and vals["one"] == 1.0
    for name in vals:
        assert reach["drawn_" + name] >= 50, name
    assert reach["drawn_lambda_huge"] == 0               # every r2cut of this scene comes from the log(255 op) branch


def test_incoherent_window_scene_reach():
    scene, cam, ref, reach = es.incoherent_window_scene()
    _check_common(reach)
    assert reach["P"] == 2048 and reach["tiles"] == 2303 and reach["tiles_mod_4"] == 3 and reach["tiles"] <= es.SCAN_PASS
    assert reach["window_blocks"] >= 2 and reach["fallback_blocks"] >= 2, reach["window_areas"]
    assert reach["common_tiles"] >= 1


def test_multipass_scan_scene_reach():
    scene, cam, ref, reach = es.multipass_scan_scene()
    _check_common(reach)
    assert reach["tiles"] == 4225 > es.SCAN_PASS and reach["tiles_mod_4"] == 1 and reach["tiles_in_last_pass"] == 129
    assert reach["nonempty_in_second_pass"] >= 10 and reach["last_tile_len"] >= 1
    assert reach["empty_in_first_pass"] >= 10 and reach["empty_in_second_pass"] >= 1 and reach["nonempty_in_first_pass"] >= 1000


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("s", [0.5, 2.0])
def test_oracle_scale_modifier_equals_scaled_scales(s):
    """Forward at ``scale_modifier = s`` on scales v == forward at modifier 1 on the fp32 products s * v, bit for bit (s a power of two: the
    product the kernel forms is exact), and so is every output of ``backward_preprocess``.  dL_dscales INCLUDED, with factor 1: the reference
    differentiates with respect to the MODIFIED scale s * v and never applies the chain-rule factor s (backward.cu computeCov3D: ``s = mod *
    scale`` enters M = S R, dL_dscale = dot(Rt, dL_dMt) is written as is) -- so a backward that multiplied by s again, or dropped s from M,
    breaks this identity by a factor of s or s^2."""
    scene, cam, ref, _ = es.scale_modifier_scene(s)
    scaled = dict(scene, scales=(np.float32(s) * scene["scales"]).astype(np.float32))
    assert np.array_equal(scaled["scales"].astype(np.float64), s * scene["scales"].astype(np.float64))      # exact products
    one = h.oracle_forward(scaled, cam)
    for k in ("radii", "tiles_touched", "point_list", "ranges", "n_contrib"):
        assert np.array_equal(ref[k], one[k]), k
    for k in ("conic_opacity", "cov3D", "means2D", "depths", "color", "depth", "alpha"):
        assert np.array_equal(_bits(ref[k]), _bits(one[k])), k
    grads = {k: scene[k] for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha")}
    acc = ro.backward_blend(ref, scene["colors"], scene["bg"], grads["dL_dcolor"], grads["dL_ddepth"], grads["dL_dalpha"])
    args = (cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"], cam["tanfovy"])
    g_s = ro.backward_preprocess(ref, acc, scene["means3D"], scene["scales"], scene["rotations"], *args, scale_modifier=s)
    g_1 = ro.backward_preprocess(one, acc, scene["means3D"], scaled["scales"], scene["rotations"], *args, scale_modifier=1.0)
    for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"):
        assert np.abs(g_s[k]).max() > 0, k
        assert np.array_equal(_bits(g_s[k]), _bits(g_1[k])), k
    # ... and the modifier is not a no-op in the backward: the same call at modifier 1 on the unscaled scales differs
    g_0 = ro.backward_preprocess(ref, acc, scene["means3D"], scene["scales"], scene["rotations"], *args, scale_modifier=1.0)
    big = np.abs(g_s["dL_dscales"]) > 1e-3 * np.abs(g_s["dL_dscales"]).max()
    ratio = g_s["dL_dscales"][big].astype(np.float64) / g_0["dL_dscales"][big]
    np.testing.assert_allclose(ratio, s, rtol=1e-4)      # dL/d(s v) is linear in M = diag(s v) R for a fixed dL/dSigma


def test_oracle_ignores_the_modifier_with_a_precomputed_covariance():
    scene, cam, ref, _ = es.scale_modifier_scene(2.0, True)
    one = h.oracle_forward(scene, cam)
    for k in ("radii", "conic_opacity", "means2D", "point_list", "ranges", "color", "alpha", "n_contrib"):
        assert np.array_equal(ref[k], one[k]), k
    grads = {k: scene[k] for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha")}
    g2 = h.oracle_backward(ref, scene, cam, grads, scale_modifier=2.0)
    g1 = h.oracle_backward(ref, scene, cam, grads)
    for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dopacity", "dL_dcolors"):
        assert np.array_equal(_bits(g2[k]), _bits(g1[k])), k
    assert not g2["dL_dscales"].any() and not g2["dL_drotations"].any()


def test_oracle_matches_the_reference_at_scale_modifier_2_on_the_clamp_scene():
    """tests/golden/raster_edge_clamp_sm2.npz: the reference's own code on ``frustum_clamp_scene`` at modifier 2.  Forward state bit for bit;
    the preprocess backward (frustum clamp with its zeroed gradient factors, both focal lengths, the scale-modifier chain) bit for bit on the
    reference's own accumulators.  The blend backward's accumulators are fp32 sums in the order of the reference's atomics, which the oracle
    reproduces only up to one 256-entry batch per tile (test_oracle_cpu.py); this scene's lists are longer, so they are compared through
    ``assert_accum_parity`` at its defaults against the oracle's float64 sums."""
    z = np.load(os.path.join(GOLD, "raster_edge_clamp_sm2.npz"))
    s = float(z["scale_modifier"][0])
    assert s == 2.0
    scene, cam, ref, reach = es.frustum_clamp_scene(s)
    for k in ("means3D", "scales", "rotations", "opacities", "colors", "bg", "dL_dcolor", "dL_ddepth", "dL_dalpha"):
        assert h.bits_digest(scene[k]) == str(z["digest_in_" + k]), f"the seeded scene no longer is what the fixture was made from: {k}"
    assert reach["x_only_frac"] >= 0.05 and reach["y_only_frac"] >= 0.05 and reach["both_frac"] > 0.0 and reach["none_frac"] >= 0.30
    assert ref["num_rendered"] == int(z["st_num_rendered"][0])
    vis = z["st_radii"] > 0
    for k in ("radii", "tiles_touched"):
        assert np.array_equal(ref[k], z["st_" + k]), k
    for k in ("depths", "means2D", "cov3D", "conic_opacity"):
        assert np.array_equal(_bits(ref[k][vis]), _bits(z["st_" + k][vis])), k
    for k in ("point_list", "ranges", "n_contrib", "color", "depth", "alpha"):
        assert h.bits_digest(ref[k]) == str(z["digest_st_" + k]), k
    g_ref = {k[2:]: z[k] for k in z.files if k.startswith("g_")}
    pre = ro.backward_preprocess(ref, g_ref, scene["means3D"], scene["scales"], scene["rotations"], cam["viewmatrix"], cam["projmatrix"],
                                 cam["tanfovx"], cam["tanfovy"], scale_modifier=s)
    for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"):
        assert np.abs(g_ref[k]).max() > 0 and not g_ref[k][~vis].any(), k
        assert np.array_equal(_bits(pre[k]), _bits(g_ref[k])), k
    acc = ro.backward_blend(ref, scene["colors"], scene["bg"], scene["dL_dcolor"], scene["dL_ddepth"], scene["dL_dalpha"])
    h.assert_accum_parity(g_ref, acc)
