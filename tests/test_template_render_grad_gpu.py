"""The template renderer's reverse pass on the GPU (``include/ag_ray_march_grad.h``; ``composite_backward``, the autograd of ``composite``,
``laplace_density``, ``render_train`` / ``training_loss`` of ``template_render.py``) against ``template_render_grad_oracle.py``.

The bar is the project's, per output array, maxima over the whole array, no element left out:

    |gpu - float64 oracle| <= 4 x max|float32 oracle - float64 oracle| + 2^-22 x max|float64 oracle|

with torch autograd of the reference's text in float64 as the float64 oracle and the header's recurrence (closed forms for the
density), evaluated element by element in float32, as the float32 oracle.  ``grad_beta``, one number: 4 x own + 8 x 2^-24 x sum|terms|,
``own`` the float32 terms summed exactly -- the six-level float32 butterfly is the only float32 summation of the kernel.
``training_loss``, one number, a mean of |map - target|: no further from the float64 chain than its two maps' bars weighted as the
loss weighs them, plus 2^-22 of the loss for the means' own rounding.  Every test prints the measured deviation and its bar.

Measured on the MI355X ("Template render backward"): ``grad_density`` at most 0.28 of its bar over the 44 cases (2.2e-6 /
1.27e-5 at R = 257, S = 64), ``grad_color`` 0.21 and equal to weights x G_rgb bit for bit; ``grad_sdf`` at most 0.17, ``grad_beta`` 0.06;
``render_train``: the maps 0.27, the parameters' gradients 0.45 .. 0.87 of the bar at R = 5 and at most 0.05 at R = 70, ``beta`` 0.25 / 0.01;
36 tests in 4.4 s.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_oracle as tfo  # noqa: E402
import template_render_grad_oracle as tgo  # noqa: E402
import template_render_oracle as tro  # noqa: E402

pytestmark = pytest.mark.gpu
MAPS = ("rgb_map", "acc_map", "depth_map", "disp_map", "weights")


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bar(name, got, w64, w32):
    g = got.detach().cpu().numpy().astype(np.float64) if hasattr(got, "detach") else np.asarray(got, np.float64)
    w64, w32 = np.asarray(w64, np.float64), np.asarray(w32, np.float64)
    assert g.shape == w64.shape, (name, g.shape, w64.shape)
    own = float(np.abs(w32 - w64).max())
    bar = 4 * own + 2.0 ** -22 * float(np.abs(w64).max())
    dev = float(np.abs(g - w64).max())
    print(f"{name}: |gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
    assert np.isfinite(g).all(), f"{name}: not finite"
    assert dev <= bar, f"{name}: {dev:.3e} > {bar:.3e}"
    return bar


# ---- composite_backward -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(R, S):
    """Inputs, upstream gradients and both oracles for both backgrounds -- built once, never modified."""
    density, color, z = tro.composite_case(R, S, seed=100 * S + R)
    G = tgo.upstream(R, S, seed=S + R)
    out = dict(density=density, color=color, z=z, G=G)
    for white in (False, True):
        out[white] = (tgo.composite_autograd(density, color, z, G, white), tgo.composite_recurrence(density, color, z, G, white, np.float32)[:2])
    for a in (density, color, z) + tuple(G.values()) + tuple(v for w in (False, True) for o in out[w] for v in o):
        a.setflags(write=False)
    return out


SHAPES = [(R, S) for S in (2, 3, 63, 64, 65, 128, 130) for R in (1, 3, 257)] + [(3, 1024)]


@pytest.mark.parametrize("R,S", SHAPES)
def test_composite_backward_against_the_float64_oracle(R, S):
    import torch
    from animatablegaussians_amd.template_render import composite, composite_backward
    c = _case(R, S)
    density, color, z = _t(c["density"]), _t(c["color"]), _t(c["z"])
    G = {k: _t(v) for k, v in c["G"].items()}
    zeros = {k: torch.zeros_like(v) for k, v in G.items()}
    weights = composite(density, color, z, want=("weights",))["weights"]
    for white in (False, True):
        (d64, c64), (d32, c32) = c[white]
        got = composite_backward(density, color, z, G, white)
        assert set(got) == {"density", "color"} and got["density"].shape == (R, S) and got["color"].shape == (R, S, 3)
        assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in got.values())
        _bar(f"R = {R}, S = {S}, white {white}: grad_density", got["density"], d64, d32)
        _bar(f"R = {R}, S = {S}, white {white}: grad_color", got["color"], c64, c32)
        assert np.array_equal(_bits(got["color"]), _bits(weights[..., None] * G["rgb_map"][:, None, :])), "grad_color is not the forward's weights x G_rgb"
        again = composite_backward(density, color, z, G, white)
        assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in got), "two calls differ"
        # a ray's gradients depend on that ray alone
        cut = lambda a, b: composite_backward(density[a:b], color[a:b], z[a:b], {k: v[a:b] for k, v in G.items()}, white)  # noqa: E731
        halves, singles = [cut(0, R // 2), cut(R // 2, R)], [cut(r, r + 1) for r in range(R)]
        for k in got:
            assert np.array_equal(_bits(torch.cat([h[k] for h in halves])), _bits(got[k])), f"{k}: two halves differ from one call"
            assert np.array_equal(_bits(torch.cat([s[k] for s in singles])), _bits(got[k])), f"{k}: one ray at a time differs from one call"
        # a gradient given alone is the same call with zeros for the others
        for name in tgo.GRADS:
            alone = composite_backward(density, color, z, {name: G[name]}, white)
            padded = composite_backward(density, color, z, {**zeros, name: G[name]}, white)
            assert np.array_equal(_bits(alone["density"]), _bits(padded["density"])), f"{name} alone differs from {name} with zeros"
            assert np.isfinite(alone["density"].cpu().numpy()).all()
            if name == "rgb_map":
                assert np.array_equal(_bits(alone["color"]), _bits(got["color"]))
            else:
                assert alone["color"] is None and not padded["color"].any()
    # the field's shapes are taken as they are; no upstream gradient at all gives zeros
    flat = composite_backward(density.reshape(-1, 1), color.reshape(-1, 3), z, G, True)
    assert all(np.array_equal(_bits(flat[k]), _bits(got[k])) for k in got)
    none = composite_backward(density, color, z, {})
    assert none["color"] is None and none["density"].shape == (R, S) and not _bits(none["density"]).any()
    no_color = composite_backward(density, None, z, {k: G[k] for k in ("acc_map", "depth_map")})
    with_color = composite_backward(density, color, z, {k: G[k] for k in ("acc_map", "depth_map")})
    assert no_color["color"] is None and np.array_equal(_bits(no_color["density"]), _bits(with_color["density"]))


def test_a_ray_of_zero_density_and_saturated_rays():
    from animatablegaussians_amd.template_render import composite_backward
    R, S = 3, 65
    c = _case(R, S)
    density = np.array(c["density"])
    density[1] = 0.0
    G = c["G"]
    d64, c64 = tgo.composite_autograd(density, c["color"], c["z"], G, True)
    d32, c32 = tgo.composite_recurrence(density, c["color"], c["z"], G, True, np.float32)[:2]
    got = composite_backward(_t(density), _t(c["color"]), _t(c["z"]), {k: _t(v) for k, v in G.items()}, True)
    _bar("zero-density ray: grad_density", got["density"], d64, d32)
    _bar("zero-density ray: grad_color", got["color"], c64, c32)
    assert not _bits(got["color"][1]).any() and got["density"][1].abs().max() > 0, "the empty ray's density gradient is dist x g, not 0"
    # the large scene holds saturated samples (alpha = 1 in float32): the gradient there is finite
    big = _case(257, 64)
    alpha = tgo.composite_recurrence(big["density"], big["color"], big["z"], {}, False, np.float32)[3]
    assert (alpha == 1).sum() >= 1


def test_composite_backward_refusals_and_empty_ray_sets():
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.template_render import composite_backward
    dens, col, z = torch.rand(10, 8, device="cuda"), torch.rand(10, 8, 3, device="cuda"), torch.rand(10, 8, device="cuda").cumsum(1)
    g = {"acc_map": torch.rand(10, device="cuda")}
    bad = [
        lambda: composite_backward(dens[:, :1], col[:, :1], z[:, :1], g), lambda: composite_backward(dens.cpu(), col, z, g),
        lambda: composite_backward(torch.rand(2, 1025, device="cuda"), None, torch.rand(2, 1025, device="cuda"), {"acc_map": torch.rand(2, device="cuda")}),
        lambda: composite_backward(dens, col, z, {"acc_map": torch.rand(9, device="cuda")}), lambda: composite_backward(dens, col, z, {"disp_map": g["acc_map"]}),
        lambda: composite_backward(dens, None, z, {"rgb_map": torch.rand(10, 3, device="cuda")}), lambda: composite_backward(dens, col, z, {"acc_map": g["acc_map"].double()}),
        lambda: composite_backward(dens, col[..., :2], z, g), lambda: composite_backward(dens[:, :7], col, z, g), lambda: composite_backward(dens, col, z, None),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the ABI names what it refuses, before it looks at a pointer
    L, null = _lib.lib(), ctypes.c_void_p(None)
    p = ctypes.c_void_p(dens.data_ptr())
    for S in (1, 1025):
        assert L.ag_ray_composite_backward(p, null, p, 4, S, 0, null, p, null, null, p, null, null) != 0 and b"S = " in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, p, p, 4, 8, 0, null, p, null, null, p, null, null) != 0 and b"color and g_rgb_map" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, p, p, null, null, p, null, null) != 0 and b"color and g_rgb_map" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, null, p, null, null, p, p, null) != 0 and b"grad_color" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, null, p, null, null, null, null, null) != 0 and b"grad_density" in L.ag_last_error()
    e = composite_backward(torch.empty((0, 8), device="cuda"), torch.empty((0, 8, 3), device="cuda"), torch.empty((0, 8), device="cuda"),
                           {"rgb_map": torch.empty((0, 3), device="cuda")})
    assert e["density"].shape == (0, 8) and e["color"].shape == (0, 8, 3)
    torch.cuda.synchronize()


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(3, 65), (257, 64)])
def test_autograd_through_composite_is_composite_backward(R, S):
    import torch
    from animatablegaussians_amd.template_render import composite, composite_backward
    c = _case(R, S)
    G = {k: _t(v) for k, v in c["G"].items()}
    z = _t(c["z"])
    plain = composite(_t(c["density"]), _t(c["color"]), z, True, want=MAPS)
    density, color = _t(c["density"]).requires_grad_(True), _t(c["color"]).requires_grad_(True)
    out = composite(density, color, z, True, want=MAPS)
    assert set(out) == set(MAPS) and all(np.array_equal(_bits(out[k]), _bits(plain[k])) for k in ("rgb_map", "acc_map", "depth_map", "weights"))
    assert np.array_equal(_bits(out["disp_map"]), _bits(plain["disp_map"]))          # NaN of an empty ray included: the bits are compared
    assert all(out[k].requires_grad for k in tgo.GRADS) and not out["disp_map"].requires_grad
    gd, gc = torch.autograd.grad(sum((out[k] * G[k]).sum() for k in tgo.GRADS), (density, color))
    want = composite_backward(density, color, z, G, True)
    assert np.array_equal(_bits(gd), _bits(want["density"])) and np.array_equal(_bits(gc), _bits(want["color"])), "autograd differs from composite_backward"
    # one map, the field's flat shapes, colour without grad
    flat_d = _t(c["density"]).reshape(-1, 1).requires_grad_(True)
    acc = composite(flat_d, _t(c["color"]).reshape(-1, 3), z, want=("acc_map",))
    assert set(acc) == {"acc_map"}
    (g_flat,) = torch.autograd.grad((acc["acc_map"] * G["acc_map"]).sum(), (flat_d,))
    alone = composite_backward(density, None, z, {"acc_map": G["acc_map"]})
    assert g_flat.shape == flat_d.shape and np.array_equal(_bits(g_flat.view(R, S)), _bits(alone["density"]))
    # .backward() accumulates into .grad; a second graph gives the same bits
    out2 = composite(density, color, z, True, want=("rgb_map", "acc_map"))
    (out2["rgb_map"] * G["rgb_map"]).sum().backward()
    only_rgb = composite_backward(density, color, z, {"rgb_map": G["rgb_map"]}, True)
    assert np.array_equal(_bits(density.grad), _bits(only_rgb["density"])) and np.array_equal(_bits(color.grad), _bits(only_rgb["color"]))
    # without grad mode: today's launches and today's bits, whatever the inputs require
    with torch.no_grad():
        quiet = composite(density, color, z, True, want=MAPS)
        assert not any(v.requires_grad for v in quiet.values()) and all(np.array_equal(_bits(quiet[k]), _bits(plain[k])) for k in MAPS)
        composite(density, color, z.clone().requires_grad_(True))                    # nothing is recorded: nothing to refuse
    with pytest.raises(ValueError, match="z_vals requires grad"):
        composite(density, color, z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="z_vals requires grad"):
        composite(_t(c["density"]), _t(c["color"]), z.clone().requires_grad_(True))


# ---- laplace_density --------------------------------------------------------------------------------------------------------------------
def test_laplace_density_equals_the_fused_fields_bit_for_bit():
    import torch
    from animatablegaussians_amd.template_field import TemplateField
    from animatablegaussians_amd.template_render import laplace_density
    for beta in (0.01, -0.02):
        net = tfo.make_net(tfo.NARROW, 4, density_beta=beta)
        arch = net["arch"]
        field = TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=net["use_viewdir"],
                                              multires_viewdir=arch["multires_viewdir"], geo_activation=net["geo_activation"])
        ret = field(_t(tfo.box_points(4099, 5)), want=("sdf", "density"))
        assert ret["sdf"].shape == (4099, 1) and float(ret["density"].max()) > 10 and float(ret["density"].min()) < 1
        by_tensor = laplace_density(ret["sdf"], torch.tensor([beta], device="cuda"))
        by_float = laplace_density(ret["sdf"], beta)
        assert by_tensor.shape == ret["sdf"].shape and not by_tensor.requires_grad
        assert np.array_equal(_bits(by_tensor), _bits(ret["density"])) and np.array_equal(_bits(by_float), _bits(ret["density"]))
    assert laplace_density(torch.empty((0, 1), device="cuda"), 0.01).shape == (0, 1)
    for bad in (lambda: laplace_density(ret["sdf"].double(), 0.01), lambda: laplace_density(ret["sdf"], torch.tensor([0.01, 0.02], device="cuda")),
                lambda: laplace_density(ret["sdf"], torch.tensor([0.01])), lambda: laplace_density(ret["sdf"].cpu(), 0.01)):
        with pytest.raises(ValueError):
            bad()


# 1 .. 4099: one lane, a group's edge, several groups, several wavefronts (512 elements each); 70001: 137 partials, runs of 3 in the fold
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4099, 70001])
def test_laplace_density_backward(N):
    import torch
    from animatablegaussians_amd.template_render import laplace_density
    sdf, g = tgo.sdf_case(N, seed=N)
    for beta in (0.01, -0.01, 0.0) if N in (257, 4099) else (0.01,):
        d64, gs64, gb64 = tgo.laplace_autograd(sdf, beta, g)
        d32, gs32, t32 = tgo.laplace_closed(sdf, beta, g, np.float32)
        t64 = tgo.laplace_closed(sdf, beta, g, np.float64)[2]
        s, bt = _t(sdf).requires_grad_(True), torch.tensor([beta], device="cuda", requires_grad=True)
        dens = laplace_density(s, bt)
        gs, gb = torch.autograd.grad(dens, (s, bt), _t(g))
        assert gs.shape == (N,) and gb.shape == (1,)
        _bar(f"N = {N}, beta = {beta}: density", dens, d64, d32)
        _bar(f"N = {N}, beta = {beta}: grad_sdf", gs, gs64, gs32)
        assert not gs.cpu().numpy()[sdf == 0].any(), "the gradient at sdf == 0 is not 0"
        own = abs(float(np.sign(np.float32(beta))) * float(t32.astype(np.float64).sum()) - gb64)
        bar = 4 * own + 8 * 2.0 ** -24 * float(np.abs(t64).sum())
        dev = abs(float(gb) - gb64)
        print(f"N = {N}, beta = {beta}: grad_beta {float(gb):.9e}, float64 oracle {gb64:.9e}: deviation {dev:.3e}, own {own:.3e}, bar {bar:.3e}")
        assert np.isfinite(float(gb)) and dev <= bar
        if beta == 0.0:
            assert float(gb) == 0.0
        gs2, gb2 = torch.autograd.grad(laplace_density(s, bt), (s, bt), _t(g))
        assert np.array_equal(_bits(gs2), _bits(gs)) and np.array_equal(_bits(gb2), _bits(gb)), "two calls differ"
        # one gradient at a time; a float beta takes none
        (only_s,) = torch.autograd.grad(laplace_density(s, beta), (s,), _t(g))
        (only_b,) = torch.autograd.grad(laplace_density(_t(sdf), bt), (bt,), _t(g))
        assert np.array_equal(_bits(only_s), _bits(gs)) and np.array_equal(_bits(only_b), _bits(gb))
    if N == 1:                                      # N = 0: grad_beta = 0
        s0, bt = torch.empty(0, device="cuda", requires_grad=True), torch.tensor([0.01], device="cuda", requires_grad=True)
        gs0, gb0 = torch.autograd.grad(laplace_density(s0, bt), (s0, bt), torch.empty(0, device="cuda"))
        assert gs0.shape == (0,) and float(gb0) == 0.0


# ---- render_train -----------------------------------------------------------------------------------------------------------------------
WEIGHTS = {"color": 1.0, "mask": 0.5}


@functools.lru_cache(maxsize=None)
def _train_case(R):
    """Rays, random numbers, targets and the host chain in both precisions -- built once, never modified."""
    import torch
    S, rs = 64, np.random.RandomState(R)
    o, d, near, far = tro.ray_scene(R, seed=R)
    u = rs.uniform(0, 1, (R, S)).astype(np.float32)
    noise = (0.1 * rs.normal(size=(R * S, 3))).astype(np.float32)
    mask = np.ones(R + 2 + R // 4, bool)
    mask[[1, 3] + list(range(5, 5 + 2 * (R // 4), 2))] = False                         # holes
    assert mask.sum() == R
    color_gt, mask_gt = rs.uniform(0, 1, (len(mask), 3)).astype(np.float32), (rs.uniform(0, 1, len(mask)) < 0.5).astype(np.float32)
    z, pts = tro.sample(o, d, near, far, S, u)
    net = tgo.tiny_net(seed=R)
    chains = [tgo.train_chain(net, 0.01, pts, z, d, noise, mask, color_gt, mask_gt, WEIGHTS, False, dt) for dt in (torch.float64, torch.float32)]
    return dict(o=o, d=d, near=near, far=far, u=u, noise=noise, mask=mask, color_gt=color_gt, mask_gt=mask_gt, z=z, pts=pts, net=net, chains=chains)


@pytest.mark.parametrize("R", [5, 70])
def test_render_train_end_to_end(R):
    import torch
    from animatablegaussians_amd.template_render import render_train, training_loss
    c = _train_case(R)
    (loss64, g64, m64), (loss32, g32, m32) = c["chains"]
    acc = m64["acc_map"][c["mask"]]
    print(f"R = {R}: acc_map {acc.min():.3f} .. {acc.max():.3f}, loss {loss64:.6f}")
    assert acc.max() > 0.9 and acc.min() < 0.5, "the scene's rays do not span opaque and (nearly) empty"
    params = {k: _t(v).requires_grad_(True) for k, v in c["net"].items()}
    beta = torch.tensor([0.01], device="cuda", requires_grad=True)
    args = (lambda p, v: tgo.tiny_field(params, p, v), beta, _t(c["o"]), _t(c["d"]), _t(c["near"]), _t(c["far"]))
    kw = dict(space="cano", sampling="uniform", u=_t(c["u"]), dir_noise=_t(c["noise"]), mask_within_patch=_t(c["mask"]))
    out = render_train(*args, **kw)
    assert np.array_equal(_bits(out["z_vals"]), _bits(c["z"])) and np.array_equal(_bits(out["cano_pts"]), _bits(c["pts"].reshape(-1, 3)))
    assert out["rgb_map"].shape == (len(c["mask"]), 3) and out["acc_map"].shape == (len(c["mask"]),) and not out["cano_pts"].requires_grad
    hole = ~c["mask"]
    assert not out["rgb_map"].detach().cpu().numpy()[hole].any() and not out["acc_map"].detach().cpu().numpy()[hole].any()
    bars = {k: _bar(f"R = {R}: {k}", out[k], m64[k], m32[k]) for k in ("rgb_map", "acc_map")}
    loss, terms = training_loss(out, _t(c["color_gt"]), _t(c["mask_gt"]), WEIGHTS)
    assert set(terms) == {"color_loss", "mask_loss"}
    by_hand = WEIGHTS["color"] * float(terms["color_loss"].detach()) + WEIGHTS["mask"] * float(terms["mask_loss"].detach())
    loss_bar = WEIGHTS["color"] * bars["rgb_map"] + WEIGHTS["mask"] * bars["acc_map"] + 2.0 ** -22 * abs(loss64)
    print(f"R = {R}: training_loss {float(loss.detach()):.9f}, float64 chain {loss64:.9f}, float32 chain {loss32:.9f}, bar {loss_bar:.3e}")
    assert abs(float(loss.detach()) - loss64) <= loss_bar and abs(by_hand - float(loss.detach())) <= 2.0 ** -22 * abs(loss64)
    names = list(params)
    grads = torch.autograd.grad(loss, [params[k] for k in names] + [beta])
    for k, g in zip(names + ["beta"], grads):
        assert g.shape == (params[k].shape if k != "beta" else (1,))
        _bar(f"R = {R}: d loss / d {k}", g.reshape(g64[k].shape), g64[k], g32[k])
        assert float(g.abs().max()) > 0
    # without grad mode the same bits; chunks of rays meet the same bar (the torch field's own kernels may round differently for another
    # batch size, so the bits are not compared); without the random numbers nothing is perturbed
    with torch.no_grad():
        whole = render_train(*args, **kw)
        assert all(np.array_equal(_bits(whole[k]), _bits(out[k])) and not whole[k].requires_grad for k in ("rgb_map", "acc_map"))
        chunked = render_train(*args, chunk_size=3, **kw)
        for k in ("rgb_map", "acc_map"):
            _bar(f"R = {R}, chunks of 3 rays: {k}", chunked[k], m64[k], m32[k])
        assert np.array_equal(_bits(chunked["z_vals"]), _bits(c["z"])) and np.array_equal(_bits(chunked["cano_pts"]), _bits(c["pts"].reshape(-1, 3)))
        calm = render_train(*args, space="cano", sampling="uniform", want=("acc_map", "weights"))
        assert set(calm) == {"acc_map", "weights", "cano_pts", "z_vals", "mask_within_patch"} and calm["weights"].shape == (R, 64)
        assert np.array_equal(_bits(calm["z_vals"]), _bits(tro.sample(c["o"], c["d"], c["near"], c["far"], 64)[0]))
    for bad in (lambda: render_train(*args, hands={}, **kw), lambda: render_train(*args, **{**kw, "dir_noise": kw["dir_noise"][:-1]}),
                lambda: render_train(*args, **{**kw, "mask_within_patch": kw["mask_within_patch"][:-1]}),
                lambda: render_train(None, *args[1:], **kw)):
        with pytest.raises(ValueError):
            bad()
