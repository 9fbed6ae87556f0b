"""The template renderer's kernels (``include/ag_ray_march.h``, ``template_render.py``) against ``template_render_oracle.py`` and the
reference's recorded outputs (``tests/golden/template_render_ref.npz``).

* near / far: bit-equal to the oracle's float32 restatement (minimum and maximum are exact, so no summation order enters).  The
  reference's kernel is CUDA and was never run: the oracle restates the header's formulas.
* sampling: ``z_vals`` / ``pts`` bit-equal to what the reference's ``sample_pts_on_rays`` gave in float32, unperturbed and with the stored
  ``u``.  The fixture holds 19 rays; a ray set of 257 is those rays repeated (ray i = fixture ray i mod 19: 19 divides neither a
  wavefront nor a workgroup, so a row that lands one wavefront or one workgroup away is a different ray).
* compositing and the rendered maps: |gpu - float64 oracle| <= 4 x max|float32 oracle - float64 oracle| + 2^-22 x max|float64 oracle|, the
  form and factor of ``test_template_field_gpu.py`` / ``test_isosurface_gpu.py``, maxima over the case's whole ray set: the kernel's scan
  and butterfly order and the device's ``expf`` are different from, and as valid as, ``torch.cumprod`` / ``torch.sum`` / ``torch.exp``.
  ``disp_map`` is 0 / 0 = NaN for a ray with ``acc = 0`` in the reference and here; it is compared on the rays whose float64 ``acc``
  exceeds 1e-6, and must be NaN exactly where the kernel's own ``acc`` is 0.
Every test prints the measured deviation and its bar.

Measured on the MI355X (DESIGN.md's "Template render" section has every figure): near / far 0 differing rays in all 23 cases; samples 0
differing elements, view directions at most 1 ulp; composite at S = 65, R = 257 deviation / bar: rgb 2.8e-7 / 1.12e-6, acc 2.9e-7 / 1.20e-6,
depth 6.9e-7 / 3.02e-6, disp 4.8e-4 / 2.50e-3, weights 1.4e-7 / 6.5e-7, at most 0.5 of the bar over the 15 shapes; render, uniform: rgb
9.7e-7 / 5.2e-6, acc 1.8e-6 / 9.7e-6, depth 4.0e-6 / 2.1e-5; smpl: 1.1e-6 / 4.4e-6, 2.2e-6 / 8.0e-6, 4.7e-6 / 1.9e-5; 54 tests in under 5 s.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_oracle as tfo  # noqa: E402
import template_render_oracle as tro  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "template_render_ref.npz")
MAPS = ("rgb_map", "acc_map", "depth_map", "disp_map", "weights")


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a) and set(a) == set(b)


def _field(net):
    from animatablegaussians_amd.template_field import TemplateField
    arch = net["arch"]
    return TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=net["use_viewdir"],
                                         multires_viewdir=arch["multires_viewdir"], geo_activation=net["geo_activation"])


def _compare(name, got, o64, o32, keys):
    """The bar of the module docstring for every map of ``keys``."""
    for k in keys:
        w64, w32 = o64[k], o32[k].astype(np.float64)
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert g.shape == w64.shape, (k, g.shape, w64.shape)
        on = np.ones(w64.shape, bool)
        if k == "disp_map":
            on = o64["acc_map"] > 1e-6
            acc0 = got["acc_map"].detach().cpu().numpy() == 0
            assert np.array_equal(np.isnan(g), acc0), f"{name}: disp_map is not NaN exactly where acc_map is 0"
        own = float(np.abs(w32 - w64)[on].max())
        bar = 4 * own + 2.0 ** -22 * float(np.abs(w64[on]).max())
        dev = float(np.abs(g - w64)[on].max())
        print(f"{name} {k}: |gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
        assert np.isfinite(g[on]).all() and dev <= bar, f"{name} {k}: {dev:.3e} > {bar:.3e}"


# ---- near / far ---------------------------------------------------------------------------------------------------------------------------
SCENE_RAYS = 1031          # larger ray sets repeat a scene of this many rays (the scene builder walks its rays one by one)


@functools.lru_cache(maxsize=None)
def _near_far_case(V, R):
    """Inputs and the float32 oracle's outputs with and without fallback -- built once, never modified."""
    n = min(R, SCENE_RAYS)
    vertices, o, d, fallback = tro.near_far_scene(V, n, seed=7 * V + R)
    with_fb = tro.near_far(vertices, o, d, 0.1, fallback, np.float32)
    without = tro.near_far(vertices, o, d, 0.1, None, np.float32)
    census = tro.near_far_census(*with_fb)
    idx = np.arange(R) % n
    out = dict(vertices=vertices, o=o[idx], d=d[idx], fallback=(fallback[0][idx], fallback[1][idx]), census=census,
               with_fb=tuple(a[idx] for a in with_fb[:3]), without=tuple(a[idx] for a in without[:3]))
    for a in (out["vertices"], out["o"], out["d"]) + out["fallback"] + out["with_fb"] + out["without"]:
        a.setflags(write=False)
    return out


# V x R of the lane-group split G = 64; the body's 10 475 vertices (11 LDS tiles, the last one partial) with a training step's 1024 rays;
# and the other splits: 8193 rays -> G = 32, 262 145 rays -> G = 1 (one lane per ray, more than one workgroup per CU)
NEAR_FAR_CASES = [(V, R) for V in (1, 63, 64, 65, 1500) for R in (1, 63, 65, 513)] + [(10475, 1024), (65, 8193), (5, 262145)]


@pytest.mark.parametrize("V,R", NEAR_FAR_CASES)
def test_near_far_equals_the_float32_oracle_bit_for_bit(V, R):
    from animatablegaussians_amd.template_render import near_far_smpl
    c = _near_far_case(V, R)
    print(f"V = {V}, R = {R}: {c['census']}")
    if R >= 63:
        for kind in ("miss", "hit", "negative_near", "behind", "graze_hit", "graze_miss"):
            assert c["census"][kind] > 0, f"the scene holds no ray of kind {kind}"
    v, o, d = _t(c["vertices"]), _t(c["o"]), _t(c["d"])
    for tag, fb in (("with_fb", (_t(c["fallback"][0]), _t(c["fallback"][1]))), ("without", None)):
        near, far, hit = near_far_smpl(v, o, d, 0.1, fallback=fb)
        wn, wf, wh = c[tag]
        assert near.is_cuda and near.shape == (R,) and far.shape == (R,) and hit.shape == (R,) and str(hit.dtype) == "torch.bool"
        assert np.array_equal(hit.cpu().numpy(), wh), f"{tag}: hit differs"
        bad = int((_bits(near) != _bits(wn)).sum()), int((_bits(far) != _bits(wf)).sum())
        print(f"  {tag}: rays whose near / far bits differ from the float32 oracle: {bad[0]} / {bad[1]} of {R}")
        assert bad == (0, 0)
        if fb is None:
            assert not near[~hit].any() and not far[~hit].any()


def test_near_far_ignores_the_order_of_the_vertices():
    from animatablegaussians_amd.template_render import near_far_smpl
    c = _near_far_case(1500, 513)
    perm = np.random.RandomState(2).permutation(1500)
    o, d = _t(c["o"]), _t(c["d"])
    a = near_far_smpl(_t(c["vertices"]), o, d, 0.1)
    b = near_far_smpl(_t(c["vertices"][perm]), o, d, 0.1)
    again = near_far_smpl(_t(c["vertices"]), o, d, 0.1)
    for x, y, z in zip(a, b, again):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), "a permutation of the vertices changes the result"
        assert np.array_equal(x.cpu().numpy().view(np.uint8), z.cpu().numpy().view(np.uint8)), "two calls differ"
    other = near_far_smpl(_t(c["vertices"]), o, d, 0.13)
    assert not np.array_equal(_bits(a[0]), _bits(other[0]))


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    fx = dict(np.load(FIXTURE))
    for a in fx.values():
        a.setflags(write=False)
    return fx


@pytest.mark.parametrize("R", [1, 257])
@pytest.mark.parametrize("S", [2, 63, 64, 65])
def test_samples_equal_the_reference_bit_for_bit(S, R):
    from animatablegaussians_amd.template_render import sample_pts_on_rays
    fx = _fixture()
    idx = np.arange(R) % len(fx["ray_o"])
    o, d, near, far = (_t(fx[k][idx]) for k in ("ray_o", "ray_d", "near", "far"))
    u = _t(fx[f"s{S}_u"][idx])
    plain = sample_pts_on_rays(o, d, near, far, S)
    jittered = sample_pts_on_rays(o, d, near, far, S, u=u)
    for tag, (pts, z) in (("", plain), ("p", jittered)):
        assert pts.shape == (R, S, 3) and z.shape == (R, S) and pts.is_cuda and str(pts.dtype) == "torch.float32"
        bz, bp = int((_bits(z) != _bits(fx[f"s{S}_z{tag}32"][idx])).sum()), int((_bits(pts) != _bits(fx[f"s{S}_pts{tag}32"][idx])).sum())
        print(f"S = {S}, R = {R} {'perturbed' if tag else 'unperturbed'}: z_vals / pts elements whose bits differ from the reference: {bz} / {bp}")
        assert (bz, bp) == (0, 0)
    assert _same(dict(zip("pz", jittered)), dict(zip("pz", sample_pts_on_rays(o, d, near, far, S, u=u)))), "the same u gives other samples"
    # the mask: unmasked rays stay at their unperturbed values
    import torch
    mask = torch.arange(R, device="cuda") % 3 == 0
    pts, z = sample_pts_on_rays(o, d, near, far, S, u=u, mask=mask)
    m = mask.cpu().numpy()
    assert np.array_equal(_bits(z)[m], _bits(jittered[1])[m]) and np.array_equal(_bits(z)[~m], _bits(plain[1])[~m])
    assert np.array_equal(_bits(pts)[m], _bits(jittered[0])[m]) and np.array_equal(_bits(pts)[~m], _bits(plain[0])[~m])
    # view directions: within 2 ulp of the float64 quotient rounded to float32 (torch's norm sums in its own order)
    p2, z2, dirs = sample_pts_on_rays(o, d, near, far, S, return_viewdirs=True)
    assert np.array_equal(_bits(p2), _bits(plain[0])) and np.array_equal(_bits(z2), _bits(plain[1])) and dirs.shape == (R, S, 3)
    want = tro.viewdirs64(fx["ray_d"][idx]).astype(np.float32)
    g = dirs.cpu().numpy()
    assert np.array_equal(_bits(g), _bits(np.repeat(g[:, :1], S, 1))), "a ray's view direction changes along the ray"
    ulps = float((np.abs(g[:, 0].astype(np.float64) - want) / np.spacing(np.abs(want))).max())
    print(f"S = {S}, R = {R}: view directions at most {ulps:.2f} ulp from the rounded float64 quotient")
    assert ulps <= 2


# ---- compositing ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _composite_case(R, S):
    import torch
    density, color, z = tro.composite_case(R, S, seed=100 * S + R)
    out = dict(density=density, color=color, z=z)
    for white in (False, True):
        out[white] = (tro.composite(density, color, z, white, torch.float64), tro.composite(density, color, z, white, torch.float32))
    for a in (density, color, z) + tuple(v for w in (False, True) for o in out[w] for v in o.values()):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("R", [1, 3, 257])
@pytest.mark.parametrize("S", [2, 63, 64, 65, 130])
def test_composite_against_the_float64_oracle(S, R):
    from animatablegaussians_amd.template_render import composite
    c = _composite_case(R, S)
    density, color, z = _t(c["density"]), _t(c["color"]), _t(c["z"])
    o64, o32 = c[False]
    if R == 257:
        acc, ones = o64["acc_map"], int((o32["alpha"] == 1).sum())
        print(f"S = {S}: {int((acc < 0.01).sum())} rays with acc < 0.01, {int((acc > 0.99).sum())} with acc > 0.99, {ones} samples with float32 alpha = 1 exactly")
        assert (acc < 0.01).any() and (acc > 0.99).any() and ones > 0
    got = composite(density, color, z, want=MAPS)
    assert all(got[k].is_cuda and str(got[k].dtype) == "torch.float32" for k in MAPS) and set(got) == set(MAPS)
    _compare(f"S = {S}, R = {R}", got, o64, o32, MAPS)
    white = composite(density, color, z, white_bkgd=True, want=MAPS)
    _compare(f"S = {S}, R = {R}, white background", white, *c[True], MAPS)
    for k in MAPS[1:]:
        assert np.array_equal(_bits(white[k]), _bits(got[k])), f"{k} changes with the background"
    # the field's shapes are taken as they are, and a subset of the maps is the same maps
    flat = composite(density.reshape(-1, 1), color.reshape(-1, 3), z)
    assert set(flat) == {"rgb_map", "acc_map"} and _same(flat, {k: got[k] for k in flat})
    # a ray's outputs depend on that ray alone: one ray at a time, and two halves
    import torch
    halves = [composite(density[a:b], color[a:b], z[a:b], want=MAPS) for a, b in ((0, R // 2), (R // 2, R))]
    singles = [composite(density[r:r + 1], color[r:r + 1], z[r:r + 1], want=MAPS) for r in range(R)]
    for k in MAPS:
        assert np.array_equal(_bits(torch.cat([h[k] for h in halves])), _bits(got[k])), f"{k}: two halves differ from one call"
        assert np.array_equal(_bits(torch.cat([s[k] for s in singles])), _bits(got[k])), f"{k}: one ray at a time differs from one call"
    no_color = composite(density, None, z, want=("acc_map", "depth_map"))
    assert _same(no_color, {k: got[k] for k in ("acc_map", "depth_map")})


def test_indices_past_2_31():
    """R * S * 3 > 2^31: the last rays of one large call equal, bit for bit, a small call on those rays alone."""
    import torch
    from animatablegaussians_amd.template_render import composite, sample_pts_on_rays
    S = 64
    R = (2 ** 31) // (3 * S) + 4099
    assert R * S * 3 > 2 ** 31 and R % 4 != 0
    o, d, near, far = tro.ray_scene(4099, 3)
    idx = torch.arange(R, device="cuda") % 4099
    o, d, near, far = _t(o)[idx], _t(d)[idx], _t(near)[idx], _t(far)[idx]
    pts, z = sample_pts_on_rays(o, d, near, far, S)
    tail = slice(R - 300, R)
    p_small, z_small = sample_pts_on_rays(o[tail], d[tail], near[tail], far[tail], S)
    assert np.array_equal(_bits(pts[tail]), _bits(p_small)) and np.array_equal(_bits(z[tail]), _bits(z_small))
    want_z, want_p = tro.sample(o[tail].cpu().numpy(), d[tail].cpu().numpy(), near[tail].cpu().numpy(), far[tail].cpu().numpy(), S)
    assert np.array_equal(_bits(z_small), _bits(want_z)) and np.array_equal(_bits(p_small), _bits(want_p))
    color = pts.abs_().clamp_(max=1.0)                       # any finite colours; the buffer is reused
    big = composite(z, color, z, want=MAPS[:3])
    small = composite(z[tail], color[tail], z[tail], want=MAPS[:3])
    for k in MAPS[:3]:
        assert np.array_equal(_bits(big[k][tail]), _bits(small[k])), f"{k}: the last rays of the large call differ from a small call"
    assert float(small["acc_map"].min()) > 0.5


# ---- render -----------------------------------------------------------------------------------------------------------------------------
RENDER_MAPS = ("rgb_map", "acc_map", "depth_map")
N_PIX = 24


@functools.lru_cache(maxsize=None)
def _sphere_net(use_viewdir=False):
    net = tfo.make_net(tfo.NARROW, 4, use_viewdir=use_viewdir, trained=False)        # geometric initialisation: an approximate sphere
    return net, _field(net)


def _camera():
    o, d = tro.pinhole_rays(N_PIX, half_width=0.5)
    return o, d, np.full(len(o), 1.3, np.float32), np.full(len(o), 3.7, np.float32)


@functools.lru_cache(maxsize=None)
def _render_oracle(sampling):
    """The chain oracle field -> oracle composite in float64 and float32 on the float32 oracle's samples (which the kernels give bit for
    bit) -- built once, never modified."""
    import torch
    net, _ = _sphere_net()
    o, d, near, far = _camera()
    body = tro.sphere_points(600, 0.7, seed=5)                                    # dense enough for every central ray to enter a front and a back ball
    hit = np.ones(len(o), bool)
    if sampling == "smpl":
        empty = np.full(len(o), 2.0, np.float32)                                     # near = far: no interval
        near, far, hit, _ = tro.near_far(body, o, d, 0.1, (empty, empty), np.float32)
    z, pts = tro.sample(o, d, near, far, 64)
    chains = []
    for dtype in (torch.float64, torch.float32):
        f = tfo.forward(net, pts.reshape(-1, 3), None, dtype)
        chains.append(tro.composite(f["density"], f["color"], z, False, dtype))
    for a in [body, hit] + [v for c in chains for v in c.values()]:
        a.setflags(write=False)
    return body, hit, chains[0], chains[1]


@pytest.mark.parametrize("sampling", ["uniform", "smpl"])
def test_render_canonical_against_the_chain_oracle(sampling):
    from animatablegaussians_amd import template_render as tr
    net, field = _sphere_net()
    body, hit, o64, o32 = _render_oracle(sampling)
    o, d, near, far = (_t(a) for a in _camera())
    if sampling == "smpl":
        near = far = _t(np.full(N_PIX * N_PIX, 2.0, np.float32))
    kw = dict(sampling=sampling, live_smpl_v=_t(body) if sampling == "smpl" else None, want=RENDER_MAPS)
    got = tr.render(field, o, d, near, far, **kw)
    assert got["rgb_map"].shape == (N_PIX * N_PIX, 3) and got["acc_map"].shape == (N_PIX * N_PIX,) and set(got) == set(RENDER_MAPS)
    _compare(f"render, {sampling} sampling", got, o64, o32, RENDER_MAPS)
    acc = got["acc_map"].cpu().numpy().reshape(N_PIX, N_PIX)
    centre = acc[N_PIX // 2 - 1:N_PIX // 2 + 1, N_PIX // 2 - 1:N_PIX // 2 + 1]
    print(f"render, {sampling} sampling: acc of the four central rays {centre.min():.6f} .. {centre.max():.6f}; rays that hit no ball: {int((~hit).sum())}")
    assert centre.min() > 0.99
    if sampling == "smpl":
        assert 0 < (~hit).sum() < hit.size and not acc.reshape(-1)[~hit].any(), "a ray outside every ball with an empty interval has acc != 0"
        assert not got["rgb_map"].cpu().numpy()[~hit].any()
    # render is the chain of the four public calls
    n, f = near, far
    if sampling == "smpl":
        n, f, h = tr.near_far_smpl(kw["live_smpl_v"], o, d, 0.1, fallback=(near, far))
        assert np.array_equal(h.cpu().numpy(), hit)
    pts, z = tr.sample_pts_on_rays(o, d, n, f, 64)
    ret = field(pts.view(-1, 3), want=("sdf", "density", "color"))
    by_hand = tr.composite(ret["density"], ret["color"], z, want=RENDER_MAPS)
    assert _same(got, by_hand), "render differs from the chain of its four public calls"
    for chunk in (7, 64, N_PIX * N_PIX):
        assert _same(got, tr.render(field, o, d, near, far, chunk_size=chunk, **kw)), f"chunk_size = {chunk} changes the maps"
    batched = tr.render(field, o[None], d[None], near[None], far[None], **kw)
    assert batched["rgb_map"].shape == (1, N_PIX * N_PIX, 3) and _same(got, {k: v[0] for k, v in batched.items()})
    white = tr.render(field, o, d, near, far, white_bkgd=True, **kw)
    assert np.array_equal(_bits(white["acc_map"]), _bits(got["acc_map"]))
    assert np.array_equal(_bits(white["rgb_map"]), _bits(got["rgb_map"] + (1 - got["acc_map"])[:, None]))


def test_render_with_view_directions_and_without_colour():
    from animatablegaussians_amd import template_render as tr
    from animatablegaussians_amd.template_field import TemplateField
    net, field = _sphere_net(use_viewdir=True)
    o, d, near, far = (_t(a) for a in _camera())
    got = tr.render(field, o, d, near, far, sampling="uniform", chunk_size=100, want=MAPS)
    pts, z, dirs = tr.sample_pts_on_rays(o, d, near, far, 64, return_viewdirs=True)
    ret = field(pts.view(-1, 3), dirs.view(-1, 3), want=("sdf", "density", "color"))
    assert _same(got, tr.composite(ret["density"], ret["color"], z, want=MAPS)), "render differs from the chain with view directions"
    blind = field(pts.view(-1, 3), None, want=("sdf", "density", "color"))
    assert not np.array_equal(_bits(blind["color"]), _bits(ret["color"])), "the view directions do not reach the colour MLP"
    # a field without a colour MLP renders everything but rgb_map
    geo, _ = tfo.folded_layers(net)
    bare = TemplateField(geo, [], multires=net["arch"]["multires"])
    maps = tr.render(bare, o, d, near, far, sampling="uniform", want=("acc_map", "depth_map"))
    assert _same(maps, {k: got[k] for k in ("acc_map", "depth_map")})
    with pytest.raises(ValueError, match="colour"):
        tr.render(bare, o, d, near, far, sampling="uniform")


def test_render_depth_guided():
    import torch
    from animatablegaussians_amd import template_render as tr
    net, field = _sphere_net()
    o, d, near, far = (_t(a) for a in _camera())
    R, S, nsd = N_PIX * N_PIX, 17, 0.05
    dist = torch.full((R,), 1.8, device="cuda") + 0.001 * torch.arange(R, device="cuda")
    dist[::3] = 0.0                                                             # no depth there: the given near / far stay
    valid = dist > 1e-6
    u = _t(np.random.RandomState(3).uniform(0, 1, (R, S)).astype(np.float32))
    want = ("rgb_map", "acc_map", "weights")
    for jitter in (None, u):
        got = tr.render(field, o, d, near, far, sampling="depth", dist=dist, near_sur_dist=nsd, n_samples=S, u=jitter, chunk_size=50, want=want)
        assert got["weights"].shape == (R, S)
        n2, f2 = torch.where(valid, dist - nsd, near), torch.where(valid, dist + nsd, far)
        pts, z = tr.sample_pts_on_rays(o, d, n2, f2, S, u=jitter, mask=valid if jitter is not None else None)
        ret = field(pts.view(-1, 3), want=("sdf", "density", "color"))
        assert _same(got, tr.composite(ret["density"], ret["color"], z, want=want)), "render differs from the depth-guided chain"
        # the rays with dist = 0: the given interval, never perturbed
        pts0, z0 = tr.sample_pts_on_rays(o, d, near, far, S)
        ret0 = field(pts0.view(-1, 3), want=("sdf", "density", "color"))
        keep = tr.composite(ret0["density"], ret0["color"], z0, want=want)
        off = (~valid).cpu().numpy()
        assert off.sum() == (R + 2) // 3
        for k in want:
            assert np.array_equal(_bits(got[k])[off], _bits(keep[k])[off]), f"{k}: a ray with dist = 0 left its given near / far"
        assert not np.array_equal(_bits(got["weights"])[~off], _bits(keep["weights"])[~off])


def test_render_posed_space_is_the_chain_by_hand():
    import inverse_skinning_oracle as iso
    import mesh_query_oracle as mqo
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd import template_render as tr
    from animatablegaussians_amd.weight_volume import WeightVolume
    net, field = _sphere_net()
    case = iso.smooth_case((16, 16, 16, 55), n=1, B=1, offset=0.05)
    vol = WeightVolume(_t(case["volume"]), _t(case["volume"]), case["bounds"], np.zeros(3, np.float32), case["bounds"])
    v, f = mqo.lattice_mesh(8, 10)
    live = dict(cano2live_jnt_mats=_t(case["jnt_mats"]), volume=vol, live_mesh_v=_t(v[None]), live_mesh_f=_t(f[None]),
                live_mesh_lbs=_t(mqo.sparse_weights(v, 55)[None]), near_thres=0.05, use_root_finding=True, with_hand=False)
    o, d = tro.pinhole_rays(8, eye=(0.1, -0.2, -2.5), target=(0.0, -0.2, 0.0), half_width=0.3)
    o, d = _t(o), _t(d)
    near, far = _t(np.full(64, 1.8, np.float32)), _t(np.full(64, 3.2, np.float32))
    got = tr.render(field, o, d, near, far, space="live", sampling="uniform", live=live, chunk_size=24, want=RENDER_MAPS)
    pts, z = tr.sample_pts_on_rays(o, d, near, far, 64)
    cano, _ = inv.transform_live2cano(pts.view(1, -1, 3), **live)
    assert not np.array_equal(_bits(cano[0]), _bits(pts.view(-1, 3))), "the samples were not moved"
    ret = field(cano[0], want=("sdf", "density", "color"))
    by_hand = tr.composite(ret["density"], ret["color"], z, want=RENDER_MAPS)
    assert _same(got, by_hand), "render(space='live') differs from sampling + transform_live2cano + field + composite"
    cano_maps = tr.render(field, o, d, near, far, sampling="uniform", want=RENDER_MAPS)
    assert not _same(got, cano_maps)
    acc = got["acc_map"].cpu().numpy()
    print(f"posed render: acc {acc.min():.4f} .. {acc.max():.4f}; |cano - posed| of the samples up to {float((cano[0] - pts.view(-1, 3)).abs().max()):.3f}")
    assert np.isfinite(acc).all() and acc.max() > 0.5


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_ray_sets():
    import ctypes
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd import template_render as tr
    net, field = _sphere_net()
    o, d, near, far = (_t(a[:10]) for a in _camera())
    body = _t(tro.sphere_points(30, 0.7, seed=5))
    dens, col, z = torch.rand(10, 8, device="cuda"), torch.rand(10, 8, 3, device="cuda"), torch.rand(10, 8, device="cuda").cumsum(1)
    torch.cuda.synchronize()
    bad = [
        lambda: tr.near_far_smpl(body.cpu(), o, d), lambda: tr.near_far_smpl(body, o.cpu(), d), lambda: tr.near_far_smpl(body.double(), o, d),
        lambda: tr.near_far_smpl(body[:, :2], o, d), lambda: tr.near_far_smpl(body, o, d[:5]), lambda: tr.near_far_smpl(body[:0], o, d),
        lambda: tr.near_far_smpl(body, o, d, radius=0.0), lambda: tr.near_far_smpl(body, o, d, fallback=(near, far[:3])),
        lambda: tr.near_far_smpl(body, o, d, fallback=near), lambda: tr.near_far_smpl(body.cpu().numpy(), o, d),
        lambda: tr.sample_pts_on_rays(o.cpu(), d, near, far), lambda: tr.sample_pts_on_rays(o, d, near.double(), far),
        lambda: tr.sample_pts_on_rays(o, d, near[:4], far), lambda: tr.sample_pts_on_rays(o, d, near, far, 1),
        lambda: tr.sample_pts_on_rays(o, d, near, far, 1025), lambda: tr.sample_pts_on_rays(o, d, near, far, 8, u=torch.rand(10, 9, device="cuda")),
        lambda: tr.sample_pts_on_rays(o, d, near, far, 8, mask=torch.ones(10, dtype=torch.bool, device="cuda")),
        lambda: tr.sample_pts_on_rays(o, d, near, far, 8, u=torch.rand(10, 8, device="cuda"), mask=torch.ones(10, device="cuda")),
        lambda: tr.composite(dens.cpu(), col, z), lambda: tr.composite(dens, col, z.double()), lambda: tr.composite(dens[:, :7], col, z),
        lambda: tr.composite(dens, col[..., :2], z), lambda: tr.composite(dens[:, :1], col[:, :1], z[:, :1]),
        lambda: tr.composite(dens, col, z, want=("normal",)), lambda: tr.composite(dens, None, z),
        lambda: tr.composite(torch.rand(2, 1025, device="cuda"), torch.rand(2, 1025, 3, device="cuda"), torch.rand(2, 1025, device="cuda")),
        lambda: tr.render(field, o, d, near, far, sampling="importance"), lambda: tr.render(field, o, d, near, far, sampling="smpl"),
        lambda: tr.render(field, o, d, near, far, sampling="depth"), lambda: tr.render(field, o, d, near, far, sampling="depth", dist=near),
        lambda: tr.render(field, o, d, near, far, sampling="depth", dist=near, near_sur_dist=0.05, n_samples=1),
        lambda: tr.render(field, o, d, near, far, sampling="depth", dist=near, near_sur_dist=0.05, n_samples=1025),
        lambda: tr.render(field, o, d, near, far, sampling="uniform", space="world"), lambda: tr.render(field, o, d, near, far, sampling="uniform", space="live"),
        lambda: tr.render(field, o.cpu(), d, near, far, sampling="uniform"), lambda: tr.render(field, o, d, near, far, sampling="uniform", chunk_size=0),
        lambda: tr.render(field, o, d, near, far, sampling="uniform", want=("normal",)), lambda: tr.render(None, o, d, near, far, sampling="uniform"),
        lambda: tr.render(field, o, d, near, far, sampling="smpl", live_smpl_v=body, u=torch.rand(10, 63, device="cuda")),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the ABI refuses the same counts itself, before it looks at a pointer
    L, null = _lib.lib(), ctypes.c_void_p(None)
    for S in (1, 1025):
        assert L.ag_ray_sample(null, null, null, null, 4, null, S, null, null, null, null, null, null) != 0 and b"S = " in L.ag_last_error()
        assert L.ag_ray_composite(null, null, null, 4, S, 0, null, null, null, null, null, null) != 0 and b"S = " in L.ag_last_error()
    assert L.ag_ray_near_far(null, 0, null, null, 4, 0.1, null, null, null, null, null, null) != 0 and b"V = 0" in L.ag_last_error()
    assert L.ag_ray_near_far(null, 3, null, null, -1, 0.1, null, null, null, null, null, null) != 0
    assert L.ag_ray_near_far(null, 3, null, null, 4, 0.1, null, null, null, null, null, null) != 0 and b"null" in L.ag_last_error()
    assert L.ag_ray_near_far(null, 3, null, null, 0, 0.1, null, null, null, null, null, null) == 0          # R = 0: nothing to do
    torch.cuda.synchronize()
    # R = 0: empty outputs of the right shapes
    e3, e1 = torch.empty((0, 3), device="cuda"), torch.empty((0,), device="cuda")
    n0, f0, h0 = tr.near_far_smpl(body, e3, e3)
    assert n0.shape == (0,) and f0.shape == (0,) and h0.shape == (0,) and str(h0.dtype) == "torch.bool"
    p0, z0, v0 = tr.sample_pts_on_rays(e3, e3, e1, e1, 8, return_viewdirs=True)
    assert p0.shape == (0, 8, 3) and z0.shape == (0, 8) and v0.shape == (0, 8, 3)
    c0 = tr.composite(torch.empty((0, 8), device="cuda"), torch.empty((0, 8, 3), device="cuda"), z0, want=MAPS)
    assert c0["rgb_map"].shape == (0, 3) and c0["acc_map"].shape == (0,) and c0["weights"].shape == (0, 8) and c0["disp_map"].shape == (0,)
    for sampling, kw in (("uniform", {}), ("smpl", dict(live_smpl_v=body)), ("depth", dict(dist=e1, near_sur_dist=0.05, n_samples=9))):
        r0 = tr.render(field, e3, e3, e1, e1, sampling=sampling, want=MAPS, **kw)
        assert r0["rgb_map"].shape == (0, 3) and r0["acc_map"].shape == (0,) and r0["weights"].shape == (0, 9 if sampling == "depth" else 64)
        assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in r0.values())
