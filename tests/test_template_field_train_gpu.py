"""The template field's training path on the GPU (``include/ag_template_field_train.h``, ``template_train.TemplateFieldModule``) against
``template_field_train_oracle.py``.

Forward: ``sdf`` and ``color`` equal the fused inference kernel (``TemplateField`` on the module's own fp32-folded weights) bit for bit.
Gradients, per tensor, ``e = max|gpu - float64| / max|float64|``:

    e <= 4 x e32 + 16 x 2^-24

with ``e32`` the same figure of the oracle's float32 CPU run on the same inputs, computed here.  The factor 4 covers another summation
order over the points (slab chains against torch's GEMM blocking); a wrong derivative or a dropped column shows at 1e-2 and above; the
floor is 16 fp32 ulps at the tensor's maximum.  Every test prints both figures per tensor ("Template field training").

Measured on the MI355X: the worst tensor of the gradient cases at 0.27 / 0.38 / 0.56 / 0.77 of its bar at N = 1 / 33 / 95 / 1057 (narrow)
and 0.38 at N = 257 (reference); through ``render_train`` 0.03 .. 0.11; 17 tests in 4.9 s.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_oracle as tfo  # noqa: E402
import template_field_train_oracle as tto  # noqa: E402
import template_render_oracle as tro  # noqa: E402

pytestmark = pytest.mark.gpu
ARCH = {"narrow": tfo.NARROW, "reference": tfo.REFERENCE}
FLOOR = 16 * 2.0 ** -24


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _net(arch, geo_activation="softplus", seed=3):
    return tfo.make_net(ARCH[arch], seed=seed, use_viewdir=True, scale=1.0, geo_activation=geo_activation)


def _module(net):
    from animatablegaussians_amd.template_train import TemplateFieldModule
    a = net["arch"]
    return TemplateFieldModule.from_state_dict(tfo.state_dict(net), a["multires"], True, a["multires_viewdir"], geo_activation=net["geo_activation"]).cuda()


@functools.lru_cache(maxsize=None)
def _case(arch, N, geo_activation="softplus"):
    """Points, directions, upstream gradients and the oracle in both precisions -- built once, never modified."""
    import torch
    net = _net(arch, geo_activation)
    rs = np.random.RandomState(N)
    xyz, dirs = tfo.box_points(N, seed=N), tfo.unit_dirs(N, seed=N + 1)
    g_sdf, g_color = rs.normal(size=(N, 1)).astype(np.float32), rs.normal(size=(N, 3)).astype(np.float32)
    o64 = tto.gradients(net, xyz, dirs, g_sdf, g_color, torch.float64)
    o32 = tto.gradients(net, xyz, dirs, g_sdf, g_color, torch.float32)
    return dict(net=net, xyz=xyz, dirs=dirs, g_sdf=g_sdf, g_color=g_color, o64=o64, o32=o32)


def _bar(what, got, f64, f32):
    """Asserts the bar of the module docstring for one tensor and prints its figures."""
    got, f64, f32 = (np.asarray(a, np.float64) for a in (got, f64, f32))
    assert got.shape == f64.shape, f"{what}: shape {got.shape}, expected {f64.shape}"
    top = np.abs(f64).max()
    assert top > 0 and np.isfinite(got).all(), what
    e, e32 = np.abs(got - f64).max() / top, np.abs(f32 - f64).max() / top
    print(f"{what}: e = {e:.3e}, e32 = {e32:.3e}, bar {4 * e32 + FLOOR:.3e}")
    assert e <= 4 * e32 + FLOOR, f"{what}: e = {e:.3e} over the bar {4 * e32 + FLOOR:.3e} (e32 = {e32:.3e})"
    return e, e32


def _run(m, xyz, dirs, g_sdf, g_color):
    """One forward and backward of the module's autograd function with the flat vector kept: -> (sdf, color, flat gradient, parameter
    gradients by name)."""
    import torch
    from animatablegaussians_amd.template_train import _FieldTrain
    m.zero_grad(set_to_none=True)
    flat = m.flat_parameters()
    flat.retain_grad()
    sdf, color = _FieldTrain.apply(flat, xyz, dirs, m)
    outs, gs = [], []
    if g_sdf is not None:
        outs.append(sdf), gs.append(g_sdf)
    if g_color is not None:
        outs.append(color), gs.append(g_color)
    torch.autograd.backward(outs, gs)
    return sdf, color, flat.grad, {k: p.grad for k, p in m.named_parameters()}


def _split(m, g_flat):
    """The flat gradient as per-layer (dW [width, K], db [width]) numpy arrays."""
    g = g_flat.detach().cpu().numpy()
    out, w_at, b_at = [], 0, m._n_weights
    for _, K, width, *_ in m.plan.layers:
        out.append((g[w_at:w_at + width * K].reshape(width, K), g[b_at:b_at + width]))
        w_at, b_at = w_at + width * K, b_at + width
    assert w_at == m._n_weights and b_at == g.size
    return out


def _assert_shares(shares, least):
    print("softplus pre-activations: linear branch %.1f %%, |beta z| < 5 %.1f %%, below -20 %.1f %%" % tuple(100 * s for s in shares))
    assert min(shares) >= least, f"the net does not cover softplus' three regions: {shares}"


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch, N, geo_activation", [("narrow", n, "softplus") for n in (1, 31, 32, 33, 95)] + [("narrow", 95, "relu"), ("reference", 257, "softplus")])
def test_forward_equals_the_fused_kernel_bit_for_bit(arch, N, geo_activation):
    import torch
    from animatablegaussians_amd.template_field import TemplateField
    net = _net(arch, geo_activation)
    a = net["arch"]
    m = _module(net)
    layers = [(w.detach().cpu().numpy(), b.detach().cpu().numpy()) for w, b in m.folded_weights()]
    n_geo = len(net["geo"])
    field = TemplateField(layers[:n_geo], layers[n_geo:], a["multires"], True, a["multires_viewdir"], geo_activation=geo_activation)
    xyz, dirs = _t(tfo.box_points(N, seed=N)), _t(tfo.unit_dirs(N, seed=N + 1))
    with torch.no_grad():
        for d in (dirs, None):
            sdf, color = m(xyz, d)
            ref = field(xyz, d, want=("sdf", "color"))
            assert sdf.shape == (N, 1) and color.shape == (N, 3)
            assert np.array_equal(_bits(sdf), _bits(ref["sdf"])), f"sdf differs from the fused kernel (viewdirs {'given' if d is not None else 'None'})"
            assert np.array_equal(_bits(color), _bits(ref["color"])), f"color differs from the fused kernel (viewdirs {'given' if d is not None else 'None'})"
        assert not np.array_equal(_bits(m(xyz, dirs)[1]), _bits(m(xyz, None)[1])), "the view directions play no part"


# ---- 2. gradients against float64 ----------------------------------------------------------------------------------------------------------
def _slab():
    from animatablegaussians_amd.template_train import SLAB
    return SLAB


@pytest.mark.parametrize("arch, N", [("narrow", 1), ("narrow", 33), ("narrow", 95), ("narrow", "slab + 33"), ("reference", 257)])
def test_gradients_against_float64(arch, N):
    N = _slab() + 33 if N == "slab + 33" else N
    c = _case(arch, N)
    if N >= 95:
        _assert_shares(c["o64"][3], 0.10 if arch == "narrow" else 0.02)
    m = _module(c["net"])
    sdf, color, g_flat, g_par = _run(m, _t(c["xyz"]), _t(c["dirs"]), _t(c["g_sdf"]), _t(c["g_color"]))
    g64, g32 = c["o64"][2], c["o32"][2]
    for l, (dw, db) in enumerate(_split(m, g_flat)):
        _bar(f"{arch}, N = {N}: dW.{l}", dw, g64[f"dW.{l}"], g32[f"dW.{l}"])
        _bar(f"{arch}, N = {N}: db.{l}", db, g64[f"db.{l}"], g32[f"db.{l}"])
    assert set(g_par) - {"density_func.beta"} == set(g64) - {k for k in g64 if k.startswith(("dW.", "db."))}
    for k, g in g_par.items():
        if k == "density_func.beta":
            assert g is None                                               # the field does not use it
            continue
        _bar(f"{arch}, N = {N}: {k}", g.cpu().numpy(), g64[k], g32[k])


# ---- 3. structure -------------------------------------------------------------------------------------------------------------------------
def test_backward_is_reproducible_and_a_missing_upstream_is_zeros():
    import torch
    N = _slab() + 33
    c = _case("narrow", N)
    _assert_shares(c["o64"][3], 0.10)
    m = _module(c["net"])
    xyz, dirs, g_sdf, g_color = (_t(c[k]) for k in ("xyz", "dirs", "g_sdf", "g_color"))
    first = _run(m, xyz, dirs, g_sdf, g_color)[2]
    again = _run(m, xyz, dirs, g_sdf, g_color)[2]
    assert np.array_equal(_bits(first), _bits(again)), "two backward calls differ"
    n_geo = len(c["net"]["geo"])
    e_pos, e_view = 3 + 6 * c["net"]["arch"]["multires"], 3 + 6 * c["net"]["arch"]["multires_viewdir"]
    layers = _split(m, first)
    for l, cols in ((0, slice(0, e_pos)), (4, slice(-e_pos, None)), (n_geo, slice(-e_view, None))):
        assert (np.abs(layers[l][0][:, cols]).max(axis=0) > 0).all(), f"layer {l}: an embedding column has no weight gradient"
    # without g_color: exact zeros in every colour slot, the geometry gradients of an explicit zero g_color
    only_sdf = _split(m, _run(m, xyz, dirs, g_sdf, None)[2])
    zero_col = _split(m, _run(m, xyz, dirs, g_sdf, torch.zeros_like(g_color))[2])
    for l, ((dw, db), (dw0, db0)) in enumerate(zip(only_sdf, zero_col)):
        if l >= n_geo:
            assert not dw.any() and not db.any(), f"colour layer {l} has a gradient without g_color"
        assert np.array_equal(dw, dw0) and np.array_equal(db, db0), f"layer {l}: g_color = None and g_color = 0 differ"
        assert l >= n_geo or dw.any()
    # without g_sdf likewise
    only_col = _split(m, _run(m, xyz, dirs, None, g_color)[2])
    zero_sdf = _split(m, _run(m, xyz, dirs, torch.zeros_like(g_sdf), g_color)[2])
    for l, ((dw, db), (dw0, db0)) in enumerate(zip(only_col, zero_sdf)):
        assert np.array_equal(dw, dw0) and np.array_equal(db, db0) and dw.any(), f"layer {l}: g_sdf = None and g_sdf = 0 differ"
    assert not np.array_equal(only_col[0][0], layers[0][0])


@pytest.mark.parametrize("N", [33, "slab + 33"])
def test_abi_writes_nothing_outside_its_outputs(N):
    """The C ABI with every output buffer longer than stated and filled with a sentinel: the tails are intact, and what lies inside is
    what the module computes."""
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.mlp_blob import ptr, stream
    N = _slab() + 33 if N == "slab + 33" else N
    c = _case("narrow", N)
    m = _module(c["net"])
    xyz, dirs, g_sdf, g_color = (_t(c[k]) for k in ("xyz", "dirs", "g_sdf", "g_color"))
    want = _run(m, xyz, dirs, g_sdf, g_color)
    L, d, dev = _lib.lib(), m.plan.desc(), xyz.device
    blob, blob_t = m.pack()
    n_stash, n_ws = (int(f(ctypes.byref(d), N)) for f in (L.ag_template_field_train_stash_floats, L.ag_template_field_train_workspace_floats))
    tail, sentinel = 256, -12345.5
    buf = {k: torch.full((n + tail,), sentinel, dtype=torch.float32, device=dev) for k, n in
           dict(stash=n_stash, ws=n_ws, sdf=N, color=3 * N, gw=m._n_weights, gb=m._n_biases).items()}
    _lib.check(L.ag_template_field_train_forward(ctypes.byref(d), ptr(blob), blob.numel(), ptr(xyz), ptr(dirs), N, ptr(buf["stash"]), n_stash, ptr(buf["sdf"]),
                                                 ptr(buf["color"]), stream(dev)), "forward")
    _lib.check(L.ag_template_field_train_backward(ctypes.byref(d), ptr(blob_t), blob_t.numel(), ptr(buf["stash"]), n_stash, ptr(g_sdf), ptr(g_color), N,
                                                  ptr(buf["ws"]), n_ws, ptr(buf["gw"]), ptr(buf["gb"]), stream(dev)), "backward")
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t[-tail:] == sentinel).all()), f"{k}: written past its stated size"
    assert not bool((buf["stash"][:n_stash] == sentinel).any()), "the stash has unwritten elements"
    assert np.array_equal(_bits(buf["sdf"][:N]), _bits(want[0]).reshape(-1)) and np.array_equal(_bits(buf["color"][:3 * N]), _bits(want[1]).reshape(-1))
    assert np.array_equal(_bits(torch.cat([buf["gw"][:-tail], buf["gb"][:-tail]])), _bits(want[2]))


def test_no_points_and_far_points():
    import torch
    c = _case("narrow", 33)
    m = _module(c["net"])
    empty = torch.empty((0, 3), device="cuda")
    sdf, color, g_flat, g_par = _run(m, empty, empty, torch.empty((0, 1), device="cuda"), torch.empty((0, 3), device="cuda"))
    assert sdf.shape == (0, 1) and color.shape == (0, 3) and g_flat.shape == (m._n_weights + m._n_biases,) and not bool(g_flat.any())
    assert all(g is None or not bool(g.any()) for g in g_par.values())
    # |x| = 50: softplus' threshold on one side, the underflow of its exponential on the other
    xyz = np.concatenate([c["xyz"][:5], 50.0 * np.sign(c["xyz"][5:13]), 50.0 * np.eye(3, dtype=np.float32), -50.0 * np.eye(3, dtype=np.float32)]).astype(np.float32)
    n = len(xyz)
    sdf, color, g_flat, g_par = _run(m, _t(xyz), _t(c["dirs"][:n]), _t(c["g_sdf"][:n]), _t(c["g_color"][:n]))
    assert bool(torch.isfinite(sdf).all()) and bool(torch.isfinite(color).all()) and bool(torch.isfinite(g_flat).all()) and bool(g_flat.any())
    assert all(g is None or bool(torch.isfinite(g).all()) for g in g_par.values())


# ---- 4. through the chain -----------------------------------------------------------------------------------------------------------------
WEIGHTS = {"color": 1.0, "mask": 0.5}
STEPS, LR = 20, 1e-3


def test_render_train_through_the_module():
    """64 canonical-space rays, ``sampling="uniform"`` (64 samples a ray: the sampling's own count) with the caller's ``u`` and
    ``dir_noise``, targets rendered by ``render`` from a teacher net."""
    import torch
    from animatablegaussians_amd.template_field import TemplateField
    from animatablegaussians_amd.template_render import render, render_train, training_loss
    R, S, arch = 64, 64, tfo.NARROW
    rs = np.random.RandomState(7)
    o, d, near, far = tro.ray_scene(R, seed=7)
    u = rs.uniform(0, 1, (R, S)).astype(np.float32)
    noise = (0.1 * rs.normal(size=(R * S, 3))).astype(np.float32)
    teacher_net = tfo.make_net(arch, seed=11, use_viewdir=True)
    geo, color = tfo.folded_layers(teacher_net)
    teacher = TemplateField(geo, color, arch["multires"], True, arch["multires_viewdir"], density_beta=float(teacher_net["beta"]))
    rays = (_t(o), _t(d), _t(near), _t(far))
    with torch.no_grad():
        target = render(teacher, *rays, space="cano", sampling="uniform")
    color_gt, mask_gt = target["rgb_map"].contiguous(), target["acc_map"].contiguous()
    print(f"teacher: acc_map {float(mask_gt.min()):.3f} .. {float(mask_gt.max()):.3f}")
    net = _net("narrow")
    m = _module(net)
    kw = dict(space="cano", sampling="uniform", u=_t(u), dir_noise=_t(noise))

    def step_loss():
        out = render_train(m, m.beta, *rays, **kw)
        return out, training_loss(out, color_gt, mask_gt, WEIGHTS)[0]

    # (a) one step's gradients against the float64 chain
    out, loss = step_loss()
    m.zero_grad(set_to_none=True)
    loss.backward()
    pts, z = out["cano_pts"].cpu().numpy(), out["z_vals"].cpu().numpy()
    chains = [tto.train_chain(net, float(net["beta"]), pts, z, d, noise, color_gt.cpu().numpy(), mask_gt.cpu().numpy(), WEIGHTS, dt)
              for dt in (torch.float64, torch.float32)]
    (loss64, g64), (loss32, g32) = chains
    print(f"loss {float(loss.detach()):.9f}, float64 chain {loss64:.9f}, float32 chain {loss32:.9f}")
    assert abs(float(loss.detach()) - loss64) <= 4 * abs(loss32 - loss64) + FLOOR * abs(loss64)
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(g64)
    for k, g in grads.items():
        assert g is not None and g.shape == m.state_dict()[k].shape, k
        _bar(f"render_train: d loss / d {k}", g.cpu().numpy().reshape(g64[k].shape), g64[k], g32[k])
    # (b) 20 Adam steps on that batch lower the loss
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    losses = [float(loss.detach())]
    opt.step()
    for _ in range(STEPS - 1):
        opt.zero_grad(set_to_none=True)
        _, loss = step_loss()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(step_loss()[1]))
    print("loss before every step and after the last:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0], "20 Adam steps did not lower the loss"
    # (c) the trained parameters as an inference field: the fold's rounding apart
    trained = tto.net_of_state_dict(m.state_dict(), net)
    xyz, dirs = tfo.box_points(95, seed=95), tfo.unit_dirs(95, seed=96)
    o64 = tto.gradients(trained, xyz, dirs, None, None, torch.float64)
    o32 = tto.gradients(trained, xyz, dirs, None, None, torch.float32)
    field = m.to_field()
    with torch.no_grad():
        ours = m(_t(xyz), _t(dirs))
        theirs = field(_t(xyz), _t(dirs), want=("sdf", "color"))
    for name, got in (("module sdf", ours[0]), ("to_field() sdf", theirs["sdf"])):
        _bar(f"after training: {name}", got.cpu().numpy(), o64[0], o32[0])
    for name, got in (("module color", ours[1]), ("to_field() color", theirs["color"])):
        _bar(f"after training: {name}", got.cpu().numpy(), o64[1], o32[1])
    out = render(field, *rays, space="cano", sampling="uniform")
    assert bool(torch.isfinite(out["rgb_map"]).all()) and out["rgb_map"].shape == (R, 3)
