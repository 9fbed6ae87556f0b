"""The fused gradient kernel (``include/ag_template_field_grad.h``, ``TemplateField.sdf_normal`` / ``surface_normals``) against
``template_field_grad_oracle.py``.

Bar, from the oracle alone, for ``normal`` and for ``sdf``: |gpu - float64 oracle| <= 4 x max|float32 oracle - float64 oracle| + 2^-22 x
max|float64 oracle|, the maxima over the case's whole point set (``test_template_field_gpu.py`` says why the factor is 4 and why the
maxima are the set's).  The float32 oracle is the autograd one, the reference's own way to this quantity.  ``sdf`` and ``density`` must
moreover be the forward kernel's bit for bit.  ReLU's derivative jumps at z = 0, so that case leaves out the points where a hidden
pre-activation of the float64 oracle is closer to 0 than 8 x the float32 oracle's own largest pre-activation error (at most 5 % of
them).  Every test prints measured deviation and bar; DESIGN.md's "Template field gradient" part has the table measured on the MI355X.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_grad_oracle as tgo  # noqa: E402
import template_field_oracle as tfo  # noqa: E402

pytestmark = pytest.mark.gpu
N_MAX = 1031
# make_net zeroes the skip layer's embedding columns [-(e_pos - 3):] at initialisation, which is every column at multires = 0: no skip layer there
MULTIRES_0 = dict(tfo.NARROW, multires=0, skip=())
MULTIRES_10 = dict(tfo.NARROW, multires=10)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


def _field(net):
    from animatablegaussians_amd.template_field import TemplateField
    arch = net["arch"]
    return TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=net["use_viewdir"],
                                         multires_viewdir=arch["multires_viewdir"], geo_activation=net["geo_activation"])


def _oracles(net, xyz):
    import torch
    o64, o32 = tgo.autograd(net, xyz, torch.float64), tgo.autograd(net, xyz, torch.float32)
    for o in (o64, o32):
        for v in o.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return o64, o32


def _compare(name, got, o64, o32, n=None, keys=("sdf", "normal"), keep=None):
    """The bar of the module docstring on the first ``n`` points (``keep``: a mask over them)."""
    for k in keys:
        w64, w32 = o64[k], o32[k].astype(np.float64)
        if keep is not None:
            w64, w32 = w64[keep], w32[keep]
        own = float(np.abs(w32 - w64).max())
        bar = 4 * own + 2.0 ** -22 * float(np.abs(w64).max())
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), f"{name} {k}: not finite"
        if keep is not None:
            g = g[keep]
        n_ = g.shape[0] if n is None else n
        assert g.shape == w64[:n_].shape, (k, g.shape, w64[:n_].shape)
        dev = float(np.abs(g - w64[:n_]).max()) if n_ else 0.0
        print(f"{name} {k}: |gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
        assert dev <= bar, f"{name} {k}: {dev:.3e} > {bar:.3e}"


@functools.lru_cache(maxsize=None)
def _reference_case():
    net = tfo.make_net(tfo.REFERENCE, 11)
    xyz = tfo.box_points(N_MAX, 5)
    return net, _field(net), xyz, _oracles(net, xyz)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 33, 257, N_MAX])
def test_reference_architecture_and_tile_tails(n):
    net, field, xyz, (o64, o32) = _reference_case()
    x = _t(xyz[:n])
    got = field.sdf_normal(x, want=("sdf", "normal", "density"))
    assert set(got) == {"sdf", "normal", "density", "cano_xyz"} and set(field.sdf_normal(x)) == {"sdf", "normal", "cano_xyz"}
    assert got["sdf"].shape == (n, 1) and got["normal"].shape == (n, 3) and got["density"].shape == (n, 1) and got["cano_xyz"].shape == (n, 3)
    assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in got.values())
    assert np.array_equal(_bits(got["cano_xyz"]), _bits(x))
    assert np.array_equal(_bits(got["sdf"]), _bits(field(x)["sdf"])), "sdf differs from the forward kernel's"
    fwd = field(x, want=("sdf", "density"))
    assert np.array_equal(_bits(got["density"]), _bits(fwd["density"])), "density differs from the forward kernel's"
    again = field.sdf_normal(x, want=("sdf", "normal", "density"))
    for k in ("sdf", "normal", "density"):
        assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k}: two calls differ"
    assert np.array_equal(_bits(got["normal"]), _bits(field.sdf_normal(x, want="normal")["normal"])), "the request for density changes the gradient"
    _compare(f"reference architecture N = {n}", got, o64, o32, n)
    if n == N_MAX:
        norm = np.linalg.norm(o64["normal"], axis=1)
        print(f"gradient norm {norm.min():.3f} .. {norm.max():.3f}")
        assert o64["raw"].min() < -0.1 and o64["raw"].max() > 0.5 and norm.min() > 0.05


def test_softplus_branches():
    net = tfo.make_net(tfo.REFERENCE, 13, scale=2.0)
    xyz = tfo.box_points(257, 9)
    o64, o32 = _oracles(net, xyz)
    z = np.concatenate([p.reshape(-1) for p in o64["pre_geo"][:-1]]) * tfo.SOFTPLUS_BETA
    linear, tiny = float((z > 20).mean()), int((z < -80).sum())
    slope = 1 / (1 + np.exp(-np.clip(z, -700, 20)))
    middle = float(((slope > 0.01) & (slope < 0.99)).mean())
    print(f"float64 oracle's pre-activations: beta z > 20 (value linear, derivative 1) for {100 * linear:.1f} %, derivative in 0.01 .. 0.99 for "
          f"{100 * middle:.1f} %, beta z < -80 for {tiny} of {z.size}")
    assert 0.05 <= linear <= 0.95 and tiny > 0 and middle > 0.01
    _compare("softplus on both branches", _field(net).sdf_normal(_t(xyz)), o64, o32)


@pytest.mark.parametrize("keep", ["embedding columns only", "embedding columns zero"])
def test_tangent_flows_through_both_inputs_of_the_skip_layer(keep):
    net = tfo.make_net(tfo.REFERENCE, 14)
    v, g, b = net["geo"][4]
    v = v.copy()
    assert v.shape == (256, 256 + 39)
    if keep == "embedding columns only":
        v[:, :256] = 0.0
    else:
        v[:, 256:] = 0.0
    net["geo"][4] = (v, g, b)
    xyz = tfo.box_points(130, 10)
    o64, o32 = _oracles(net, xyz)
    assert np.abs(o64["pre_geo"][4]).max() > 1e-2 and np.abs(o64["normal"]).max() > 1e-2
    _compare(f"skip layer, {keep}", _field(net).sdf_normal(_t(xyz)), o64, o32)


def test_narrow_softplus_net():
    net = tfo.make_net(tfo.NARROW, 15)
    xyz = tfo.box_points(130, 11)
    _compare("narrow softplus net", _field(net).sdf_normal(_t(xyz)), *_oracles(net, xyz))


def test_narrow_relu_net():
    net = tfo.make_net(tfo.NARROW, 15, geo_activation="relu")
    xyz = tfo.box_points(130, 11)
    o64, o32 = _oracles(net, xyz)
    pre_err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(o32["pre_geo"][:-1], o64["pre_geo"][:-1]))
    margin = 8 * pre_err
    closest = np.min([np.abs(p).min(axis=1) for p in o64["pre_geo"][:-1]], axis=0)
    keep = closest >= margin
    print(f"ReLU: the float32 oracle's largest pre-activation error {pre_err:.3e}, margin {margin:.3e}, {int((~keep).sum())} of {len(keep)} points left out")
    assert (~keep).sum() <= 0.05 * len(keep), "more than 5 % of the points sit on a ReLU kink"
    got = _field(net).sdf_normal(_t(xyz))
    _compare("narrow ReLU net", got, o64, o32, keys=("sdf",))
    _compare("narrow ReLU net (off the kinks)", got, o64, o32, keys=("normal",), keep=keep)


def test_view_directions_play_no_part():
    xyz = tfo.box_points(130, 11)
    plain, view = tfo.make_net(tfo.NARROW, 15), tfo.make_net(tfo.NARROW, 15, use_viewdir=True)
    for (va, ga, ba), (vb, gb, bb) in zip(plain["geo"], view["geo"]):
        assert np.array_equal(va, vb) and np.array_equal(ga, gb) and np.array_equal(ba, bb)
    fv = _field(view)
    assert fv.use_viewdir and fv.layers[7][4] == 2
    a, b = _field(plain).sdf_normal(_t(xyz), want=("sdf", "normal", "density")), fv.sdf_normal(_t(xyz), want=("sdf", "normal", "density"))
    for k in ("sdf", "normal", "density"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{k}: a field with use_viewdir differs"
    _compare("use_viewdir field", b, *_oracles(view, xyz))


@pytest.mark.parametrize("arch,seed", [(MULTIRES_0, 20), (MULTIRES_10, 21)], ids=["multires 0", "multires 10"])
def test_smallest_and_largest_embedding(arch, seed):
    net = tfo.make_net(arch, seed)
    field = _field(net)
    assert field.layers[0][1] == 3 + 6 * arch["multires"]
    xyz = tfo.box_points(130, 13)
    o64, o32 = _oracles(net, xyz)
    norm = np.linalg.norm(o64["normal"], axis=1)
    print(f"multires {arch['multires']}: gradient norm {norm.min():.3f} .. {norm.max():.3f}")
    assert norm.max() > 0.1
    x = _t(xyz)
    got = field.sdf_normal(x)
    assert np.array_equal(_bits(got["sdf"]), _bits(field(x)["sdf"]))
    _compare(f"multires {arch['multires']}", got, o64, o32)


def test_no_points_argument_errors_and_views():
    import torch
    net = tfo.make_net(tfo.NARROW, 18)
    field = _field(net)
    out = field.sdf_normal(torch.empty((0, 3), device="cuda"), want=("sdf", "normal", "density"))
    assert out["sdf"].shape == (0, 1) and out["normal"].shape == (0, 3) and out["density"].shape == (0, 1) and out["cano_xyz"].shape == (0, 3)
    assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in out.values())
    assert field.surface_normals(torch.empty((0, 3), device="cuda")).shape == (0, 3)
    x = _t(tfo.box_points(5, 1))
    for bad in (lambda: field.sdf_normal(x.cpu()), lambda: field.sdf_normal(x.double()), lambda: field.sdf_normal(x[:, :2]),
                lambda: field.sdf_normal(x.reshape(-1)), lambda: field.sdf_normal(x.cpu().numpy()), lambda: field.sdf_normal(x, want=("color",)),
                lambda: field.sdf_normal(x, want=("sdf", "normals")), lambda: field.surface_normals(x.cpu()), lambda: field.surface_normals(x.double()),
                lambda: field(x, want=("normal",))):
        with pytest.raises(ValueError):
            bad()
    for call in (lambda: field.sdf_normal(x.cpu()), lambda: field(x.cpu())):          # the messages of __call__
        with pytest.raises(ValueError, match="xyz must be a tensor on the GPU"):
            call()
    with pytest.raises(ValueError, match=r"xyz must be float32 \[N, 3\]"):
        field.sdf_normal(x.double())
    # a non-contiguous view is taken
    y = torch.stack([x, x], 1)[:, 1]
    assert not y.is_contiguous()
    a, b = field.sdf_normal(y), field.sdf_normal(x)
    assert np.array_equal(_bits(a["normal"]), _bits(b["normal"])) and np.array_equal(_bits(a["sdf"]), _bits(b["sdf"]))
    # eikonal_loss on the device, against its formula on the host
    from animatablegaussians_amd.template_field import eikonal_loss
    loss = eikonal_loss(b["normal"])
    want = tgo.eikonal(b["normal"].cpu().numpy())
    assert loss.is_cuda and loss.shape == () and abs(float(loss) - want) <= 8 * 2.0 ** -24 * max(1.0, want)


def test_surface_normals_on_the_extracted_mesh():
    import torch
    net = tfo.make_net(tfo.NARROW, 4, trained=False)             # geometric initialisation: an approximate sphere
    field = _field(net)
    bounds = np.array([[-1, -1, -1], [1, 1, 1]], np.float32)
    v, f, mesh_n = field.extract_mesh(bounds, (48, 48, 48))
    got = field.surface_normals(v)
    assert got.shape == v.shape and got.is_cuda and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    length = np.linalg.norm(g, axis=1)
    print(f"{len(g)} vertices: |unit normal| - 1 within {np.abs(length - 1).max():.3e} (bar {4 * 2.0 ** -24:.3e})")
    assert np.abs(length - 1).max() <= 4 * 2.0 ** -24
    m = mesh_n.cpu().numpy().astype(np.float64)
    cos = (g * m).sum(1) / np.maximum(np.linalg.norm(m, axis=1), 1e-30)
    print(f"cosine with extract_mesh's normals: min {cos.min():.4f}, median {np.median(cos):.4f}")
    assert cos.min() > 0, "surface_normals and extract_mesh's normals point to opposite sides"
    o64, o32 = _oracles(net, v.cpu().numpy())
    u64, u32 = tgo.unit(o64["normal"]), tgo.unit(o32["normal"].astype(np.float64))
    own = float(np.abs(u32 - u64).max())
    bar = 4 * own + 2.0 ** -22 * float(np.abs(u64).max())
    dev = float(np.abs(g - u64).max())
    print(f"surface_normals: |gpu - normalised float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
    assert dev <= bar
    radial = (u64 * tgo.unit(v.cpu().numpy().astype(np.float64))).sum(1)
    assert radial.min() > 0.5, "the oracle's gradient does not point out of the sphere"
