"""The fused template-field kernel (``include/ag_template_field.h``, ``template_field.TemplateField``) against ``template_field_oracle.py``.

Bars, from the oracle alone: for every output, |gpu - float64 oracle| <= 4 x max|float32 oracle - float64 oracle| + 2^-22 x max|float64 oracle|.
The factor 4 is ``test_isosurface_gpu.py``'s, for the same reason: the kernel's fp32 summation order (header: groups of 8 k, interleaved)
and the device's libm are different from, and as valid as, the float32 oracle's.  Density has its own bar from its own oracle values (it
amplifies an SDF error by up to 1 / b^2).  The maxima are taken over the oracle's whole point set of a case (computed once, shared by
the sizes that are prefixes of it): the bar describes the fp32 error of this computation over that point distribution, which the
float32 oracle's error at one single point (N = 1) does not estimate.  The oracle folds weight normalisation in the precision it runs in;
the kernel's weights are folded in float64 and rounded once.  Every test prints measured deviation and bar.

Measured on the MI355X, deviation from the float64 oracle / bar (the table of DESIGN.md's "Template field" section has every case):
reference architecture at N = 4099: sdf 1.08e-6 / 4.12e-6, density 2.45e-3 / 3.56e-3, colour 6.7e-8 / 3.96e-7, the sdf of the two requests
bit-identical at every N; use_viewdir: 9.1e-7 / 3.69e-6, 4.7e-4 / 4.06e-3, 6.6e-8 / 3.51e-7, None == zeros bit for bit; softplus on both
branches (32.2 % linear, 85 463 entries below -80): sdf 4.72e-5 / 1.65e-4, colour 4.0e-7 / 1.33e-6; skip layer: 4.85e-6 / 1.60e-5 and
7.8e-7 / 2.70e-6; narrow nets: sdf 9.1e-7 / 4.73e-6 (softplus), 7.3e-7 / 5.62e-6 (ReLU); s = 0, +-1e-6: sdf the bias bit for bit, density
equal to the float32 oracle's own 1.26e-7 .. 4.34e-6 (bars 1.2e-5 .. 2.9e-5); sdf_grid equal to field() bit for bit; chain at 48^3: 4188
vertices, 8372 faces, two faces per edge, Euler 2, radius 0.3733 .. 0.9071 inside 0.2085 .. 1.1004; 19 tests in 3 s.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isosurface_oracle as io  # noqa: E402
import template_field_oracle as tfo  # noqa: E402

pytestmark = pytest.mark.gpu
N_MAX = 4099


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


def _oracles(net, xyz, dirs=None):
    import torch
    o64, o32 = tfo.forward(net, xyz, dirs, torch.float64), tfo.forward(net, xyz, dirs, torch.float32)
    for o in (o64, o32):
        for v in o.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return o64, o32


def _compare(name, got, o64, o32, n=None, keys=("sdf", "density", "color")):
    """The bars of the module docstring on the first ``n`` points; on a miss, the first layer whose float32 oracle is not the culprit is
    found from ``o64['pre_geo']`` by hand -- the figures printed here say which output missed."""
    for k in keys:
        w64, w32 = o64[k], o32[k].astype(np.float64)
        own = float(np.abs(w32 - w64).max())
        bar = 4 * own + 2.0 ** -22 * float(np.abs(w64).max())
        g = got[k].detach().cpu().numpy().astype(np.float64)
        n_ = g.shape[0] if n is None else n
        assert g.shape == w64[:n_].shape, (k, g.shape, w64[:n_].shape)
        dev = float(np.abs(g - w64[:n_]).max()) if n_ else 0.0
        print(f"{name} {k}: |gpu - float64 oracle| {dev:.3e}, the float32 oracle's own {own:.3e}, bar {bar:.3e}")
        assert np.isfinite(g).all() and dev <= bar, f"{name} {k}: {dev:.3e} > {bar:.3e}"


@functools.lru_cache(maxsize=None)
def _reference_case():
    net = tfo.make_net(tfo.REFERENCE, 11)
    xyz = tfo.box_points(N_MAX, 5)
    return net, _field(net), xyz, _oracles(net, xyz)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, N_MAX])
def test_reference_architecture_and_tile_tails(n):
    net, field, xyz, (o64, o32) = _reference_case()
    x = _t(xyz[:n])
    only = field(x)
    full = field(x, want=("sdf", "density", "color"))
    assert set(only) == {"sdf", "cano_xyz"} and set(full) == {"sdf", "density", "color", "cano_xyz"}
    assert only["sdf"].shape == (n, 1) and full["density"].shape == (n, 1) and full["color"].shape == (n, 3) and full["cano_xyz"].shape == (n, 3)
    assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in full.values())
    assert np.array_equal(_bits(only["sdf"]), _bits(full["sdf"])), "the sdf of the two requests differs"
    assert np.array_equal(_bits(full["cano_xyz"]), _bits(x))
    _compare(f"reference architecture N = {n}", full, o64, o32, n)
    if n == N_MAX:
        raw = o64["raw"]
        assert raw.min() < -0.1 and raw.max() > 0.5 and (o64["density"] > 1e-3).sum() > 100, "the points do not cross the surface"


def test_view_directions_and_none_is_zeros():
    import torch
    net = tfo.make_net(tfo.REFERENCE, 12, use_viewdir=True)
    field = _field(net)
    n = 257
    xyz, dirs = tfo.box_points(n, 7), tfo.unit_dirs(n, 8)
    assert [r[1] for r in field.layers][7] == 277
    x = _t(xyz)
    want = ("sdf", "density", "color")
    _compare("use_viewdir, unit directions", field(x, _t(dirs), want), *_oracles(net, xyz, dirs))
    none = field(x, None, want)
    zeros = field(x, torch.zeros_like(x), want)
    _compare("use_viewdir, viewdirs = None", none, *_oracles(net, xyz, None))
    for k in want:
        assert np.array_equal(_bits(none[k]), _bits(zeros[k])), f"{k}: viewdirs = None differs from explicit zeros"
    assert not np.array_equal(_bits(none["color"]), _bits(field(x, _t(dirs), want)["color"]))


def test_softplus_branches():
    net = tfo.make_net(tfo.REFERENCE, 13, scale=2.0)
    xyz = tfo.box_points(257, 9)
    o64, o32 = _oracles(net, xyz)
    z = np.concatenate([p.reshape(-1) for p in o64["pre_geo"][:-1]]) * tfo.SOFTPLUS_BETA
    linear, tiny = float((z > 20).mean()), int((z < -80).sum())
    print(f"float64 oracle's pre-activations: beta x > 20 for {100 * linear:.1f} %, beta x < -80 for {tiny} of {z.size}")
    assert 0.05 <= linear <= 0.95 and tiny > 0
    _compare("softplus on both branches", _field(net)(_t(xyz), want=("sdf", "density", "color")), o64, o32)


@pytest.mark.parametrize("keep", ["embedding columns only", "embedding columns zero"])
def test_skip_layer_concatenates_the_embedding_last(keep):
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
    assert np.abs(o64["pre_geo"][4]).max() > 1e-2
    _compare(f"skip layer, {keep}", _field(net)(_t(xyz), want=("sdf", "density", "color")), o64, o32)


@pytest.mark.parametrize("activation,use_viewdir", [("softplus", False), ("relu", True)])
def test_narrow_architecture(activation, use_viewdir):
    net = tfo.make_net(tfo.NARROW, 15, use_viewdir=use_viewdir, geo_activation=activation)
    field = _field(net)
    assert [r[2] for r in field.layers] == [64, 32, 32, 32, 32, 32, 33, 32, 3] and field.multires == 2
    xyz, dirs = tfo.box_points(130, 11), tfo.unit_dirs(130, 12)
    got = field(_t(xyz), _t(dirs) if use_viewdir else None, want=("sdf", "density", "color"))
    _compare(f"narrow {activation} net", got, *_oracles(net, xyz, dirs if use_viewdir else None))


@pytest.mark.parametrize("bias", [0.0, 1e-6, -1e-6])
def test_density_at_and_around_zero(bias):
    net = tfo.make_net(tfo.NARROW, 16, density_beta=-0.01)
    v, g, b = net["geo"][-1]
    b = b.copy()
    b[0] = bias
    net["geo"][-1] = (v, np.zeros_like(g), b)                    # weight_g = 0: the folded last layer is zero, s is its bias exactly
    xyz = tfo.box_points(40, 13)
    o64, o32 = _oracles(net, xyz)
    s = np.float32(bias)
    assert (o64["raw"] == np.float64(s)).all() and o64["density"].min() > 40
    field = _field(net)
    assert field.density_b == float(np.float32(0.01) + np.float32(1e-4))          # the abs of a negative beta
    got = field(_t(xyz), want=("sdf", "density"))
    assert (_bits(got["sdf"]) == np.float32(-s).view(np.uint32)).all(), "s is not the bias exactly"
    _compare(f"s = {bias:g}, beta = -0.01", got, o64, o32, keys=("sdf", "density"))


@pytest.mark.parametrize("res", [(5, 4, 3), (33, 17, 9)])
def test_sdf_grid(res, monkeypatch):
    from animatablegaussians_amd import template_field as tf
    net = tfo.make_net(tfo.NARROW, 17)
    field = _field(net)
    bounds = np.array([[-0.93, -1.27, -0.31], [0.89, 0.77, 0.42]], np.float32)
    pts = tfo.volume_points(bounds, res)
    want = field(_t(pts))["sdf"]
    a = field.sdf_grid(bounds, res)
    assert a.is_cuda and tuple(a.shape) == res and str(a.dtype) == "torch.float32"
    assert np.array_equal(_bits(a).reshape(-1), _bits(want).reshape(-1)), "sdf_grid differs from field() at generate_volume_points' points"
    assert np.array_equal(_bits(a), _bits(field.sdf_grid(_t(bounds), res))), "two calls differ"
    monkeypatch.setattr(tf, "GRID_CHUNK", res[1] * res[2] * 4)              # slabs of 4 planes, the last one partial
    assert np.array_equal(_bits(a), _bits(field.sdf_grid(bounds, res))), "the slab size changes the grid"
    _compare(f"sdf_grid {res}", {"sdf": a.reshape(-1, 1)}, *_oracles(net, pts), keys=("sdf",))


def test_no_points_and_argument_errors():
    import torch
    net = tfo.make_net(tfo.NARROW, 18)
    field = _field(net)
    out = field(torch.empty((0, 3), device="cuda"), want=("sdf", "density", "color"))
    assert out["sdf"].shape == (0, 1) and out["density"].shape == (0, 1) and out["color"].shape == (0, 3) and out["cano_xyz"].shape == (0, 3)
    assert all(v.is_cuda and str(v.dtype) == "torch.float32" for v in out.values())
    x = _t(tfo.box_points(5, 1))
    for bad in (lambda: field(x.cpu()), lambda: field(x.double()), lambda: field(x[:, :2]), lambda: field(x.reshape(-1)), lambda: field(x.cpu().numpy()),
                lambda: field(x, want=("normal",)), lambda: field(x, x[:3]), lambda: field(x, x.cpu()), lambda: field(x, x.double()),
                lambda: field.sdf_grid(np.zeros((3, 2)), (4, 4, 4)), lambda: field.sdf_grid(np.zeros((2, 3)), (4, 4)),
                lambda: field.sdf_grid(np.zeros((2, 3)), (4, 4, 4), device="cpu")):
        with pytest.raises(ValueError):
            bad()
    # a non-contiguous view is taken
    y = torch.stack([x, x], 1)[:, 1]
    assert not y.is_contiguous() and np.array_equal(_bits(field(y)["sdf"]), _bits(field(x)["sdf"]))


def test_chain_to_a_closed_mesh():
    from animatablegaussians_amd.isosurface import recon_mesh
    net = tfo.make_net(tfo.NARROW, 4, trained=False)             # geometric initialisation: an approximate sphere
    field = _field(net)
    res = (48, 48, 48)
    bounds = np.array([[-1, -1, -1], [1, 1, 1]], np.float32)
    v, f, nrm = field.extract_mesh(bounds, res)
    v2, f2, n2 = recon_mesh(field.sdf_grid(bounds, res), res, bounds, iso_value=0.0)
    assert np.array_equal(_bits(v), _bits(v2)) and np.array_equal(f.cpu().numpy(), f2.cpu().numpy()) and np.array_equal(_bits(nrm), _bits(n2))
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    keys, counts, closed = io.directed_edge_census(fh)
    chi = io.euler_characteristics(fh, len(vh))
    e = np.sort(np.concatenate([fh[:, [0, 1]], fh[:, [1, 2]], fh[:, [2, 0]]]), axis=1)
    _, per_edge = np.unique(e[:, 0].astype(np.int64) * len(vh) + e[:, 1], return_counts=True)
    # nodes next to a sign change of the float64 oracle's grid
    pts = tfo.volume_points(bounds, res)
    o64, _ = _oracles(net, pts)
    inside = (o64["sdf"].reshape(res) >= 0)
    near = np.zeros(res, bool)
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        flip = inside[tuple(a)] != inside[tuple(b)]
        near[tuple(a)] |= flip
        near[tuple(b)] |= flip
    radius = np.linalg.norm(pts.astype(np.float64), axis=1).reshape(res)[near]
    diag = float(np.linalg.norm((bounds[1] - bounds[0]) / np.array(res, np.float32)))
    lo, hi = float(radius.min()) - 2 * diag, float(radius.max()) + 2 * diag
    r = np.linalg.norm(vh.astype(np.float64), axis=1)
    print(f"V {len(vh)}, F {len(fh)}, faces per edge {int(per_edge.min())} .. {int(per_edge.max())}, closed and oriented {closed}, Euler {chi}; vertex radius "
          f"{r.min():.4f} .. {r.max():.4f}, allowed {lo:.4f} .. {hi:.4f} ({int(near.sum())} nodes next to a sign change, radius {radius.min():.4f} .. {radius.max():.4f})")
    assert len(fh) > 1000 and (per_edge == 2).all() and closed and chi == [2]
    assert lo <= r.min() and r.max() <= hi
