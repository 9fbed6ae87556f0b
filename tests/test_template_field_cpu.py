"""Host-side checks of the template field (``template_field.py``, ``include/ag_template_field.h``): the oracle against the reference's own
modules (``tests/golden/template_field_ref.npz``, written by ``make_golden_template_field.py``), state-dict loading and the weight-norm
fold, the packed blob, the grid points and the binding table.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_oracle as tfo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "template_field_ref.npz")
HEADER = os.path.join(ROOT, "include", "ag_template_field.h")


@pytest.mark.parametrize("use_viewdir", [False, True])
def test_oracle_equals_the_reference_modules(use_viewdir):
    fx = np.load(FIXTURE)
    tag = "view" if use_viewdir else "plain"
    net = tfo.make_net(tfo.REFERENCE, int(fx["seed"]), use_viewdir=use_viewdir)
    o64 = tfo.forward(net, fx["xyz"], fx["viewdirs"], torch.float64)
    o32 = tfo.forward(net, fx["xyz"], fx["viewdirs"], torch.float32)
    for k in ("sdf", "density", "color"):
        f64, f32 = fx[f"{tag}_{k}64"], fx[f"{tag}_{k}32"]
        assert f64.dtype == np.float64 and f32.dtype == np.float32 and o64[k].shape == f64.shape
        rel = float(np.abs(o64[k] - f64).max() / np.abs(f64).max())
        own = float(np.abs(f32.astype(np.float64) - f64).max())
        d32 = float(np.abs(o32[k].astype(np.float64) - f32).max())
        print(f"{tag} {k}: float64 oracle - fixture {rel:.2e} of the largest value; float32 oracle - fixture {d32:.3e}, the fixture's own {own:.3e}")
        assert rel <= 1e-12
        assert own > 0 and d32 <= 4 * own
    raw = -fx[f"{tag}_sdf64"]
    assert raw.min() < -0.1 and raw.max() > 0.5 and (fx[f"{tag}_density64"] > 1e-3).sum() > 20, "the fixture does not cross the surface"


def _field(net, **kw):
    from animatablegaussians_amd.template_field import TemplateField
    arch = net["arch"]
    return TemplateField.from_state_dict(tfo.state_dict(net, kw.pop("spelling", "weight_g")), multires=arch["multires"], use_viewdir=net["use_viewdir"],
                                         multires_viewdir=arch["multires_viewdir"], geo_activation=net["geo_activation"], **kw)


def test_both_weight_norm_spellings_fold_to_the_same_matrices():
    net = tfo.make_net(tfo.REFERENCE, 2, use_viewdir=True)
    a, b = _field(net), _field(net, spelling="parametrizations")
    want_geo, want_color = tfo.folded_layers(net)
    assert len(a.geo) == 7 and len(a.color) == 4
    for (wa, ba), (wb, bb), (ww, bw) in zip(a.geo + a.color, b.geo + b.color, want_geo + want_color):
        assert wa.dtype == np.float32 and np.array_equal(wa, wb) and np.array_equal(ba, bb) and np.array_equal(wa, ww) and np.array_equal(ba, bw)
    assert [r[4] for r in a.layers] == [1, 0, 0, 0, 1, 0, 0, 2, 0, 0, 0] and [r[1] for r in a.layers][:5] == [39, 512, 256, 256, 295] and a.layers[7][1] == 277
    assert a.density_b == float(np.float32(0.01) + np.float32(1e-4)) and np.array_equal(a.blob, b.blob)


def test_fold_equals_torch_weight_norm():
    """torch's own forward (``v * (g / ||v||)`` in float32) is at most 3 roundings and a float32 norm away from the exact quotient; the
    fold here is one rounding away.  Bar per element: (4 + log2 K) * 2^-24 * |W|, log2 K for a pairwise-summed norm of K squares."""
    net = tfo.make_net(tfo.REFERENCE, 3)
    f = _field(net)
    for l, (v, g, b) in enumerate(net["geo"]):
        lin = torch.nn.utils.weight_norm(torch.nn.Linear(v.shape[1], v.shape[0]))
        with torch.no_grad():
            lin.weight_g.copy_(torch.from_numpy(g))
            lin.weight_v.copy_(torch.from_numpy(v))
            x = torch.zeros(1, v.shape[1])
            lin(x)                                       # the forward pre-hook recomputes lin.weight
            w_torch = lin.weight.detach().numpy().astype(np.float64)
        w = f.geo[l][0].astype(np.float64)
        ulps = float((np.abs(w - w_torch) / np.maximum(np.abs(w), 1e-30)).max() / 2.0 ** -24)
        print(f"layer {l} {v.shape}: fold - torch's weight_norm at most {ulps:.2f} x 2^-24 of the element")
        assert ulps <= 4 + np.log2(v.shape[1])


def test_missing_and_misshaped_keys_are_named():
    from animatablegaussians_amd.template_field import TemplateField
    net = tfo.make_net(tfo.NARROW, 1, use_viewdir=True)
    good = tfo.state_dict(net)
    TemplateField.from_state_dict(good, multires=2, use_viewdir=True)
    for key in ("geo_mlp.fc_list.2.0.weight_g", "geo_mlp.fc_list.2.0.bias", "geo_mlp.fc_list.6.weight_v", "tex_mlp.fc_list.0.0.bias", "density_func.beta"):
        sd = dict(good)
        del sd[key]
        with pytest.raises(KeyError, match=re.escape(key)):
            TemplateField.from_state_dict(sd, multires=2, use_viewdir=True)
    sd = {k: v for k, v in good.items() if not k.startswith("tex_mlp.fc_list.1.")}
    with pytest.raises(KeyError, match=re.escape("tex_mlp.fc_list.1.")):
        TemplateField.from_state_dict(sd, multires=2, use_viewdir=True)
    sd = dict(good)
    sd["geo_mlp.fc_list.1.0.weight"] = sd.pop("geo_mlp.fc_list.1.0.weight_v")       # a plain linear inside the weight-normalised net
    with pytest.raises(KeyError, match=re.escape("geo_mlp.fc_list.1.0.weight_")):
        TemplateField.from_state_dict(sd, multires=2, use_viewdir=True)
    for key, shape, word in (("geo_mlp.fc_list.3.0.weight_g", (31, 1), "geo_mlp.fc_list.3.0.weight_g"), ("geo_mlp.fc_list.3.0.bias", (31,), "geo_mlp.fc_list.3.0.bias"),
                             ("geo_mlp.fc_list.3.0.weight_v", (32, 31), "geo_mlp.fc_list.3"), ("geo_mlp.fc_list.4.0.weight_v", (32, 35), "geo_mlp.fc_list.4"),
                             ("tex_mlp.fc_list.1.weight", (4, 32), "tex_mlp.fc_list.1"), ("tex_mlp.fc_list.0.0.weight", (32, 32), "tex_mlp.fc_list.0"),
                             ("density_func.beta", (2,), "density_func.beta")):
        sd = dict(good)
        sd[key] = torch.zeros(shape)
        if key.endswith("weight_v"):                                                   # keep g and bias consistent: the input width is what is wrong
            sd[key] = torch.ones(shape)
        with pytest.raises(ValueError, match=re.escape(word)):
            TemplateField.from_state_dict(sd, multires=2, use_viewdir=True)
    with pytest.raises(ValueError, match=re.escape("geo_mlp.fc_list.0")):                           # the wrong multires: layer 0 does not take 3 + 6 * 3 columns
        TemplateField.from_state_dict(good, multires=3, use_viewdir=True)
    with pytest.raises(ValueError, match=re.escape("tex_mlp.fc_list.0")):
        TemplateField.from_state_dict(good, multires=2, use_viewdir=False)


@pytest.mark.parametrize("arch,use_viewdir", [("REFERENCE", True), ("REFERENCE", False), ("NARROW", True)])
def test_packed_blob_round_trips(arch, use_viewdir):
    net = tfo.make_net(getattr(tfo, arch), 4, use_viewdir=use_viewdir)
    f = _field(net)
    layers, padding = f.unpack()
    for (w, b), (uw, ub) in zip(f.geo + f.color, layers):
        assert np.array_equal(w, uw) and np.array_equal(b, ub)
    assert padding.size > 0 and not padding.any(), "padding of the blob is not zero"
    assert f.blob.size == sum(w.size + b.size for w, b in f.geo + f.color) + padding.size
    # the last geometry layer: features first, the SDF column alone in the last 32-column tile
    layout, total = f._layout()
    Ka, e_cols, Ke, Np, w_off, b_off = layout[len(f.geo) - 1]
    rows = f.blob[w_off:b_off].reshape((Ka + Ke) // 4, Np, 4)
    w_last, b_last = f.geo[-1]
    assert np.array_equal(rows[:, Np - 32, :].reshape(-1)[:Ka], w_last[0]) and f.blob[b_off + Np - 32] == b_last[0]
    assert np.array_equal(rows[:, 5, :].reshape(-1)[:Ka], w_last[6]) and not rows[:, Np - 31:, :].any()
    if arch == "REFERENCE":
        print(f"blob of the reference architecture (use_viewdir {use_viewdir}): {4 * total} bytes")
        assert 2.7e6 < 4 * total < 3.0e6
    # the library lays the same table out to the same size (host code: no GPU needed)
    from animatablegaussians_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.ag_template_field_blob_floats.restype = ctypes.c_size_t
    L.ag_template_field_desc_bytes.restype = ctypes.c_size_t
    d = f.desc()
    assert L.ag_template_field_desc_bytes() == ctypes.sizeof(_lib.AgTemplateFieldDesc) == 24 + 2 * 8 * 16
    assert L.ag_template_field_blob_floats(ctypes.byref(d)) == total
    d.geo[1].width = 250
    assert L.ag_template_field_blob_floats(ctypes.byref(d)) == 0


@pytest.mark.parametrize("res", [(5, 4, 3), (33, 17, 9)])
def test_grid_points_equal_generate_volume_points(res):
    from animatablegaussians_amd.template_field import volume_axes, volume_points
    bounds = np.array([[-0.93, -1.27, -0.31], [0.89, 0.77, 0.42]], np.float32)
    want = tfo.volume_points(bounds, res)
    axes = volume_axes(bounds, res)
    got = volume_points(axes, 0, res[0]).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    slabs = np.concatenate([volume_points(axes, x0, min(res[0], x0 + 2)).numpy() for x0 in range(0, res[0], 2)])
    assert np.array_equal(slabs.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(volume_points(volume_axes(torch.from_numpy(bounds), res), 0, res[0]).numpy(), want)


def test_abi_symbols_match_the_header():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^(?:int|size_t)\s+(ag_\w+)\s*\(", hdr, flags=re.M)
    assert set(names) == {"ag_template_field_desc_bytes", "ag_template_field_blob_floats", "ag_template_field_forward"}
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in table and hasattr(L, name), name
    assert len(table["ag_template_field_forward"][2]) == 10
    from animatablegaussians_amd import template_field as tf
    for word, value in (("AG_FIELD_ACT_SOFTPLUS", tf.ACT_SOFTPLUS), ("AG_FIELD_ACT_RELU", tf.ACT_RELU), ("AG_FIELD_ACT_SIGMOID", tf.ACT_SIGMOID),
                        ("AG_FIELD_CONCAT_POSITION", tf.CONCAT_POSITION), ("AG_FIELD_CONCAT_VIEW", tf.CONCAT_VIEW)):
        assert re.search(word + r"\s*=\s*" + str(value) + r"\b", hdr), word
    assert re.search(r"#define AG_FIELD_MAX_LAYERS\s+8\b", hdr) and _lib.AG_FIELD_MAX_LAYERS == tf.MAX_LAYERS == 8
    import animatablegaussians_amd as pkg
    assert pkg.TemplateField is tf.TemplateField
