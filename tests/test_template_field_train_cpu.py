"""Host-side checks of the template field's training path (``template_train.py``, ``include/ag_template_field_train.h``): the header, the
binding table and the library's exports; the refusals, which fire before any launch and need no device; the two blobs as gathers
against ``TemplateField.pack()``; the state dict's round trips; the geometric initialisation.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_oracle as tfo  # noqa: E402
import template_field_train_oracle as tto  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ag_template_field_train.h")
NAMES = {"ag_template_field_train_slab", "ag_template_field_train_blob_t_floats", "ag_template_field_train_stash_floats",
         "ag_template_field_train_workspace_floats", "ag_template_field_train_forward", "ag_template_field_train_backward"}


def _module(arch, use_viewdir, seed=3, spelling="weight_g", **kw):
    from animatablegaussians_amd.template_train import TemplateFieldModule
    net = tfo.make_net(arch, seed=seed, use_viewdir=use_viewdir, **kw)
    return net, TemplateFieldModule.from_state_dict(tfo.state_dict(net, spelling), arch["multires"], use_viewdir, arch["multires_viewdir"])


def test_abi_symbols_match_the_header():
    from animatablegaussians_amd import _lib, template_train
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^(?:int|size_t|int64_t)\s+(ag_\w+)\s*\(", hdr, flags=re.M)
    assert set(names) == NAMES and len(names) == len(NAMES)
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in table and hasattr(L, name), name
    assert len(table["ag_template_field_train_forward"][2]) == 11 and len(table["ag_template_field_train_backward"][2]) == 13
    slab = int(re.search(r"#define AG_FIELD_TRAIN_SLAB\s+(\d+)\b", hdr).group(1))
    assert slab == template_train.SLAB == _lib.lib().ag_template_field_train_slab()
    import animatablegaussians_amd as pkg
    assert pkg.TemplateFieldModule is template_train.TemplateFieldModule and "TemplateFieldModule" in pkg.__all__


@pytest.mark.parametrize("arch, use_viewdir", [(tfo.NARROW, False), (tfo.NARROW, True), (tfo.REFERENCE, False), (tfo.REFERENCE, True)])
def test_sizes_follow_the_header(arch, use_viewdir):
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.template_train import SLAB
    _, m = _module(arch, use_viewdir)
    L, d = _lib.lib(), m.plan.desc()
    pad = lambda v, k: (v + k - 1) // k * k  # noqa: E731
    widths = [w for _, _, w, *_ in m.plan.layers]
    layout, total = m.plan._layout()
    ep, ev = pad(3 + 6 * arch["multires"], 8), pad(3 + 6 * arch["multires_viewdir"], 8) if use_viewdir else 0
    nps = [pad(w, 32) for w in widths]
    N = SLAB + 33
    assert L.ag_template_field_train_stash_floats(ctypes.byref(d), N) == N * (ep + ev + sum(nps))
    assert L.ag_template_field_train_blob_t_floats(ctypes.byref(d)) == sum(Np * Ka for (Ka, _, _, Np, _, _) in layout) == m._idx_t.size
    partial = max(Np * (Ka + Ke) + Np for (Ka, _, Ke, Np, _, _) in layout)
    assert L.ag_template_field_train_workspace_floats(ctypes.byref(d), N) == 2 * N * max(nps) + 2 * partial
    assert L.ag_template_field_train_workspace_floats(ctypes.byref(d), 0) == 0 and m._idx_fwd.size == total
    if arch is tfo.REFERENCE and use_viewdir:
        assert ep + ev + sum(nps) == 2944          # 11.8 KB per point


def test_refusals_fire_before_any_launch():
    """Every call below must return AG_ERR_INVALID_ARGUMENT (-1) with a message: the pointers are made-up addresses, so a call that got
    as far as a launch (or a read) would not come back with -1."""
    from animatablegaussians_amd import _lib
    _, m = _module(tfo.NARROW, True)
    L, d = _lib.lib(), m.plan.desc()
    N = 40
    blob, blob_t = m._idx_fwd.size, m._idx_t.size
    stash, ws = L.ag_template_field_train_stash_floats(ctypes.byref(d), N), L.ag_template_field_train_workspace_floats(ctypes.byref(d), N)
    p = lambda a=1 << 20: ctypes.c_void_p(a)  # noqa: E731
    null = ctypes.c_void_p(None)

    def fwd(desc=d, blob_p=p(), blob_n=blob, n=N, stash_p=p(), stash_n=stash, sdf=p(), color=p(), xyz=p()):
        return L.ag_template_field_train_forward(ctypes.byref(desc), blob_p, blob_n, xyz, null, n, stash_p, stash_n, sdf, color, null)

    def bwd(desc=d, bt_p=p(), bt_n=blob_t, stash_p=p(), stash_n=stash, n=N, ws_p=p(), ws_n=ws, gw=p(), gb=p(), g_color=p()):
        return L.ag_template_field_train_backward(ctypes.byref(desc), bt_p, bt_n, stash_p, stash_n, p(), g_color, n, ws_p, ws_n, gw, gb, null)

    wide = m.plan.desc()
    wide.geo[1].width = 48                                                 # not a multiple of 32
    deep = m.plan.desc()
    deep.n_geo = 9
    no_color = m.plan.desc()
    no_color.n_color = 0
    cases = {
        "forward, N < 0": lambda: fwd(n=-1), "forward, N > 2^31 - 1": lambda: fwd(n=1 << 31),
        "forward, blob size": lambda: fwd(blob_n=blob - 1), "forward, stash size": lambda: fwd(stash_n=stash + 1),
        "forward, blob misaligned": lambda: fwd(blob_p=p((1 << 20) + 4)), "forward, stash misaligned": lambda: fwd(stash_p=p((1 << 20) + 8)),
        "forward, blob NULL": lambda: fwd(blob_p=null), "forward, stash NULL": lambda: fwd(stash_p=null), "forward, sdf NULL": lambda: fwd(sdf=null),
        "forward, xyz NULL": lambda: fwd(xyz=null), "forward, width": lambda: fwd(desc=wide), "forward, layers": lambda: fwd(desc=deep),
        "forward, colour without a colour MLP": lambda: fwd(desc=no_color),
        "backward, N < 0": lambda: bwd(n=-1), "backward, transposed blob size": lambda: bwd(bt_n=blob_t + 4),
        "backward, stash size": lambda: bwd(stash_n=stash - 1), "backward, workspace size": lambda: bwd(ws_n=ws - 1),
        "backward, transposed blob misaligned": lambda: bwd(bt_p=p((1 << 20) + 4)), "backward, workspace misaligned": lambda: bwd(ws_p=p((1 << 20) + 4)),
        "backward, stash misaligned": lambda: bwd(stash_p=p((1 << 20) + 4)), "backward, g_weight NULL": lambda: bwd(gw=null),
        "backward, g_bias NULL": lambda: bwd(gb=null), "backward, width": lambda: bwd(desc=wide),
        "backward, colour without a colour MLP": lambda: bwd(desc=no_color),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.ag_last_error().decode()
        assert rc == -1 and msg, f"{what}: code {rc}, message {msg!r}"
    for fn in (L.ag_template_field_train_stash_floats, L.ag_template_field_train_workspace_floats):
        assert fn(ctypes.byref(d), -1) == 0 and fn(ctypes.byref(wide), N) == 0
    assert L.ag_template_field_train_blob_t_floats(ctypes.byref(wide)) == 0
    # N == 0: the forward returns 0 without a launch (its sizes are still checked)
    assert fwd(n=0, stash_n=0, stash_p=null) == 0 and fwd(n=0, stash_n=0, stash_p=null, blob_n=blob + 1) == -1


@pytest.mark.parametrize("arch", [tfo.NARROW, tfo.REFERENCE], ids=["narrow", "reference"])
@pytest.mark.parametrize("use_viewdir", [False, True])
def test_index_maps_pack_what_the_field_packs(arch, use_viewdir):
    from animatablegaussians_amd.template_field import TemplateField
    net, m = _module(arch, use_viewdir)
    layers = [(w.detach().numpy(), b.detach().numpy()) for w, b in m.folded_weights()]
    n_geo = len(net["geo"])
    f = TemplateField(layers[:n_geo], layers[n_geo:], arch["multires"], use_viewdir, arch["multires_viewdir"])
    blob, blob_t = m.pack()
    assert blob.dtype == torch.float32 and np.array_equal(blob.numpy().view(np.uint32), f.blob.view(np.uint32))
    back = m.unpack_transposed(blob_t.numpy())
    seen = 0
    for (w, _), (_, K, width, _, _, prev), wt in zip(layers, f.layers, back):
        if prev == 0:
            assert wt is None
            continue
        assert wt.shape == (prev, width) and np.array_equal(wt.view(np.uint32), np.ascontiguousarray(w[:, :prev].T).view(np.uint32))
        seen += 1
    assert seen == len(layers) - 1
    # every element of the transposed blob that is not a weight is the zero slot
    zero = m._n_weights + m._n_biases
    assert int((m._idx_t != zero).sum()) == sum(width * prev for _, _, width, _, _, prev in f.layers)
    assert m._idx_t.max() <= zero and m._idx_fwd.max() <= zero and len(set(m._idx_fwd[m._idx_fwd != zero].tolist())) == zero


@pytest.mark.parametrize("spelling", ["weight_g", "parametrizations"])
def test_state_dict_round_trips(spelling):
    from animatablegaussians_amd.template_field import TemplateField
    from animatablegaussians_amd.template_train import TemplateFieldModule
    arch = tfo.NARROW
    net, m = _module(arch, True, spelling=spelling)
    sd = m.state_dict()
    want = tfo.state_dict(net, "weight_g")
    assert list(sd) == list(want)
    for k in want:
        assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]), k
    # the inference field reads it: the float64 fold of the same parameters
    geo, color = tfo.folded_layers(net)
    f = TemplateField.from_state_dict(sd, arch["multires"], True, arch["multires_viewdir"])
    for (w, b), (w0, b0) in zip(f.geo + f.color, geo + color):
        assert np.array_equal(w, w0) and np.array_equal(b, b0)
    assert f.density_beta == float(net["beta"])
    again = TemplateFieldModule.from_state_dict(sd, arch["multires"], True, arch["multires_viewdir"])
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), sd.values()))
    assert m.beta is m.density_func.beta and m.beta.numel() == 1
    assert set(dict(m.named_parameters())) == set(sd)
    # the fp32 fold is torch's weight_norm
    for (w, _), (v, g, _) in zip(m.folded_weights(), net["geo"]):
        assert torch.equal(w.detach(), tfo.fold(v, g, torch.float32))


def test_geometric_init_has_the_reference_statistics():
    from animatablegaussians_amd.template_train import TemplateFieldModule
    arch = tfo.REFERENCE
    kw = dict(multires=arch["multires"], widths=arch["widths"], out=arch["out"], skip=arch["skip"], color=arch["color"], use_viewdir=True,
              multires_viewdir=arch["multires_viewdir"])
    m = TemplateFieldModule.geometric_init(generator=torch.Generator().manual_seed(5), **kw)
    same = TemplateFieldModule.geometric_init(generator=torch.Generator().manual_seed(5), **kw)
    other = TemplateFieldModule.geometric_init(generator=torch.Generator().manual_seed(6), **kw)
    sd = m.state_dict()
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), same.state_dict().values()))
    assert not torch.equal(sd["geo_mlp.fc_list.1.0.weight_v"], other.state_dict()["geo_mlp.fc_list.1.0.weight_v"])
    e = 3 + 6 * arch["multires"]
    lins = m.geo_mlp.linears()
    assert [tuple(l.weight_v.shape) for l in lins] == [(512, e), (256, 512), (256, 256), (256, 256), (256, 256 + e), (256, 256), (257, 256)]
    v0, vs, vl = lins[0].weight_v.detach(), lins[4].weight_v.detach(), lins[-1].weight_v.detach()
    assert not v0[:, 3:].any() and v0[:, :3].all()
    assert not vs[:, -(e - 3):].any() and vs[:, :-(e - 3)].all()
    for l, lin in enumerate(lins[:-1]):
        v = lin.weight_v.detach()
        live = v[:, :3] if l == 0 else v[:, :-(e - 3)] if l == 4 else v
        std = np.sqrt(2) / np.sqrt(v.shape[0])
        assert abs(float(live.std()) / std - 1) < 0.05 and abs(float(live.mean())) < 4 * std / np.sqrt(live.numel()), l
        assert not lin.bias.detach().any()
        assert torch.equal(lin.weight_g.detach(), v.norm(dim=1, keepdim=True))
    mean = np.sqrt(np.pi) / np.sqrt(256)
    assert abs(float(vl.mean()) - mean) < 4 * 1e-4 / np.sqrt(vl.numel()) + 1e-7 and abs(float(vl.std()) / 1e-4 - 1) < 0.05
    assert torch.equal(lins[-1].bias.detach(), torch.full((257,), -0.7)) and torch.equal(lins[-1].weight_g.detach(), vl.norm(dim=1, keepdim=True))
    assert float(TemplateFieldModule.geometric_init(bias=0.5, generator=torch.Generator().manual_seed(1)).geo_mlp.linears()[-1].bias.detach()[0]) == -0.5
    tex = m.tex_mlp.linears()
    assert [tuple(l.weight.shape) for l in tex] == [(256, 256 + 21), (256, 256), (256, 256), (3, 256)]
    for lin in tex:
        bound, w, b = 1 / np.sqrt(lin.weight.shape[1]), lin.weight.detach(), lin.bias.detach()
        assert float(w.abs().max()) <= bound and float(b.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    # the initial field is about a sphere of radius `bias`: inside positive, outside negative
    f64 = tto.field({k: v.double() for k, v in sd.items() if k != "density_func.beta"}, dict(tfo.make_net(arch, use_viewdir=True), geo_activation="softplus"),
                    torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.3, 0.0], [1.2, 0.0, 0.0]], dtype=torch.float64), None)[0].reshape(-1)
    assert f64[0] > 0.3 and f64[1] > 0.1 and f64[2] < -0.2, f64
