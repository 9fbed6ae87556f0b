"""Host-side checks of the template field's gradient (``include/ag_template_field_grad.h``, ``TemplateField.sdf_normal``): the two
derivations of ``template_field_grad_oracle.py`` against each other and against the reference's own modules under ``compute_grad``
(``tests/golden/template_field_grad_ref.npz``, written by ``make_golden_template_field_grad.py``), the header, the binding row, the package
exports and ``eikonal_loss``.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_field_grad_oracle as tgo  # noqa: E402
import template_field_oracle as tfo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "template_field_grad_ref.npz")
HEADER = os.path.join(ROOT, "include", "ag_template_field_grad.h")
# multires 0 without a skip layer: make_net's geometric initialisation zeroes the skip layer's columns [-(e_pos - 3):], all of them at e_pos = 3
PLAIN_0 = dict(tfo.NARROW, multires=0, skip=())
RELU_SKIP = dict(multires=3, widths=(64, 32, 32), out=33, skip=(2,), color=(32,), multires_viewdir=3)


@pytest.mark.parametrize("case", ["reference", "softplus branches", "narrow relu", "relu skip at 2", "multires 0"])
def test_autograd_equals_the_written_out_tangents(case):
    net, xyz = {
        "reference": lambda: (tfo.make_net(tfo.REFERENCE, 11), tfo.box_points(257, 5)),
        "softplus branches": lambda: (tfo.make_net(tfo.REFERENCE, 13, scale=2.0), tfo.box_points(257, 9)),
        "narrow relu": lambda: (tfo.make_net(tfo.NARROW, 15, geo_activation="relu"), tfo.box_points(130, 11)),
        "relu skip at 2": lambda: (tfo.make_net(RELU_SKIP, 19, geo_activation="relu"), tfo.box_points(130, 12)),
        "multires 0": lambda: (tfo.make_net(PLAIN_0, 20), tfo.box_points(130, 13)),
    }[case]()
    a, b = tgo.autograd(net, xyz, torch.float64), tgo.tangents(net, xyz, torch.float64)
    top = float(np.abs(a["normal"]).max())
    rel = float(np.abs(a["normal"] - b["normal"]).max() / top)
    print(f"{case}: autograd - tangents {rel:.2e} of the largest component ({top:.3f}); gradient norm "
          f"{np.linalg.norm(a['normal'], axis=1).min():.3f} .. {np.linalg.norm(a['normal'], axis=1).max():.3f}")
    assert a["normal"].shape == (len(xyz), 3) and a["normal"].dtype == np.float64 and top > 0.1
    assert rel <= 1e-12
    assert np.array_equal(a["raw"], b["raw"]) and np.array_equal(a["raw"], tfo.forward(net, xyz, None, torch.float64)["raw"])
    # float32: the two derivations differ by rounding only
    a32, b32 = tgo.autograd(net, xyz, torch.float32), tgo.tangents(net, xyz, torch.float32)
    assert a32["normal"].dtype == np.float32 and b32["normal"].dtype == np.float32


def test_oracle_equals_the_reference_modules_under_compute_grad():
    fx = np.load(FIXTURE)
    assert fx["xyz"].shape == (257, 3) and np.array_equal(fx["xyz"], tfo.box_points(257, 5))
    net = tfo.make_net(tfo.REFERENCE, int(fx["seed"]))
    for name, fn in (("autograd", tgo.autograd), ("tangents", tgo.tangents)):
        o64, o32 = fn(net, fx["xyz"], torch.float64), fn(net, fx["xyz"], torch.float32)
        for k in ("sdf", "normal"):
            f64, f32 = fx[f"{k}64"], fx[f"{k}32"]
            assert f64.dtype == np.float64 and f32.dtype == np.float32 and o64[k].shape == f64.shape
            rel = float(np.abs(o64[k] - f64).max() / np.abs(f64).max())
            own = float(np.abs(f32.astype(np.float64) - f64).max())
            d32 = float(np.abs(o32[k].astype(np.float64) - f32).max())
            print(f"{name} {k}: float64 oracle - fixture {rel:.2e} of the largest value; float32 oracle - fixture {d32:.3e}, the fixture's own {own:.3e}")
            assert rel <= 1e-12
            assert own > 0 and d32 <= 4 * own
    norm = np.linalg.norm(fx["normal64"], axis=1)
    assert 0.05 < norm.min() and norm.max() < 5 and (-fx["sdf64"]).min() < -0.1 and (-fx["sdf64"]).max() > 0.5


def test_header_binding_and_exports():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^(?:int|size_t)\s+(ag_\w+)\s*\(", hdr, flags=re.M)
    assert names == ["ag_template_field_sdf_grad"]
    decl = re.search(r"int\s+ag_template_field_sdf_grad\s*\(([^)]*)\)", hdr).group(1)
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
    assert args == ["const AgTemplateFieldDesc* desc", "const float* blob", "size_t blob_floats", "const float* xyz", "int64_t N", "float* sdf", "float* grad",
                    "float* density", "void* stream"]
    table = {s[0]: s for s in _lib.SYMBOLS}
    name, restype, argtypes = table["ag_template_field_sdf_grad"]
    c_vp = ctypes.c_void_p
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.POINTER(_lib.AgTemplateFieldDesc), c_vp, ctypes.c_size_t, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp]
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ag_template_field_sdf_grad")
    import animatablegaussians_amd as pkg
    from animatablegaussians_amd import template_field as tf
    from animatablegaussians_amd import template_render as tr
    assert pkg.eikonal_loss is tf.eikonal_loss and pkg.render_normals is tr.render_normals and pkg.TemplateField is tf.TemplateField
    assert {"eikonal_loss", "render_normals"} <= set(pkg.__all__)
    assert callable(tf.TemplateField.sdf_normal) and callable(tf.TemplateField.surface_normals)


def test_entry_point_validates_without_a_device():
    """The checks of the entry point run before anything touches the GPU: a bad table, a wrong blob size and a negative N are refused
    and N == 0 succeeds, all on the host."""
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.template_field import TemplateField
    net = tfo.make_net(tfo.NARROW, 1)
    f = TemplateField.from_state_dict(tfo.state_dict(net), multires=2)
    L = ctypes.CDLL(_lib.LIB_PATH)
    fn = L.ag_template_field_sdf_grad
    fn.restype, fn.argtypes = ctypes.c_int, dict((s[0], s[2]) for s in _lib.SYMBOLS)["ag_template_field_sdf_grad"]
    d = f.desc()
    assert fn(ctypes.byref(d), None, f.blob.size, None, 0, None, None, None, None) == 0
    assert fn(ctypes.byref(d), None, f.blob.size + 1, None, 0, None, None, None, None) != 0
    assert fn(ctypes.byref(d), None, f.blob.size, None, -1, None, None, None, None) != 0
    assert fn(ctypes.byref(d), None, f.blob.size, None, 5, None, None, None, None) != 0          # null pointers with N > 0
    d.geo[1].width = 250
    assert fn(ctypes.byref(d), None, f.blob.size, None, 0, None, None, None, None) != 0
    d = f.desc()
    d.geo[2].concat = 2
    assert fn(ctypes.byref(d), None, f.blob.size, None, 0, None, None, None, None) != 0


def test_eikonal_loss_is_its_formula():
    from animatablegaussians_amd.template_field import eikonal_loss
    rs = np.random.RandomState(3)
    n = rs.normal(size=(4, 17, 3)) * rs.uniform(0.2, 3.0, (4, 17, 1))
    want = float(((np.sqrt((n * n).sum(-1)) - 1.0) ** 2).mean())
    got64 = eikonal_loss(torch.from_numpy(n))
    got32 = eikonal_loss(torch.from_numpy(n.astype(np.float32)))
    assert got64.shape == () and got64.dtype == torch.float64 and got32.dtype == torch.float32
    assert abs(float(got64) - want) <= 1e-14 * want and abs(float(got32) - want) <= 8 * 2.0 ** -24 * max(1.0, want)
    assert float(eikonal_loss(torch.from_numpy(tgo.unit(n)))) <= 1e-30 and abs(tgo.eikonal(n) - want) <= 1e-15
    # main_template.py:55, the reference's own spelling
    t = torch.from_numpy(n)
    assert float(got64) == float(((torch.linalg.norm(t, ord=2, dim=-1) - 1.) ** 2).mean())
