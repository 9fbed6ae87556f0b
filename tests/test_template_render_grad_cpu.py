"""Host-side checks of the template renderer's reverse pass (``include/ag_ray_march_grad.h``): the division-free recurrence of the
header against torch autograd of the reference's text in float64, the density's closed-form derivatives against autograd, the binding
table against the header, and the refusals that need no GPU.  No GPU.

Measured while writing: the float64 recurrence is within 5e-16 of the largest element of autograd's ``grad_density`` and equal for
``grad_color`` on all four scenes; the float32 recurrence is within 1.2e-7 .. 3.7e-7 of the float64 gradient; the density chain
agrees to 3e-8 of the largest element or better (``b`` is a float32 sum in both).
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_render_grad_oracle as tgo  # noqa: E402
import template_render_oracle as tro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ag_ray_march_grad.h")
SCENES = [(1, 2), (3, 63), (257, 64), (5, 130)]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_oracle_chain_is_the_render_oracles():
    density, color, z = tro.composite_case(5, 63)
    for white in (False, True):
        want = tro.composite(density, color, z, white, torch.float64)
        got = tgo.composite_torch(*(torch.from_numpy(a).double() for a in (density, color, z)), white)
        for k in ("rgb_map", "acc_map", "depth_map", "weights", "alpha"):
            assert np.array_equal(got[k].numpy(), want[k]), k


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("R,S", SCENES)
def test_recurrence_equals_autograd_in_float64(R, S, white):
    density, color, z = tro.composite_case(R, S)
    G = tgo.upstream(R, S, seed=R + S)
    for names in [(k,) for k in tgo.GRADS] + [tgo.GRADS]:
        grads = {k: G[k] for k in names}
        ad, ac = tgo.composite_autograd(density, color, z, grads, white)
        rd, rc, _, _ = tgo.composite_recurrence(density, color, z, grads, white, np.float64)
        assert np.isfinite(ad).all() and np.isfinite(rd).all()
        ed = float(np.abs(rd - ad).max() / np.abs(ad).max())
        ec = float(np.abs(rc - ac).max() / max(np.abs(ac).max(), 1e-300))
        d32, c32, _, _ = tgo.composite_recurrence(density, color, z, grads, white, np.float32)
        e32 = float(np.abs(d32 - ad).max() / np.abs(ad).max())
        print(f"R = {R}, S = {S}, white {white}, {'+'.join(names)}: recurrence - autograd {ed:.2e} (density), {ec:.2e} (colour) of the largest element; "
              f"float32 recurrence {e32:.2e}")
        assert ed <= 1e-12 and ec <= 1e-12
        assert np.isfinite(d32).all() and np.isfinite(c32).all()
        if "rgb_map" not in names:
            assert not ac.any() and not rc.any()


def test_the_saturated_scene_holds_alpha_one_and_float32_autograd_is_finite():
    density, color, z = tro.composite_case(257, 64)
    _, _, _, alpha = tgo.composite_recurrence(density, color, z, {}, False, np.float32)
    ones = int((alpha == 1).sum())
    ones_torch = int((tro.composite(density, color, z, False, torch.float32)["alpha"] == 1).sum())      # torch.exp and numpy.exp differ by an ulp
    print(f"(257, 64): {ones} samples with float32 alpha = 1 exactly in the recurrence oracle, {ones_torch} in torch's chain")
    assert alpha.dtype == np.float32 and ones >= 1 and ones_torch >= 1
    gd, gc = tgo.composite_autograd(density, color, z, tgo.upstream(257, 64, 1), False, torch.float32)
    assert np.isfinite(gd).all() and np.isfinite(gc).all()


@pytest.mark.parametrize("beta", [0.01, -0.01, 0.0, 0.3])
def test_density_closed_forms_equal_autograd(beta):
    sdf, g = tgo.sdf_case(4099, seed=3)
    assert (sdf == 0).sum() > 500 and (sdf > 0).any() and (sdf < 0).any()
    d64, gs64, gb64 = tgo.laplace_autograd(sdf, beta, g)
    dens, gs, terms = tgo.laplace_closed(sdf, beta, g, np.float64)
    gb = float(np.sign(np.float32(beta)) * terms.sum())
    scale_b = float(np.abs(terms).sum())
    print(f"beta = {beta}: density {_rel(dens, d64):.2e}, grad_sdf {_rel(gs, gs64):.2e} of the largest element; grad_beta {gb:.9e} vs autograd {gb64:.9e} "
          f"(sum |terms| {scale_b:.3e})")
    assert _rel(dens, d64) <= 1e-12 and _rel(gs, gs64) <= 1e-12
    assert abs(gb - gb64) <= 1e-12 * scale_b
    assert not gs[sdf == 0].any() and not gs64[sdf == 0].any(), "the gradient at sdf == 0 is not 0"
    if beta == 0.0:
        assert gb == 0.0 and gb64 == 0.0
    if beta < 0:
        _, _, pos = tgo.laplace_autograd(sdf, -beta, g)
        assert gb64 == -pos and gb64 != 0, "the sign of beta does not flip grad_beta"
    # the float32 closed forms stay near the float64 ones (what the kernel evaluates)
    d32, gs32, t32 = tgo.laplace_closed(sdf, beta, g, np.float32)
    assert _rel(d32.astype(np.float64), d64) <= 1e-5 and _rel(gs32.astype(np.float64), gs64) <= 1e-5
    # the oracle of the forward kernels states the same density (its b is a float64 sum: 3e-8)
    assert _rel(tro.laplace_density(-sdf.astype(np.float64), float(np.abs(np.float32(beta))) + 1e-4), d64) <= 1e-6


def test_abi_symbols_match_the_header():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {name: (ret, args) for ret, name, args in re.findall(r"^(int|size_t)\s+(ag_\w+)\s*\(([^;]*)\)\s*;", hdr, flags=re.M)}
    assert set(protos) == {"ag_ray_composite_backward", "ag_laplace_density", "ag_laplace_density_backward_workspace_bytes", "ag_laplace_density_backward"}
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name, (ret, args) in protos.items():
        assert name in table and hasattr(L, name), name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        assert table[name][1] is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
        assert table[name][2] == want, f"{name}: the binding's argument types are not the header's"
    groups = int(re.search(r"#define AG_LAPLACE_GROUPS_PER_WAVE\s+(\d+)\b", hdr).group(1))
    fn = L.ag_laplace_density_backward_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int64]
    for n in (0, 1, 64 * groups, 64 * groups + 1, 4099, 2 ** 24):
        assert fn(n) == 8 * max(1, -(-n // (64 * groups))), n
    # the forward's header keeps its three prototypes
    fwd = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_ray_march.h")).read(), flags=re.S)
    assert len(re.findall(r"^int\s+ag_\w+\s*\(", fwd, flags=re.M)) == 3
    import animatablegaussians_amd as pkg
    from animatablegaussians_amd import template_render as tr
    for name in ("composite_backward", "laplace_density", "render_train", "training_loss"):
        assert getattr(pkg, name) is getattr(tr, name) and name in pkg.__all__


def test_the_abi_refuses_bad_counts_and_pairs_before_any_launch():
    from animatablegaussians_amd import _lib
    L, null, p = _lib.lib(), ctypes.c_void_p(None), ctypes.c_void_p(64)     # `p`: never dereferenced, every call below is refused first
    for S in (1, 1025):
        assert L.ag_ray_composite_backward(p, null, p, 4, S, 0, null, p, null, null, p, null, null) != 0 and b"S = " in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, -1, 8, 0, null, p, null, null, p, null, null) != 0 and b"R = " in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, p, p, 4, 8, 0, null, p, null, null, p, null, null) != 0 and b"color and g_rgb_map" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, p, p, null, null, p, null, null) != 0 and b"color and g_rgb_map" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, null, p, null, null, p, p, null) != 0 and b"grad_color" in L.ag_last_error()
    assert L.ag_ray_composite_backward(p, null, p, 4, 8, 0, null, p, null, null, null, null, null) != 0 and b"grad_density" in L.ag_last_error()
    assert L.ag_ray_composite_backward(null, null, null, 4, 8, 0, null, p, null, null, p, null, null) != 0 and b"null" in L.ag_last_error()
    assert L.ag_ray_composite_backward(null, null, null, 0, 8, 0, null, null, null, null, p, null, null) == 0          # R = 0: nothing to do
    assert L.ag_laplace_density(p, -1, p, p, null) != 0 and b"N = " in L.ag_last_error()
    assert L.ag_laplace_density(null, 4, p, p, null) != 0 and b"null" in L.ag_last_error()
    assert L.ag_laplace_density(null, 0, null, null, null) == 0
    assert L.ag_laplace_density_backward(p, p, -1, p, p, null, null, null) != 0 and b"N = " in L.ag_last_error()
    assert L.ag_laplace_density_backward(p, p, 4, p, null, null, null, null) != 0 and b"grad_sdf" in L.ag_last_error()
    assert L.ag_laplace_density_backward(p, p, 4, p, null, p, null, null) != 0 and b"workspace" in L.ag_last_error()
    assert L.ag_laplace_density_backward(p, p, 4, null, p, null, null, null) != 0 and b"beta" in L.ag_last_error()


def test_host_tensors_and_bad_arguments_are_refused_without_a_gpu():
    from animatablegaussians_amd import template_render as tr
    d, c, z = torch.zeros(4, 8), torch.zeros(4, 8, 3), torch.zeros(4, 8)
    for bad in (lambda: tr.composite_backward(d, c, z, {"acc_map": torch.zeros(4)}), lambda: tr.laplace_density(d, 0.01)):
        with pytest.raises(ValueError, match="GPU"):
            bad()
    with pytest.raises(ValueError, match="grads names"):
        tr.composite_backward(d, c, z, {"disp_map": torch.zeros(4)})
    with pytest.raises(ValueError, match="z_vals requires grad"):
        tr.composite(d, c, z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="hands"):
        tr.render_train(lambda p, v: None, 0.01, z, z, z, z, hands={})
    with pytest.raises(ValueError, match="callable"):
        tr.render_train(None, 0.01, z, z, z, z)
