"""Host-side checks of the template renderer (``template_render.py``, ``include/ag_ray_march.h``): the oracle of
``template_render_oracle.py`` against the reference's own ``sample_pts_on_rays`` / ``raw2outputs`` (``tests/golden/template_render_ref.npz``,
written by ``make_golden_template_render.py``), the oracle's near / far in its two precisions, ``t`` and the binding table.  No GPU.

Near / far has no fixture: the reference's kernel is CUDA and cannot run on the host; the oracle restates the formulas of the header.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_render_oracle as tro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "template_render_ref.npz")
HEADER = os.path.join(ROOT, "include", "ag_ray_march.h")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("S", [2, 63, 64, 65])
def test_sampling_oracle_equals_the_reference(S):
    fx = np.load(FIXTURE)
    o, d, near, far = fx["ray_o"], fx["ray_d"], fx["near"], fx["far"]
    for tag, u in (("", None), ("p", fx[f"s{S}_u"])):
        z, pts = tro.sample(o, d, near, far, S, u)
        want_z, want_pts = fx[f"s{S}_z{tag}32"], fx[f"s{S}_pts{tag}32"]
        assert want_z.dtype == np.float32 and want_z.shape == (len(o), S) and want_pts.shape == (len(o), S, 3)
        assert np.array_equal(_bits(z), _bits(want_z)), f"S = {S} {tag}: z_vals differ from the reference's float32 bits"
        assert np.array_equal(_bits(pts), _bits(want_pts)), f"S = {S} {tag}: pts differ from the reference's float32 bits"
        # float64: the same formulas on the float32 inputs, to rounding
        n = fx[f"s{S}_z64"].shape[0]
        u64 = None if u is None else fx[f"s{S}_u64"].astype(np.float64)
        t = torch.linspace(0., 1., steps=S).numpy().astype(np.float64)
        z64 = near[:n, None].astype(np.float64) * (1. - t) + far[:n, None].astype(np.float64) * t
        if u64 is not None:
            mids = .5 * (z64[:, 1:] + z64[:, :-1])
            upper, lower = np.concatenate([mids, z64[:, -1:]], 1), np.concatenate([z64[:, :1], mids], 1)
            z64 = lower + (upper - lower) * u64
        p64 = o[:n, None].astype(np.float64) + d[:n, None].astype(np.float64) * z64[..., None]
        rel = max(float(np.abs(z64 - fx[f"s{S}_z{tag}64"]).max()), float(np.abs(p64 - fx[f"s{S}_pts{tag}64"]).max())) / float(np.abs(fx[f"s{S}_z64"]).max())
        print(f"S = {S} {'perturbed' if tag else 'unperturbed'}: float32 bits equal; float64 restatement - fixture {rel:.2e} of the largest value")
        assert rel <= 1e-14
    assert not np.array_equal(fx[f"s{S}_z32"], fx[f"s{S}_zp32"]) and (np.diff(fx[f"s{S}_zp32"], axis=1) > 0).all()


@pytest.mark.parametrize("S", [2, 63, 64, 65, 130])
def test_composite_oracle_equals_the_reference(S):
    fx = np.load(FIXTURE)
    density, color, z = fx[f"c{S}_density"], fx[f"c{S}_color"], fx[f"c{S}_z"]
    d2, c2, z2 = tro.composite_case(len(z), S, int(fx["seed"]) + S)
    assert np.array_equal(density, d2) and np.array_equal(color, c2) and np.array_equal(z, z2), "the scene recipe no longer gives the fixture's inputs"
    for white in (False, True):
        o64, o32 = tro.composite(density, color, z, white, torch.float64), tro.composite(density, color, z, white, torch.float32)
        for key, name in (("rgb_map", "rgb_white" if white else "rgb"), ("acc_map", "acc"), ("depth_map", "depth"), ("disp_map", "disp"), ("weights", "weights")):
            f64, f32 = fx[f"c{S}_{name}64"], fx[f"c{S}_{name}32"]
            assert f64.dtype == np.float64 and f32.dtype == np.float32 and o64[key].shape == f64.shape
            ok = np.isfinite(f64) & np.isfinite(f32)            # disp_map of a ray with acc = 0 is 0 / 0 = NaN in the reference
            assert np.array_equal(np.isnan(o64[key]), np.isnan(f64)) and np.array_equal(np.isnan(o32[key]), np.isnan(f32)) and (ok.all() or key == "disp_map")
            rel = float(np.abs(o64[key] - f64)[ok].max() / np.abs(f64[ok]).max())
            own = float(np.abs(f32.astype(np.float64) - f64)[ok].max())
            d32 = float(np.abs(o32[key].astype(np.float64) - f32)[ok].max())
            print(f"S = {S} white {white} {key}: float64 oracle - fixture {rel:.2e} of the largest value; float32 oracle - fixture {d32:.3e}, the fixture's own {own:.3e}")
            assert rel <= 1e-12
            assert d32 <= 4 * own
    acc = fx[f"c{S}_acc64"]
    assert acc.min() < 0.01 and acc.max() > 0.99, "the fixture's rays do not span empty and opaque"


@pytest.mark.parametrize("V,R", [(1, 65), (65, 63), (1500, 513)])
def test_near_far_oracle_precisions_agree_on_hit(V, R):
    vertices, o, d, fallback = tro.near_far_scene(V, R, seed=V + R)
    n32, f32, h32, disc32 = tro.near_far(vertices, o, d, 0.1, fallback, np.float32)
    n64, f64, h64, disc64 = tro.near_far(vertices, o, d, 0.1, fallback, np.float64)
    census = tro.near_far_census(n32, f32, h32, disc32)
    # a grazing PAIR may fall on either side of 1e-8 in the two precisions (its disc is a rounding residue); `hit` of the RAY must agree
    flipped = int(((disc32.astype(np.float64) < 1e-8) != (disc64 < 1e-8)).sum())
    print(f"V = {V}, R = {R}: {census}; pairs whose side of 1e-8 differs between float32 and float64: {flipped}")
    assert np.array_equal(h32, h64), "float32 and float64 disagree on hit"
    for k in ("miss", "hit", "negative_near", "behind", "graze_hit", "graze_miss"):
        assert census[k] > 0, f"the scene holds no ray of kind {k}"
    both = h32 & ~(np.abs(disc32) < 1e-5).any(1)
    scale = float(np.abs(f64[both]).max())
    assert float(np.abs(n32[both] - n64[both]).max()) <= 1e-4 * scale and float(np.abs(f32[both] - f64[both]).max()) <= 1e-4 * scale
    assert np.array_equal(n32[~h32], fallback[0][~h32]) and np.array_equal(f32[~h32], fallback[1][~h32])
    n0, f0, _, _ = tro.near_far(vertices, o, d, 0.1, None, np.float32)
    assert not n0[~h32].any() and not f0[~h32].any()


@pytest.mark.parametrize("S", [2, 3, 63, 64, 65, 130, 1024])
def test_t_is_torch_linspace(S):
    from animatablegaussians_amd import template_render as tr
    t = tr._t_vals(S, torch.device("cpu"))
    want = torch.linspace(0., 1., steps=S)
    assert t.dtype == torch.float32 and tuple(t.shape) == (S,) and np.array_equal(_bits(t.numpy()), _bits(want.numpy()))
    assert np.array_equal(_bits(tro.t_vals(S)), _bits(want.numpy())) and t[0] == 0 and t[-1] == 1


def test_abi_symbols_match_the_header():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(ag_\w+)\s*\(([^;]*)\)\s*;", hdr, flags=re.M))
    assert set(protos) == {"ag_ray_near_far", "ag_ray_sample", "ag_ray_composite"}
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name, args in protos.items():
        assert name in table and hasattr(L, name), name
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        assert table[name][1] is ctypes.c_int and table[name][2] == want, f"{name}: the binding's argument types are not the header's"
    from animatablegaussians_amd import template_render as tr
    assert re.search(r"#define AG_RAY_MIN_SAMPLES\s+2\b", hdr) and re.search(r"#define AG_RAY_MAX_SAMPLES\s+1024\b", hdr)
    assert (tr.MIN_SAMPLES, tr.MAX_SAMPLES) == (2, 1024)
    import animatablegaussians_amd as pkg
    assert pkg.render is tr.render and pkg.near_far_smpl is tr.near_far_smpl and pkg.sample_pts_on_rays is tr.sample_pts_on_rays
    assert pkg.composite is tr.composite


def test_host_tensors_are_refused_without_a_gpu():
    from animatablegaussians_amd import template_render as tr
    o = torch.zeros(4, 3)
    for bad in (lambda: tr.near_far_smpl(o, o, o), lambda: tr.sample_pts_on_rays(o, o, o[:, 0], o[:, 0]),
                lambda: tr.composite(torch.zeros(4, 8), torch.zeros(4, 8, 3), torch.zeros(4, 8))):
        with pytest.raises(ValueError, match="GPU"):
            bad()
