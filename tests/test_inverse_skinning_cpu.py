"""Inverse skinning, the part that needs no GPU: the float64 oracle (``inverse_skinning_oracle.py``) against what the REFERENCE's own
code computed (``golden/inverse_skinning_ref.npz``, written by ``golden/make_golden_inverse_skinning.py``: its
``compute_gradient_volume`` and its root-finding kernel compiled for the host), the oracle's own properties that the GPU tests lean
on, the ABI surface, the pinned Python signatures and the argument checks that run without a device.

Bars, none derived from the code under test: 4 x the worst |float32 oracle - float64 oracle| on the same input plus 2^-22 x the largest
magnitude (of the gradient; of the bounds for points).  Points are compared where the float32 and the float64 oracle visited the same
node at every iteration (the weights are the NEAREST node's: a run that steps into another cell solves another equation); the
share left out is capped at 1 % and printed."""
import ctypes
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_skinning_oracle as iso  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.sh recompiles a unit when ANY header under csrc/ or include/ is newer than its object
STALE_HEADERS = 'find "$HERE" "$HERE/../../include" -maxdepth 1 -name \'*.h\' -newer "$obj"'
GOLDEN = os.path.join(ROOT, "tests", "golden", "inverse_skinning_ref.npz")
CAP = 0.01


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as data:
        return {k: data[k] for k in data.files}


def _golden_case(tag):
    g = _golden()
    base = "big" if tag == "big5" else tag
    case = {k: g[f"{base}_{k}"] for k in ("volume", "bounds", "spacing", "jnt_mats", "xt")}
    case["xc_init"] = g[f"{tag}_xc_init"]
    return case, g[f"{tag}_ref_xc"]


def test_oracle_gradient_is_the_sobel_filter_written_out():
    for shape in [(9, 7, 5, 6), (5, 4, 3, 1), (2, 2, 2, 3)]:
        vol = iso.random_volume(shape)
        spacing = np.float32([0.031, 0.02, 0.0173])
        ours, plain = iso.gradient(vol, spacing), iso.sobel_plain(vol, spacing)
        assert ours.shape == shape + (3,) and np.abs(ours - plain).max() <= 1e-12 * np.abs(plain).max()
    # a linear ramp along an axis has that slope at every interior node and half of it is lost at a face (zero padding)
    ramp = np.broadcast_to((0.5 * np.arange(6))[:, None, None, None], (6, 5, 4, 1)).astype(np.float32)
    g = iso.gradient(ramp, np.float32([0.25, 1, 1]))
    assert np.abs(g[1:-1, 1:-1, 1:-1, 0, 0] - 2.0).max() <= 1e-12 and np.abs(g[1:-1, 1:-1, 1:-1, 0, 1:]).max() <= 1e-12
    assert g[0, 2, 2, 0, 0] == pytest.approx(0.5 / 0.5) and g[2, 0, 2, 0, 1] != 0                   # (v(1) - 0) / (2 h); the padded side pulls


def test_float64_oracle_against_the_reference_gradient():
    g = _golden()
    for tag in ("small", "big"):
        vol, spacing, ref = g[f"{tag}_volume"], g[f"{tag}_spacing"], g[f"{tag}_ref_grad"]
        o64, o32 = iso.gradient(vol, spacing), iso.gradient(vol, spacing, np.float32)
        if tag == "big":
            n = g["big_grad_nodes"]
            res = np.array(vol.shape[:3])
            on_face = ((n == 0) | (n == res - 1)).sum(-1)
            assert (on_face == 3).sum() >= 8 and (on_face == 2).any() and (on_face == 1).any() and (on_face == 0).any()
            o64, o32 = o64[n[:, 0], n[:, 1], n[:, 2]], o32[n[:, 0], n[:, 1], n[:, 2]]
        limit, own = iso.bar(o32, o64, np.abs(o64).max())
        worst = float(np.abs(ref.astype(np.float64) - o64).max())
        print(f"{tag}: |reference - float64 oracle| {worst:.3e}, float32 oracle's own deviation {own:.3e}, bar {limit:.3e}, largest |gradient| "
              f"{np.abs(o64).max():.3f}")
        assert ref.shape == o64.shape and own > 0 and worst <= limit


@pytest.mark.parametrize("tag", ["small", "big", "big5"])
def test_float64_oracle_against_the_reference_root_finding(tag):
    case, ref = _golden_case(tag)
    args = (case["volume"], case["bounds"], case["spacing"], case["xt"], case["xc_init"], case["jnt_mats"])
    o64, n64 = iso.root_find(*args, dtype=np.float64)
    o32, n32 = iso.root_find(*args, dtype=np.float32)
    keep = iso.kept(n32, n64)
    left_out = 1.0 - keep.mean()
    limit, own = iso.bar(o32[keep], o64[keep], np.abs(case["bounds"]).max())
    dev = np.abs(ref.astype(np.float64) - o64).max(-1)
    moved = float(np.abs(o64 - case["xc_init"]).max())
    print(f"{tag}: {keep.size} points, left out {left_out:.4%}; |reference - float64 oracle| over the kept points {dev[keep].max():.3e}, float32 oracle's own "
          f"deviation {own:.3e}, bar {limit:.3e}; the iteration moved the points by up to {moved:.3e}")
    assert ref.shape == o64.shape == (1, iso.N_POINTS, 3) and left_out <= CAP
    assert moved > 0.01                                                             # more than one clamped step: the ten iterations ran
    assert dev[keep].max() <= limit


def test_oracle_node_choice_rounds_halves_away_and_clamps():
    x = np.float32([0.0, 0.49999997, 0.5, 1.5, 2.5, 3.0, 7.5])
    assert np.array_equal(iso.round_half_away(x), [0, 0, 1, 2, 3, 3, 8])
    assert np.array_equal(iso.round_half_away(x.astype(np.float64)), [0, 0, 1, 2, 3, 3, 8])
    for shape in [(9, 7, 5, 6), (5, 4, 3, 1)]:
        case, want = iso.exact_grid_case(shape)
        for dtype in (np.float32, np.float64):
            assert np.array_equal(iso.nodes_of(case["xc_init"].astype(dtype), case["bounds"], shape[:3], dtype), want)
        res = np.array(shape[:3])
        assert (want == 0).any() and (want == res - 1).any() and want.shape[1] >= 100
        assert ((case["xc_init"] % 1) == 0.5).any() and (case["xc_init"] < 0).any() and (case["xc_init"] > res - 1).any()
    assert np.array_equal(iso.nodes_of(np.float32([[np.nan, -np.inf, np.inf]]), np.float32([[0, 0, 0], [1, 1, 1]]), (4, 5, 6), np.float32), [[3, 0, 5]])


def test_oracle_singular_step_moves_by_plus_one_centimetre():
    case = iso.smooth_case((5, 4, 3, 1), n=3)
    mats = np.zeros_like(case["jnt_mats"])
    for dtype in (np.float32, np.float64):
        xc, _ = iso.root_find(case["volume"], case["bounds"], case["spacing"], case["xt"], case["xc_init"], mats, iterations=1, dtype=dtype)
        assert np.isfinite(xc).all() and np.array_equal(xc, case["xc_init"].astype(dtype) - dtype(iso.STEP))


def test_oracle_init_is_the_inverse_of_the_blend():
    rng = np.random.RandomState(5)
    c = iso.smooth_case((9, 7, 5, 6), n=200, B=2)
    w = rng.uniform(0, 1, (2, 200, 6)) ** 3
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    n = rng.normal(0, 1, (2, 200, 3)).astype(np.float32)
    p64, n64 = iso.init(c["xt"], w, c["jnt_mats"], n)
    M = np.einsum("bnj,bjrc->bnrc", w.astype(np.float64), c["jnt_mats"].astype(np.float64))
    M[..., 3, :] = [0, 0, 0, 1]                # the blend as an AFFINE map (the header): float32 weights sum to 1 only within 2^-24 J
    Mi = np.linalg.inv(M)
    want_p = np.einsum("bnrc,bnc->bnr", Mi[..., :3, :3], c["xt"].astype(np.float64)) + Mi[..., :3, 3]
    want_n = np.einsum("bnrc,bnc->bnr", Mi[..., :3, :3], n.astype(np.float64))
    assert np.abs(p64 - want_p).max() <= 1e-12 and np.abs(n64 - want_n).max() <= 1e-12
    p32, n32 = iso.init(c["xt"], w, c["jnt_mats"], n, np.float32)
    assert p32.dtype == np.float32 and 0 < np.abs(p32 - p64).max() <= 1e-5


def test_inactive_points_and_zero_iterations_copy_in_the_oracle():
    c = iso.smooth_case((5, 4, 3, 1), n=40)
    active = np.arange(40)[None] % 3 != 0
    xc, nodes = iso.root_find(c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], c["jnt_mats"], active, iterations=2, dtype=np.float32)
    assert np.array_equal(xc[~active], c["xc_init"][~active]) and (xc[active] != c["xc_init"][active]).any() and nodes.shape == (2, 1, 40, 3)
    xc, nodes = iso.root_find(c["volume"], c["bounds"], c["spacing"], c["xt"], c["xc_init"], c["jnt_mats"], iterations=0, dtype=np.float32)
    assert np.array_equal(xc, c["xc_init"]) and nodes.shape[0] == 0 and iso.kept(nodes, nodes).all()


ENTRY_POINTS = (("ag_weight_volume_gradient", 8), ("ag_inverse_skinning_init", 10), ("ag_inverse_skinning_root_find", 18))


def test_entry_points_declared_bound_and_exported():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_inverse_skinning.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_want in ENTRY_POINTS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_inverse_skinning.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in table and len(table[name][2]) == n_args == n_want, name
        assert table[name][1] is ctypes.c_int and hasattr(L, name), f"{name} is not exported"
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_inverse_skinning\.hip" \$EXACT', build) and STALE_HEADERS in build


def test_bad_sizes_are_refused_by_return_code_without_a_device():
    from animatablegaussians_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    table = {s[0]: s for s in _lib.SYMBOLS}
    for name, _ in ENTRY_POINTS:
        getattr(L, name).restype, getattr(L, name).argtypes = table[name][1], table[name][2]
    L.ag_last_error.restype = ctypes.c_char_p
    f3 = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    f6 = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    INVALID = -1                                                                    # AG_ERR_INVALID_ARGUMENT

    def root(X=4, Y=4, Z=4, J=3, B=1, N=5, iterations=10, bounds=f6, spacing=f3):
        return L.ag_inverse_skinning_root_find(None, None, X, Y, Z, J, bounds, spacing, None, None, None, None, None, B, N, 0.1, iterations, None)

    for bad in (dict(X=1), dict(Y=1), dict(Z=1), dict(J=0), dict(J=129), dict(N=-1), dict(iterations=-1), dict(B=-1), dict(B=65536)):
        assert root(**bad) == INVALID and L.ag_last_error(), bad
    assert root(N=0) == 0 and root(B=0) == 0 and root(N=0, J=128, iterations=0) == 0           # nothing to launch: no device is touched
    assert root() == INVALID and b"null pointer" in L.ag_last_error()                          # valid sizes, no arrays: still no launch
    assert root(spacing=(ctypes.c_float * 3)(0.1, 0.0, 0.1)) == INVALID
    grad = lambda **k: L.ag_weight_volume_gradient(None, k.get("X", 4), 4, 4, k.get("C", 3), k.get("spacing", f3), None, None)  # noqa: E731
    assert grad(X=1) == INVALID and grad(C=0) == INVALID and grad(C=129) == INVALID and grad(spacing=None) == INVALID and grad() == INVALID
    init = lambda B=1, N=5, J=3: L.ag_inverse_skinning_init(None, None, None, None, None, None, B, N, J, None)  # noqa: E731
    assert init(J=0) == INVALID and init(J=129) == INVALID and init(N=-1) == INVALID and init(B=-1) == INVALID and init() == INVALID
    assert init(N=0) == 0 and init(B=0) == 0


def test_signatures_and_defaults_are_pinned():
    from animatablegaussians_amd import inverse_skinning as inv
    from animatablegaussians_amd.weight_volume import WeightVolume
    p = inspect.signature(WeightVolume.gradient_volume).parameters
    assert list(p) == ["self", "volume_type"] and p["volume_type"].default == "diff"
    p = inspect.signature(WeightVolume.root_find).parameters
    assert list(p) == ["self", "posed_pts", "cano_init", "jnt_mats", "active", "lam", "iterations", "volume_type", "grad_volume"]
    kw = ("active", "lam", "iterations", "volume_type", "grad_volume")
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw) and tuple(p[k].default for k in kw) == (None, 0.1, 10, "diff", None)
    p = inspect.signature(inv.transform_live2cano).parameters
    assert list(p) == ["posed_pts", "cano2live_jnt_mats", "volume", "live_mesh_v", "live_mesh_f", "live_mesh_lbs", "normals", "near_thres",
                       "use_root_finding", "with_hand", "nonopt_bone_ids", "lam", "iterations", "volume_type"]
    kw = list(p)[6:]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    assert tuple(p[k].default for k in kw) == (None, 0.08, True, False, (7, 8, 10, 11), 0.1, 10, "diff")
    p = inspect.signature(inv.transform_cano2live).parameters
    assert list(p)[:5] == ["cano_pts", "cano2live_jnt_mats", "volume", "normals", "with_hand"] and p["with_hand"].default is False
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])


def test_rigid_hands_and_host_tensors_are_refused_before_anything_is_launched():
    import torch
    from animatablegaussians_amd import inverse_skinning as inv
    m = torch.arange(2 * 55 * 16, dtype=torch.float32).view(2, 55, 4, 4)
    r = inv.rigid_hands(m)
    assert torch.equal(r[:, :25], m[:, :25]) and all(torch.equal(r[:, j], m[:, 20]) for j in range(25, 40))
    assert all(torch.equal(r[:, j], m[:, 21]) for j in range(40, 55)) and r.data_ptr() != m.data_ptr()
    with pytest.raises(ValueError, match="55"):
        inv.rigid_hands(m[:, :24])
    with pytest.raises(ValueError, match="GPU"):
        inv.initial_guess(torch.zeros(1, 4, 3), torch.zeros(1, 4, 6), torch.zeros(1, 6, 4, 4))
