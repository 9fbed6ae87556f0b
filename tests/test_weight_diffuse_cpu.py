"""The diffused blend-weight volume, the part that needs no GPU: the properties of the float64 oracle that the GPU tests lean on
(``weight_diffuse_oracle.py``: the operator is symmetric positive definite on the free nodes, its conjugate gradients reach the direct
solution, the direct solution obeys the maximum principle, keeps the partition of unity and is continuous where the target jumps),
the ABI surface, the pinned Python signatures, and every exclusion or cap of ``test_weight_diffuse_gpu.py`` on the oracle alone."""
import ctypes
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_diffuse_oracle as wdo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# build.sh recompiles a unit when ANY header under csrc/ or include/ is newer than its object
STALE_HEADERS = 'find "$HERE" "$HERE/../../include" -maxdepth 1 -name \'*.h\' -newer "$obj"'
SMALL = [s for s in wdo.SHAPES if s != (12, 12, 12, 55)]                            # the dense matrices of the largest case: once, below


@functools.lru_cache(maxsize=None)
def _solved(shape):
    """(target, fixed, w, direct, (u, iterations, rel) of CG in float64, the same in float32) -- built once, never modified."""
    target, fixed, w = wdo.band_case(shape)
    return (target, fixed, w, wdo.direct_solve(target, fixed, w), wdo.cg(target, fixed, w, dtype=np.float64),
            wdo.cg(target, fixed, w, dtype=np.float32))


@pytest.mark.parametrize("shape", SMALL)
def test_operator_is_symmetric_positive_definite_on_the_free_nodes(shape):
    target, fixed, w = wdo.band_case(shape)
    Aff, Afc = wdo.free_matrix(fixed, w)
    assert np.array_equal(Aff, Aff.T)
    lo = float(np.linalg.eigvalsh(Aff).min())
    print(f"{shape}: {Aff.shape[0]} free nodes, smallest eigenvalue {lo:.3e}")
    assert lo > 0
    # the matrix-free function IS that matrix: A_ff on a vector that vanishes on the fixed nodes, A_fc t on one that vanishes elsewhere
    rng = np.random.RandomState(3)
    v = rng.normal(0, 1, shape) * ~fixed[..., None]
    fr = ~fixed.reshape(-1)
    J = shape[3]
    assert np.abs(wdo.apply(v, fixed, w).reshape(-1, J)[fr] - Aff @ v.reshape(-1, J)[fr]).max() <= 1e-12
    t = rng.normal(0, 1, shape) * fixed[..., None]
    assert np.abs(wdo.apply(t, fixed, w).reshape(-1, J)[fr] - Afc @ t.reshape(-1, J)[~fr]).max() <= 1e-12
    assert (wdo.apply(v + t, fixed, w)[fixed] == 0).all()


@pytest.mark.parametrize("shape", wdo.SHAPES)
def test_oracle_cg_agrees_with_the_direct_solve_and_its_properties_hold(shape):
    target, fixed, w, direct, (u64, it64, rel64), (u32, it32, rel32) = _solved(shape)
    e64, e32 = float(np.abs(u64 - direct).max()), float(np.abs(u32.astype(np.float64) - direct).max())
    t64, t32 = wdo.true_rel_residual(u64, target, fixed, w), wdo.true_rel_residual(u32, target, fixed, w)
    print(f"{shape}: {int(fixed.sum())} of {fixed.size} nodes fixed; CG iterations float64 {it64} float32 {it32}; |CG - direct| {e64:.3e} / {e32:.3e}; "
          f"true relative residual {t64.max():.3e} / {t32.max():.3e}")
    # CG at tol leaves an error of the order of tol x the condition number's root; 1e-3 says "the same solution", the GPU bar is e64, e32
    assert e64 <= 1e-3 and e32 <= 1e-3 and (rel64 <= wdo.TOL).all() and (rel32 <= wdo.TOL).all()
    assert np.array_equal(u64[fixed], target[fixed].astype(np.float64)) and np.array_equal(u32[fixed], target[fixed])
    # maximum principle, per channel, and what follows for rows
    tf = target[fixed].astype(np.float64)
    assert (direct >= tf.min(0) - 1e-12).all() and (direct <= tf.max(0) + 1e-12).all()
    J = shape[3]
    if J >= 3:
        assert (direct[..., 0] == 0).all() and np.abs(direct[..., 1] - 1).max() <= 1e-12
        assert (u64[..., 0] == 0).all() and (u32[..., 0] == 0).all()                   # a channel with b = 0 never moves
    # the caps of the GPU file, on the oracle alone
    assert it32 <= 1.5 * it64 and it64 <= 20 * max(shape[:3])
    assert t32.max() <= 4 * max(t64.max(), wdo.TOL) and (t32[rel32 == 0] == 0).all()
    assert fixed[0, 0, 0] and fixed[-1, -1, -1] and fixed[0, 1:-1, 1:-1].any() and not fixed.all()


def test_partition_of_unity_survives_the_direct_solve():
    shape = (9, 12, 14, 5)
    target, fixed, w = wdo.band_case(shape)
    t = target.astype(np.float64) + 0.05
    t /= t.sum(-1, keepdims=True)
    u = wdo.direct_solve(t, fixed, w)
    assert np.abs(u.sum(-1) - 1).max() <= 1e-12 and u.min() >= 0 and u.max() <= 1
    assert np.abs(wdo.clip_renormalise(u) - u).max() <= 1e-12


def test_two_lobes_the_solution_is_continuous_where_the_target_jumps():
    target, fixed, w = wdo.two_lobe_case()
    u = wdo.direct_solve(target, fixed, w)
    jt, ju = wdo.midplane_jump(target), wdo.midplane_jump(u)
    print(f"largest jump between mid-plane neighbours: target {jt:.3f}, harmonic extension {ju:.3f}")
    assert jt == 1.0 and ju < 0.5 * jt
    assert np.abs(u.sum(-1) - 1).max() <= 1e-12                                      # the two lobes' weights sum to 1 everywhere
    Y = u.shape[1]
    assert np.abs(u[:, Y // 2 - 1, :, 0] - u[:, Y // 2, :, 1]).max() <= 1e-12       # mirror symmetry about the mid-plane


def test_operator_oracle_float32_deviation_and_the_row_sum_bar():
    for shape in wdo.SHAPES:
        target, fixed, w = wdo.band_case(shape)
        probe = wdo.probe_input(shape)
        o64, o32 = wdo.apply(probe, fixed, w), wdo.apply(probe, fixed, w, np.float32)
        own = float(np.abs(o32.astype(np.float64) - o64).max())
        assert o32.dtype == np.float32 and 0 < own <= 64 * 2.0 ** -24 * float(np.abs(probe).max()) and (o32[fixed] == 0).all()
    assert wdo.row_sum_bar(55) == 56 * 2.0 ** -24
    rng = np.random.RandomState(1)
    u = rng.uniform(0, 1, (4096, 55)).astype(np.float32) ** 4
    q = u / u.sum(-1, keepdims=True, dtype=np.float32)
    assert q.dtype == np.float32 and np.abs(q.astype(np.float64).sum(-1) - 1).max() <= wdo.row_sum_bar(55)
    z = wdo.clip_renormalise(np.array([[0.0, 0.0], [-0.5, 0.0], [2.0, 1.0]]))
    assert np.array_equal(z, [[0, 0], [0, 0], [0.5, 0.5]])


def test_entry_points_declared_bound_and_exported():
    from animatablegaussians_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ag_weight_diffuse.h")).read(), flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_want in (("ag_weight_diffuse_workspace_bytes", 4), ("ag_weight_diffuse_apply", 9), ("ag_weight_diffuse_init", 16),
                         ("ag_weight_diffuse_iterate", 15)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, f"{name} is not declared in include/ag_weight_diffuse.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in table and len(table[name][2]) == n_args == n_want, name
        assert hasattr(L, name), f"{name} is not exported"
    assert table["ag_weight_diffuse_workspace_bytes"][1] is ctypes.c_size_t
    build = open(os.path.join(ROOT, "animatablegaussians_amd", "csrc", "build.sh")).read()
    assert re.search(r'compile "\$HERE/ag_weight_diffuse\.hip" \$EXACT', build) and STALE_HEADERS in build
    # host-side argument checks run without a device: sizes and null pointers are refused by return code
    fn = L.ag_weight_diffuse_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int32] * 4
    assert fn(1, 4, 4, 2) == 0 and fn(4, 4, 4, 0) == 0 and fn(2048, 2048, 2048, 1) == 0
    assert fn(128, 128, 128, 55) >= 2048 * 55 * 4 and fn(2, 2, 2, 1) > 0


def test_signatures_and_defaults_are_pinned():
    from animatablegaussians_amd import weight_volume as wv
    p = inspect.signature(wv.diffuse_weights).parameters
    assert list(p) == ["target", "fixed", "spacing", "tol", "max_iter", "check_every"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("tol", "max_iter", "check_every"))
    assert (p["tol"].default, p["max_iter"].default, p["check_every"].default) == (1e-5, None, 16)
    p = inspect.signature(wv.WeightVolume.diffuse).parameters
    assert list(p) == ["self", "band", "tol", "max_iter"] and p["band"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("tol", "max_iter")) and (p["tol"].default, p["max_iter"].default) == (1e-5, None)
    p = inspect.signature(wv.WeightVolume.from_body_mesh).parameters
    assert list(p) == ["vertices", "faces", "lbs_weights", "res"] and p["res"].default == 128
    p = inspect.signature(wv.WeightVolume.save).parameters
    assert list(p) == ["self", "path", "alias_diff"] and p["alias_diff"].default is True
    assert wv.WeightVolume.diffused is True and wv.WeightVolume.diffusion is None
    assert np.array_equal(wv.stencil_weights((0.02, 0.02, 0.02)), np.ones(3, np.float32))
    assert np.array_equal(wv.stencil_weights((0.031, 0.02, 0.0173)), wdo.weights((0.031, 0.02, 0.0173)))
    with pytest.raises(ValueError, match="spacing"):
        wv.stencil_weights((0.02, 0.0, 0.02))


def test_host_tensors_are_refused_before_anything_is_launched():
    import torch
    from animatablegaussians_amd import weight_volume as wv
    with pytest.raises(ValueError, match="GPU"):
        wv.diffuse_weights(torch.zeros(3, 3, 3, 2), torch.zeros(3, 3, 3, dtype=torch.bool), (1, 1, 1))
    with pytest.raises(ValueError, match="GPU"):
        wv.diffusion_operator(torch.zeros(3, 3, 3, 2), torch.zeros(3, 3, 3, dtype=torch.bool), (1, 1, 1))
