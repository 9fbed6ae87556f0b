"""Host-side checks of what tests/test_smplx_forward_edges_gpu.py stands on (no GPU): the generic oracle equals the committed one, every
input kind reaches the edge it is named after, every tree has its depth, the float32 side of the bar is a measurement (finite and
non-zero on every case the GPU file runs), and the bar is sharp enough to tell five named kernel mistakes from a right kernel by a
factor of ten."""
import math

import numpy as np
import pytest

import smplx_forward_oracle as fo


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_generic_oracle_equals_the_committed_oracle(dtype):
    import torch
    fo.assert_equals_committed_oracle(fo.standard_tensors("default", getattr(torch, dtype)))


def test_generic_oracle_equals_the_committed_oracle_on_the_variants():
    import torch
    for variant in ("dims20", "hand_mean", "betas5_expr3"):
        m = fo.standard_tensors(variant, torch.float64)
        nb, ne = fo.VARIANTS[variant][1].get("num_betas", 10), fo.VARIANTS[variant][1].get("num_expression_coeffs", 10)
        assert m['shapedirs'].shape[-1] == nb and m['expr_dirs'].shape[-1] == ne
        if variant != "betas5_expr3":           # smplx_oracle.forward takes exactly the coefficients the model keeps
            fo.assert_equals_committed_oracle(m)
    assert float(fo.standard_tensors("hand_mean", torch.float64)['left_hand_mean'].abs().max()) > 0
    assert float(fo.standard_tensors("default", torch.float64)['left_hand_mean'].abs().max()) == 0


@pytest.mark.parametrize("kind", fo.KINDS)
def test_each_input_kind_reaches_its_edge(kind):
    import torch
    B = 4
    inp = fo.draw_inputs(B, 11, kind, True)
    pose_keys = [k for k, _ in fo.ARGS if k not in ("betas", "expression", "transl")]
    for k, n in fo.ARGS:
        assert inp[k].shape == (B, n) and inp[k].dtype == torch.float32
    assert "transl" not in fo.draw_inputs(B, 11, kind, False)
    for k in ("betas", "expression"):           # every row its own shape: the rows differ pairwise
        for i in range(B):
            for j in range(i):
                assert float((inp[k][i] - inp[k][j]).abs().max()) > 1e-2, (k, i, j)
    for j, angle in fo.EDGE_ANGLES.get(kind, {}).items():
        got = fo.joint_angles(inp, j)
        # float32 accuracy: well inside the 2e-3 (near_pi: 1e-2) that separates the angle from the multiple of pi next to it
        assert float((got - angle).abs().max()) <= 1e-5, (kind, j, got.tolist(), angle)
        assert float((got - angle).abs().max()) <= (1e-2 if kind == "near_pi" else 2e-3)
    allpose = torch.cat([inp[k] for k in pose_keys], 1)
    if kind == "zero":
        assert bool((allpose == 0).all())
    elif kind == "tiny":
        a = allpose.abs()
        assert float(a.min()) >= float(np.float32(1e-5)) and float(a.max()) <= float(np.float32(1e-3))
        assert float(a.min()) < 3e-5 and float(a.max()) > 3e-4, "the draw covers both ends of [1e-5, 1e-3]"
        assert bool((allpose < 0).any()) and bool((allpose > 0).any())
    else:                                       # the singular point of the reference formula is kept at a distance
        nz = allpose[allpose != 0]
        assert float((nz.double() + 1e-8).abs().min()) >= 1e-6 * (1 - 1e-6)
    if kind == "beyond_pi":
        ang = sorted(float(fo.joint_angles(inp, j)[0]) for j in fo.EDGE_ANGLES[kind])
        assert ang[0] < math.pi < ang[1] < ang[2] < 2 * math.pi < 3 * math.pi < ang[3]


def test_off_the_singularity_moves_what_lands_on_it():
    import torch
    v = torch.tensor([0.0, -1e-8, -1e-8 + 5e-7, -1e-8 - 5e-7, 0.25, -2e-6])
    w = fo._off_the_singularity(v)
    assert w.tolist() == pytest.approx([0.0, 1e-6, 1e-6, 1e-6, 0.25, -2e-6], rel=1e-6)


def test_trees_have_their_depth():
    rng = np.random.default_rng(0)
    for J in (1, 2, 40, 64):
        chain, star = fo.tree_parents("chain", J), fo.tree_parents("star", J)
        assert fo.tree_depth(chain) == J - 1 and fo.tree_depth(star) == min(1, J - 1)
        rnd = fo.tree_parents("random", J, rng)
        assert rnd[0] == -1 and all(0 <= rnd[j] < j for j in range(1, J))
    from animatablegaussians_amd import synth
    assert fo.tree_parents("smplx", 55).tolist() == list(synth.SMPLX_PARENTS) and fo.tree_depth(fo.tree_parents("smplx", 55)) == 10
    assert fo.tree_parents("smplx", 24).tolist() == list(synth.SMPLX_PARENTS[:24])
    for V, J, NB, tree, B in fo.GRID_SMALL:
        a = fo.small_case(V, J, NB, tree, B)['arrays']
        assert a['v_template'].shape == (V, 3) and a['shapedirs'].shape == (V, 3, NB) and a['posedirs'].shape == (9 * (J - 1), 3 * V)
        assert a['J_regressor'].shape == (J, V) and a['lbs_weights'].shape == (V, J) and a['parents'].dtype == np.int32
        assert np.allclose(a['J_regressor'].sum(1), 1) and np.allclose(a['lbs_weights'].sum(1), 1) and (a['J_regressor'] >= 0).all()
        assert ((a['J_regressor'] > 0).sum(1) == min(V, 32)).all() and ((a['lbs_weights'] > 0).sum(1) <= 4).all()
        want = {"chain": J - 1, "star": min(1, J - 1)}.get(tree)
        if want is not None:
            assert fo.tree_depth(a['parents']) == want
    assert fo.tree_depth(fo.small_case(95, 64, 20, "chain", 3)['arrays']['parents']) == 63


def _d32(name, f64, f32):
    import torch
    assert torch.isfinite(f32).all() and torch.isfinite(f64).all(), f"{name}: the oracle is not finite"
    d = float((f32.double() - f64).abs().max())
    assert d > 0, f"{name}: the float32 oracle equals the float64 one -- the bar would be a constant"
    return d


@pytest.mark.parametrize("case", fo.GRID_KINDS + fo.GRID_BATCH + fo.GRID_VARIANTS, ids=lambda c: "-".join(str(x) for x in c))
def test_float32_oracle_is_a_measurement_on_the_standard_grid(case):
    _, o64, o32 = fo.standard_case(*case)
    ds = {k: _d32(f"{case} {k}", o64[k], o32[k]) for k in ("vertices", "joints", "A", "v_shaped")}
    print(case, " ".join(f"{k} {d:.2e}" for k, d in ds.items()))
    assert o64['joints'].shape[1:] == (127, 3) and o64['full_pose'].shape[1] == 165
    assert max(ds.values()) < 1e-5, "float32 loses more than 1e-5 on a body-sized model: the oracle itself is off"


@pytest.mark.parametrize("row", fo.GRID_SMALL, ids=lambda c: "-".join(str(x) for x in c))
def test_float32_oracle_is_a_measurement_on_the_small_grid(row):
    V, J, NB, tree, B = row
    c = fo.small_case(*row)
    assert (c['transl'] is not None) == (B % 2 == 1)
    ds = {k: _d32(f"{row} {k}", c['o64'][k], c['o32'][k]) for k in ("vertices", "joints", "A", "A_skin", "v_posed", "v_shaped")}
    ds['joint_template'] = _d32(f"{row} joint_template", c['joint_template64'], c['joint_template32'])
    if NB > 0:
        ds['joint_dirs'] = _d32(f"{row} joint_dirs", c['joint_dirs64'], c['joint_dirs32'])
        for i in range(B):
            for j in range(i):
                assert float((c['comps'][i] - c['comps'][j]).abs().max()) > 1e-2
    print(row, " ".join(f"{k} {d:.2e}" for k, d in ds.items()))
    for K in fo.KEYPOINT_KS:
        idx, w = fo.draw_keypoint_table(K, V, K)
        assert idx.shape == (K, 3) and 0 <= idx.min() and idx.max() < V and np.allclose(w.sum(1), 1, atol=1e-6)
        assert (idx[0] == idx[0, 0]).all(), "a vertex id repeats within a key point"
        if K > 12:
            assert len(np.unique(idx)) < idx.size // 2, "vertex ids repeat across key points"


@pytest.mark.parametrize("row", fo.GRID_SMALL, ids=lambda c: "-".join(str(x) for x in c))
def test_differentiable_oracle_equals_the_in_place_one_and_its_gradients_are_a_measurement(row):
    """forward_generic(differentiable=True) -- the chain as a list -- returns the in-place form's values exactly, in both dtypes; all
    eight trees have parents[j] < j (the kernel's child gather walks c = j + 1 .. J); the float32 autograd gradients of
    `small_case_gradients` differ from the float64 ones on every row, so the bar of the GPU test is no constant."""
    import torch
    V, J, NB, tree, B = row
    c = fo.small_case(*row)
    par = c['arrays']['parents']
    assert par[0] == -1 and all(0 <= par[j] < j for j in range(1, J))
    for tag in ('64', '32'):
        o = fo.forward_generic(c['m' + tag], c['comps'], c['pose'], c['transl'], differentiable=True)
        for k, v in c['o' + tag].items():
            assert torch.equal(o[k], v), f"{row} float{tag}: {k} of the list-based chain differs from the in-place one"
    for with_transl in (True, False):
        g = fo.small_case_gradients(*row, with_transl)
        for loss in ('chain', 'full'):
            names = ['pose'] + (['comps'] if NB > 0 else []) + (['transl'] if with_transl else [])
            ds = {k: _d32(f"{row} {loss} d{k}", g[loss]['64'][k], g[loss]['32'][k]) / float(g[loss]['64'][k].abs().max()) for k in names}
            print(row, f"transl={with_transl}", loss, " ".join(f"d{k} {d:.2e}" for k, d in ds.items()))
            assert max(ds.values()) < 1e-3, "float32 autograd loses more than 1e-3 of a gradient's scale: the oracle itself is off"
            assert (g[loss]['64']['transl'] is None) == (not with_transl) and g[loss]['64']['comps'].shape == (B, NB)


def test_float32_oracle_is_a_measurement_on_the_data_item():
    import torch
    from oracle import smplx_oracle as so
    import test_smplx
    p = fo.item_params()
    go, tr, bp = fo.cano_pose()
    assert fo.ITEM_KEYS == test_smplx.ITEM_KEYS and all(torch.equal(a, b) for a, b in zip(fo.cano_pose(), test_smplx._cano()))
    ang = [float(np.linalg.norm(p['global_orient'][0].astype(np.float64))), float(np.abs(p['body_pose'][1]).max())]
    assert abs(ang[0] - (math.pi + 1e-3)) < 1e-5 and ang[1] == 0 and float(np.abs(p['transl'][1]).min()) > 0
    for i in range(2):
        i64 = so.data_item(fo.standard_tensors("default", torch.float64), p, i, go, tr, bp)
        i32 = so.data_item(fo.standard_tensors("default", torch.float32), p, i, go, tr, bp)
        for k in fo.ITEM_KEYS:
            assert i32[k].dtype == torch.float32
            print(i, k, f"{_d32(f'frame {i} {k}', i64[k], i32[k]):.2e}")


# The cases the mutants run on are cases of the GPU grids: GRID_KINDS' ("default", "beyond_pi", 3, True), GRID_VARIANTS' ("hand_mean",
# "beyond_pi", 3, True) and GRID_SMALL's (31, 24, 20, "smplx", 2) and (95, 64, 20, "chain", 3).
MUTANT_OUTPUT = {"feature_joint": "vertices", "row0_shape": "vertices", "no_hand_mean": "vertices", "transl_not_on_joints": "joints",
                 "child_first": "A"}


def _exceeds(name, mut, f64, f32, factor=10.0):
    (e, d, lim), (e2, d2, lim2) = fo.bar(mut, f64, f32, name, check=False)
    assert e >= factor * lim, f"{name}: the mistake moves the value by {e:.3e}, less than {factor} x the bar {lim:.3e}"
    assert e2 >= factor * lim2, f"{name}: the mistake moves the value by {e2:.3e} in L2, less than {factor} x the bar {lim2:.3e}"


@pytest.mark.parametrize("mutant", fo.MUTANTS)
def test_the_bar_tells_a_wrong_kernel_on_the_standard_model(mutant):
    import torch
    case = ("hand_mean" if mutant == "no_hand_mean" else "default", "beyond_pi", 3, True)
    assert case in fo.GRID_KINDS + fo.GRID_VARIANTS
    inp, o64, o32 = fo.standard_case(*case)
    mut = fo.standard_forward(fo.standard_tensors(case[0], torch.float64), inp, mutant)
    k = MUTANT_OUTPUT[mutant]
    _exceeds(f"{mutant} on {case}, {k}", mut[k], o64[k], o32[k])
    if mutant == "transl_not_on_joints":        # ... and only there: the vertices, the key points and A carry transl
        assert torch.equal(mut['vertices'], o64['vertices']) and torch.equal(mut['A'], o64['A']) and torch.equal(mut['joints'][:, 55:], o64['joints'][:, 55:])


@pytest.mark.parametrize("mutant", [m for m in fo.MUTANTS if m != "no_hand_mean"])      # a small model has no hand means
def test_the_bar_tells_a_wrong_kernel_on_a_small_model(mutant):
    row = (95, 64, 20, "chain", 3) if mutant == "transl_not_on_joints" else (31, 24, 20, "smplx", 2)
    assert row in fo.GRID_SMALL
    c = fo.small_case(*row)
    assert mutant != "transl_not_on_joints" or c['transl'] is not None
    comps, pose = fo.mutate_inputs(None, c['comps'], c['pose'], mutant)
    mut = fo.forward_generic(c['m64'], comps, pose, c['transl'], mutant if mutant not in ("row0_shape",) else None)
    k = MUTANT_OUTPUT[mutant]
    _exceeds(f"{mutant} on {row}, {k}", mut[k], c['o64'][k], c['o32'][k])
