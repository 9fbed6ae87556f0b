"""The SMPL-X forward VALUES on the GPU (csrc/ag_smplx.hip: shape, prepare, chain, skin, keypoints, mat4_mul_inverse) against the float64
oracle of tests/smplx_forward_oracle.py, at the edges of Rodrigues' formula and of the launch shapes.

Bar, wherever a value meets float64 (that of test_pose_grad_gpu._bar, `smplx_forward_oracle.bar`): within 4 x the float32 oracle's own
deviation from float64 (`d32`) + 2e-6 of the float64 value's scale, in the max norm and in the L2 norm; nothing comes from what the
kernels return.  tests/test_smplx_forward_edges_cpu.py shows that d32 is non-zero on every case below and that five named kernel
mistakes miss this bar by more than ten times.  Every comparison prints GPU error, d32 and the limit.

  A  standard model (V = 10475, J = 55): five input kinds x transl given / None, batch sizes 1 .. 9, the < 400-column shape basis,
     non-zero hand means, 5 betas + 3 expression coefficients; vertices, 127 joints, A, v_shaped, full_pose
  B  bits: a batch equals its single calls, a reversed batch the reversed outputs, transl None equals zeros, a call repeats
  C  data_item on a pose beyond pi and on a zero pose with transl: values against smplx_oracle.data_item, bits against three forwards
  D  models of other sizes and trees through the C interface (GRID_SMALL), guarded output buffers, key-point shapes, refusals
  E  mat4_mul_inverse shapes

Measured on the MI355X, worst case of each section as GPU error / d32 / limit (max norm):
  A kinds     7.4e-7 / 7.9e-7 / 5.1e-6   (A, beyond_pi, B = 3, transl given)
  A batch     6.8e-7 / 6.6e-7 / 4.6e-6   (A, B = 4)
  A variants  8.4e-7 / 9.9e-7 / 6.0e-6   (A, 5 betas + 3 expression coefficients)
  C           4.7e-7 / 4.3e-7 / 3.4e-6   (live_smpl_v, frame 0)
  D           4.9e-7 / 1.4e-7 / 2.9e-6   (v_shaped, V = 97, J = 64, NB = 401, B = 7)
  D keypoints 1.2e-7 / 1.2e-7 / 3.9e-6   (K = 43)
  E           error / (|ref| cond(b)) at most 2.7e-9 against 1e-6 (n = 130, b_batch = 65), cond(b) up to 4462
No case comes nearer than 0.17 of its limit; every bit comparison holds; every refusal returns its code and writes nothing.
Wall time of the file: 3.8 s.
"""
import ctypes
import time

import numpy as np
import pytest

import smplx_forward_oracle as fo

pytestmark = pytest.mark.gpu

WORST = {}          # section -> (error / limit, error, d32, limit, where): printed when the module is done
SENTINEL = -777.25


def _bar(section, got, f64, f32, name):
    (e, d, lim), _ = fo.bar(got, f64, f32, name)
    ratio = e / lim if lim > 0 else 0.0         # limit 0: an exactly zero value (the zero pose's full_pose), met exactly
    if section not in WORST or ratio > WORST[section][0]:
        WORST[section] = (ratio, e, d, lim, name)


@pytest.fixture(scope="module")
def models():
    """variant -> SMPLX on the GPU, each built once for the whole file."""
    import torch
    from animatablegaussians_amd.smplx import SMPLX
    built, t0 = {}, time.time()

    def get(variant):
        if variant not in built:
            kw = dict(flat_hand_mean=True)
            kw.update(fo.VARIANTS[variant][1])
            same = [v for v in fo.VARIANTS if fo.VARIANTS[v][0] == fo.VARIANTS[variant][0]][0]
            built[variant] = SMPLX(fo.standard_arrays(same), gender='neutral', use_pca=False, device=torch.device("cuda", 0), **kw)
        return built[variant]

    fo.assert_equals_committed_oracle(fo.standard_tensors("default", torch.float64))
    fo.assert_equals_committed_oracle(fo.standard_tensors("default", torch.float32))
    yield get
    torch.cuda.synchronize()
    for section in sorted(WORST):
        r, e, d, lim, name = WORST[section]
        print(f"\nworst of section {section}: GPU error {e:.3e}, d32 {d:.3e}, limit {lim:.3e} ({r:.2f} of the limit) at {name}")
    print(f"wall time of the file: {time.time() - t0:.1f} s")


def _run(model, inp, **kw):
    return model(return_full_pose=True, return_shaped=True, **{k: v.cuda() for k, v in inp.items()}, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# A: standard model, values
# ---------------------------------------------------------------------------------------------------------------------------
def _values(models, case, section):
    variant, kind, B, with_transl = case
    inp, o64, o32 = fo.standard_case(*case)
    out = _run(models(variant), inp)
    assert out.joints.shape == (B, 127, 3) and out.A.shape == (B, 55, 4, 4) and (out.transl is None) == (not with_transl)
    for k in ("vertices", "joints", "A", "v_shaped", "full_pose"):
        _bar(section, out[k], o64[k], o32[k], f"{section} {variant} {kind} B={B} transl={with_transl}: {k}")


@pytest.mark.parametrize("case", fo.GRID_KINDS, ids=lambda c: f"{c[1]}-transl{int(c[3])}")
def test_values_at_every_input_kind(models, case):
    _values(models, case, "A.kinds")


@pytest.mark.parametrize("case", fo.GRID_BATCH, ids=lambda c: f"B{c[2]}")
def test_values_at_every_batch_size(models, case):
    _values(models, case, "A.batch")


@pytest.mark.parametrize("case", fo.GRID_VARIANTS, ids=lambda c: c[0])
def test_values_on_the_model_variants(models, case):
    import torch
    model = models(case[0])
    m64 = fo.standard_tensors(case[0], torch.float64)
    assert model._dirs.shape[-1] == m64['shapedirs'].shape[-1] + m64['expr_dirs'].shape[-1]
    assert (float(model.pose_mean.abs().max()) > 0) == (case[0] == "hand_mean")
    if case[0] == "betas5_expr3":           # the oracle takes the coefficients the model keeps; so does the GPU model
        inp, o64, o32 = fo.standard_case(*case)
        inp = dict(inp, betas=inp['betas'][:, :5], expression=inp['expression'][:, :3])
        out = _run(model, inp)
        for k in ("vertices", "joints", "A", "v_shaped", "full_pose"):
            _bar("A.variants", out[k], o64[k], o32[k], f"A.variants {case[0]} beyond_pi B=3: {k}")
    else:
        _values(models, case, "A.variants")


# ---------------------------------------------------------------------------------------------------------------------------
# B: standard model, bits
# ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    import torch
    for k in ("vertices", "joints", "A"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in its bits (max {float((a[k] - b[k]).abs().max()):.3e})"


@pytest.mark.parametrize("B", [2, 3, 4, 6, 7, 8, 9])
def test_a_batch_equals_its_single_calls(models, B):
    """smplx_forward_impl deals B over launches of four poses: 2, 3, 4 | 4 + 2 | 4 + 3 | 4 + 4 | 4 + 4 + 1 -- every NBATCH
    instantiation of the skin kernel runs as a first and as a last launch, and each is compared with NBATCH = 1."""
    import torch
    model = models("default")
    inp = fo.draw_inputs(B, 300 + B, "beyond_pi", True)
    allb = _run(model, inp)
    for i in range(B):
        one = _run(model, {k: v[i:i + 1] for k, v in inp.items()})
        for k in ("vertices", "joints", "A"):
            assert torch.equal(one[k][0], allb[k][i]), f"B={B}, row {i}: {k} of the batch differs from the single call"


def test_batch_order_transl_none_and_repetition(models):
    import torch
    model = models("default")
    inp = fo.draw_inputs(7, 77, "beyond_pi", True)
    a = _run(model, inp)
    b = _run(model, {k: v.flip(0) for k, v in inp.items()})
    _same_bits(a, {k: b[k].flip(0) for k in ("vertices", "joints", "A")}, "reversed batch")
    _same_bits(a, _run(model, inp), "the same call twice")
    no_tr = {k: v for k, v in inp.items() if k != "transl"}
    _same_bits(_run(model, no_tr), _run(model, dict(no_tr, transl=torch.zeros(7, 3))), "transl None against zeros")


# ---------------------------------------------------------------------------------------------------------------------------
# C: data_item
# ---------------------------------------------------------------------------------------------------------------------------
def test_data_item_values_and_bits(models):
    import torch
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    from oracle import smplx_oracle as so
    model = models("default")
    m64, m32 = fo.standard_tensors("default", torch.float64), fo.standard_tensors("default", torch.float32)
    p = fo.item_params()
    go, tr, bp = fo.cano_pose()
    t = {k: torch.from_numpy(v) for k, v in p.items()}
    for i in range(2):
        item = model.data_item(p, i, go, tr, bp)
        i64, i32 = so.data_item(m64, p, i, go, tr, bp), so.data_item(m32, p, i, go, tr, bp)     # float32: inverse by torch.linalg.inv in float32
        for k in fo.ITEM_KEYS:
            cut = (lambda x: x[:22]) if k == "joints" else (lambda x: x)                          # dataset_mv_rgb.py:155
            assert i32[k].dtype == torch.float32
            _bar("C", item[k], cut(i64[k]), cut(i32[k]), f"C frame {i}: {k}")
        s = lambda k: t[k][i:i + 1]  # noqa: E731
        live = model(betas=t['betas'], global_orient=s('global_orient'), body_pose=s('body_pose'), left_hand_pose=s('left_hand_pose'),
                     right_hand_pose=s('right_hand_pose'), transl=s('transl'), expression=s('expression'), jaw_pose=s('jaw_pose'))
        cano = model(betas=t['betas'], global_orient=go[None], body_pose=bp[None], transl=tr[None], expression=s('expression'),
                     jaw_pose=s('jaw_pose'))
        woroot = model(betas=t['betas'], body_pose=s('body_pose'), expression=s('expression'), jaw_pose=s('jaw_pose'))
        c2l = mat4_mul_inverse(torch.stack([live.A[0], woroot.A[0]]), cano.A[0])
        want = {'live_smpl_v': live.vertices[0], 'cano_smpl_v': cano.vertices[0], 'live_smpl_v_woRoot': woroot.vertices[0],
                'joints': live.joints[0, :22], 'cano_jnts': cano.joints[0], 'cano2live_jnt_mats': c2l[0], 'cano2live_jnt_mats_woRoot': c2l[1]}
        for k in fo.ITEM_KEYS:
            assert torch.equal(item[k], want[k]), f"frame {i}: {k} of data_item differs from three forward() calls + mat4_mul_inverse"


# ---------------------------------------------------------------------------------------------------------------------------
# D: small models through the C interface
# ---------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _guarded(n):
    """n floats of NaN with 64 floats of SENTINEL behind them."""
    import torch
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:n] = float("nan")
    return buf


def _written(buf, n, name):
    """Every one of the n floats was written, nothing behind them was."""
    import torch
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:n]).any()), f"{name}: {int(torch.isnan(buf[:n]).sum())} of {n} floats were never written"
    assert bool((buf[n:] == SENTINEL).all()), f"{name}: the kernel wrote behind its output"
    return buf[:n]


def _untouched(buf, n, name):
    import torch
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:n]).all()) and bool((buf[n:] == SENTINEL).all()), f"{name}: a call that should write nothing wrote"


class _CModel:
    """A `small_model` on the device behind an AgSmplxModel, folded by ag_smplx_prepare into guarded buffers."""

    def __init__(self, arrays):
        import torch
        from animatablegaussians_amd import _lib
        self.L = _lib.lib()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
        V, J, NB = arrays['v_template'].shape[0], arrays['J_regressor'].shape[0], arrays['shapedirs'].shape[-1]
        self.V, self.J, self.NB = V, J, NB
        self.keep = {k: up(arrays[k]) for k in ("v_template", "shapedirs", "J_regressor", "lbs_weights")}
        # model_ok wants a non-null posedirs even when there is no pose feature (J = 1): one float nobody reads
        self.keep['posedirs'] = up(arrays['posedirs']) if J > 1 else torch.zeros(1, device="cuda")
        self.keep['parents'] = torch.from_numpy(np.ascontiguousarray(arrays['parents'], np.int32)).cuda()
        m = _lib.AgSmplxModel()
        m.V, m.J, m.NB = V, J, NB
        for k, t in self.keep.items():
            setattr(m, k, t.data_ptr() if t.numel() > 0 else None)
        self.jt, self.jd = _guarded(3 * J), _guarded(3 * J * NB)
        self.stream = _lib.stream(torch.device("cuda", 0))
        rc = self.L.ag_smplx_prepare(ctypes.byref(m), _p(self.jt), _p(self.jd) if NB > 0 else None, self.stream)
        assert rc == 0, self.L.ag_last_error().decode()
        m.joint_template, m.joint_dirs = self.jt.data_ptr(), (self.jd.data_ptr() if NB > 0 else None)
        self.m = m

    def copy(self, **fields):
        from animatablegaussians_amd import _lib
        m = _lib.AgSmplxModel.from_buffer_copy(self.m)
        for k, v in fields.items():
            setattr(m, k, v)
        return m

    def sizes(self, B):
        nws = int(self.L.ag_smplx_workspace_floats(ctypes.byref(self.m), B))
        nsv = int(self.L.ag_smplx_saved_floats(ctypes.byref(self.m), B))
        return nws, nsv

    def outputs(self, B):
        nws, nsv = self.sizes(B)
        return {'vertices': _guarded(3 * B * self.V), 'joints': _guarded(3 * B * self.J), 'A': _guarded(16 * B * self.J), 'ws': _guarded(nws),
                'saved': _guarded(nsv)}

    def forward(self, B, comps, pose, transl, o, m=None, nws=None, keep=False, nsv=None):
        m = self.m if m is None else m
        nws = self.sizes(B)[0] if nws is None else nws
        args = [ctypes.byref(m), B, _p(comps), _p(pose), _p(transl), _p(o['vertices']), _p(o['joints']), _p(o['A']), _p(o['ws']), nws]
        if keep:
            return self.L.ag_smplx_forward_keep(*args, _p(o['saved']), self.sizes(B)[1] if nsv is None else nsv, self.stream)
        return self.L.ag_smplx_forward(*args, self.stream)


@pytest.mark.parametrize("row", fo.GRID_SMALL, ids=lambda c: "-".join(str(x) for x in c))
def test_small_models_through_the_c_interface(row):
    import torch
    V, J, NB, tree, B = row
    c = fo.small_case(*row)
    o64, o32 = c['o64'], c['o32']
    cm = _CModel(c['arrays'])
    tag = f"D V={V} J={J} NB={NB} {tree} B={B}"
    # ag_smplx_prepare: the regressor folded through the shape basis, against the product it replaces
    _bar("D", _written(cm.jt, 3 * J, "joint_template").view(J, 3), c['joint_template64'], c['joint_template32'], f"{tag}: joint_template")
    if NB > 0:
        _bar("D", _written(cm.jd, 3 * J * NB, "joint_dirs").view(J, 3, NB), c['joint_dirs64'], c['joint_dirs32'], f"{tag}: joint_dirs")
    comps, pose = c['comps'].cuda().contiguous(), c['pose'].cuda().contiguous()
    transl = None if c['transl'] is None else c['transl'].cuda().contiguous()
    nws, nsv = cm.sizes(B)
    assert nws == B * (3 * V + 12 * J + 9 * (J - 1)) and nsv == B * (3 * V + 12 * J)
    o = cm.outputs(B)
    assert cm.forward(B, comps, pose, transl, o) == 0, cm.L.ag_last_error().decode()
    got = {'vertices': _written(o['vertices'], 3 * B * V, "vertices").view(B, V, 3), 'joints': _written(o['joints'], 3 * B * J, "joints").view(B, J, 3),
           'A': _written(o['A'], 16 * B * J, "A").view(B, J, 4, 4)}
    _untouched(o['saved'], nsv, "saved (ag_smplx_forward)")
    assert bool((o['ws'][nws:] == SENTINEL).all()), "the kernels wrote behind the workspace"
    for k in ("vertices", "joints", "A"):
        _bar("D", got[k], o64[k], o32[k], f"{tag}: {k}")
    assert bool((got['A'][:, :, 3] == torch.tensor([0., 0., 0., 1.], device="cuda")).all())
    # ag_smplx_forward_keep: the same bits, and what it keeps
    k2 = cm.outputs(B)
    assert cm.forward(B, comps, pose, transl, k2, keep=True) == 0, cm.L.ag_last_error().decode()
    for k, n in (("vertices", 3 * B * V), ("joints", 3 * B * J), ("A", 16 * B * J)):
        assert torch.equal(_written(k2[k], n, k + " (keep)"), o[k][:n]), f"{tag}: {k} of forward_keep differs from forward in its bits"
    saved = _written(k2['saved'], nsv, "saved")
    assert bool((k2['ws'][nws:] == SENTINEL).all())
    _bar("D", saved[:3 * B * V].view(B, V, 3), o64['v_posed'], o32['v_posed'], f"{tag}: saved v_posed")
    _bar("D", saved[3 * B * V:].view(B, J, 3, 4), o64['A_skin'][:, :, :3], o32['A_skin'][:, :, :3], f"{tag}: saved A_skin")
    # ag_smplx_shape
    vs = _guarded(3 * B * V)
    assert cm.L.ag_smplx_shape(ctypes.byref(cm.m), B, _p(comps), _p(vs), cm.stream) == 0, cm.L.ag_last_error().decode()
    _bar("D", _written(vs, 3 * B * V, "v_shaped").view(B, V, 3), o64['v_shaped'], o32['v_shaped'], f"{tag}: v_shaped")


@pytest.mark.parametrize("K", fo.KEYPOINT_KS + (0,))
def test_keypoints_at_the_block_boundary(K):
    """The (V = 97, B = 7) row's float32 oracle vertices through ag_smplx_keypoints: 3 K = 3, 63, 66 and 129 coordinates against blocks of
    64; vertex ids repeat within and across key points."""
    import torch
    from animatablegaussians_amd import _lib
    L = _lib.lib()
    row = (97, 64, 401, "random", 7)
    assert row in fo.GRID_SMALL
    V, B = row[0], row[4]
    x = fo.small_case(*row)['o32']['vertices'].contiguous()
    idx, w = fo.draw_keypoint_table(max(K, 1), V, K)
    out = _guarded(3 * B * K)
    stream = _lib.stream(torch.device("cuda", 0))
    xd, idxd, wd = x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda()
    assert L.ag_smplx_keypoints(_p(out), _p(xd), _p(idxd), _p(wd), B, V, K, stream) == 0, L.ag_last_error().decode()
    if K == 0:
        some = _guarded(3 * B)
        assert L.ag_smplx_keypoints(_p(some), _p(xd), _p(idxd), _p(wd), B, V, 0, stream) == 0
        _untouched(some, 3 * B, "K = 0")
        return
    got = _written(out, 3 * B * K, "keypoints").view(B, K, 3)
    _bar("D.keypoints", got, fo.keypoints(x.double(), idx, w.astype(np.float64)), fo.keypoints(x, idx, w), f"D.keypoints V={V} B={B} K={K}")


def test_refusals_write_nothing():
    import torch
    from animatablegaussians_amd import _lib
    row = (32, 55, 20, "smplx", 4)
    V, J, NB, _, B = row
    c = fo.small_case(*row)
    cm = _CModel(c['arrays'])
    comps, pose, transl = c['comps'].cuda(), c['pose'].cuda(), torch.zeros(B, 3, device="cuda")
    o = cm.outputs(B)
    nws, nsv = cm.sizes(B)
    big = B * (3 * V + 12 * 65)                         # forward_keep sizes `saved` by the model it is handed, J = 65 included
    o['saved'] = _guarded(big)
    INV, SMALL = -1, _lib.AG_ERR_SCRATCH_TOO_SMALL      # include/ag_raster.h

    def refused(rc, code, *words):
        msg = cm.L.ag_last_error().decode()
        print(f"  {rc}: {msg}")
        assert rc == code and all(w in msg for w in words), (rc, msg)

    for keep in (False, True):
        refused(cm.forward(B, comps, pose, transl, o, m=cm.copy(J=65), keep=keep, nsv=big), INV, "bad model")
        refused(cm.forward(B, comps, pose, transl, o, m=cm.copy(J=0), keep=keep, nsv=big), INV, "bad model")
        refused(cm.forward(B, comps, pose, transl, o, nws=nws - 1, keep=keep), SMALL, "workspace too small")
        refused(cm.forward(B, comps, None, transl, o, keep=keep), INV, "null")
        refused(cm.forward(B, None, pose, transl, o, keep=keep), INV, "null")
        refused(cm.forward(B, comps, pose, transl, o, m=cm.copy(joint_template=None), keep=keep, nsv=big), INV, "ag_smplx_prepare")
        refused(cm.forward(B, comps, pose, transl, o, m=cm.copy(joint_dirs=None), keep=keep, nsv=big), INV, "ag_smplx_prepare")
    refused(cm.forward(-1, comps, pose, transl, o), INV, "B < 0")
    refused(cm.forward(B, comps, pose, transl, o, keep=True, nsv=nsv - 1), INV, "saved")
    vs, jt = _guarded(3 * B * V), _guarded(3 * J)
    refused(cm.L.ag_smplx_shape(ctypes.byref(cm.copy(J=65)), B, _p(comps), _p(vs), cm.stream), INV, "bad model")
    refused(cm.L.ag_smplx_shape(ctypes.byref(cm.m), -1, _p(comps), _p(vs), cm.stream), INV, "B < 0")
    refused(cm.L.ag_smplx_shape(ctypes.byref(cm.m), B, None, _p(vs), cm.stream), INV, "null")
    refused(cm.L.ag_smplx_prepare(ctypes.byref(cm.copy(J=0)), _p(jt), _p(cm.jd), cm.stream), INV, "bad model")
    refused(cm.L.ag_smplx_prepare(ctypes.byref(cm.copy(J=65)), _p(jt), _p(cm.jd), cm.stream), INV, "bad model")
    refused(cm.L.ag_smplx_prepare(ctypes.byref(cm.m), None, _p(cm.jd), cm.stream), INV, "null")
    # B = 0 is no error and no work
    assert cm.forward(0, comps, pose, transl, o) == 0 and cm.forward(0, comps, pose, transl, o, keep=True) == 0
    assert cm.L.ag_smplx_shape(ctypes.byref(cm.m), 0, _p(comps), _p(vs), cm.stream) == 0
    assert cm.sizes(0) == (0, 0)
    for k, n in (("vertices", 3 * B * V), ("joints", 3 * B * J), ("A", 16 * B * J), ("ws", nws), ("saved", big)):
        _untouched(o[k], n, k)
    _untouched(vs, 3 * B * V, "v_shaped")
    _untouched(jt, 3 * J, "joint_template")
    # ... and the model still works after all of that
    assert cm.forward(B, comps, pose, None, o) == 0
    _bar("D", _written(o['vertices'], 3 * B * V, "vertices").view(B, V, 3), c['o64']['vertices'], c['o32']['vertices'], "D after the refusals: vertices")


# ---------------------------------------------------------------------------------------------------------------------------
# E: mat4_mul_inverse shapes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b_batch", [(1, 1), (63, 63), (64, 1), (65, 65), (130, 65), (129, 43)])
def test_mat4_mul_inverse_shapes(n, b_batch):
    """b: rigid transforms scaled by 1.3 with translations up to 50 (what `cano.A` is, and then some); a: random.  The criterion of
    test_smplx.test_mat4_mul_inverse_general_matrices: error / (|ref| cond(b)) < 1e-6 against the float64 product."""
    import torch
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    from oracle import smplx_oracle as so
    g = torch.Generator().manual_seed(1000 * n + b_batch)
    a = torch.randn(n, 4, 4, generator=g)
    b = torch.zeros(b_batch, 4, 4)
    b[:, :3, :3] = 1.3 * so.rodrigues(torch.randn(b_batch, 3, generator=g))
    b[:, :3, 3] = (torch.rand(b_batch, 3, generator=g) * 2 - 1) * 50
    b[:, 3, 3] = 1
    reps = n // b_batch
    ref = (a.double().reshape(reps, b_batch, 4, 4) @ torch.linalg.inv(b.double())).reshape(n, 4, 4)
    got = mat4_mul_inverse(a.cuda(), b.cuda()).cpu().double()
    cond = torch.linalg.cond(b.double()).repeat(reps)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    rel = float(((got - ref).abs().amax((1, 2)) / (ref.abs().amax((1, 2)) * cond)).max())
    print(f"E n={n} b_batch={b_batch}: error / (|ref| cond(b)) {rel:.3e} (limit 1e-6), cond(b) up to {float(cond.max()):.1f}")
    assert rel < 1e-6
    if n == 130:                             # a b_batch that does not divide n stays refused
        with pytest.raises(RuntimeError):
            mat4_mul_inverse(a.cuda(), torch.randn(7, 4, 4).cuda())
        with pytest.raises(RuntimeError):
            mat4_mul_inverse(a.cuda(), b[:0].cuda())
