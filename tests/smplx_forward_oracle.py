"""Generic float64 / float32 oracle of the SMPL-X forward VALUES -- TEST INFRASTRUCTURE ONLY.

oracle/smplx_oracle.forward is written for the one model the reference builds (55 joints, 165 pose numbers, 21 vertex picks).  The
kernels of csrc/ag_smplx.hip take any V, J <= 64, NB and parent table, so `forward_generic` restates smplx/lbs.py:152-246 and
body_models.py:1272-1275 on (shape components, full pose, transl) -- the arguments of ag_smplx_forward -- from the committed oracle's
own `rodrigues` and `rigid_chain`, in its order of operations: on the standard model it returns smplx_oracle.forward's values exactly
(`assert_equals_committed_oracle`).  It also returns what the kernels keep between launches (v_shaped, v_posed, the rest joints, the
pose features, the un-translated A), which the C interface exposes through `ag_smplx_shape` and the `saved` block of
`ag_smplx_forward_keep`.

`small_model` draws models of any size and tree, `draw_inputs` the standard model's arguments at the edges of Rodrigues' formula,
`draw_generic` the same edges for a J-joint model.  `GRID_*` are the cases the GPU tests run; the CPU tests walk the same lists.

`MUTANTS` are five named mistakes a kernel could make; `forward_generic(..., mutant=...)` / `mutate_inputs` commit them on purpose so
that the CPU tests can show the bar of the GPU tests tells them from a right kernel.
"""
import functools
import math

import numpy as np
import torch

ARGS = (("betas", 10), ("global_orient", 3), ("body_pose", 63), ("left_hand_pose", 45), ("right_hand_pose", 45), ("transl", 3),
        ("expression", 10), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3))
KINDS = ("random", "zero", "tiny", "near_pi", "beyond_pi")
# joint of full_pose -> rotation angle the kind puts there (every row, each about an axis of its own)
EDGE_ANGLES = {
    "near_pi": {5: math.pi - 1e-2},           # body_pose[:, 12:15], the joint smplx_vertex_oracle.draw_inputs bends
    "beyond_pi": {4: math.pi - 1e-3, 0: math.pi + 1e-3, 15: 2 * math.pi - 1e-3, 18: 3 * math.pi + 0.2},
}
MUTANTS = ("feature_joint", "row0_shape", "no_hand_mean", "transl_not_on_joints", "child_first")

# ---- the cases of tests/test_smplx_forward_edges_gpu.py --------------------------------------------------------------------------
VARIANTS = {                                  # name -> (smplx_model_arrays arguments, SMPLX / model_tensors arguments)
    "default": ({}, {}),
    "dims20": ({"shape_dims": 20}, {}),
    "hand_mean": ({}, {"flat_hand_mean": False}),
    "betas5_expr3": ({}, {"num_betas": 5, "num_expression_coeffs": 3}),
}
GRID_KINDS = tuple(("default", kind, 3, tr) for kind in KINDS for tr in (True, False))
GRID_BATCH = tuple(("default", "beyond_pi", B, True) for B in (1, 2, 4, 5, 7, 8, 9))
GRID_VARIANTS = tuple((v, "beyond_pi", 3, True) for v in ("dims20", "hand_mean", "betas5_expr3"))
GRID_SMALL = ((1, 2, 1, "chain", 1), (31, 24, 20, "smplx", 2), (32, 55, 20, "smplx", 4), (33, 55, 0, "smplx", 5),
              (95, 64, 20, "chain", 3), (97, 64, 401, "random", 7), (257, 1, 20, "star", 2), (64, 40, 300, "star", 9))
KEYPOINT_KS = (1, 21, 22, 43)                 # 3 K = 63 and 66 straddle the 64-thread block of smplx_keypoints_kernel


def case_seed(*case):
    """One seed per case, a pure function of the case (no hash(): that changes between interpreter runs)."""
    s = 17
    for x in case:
        for ch in str(x):
            s = (s * 131 + ord(ch)) % 1000003
    return s


# ---- the bar ----------------------------------------------------------------------------------------------------------------------
def bar(got, f64, f32, name, check=True):
    """test_pose_grad_gpu._bar: |got - float64| <= 4 |float32 oracle - float64 oracle| + 2e-6 scale of the float64 value, in the max
    norm and in the L2 norm.  Prints the three figures; returns (error, d32, limit) of both norms."""
    got, f64, f32 = (t.detach().cpu().double() for t in (got, f64, f32))
    assert got.shape == f64.shape == f32.shape, f"{name}: shapes {tuple(got.shape)}, {tuple(f64.shape)}, {tuple(f32.shape)}"
    e_max, e_l2 = float((got - f64).abs().max()), float((got - f64).norm())
    d_max, d_l2 = float((f32 - f64).abs().max()), float((f32 - f64).norm())
    lim_max = 4 * d_max + 2e-6 * float(f64.abs().max())
    lim_l2 = 4 * d_l2 + 2e-6 * float(f64.norm())
    print(f"{name}: max error {e_max:.3e} (limit {lim_max:.3e}, fp32 oracle {d_max:.3e}), L2 error {e_l2:.3e} (limit {lim_l2:.3e}, "
          f"fp32 oracle {d_l2:.3e})")
    if check:
        assert torch.isfinite(got).all(), f"{name}: non-finite values"
        assert e_max <= lim_max, f"{name}: max error {e_max:.3e} > {lim_max:.3e} (fp32 oracle {d_max:.3e})"
        assert e_l2 <= lim_l2, f"{name}: L2 error {e_l2:.3e} > {lim_l2:.3e} (fp32 oracle {d_l2:.3e})"
    return (e_max, d_max, lim_max), (e_l2, d_l2, lim_l2)


# ---- the forward --------------------------------------------------------------------------------------------------------------------
def _dirs(m):
    return m['dirs'] if 'dirs' in m else torch.cat([m['shapedirs'], m['expr_dirs']], -1)


def _chain_child_first(R, Jrest, parents):
    """smplx_oracle.rigid_chain with the one product the wrong way round (mutant `child_first`)."""
    B, Jn = R.shape[:2]
    G = torch.zeros(B, Jn, 4, 4, dtype=R.dtype)
    for j in range(Jn):
        M = torch.zeros(B, 4, 4, dtype=R.dtype)
        M[:, :3, :3] = R[:, j]
        M[:, 3, 3] = 1
        p = int(parents[j])
        M[:, :3, 3] = Jrest[:, j] - (Jrest[:, p] if p >= 0 else 0)
        G[:, j] = M if p < 0 else M @ G[:, p]
    A = G.clone()
    A[:, :, :3, 3] -= (G[:, :, :3, :3] @ Jrest[..., None])[..., 0]
    return G[:, :, :3, 3], A


def _chain_as_list(R, Jrest, parents):
    """smplx_oracle.rigid_chain for autograd: that one fills its [B, J, 4, 4] chain in place while later joints read earlier rows, which
    autograd refuses to differentiate.  Same products in the same order, the chain kept as a list and A put together by concatenation
    (test_pose_grad_gpu._smplx_chain_oracle does this for the standard model): the values are those of rigid_chain exactly."""
    B, Jn = R.shape[:2]
    bottom = torch.zeros(B, 1, 4, dtype=R.dtype)
    bottom[..., 3] = 1
    G = []
    for j in range(Jn):
        p = int(parents[j])
        t = Jrest[:, j] - (Jrest[:, p] if p >= 0 else 0)
        M = torch.cat([torch.cat([R[:, j], t[..., None]], 2), bottom], 1)
        G.append(M if p < 0 else G[p] @ M)
    G = torch.stack(G, 1)
    rel = G[:, :, :3, 3] - (G[:, :, :3, :3] @ Jrest[..., None])[..., 0]
    return G[:, :, :3, 3], torch.cat([torch.cat([G[:, :, :3, :3], rel[..., None]], 3), G[:, :, 3:]], 2)


def forward_generic(m, comps, full_pose, transl=None, mutant=None, differentiable=False):
    """m: v_template [V,3], dirs [V,3,NB] (or shapedirs + expr_dirs, as smplx_oracle.model_tensors keeps them), posedirs [9(J-1), 3V],
    J_regressor [J,V], parents [J], lbs_weights [V,J], all of one dtype.  comps [B,NB]; full_pose [B,J,3] or [B,3J] with the pose mean
    already added; transl [B,3] or None.  Returns v_shaped, v_posed, rest joints, pose_feature, A_skin (before transl), A, joints
    (posed, [B,J,3]), vertices and `skinned` (the vertices before transl), in the arithmetic and order of smplx_oracle.forward.
    `mutant`: one of the in-model MUTANTS.  `differentiable`: the chain through `_chain_as_list`, so that torch autograd runs through
    the result (same values)."""
    from oracle import smplx_oracle as so
    assert mutant in (None, "feature_joint", "transl_not_on_joints", "child_first"), mutant
    assert not (differentiable and mutant == "child_first")
    dt = m['v_template'].dtype
    dirs = _dirs(m)
    V, Jn = dirs.shape[0], m['J_regressor'].shape[0]
    B = full_pose.shape[0]
    comps, full_pose = comps.to(dt).reshape(B, dirs.shape[-1]), full_pose.to(dt)
    v_shaped = m['v_template'] + (dirs.reshape(V * 3, -1) @ comps.T).T.reshape(B, V, 3)
    Jrest = torch.einsum('jv,bvc->bjc', m['J_regressor'], v_shaped)
    R = so.rodrigues(full_pose.reshape(B, -1, 3))
    assert R.shape[1] == Jn, f"full_pose has {R.shape[1]} joints, the model {Jn}"
    eye = torch.eye(3, dtype=dt)
    if mutant == "feature_joint":               # (a) pose features of joints 0 .. J-2 where 1 .. J-1 belong
        feat = (R[:, :-1] - eye).reshape(B, -1)
    else:
        feat = (R[:, 1:] - eye).reshape(B, -1)
    v_posed = v_shaped + (feat @ m['posedirs']).reshape(B, V, 3)
    chain = _chain_child_first if mutant == "child_first" else _chain_as_list if differentiable else so.rigid_chain
    Jposed, A = chain(R, Jrest, m['parents'])
    A_skin = A
    T = (m['lbs_weights'] @ A.reshape(B, -1, 16)).reshape(B, V, 4, 4)
    verts = skinned = (T[..., :3, :3] @ v_posed[..., None])[..., 0] + T[..., :3, 3]
    if transl is not None:
        tr = transl.to(dt).reshape(-1, 1, 3)
        verts = verts + tr
        if mutant != "transl_not_on_joints":    # (d)
            Jposed = Jposed + tr
        A = A.clone()
        A[:, :, :3, 3] += tr
    return {'v_shaped': v_shaped, 'v_posed': v_posed, 'rest_joints': Jrest, 'pose_feature': feat, 'A_skin': A_skin, 'A': A,
            'joints': Jposed, 'vertices': verts, 'skinned': skinned}


def keypoints(vertices, idx, w):
    """out[b][k] = sum_t w[k][t] vertices[b][idx[k][t]] (vertex_joint_selector.py:72-76, lbs.py:108-149), summed as
    smplx_oracle.forward sums its landmarks."""
    idx = torch.as_tensor(np.asarray(idx)).long()
    if idx.shape[0] == 0:
        return vertices.new_zeros(vertices.shape[0], 0, 3)
    return (vertices[:, idx] * torch.as_tensor(w).to(vertices.dtype)[None, :, :, None]).sum(2)


def standard_keypoint_table(m):
    """idx [72,3], w [72,3] of the 21 vertex picks and 51 face landmarks of a smplx_oracle.model_tensors dict."""
    from oracle import smplx_oracle as so
    dt = m['v_template'].dtype
    extra = torch.as_tensor(so.EXTRA_JOINT_VERTS)[:, None].expand(-1, 3)
    idx = torch.cat([extra, m['faces'][m['lmk_faces_idx']]], 0)
    w = torch.cat([torch.tensor([[1., 0., 0.]], dtype=dt).expand(len(extra), -1), m['lmk_bary_coords']], 0)
    return idx, w


def assemble(m, inp):
    """The standard model's arguments -> (comps [B,NB], full_pose [B,165] with the hand means, transl or None), body_models.py:1203-1233.
    betas / expression are cut to the coefficients the model keeps."""
    dt = m['v_template'].dtype
    B = inp['betas'].shape[0]
    g = lambda k, n: inp[k].to(dt) if k in inp else torch.zeros(B, n, dtype=dt)  # noqa: E731
    full_pose = torch.cat([g('global_orient', 3), g('body_pose', 63), g('jaw_pose', 3), g('leye_pose', 3), g('reye_pose', 3),
                           g('left_hand_pose', 45), g('right_hand_pose', 45)], 1)
    full_pose = full_pose + torch.cat([torch.zeros(75, dtype=dt), m['left_hand_mean'], m['right_hand_mean']])
    nb, ne = m['shapedirs'].shape[-1], m['expr_dirs'].shape[-1]
    comps = torch.cat([g('betas', 10)[:, :nb], g('expression', 10)[:, :ne]], 1)
    return comps, full_pose, (inp['transl'].to(dt) if 'transl' in inp else None)


def mutate_inputs(m, comps, full_pose, mutant):
    """The two MUTANTS that sit ahead of the kernels: (b) every row reads row 0's shape components, (c) the hand means left out."""
    if mutant == "row0_shape":
        comps = comps[:1].expand(comps.shape[0], -1)
    if mutant == "no_hand_mean":
        full_pose = full_pose - torch.cat([torch.zeros(75, dtype=full_pose.dtype), m['left_hand_mean'], m['right_hand_mean']])
    return comps, full_pose


def standard_forward(m, inp, mutant=None):
    """SMPLX.forward's outputs on a smplx_oracle.model_tensors dict: vertices, joints [B,127,3], A, v_shaped (the betas alone,
    body_models.py:1277-1279), full_pose, plus forward_generic's intermediates."""
    comps, full_pose, transl = assemble(m, inp)
    comps, full_pose = mutate_inputs(m, comps, full_pose, mutant)
    out = forward_generic(m, comps, full_pose, transl, mutant if mutant in ("feature_joint", "transl_not_on_joints", "child_first") else None)
    idx, w = standard_keypoint_table(m)          # the picks carry weights (1, 0, 0): taken directly, as smplx_oracle.forward takes them
    kp = torch.cat([out['skinned'][:, idx[:21, 0]], keypoints(out['skinned'], idx[21:], w[21:])], 1)
    if transl is not None:                       # body_models.py:1272-1275: the key points are taken first, transl is added to all joints
        kp = kp + transl.reshape(-1, 1, 3)
    nb = m['shapedirs'].shape[-1]
    V = m['v_template'].shape[0]
    betas = comps[:, :nb]
    only_betas = m['v_template'] + (m['shapedirs'].reshape(V * 3, nb) @ betas.T).T.reshape(-1, V, 3)
    out.update(joints=torch.cat([out['joints'], kp], 1), v_shaped=only_betas, full_pose=full_pose)
    return out


def assert_equals_committed_oracle(m, B=3, seed=5):
    """The restatement is pinned to oracle/smplx_oracle.forward on the standard model: identical values on the vertices, A and the 55
    chain joints through `forward_generic`, and on all 127 joints through `standard_forward`."""
    from oracle import smplx_oracle as so
    dt = m['v_template'].dtype
    inp = draw_inputs(B, seed, "beyond_pi")
    x = {k: v.to(dt) for k, v in inp.items()}
    ref = so.forward(m, **x)
    comps, full_pose, transl = assemble(m, x)
    mine = forward_generic(m, comps, full_pose, transl)
    full = standard_forward(m, x)
    for k, a, b in (('vertices', mine['vertices'], ref['vertices']), ('A', mine['A'], ref['A']), ('joints[:, :55]', mine['joints'], ref['joints'][:, :55]),
                    ('joints', full['joints'], ref['joints']), ('full_pose', full['full_pose'], ref['full_pose'])):
        d = float((a - b).abs().max())
        assert a.shape == b.shape and d == 0.0, f"{k} ({dt}): restatement differs from smplx_oracle.forward by {d:.3e}"
    assert full['joints'].shape[1] == 127 and mine['joints'].shape[1] == 55


# ---- models -------------------------------------------------------------------------------------------------------------------------
def tree_parents(tree, J, rng=None):
    from animatablegaussians_amd import synth
    if tree == "smplx":
        assert J <= len(synth.SMPLX_PARENTS)
        par = list(synth.SMPLX_PARENTS[:J])
    elif tree == "chain":
        par = [j - 1 for j in range(J)]
    elif tree == "star":
        par = [-1] + [0] * (J - 1)
    elif tree == "random":
        par = [-1] + [int(rng.integers(0, j)) for j in range(1, J)]
    else:
        raise ValueError(tree)
    return np.asarray(par, np.int32)


def tree_depth(parents):
    depth = [0] * len(parents)
    for j in range(1, len(parents)):
        depth[j] = depth[int(parents[j])] + 1
    return max(depth)


def small_model(V, J, NB, tree, seed):
    """float64 arrays in the layout AgSmplxModel reads: v_template [V,3], shapedirs [V,3,NB], posedirs [9(J-1), 3V], J_regressor [J,V],
    parents [J] int32 (parents[0] = -1), lbs_weights [V,J].  Sized as synth.smplx_model_arrays: vertices in a 0.6 x 1.7 x 0.3 m box, 1-cm
    shape and 2-mm pose-corrective bases, each joint a convex combination of min(V, 32) vertices, 4 skinning weights per vertex."""
    rng = np.random.default_rng(seed)
    P = 9 * (J - 1)
    m = {'v_template': (rng.random((V, 3)) - 0.5) * np.array([0.6, 1.7, 0.3]),
         'shapedirs': rng.standard_normal((V, 3, NB)) * 0.01,
         'posedirs': rng.standard_normal((P, 3 * V)) * 0.002}
    n = min(V, 32)
    Jr = np.zeros((J, V))
    for j in range(J):
        idx = rng.choice(V, n, replace=False)
        w = rng.random(n) + 0.05
        Jr[j, idx] = w / w.sum()
    m['J_regressor'] = Jr
    W = np.zeros((V, J))
    for k, idx in enumerate(rng.integers(0, J, (4, V))):
        W[np.arange(V), idx] += rng.random(V) + (1.0 if k == 0 else 0.0)
    m['lbs_weights'] = W / W.sum(1, keepdims=True)
    m['parents'] = tree_parents(tree, J, rng)
    return m


def small_tensors(arrays, dtype):
    """`small_model` arrays -> what forward_generic reads."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    return {'v_template': t(arrays['v_template']), 'dirs': t(arrays['shapedirs']), 'posedirs': t(arrays['posedirs']),
            'J_regressor': t(arrays['J_regressor']), 'parents': torch.as_tensor(np.asarray(arrays['parents'], np.int64)),
            'lbs_weights': t(arrays['lbs_weights'])}


@functools.lru_cache(maxsize=None)
def standard_arrays(variant):
    from animatablegaussians_amd import synth
    return synth.smplx_model_arrays(**VARIANTS[variant][0])


@functools.lru_cache(maxsize=None)
def standard_tensors(variant, dtype):
    """smplx_oracle.model_tensors of one of VARIANTS; built once and shared (nobody writes into them)."""
    from oracle import smplx_oracle as so
    same = [v for v in VARIANTS if VARIANTS[v][0] == VARIANTS[variant][0]][0]
    return so.model_tensors(standard_arrays(same), dtype, **VARIANTS[variant][1])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _off_the_singularity(v):
    """angle = |rv + 1e-8| vanishes at rv = (-1e-8, -1e-8, -1e-8): there axis = rv / angle is 0 / 0 and the reference formula itself is
    singular.  Every NON-ZERO pose component is kept at least 1e-6 away from -1e-8 (moved to +1e-6 if a draw lands closer); an exact
    zero stays: it is the reference's default pose and regular (angle = sqrt(3) 1e-8, axis 0)."""
    near = (v != 0) & ((v + 1e-8).abs() < 1e-6)
    return torch.where(near, torch.full_like(v, 1e-6), v)


def _axes(n, g):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)


def _set_joint(inp, j, rv):
    if j == 0:
        inp["global_orient"] = rv
    else:
        assert 1 <= j <= 21
        inp["body_pose"][:, 3 * (j - 1):3 * j] = rv


def draw_inputs(B, seed, kind="random", with_transl=True):
    """float32 arguments of SMPLX.forward for B poses; every row has betas and an expression of its own (a kernel that read row 0's
    for every pose would be caught).  Kinds:
      random     smplx_vertex_oracle.draw_inputs: N(0, 0.3) pose components, N(0, 1) shape and expression
      zero       every pose argument exactly 0, shape / expression / transl random
      tiny       every pose component +-10^u, u uniform in [-5, -3]: sin(angle) / angle and (1 - cos(angle)) / angle^2 at their limits
      near_pi    random, one joint (EDGE_ANGLES) at pi - 1e-2
      beyond_pi  random, four joints (EDGE_ANGLES) at pi -+ 1e-3, 2 pi - 1e-3 and 3 pi + 0.2, each about a random axis per row
    Singularity of the reference formula: see _off_the_singularity; zero rows are exact zeros, tiny rows lie in [1e-5, 1e-3], the
    rest is moved off it."""
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(seed)
    inp = {}
    for name, n in ARGS:
        if name == "transl" and not with_transl:
            continue
        scale = {"betas": 1.0, "expression": 1.0}.get(name, 0.3)
        v = torch.randn(B, n, generator=g) * scale
        if name not in ("betas", "expression", "transl"):
            if kind == "zero":
                v = torch.zeros(B, n)
            elif kind == "tiny":
                u = torch.rand(B, n, generator=g) * 2 - 5
                sign = (torch.rand(B, n, generator=g) < 0.5).float() * 2 - 1
                v = (sign * 10.0 ** u.double()).float().clamp(-1e-3, 1e-3)
                v = torch.where(v.abs() < 1e-5, torch.copysign(torch.full_like(v, 1e-5), v), v)
            else:
                v = _off_the_singularity(v)
        inp[name] = v
    for j, angle in EDGE_ANGLES.get(kind, {}).items():
        _set_joint(inp, j, _axes(B, g) * angle)
    return inp


def joint_angles(inp, j):
    rv = inp["global_orient"] if j == 0 else inp["body_pose"][:, 3 * (j - 1):3 * j]
    return rv.double().norm(dim=1)


def draw_generic(B, J, NB, seed, with_transl=True):
    """(comps [B,NB], full_pose [B,J,3], transl) for a `small_model`, float32: N(0, 0.3) pose components with the root at pi + 1e-3, the
    last joint at 2 pi - 1e-3, joint J // 2 at 3 pi + 0.2 and joint 1 at pi - 1e-3 where the model has them (later entries win on a
    short tree); from B = 3 on, row 1 is the zero pose and row 2 a tiny one.  Every row has components of its own."""
    g = torch.Generator().manual_seed(seed)
    comps = torch.randn(B, NB, generator=g)
    pose = _off_the_singularity(torch.randn(B, J, 3, generator=g) * 0.3)
    for j, angle in ((1, math.pi - 1e-3), (J // 2, 3 * math.pi + 0.2), (J - 1, 2 * math.pi - 1e-3), (0, math.pi + 1e-3)):
        if j < J:
            pose[:, j] = _axes(B, g) * angle
    if B >= 3:
        pose[1] = 0
        u = torch.rand(J, 3, generator=g) * 2 - 5
        sign = (torch.rand(J, 3, generator=g) < 0.5).float() * 2 - 1
        pose[2] = (sign * 10.0 ** u.double()).float().clamp(-1e-3, 1e-3)
        pose[2] = torch.where(pose[2].abs() < 1e-5, torch.copysign(torch.full_like(pose[2], 1e-5), pose[2]), pose[2])
    transl = torch.randn(B, 3, generator=g) * 0.5 if with_transl else None
    return comps, pose, transl


@functools.lru_cache(maxsize=None)
def standard_case(variant, kind, B, with_transl):
    """(inputs, float64 oracle, float32 oracle) of one GRID_KINDS / GRID_BATCH / GRID_VARIANTS case: computed once, never modified."""
    inp = draw_inputs(B, case_seed(variant, kind, B, with_transl), kind, with_transl)
    return inp, standard_forward(standard_tensors(variant, torch.float64), inp), standard_forward(standard_tensors(variant, torch.float32), inp)


@functools.lru_cache(maxsize=None)
def small_case(V, J, NB, tree, B):
    """One GRID_SMALL row: the model's arrays, its inputs (transl given on the odd batch sizes, NULL on the even ones), both oracles
    and the folded joint regressor in both precisions.  Computed once, never modified."""
    arrays = small_model(V, J, NB, tree, case_seed(V, J, NB, tree))
    comps, pose, transl = draw_generic(B, J, NB, case_seed(V, J, NB, tree, B), with_transl=B % 2 == 1)
    case = {'arrays': arrays, 'comps': comps, 'pose': pose, 'transl': transl}
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        m = small_tensors(arrays, dt)
        case['m' + tag] = m
        case['o' + tag] = forward_generic(m, comps, pose, transl)
        case['joint_template' + tag] = m['J_regressor'] @ m['v_template']
        case['joint_dirs' + tag] = torch.einsum('jv,vcl->jcl', m['J_regressor'], m['dirs'])
    return case


@functools.lru_cache(maxsize=None)
def small_case_gradients(V, J, NB, tree, B, with_transl):
    """Torch autograd through `forward_generic(..., differentiable=True)` on one GRID_SMALL row (its model, components and pose; a transl
    of this function's own, or None), in float64 and float32, for two losses with seeded weights:
      chain  sum(A wA) + sum(joints wJ)                 what ag_smplx_backward differentiates
      full   chain + sum(vertices wV)                   ag_smplx_vertex_backward -> ag_smplx_backward_full
    Returns transl, wA [B,J,4,4] (row 3 meets the constant row of A: no gradient), wJ, wV and g[loss][dtype tag] = {pose, comps, transl
    (None without transl)}.  Computed once, never modified."""
    c = small_case(V, J, NB, tree, B)
    g = torch.Generator().manual_seed(case_seed(V, J, NB, tree, B, "gradients"))
    wA, wJ, wV = torch.randn(B, J, 4, 4, generator=g), torch.randn(B, J, 3, generator=g), torch.randn(B, V, 3, generator=g)
    transl = torch.randn(B, 3, generator=g) * 0.5 if with_transl else None
    out = {'transl': transl, 'wA': wA, 'wJ': wJ, 'wV': wV, 'chain': {}, 'full': {}}
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        x = [t.detach().to(dt).clone().requires_grad_(True) for t in (c['pose'], c['comps']) + ((transl,) if with_transl else ())]
        o = forward_generic(c['m' + tag], x[1], x[0], x[2] if with_transl else None, differentiable=True)
        chain = (o['A'] * wA.to(dt)).sum() + (o['joints'] * wJ.to(dt)).sum()
        for loss, L in (('chain', chain), ('full', chain + (o['vertices'] * wV.to(dt)).sum())):
            gr = torch.autograd.grad(L, x, retain_graph=True)
            out[loss][tag] = {'pose': gr[0], 'comps': gr[1], 'transl': gr[2] if with_transl else None}
    return out


ITEM_KEYS = ("live_smpl_v", "cano_smpl_v", "live_smpl_v_woRoot", "joints", "cano_jnts", "cano2live_jnt_mats", "cano2live_jnt_mats_woRoot")


def cano_pose():
    """The canonical pose of test_smplx._cano (config.py:9-15): global_orient, transl, body_pose."""
    cp = np.zeros(75, np.float32)
    cp[3 + 3 * 1 + 2] = math.radians(25)
    cp[3 + 3 * 2 + 2] = math.radians(-25)
    cp = torch.from_numpy(cp)
    return cp[3:6], cp[:3], cp[6:69]


def item_params(seed=41):
    """Two frames of smpl_params.npz arrays (synth.smplx_pose_params' keys): frame 0 is a `beyond_pi` pose (root at pi + 1e-3), frame 1
    the zero pose with a non-zero transl.  One betas row for the subject, as the dataset holds it."""
    inp = draw_inputs(2, seed, "beyond_pi", True)
    p = {k: inp[k].clone() for k in ("global_orient", "transl", "body_pose", "jaw_pose", "expression", "left_hand_pose", "right_hand_pose")}
    for k in p:
        if k not in ("transl", "expression"):
            p[k][1] = 0
    p["betas"] = inp["betas"][:1].clone()
    return {k: v.numpy() for k, v in p.items()}


def draw_keypoint_table(K, V, seed):
    """idx [K,3] int32, w [K,3] float32: vertex ids repeat within a key point (every third one names one vertex three times, as the
    vertex picks do) and across key points (ids come from a pool of min(V, 12) vertices)."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(V, min(V, 12), replace=False)
    idx = pool[rng.integers(0, len(pool), (K, 3))]
    idx[::3] = idx[::3, :1]
    w = rng.random((K, 3)) + 0.1
    w /= w.sum(1, keepdims=True)
    return idx.astype(np.int32), w.astype(np.float32)
