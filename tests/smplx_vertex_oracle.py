"""float64 / float32 autograd oracle of every SMPLX.forward output -- TEST INFRASTRUCTURE ONLY.

oracle/smplx_oracle.forward restated so that autograd can run through it: its rigid_chain fills the [B, J, 4, 4] chain in place while
later joints read earlier rows, which autograd refuses.  Same arithmetic in the same order (smplx/lbs.py:208-246, :347-405,
body_models.py:1185-1290), the chain kept as a list and `A` assembled by concatenation; tests assert that the values equal
smplx_oracle.forward's exactly.  Adds `v_shaped` (body_models.py:1277-1279: the betas alone)."""
import torch

ARGS = (("betas", 10), ("global_orient", 3), ("body_pose", 63), ("left_hand_pose", 45), ("right_hand_pose", 45), ("transl", 3),
        ("expression", 10), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3))


def forward(m, x):
    """m: smplx_oracle.model_tensors(...); x: dict of the ARGS present (betas required).  Returns vertices, joints [B, 127, 3], A,
    v_shaped."""
    from oracle import smplx_oracle as so
    dt = m['v_template'].dtype
    B = x['betas'].shape[0]
    z = lambda n: torch.zeros(B, n, dtype=dt)  # noqa: E731
    g = lambda k, n: x[k] if k in x else z(n)  # noqa: E731
    full_pose = torch.cat([g('global_orient', 3), g('body_pose', 63), g('jaw_pose', 3), g('leye_pose', 3), g('reye_pose', 3),
                           g('left_hand_pose', 45), g('right_hand_pose', 45)], 1)
    full_pose = full_pose + torch.cat([torch.zeros(75, dtype=dt), m['left_hand_mean'], m['right_hand_mean']])
    comps = torch.cat([x['betas'], g('expression', m['expr_dirs'].shape[-1])], 1)
    dirs = torch.cat([m['shapedirs'], m['expr_dirs']], -1)
    V = dirs.shape[0]
    v_shaped = m['v_template'] + (dirs.reshape(V * 3, -1) @ comps.T).T.reshape(B, V, 3)
    Jrest = torch.einsum('jv,bvc->bjc', m['J_regressor'], v_shaped)
    R = so.rodrigues(full_pose.reshape(B, -1, 3))
    feat = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, -1)
    v_posed = v_shaped + (feat @ m['posedirs']).reshape(B, V, 3)
    parents = m['parents']
    bottom = torch.zeros(B, 1, 4, dtype=dt)
    bottom[..., 3] = 1
    G = []
    for j in range(R.shape[1]):
        p = int(parents[j])
        t = Jrest[:, j] - (Jrest[:, p] if p >= 0 else 0)
        M = torch.cat([torch.cat([R[:, j], t[..., None]], 2), bottom], 1)
        G.append(M if p < 0 else G[p] @ M)
    G = torch.stack(G, 1)
    Jposed = G[:, :, :3, 3]
    A = torch.cat([torch.cat([G[:, :, :3, :3], (G[:, :, :3, 3] - (G[:, :, :3, :3] @ Jrest[..., None])[..., 0])[..., None]], 3),
                   G[:, :, 3:]], 2)
    T = (m['lbs_weights'] @ A.reshape(B, -1, 16)).reshape(B, V, 4, 4)
    verts = (T[..., :3, :3] @ v_posed[..., None])[..., 0] + T[..., :3, 3]
    tri = m['faces'][m['lmk_faces_idx']]
    lmk = (verts[:, tri] * m['lmk_bary_coords'][None, :, :, None]).sum(2)
    joints = torch.cat([Jposed, verts[:, list(so.EXTRA_JOINT_VERTS)], lmk], 1)
    if 'transl' in x:
        tr = x['transl'].reshape(B, 1, 3)
        joints, verts = joints + tr, verts + tr
        A = torch.cat([torch.cat([A[:, :, :3, :3], (A[:, :, :3, 3] + tr)[..., None]], 3), A[:, :, 3:]], 2)
    nb = m['shapedirs'].shape[-1]
    only_betas = m['v_template'] + (m['shapedirs'].reshape(V * 3, nb) @ x['betas'].T).T.reshape(B, V, 3)
    return {'vertices': verts, 'joints': joints, 'A': A, 'v_shaped': only_betas}


def draw_inputs(B, seed, kind="random", with_transl=True):
    """The input grid of test_pose_grad_gpu.test_smplx_gradient_matches_float64_oracle."""
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    inp = {}
    for name, n in ARGS:
        if name == "transl" and not with_transl:
            continue
        scale = {"betas": 1.0, "expression": 1.0}.get(name, 0.3)
        v = torch.randn(B, n, generator=g) * scale
        if kind == "zero" and name not in ("betas", "expression", "transl"):
            v = torch.zeros(B, n)
        inp[name] = v
    if kind == "near_pi":
        ax = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
        inp["body_pose"][:, 3 * 4:3 * 5] = ax * (np.pi - 1e-2)      # one joint (left knee) rotated by ~pi
    return inp, g


def assert_equals_committed_oracle(m, B=3, seed=5):
    """The restatement is pinned to oracle/smplx_oracle.forward: identical values on the vertices, all 127 joints and A."""
    from oracle import smplx_oracle as so
    dt = m['v_template'].dtype
    inp, _ = draw_inputs(B, seed)
    x = {k: v.to(dt) for k, v in inp.items()}
    mine = forward(m, x)
    ref = so.forward(m, **x)
    for k in ('vertices', 'joints', 'A'):
        d = float((mine[k] - ref[k]).abs().max())
        assert mine[k].shape == ref[k].shape and d == 0.0, f"{k} ({dt}): restatement differs from smplx_oracle.forward by {d:.3e}"
    assert mine['joints'].shape[1] == 127
