"""Gradients of the avatar render with respect to the SMPL-X body pose (test-time pose refinement).

The three links the reference differentiates with plain torch -- AvatarNet.transform_cano2live (network/avatar.py:84-91),
AvatarNet.get_pose_map (:149-159) and the SMPL-X model -- against float64 autograd through the oracle/ restatements on the CPU.
Bar (that of the float64-oracle tests before it): a result passes when it is within 4 x the float32 oracle's own deviation from
float64 + 2e-6 of the float64 value's scale, in the max norm and in the L2 norm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bar(got, f64, f32, name):
    import torch
    got, f64, f32 = (t.detach().cpu().double() for t in (got, f64, f32))
    assert got.shape == f64.shape, f"{name}: shape {tuple(got.shape)} != {tuple(f64.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    e_max, e_l2 = float((got - f64).abs().max()), float((got - f64).norm())
    d_max, d_l2 = float((f32 - f64).abs().max()), float((f32 - f64).norm())
    lim_max = 4 * d_max + 2e-6 * float(f64.abs().max())
    lim_l2 = 4 * d_l2 + 2e-6 * float(f64.norm())
    assert e_max <= lim_max, f"{name}: max error {e_max:.3e} > {lim_max:.3e} (fp32 oracle {d_max:.3e})"
    assert e_l2 <= lim_l2, f"{name}: L2 error {e_l2:.3e} > {lim_l2:.3e} (fp32 oracle {d_l2:.3e})"


def _joints(J, seed, max_shift=0.05):
    import torch
    g = torch.Generator().manual_seed(seed)
    ax = torch.nn.functional.normalize(torch.randn(J, 3, generator=g))
    ang = torch.rand(J, generator=g) * (np.pi / 6)
    K = torch.zeros(J, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    A = torch.eye(4)[None].repeat(J, 1, 1)
    A[:, :3, :3] = torch.eye(3)[None] + torch.sin(ang)[:, None, None] * K + (1 - torch.cos(ang))[:, None, None] * (K @ K)
    A[:, :3, 3] = (torch.rand(J, 3, generator=g) - 0.5) * 2 * max_shift
    A[:, 3, :3] = torch.randn(J, 3, generator=g)      # row 3 is never read: its gradient must be exactly 0
    return A


def _lbs_case(N, J, K, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, J, generator=g)
    top = torch.topk(w, K, dim=1)
    lbs = torch.zeros(N, J).scatter_(1, top.indices, top.values + 0.05)
    lbs = lbs / lbs.sum(1, keepdim=True)
    pos = torch.randn(N, 3, generator=g) * 0.5
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g))
    ups = (torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g))
    return lbs, pos, rot, _joints(J, seed + 1), ups


def _oracle_lbs_vjp(lbs, pos, rot, A, up, ur, dtype):
    """float64 / float32 autograd through avatar_oracle.transform_cano2live: (dL/dA, dL/dpos, dL/drot)."""
    import torch
    from oracle import avatar_oracle as ao
    A_ = A.detach().to(dtype).clone().requires_grad_(True)
    p_ = pos.detach().to(dtype).clone().requires_grad_(True)
    r_ = rot.detach().to(dtype).clone().requires_grad_(True)
    lp, lr = ao.transform_cano2live(p_, r_, lbs.to(dtype), A_)
    outs, grads = [], []
    if up is not None:
        outs.append(lp), grads.append(up.to(dtype))
    if ur is not None:
        outs.append(lr), grads.append(ur.to(dtype))
    torch.autograd.backward(outs, grads)
    return A_.grad, p_.grad, r_.grad


def _gpu_lbs_vjp(lbs, pos, rot, A, up, ur, sparse):
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    A_ = A.detach().cuda().requires_grad_(True)
    p_ = pos.detach().cuda().requires_grad_(True)
    r_ = rot.detach().cuda().requires_grad_(True)
    lp, lr = ops.lbs_transform(p_, r_, lbs.cuda(), A_, sparse)
    outs, grads = [], []
    if up is not None:
        outs.append(lp), grads.append(up.cuda())
    if ur is not None:
        outs.append(lr), grads.append(ur.cuda())
    torch.autograd.backward(outs, grads)
    return A_.grad, p_.grad, r_.grad


# ---------------------------------------------------------------------------------------------------------------------------
# 1 + 2: the joint-matrix gradient of the LBS, its bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [55, 24])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 100003])
@pytest.mark.parametrize("K", [4, 12])
def test_lbs_joint_gradient_matches_float64_oracle(J, N, K):
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    lbs, pos, rot, A, (up, ur) = _lbs_case(N, J, K, seed=N * 7 + J + K)
    sp = ops.SparseLbs.build(lbs.cuda())
    assert sp is not None and sp.K == K
    for tag, u_p, u_r in (("positions", up, None), ("rotations", None, ur), ("both", up, ur)):
        want = _oracle_lbs_vjp(lbs, pos, rot, A, u_p, u_r, torch.float64)
        f32 = _oracle_lbs_vjp(lbs, pos, rot, A, u_p, u_r, torch.float32)
        dense = _gpu_lbs_vjp(lbs, pos, rot, A, u_p, u_r, None)
        sparse = _gpu_lbs_vjp(lbs, pos, rot, A, u_p, u_r, sp)
        assert torch.equal(dense[0][:, 3], torch.zeros_like(dense[0][:, 3])), f"{tag}: row 3 of dL/dA is not exactly 0"
        _bar(dense[0], want[0], f32[0], f"dL/dA ({tag}, dense, J={J} N={N})")
        for a, b, what in zip(dense, sparse, ("dL/dA", "dL/dpos", "dL/drot")):
            assert torch.equal(a, b), f"{what} ({tag}): sparse K={K} differs from dense by {float((a - b).abs().max()):.3e}"


def test_lbs_joint_gradient_all_matrix_to_quaternion_branches():
    """The four arg-max candidates of matrix_to_quaternion and the 0.1 floor (construction of test_avatar_gpu.py:101), with the
    joint matrices requiring grad."""
    import torch
    qs = torch.tensor([[1.0, 0.02, 0.01, 0.03], [0.02, 1.0, 0.03, 0.01], [0.01, 0.02, 1.0, 0.03], [0.03, 0.01, 0.02, 1.0]])
    qs = torch.nn.functional.normalize(qs).repeat(16, 1)
    N = qs.shape[0]
    lbs = torch.zeros(N, 3)
    lbs[:, 0] = 1.0
    lbs[N // 2:, 0] = 0.004
    A = torch.eye(4)[None].repeat(3, 1, 1)
    g = torch.Generator().manual_seed(11)
    pos = torch.randn(N, 3, generator=g)
    ur = torch.randn(N, 4, generator=g)
    want = _oracle_lbs_vjp(lbs, pos, qs, A, None, ur, torch.float64)
    f32 = _oracle_lbs_vjp(lbs, pos, qs, A, None, ur, torch.float32)
    got = _gpu_lbs_vjp(lbs, pos, qs, A, None, ur, None)
    _bar(got[0], want[0], f32[0], "dL/dA (m2q branches + floor)")
    assert float(want[0][0].abs().max()) > 0


@pytest.mark.parametrize("dense", [True, False])
def test_lbs_joint_gradient_at_full_size_and_bits(dense):
    """268 348 Gaussians (AvatarRenderCore.synthetic's count), J = 55, 4-sparse rows: the slab reduction at full size; two calls give
    the same bits; dL/dpos and dL/drot are bit-identical to the plain ag_lbs_backward's (asking for the joint gradient perturbs
    nothing)."""
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    N, J = 268348, 55
    lbs, pos, rot, A, (up, ur) = _lbs_case(N, J, 4, seed=5)
    sp = None if dense else ops.SparseLbs.build(lbs.cuda())
    want = _oracle_lbs_vjp(lbs, pos, rot, A, up, ur, torch.float64)
    f32 = _oracle_lbs_vjp(lbs, pos, rot, A, up, ur, torch.float32)
    a = _gpu_lbs_vjp(lbs, pos, rot, A, up, ur, sp)
    b = _gpu_lbs_vjp(lbs, pos, rot, A, up, ur, sp)
    _bar(a[0], want[0], f32[0], "dL/dA (N = 268348)")
    for x, y, what in zip(a, b, ("dL/dA", "dL/dpos", "dL/drot")):
        assert torch.equal(x, y), f"{what}: two calls differ"
    # the plain backward (joint matrices that do not require grad)
    p_, r_ = pos.cuda().requires_grad_(True), rot.cuda().requires_grad_(True)
    lp, lr = ops.lbs_transform(p_, r_, lbs.cuda(), A.cuda(), sp)
    torch.autograd.backward([lp, lr], [up.cuda(), ur.cuda()])
    assert torch.equal(p_.grad, a[1]) and torch.equal(r_.grad, a[2]), "the joint-gradient pass changed dL/dpos or dL/drot"
    _bar(a[1], want[1], f32[1], "dL/dpos")


# ---------------------------------------------------------------------------------------------------------------------------
# 3: SMPL-X
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smplx_pair():
    import torch
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.smplx import SMPLX
    from oracle import smplx_oracle as so
    arrays = synth.smplx_model_arrays()
    gpu = SMPLX(arrays, gender='neutral', use_pca=False, flat_hand_mean=True, device=torch.device("cuda", 0))
    return gpu, so.model_tensors(arrays, torch.float64), so.model_tensors(arrays, torch.float32)


def _smplx_chain_oracle(m, x):
    """A and joints[:, :55] of smplx_oracle.forward, restated for autograd: the oracle's rigid_chain fills its [B, J, 4, 4] chain in
    place while later joints read earlier rows, which autograd refuses to differentiate.  Same arithmetic (smplx/lbs.py:208-212,
    :347-405, body_models.py:1185-1275), the chain kept as a list."""
    import torch
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
    if 'transl' in x:
        tr = x['transl'].reshape(B, 1, 3)
        Jposed = Jposed + tr
        A = torch.cat([torch.cat([A[:, :, :3, :3], (A[:, :, :3, 3] + tr)[..., None]], 3), A[:, :, 3:]], 2)
    return {'A': A, 'joints': Jposed}


_ARGS = (("betas", 10), ("global_orient", 3), ("body_pose", 63), ("left_hand_pose", 45), ("right_hand_pose", 45), ("transl", 3),
         ("expression", 10), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["random", "zero", "near_pi"])
@pytest.mark.parametrize("with_transl", [True, False])
def test_smplx_gradient_matches_float64_oracle(smplx_pair, B, kind, with_transl):
    import torch
    from oracle import smplx_oracle as so
    gpu, m64, m32 = smplx_pair
    g = torch.Generator().manual_seed(B * 10 + len(kind) + with_transl)
    inp = {}
    for name, n in _ARGS:
        if name == "transl" and not with_transl:
            continue
        scale = {"betas": 1.0, "expression": 1.0, "transl": 0.3}.get(name, 0.3)
        x = torch.randn(B, n, generator=g) * scale
        if kind == "zero" and name not in ("betas", "expression", "transl"):
            x = torch.zeros(B, n)
        inp[name] = x
    if kind == "near_pi":
        ax = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
        inp["body_pose"][:, 3 * 4:3 * 5] = ax * (np.pi - 1e-2)      # one joint (left knee) rotated by ~pi
    J = 55
    wA = torch.randn(B, J, 4, 4, generator=g)
    wJ = torch.randn(B, J, 3, generator=g)

    def oracle(m, dt):
        x = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in inp.items()}
        out = _smplx_chain_oracle(m, x)
        L = (out["A"] * wA.to(dt)).sum() + (out["joints"][:, :J] * wJ.to(dt)).sum()
        L.backward()
        return {k: v.grad for k, v in x.items()}

    want, f32 = oracle(m64, torch.float64), oracle(m32, torch.float32)
    x = {k: v.cuda().requires_grad_(True) for k, v in inp.items()}
    out = gpu(**x)
    L = (out.A * wA.cuda()).sum() + (out.joints[:, :J] * wJ.cuda()).sum()
    L.backward()
    for k in inp:
        assert x[k].grad is not None, f"no gradient for {k}"
        _bar(x[k].grad, want[k], f32[k], f"dL/d{k} (B={B}, {kind}, transl={with_transl})")


def test_mat4_mul_inverse_gradient(smplx_pair):
    import torch
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    J = 55
    a = torch.stack([_joints(J, 21, 0.3), _joints(J, 22, 0.3)]).reshape(2 * J, 4, 4)
    a[:, 3] = torch.tensor([0., 0., 0., 1.])
    b = _joints(J, 23, 0.3)
    b[:, 3] = torch.tensor([0., 0., 0., 1.])
    b[:, :3, :3] *= 1.3
    w = torch.randn(2 * J, 4, 4, generator=torch.Generator().manual_seed(24))

    def oracle(dt):
        a_, b_ = a.detach().to(dt).clone().requires_grad_(True), b.detach().to(dt).clone().requires_grad_(True)
        out = a_.view(2, J, 4, 4) @ torch.linalg.inv(b_)[None]
        (out.reshape(2 * J, 4, 4) * w.to(dt)).sum().backward()
        return a_.grad, b_.grad

    want, f32 = oracle(torch.float64), oracle(torch.float32)
    a_, b_ = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    (mat4_mul_inverse(a_, b_) * w.cuda()).sum().backward()
    _bar(a_.grad, want[0], f32[0], "dL/da")
    _bar(b_.grad, want[1], f32[1], "dL/db")


def test_smplx_vertex_and_keypoint_gradients_raise(smplx_pair):
    import torch
    gpu = smplx_pair[0]
    bp = (torch.randn(1, 63) * 0.2).cuda().requires_grad_(True)
    out = gpu(body_pose=bp)
    with pytest.raises(NotImplementedError, match="vertices"):
        out.vertices.sum().backward()
    out = gpu(body_pose=bp)
    with pytest.raises(NotImplementedError, match="key points"):
        out.joints[:, 55:].sum().backward()
    out = gpu(body_pose=bp)                       # a slice of the chain joints alone: no error, gradient reaches the pose
    out.joints[:, :55].sum().backward()
    assert bp.grad is not None and torch.isfinite(bp.grad).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the avatar render
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def avatar():
    import torch
    from animatablegaussians_amd.avatar import AvatarNet
    torch.manual_seed(31359)
    net = AvatarNet.synthetic({'with_viewdirs': True})
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _items(seed=3, S=1024):
    import torch
    from animatablegaussians_amd import camera
    A = _joints(55, seed, 0.01)
    A[:, 3] = torch.tensor([0., 0., 0., 1.])
    extr = torch.from_numpy(camera.calc_front_mv(np.zeros(3, np.float32), tar_pos=(0.0, 0.0, 2.5)))
    intr = torch.tensor([[1100.0, 0, S / 2], [0, 1100.0, S / 2], [0, 0, 1]])
    return {'cano2live_jnt_mats': A.cuda(), 'cano2live_jnt_mats_woRoot': _joints(55, seed + 1, 0.01).cuda(), 'extr': extr.cuda(),
            'intr': intr.cuda(), 'img_w': S, 'img_h': S}


def test_render_pose_gradient_composes_the_oracle_vjps(avatar, monkeypatch):
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    from oracle import avatar_oracle as ao
    net = avatar
    items = _items()
    A = items['cano2live_jnt_mats'].clone().requires_grad_(True)
    Aw = items['cano2live_jnt_mats_woRoot'].clone().requires_grad_(True)
    it = dict(items, cano2live_jnt_mats=A, cano2live_jnt_mats_woRoot=Aw)
    calls = []
    real = ops.lbs_transform

    def recording(positions, rotations, lbs, jnt_mats, sparse=None):
        out = real(positions, rotations, lbs, jnt_mats, sparse)
        calls.append((positions.detach().clone(), rotations.detach().clone(), jnt_mats, out))
        return out

    monkeypatch.setattr(ops, "lbs_transform", recording)
    pose_map = net.get_pose_map(it)
    pm_grad = []
    pose_map.register_hook(lambda g: pm_grad.append(g.detach().clone()))
    ret = net.render(it)
    monkeypatch.setattr(ops, "lbs_transform", real)
    lbs_call = [c for c in calls if c[2] is A and c[3][0].requires_grad]     # (the view-direction blend runs under no_grad)
    assert len(lbs_call) == 1
    outs = lbs_call[0][3]
    out_grads = [None, None]
    outs[0].register_hook(lambda g: out_grads.__setitem__(0, g.detach().clone()))
    outs[1].register_hook(lambda g: out_grads.__setitem__(1, g.detach().clone()))
    target = torch.rand_like(ret['rgb_map'])
    (ret['rgb_map'] - target).abs().mean().backward()
    assert A.grad is not None and Aw.grad is not None and out_grads[0] is not None and pm_grad
    lbs = net.core.lbs.cpu()
    pos, rot = lbs_call[0][0].cpu(), lbs_call[0][1].cpu()
    gp, gr = out_grads[0].cpu(), out_grads[1].cpu()
    want = _oracle_lbs_vjp(lbs, pos, rot, A.detach().cpu(), gp, gr, torch.float64)
    f32 = _oracle_lbs_vjp(lbs, pos, rot, A.detach().cpu(), gp, gr, torch.float32)
    _bar(A.grad, want[0], f32[0], "dL/d cano2live_jnt_mats")
    # the pose map: get_pose_map's float64 VJP of the captured gradient
    H, W = net.map_shape
    mask = net.cano_smpl_mask.cpu()
    cano = torch.zeros(H, W, 3)
    cano[mask] = net.core.xyz.cpu()

    def pm_oracle(dt):
        a = Aw.detach().cpu().to(dt).requires_grad_(True)
        out = ao.get_pose_map(cano.to(dt), mask, lbs.to(dt), a)
        out.backward(pm_grad[0].cpu().to(dt).reshape(out.shape))
        return a.grad

    _bar(Aw.grad, pm_oracle(torch.float64), pm_oracle(torch.float32), "dL/d cano2live_jnt_mats_woRoot")
    assert net.core.xyz.grad is None


def test_render_views_pose_gradient_is_the_sum_of_two_renders(avatar):
    import torch
    from animatablegaussians_amd import synth
    net = avatar
    items = _items(seed=5)
    cams = synth.free_view_cameras(8, img=1024)
    views = [{'extr': torch.from_numpy(np.ascontiguousarray(cams[i]["extr"])).float().cuda(),
              'intr': torch.from_numpy(np.ascontiguousarray(cams[i]["intr"])).float().cuda(), 'img_w': 1024, 'img_h': 1024} for i in (0, 3)]
    with torch.no_grad():
        net.get_pose_map(items)
    g = torch.Generator().manual_seed(9)
    targets = [torch.rand(1024, 1024, 3, generator=g).cuda() for _ in views]
    A = items['cano2live_jnt_mats'].clone().requires_grad_(True)
    rets = net.render_views(dict(items, cano2live_jnt_mats=A), views)
    sum(((r['rgb_map'] - t).abs().mean() for r, t in zip(rets, targets))).backward()
    got = A.grad.clone()
    sums = []
    for dt in (torch.float64, torch.float32):
        acc = torch.zeros(55, 4, 4, dtype=dt)
        for v, t in zip(views, targets):
            A1 = items['cano2live_jnt_mats'].clone().requires_grad_(True)
            r = net.render(dict(items, cano2live_jnt_mats=A1, **v))
            (r['rgb_map'] - t).abs().mean().backward()
            acc += A1.grad.cpu().to(dt)
        sums.append(acc)
    # the per-view gradients in float64 are the truth; their float32 sum is the yardstick
    _bar(got, sums[0], sums[1].float(), "render_views dL/dA vs the sum of two renders")


def test_render_bits_unchanged_without_pose_grad(avatar):
    import torch
    net = avatar
    items = _items(seed=7)
    with torch.no_grad():
        net.get_pose_map(items)
        a = net.render(items)['rgb_map'].clone()
    b = net.render(items)['rgb_map'].detach().clone()                    # grad enabled, nothing requires grad
    A = items['cano2live_jnt_mats'].clone().requires_grad_(True)
    c = net.render(dict(items, cano2live_jnt_mats=A))['rgb_map'].detach().clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    with torch.no_grad():
        pm0 = net.get_pose_map(dict(items)).clone()
    pm1 = net.get_pose_map(dict(items, cano2live_jnt_mats_woRoot=items['cano2live_jnt_mats_woRoot'].clone().requires_grad_(True)))
    assert torch.equal(pm0, pm1.detach())


# ---------------------------------------------------------------------------------------------------------------------------
# 5: pose recovery, end to end
# ---------------------------------------------------------------------------------------------------------------------------
# measured on MI355X: after 30 Adam steps (lr 0.002) the L1 image loss is at 0.395 of its start (4.02e-2 -> 1.59e-2); the bound allows
# twice that ratio
RECOVERY_MEASURED = 0.395
RECOVERY_BOUND = 0.8


def _pose_items(smplx, body_pose, cano):
    import torch
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    B = body_pose.shape[0]
    live = smplx(body_pose=body_pose, global_orient=torch.tensor([[0.05, 0.0, 0.0]], device='cuda').expand(B, 3),
                 transl=torch.tensor([[0.0, 0.01, 0.0]], device='cuda').expand(B, 3))
    woroot = smplx(body_pose=body_pose)
    c2l = mat4_mul_inverse(torch.stack([live.A[0], woroot.A[0]]), cano)
    return c2l[0], c2l[1]


def pose_refinement_run(net, smplx, steps=30, lr=0.002, seed=0):
    """Target = the render at theta*; start from theta* + 0.05 rad on six body joints; Adam on body_pose alone with an L1 image loss.
    Returns the per-step losses."""
    import torch
    g = torch.Generator().manual_seed(seed)
    theta = (torch.randn(1, 63, generator=g) * 0.1).cuda()
    with torch.no_grad():
        cano = smplx(body_pose=torch.zeros(1, 63, device='cuda')).A[0]
    base = _items(seed=11)
    with torch.no_grad():
        A, Aw = _pose_items(smplx, theta, cano)
        it = dict(base, cano2live_jnt_mats=A, cano2live_jnt_mats_woRoot=Aw)
        net.get_pose_map(it)
        target = net.render(it)['rgb_map'].clone()
    start = theta.clone()
    for j in (0, 3, 4, 15, 16, 17):                 # hips, knees, shoulders (body joint indices 1..21 -> rows 0..20)
        start[0, 3 * j:3 * j + 3] += 0.05
    bp = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([bp], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        A, Aw = _pose_items(smplx, bp, cano)
        it = dict(base, cano2live_jnt_mats=A, cano2live_jnt_mats_woRoot=Aw)
        net.get_pose_map(it)
        loss = (net.render(it)['rgb_map'] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


def test_pose_recovery_end_to_end(avatar, smplx_pair):
    losses = pose_refinement_run(avatar, smplx_pair[0])
    print(f"pose recovery: loss {losses[0]:.4e} -> {losses[-1]:.4e} (ratio {losses[-1] / losses[0]:.3f})")
    assert all(np.isfinite(losses))
    assert losses[-1] < RECOVERY_BOUND * losses[0], f"loss fell only from {losses[0]:.4e} to {losses[-1]:.4e}"
