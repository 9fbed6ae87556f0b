"""Gradients of the SMPL-X vertices, vertex key points and v_shaped (``SMPLX(vertex_grad=True)``) against float64 autograd through
tests/smplx_vertex_oracle.py, the autograd-friendly restatement of oracle/smplx_oracle.forward (asserted equal to it first).

Bar (that of test_pose_grad_gpu.py, copied): a result passes when it is within 4 x the float32 oracle's own deviation from float64 +
2e-6 of the float64 value's scale, in the max norm and in the L2 norm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIT_ARGS = ("betas", "expression", "global_orient", "body_pose", "jaw_pose", "left_hand_pose", "right_hand_pose", "transl")
FIT_REL = 1e-3          # GPU fit loss within 1e-3 relative of the float64 oracle's: 10 x the float32 oracle's own agreement (< 1e-4)


def _bar(got, f64, f32, name):
    import torch
    got, f64, f32 = (t.detach().cpu().double() for t in (got, f64, f32))
    assert got.shape == f64.shape, f"{name}: shape {tuple(got.shape)} != {tuple(f64.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    e_max, e_l2 = float((got - f64).abs().max()), float((got - f64).norm())
    d_max, d_l2 = float((f32 - f64).abs().max()), float((f32 - f64).norm())
    lim_max = 4 * d_max + 2e-6 * float(f64.abs().max())
    lim_l2 = 4 * d_l2 + 2e-6 * float(f64.norm())
    print(f"{name}: max error {e_max:.3e} (limit {lim_max:.3e}, fp32 oracle {d_max:.3e}), L2 error {e_l2:.3e} (limit {lim_l2:.3e})")
    assert e_max <= lim_max, f"{name}: max error {e_max:.3e} > {lim_max:.3e} (fp32 oracle {d_max:.3e})"
    assert e_l2 <= lim_l2, f"{name}: L2 error {e_l2:.3e} > {lim_l2:.3e} (fp32 oracle {d_l2:.3e})"


def _build(arrays, vertex_grad):
    import torch
    from animatablegaussians_amd.smplx import SMPLX
    kw = {"vertex_grad": True} if vertex_grad else {}
    return SMPLX(arrays, gender='neutral', use_pca=False, flat_hand_mean=True, device=torch.device("cuda", 0), **kw)


@pytest.fixture(scope="module")
def models():
    import torch
    import smplx_vertex_oracle as vo
    from animatablegaussians_amd import synth
    from oracle import smplx_oracle as so
    arrays = synth.smplx_model_arrays()
    m64, m32 = so.model_tensors(arrays, torch.float64), so.model_tensors(arrays, torch.float32)
    vo.assert_equals_committed_oracle(m64)
    vo.assert_equals_committed_oracle(m32)
    return _build(arrays, True), _build(arrays, False), m64, m32


LOSSES = ("all", "vertices", "keypoints", "v_shaped")


def _loss(out, w, which, J=55):
    get = (lambda k: out[k]) if isinstance(out, dict) else (lambda k: getattr(out, k))
    to = lambda t: t.to(get('A').dtype).to(get('A').device)  # noqa: E731
    if which == "all":
        return (get('vertices') * to(w['V'])).sum() + (get('joints') * to(w['J'])).sum() + (get('A') * to(w['A'])).sum()
    if which == "vertices":
        return (get('vertices') * to(w['V'])).sum()
    if which == "keypoints":
        return (get('joints')[:, J:] * to(w['J'])[:, J:]).sum()
    return (get('v_shaped') * to(w['S'])).sum()


def _oracle_grads(m, inp, w, which):
    import torch
    import smplx_vertex_oracle as vo
    dt = m['v_template'].dtype
    x = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in inp.items()}
    _loss(vo.forward(m, x), w, which).backward()
    return {k: v.grad for k, v in x.items()}


def _gpu_grads(gpu, inp, w, which):
    x = {k: v.cuda().requires_grad_(True) for k, v in inp.items()}
    out = gpu(return_shaped=True, **x)
    _loss(out, w, which).backward()
    return {k: v.grad for k, v in x.items()}, out


def _weights(B, g, V=10475):
    import torch
    return {'V': torch.randn(B, V, 3, generator=g), 'J': torch.randn(B, 127, 3, generator=g), 'A': torch.randn(B, 55, 4, 4, generator=g),
            'S': torch.randn(B, V, 3, generator=g)}


def _compare(gpu, m64, m32, inp, w, which, tag):
    import torch
    want, f32 = _oracle_grads(m64, inp, w, which), _oracle_grads(m32, inp, w, which)
    got, _ = _gpu_grads(gpu, inp, w, which)
    for k in inp:
        if want[k] is None:             # the output does not depend on this input (v_shaped: the betas alone)
            assert got[k] is None or not bool(got[k].ne(0).any()), f"dL/d{k} ({which}, {tag}): the oracle has no gradient here"
            continue
        assert got[k] is not None, f"no gradient for {k} ({which}, {tag})"
        _bar(got[k], want[k], f32[k], f"dL/d{k} ({which}, {tag})")
    if which == "all":
        assert all(want[k] is not None for k in inp)


# ---------------------------------------------------------------------------------------------------------------------------
# 1: gradients against float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["random", "zero", "near_pi"])
@pytest.mark.parametrize("with_transl", [True, False])
def test_vertex_gradients_match_float64_oracle(models, B, kind, with_transl):
    import smplx_vertex_oracle as vo
    gpu, _, m64, m32 = models
    inp, g = vo.draw_inputs(B, B * 10 + len(kind) + with_transl, kind, with_transl)
    w = _weights(B, g)
    for which in LOSSES:
        _compare(gpu, m64, m32, inp, w, which, f"B={B}, {kind}, transl={with_transl}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the flag changes neither the forward nor the chain gradients
# ---------------------------------------------------------------------------------------------------------------------------
def test_flag_off_changes_nothing(models):
    import torch
    import smplx_vertex_oracle as vo
    on, off, _, _ = models
    assert on.vertex_grad and not off.vertex_grad
    inp, g = vo.draw_inputs(3, 77)
    wA, wJ = torch.randn(3, 55, 4, 4, generator=g).cuda(), torch.randn(3, 55, 3, generator=g).cuda()
    res = []
    for model in (on, off):
        x = {k: v.cuda().requires_grad_(True) for k, v in inp.items()}
        out = model(return_shaped=True, **x)
        ((out.A * wA).sum() + (out.joints[:, :55] * wJ).sum()).backward()
        res.append((out, {k: v.grad for k, v in x.items()}))
    for k in ("vertices", "joints", "A", "v_shaped"):
        assert torch.equal(res[0][0][k], res[1][0][k]), f"{k}: forward bits depend on vertex_grad"
    for k in inp:
        assert res[0][1][k] is not None and torch.equal(res[0][1][k], res[1][1][k]), f"dL/d{k}: chain-gradient bits depend on vertex_grad"
    assert res[0][0].v_shaped.requires_grad and not res[1][0].v_shaped.requires_grad
    with pytest.raises(NotImplementedError, match="vertices"):          # the default model still refuses
        off(body_pose=inp["body_pose"].cuda().requires_grad_(True)).vertices.sum().backward()


# ---------------------------------------------------------------------------------------------------------------------------
# 3: determinism
# ---------------------------------------------------------------------------------------------------------------------------
def test_gradient_bits_repeat(models):
    import torch
    import smplx_vertex_oracle as vo
    gpu = models[0]
    inp, g = vo.draw_inputs(3, 91)
    w = _weights(3, g)
    a, _ = _gpu_grads(gpu, inp, w, "all")
    b, _ = _gpu_grads(gpu, inp, w, "all")
    for k in inp:
        assert torch.equal(a[k], b[k]), f"dL/d{k}: two calls differ by {float((a[k] - b[k]).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# 4: key points whose vertices repeat
# ---------------------------------------------------------------------------------------------------------------------------
def test_repeated_keypoint_vertices():
    """Landmark triangles that share vertices with each other and with the 21 vertex picks: a scatter that overwrites or races
    duplicates loses part of the gradient."""
    import torch
    import smplx_vertex_oracle as vo
    from animatablegaussians_amd import synth
    from oracle import smplx_oracle as so
    arrays = dict(synth.smplx_model_arrays())
    f = np.array(arrays['f'], copy=True)
    picks = so.EXTRA_JOINT_VERTS
    for i, face in enumerate(np.asarray(arrays['lmk_faces_idx'])):
        f[face] = (picks[i % 21], picks[(i + 5) % 21], 100 + i // 8)      # every landmark corner is shared several times
    arrays['f'] = f
    tri = f[np.asarray(arrays['lmk_faces_idx'])].reshape(-1)
    assert len(np.unique(tri)) < len(tri) // 3 and set(tri[::3]) <= set(picks)
    gpu = _build(arrays, True)
    m64, m32 = so.model_tensors(arrays, torch.float64), so.model_tensors(arrays, torch.float32)
    for B in (1, 3):
        inp, g = vo.draw_inputs(B, 40 + B)
        _compare(gpu, m64, m32, inp, _weights(B, g), "keypoints", f"shared landmark vertices, B={B}")


# ---------------------------------------------------------------------------------------------------------------------------
# 5: fitting
# ---------------------------------------------------------------------------------------------------------------------------
def _fit(forward, make, target, on, steps=40):
    """Adam (lr 0.02) from all-zero parameters towards `target`, loss = mean squared distance over joints[:, 55:] ('keypoints') or the
    vertices; returns the losses at steps 0 .. steps."""
    import torch
    import smplx_vertex_oracle as vo
    x = {k: make(torch.zeros(1, dict(vo.ARGS)[k])).requires_grad_(True) for k in FIT_ARGS}
    opt = torch.optim.Adam(list(x.values()), lr=0.02)
    pick = (lambda o: o['joints'][:, 55:]) if on == "keypoints" else (lambda o: o['vertices'])
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = (pick(forward(x)) - target).square().sum(-1).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("on", ["keypoints", "vertices"])
def test_fit_follows_the_float64_oracle(models, on):
    import torch
    import smplx_vertex_oracle as vo
    gpu, _, m64, _ = models
    g = torch.Generator().manual_seed(31359)
    sigma = {"betas": 1.0, "expression": 1.0}
    truth = {k: torch.randn(1, dict(vo.ARGS)[k], generator=g) * sigma.get(k, 0.3) for k in FIT_ARGS}
    pick = (lambda o: o['joints'][:, 55:]) if on == "keypoints" else (lambda o: o['vertices'])
    with torch.no_grad():
        target = pick(vo.forward(m64, {k: v.double() for k, v in truth.items()}))
    want = _fit(lambda x: vo.forward(m64, x), lambda t: t.double(), target, on)
    got = _fit(lambda x: gpu(**x), lambda t: t.cuda(), target.float().cuda(), on)
    print(f"fit on the {on}: float64 oracle {want[0]:.4e} -> {want[20]:.4e} -> {want[40]:.4e} (ratio {want[40] / want[0]:.4f}); "
          f"GPU {got[0]:.4e} -> {got[20]:.4e} -> {got[40]:.4e}")
    assert want[40] < 0.05 * want[0], "the oracle fit itself does not converge"
    for step in (20, 40):
        rel = abs(got[step] - want[step]) / want[step]
        assert rel <= FIT_REL, f"fit on the {on}, step {step}: GPU loss {got[step]:.6e} vs float64 oracle {want[step]:.6e} (relative {rel:.2e})"


# ---------------------------------------------------------------------------------------------------------------------------
# 6: end to end with the render
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


def test_pose_refinement_with_a_keypoint_term(models, avatar):
    """One iteration of bench_avatar.py's pose-refinement path (SMPL-X live and without root -> mat4_mul_inverse -> pose map -> render
    -> L1) with a key-point term on the live model's joints[:, 55:], one shared body_pose leaf.  With the image term's weight at 0 the
    render branch contributes exact zeros, so the gradient must be the oracle's key-point-only gradient."""
    import torch
    import smplx_vertex_oracle as vo
    from animatablegaussians_amd import camera
    from animatablegaussians_amd.smplx import mat4_mul_inverse
    smplx, _, m64, m32 = models
    net, S = avatar, 1024
    extr = torch.from_numpy(camera.calc_front_mv(np.zeros(3, np.float32), tar_pos=(0.0, 0.0, 2.5))).cuda()
    intr = torch.tensor([[1100.0, 0, S / 2], [0, 1100.0, S / 2], [0, 0, 1]]).cuda()
    go, tr = torch.tensor([[0.05, 0.0, 0.0]]), torch.tensor([[0.0, 0.01, 0.0]])
    g = torch.Generator().manual_seed(0)
    theta = torch.randn(1, 63, generator=g) * 0.1
    kp_target = torch.randn(1, 72, 3, generator=g) * 0.3
    with torch.no_grad():
        cano = smplx(body_pose=torch.zeros(1, 63, device='cuda')).A[0]

    def run(bp, w_img, target):
        live, woroot = smplx(body_pose=bp, global_orient=go.cuda(), transl=tr.cuda()), smplx(body_pose=bp)
        c2l = mat4_mul_inverse(torch.stack([live.A[0], woroot.A[0]]), cano)
        it = {'cano2live_jnt_mats': c2l[0], 'cano2live_jnt_mats_woRoot': c2l[1], 'extr': extr, 'intr': intr, 'img_w': S, 'img_h': S}
        net.get_pose_map(it)
        rgb = net.render(it)['rgb_map']
        img = (rgb - (rgb.detach() * 0.5 if target is None else target)).abs().mean()
        return w_img * img + (live.joints[:, 55:] - kp_target.cuda()).square().sum(-1).mean()

    bp = (theta + 0.05).cuda().requires_grad_(True)
    run(bp, 1.0, None).backward()
    assert bp.grad is not None and torch.isfinite(bp.grad).all() and float(bp.grad.abs().max()) > 0
    bp0 = (theta + 0.05).cuda().requires_grad_(True)
    run(bp0, 0.0, None).backward()

    def oracle(m):
        dt = m['v_template'].dtype
        x = {'betas': torch.zeros(1, 10, dtype=dt), 'global_orient': go.to(dt), 'transl': tr.to(dt),
             'body_pose': (theta + 0.05).to(dt).requires_grad_(True)}
        (vo.forward(m, x)['joints'][:, 55:] - kp_target.to(dt)).square().sum(-1).mean().backward()
        return x['body_pose'].grad

    _bar(bp0.grad, oracle(m64), oracle(m32), "dL/dbody_pose (key-point term, image weight 0)")
