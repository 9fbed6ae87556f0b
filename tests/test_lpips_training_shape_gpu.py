"""LPIPS-VGG16 and the training loss tail at the 512^2 training crop against the float64 CPU oracle, layer by layer and end to end.

main_avatar.py:117-124,227-238 runs the perceptual term on a 512^2 crop of a render and a ground truth that is nearly equal to it, with a
constant-background border that gives both branches identical inputs.  test_lpips.py pins the module to the reference class's 64^2 golden;
here the yardstick is oracle/lpips_oracle.py (pinned to that golden by test_lpips.py) run live on the CPU, in float64 for the values and in
float32 for the tolerance: per tensor, max|ours - o64| / max|o64| <= K x (the same for the fp32 oracle) + FLOOR.

  A. every trunk unit (agc.conv2d + noise_bias_act with slope 0) at its 512^2-crop shape, from the same float32 input as the oracle;
  B. maxpool2x2 at every pool shape of the crop and one odd size: bit-identical to F.max_pool2d (the grid-stride loops iterate here);
  C. _LpipsLevel at every tap shape and at HW > 524 288 (the level kernels' loop iterates): nearly equal, independent, zero feature vectors;
  D. LPIPS.forward(retPerLayer=True, normalize=True) at 512^2 and at an odd 200 x 148: total, the five levels, the prediction's gradient;
  E. losses.training_loss at a 1024^2 render against a float64 restatement of main_avatar.py:196-245.

Weights come from lpips.lpips_named_fill, as in the golden."""
import numpy as np
import pytest
from helpers import cpu_threads

pytestmark = pytest.mark.gpu

MODES = ["split_f16", "split_bf16", "fp32"]
K, FLOOR = 4.0, 2e-6               # the bar of every comparison against the oracle
S = 512                            # the training crop (main_avatar.py patch_size)
BORDER = 100                       # constant-background columns on each side of the crop (a bounding box taller than wide)
BG = (1.0, 1.0, 1.0)
# The image gradient through all thirteen convolutions and four pools (module "grad in0", loss "grad rgb_map") cannot be masked the way one
# unit's can: in every math mode the product routes 2-5 windows of pools 3 and 4 differently from float64 where float64's own margin is
# 2e-8 - 6e-7 of the largest activation, and flips 1-2 ReLUs per layer within 4e-7 of it (measured on the nearly-equal 512^2 crop).  Each
# moves a blob of the gradient: max-norm deviation 1.37e-2 (split_f16, fp32) and 1.94e-2 (split_bf16) against the fp32 oracle's 1.50e-3, L2
# 1.46e-3 - 1.99e-3 against 4.41e-4.  Those two tensors get 16x (max) and 8x (L2) the fp32 oracle's deviation; everything else gets K.
CHAIN = {"max": 16.0, "l2": 8.0}
RELU_MASK = 1e-4                   # no upstream gradient where the float64 pre-activation is within this fraction of its maximum from zero


def _torch():
    import torch
    return torch


class _Math:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from animatablegaussians_amd import conv as agc
        self.prev = agc.set_math(self.mode)

    def __exit__(self, *exc):
        from animatablegaussians_amd import conv as agc
        agc.set_math(self.prev)


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads():
    torch = _torch()
    prev = torch.get_num_threads()
    torch.set_num_threads(cpu_threads())
    yield
    torch.set_num_threads(prev)


def _rel(got, ref):
    """max|got - ref| / max|ref| in float64 (``ref`` a CPU float64 tensor)."""
    got = got.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _rel2(got, ref):
    """|got - ref|_2 / |ref|_2: where isolated ReLU / max-pool selection flips set the maximum, the whole tensor is still held to the bar."""
    got = got.detach().double().cpu()
    return float((got - ref).norm()) / max(float(ref.norm()), 1e-300)


def _check(tag, got, o64, o32, fails, chain=()):
    """Per tensor: ours within K x the fp32 oracle's deviation from the float64 oracle, + FLOOR, in the maximum norm and (tensors) in the L2
    norm.  A scalar is one sample of the fp32 oracle's error, which can cancel by luck (8e-9 on one level where its neighbours show 3e-7), so the
    scalars of one call share the largest fp32 deviation among them.  ``chain``: keys held to the CHAIN bars instead.  Prints the measured
    values and appends the misses to ``fails`` (the test asserts it empty at its end, after every check is printed).  Returns the worst ratio."""
    worst = 0.0
    d32_scalar = max((_rel(o32[k], o64[k]) for k in o64 if o64[k].numel() == 1), default=0.0)
    for k in o64:
        assert got.get(k) is not None, (tag, k)
        for norm, rel in (("max", _rel), ("l2", _rel2)) if o64[k].numel() > 1 else (("max", _rel),):
            d, d32 = rel(got[k], o64[k]), rel(o32[k], o64[k]) if o64[k].numel() > 1 else d32_scalar
            lim = (CHAIN[norm] if k in chain else K) * d32 + FLOOR
            worst = max(worst, d / lim)
            print(f"[lpips] {tag} {k} ({norm}): ours {d:.2e} oracle-fp32 {d32:.2e} ours/bar {d / lim:.2f}")
            if not (np.isfinite(d) and d <= lim):
                fails.append((tag, k, norm, d, d32))
    return worst


def _sd(dt=None):
    """The fill of the golden, {reference state_dict key: CPU tensor} (``dt``: cast for the oracle)."""
    from animatablegaussians_amd.lpips import LPIPS, lpips_named_fill
    sd = lpips_named_fill({k: v for k, v in LPIPS().reference_state_dict().items() if not k.startswith("scaling_layer")})
    return sd if dt is None else {k: v.to(dt) for k, v in sd.items()}


def _module():
    from animatablegaussians_amd.lpips import LPIPS
    m = LPIPS(net='vgg')
    m.load_reference_state_dict({**_sd(), "scaling_layer.shift": m.scaling_layer__shift, "scaling_layer.scale": m.scaling_layer__scale})
    return m.cuda()


def _smooth(g, c, h, w, cells):
    """A band-limited random field in [0, 1]: uniform noise on a cells x cells lattice, bicubically upsampled."""
    torch = _torch()
    import torch.nn.functional as F
    z = torch.rand(1, c, cells, cells, generator=g)
    return F.interpolate(z, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1)


def _texture(g, h, w):
    torch = _torch()
    return (0.55 * _smooth(g, 3, h, w, 6) + 0.3 * _smooth(g, 3, h, w, 48) + 0.15 * torch.rand(3, h, w, generator=g)).clamp(0, 1)


def _crop_pair(seed, h=S, w=S, border=BORDER):
    """(prediction, ground truth) [1, 3, h, w] as the loss sees them: a textured subject between two constant background bands; the prediction
    is the ground truth plus a smooth residual of amplitude 1e-2 on the subject, the bands identical."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    gt = _texture(g, h, w)
    gt[:, :, :border] = gt[:, :, w - border:] = torch.tensor(BG)[:, None, None]
    pred = gt.clone()
    pred[:, :, border:w - border] += 1e-2 * (2 * _smooth(g, 3, h, w - 2 * border, 12) - 1)
    return pred[None].contiguous(), gt[None].contiguous()


def _indep_pair(seed, h=S, w=S):
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    return _texture(g, h, w)[None].contiguous(), _texture(g, h, w)[None].contiguous()


def _oracle_lpips(in0, in1, sd, dt):
    """oracle LPIPS(normalize=True) in ``dt``: total, the five levels, d total / d in0, and the per-pixel distance maps [HW] of the levels."""
    torch = _torch()
    import torch.nn.functional as F
    from oracle import lpips_oracle as lo
    a = in0.detach().to(dt).requires_grad_(True)
    b = in1.detach().to(dt)
    o0 = lo.vgg_taps((2 * a - 1 - lo.SHIFT) / lo.SCALE, sd)
    with torch.no_grad():
        o1 = lo.vgg_taps((2 * b - 1 - lo.SHIFT) / lo.SCALE, sd)
    # lpips_oracle.lpips(normalize=True) with the per-pixel maps kept
    maps = [F.conv2d((lo.normalize_tensor(o0[k]) - lo.normalize_tensor(o1[k])) ** 2, sd[f"lin{k}.model.1.weight"]) for k in range(5)]
    res = [mp.mean() for mp in maps]
    val = res[0]
    for r in res[1:]:
        val = val + r
    val.backward()
    return {"total": val.detach().double(), **{f"level{k}": res[k].detach().double() for k in range(5)}, "grad in0": a.grad.double()}, \
        [mp.detach().double().reshape(-1) for mp in maps]


# ---------------------------------------------------------------------------------------------------------------------------------
# A.  every trunk unit at its 512^2-crop shape
# ---------------------------------------------------------------------------------------------------------------------------------
def _trunk_units():
    """(slice, torchvision index, Cin, Cout, pooled before) of the thirteen convolutions, in order."""
    from animatablegaussians_amd.lpips import _SLICES
    return [(si + 1, idx, cin, cout, si > 0 and j == 0) for si, convs in enumerate(_SLICES) for j, (idx, cin, cout) in enumerate(convs)]


@pytest.fixture(scope="module")
def trunk_cases():
    """The prediction branch's input of every trunk unit (the float32 oracle's activations of the nearly-equal 512^2 crop), a random upstream
    gradient masked where the float64 pre-activation is within RELU_MASK of its maximum from zero, and the unit in float64 / float32."""
    torch = _torch()
    import torch.nn.functional as F
    from oracle import lpips_oracle as lo
    sd32, sd64 = _sd(torch.float32), _sd(torch.float64)
    pred, _ = _crop_pair(11)
    g = torch.Generator().manual_seed(12)
    h = ((2 * pred - 1 - lo.SHIFT) / lo.SCALE).contiguous()
    cases = []
    for si, idx, cin, cout, pooled in _trunk_units():
        if pooled:
            h = F.max_pool2d(h, 2, 2)
        x = h.contiguous()
        wk, bk = f"net.slice{si}.{idx}.weight", f"net.slice{si}.{idx}.bias"
        o = {}
        for dt, sd in ((torch.float64, sd64), (torch.float32, sd32)):
            xs = x.detach().to(dt, copy=True).requires_grad_(True)
            pre = F.conv2d(xs, sd[wk], sd[bk], padding=1)
            y = F.relu(pre)
            if dt == torch.float64:
                keep = pre.detach().abs() > RELU_MASK * float(pre.detach().abs().max())
                up = torch.randn(y.shape, generator=g) * keep
            (y * up.to(dt)).sum().backward()
            o[dt] = {"out": y.detach().double(), "grad x": xs.grad.double()}
            if dt == torch.float32:
                h = y.detach()
        cases.append(dict(name=f"slice{si}.{idx} {cin}->{cout}@{x.shape[2]}x{x.shape[3]}", x=x, w=sd32[wk], b=sd32[bk], up=up,
                          masked=1.0 - float(keep.double().mean()), o64=o[torch.float64], o32=o[torch.float32]))
    return cases


@pytest.mark.parametrize("mode", MODES)
def test_trunk_units_at_crop_shape_vs_oracle(mode, trunk_cases, monkeypatch):
    """Each conv 3x3 + bias + ReLU of the frozen trunk, forward and input gradient, from the oracle's float32 input at its 512^2-crop shape
    (3->64 with K = 27 on 512-wide rows, 64->64 at 512^2 through the per-tensor maximum, 512->512 at 64^2 and 32^2).  The trunk parameters get no
    gradient and no weight-gradient or bias-reduction work is launched."""
    torch = _torch()
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd import conv as agc
    from animatablegaussians_amd.styleunet_ops import noise_bias_act
    calls = _spy_frozen_trunk(monkeypatch, _lib.lib())
    dev = torch.device("cuda:0")
    worst, fails = 0.0, []
    assert len(trunk_cases) == 13
    with _Math(mode):
        for c in trunk_cases:
            w, b = c["w"].to(dev), c["b"].to(dev)
            x = c["x"].to(dev).requires_grad_(True)
            y = noise_bias_act(agc.conv2d(x, w, stride=1, padding=1), None, None, b, 0.0, 1.0)
            y.backward(c["up"].to(dev))
            torch.cuda.synchronize()
            agc.check_status()
            print(f"[lpips] {mode} {c['name']}: ReLU-flip mask {c['masked']:.2e} of the upstream gradient")
            worst = max(worst, _check(f"{mode} unit {c['name']}", {"out": y, "grad x": x.grad}, c["o64"], c["o32"], fails))
    print(f"[lpips] {mode} trunk units: worst ours/bar {worst:.2f}")
    assert not fails, fails
    assert calls["weight"] == 0 and calls["nba"] == 13 and calls["nba_reduction"] == 0, calls


def _spy_frozen_trunk(monkeypatch, L):
    """Counts the weight-gradient convolutions and the bias / noise-strength reductions the backward asks the library for."""
    calls = {"weight": 0, "nba": 0, "nba_reduction": 0}
    conv_w, nba = L.ag_conv_backward_weight, L.ag_noise_bias_act_backward

    def spy_w(*a):
        calls["weight"] += 1
        return conv_w(*a)

    def spy_nba(*a):             # (gx, gy, y, noise, gbias, gnoise_weight, partials, ...)
        calls["nba"] += 1
        calls["nba_reduction"] += any(p is not None for p in a[4:7])
        return nba(*a)

    monkeypatch.setattr(L, "ag_conv_backward_weight", spy_w)
    monkeypatch.setattr(L, "ag_noise_bias_act_backward", spy_nba)
    return calls


# ---------------------------------------------------------------------------------------------------------------------------------
# B.  maxpool2x2 at every pool shape of the crop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(64, 512, 512), (128, 256, 256), (256, 128, 128), (512, 64, 64), (96, 385, 513)])
def test_maxpool_at_crop_shapes_bit_identical(C, H, W):
    """Forward, argmax routing and backward bit-identical to F.max_pool2d, on post-ReLU values quantised to 1/8 (ties between positive
    values and between zeros everywhere: the first maximum wins).  At these sizes the forward's grid-stride loop runs up to twice and the
    backward's (one thread per input element) up to ten times.  The gradient buffer is handed out poisoned with NaN by the caching allocator,
    so every element the backward fails to write -- the dropped trailing row and column of the odd size included -- shows."""
    torch = _torch()
    import torch.nn.functional as F
    from animatablegaussians_amd.lpips import maxpool2x2
    g = torch.Generator().manual_seed(C * 7 + H)
    x = torch.relu(torch.round(torch.randn(1, C, H, W, generator=g) * 8) / 8)
    xc = x.clone().requires_grad_(True)
    yc = F.max_pool2d(xc, 2, 2)
    up = torch.randn(yc.shape, generator=g)
    (yc * up).sum().backward()
    ties = float((yc.detach() > 0).double().mean())
    xg = x.cuda().requires_grad_(True)
    yg = maxpool2x2(xg)
    poison = torch.full_like(xg, float("nan"))               # the backward's torch.empty is served from this block
    del poison
    yg.backward(up.cuda())
    torch.cuda.synchronize()
    gx = xg.grad.cpu()
    assert torch.equal(yg.detach().cpu(), yc.detach())
    assert torch.equal(gx, xc.grad), float((gx - xc.grad).abs().nan_to_num(1e30).max())
    if H % 2 or W % 2:
        assert not gx[..., H - 1, :].any() and not gx[..., W - 1].any()
    print(f"[lpips] maxpool {C}x{H}x{W}: bit-identical ({ties:.2f} of the outputs positive, "
          f"grid passes fwd {-(-C * (H // 2) * (W // 2) // (8192 * 256))} bwd {-(-C * H * W // (8192 * 256))})")


# ---------------------------------------------------------------------------------------------------------------------------------
# C.  _LpipsLevel at every tap shape
# ---------------------------------------------------------------------------------------------------------------------------------
def _level_ref(f0, f1, lin, gout, dt):
    torch = _torch()
    from oracle import lpips_oracle as lo
    import torch.nn.functional as F
    a = f0.detach().to(dt, copy=True).requires_grad_(True)
    v = F.conv2d((lo.normalize_tensor(a) - lo.normalize_tensor(f1.to(dt))) ** 2, lin.to(dt).view(1, -1, 1, 1)).mean()
    (gout * v).backward()
    return {"value": v.detach().double(), "grad f0": a.grad.double()}


def _level_features(C, H, W, regime, g):
    """Post-ReLU-like feature stacks [1, C, H, W]: per-pixel scales spanning four decades; a quarter of the columns exactly equal on both sides
    (the background), and pixels whose whole feature vector is zero on both sides, on one side only, or of norm ~1e-3."""
    torch = _torch()
    scale = 10 ** (torch.rand(1, 1, H, W, generator=g) * 4 - 2)
    pre1 = torch.randn(1, C, H, W, generator=g)
    f1 = torch.relu(pre1) * scale
    if regime == "near":
        f0 = torch.relu(pre1 + 1e-2 * torch.randn(1, C, H, W, generator=g)) * scale
    else:
        f0 = torch.relu(torch.randn(1, C, H, W, generator=g)) * scale
    f0[..., : W // 4] = f1[..., : W // 4]
    sel = torch.rand(H, W, generator=g)
    both, only0, only1, tiny = sel < 0.02, (sel >= 0.02) & (sel < 0.03), (sel >= 0.03) & (sel < 0.04), (sel >= 0.04) & (sel < 0.05)
    f0[..., both] = 0.0
    f1[..., both] = 0.0
    f0[..., only0] = 0.0
    f1[..., only1] = 0.0
    f0[..., tiny] *= 1e-3 / f0[..., tiny].norm(dim=1, keepdim=True).clamp_min(1e-30)
    return f0.contiguous(), f1.contiguous()


@pytest.fixture(scope="module")
def level_cases():
    torch = _torch()
    cases = []
    for i, (C, H, W) in enumerate([(64, 512, 512), (128, 256, 256), (256, 128, 128), (512, 64, 64), (512, 32, 32), (8, 768, 1024)]):
        for regime in ("near", "indep"):
            g = torch.Generator().manual_seed(900 + 10 * i + (regime == "indep"))
            f0, f1 = _level_features(C, H, W, regime, g)
            lin = torch.rand(C, generator=g) / C ** 0.5
            cases.append(dict(name=f"{regime} {C}@{H}x{W}", f0=f0, f1=f1, lin=lin,
                              o64=_level_ref(f0, f1, lin, 3.0, torch.float64), o32=_level_ref(f0, f1, lin, 3.0, torch.float32)))
    return cases


def test_level_at_tap_shapes_vs_oracle(level_cases):
    """The fused per-level distance, forward and backward, against the float64 formula at every tap shape of the 512^2 crop and at
    8@768x1024 (HW > 2048 x 256: the grid-stride loop runs); equal feature vectors give (next to) zero distance and gradient."""
    torch = _torch()
    from animatablegaussians_amd.lpips import _LpipsLevel
    worst, fails = 0.0, []
    for c in level_cases:
        f0 = c["f0"].cuda().requires_grad_(True)
        got = _LpipsLevel.apply(f0, c["f1"].cuda(), c["lin"].cuda())
        (3.0 * got).sum().backward()
        torch.cuda.synchronize()
        worst = max(worst, _check(f"level {c['name']}", {"value": got.reshape(()), "grad f0": f0.grad}, c["o64"], c["o32"], fails))
        # where the two feature vectors are equal (the shared background, pixels zero on both sides) the float64 distance and gradient are 0;
        # the kernel leaves a rounding residue there (measured 1e-8 of max|grad|): reported, and held far below the bar
        eq = (c["f0"][0] == c["f1"][0]).all(0).cuda()
        resid = float(f0.grad[0][:, eq].abs().max()) / float(c["o64"]["grad f0"].abs().max())
        print(f"[lpips] level {c['name']}: gradient on equal pixels {resid:.1e} of max|grad|")
        if resid > 1e-6:
            fails.append((c["name"], "gradient on equal pixels", resid))
    print(f"[lpips] level: worst ours/bar {worst:.2f}")
    assert not fails, fails
    for C, H, W in ((64, 512, 512), (8, 768, 1024)):          # both images equal: the float64 distance is exactly 0
        g = torch.Generator().manual_seed(C)
        f = _level_features(C, H, W, "near", g)[1].cuda()
        f0 = f.clone().requires_grad_(True)
        lin = torch.rand(C, generator=g).cuda()
        got = _LpipsLevel.apply(f0, f, lin)
        got.sum().backward()
        gmax = float(_LpipsLevel.apply(f.clone().requires_grad_(True), f.flip(-1), lin))   # the scale of a distance between unequal stacks
        print(f"[lpips] level equal stacks {C}@{H}x{W}: value {float(got):.1e} (vs {gmax:.1e} for unequal ones), max|grad| {float(f0.grad.abs().max()):.1e}")
        assert float(got) <= 1e-9 * gmax and float(f0.grad.abs().max()) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
# D.  the whole module
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_cases():
    """Input pairs and the oracle in float64 / float32: the nearly-equal 512^2 crop, two independent 512^2 images, and a nearly-equal
    200 x 148 crop (every pool floors).  Also where the float64 per-pixel distance is exactly zero, per level."""
    torch = _torch()
    sd32, sd64 = _sd(torch.float32), _sd(torch.float64)
    cases = {}
    for name, (in0, in1) in (("near 512x512", _crop_pair(11)), ("indep 512x512", _indep_pair(13)), ("near 200x148", _crop_pair(15, 200, 148, 30))):
        o64, maps64 = _oracle_lpips(in0, in1, sd64, torch.float64)
        o32, _ = _oracle_lpips(in0, in1, sd32, torch.float32)
        cases[name] = dict(in0=in0, in1=in1, o64=o64, o32=o32, zero=[mp == 0 for mp in maps64])
    return cases


class _LevelSpy:
    """Stands in for lpips._LpipsLevel and keeps every level's value (LPIPS returns the total in slot 0 of its per-layer list)."""

    def __init__(self, real):
        self.real, self.outs = real, []

    def apply(self, *a):
        r = self.real.apply(*a)
        self.outs.append(r)
        return r


@pytest.mark.parametrize("mode", MODES)
def test_module_at_crop_shape_vs_oracle(mode, module_cases, monkeypatch):
    """LPIPS.forward(retPerLayer=True, normalize=True): total, the five level values and the gradient w.r.t. the prediction.  Also reports what
    the product's distance picks up where the float64 one is exactly zero (receptive fields inside the identical background): in split_f16 the
    two branches' convolutions are rounded on their own per-tensor scales there."""
    torch = _torch()
    import torch.nn.functional as F
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd import conv as agc
    from animatablegaussians_amd import lpips as lp
    from oracle import lpips_oracle as lo
    m = _module()
    calls = _spy_frozen_trunk(monkeypatch, _lib.lib())
    worst, fails = 0.0, []
    with _Math(mode):
        for name, c in module_cases.items():
            spy = _LevelSpy(lp._LpipsLevel)
            monkeypatch.setattr(lp, "_LpipsLevel", spy)
            a = c["in0"].cuda().requires_grad_(True)
            val, res = m(a, c["in1"].cuda(), retPerLayer=True, normalize=True)
            val.sum().backward()
            torch.cuda.synchronize()
            agc.check_status()
            monkeypatch.setattr(lp, "_LpipsLevel", spy.real)
            assert len(spy.outs) == 5 and torch.equal(res[0], val) and all(torch.equal(r.reshape(-1), o) for r, o in zip(res[1:], spy.outs[1:]))
            got = {"total": val.reshape(()), **{f"level{k}": spy.outs[k].reshape(()) for k in range(5)}, "grad in0": a.grad}
            worst = max(worst, _check(f"{mode} module {name}", got, c["o64"], c["o32"], fails, chain=("grad in0",)))
            # the product's per-pixel distance, in float64 from its own float32 taps, where the oracle's is exactly zero
            with torch.no_grad():
                t0 = m.features(((2 * a - 1 - m.scaling_layer__shift) / m.scaling_layer__scale).contiguous())
                t1 = m.features(((2 * c["in1"].cuda() - 1 - m.scaling_layer__shift) / m.scaling_layer__scale).contiguous())
            pick, frac = 0.0, []
            for k in range(5):
                d = F.conv2d((lo.normalize_tensor(t0[k].double()) - lo.normalize_tensor(t1[k].double())) ** 2,
                             m._w(f"lin{k}.model.1.weight").double()).reshape(-1).cpu()
                z = c["zero"][k]
                pick += float(d[z].sum()) / d.numel()
                frac.append(float(z.double().mean()))
            print(f"[lpips] {mode} module {name}: exactly-equal region {', '.join(f'{f:.2f}' for f in frac)} of the pixels per level, "
                  f"picks up {pick:.3e} = {pick / float(c['o64']['total']):.2e} of the total")
            if pick > (K * _rel(c["o32"]["total"], c["o64"]["total"]) + FLOOR) * float(c["o64"]["total"]):
                fails.append((name, "equal-region pickup", pick))
            del a, val, res, t0, t1
    print(f"[lpips] {mode} module: worst ours/bar {worst:.2f}")
    assert not fails, fails
    assert calls["weight"] == 0 and calls["nba_reduction"] == 0, calls
    assert all(p.grad is None for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------------------------
# E.  the loss tail end to end
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_WEIGHT = {"l1": 1.0, "mask": 0.1, "lpips": 0.1, "offset": 0.005}
RENDER = 1024


def _crop_ref(mask, patch, randomly, bg, *images):
    """main_avatar.py:75-115 in the oracle's dtype: the square around the mask's bounding box (last row / column excluded, as there), the
    background around the shorter side, then a random patch x patch window (one draw for all images) or a bilinear resize."""
    torch = _torch()
    import torch.nn.functional as F
    rows = torch.nonzero(mask.any(1)).reshape(-1)
    cols = torch.nonzero(mask.any(0)).reshape(-1)
    v0, v1, u0, u1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    hv, hu = v1 - v0, u1 - u0
    side = max(hv, hu)
    window = None
    if randomly and side > patch:
        window = (int(torch.randint(0, side - patch + 1, (1,))), int(torch.randint(0, side - patch + 1, (1,))))
    out = []
    for im in images:
        sq = bg.reshape(3, 1, 1).expand(3, side, side).clone()
        top, left = (0, (side - hu) // 2) if hv > hu else ((side - hv) // 2, 0)
        sq[:, top:top + hv, left:left + hu] = im[:, v0:v1, u0:u1]
        if window is not None:
            sq = sq[:, window[0]:window[0] + patch, window[1]:window[1] + patch]
        else:
            sq = F.interpolate(sq[None], size=(patch, patch), mode="bilinear")[0]
        out.append(sq)
    return out


def _loss_ref(inp, case, sd, dt, patch, randomly, seed):
    """main_avatar.py:196-245 (forward_one_pass_pretrain's loss) in ``dt``, the LPIPS term by the oracle with the [2, 1, 0] channel flip."""
    torch = _torch()
    from oracle import lpips_oracle as lo
    x = {k: inp[k].detach().to(dt).requires_grad_(True) for k in ("rgb_map", "mask_map", "offset")}
    bg = torch.tensor(BG, dtype=dt)
    keep = 1.0 - case["boundary"].to(dt)
    gt = case["color"].to(dt).clone()
    gt[~case["mask"]] = bg
    gt = gt.permute(2, 0, 1)
    image = x["rgb_map"].permute(2, 0, 1)
    image = image * keep + (1.0 - keep) * bg[:, None, None]
    gt = gt * keep + (1.0 - keep) * bg[:, None, None]
    parts = {"l1_loss": (image - gt).abs().mean(),
             "mask_loss": (x["mask_map"][..., 0] * keep - case["mask"].to(dt) * keep).abs().mean()}
    torch.manual_seed(seed)
    ci, cg = _crop_ref(case["mask"], patch, randomly, bg, image, gt)
    parts["lpips_loss"] = lo.lpips(ci[None, [2, 1, 0]], cg[None, [2, 1, 0]], sd, normalize=True)[0].mean()
    parts["offset_loss"] = x["offset"].norm(dim=-1).mean()
    total = sum(LOSS_WEIGHT[k[:-5]] * v for k, v in parts.items())
    total.backward()
    res = {"total": total.detach().double(), **{k: v.detach().double() for k, v in parts.items()}}
    res.update({f"grad {k}": v.grad.double() for k, v in x.items()})
    return res


def _render_case(tall, seed):
    """A 1024^2 'render' and dataset item: an elliptic subject (taller than wide, or wider than tall) with a 3-pixel boundary band, the ground
    truth textured, the render equal to the composited ground truth plus a smooth 1e-2 residual, a soft rendered mask, 5000 offsets."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    n = RENDER
    yy, xx = torch.meshgrid(torch.arange(n, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij")
    ry, rx = (350.0, 210.0) if tall else (210.0, 350.0)
    r = torch.sqrt(((yy - 520) / ry) ** 2 + ((xx - 490) / rx) ** 2)
    mask = r <= 1.0
    boundary = (r - 1.0).abs() * min(ry, rx) <= 1.5
    color = _texture(g, n, n).permute(1, 2, 0).contiguous()
    comp = color.clone()
    comp[~mask] = torch.tensor(BG)
    rgb = (comp + 1e-2 * (2 * _smooth(g, 3, n, n, 16).permute(1, 2, 0) - 1)).contiguous()
    mask_map = (mask.float() + 0.05 * (2 * _smooth(g, 1, n, n, 32)[0] - 1)).clamp(0, 1)[..., None].contiguous()
    offset = torch.randn(5000, 3, generator=g) * 0.01
    return dict(color=color, mask=mask, boundary=boundary, inp={"rgb_map": rgb, "mask_map": mask_map, "offset": offset})


LOSS_CASES = [("tall resize", True, False), ("wide resize", False, False), ("tall random", True, True), ("wide random", False, True)]


@pytest.fixture(scope="module")
def loss_cases():
    torch = _torch()
    sd32, sd64 = _sd(torch.float32), _sd(torch.float64)
    cases = []
    for i, (name, tall, randomly) in enumerate(LOSS_CASES):
        c = _render_case(tall, 700 + i)
        from animatablegaussians_amd.losses import mask_bbox
        v0, u0, v1, u1 = mask_bbox(c["mask"].numpy())
        assert ((v1 - v0) > (u1 - u0)) == tall and max(v1 - v0, u1 - u0) > S
        seed = 4000 + i
        cases.append(dict(name=name, randomly=randomly, seed=seed, **c,
                          o64=_loss_ref(c["inp"], c, sd64, torch.float64, S, randomly, seed),
                          o32=_loss_ref(c["inp"], c, sd32, torch.float32, S, randomly, seed)))
    return cases


@pytest.mark.parametrize("mode", MODES)
def test_training_loss_tail_vs_oracle(mode, loss_cases):
    """losses.training_loss at a 1024^2 render: the total, every part, and the gradients w.r.t. rgb_map, mask_map and offset, for a bounding box
    taller and one wider than the crop, the resized and the random-window crop, with the host bounding box passed in and without it."""
    torch = _torch()
    from animatablegaussians_amd import losses
    m = _module()
    bg = torch.tensor(BG).cuda()
    worst, fails = 0.0, []
    with _Math(mode):
        for c in loss_cases:
            items = {"color_img": c["color"].cuda(), "mask_img": c["mask"].cuda(), "boundary_mask_img": c["boundary"].cuda()}
            for bbox in (False, True):
                it = {**items, "mask_bbox": losses.mask_bbox(c["mask"].numpy())} if bbox else items
                x = {k: v.cuda().requires_grad_(True) for k, v in c["inp"].items()}
                torch.manual_seed(c["seed"])
                total, parts = losses.training_loss(x, it, bg, LOSS_WEIGHT, lpips=m, patch_size=S, random_patch=c["randomly"])
                total.backward()
                torch.cuda.synchronize()
                got = {"total": total, **parts, **{f"grad {k}": v.grad for k, v in x.items()}}
                assert set(got) == set(c["o64"])
                tag = f"{mode} loss {c['name']} {'host bbox' if bbox else 'device bbox'}"
                worst = max(worst, _check(tag, got, c["o64"], c["o32"], fails, chain=("grad rgb_map",)))
    print(f"[lpips] {mode} loss tail: worst ours/bar {worst:.2f}")
    assert not fails, fails
