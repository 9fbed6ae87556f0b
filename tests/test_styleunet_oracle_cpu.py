"""Pins oracle/dual_styleunet_oracle.py -- the plain-torch CPU restatement of the reference's DualStyleUNet.forward that bench.py times
as `cpu_baseline_styleunet` -- against the fixture the REFERENCE MODULE ITSELF produced (tests/golden/make_golden_dual_styleunet.py):
forward images and every parameter gradient, in float32 (the reference as shipped).  The restatement runs the same torch CPU ops
in the same order, so it must agree with the reference's own float32 run to rounding: held here to 2x the reference's float32-vs-float64
deviation + 1e-6 per stored tensor."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "dual_styleunet_512_1024.npz")


def _sub(t, n=256):
    f = t.detach().flatten()
    step = max(1, f.numel() // n)
    return f[::step][:n].double().numpy()


def test_cpu_oracle_of_the_whole_network_matches_the_reference_modules_golden():
    from animatablegaussians_amd import synth
    from oracle.dual_styleunet_oracle import DualStyleUNetOracle
    gold = np.load(GOLD)
    shapes = {k[len("shape:"):]: tuple(int(v) for v in gold[k]) for k in gold.files if k.startswith("shape:")}
    sd = synth.named_fill({k: torch.empty(s) for k, s in shapes.items()})
    learn = [k for k in sd if not k.startswith("noises.")]
    for k in learn:
        sd[k].requires_grad_(True)
    pose = synth.pose_map(512).requires_grad_(True)
    style = torch.ones(1, 512) / np.sqrt(512)
    torch.set_num_threads(os.cpu_count() or 1)
    images = DualStyleUNetOracle(sd).forward(style, pose)
    assert images.shape == (1, 6, 1024, 1024)
    scale = float(gold["images_max"])
    for key, got in (("images_sub16", images[0, :, ::16, ::16]), ("images_crop_a", images[0, :, 500:532, 500:532]),
                     ("images_crop_b", images[0, :, 100:132, 700:732])):
        d = np.abs(got.detach().numpy() - gold[key]).max() / scale
        assert d <= 2 * float(gold["err32:" + key]) + 1e-6, (key, d, float(gold["err32:" + key]))
    G = torch.randn(images.shape, generator=torch.Generator().manual_seed(4242))
    (images * G).sum().backward()
    d = np.abs(pose.grad[0, :, ::8, ::8].numpy() - gold["pose_grad_sub8"]).max() / float(gold["pose_grad_max"])
    assert d <= 2 * float(gold["err32:pose_grad_sub8"]) + 1e-6, d
    worst = 0.0
    for k in learn:
        g = sd[k].grad
        assert g is not None, k
        d = np.abs(_sub(g) - gold["grad:" + k]).max() / max(float(gold["gmax:" + k]), 1e-30)
        lim = 2 * float(gold["err32:grad:" + k]) + 1e-6
        worst = max(worst, d / lim)
        assert d <= lim, (k, d, lim)
    print(f"oracle vs the reference module's golden: {len(learn)} parameter gradients, worst ratio to 2x the reference's own fp32 noise {worst:.2f}")


def test_the_one_number_gradients_move_by_factors_when_the_reference_arithmetic_is_reassociated():
    """Why tests/test_styleunet_net.py holds the noise strengths and the pose-map gradient to caps of their own, and why the product's grouped chain
    (comb convolutions as two halves, grouped.py) reads differently on exactly those rows than the one-network path (round-4 review, weak #1):
    in the REFERENCE'S OWN arithmetic (torch CPU fp32, oneDNN) re-associating the comb convolutions the same way leaves the forward and the bulk of
    the gradients where they were, and moves single noise-strength scalars by factors -- they are sums over a whole feature map of products with
    mixed signs behind leaky-ReLU slope selections of pre-activations within rounding of zero.  Measured here (profiles/r05_comb_split_conditioning_cpu.txt):
    convs2.5.noise.weight 6.1e-2 -> 3.6e-2, convs1.5.noise.weight 1.9e-4 -> 5.1e-5 of the value; forward 1.0e-6, median tensor 9e-5 -> 7e-5,
    90th percentile 6.7e-4 -> 7.3e-4."""
    from animatablegaussians_amd import synth
    from oracle.dual_styleunet_oracle import DualStyleUNetOracle
    gold = np.load(GOLD)
    shapes = {k[len("shape:"):]: tuple(int(v) for v in gold[k]) for k in gold.files if k.startswith("shape:")}
    sd = synth.named_fill({k: torch.empty(s) for k, s in shapes.items()})
    learn = [k for k in sd if not k.startswith("noises.")]
    for k in learn:
        sd[k].requires_grad_(True)
    pose = synth.pose_map(512).requires_grad_(True)
    style = torch.ones(1, 512) / np.sqrt(512)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    images = DualStyleUNetOracle(sd, comb_as_two_halves=True).forward(style, pose)
    scale = float(gold["images_max"])
    assert np.abs(images[0, :, ::16, ::16].detach().numpy() - gold["images_sub16"]).max() / scale <= 2 * float(gold["err32:images_sub16"]) + 1e-6
    G = torch.randn(images.shape, generator=torch.Generator().manual_seed(4242))
    (images * G).sum().backward()
    two = {k: np.abs(_sub(sd[k].grad) - gold["grad:" + k]).max() / max(float(gold["gmax:" + k]), 1e-30) for k in learn}
    one = {k: float(gold["err32:grad:" + k]) for k in learn}
    ratio = {k: max(two[k], 1e-5) / max(one[k], 1e-5) for k in learn}               # deviations below 1e-5 of the value count as equal
    scalars = [k for k in learn if k.endswith("noise.weight")]
    moved = sorted(((max(ratio[k], 1 / ratio[k]), k) for k in scalars), reverse=True)
    print("noise strengths, factor between the two associations (reference arithmetic): " + ", ".join(f"{k} {f:.1f}x" for f, k in moved[:5]))
    assert moved[0][0] >= 2.0 and moved[1][0] >= 1.5                       # single scalars move by factors ...
    tens = [k for k in learn if k not in scalars]
    v1, v2 = np.array([one[k] for k in tens]), np.array([two[k] for k in tens])
    for q in (50, 90):                                                     # ... the bulk of the tensors does not
        assert 0.6 <= np.percentile(v2, q) / np.percentile(v1, q) <= 1.6, (q, np.percentile(v1, q), np.percentile(v2, q))


def test_forward_views_is_forward_per_view_and_sums_the_shared_gradients():
    """DualStyleUNetOracle.forward_views -- the encoder and decoder stages 0..4 once per branch, the view feature and the tail per view, the yardstick
    of tests/test_multiview_tail_gpu.py -- against ``forward`` run once per view, in float64, on a network small enough for the CPU (256 -> 512,
    middle 4: the same stage layout, the view stage followed by a comb convolution).  Every view's image must equal forward's BIT FOR BIT (the same
    operations on the same values); after a backward of per-view upstream gradients every parameter gradient and every view feature's gradient must
    equal the sum of the single-view passes' up to float64 summation order."""
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.styleunet import DualStyleUNet
    from oracle.dual_styleunet_oracle import DualStyleUNetOracle
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    net = DualStyleUNet(inp_size=256, out_size=512, middle_size=4, channel_multiplier=1, style_dim=64)
    base = {k: v.double() for k, v in synth.named_fill(net.reference_state_dict(), seed=77).items()}
    learn = [k for k in base if not k.startswith("noises.")]

    def make():
        sd = {k: v.clone().requires_grad_(k in learn) for k, v in base.items()}
        return sd, DualStyleUNetOracle(sd, inp_size=256, out_size=512, middle_size=4)
    g = torch.Generator().manual_seed(78)
    style = torch.randn(1, 64, generator=g, dtype=torch.float64)
    pose = torch.randn(1, 3, 256, 256, generator=g, dtype=torch.float64)
    vfs = [[torch.randn(1, 128, 32, 32, generator=g, dtype=torch.float64) for _ in range(2)] for _ in range(2)]
    ups = [torch.randn(1, 6, 512, 512, generator=g, dtype=torch.float64) for _ in range(2)]
    _, o = make()
    assert o.VIEW_STAGE + 1 < o.n_enc + 1 and o.VIEW_STAGE + 1 < o.n_dec            # the tail starts with a comb convolution, as in the product

    # forward only: bit for bit
    with torch.no_grad():
        multi = o.forward_views(style, pose, vfs)
        for v in range(2):
            assert torch.equal(multi[v], o.forward(style, pose, *vfs[v])), v
        # a view without features, and features on one branch only
        mixed = o.forward_views(style, pose, [(None, None), (vfs[1][0], None)])
        assert torch.equal(mixed[0], o.forward(style, pose)) and torch.equal(mixed[1], o.forward(style, pose, vfs[1][0], None))

    # with the upstream gradients: one backward per view, the shared gradients summed
    sd_m, o_m = make()
    vm = [[t.clone().requires_grad_(True) for t in pair] for pair in vfs]
    seen = []
    imgs = o_m.forward_views(style, pose, vm, upstream=ups, after_view=lambda v: seen.append((v, sd_m["convs1.0.conv.weight"].grad.clone())))
    assert [v for v, _ in seen] == [0, 1] and all(not i.requires_grad for i in imgs)
    sd_s, o_s = make()
    vs = [[t.clone().requires_grad_(True) for t in pair] for pair in vfs]
    for v in range(2):
        img = o_s.forward(style, pose, *vs[v])
        assert torch.equal(img.detach(), imgs[v]), v
        (img * ups[v]).sum().backward()
        if v == 0:                                                                    # after view 0: the first view's gradient alone
            assert torch.allclose(seen[0][1], sd_s["convs1.0.conv.weight"].grad, rtol=0, atol=1e-12 * float(seen[0][1].abs().max()))
    for k in learn:
        a, b = sd_m[k].grad, sd_s[k].grad
        assert a is not None and b is not None, k
        assert float((a - b).abs().max()) <= 1e-10 * max(float(b.abs().max()), 1e-300), (k, float((a - b).abs().max()), float(b.abs().max()))
    for v in range(2):
        for b in range(2):
            assert torch.equal(vm[v][b].grad, vs[v][b].grad) or float((vm[v][b].grad - vs[v][b].grad).abs().max()) <= 1e-12 * float(vs[v][b].grad.abs().max())
