"""Shared helpers of the parity tests (tests only)."""
import ctypes
import os

import numpy as np

from animatablegaussians_amd import camera


def cam_of(scene_or_cam):
    return camera.camera_from_intr_extr(scene_or_cam["extr"], scene_or_cam["intr"], scene_or_cam["img_w"], scene_or_cam["img_h"])


def oracle_forward(scene, cam, scale_modifier=1.0, **kw):
    from oracle import raster_oracle as ro
    return ro.forward(scene["means3D"], scene["colors"], scene["opacities"], scene.get("scales"), scene.get("rotations"),
                      scene["bg"], cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"], cam["tanfovy"],
                      cam["img_w"], cam["img_h"], scale_modifier=scale_modifier, cov3D_precomp=scene.get("cov3D_precomp"), **kw)


def oracle_backward(st, scene, cam, grads, scale_modifier=1.0):
    from oracle import raster_oracle as ro
    return ro.backward(st, scene["means3D"], scene["colors"], scene.get("scales"), scene.get("rotations"), scene["bg"],
                       cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"], cam["tanfovy"],
                       grads["dL_dcolor"], grads["dL_ddepth"], grads["dL_dalpha"], scale_modifier=scale_modifier,
                       cov3D_precomp=scene.get("cov3D_precomp"))


def gpu_settings(scene, cam, device="cuda", debug=False, scale_modifier=1.0):
    import torch
    from animatablegaussians_amd.rasterizer import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return GaussianRasterizationSettings(
        image_height=cam["img_h"], image_width=cam["img_w"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=t(scene["bg"]), scale_modifier=scale_modifier, viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]),
        sh_degree=0, campos=t(cam["campos"]), prefiltered=False, debug=debug)


def gpu_inputs(scene, device="cuda", requires_grad=False):
    import torch
    out = {}
    for k in ("means3D", "colors", "opacities", "scales", "rotations", "cov3D_precomp"):
        if scene.get(k) is None:
            out[k] = None
            continue
        v = torch.from_numpy(np.ascontiguousarray(scene[k])).to(device)
        if requires_grad:
            v.requires_grad_(True)
        out[k] = v
    return out


def _scratch_view(buf, off, nbytes, dtype):
    base = buf.data_ptr()
    start = ((base + 255) & ~255) - base + off
    return buf[start:start + nbytes].cpu().numpy().view(dtype)


def gpu_native_forward(scene, cam, device="cuda", scale_modifier=1.0):
    """Call the `_C.rasterize_gaussians` equivalent and unpack the private scratch for comparison."""
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.rasterizer import native_rasterize_gaussians
    rs = gpu_settings(scene, cam, device, scale_modifier=scale_modifier)
    inp = gpu_inputs(scene, device)
    empty = torch.Tensor([])
    e = lambda v: empty if v is None else v  # noqa: E731
    R, color, depth, alpha, radii, geom, binning, img = native_rasterize_gaussians(
        rs.bg, inp["means3D"], inp["colors"], inp["opacities"], e(inp["scales"]), e(inp["rotations"]), scale_modifier,
        e(inp["cov3D_precomp"]), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width,
        empty, 0, rs.campos, False, True)
    P, W, H = scene["means3D"].shape[0], cam["img_w"], cam["img_h"]
    st = {"num_rendered": R, "color": color.cpu().numpy(), "depth": depth.cpu().numpy(), "alpha": alpha.cpu().numpy(),
          "radii": radii.cpu().numpy(),
          "_torch": dict(rs=rs, inp=inp, radii=radii, geom=geom, binning=binning, img=img, alpha=alpha)}
    if P == 0:
        return st
    L = _lib.lib()
    lay = _lib.AgRasterScratchLayout()
    _lib.check(L.ag_raster_describe_scratch(P, W, H, R, ctypes.byref(lay)), "describe")
    view = _scratch_view
    rec = view(geom, lay.geom_rec_off, P * lay.geom_rec_stride, np.float32).reshape(P, lay.geom_rec_stride // 4)
    vis = st["radii"] > 0
    z = lambda a: np.where(vis.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(a.dtype)  # noqa: E731
    st["means2D"] = z(rec[:, 0:2].copy())
    st["conic_opacity"] = z(rec[:, 2:6].copy())
    st["depths"] = z(rec[:, 9].copy())
    st["r2cut"] = rec[:, 10].copy()
    st["cov3D"] = z(view(geom, lay.geom_cov3d_off, P * 24, np.float32).reshape(P, 6).copy())
    st["tiles_touched"] = view(geom, lay.geom_tiles_touched_off, P * 4, np.uint32).copy()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    st["ranges"] = view(img, lay.img_ranges_off, T * 8, np.uint32).reshape(T, 2).copy()
    st["n_contrib"] = view(img, lay.img_n_contrib_off, W * H * 4, np.uint32).reshape(H, W).copy()
    st["tile_count"] = view(img, lay.img_tile_count_off, T * 4, np.uint32).copy()
    if R > 0:
        st["point_list"] = view(binning, lay.bin_point_list_off, R * 4, np.uint32).copy()
        st["keys"] = view(binning, lay.bin_keys_off, R * 8, np.uint64).copy()
    else:
        st["point_list"] = np.zeros(0, np.uint32)
        st["keys"] = np.zeros(0, np.uint64)
    return st


def gpu_native_backward(fw, grads, alphas=None, scale_modifier=1.0):
    """`_C.rasterize_gaussians_backward` equivalent on the forward state `fw` (from gpu_native_forward).
    `alphas` overrides the saved forward alpha map (an explicit input of the reference's backward too).
    Returns the 8 API gradients plus the internal accumulators dL_dconic [P,4] and dL_ddepths [P,1]."""
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd.rasterizer import native_rasterize_gaussians_backward
    t = fw["_torch"]
    rs, inp = t["rs"], t["inp"]
    dev = inp["means3D"].device
    empty = torch.Tensor([])
    e = lambda v: empty if v is None else v  # noqa: E731
    P = inp["means3D"].shape[0]
    accum = torch.empty((_lib.lib().ag_raster_accum_bytes(P),), dtype=torch.uint8, device=dev)
    al = t["alpha"] if alphas is None else torch.from_numpy(np.ascontiguousarray(alphas)).to(dev)
    g = lambda k: torch.from_numpy(np.ascontiguousarray(grads[k])).to(dev)  # noqa: E731
    out = native_rasterize_gaussians_backward(
        rs.bg, inp["means3D"], t["radii"], inp["colors"], e(inp["scales"]), e(inp["rotations"]), scale_modifier,
        e(inp["cov3D_precomp"]), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, g("dL_dcolor"), g("dL_ddepth"),
        g("dL_dalpha"), empty, 0, rs.campos, t["geom"], fw["num_rendered"], t["binning"], t["img"], al, True,
        _accum_buffer=accum)
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
    res = {n: o.cpu().numpy() for n, o in zip(names, out)}
    acc = _scratch_view(accum, 0, P * 64, np.float32).reshape(P, 16)
    # the accumulator row holds the MOMENTS of q = G dL/dalpha (csrc/ag_common.h AccumSlot); dL/dconic = -0.5 * opacity * (q dx^2, q dx dy,
    # q dy^2) is applied by the preprocess backward and restated here in float64 for the comparison with the oracle's dL_dconic
    nhop = -0.5 * inp["opacities"].detach().cpu().numpy().astype(np.float64).reshape(P)
    res["dL_dconic"] = np.stack([nhop * acc[:, 2], nhop * acc[:, 3], np.zeros(P), nhop * acc[:, 4]], 1)
    res["dL_ddepths"] = acc[:, 9:10].copy()
    return res


def _bitexact(gpu, ref):
    for k in ("radii", "tiles_touched"):
        assert np.array_equal(gpu[k], ref[k]), f"{k} not bit-exact: {(gpu[k] != ref[k]).sum()} differ"
    vis = ref["radii"] > 0   # per-Gaussian state is only defined (and only consumed) for rasterized Gaussians
    for k in ("means2D", "depths", "conic_opacity", "cov3D"):
        a, b = gpu[k][vis].view(np.uint32), ref[k][vis].view(np.uint32)
        assert np.array_equal(a, b), f"{k} not bit-exact: {(a != b).sum()} words differ, max abs {np.abs(gpu[k] - ref[k]).max()}"
    assert gpu["num_rendered"] == ref["num_rendered"]
    assert np.array_equal(gpu["ranges"], ref["ranges"]), "tile ranges differ"
    assert np.array_equal(gpu["point_list"], ref["point_list"]), "sorted point_list differs"


def assert_image_parity(gpu, ref, atol=1e-4, fragile_atol=6e-3, max_fragile_frac=5e-3):
    """colour/depth/alpha within atol (fp32 tolerance stated by BASELINE.json north_star: 1e-4) at every pixel the
    oracle did not flag as sitting on a discrete blend threshold; flagged pixels may flip one 1/255-sized term."""
    frag = ref["fragile"].astype(bool)
    assert frag.mean() <= max_fragile_frac, f"too many fragile pixels: {frag.mean()}"
    for k in ("color", "depth", "alpha"):
        d = np.abs(gpu[k] - ref[k])
        scale = np.maximum(1.0, np.abs(ref[k]))
        bad = (d > atol * scale) & ~frag[None]
        assert not bad.any(), f"{k}: {bad.sum()} non-fragile pixels differ, max {d[~np.broadcast_to(frag[None], d.shape)].max()}"
        assert (d[np.broadcast_to(frag[None], d.shape)] <= fragile_atol * scale[np.broadcast_to(frag[None], d.shape)]).all(), f"{k}: fragile pixel off by more than one threshold term"
    nc = gpu["n_contrib"] != ref["n_contrib"]
    assert not (nc & ~frag).any(), f"n_contrib differs at {int((nc & ~frag).sum())} non-fragile pixels"
    worst = max(float((np.abs(gpu[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])))[:, ~frag].max()) for k in ("color", "depth", "alpha"))
    print(f"\n[parity] image {ref['color'].shape[2]}x{ref['color'].shape[1]}: {frag.mean():.2e} of pixels fragile (cap {max_fragile_frac:g}), "
          f"worst non-fragile image difference {worst:.2e} (bar {atol:g})")


_SLOT_OF = {"dL_dmeans2D": (0, 1, None), "dL_dconic": (2, 3, None, 4), "dL_dopacity": (5,), "dL_dcolors": (6, 7, 8),
            "dL_ddepths": (9,)}


def assert_accum_parity(got, ref, rtol=1e-4, k_eps=64.0, ref_perturbed=None, k_sens=0.0, max_ratio=1.0):
    """Blend-backward accumulators vs the fp64-accumulated oracle.

    |got - ref| <= rtol*|ref| + k_eps*eps_fp32*sum|term| + 1e-7: the first term is the stated 1e-4 fp32 bar, the
    second is the spread between admissible float summation orders of the reference's atomicAdds (any order is
    "the reference"), with abs_sum measured by the oracle.  ``ref_perturbed`` (end-to-end comparisons only): the oracle's result
    with every exp() scaled by 1 + 2^-20 -- k_sens * |ref_perturbed - ref| is the reference algorithm's own movement under a
    rounding-sized change of its transcendental, added per element.  ``max_ratio``: the cap on the worst ratio to the limit (1.0 = the limit
    itself; a measured-and-capped comparison passes its cap here).  Returns the worst ratio to the limit."""
    eps = float(np.finfo(np.float32).eps)
    worst_all = 0.0
    for name, slots in _SLOT_OF.items():
        g = np.asarray(got[name], np.float64)
        r = np.asarray(ref[name], np.float64)
        assert np.isfinite(g).all(), f"{name}: non-finite"
        for col, slot in enumerate(slots):
            if slot is None:
                assert not g[:, col].any(), f"{name}[:, {col}] must stay zero"
                continue
            d = np.abs(g[:, col] - r[:, col])
            lim = rtol * np.abs(r[:, col]) + k_eps * eps * ref["abs_sum"][:, slot].astype(np.float64) + 1e-7
            if ref_perturbed is not None:
                lim = lim + k_sens * np.abs(np.asarray(ref_perturbed[name], np.float64)[:, col] - r[:, col])
            worst = float((d / lim).max()) if d.size else 0.0
            worst_all = max(worst_all, worst)
            assert worst <= max_ratio, (f"{name}[:, {col}]: {int((d > lim * max_ratio).sum())} of {d.size} over tolerance x {max_ratio:g}, worst ratio "
                                  f"{worst:.2f}, max |diff| {d.max():.3e}, ref max {np.abs(r[:, col]).max():.3e}")
    return worst_all


def assert_rows_close(got, ref, name, rtol=1e-4, row_rtol=1e-5):
    """Per-Gaussian outputs of the streaming backward: |got - ref| <= rtol*|ref| + row_rtol*max|ref row| + 1e-9.
    The row term covers cancellation inside one Gaussian's chain rule (fp32 op order / FMA differ)."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    ref = np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite"
    d = np.abs(got - ref)
    lim = rtol * np.abs(ref) + row_rtol * np.abs(ref).max(axis=1, keepdims=True) + 1e-9
    worst = float((d / lim).max()) if d.size else 0.0
    assert worst <= 1.0, f"{name}: {int((d > lim).sum())} of {d.size} over tolerance, worst ratio {worst:.2f}, max |diff| {d.max():.3e}"




# ---- the reference build's results on two scenes, stored as fixtures (tests/golden/make_golden_ref_live.py) ----------------------------
def live_scene(name):
    """The seeded scenes of tests/golden/ref_live_<name>.npz: ``config1`` (BASELINE.json configs[0]: 10k random Gaussians, one 512x512
    camera) and ``long_lists`` (tile lists longer than one 256-entry batch, near-plane culling, off-screen splats, a ragged image)."""
    from animatablegaussians_amd import synth
    if name == "config1":
        sc = synth.random_gaussians()
    elif name == "long_lists":
        sc = synth.random_gaussians(P=6000, img=200, focal=180.0)
        sc["img_w"], sc["img_h"] = 200, 120
        sc["intr"] = np.array([[180.0, 0, 100], [0, 180.0, 60], [0, 0, 1]], np.float32)
        sc["means3D"][:, :2] *= 0.35
        sc["means3D"][::7, 2] += 2.45           # a band of Gaussians at / behind the near plane
        sc.update(synth.upstream_grads(200, 120, 99))
    else:
        raise KeyError(name)
    return sc, cam_of(sc)


def bits_digest(a):
    """SHA-256 of an array's values for bit-for-bit comparison against a stored fixture: float32 by its bits, integers and booleans by value
    (as int64), the shape included."""
    import hashlib
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        assert a.dtype == np.float32, a.dtype
        body = a.view(np.uint32).tobytes()
    else:
        body = a.astype(np.int64).tobytes()
    return hashlib.sha256(repr(a.shape).encode() + body).hexdigest()


# ---- render3 through the drop-in: the native call it issues (tests/test_dropin_cpu.py, tests/golden/make_golden_dropin.py) ---------------
def render3_cases():
    """Seeded inputs of ``render3(vals, bg, extr, intr, 512, 480, 1.0)``: a colour call and a spherical-harmonics call."""
    import torch
    g = torch.Generator().manual_seed(5)
    P = 37
    base = {"positions": torch.randn(P, 3, generator=g) + torch.tensor([0., 0., 3.]), "opacity": torch.rand(P, 1, generator=g),
            "scales": torch.rand(P, 3, generator=g) * 0.05, "rotations": torch.nn.functional.normalize(torch.randn(P, 4, generator=g)),
            "max_sh_degree": 0}
    extr = torch.eye(4)
    extr[:3, :3] = torch.tensor([[0.8, 0., 0.6], [0., 1., 0.], [-0.6, 0., 0.8]])
    extr[:3, 3] = torch.tensor([0.1, -0.2, 2.5])
    intr = torch.tensor([[1100., 0., 250.], [0., 1090., 260.], [0., 0., 1.]])
    bg = torch.tensor([0.1, 0.2, 0.3])
    cases = []
    for variant in ("colors", "shs"):
        vals = dict(base)
        if variant == "colors":
            vals["colors"] = torch.rand(P, 3, generator=g)
        else:
            vals["shs"] = torch.randn(P, 3, 4, generator=g) * 0.3
            vals["max_sh_degree"] = 1
        cases.append((variant, (vals, bg, extr, intr, 512, 480, 1.0)))
    return cases


class NativeCallRecorder:
    """Replaces ``rasterizer.native_rasterize_gaussians`` (the ``_C.rasterize_gaussians`` equivalent) by a recorder of its arguments and maps
    ``.cuda()`` / ``zeros_like(device=...)`` to the CPU, for as long as the ``with`` block runs."""

    def __enter__(self):
        import torch
        from animatablegaussians_amd import rasterizer as rz
        self.calls = []

        def recorder(*args, **kw):
            self.calls.append((args, kw))
            H, W, P = int(args[12]), int(args[13]), args[1].shape[0]
            z = lambda *s: torch.zeros(*s)  # noqa: E731
            return (0, 0), z(3, H, W), z(1, H, W), z(1, H, W), torch.zeros(P, dtype=torch.int32), z(1), z(1), z(1)

        def zeros_like_cpu(t, **kw):
            kw.pop("device", None)
            return self._real[2](t, **kw)

        self._real = (rz.native_rasterize_gaussians, torch.Tensor.cuda, torch.zeros_like)
        rz.native_rasterize_gaussians = recorder
        torch.Tensor.cuda = lambda self_, *a, **k: self_
        torch.zeros_like = zeros_like_cpu
        return self

    def __exit__(self, *exc):
        import torch
        from animatablegaussians_amd import rasterizer as rz
        rz.native_rasterize_gaussians, torch.Tensor.cuda, torch.zeros_like = self._real
        return False


def cpu_threads():
    """CPUs this process may use: the affinity mask, capped by a cgroup CPU quota (a container can see hundreds of CPUs and be allowed 16; torch's
    default of one thread per visible CPU then spends a CPU oracle's time throttled)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


# ---------------------------------------------------------------------------------------------------------------------------------
# The avatar's StyleUNets against the float64 CPU oracle (oracle/dual_styleunet_oracle.py): tests/test_styleunet_heads_gpu.py,
# tests/test_multiview_tail_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
SEEDS = {"position_net": 1101, "color_net": 2202, "other_net": 3303}
NETS = ("position_net", "other_net", "color_net")            # the order get_maps returns the maps in


class Math:
    """``with Math(mode):`` the product's arithmetic mode (conv.set_math) for the block."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from animatablegaussians_amd import conv as agc
        self.prev = agc.set_math(self.mode)

    def __exit__(self, *exc):
        from animatablegaussians_amd import conv as agc
        agc.set_math(self.prev)


def rel(got, ref):
    """max|got - ref| / max|ref| in float64 (``ref`` a CPU float64 tensor)."""
    got = got.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def oracle_sd(sd, dt):
    return {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}


def filled_avatar():
    """AvatarNet.synthetic with view directions, the three networks filled with three synth.named_fill seeds (equal weights would hide a member
    mix-up; the fill keeps non-zero biases and noise strengths), eval mode (colour style = the fixed buffer) -> (net, items, pose map [3, S, S])."""
    import sys
    import torch
    from animatablegaussians_amd import synth
    from animatablegaussians_amd.avatar import AvatarNet
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_avatar_net_gpu import _items
    torch.manual_seed(31359)
    net = AvatarNet.synthetic({'with_viewdirs': True})
    for name, seed in SEEDS.items():
        sub = getattr(net, name)
        sub.load_reference_state_dict(synth.named_fill(sub.reference_state_dict(), seed=seed))
    net.eval()
    items = _items(net)
    net.get_pose_map(items)
    return net, items, items['smpl_pos_map'][:3].contiguous()


def oracle_net(sd_gpu, style, pose, up, vfs, dt, learn):
    """One network through the oracle on the CPU in ``dt`` -> (images float64, {key: gradient}, pose gradient, (vf1 grad, vf2 grad) or None)."""
    import torch
    from oracle.dual_styleunet_oracle import DualStyleUNetOracle
    sd = {k: v.detach().cpu().to(dt).clone().requires_grad_(k in learn) for k, v in sd_gpu.items()}
    p = pose.detach().cpu().to(dt).requires_grad_(True)
    vs = [v.detach().cpu().to(dt).requires_grad_(True) for v in vfs] if vfs else None
    img = DualStyleUNetOracle(sd).forward(style.detach().cpu().to(dt), p, *(vs or (None, None)))
    (img * up.to(dt)).sum().backward()
    grads = {k: sd[k].grad for k in learn}
    return img.detach().double(), grads, p.grad.double(), ([v.grad.double() for v in vs] if vs else None)


NBLK = 16


def _sub(t, n=256):
    f = t.detach().flatten()
    step = max(1, f.numel() // n)
    return f[::step][:n].double().cpu().clone()          # a copy: a float64 CPU gradient that keeps accumulating must not move the samples


def summary(g):
    """What the comparison reads of one gradient tensor: 256 samples, max |g|, and full-tensor statistics in float64 -- the sum, the sums of
    16 contiguous blocks (dimension 0, output channels, slowest), their sums of magnitudes, the sum of squares."""
    import torch
    g = g.detach().double().flatten()
    n = g.numel()
    edges = [(n * b) // NBLK for b in range(NBLK + 1)]
    blk = torch.stack([g[edges[b]:edges[b + 1]].sum() for b in range(NBLK)]).cpu()
    blkabs = torch.stack([g[edges[b]:edges[b + 1]].abs().sum() for b in range(NBLK)]).cpu()
    return {"sub": _sub(g), "max": float(g.abs().max()), "sum": float(g.sum()), "abs": float(g.abs().sum()), "blk": blk, "blkabs": blkabs,
            "sq": float((g * g).sum()), "n": n}


def deviation(s, ref):
    """(sample deviation / max|ref|, block-sum, sum and square-sum deviations) of summary ``s`` from the float64 oracle's ``ref``."""
    d = float((s["sub"] - ref["sub"]).abs().max()) / max(ref["max"], 1e-30)
    d_sum = abs(s["sum"] - ref["sum"]) / max(ref["abs"], 1e-300)
    d_blk = float(((s["blk"] - ref["blk"]).abs() / ref["blkabs"].clamp_min(1e-300)).max())
    d_sq = abs(s["sq"] - ref["sq"]) / max(ref["sq"], 1e-300)
    return d, d_sum, d_blk, d_sq


# The end-to-end bars (test_styleunet_net.py::_golden_body with the live fp32 oracle as err32) on every parameter gradient of one network
FULL_MULT = 5.0                        # full-tensor statistics: ours within 5x the fp32 oracle's at p50 / p90 / p99
FULL_CAP = {"sum": 1e-2, "blk": 2e-2, "sq": 2e-2}
FULL_CAP_SCALAR = 8e-2                 # one-element tensors (noise strengths): relative error of the number (sq: 2x)
# One named exception to the caps, for the SEEDS above and the upstream gradients of test_styleunet_heads_gpu.py's `avatar` fixture (which
# test_multiview_tail_gpu.py reuses for position_net).  position_net's convs1.11.activate.bias (64 numbers, so a "block" is 4 channels): block 11
# deviates by 1.72e-2 of its magnitude in the fp32 oracle, the fp32 oracle with the comb convolutions re-associated AND the product in split_f16
# -- identical to four digits in three different arithmetics -- 0.93e-2 in the product's fp32 mode, 2.44e-2 in split_bf16 (one network).  The
# channel sums are ill-conditioned (sum|terms| / |sum| up to 1.4e4 in float64); the product's own reduction matches a float64 sum of its own
# pre-activation gradient to 1e-9 of sum|terms|; the deviation is leaky-ReLU slope selections at pre-activations within fp32 rounding of zero,
# each moving the block by a fixed amount: a handful of pixels, not arithmetic error.  Cap for this one statistic: 2x the fp32 oracle's 1.72e-2.
FULL_CAP_NAMED = {("position_net", "convs1.11.activate.bias", "blk"): 3.5e-2}


def check_network_grads(tag, name, grads, learn, s64, e32, named=None):
    """Every parameter gradient ``grads[k]`` (k in ``learn``) of network ``name`` against the float64 oracle's summaries ``s64`` with the fp32
    oracle's deviations ``e32`` as the yardstick: sample deviations at p50..p95 within 3x the oracle's, p99 (noise strengths aside) within 3x,
    per-tensor caps; full-tensor statistics (sum, block sums, square sum) within 5x the oracle's at p50 / p90 / p99 and per-tensor caps.
    ``named``: {parameter key: cap} -- a caller's named exceptions, with their measured evidence written where they are given: the cap replaces
    the per-tensor caps of that tensor (its samples and full-tensor statistics; the square sum 2x).
    Prints the statistics; returns the worst ratio of a measured value to its bar."""
    named = named or {}
    rows, full = [], []
    for k in learn:
        gk = grads[k]
        assert gk is not None, (name, k)
        d, d_sum, d_blk, d_sq = deviation(summary(gk), s64[k])
        r, r_sum, r_blk, r_sq = e32[k]
        rows.append((d, r, k))
        full.append((k, d_sum, r_sum, d_blk, r_blk, d_sq, r_sq, s64[k]["n"]))
    worst = 0.0
    ours, ref = np.array([o for o, _, _ in rows]), np.array([r for _, r, _ in rows])
    print(f"[e2e] {tag} {name}: gradient rows over {len(rows)} tensors, ours / oracle fp32: "
          + " ".join(f"p{q} {np.percentile(ours, q):.2e}/{np.percentile(ref, q):.2e}" for q in (50, 75, 90, 95, 99, 100)))
    for q in (50, 75, 90, 95):
        worst = max(worst, np.percentile(ours, q) / max(3 * np.percentile(ref, q), 1e-300))
        assert np.percentile(ours, q) <= 3 * np.percentile(ref, q), (name, q, np.percentile(ours, q), np.percentile(ref, q))
    tens = [(o, r) for o, r, k in rows if not k.endswith("noise.weight")]
    o99, r99 = np.percentile([o for o, _ in tens], 99), np.percentile([r for _, r in tens], 99)
    worst = max(worst, o99 / max(3 * r99, 1e-300))
    assert o99 <= 3 * r99, (name, o99, r99)
    # per-tensor caps of _golden_body: 1e-2, and 5e-2 for the noise strengths -- except a noise strength on which the fp32 oracle ITSELF
    # misses 5e-2 (a one-number gradient, a sum over a whole map with cancellation): 2x the oracle's own deviation there.  Measured: other_net
    # convs2.11.noise.weight, oracle fp32 0.142 of the value, ours 0.128-0.149 in the three modes on both paths; no other tensor
    for o, r, k in rows:
        cap = 1e-2
        if k.endswith("noise.weight"):
            cap = 2 * r if r > 5e-2 else 5e-2
        cap = named.get(k, cap)
        worst = max(worst, o / cap)
        assert o <= cap, (name, k, o, r)
    fo = {kk: np.array([r[i] for r in full]) for kk, i in (("sum", 1), ("rsum", 2), ("blk", 3), ("rblk", 4), ("sq", 5), ("rsq", 6))}
    print(f"[e2e] {tag} {name}: full-tensor statistics, ours/oracle fp32 at p50 p90 p99 max: "
          + "; ".join(f"{kk}: " + " ".join(f"{np.percentile(fo[kk], q):.1e}/{np.percentile(fo['r' + kk], q):.1e}" for q in (50, 90, 99, 100))
                      for kk in ("sum", "blk", "sq"))
          + " | p99 ratio " + " ".join(f"{kk} {np.percentile(fo[kk], 99) / max(np.percentile(fo['r' + kk], 99), 1e-7):.2f}" for kk in ("sum", "blk", "sq")))
    for kk in ("sum", "blk", "sq"):
        for q in (50, 90, 99):
            lim = FULL_MULT * max(np.percentile(fo["r" + kk], q), 1e-7)
            worst = max(worst, np.percentile(fo[kk], q) / lim)
            assert np.percentile(fo[kk], q) <= lim, (name, kk, q, np.percentile(fo[kk], q), np.percentile(fo["r" + kk], q))
        col = {"sum": 1, "blk": 3, "sq": 5}[kk]
        for r in full:
            cap = (2 * FULL_CAP_SCALAR if kk == "sq" else FULL_CAP_SCALAR) if r[7] == 1 else FULL_CAP[kk]
            cap = FULL_CAP_NAMED.get((name, r[0], kk), cap)
            if r[7] == 1 and r[0].endswith("noise.weight") and r[col + 1] > cap:
                cap = 2 * r[col + 1]          # the noise-strength rule of the rows above: the fp32 oracle itself misses the cap (convs2.11, 0.142)
            if r[0] in named:
                cap = named[r[0]] * (2 if kk == "sq" else 1)
            worst = max(worst, r[col] / cap)
            assert r[col] <= cap, (name, kk, r)
    return worst


def check_maps(maps, ref_maps, err32, tag):
    """Forward maps against the float64 oracle: max|ours - o64| / max|o64| <= 1e-4 each.  Returns the worst ratio to the bar."""
    worst = 0.0
    for name, m in maps:
        ref = ref_maps[name]
        assert tuple(m.shape) == tuple(ref.shape), (name, tuple(m.shape))
        d = rel(m, ref)
        print(f"[e2e] {tag} forward {name}: ours {d:.2e} oracle-fp32 {err32[name]:.2e} (bar 1e-4)")
        worst = max(worst, d / 1e-4)
        assert d <= 1e-4, (tag, name, d)
    return worst


def check_vf_grad(got, ref, what):
    """An ACTIVATION gradient (2 M elements): leaky-ReLU slope flips near zero make isolated elements differ by factors, so relative L2 and the
    fraction of elements off by more than 1e-3 of the largest (the bars of test_grouped_gpu.py::test_three_networks_as_one_chain...).
    Returns the worst ratio to the bars."""
    got = got.detach().double().cpu()
    l2 = float((got - ref).norm() / ref.norm())
    off = float(((got - ref).abs() > 1e-3 * float(ref.abs().max())).double().mean())
    print(f"[e2e] {what}: relative L2 {l2:.2e} (bar 3e-3), fraction off by > 1e-3 of max {off:.2e} (bar 5e-3)")
    assert l2 <= 3e-3 and off <= 5e-3, (what, l2, off)
    return max(l2 / 3e-3, off / 5e-3)
