"""``ray_select`` on the GPU against the numpy float32 restatement of ``tests/ray_select_oracle.py`` (which ``test_ray_select_cpu.py`` ties
to the reference's own outputs).  Every value check is exact: integers and flags with ``array_equal``, float32 as int32 bit patterns.
Frames from 1 x 1 to 130 x 257 (tails below one wave, across a wave, a workgroup and a compaction run of 512), three cameras, four
mattes; pixel lists of 0, 1, 63, 64, 65 and 1025 entries."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_select_oracle as ro  # noqa: E402
import template_field_oracle as tfo  # noqa: E402
import template_render_grad_oracle as tgo  # noqa: E402

pytestmark = pytest.mark.gpu
BATCH = ("uv", "ray_o", "ray_d", "near", "far", "color_gt", "mask_gt", "depth_gt", "dist")
PATCH = BATCH + ("mask_within_patch",)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _equal(name, got, want):
    """Exact: float32 by bit pattern, everything else by value; shapes and the kind of dtype included."""
    g, w = _np(got), np.asarray(want)
    assert g.shape == w.shape, f"{name}: shape {g.shape}, expected {w.shape}"
    if w.dtype.kind == "f":
        assert g.dtype == np.float32 and w.dtype == np.float32, (name, g.dtype, w.dtype)
        bad = g.view(np.int32) != w.view(np.int32)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} float32 values differ in their bits, first at {np.argwhere(bad)[0].tolist()}"
    else:
        assert g.dtype.kind == w.dtype.kind or {g.dtype.kind, w.dtype.kind} <= {"i", "u"}, (name, g.dtype, w.dtype)
        assert np.array_equal(g, w), f"{name}: differs at {np.argwhere(g != w)[:5].tolist()}"


def _same(a, b):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            x, y = a[k], b[k]
            assert x.dtype == y.dtype and x.shape == y.shape, k
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), f"{k}: two calls differ"
        else:
            assert a[k] == b[k], k


@functools.lru_cache(maxsize=None)
def _device_images(H, W, matte="blob"):
    return tuple(None if a is None else _t(a) for a in ro.scene_images(H, W, matte))


@functools.lru_cache(maxsize=None)
def _oracle_frame(cam, H, W):
    """The float32 oracle over all pixels of a scene with the blob images -- built once, never modified."""
    extr, intr = ro.scene_camera(cam, H, W)
    color, mask, depth, _ = ro.scene_images(H, W)
    return ro.build(None, extr, intr, ro.BOX, H, W, color, mask, depth, ro.F32)


# ---- 1. classify + compaction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ro.FRAMES)
def test_bound_mask_and_candidate_lists(H, W):
    import torch
    from animatablegaussians_amd import ray_select as rs
    for cam in ro.CAMERAS:
        extr, intr = ro.scene_camera(cam, H, W)
        _equal(f"{cam} bound_mask", rs.bound_mask(ro.BOX, intr, extr, H, W), ro.bound_mask(ro.BOX, intr, extr, H, W))
        for matte in ro.MATTES:
            _, mask, _, unsample = ro.scene_images(H, W, matte)
            inside, outside, bound = ro.candidates(mask, ro.BOX, extr, intr, unsample)
            _, dmask, _, dunsample = _device_images(H, W, matte)
            c = rs.candidates(dmask, ro.BOX, extr, intr, dunsample)
            tag = f"{H} x {W} {cam} {matte}"
            assert c.inside.dtype == c.outside.dtype == c.counts.dtype == torch.int32 and c.bound_mask.dtype == torch.bool
            _equal(f"{tag} inside", c.inside, inside)
            _equal(f"{tag} outside", c.outside, outside)
            _equal(f"{tag} bound_mask", c.bound_mask, bound)
            assert c.counts.tolist() == [len(inside), len(outside)] and (c.H, c.W) == (H, W)
            if matte == "all_false":
                assert len(inside) == 0 and c.inside.numel() == 0
            if matte == "blob" and H >= 37:
                u8 = rs.candidates(dmask.to(torch.uint8) * 200, ro.BOX, extr, intr)        # a uint8 matte: non-zero is the subject
                _same({"i": u8.inside, "o": u8.outside, "b": u8.bound_mask}, {"i": c.inside, "o": c.outside, "b": c.bound_mask})
    extr, intr = ro.scene_camera("axis", H, W)
    moved = ro.BOX + np.float32([40, 0, 0])                                                # off the frame: both lists empty
    c = rs.candidates(_device_images(H, W)[1], moved, extr, intr)
    assert c.inside.numel() == 0 and c.outside.numel() == 0 and c.counts.tolist() == [0, 0] and not c.bound_mask.any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 1025, 130 * 257])
def test_compaction_of_a_flag_array(n):
    """The routine alone on random classes 0 / 1 / 2 / 3 (3 belongs to no list), with and without the second list."""
    from animatablegaussians_amd import ray_select as rs
    flags = np.random.RandomState(n).randint(0, 4, n).astype(np.uint8)
    one, two, counts = rs._compact(_t(flags), True)
    want1, want2 = np.flatnonzero(flags == 1), np.flatnonzero(flags == 2)
    assert counts.tolist() == [len(want1), len(want2)] and one.numel() == two.numel() == n
    _equal("list1", one[:len(want1)], want1.astype(np.int32))
    _equal("list2", two[:len(want2)], want2.astype(np.int32))
    one_b, none, counts_b = rs._compact(_t(flags), False)
    assert none is None and counts_b.tolist() == [len(want1), 0]
    _equal("list1 alone", one_b[:len(want1)], want1.astype(np.int32))


# ---- 2. build -------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("uv", "ray_o", "ray_d", "near", "far", "hit", "color_gt", "mask_gt", "depth_gt", "dist")


@pytest.mark.parametrize("H,W", ro.FRAMES)
def test_build_over_all_pixels(H, W):
    from animatablegaussians_amd import ray_select as rs
    color, mask, depth, _ = _device_images(H, W)
    for cam in ro.CAMERAS:
        extr, intr = ro.scene_camera(cam, H, W)
        want = _oracle_frame(cam, H, W)
        got = rs._build(rs._camera(extr, intr, ro.BOX, H, W), H * W, color.device, images=(color, mask, depth))
        for k in FIELDS:
            _equal(f"{H} x {W} {cam} {k}", got[k], want[k].astype(np.uint8) if k == "hit" else want[k])
        no_depth = rs._build(rs._camera(extr, intr, ro.BOX, H, W), H * W, color.device, images=(color, mask, None))
        assert not no_depth["depth_gt"].any() and not no_depth["dist"].any()
        _equal("color_gt without depth", no_depth["color_gt"], want["color_gt"])
        # the public pieces: get_rays on explicit coordinates, get_near_far on rays the caller holds, image_rays
        ray_d, ray_o = rs.get_rays(_t(want["uv"]), extr, intr)
        _equal("get_rays ray_d", ray_d, want["ray_d"])
        _equal("get_rays ray_o", ray_o, want["ray_o"])
        near, far, at_box = rs.get_near_far(ro.BOX, ray_o, ray_d)
        hit = want["hit"]
        _equal("get_near_far mask", at_box, hit)
        _equal("get_near_far near", near, want["near"][hit])
        _equal("get_near_far far", far, want["far"][hit])
        rays = rs.image_rays(extr, intr, W, H, ro.BOX)
        for k in ("uv", "ray_o", "ray_d", "near", "far"):
            _equal(f"image_rays {k}", rays[k], want[k][hit])
        assert not rays["dist"].any() and rays["dist"].shape == rays["near"].shape and (rays["img_w"], rays["img_h"]) == (W, H)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_build_over_a_pixel_list(n):
    from animatablegaussians_amd import ray_select as rs
    H, W = 130, 257
    color, mask, depth, _ = _device_images(H, W)
    extr, intr = ro.scene_camera("tilted", H, W)
    pix = np.random.RandomState(n).randint(0, H * W, n).astype(np.int32)                   # unordered, with repeats
    want_all = _oracle_frame("tilted", H, W)
    got = rs._build(rs._camera(extr, intr, ro.BOX, H, W), n, color.device, pix=_t(pix), images=(color, mask, depth))
    for k in FIELDS:
        w = want_all[k][pix]
        _equal(f"n = {n} {k}", got[k], w.astype(np.uint8) if k == "hit" else w)
    if n == 65:                                                                            # entries outside the frame: a miss, all zeros
        pix[[3, 40]] = [-1, H * W]
        got = rs._build(rs._camera(extr, intr, ro.BOX, H, W), n, color.device, pix=_t(pix), images=(color, mask, depth))
        ok = (pix >= 0) & (pix < H * W)
        for k in FIELDS:
            g = _np(got[k])
            assert not g[~ok].any(), k
            w = want_all[k][pix[ok]]
            _equal(f"beside an entry off the frame: {k}", got[k][_t(ok)], w.astype(np.uint8) if k == "hit" else w)


# ---- 3. sample_randomly -------------------------------------------------------------------------------------------------------------------
RANDOM = [("tilted", 37, 70, "blob", 128, 0.5, True), ("tilted", 48, 64, "band", 200, 0.7, True), ("axis", 64, 65, "band", 96, 0.3, False),
          ("close", 130, 257, "blob", 1024, 0.5, False), ("close", 5, 3, "blob", 4, 0.5, False)]


@pytest.mark.parametrize("cam,H,W,matte,num,ratio,force", RANDOM)
def test_sample_randomly_with_picks_equals_the_oracle(cam, H, W, matte, num, ratio, force):
    from animatablegaussians_amd import ray_select as rs
    extr, intr = ro.scene_camera(cam, H, W)
    missing = ro.missing_bound_pixels(cam, H, W)[:2] if force else ()
    picks = ro.make_picks(cam, H, W, matte, num, ratio, seed=H + W, force=missing)
    color, mask, depth, unsample = ro.scene_images(H, W, matte)
    want = ro.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, unsample, picks, ro.F32)
    if force:
        assert len(missing) == 2 and want["rounds"] >= 2, "the forced misses must cause a second round"
    dev = _device_images(H, W, matte)
    got = rs.sample_randomly(dev[0], dev[1], dev[2], extr, intr, ro.BOX, num, ratio, dev[3], picks=picks)
    assert set(got) == set(BATCH) and got["uv"].shape == (num, 2), "exactly sample_num rays"
    for k in BATCH:
        _equal(f"{cam} {H} x {W} {k}", got[k], want[k])
    _same(got, rs.sample_randomly(dev[0], dev[1], dev[2], extr, intr, ro.BOX, num, ratio, dev[3], picks=picks))
    if depth is not None and cam == "close":
        no_depth = rs.sample_randomly(dev[0], dev[1], None, extr, intr, ro.BOX, num, ratio, dev[3], picks=picks)
        assert not no_depth["depth_gt"].any() and not no_depth["dist"].any()


@pytest.mark.parametrize("where", ["cpu", "cuda", None])
def test_sample_randomly_with_a_generator(where):
    import torch
    from animatablegaussians_amd import ray_select as rs
    for cam, H, W, num, ratio in (("close", 37, 70, 300, 0.4), ("tilted", 37, 70, 500, 0.5)):
        extr, intr = ro.scene_camera(cam, H, W)
        color, mask, depth, _ = _device_images(H, W)
        if where is None:
            a = rs.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio)
        else:
            a = rs.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, generator=torch.Generator(device=where).manual_seed(5))
            _same(a, rs.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, generator=torch.Generator(device=where).manual_seed(5)))
            b = rs.sample_randomly(color, mask, depth, extr, intr, ro.BOX, num, ratio, generator=torch.Generator(device=where).manual_seed(6))
            assert not torch.equal(a["uv"], b["uv"]), "another seed draws other pixels"
        assert a["uv"].shape == (num, 2)
        inside, outside, _ = ro.candidates(ro.scene_images(H, W)[1], ro.BOX, extr, intr)
        uv = _np(a["uv"]).astype(np.int64)
        pix = uv[:, 1] * W + uv[:, 0]
        want = _oracle_frame(cam, H, W)
        assert want["hit"][pix].all(), "every ray of the batch hits the box"
        for k in BATCH:                                                                    # whatever was drawn, the values are the oracle's
            _equal(f"{cam} {k}", a[k], want[k][pix])
        if cam == "close":                                                                 # every pixel of this mask hits: one round
            k_in = int(num * ratio)
            assert len(np.unique(pix)) == num, "a round draws without replacement"
            assert np.isin(pix[:k_in], inside).all() and np.isin(pix[k_in:], outside).all(), "the inside share is int(rest * ratio)"
        else:
            assert np.isin(pix, np.concatenate([inside, outside])).all()


# ---- 4. sample_patches --------------------------------------------------------------------------------------------------------------------
def _border_picks(inside, outside, W):
    """(use_inside, index) of the candidate nearest to the left, right, top and bottom border, from whichever list holds it."""
    picks = []
    for key, sign in (("x", 1), ("x", -1), ("y", 1), ("y", -1)):
        best = []
        for use_inside, lst in ((True, inside), (False, outside)):
            coord = sign * (lst % W if key == "x" else lst // W)
            if len(lst):
                best.append((int(coord.min()), not use_inside, use_inside, int(np.argmin(coord))))
        picks.append(min(best)[2:])
    return picks


@pytest.mark.parametrize("cam,H,W,matte,ps", [("cover", 37, 70, "blob", 16), ("close", 37, 70, "blob", 16), ("close", 37, 70, "band", 32), ("tilted", 48, 64, "blob", 8),
                                              ("close", 130, 257, "blob", 32), ("tilted", 48, 64, "blob", 48)])
def test_sample_patches_with_picks_equals_the_oracle(cam, H, W, matte, ps):
    import torch
    from animatablegaussians_amd import ray_select as rs
    from animatablegaussians_amd.template_render import render_train, training_loss
    extr, intr = ro.scene_camera(cam, H, W)
    color, mask, depth, unsample = ro.scene_images(H, W, matte)
    inside, outside, _ = ro.candidates(mask, ro.BOX, extr, intr, unsample)
    picks = _border_picks(inside, outside, W)
    if cam == "cover":                                                                     # the box fills the frame: a centre on each border
        centres = [int((inside if u else outside)[i]) for u, i in picks]
        assert centres[0] % W == 0 and centres[1] % W == W - 1 and centres[2] // W == 0 and centres[3] // W == H - 1, "the patches must clip"
        assert {True, False} == {u for u, _ in picks}, "centres from both lists"
    want = ro.sample_patches(color, mask, depth, extr, intr, ro.BOX, 4, ps, unsample, picks, ro.F32)
    dev = _device_images(H, W, matte)
    got = rs.sample_patches(dev[0], dev[1], dev[2], extr, intr, ro.BOX, 4, ps, 0.5, dev[3], picks=picks)
    assert set(got) == set(PATCH) and got["uv"].shape == (4 * ps * ps, 2) and got["mask_within_patch"].dtype == torch.bool
    for k in PATCH:
        _equal(f"{cam} {H} x {W} ps = {ps} {k}", got[k], want[k])
    R = int(got["mask_within_patch"].sum())
    assert R == got["ray_o"].shape[0] == got["dist"].shape[0] and 0 < R and (R < 4 * ps * ps or cam == "cover")
    _same(got, rs.sample_patches(dev[0], dev[1], dev[2], extr, intr, ro.BOX, 4, ps, 0.5, dev[3], picks=picks))
    if ps == 8:                                                                            # the batch feeds the training path as it is
        params = {k: _t(v).requires_grad_(True) for k, v in tgo.tiny_net(seed=1).items()}
        beta = torch.tensor([0.01], device="cuda", requires_grad=True)
        out = render_train(lambda p, v: tgo.tiny_field(params, p, v), beta, got["ray_o"], got["ray_d"], got["near"], got["far"], space="cano",
                           sampling="uniform", mask_within_patch=got["mask_within_patch"])
        assert out["rgb_map"].shape == (4 * ps * ps, 3) and out["acc_map"].shape == (4 * ps * ps,)
        loss, terms = training_loss(out, got["color_gt"], got["mask_gt"], {"color": 1.0, "mask": 0.5})
        loss.backward()
        assert set(terms) == {"color_loss", "mask_loss"} and np.isfinite(float(loss.detach())) and all(p.grad is not None for p in params.values())


def test_sample_patches_with_a_generator():
    import torch
    from animatablegaussians_amd import ray_select as rs
    H, W, ps = 48, 64, 8
    extr, intr = ro.scene_camera("tilted", H, W)
    color, mask, depth, _ = _device_images(H, W)
    want = _oracle_frame("tilted", H, W)
    bound = ro.bound_mask(ro.BOX, intr, extr, H, W).reshape(-1)
    for where in ("cpu", "cuda"):
        a = rs.sample_patches(color, mask, depth, extr, intr, ro.BOX, 3, ps, generator=torch.Generator(device=where).manual_seed(2))
        _same(a, rs.sample_patches(color, mask, depth, extr, intr, ro.BOX, 3, ps, generator=torch.Generator(device=where).manual_seed(2)))
        uv = _np(a["uv"]).astype(np.int64).reshape(3, ps, ps, 2)
        assert (np.diff(uv[..., 0], axis=2) == 1).all() and (np.diff(uv[..., 1], axis=1) == 1).all(), "row-major patches"
        assert uv[..., 0].min() >= 0 and uv[..., 0].max() < W and uv[..., 1].min() >= 0 and uv[..., 1].max() < H
        pix = (uv[..., 1] * W + uv[..., 0]).reshape(-1)
        within = bound[pix] & want["hit"][pix]
        _equal("mask_within_patch", a["mask_within_patch"], within)
        for k in ("color_gt", "mask_gt", "depth_gt"):
            _equal(k, a[k], want[k][pix])
        for k in ("ray_o", "ray_d", "near", "far", "dist"):
            _equal(k, a[k], want[k][pix][within])


# ---- 5. image_rays + render_image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_render_image_equals_render_on_the_same_rays(white):
    import torch
    from animatablegaussians_amd import ray_select as rs
    from animatablegaussians_amd.template_field import TemplateField
    from animatablegaussians_amd.template_render import render
    H, W = 48, 64
    net = tfo.make_net(tfo.NARROW, 4, use_viewdir=True)
    arch = net["arch"]
    field = TemplateField.from_state_dict(tfo.state_dict(net), multires=arch["multires"], use_viewdir=net["use_viewdir"],
                                          multires_viewdir=arch["multires_viewdir"], geo_activation=net["geo_activation"])
    extr, intr = ro.scene_camera("tilted", H, W)
    rays = rs.image_rays(extr, intr, W, H, ro.BOX)
    hit = _oracle_frame("tilted", H, W)["hit"]
    assert rays["uv"].shape[0] == int(hit.sum()) and 0 < hit.sum() < H * W
    direct = render(field, rays["ray_o"], rays["ray_d"], rays["near"], rays["far"], sampling="uniform", white_bkgd=white)
    img = rs.render_image(field, extr, intr, W, H, ro.BOX, sampling="uniform", white_bkgd=white)
    assert img["rgb"].shape == (H, W, 3) and img["acc"].shape == (H, W)
    rgb = torch.full((H * W, 3), 1.0 if white else 0.0, device="cuda")
    acc = torch.zeros(H * W, device="cuda")
    at = _t(np.flatnonzero(hit))
    rgb[at], acc[at] = direct["rgb_map"], direct["acc_map"]
    assert torch.equal(img["rgb"].view(torch.int32), rgb.view(H, W, 3).view(torch.int32)), "rgb differs from render on the same rays"
    assert torch.equal(img["acc"].view(torch.int32), acc.view(H, W).view(torch.int32))
    off = _t(~hit.reshape(H, W))
    assert (img["rgb"][off] == (1.0 if white else 0.0)).all() and not img["acc"][off].any(), "background where no ray exists"
    print(f"white = {white}: {int(hit.sum())} rays, acc up to {float(img['acc'].max()):.3f}")
    _same({k: img[k] for k in ("rgb", "acc")}, {k: v for k, v in rs.render_image(field, extr, intr, W, H, ro.BOX, sampling="uniform", white_bkgd=white).items()
                                               if k in ("rgb", "acc")})
    with pytest.raises(ValueError, match="want"):
        rs.render_image(field, extr, intr, W, H, ro.BOX, sampling="uniform", want=("acc_map",))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_value_error():
    import torch
    from animatablegaussians_amd import ray_select as rs
    H, W = 37, 70
    extr, intr = ro.scene_camera("tilted", H, W)
    color, mask, depth, _ = _device_images(H, W)
    behind = extr.copy()
    behind[2, 3] = 0.2
    inside, outside, _ = ro.candidates(ro.scene_images(H, W)[1], ro.BOX, extr, intr)
    args = (extr, intr, ro.BOX)
    cases = {
        "host color": lambda: rs.sample_randomly(color.cpu(), mask, depth, *args),
        "host mask": lambda: rs.sample_patches(color, mask.cpu(), depth, *args),
        "host unsample": lambda: rs.candidates(mask, ro.BOX, extr, intr, mask.cpu()),
        "color dtype": lambda: rs.sample_randomly(color.double(), mask, depth, *args),
        "mask dtype": lambda: rs.candidates(mask.float(), ro.BOX, extr, intr),
        "depth dtype": lambda: rs.sample_patches(color, mask, depth.half(), *args),
        "color shape": lambda: rs.sample_randomly(color[:, :, :2], mask, depth, *args),
        "mask shape": lambda: rs.sample_randomly(color, mask[:, :-1], depth, *args),
        "depth shape": lambda: rs.sample_randomly(color, mask, depth[None], *args),
        "unsample shape": lambda: rs.candidates(mask, ro.BOX, extr, intr, mask[:-1]),
        "uv dtype": lambda: rs.get_rays(torch.zeros(4, 2, device="cuda"), extr, intr),
        "uv shape": lambda: rs.get_rays(torch.zeros(4, 3, dtype=torch.int32, device="cuda"), extr, intr),
        "ray shapes": lambda: rs.get_near_far(ro.BOX, torch.zeros(4, 3, device="cuda"), torch.zeros(5, 3, device="cuda")),
        "behind, random": lambda: rs.sample_randomly(color, mask, depth, behind, intr, ro.BOX),
        "behind, patches": lambda: rs.sample_patches(color, mask, depth, behind, intr, ro.BOX),
        "behind, candidates": lambda: rs.candidates(mask, ro.BOX, behind, intr),
        "more than the inside list holds": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=2 * len(inside) + 2),
        "more than the outside list holds": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=len(outside) + 1, inside_ratio=0.0),
        "pick beyond the list": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=4, picks=[([0, len(inside)], [0, 1])]),
        "pick twice": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=4, picks=[([3, 3], [0, 1])]),
        "pick count": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=4, picks=[([0, 1, 2], [0])]),
        "picks run out": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=4, picks=[]),
        "ratio": lambda: rs.sample_randomly(color, mask, depth, *args, inside_ratio=1.5),
        "sample_num": lambda: rs.sample_randomly(color, mask, depth, *args, sample_num=0),
        "patch larger than the frame": lambda: rs.sample_patches(color, mask, depth, *args, patch_size=38),
        "resize_factor": lambda: rs.sample_patches(color, mask, depth, *args, resize_factor=0.5),
        "patch index": lambda: rs.sample_patches(color, mask, depth, *args, patch_num=1, patch_size=8, picks=[(True, len(inside))]),
        "too few patch picks": lambda: rs.sample_patches(color, mask, depth, *args, patch_num=2, patch_size=8, picks=[(True, 0)]),
    }
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: not refused")
    empty = torch.zeros_like(mask)
    with pytest.raises(ValueError, match="empty"):
        rs.sample_patches(color, empty, depth, *args, patch_num=1, patch_size=8, picks=[(True, 0)])


# ---- 7. two calls -----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    from animatablegaussians_amd import ray_select as rs
    H, W = 130, 257
    extr, intr = ro.scene_camera("tilted", H, W)
    color, mask, depth, unsample = _device_images(H, W, "band")
    for call in (lambda: {"m": rs.bound_mask(ro.BOX, intr, extr, H, W)},
                 lambda: (lambda c: {"i": c.inside, "o": c.outside, "b": c.bound_mask, "n": c.counts})(rs.candidates(mask, ro.BOX, extr, intr, unsample)),
                 lambda: rs.image_rays(extr, intr, W, H, ro.BOX),
                 lambda: dict(zip("do", rs.get_rays(_t(_oracle_frame("tilted", H, W)["uv"]), extr, intr))),
                 lambda: dict(zip("nfm", rs.get_near_far(ro.BOX, _t(_oracle_frame("tilted", H, W)["ray_o"]), _t(_oracle_frame("tilted", H, W)["ray_d"]))))):
        _same(call(), call())
