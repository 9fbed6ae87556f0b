"""``targets.prepare_targets`` / ``boundary_mask`` on the GPU against the numpy restatement of the reference's loader
(``tests/targets_oracle.py``).  Every value check is bit-exact: masks with ``array_equal``, float colour as int32 bit patterns."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

STRUCTURED = to.structured_scenes()


def _check(out, color, matte, k=5):
    """Device items against the oracle's, shapes and dtypes included."""
    want = to.prepare(color, matte, k)
    assert out["color_img"].dtype == torch.float32 and out["mask_img"].dtype == torch.bool and out["boundary_mask_img"].dtype == torch.bool
    for key in ("color_img", "mask_img", "boundary_mask_img"):
        assert out[key].is_cuda and tuple(out[key].shape) == want[key].shape, key
    assert np.array_equal(out["color_img"].cpu().numpy().view(np.int32), want["color_img"].view(np.int32)), "colour bits differ"
    got_m, got_b = out["mask_img"].cpu().numpy(), out["boundary_mask_img"].cpu().numpy()
    assert np.array_equal(got_m, want["mask_img"]), f"mask differs at {np.argwhere(got_m != want['mask_img'])[:5].tolist()}"
    assert np.array_equal(got_b, want["boundary_mask_img"]), f"band differs at {np.argwhere(got_b != want['boundary_mask_img'])[:5].tolist()}"
    return want


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "mask_bbox":
            assert a[key] == b[key]
        else:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape
            x, y = a[key], b[key]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), key


def test_value_table():
    from animatablegaussians_amd.targets import prepare_targets
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    color = np.stack([v, np.roll(v, 85), np.roll(v, 170)], -1)                 # every value in every channel
    out = prepare_targets(color, v, kernel_size=1, bbox=False)
    want32 = np.float32(color / 255.)
    assert np.array_equal(out["color_img"].cpu().numpy().view(np.int32), want32.view(np.int32))
    assert np.array_equal(out["mask_img"].cpu().numpy(), v > 128)
    assert np.array_equal(out["boundary_mask_img"].cpu().numpy(), (v > 5) & (v < 250))
    _check(out, color, v, 1)


@pytest.mark.parametrize("shape", to.SCENE_SHAPES)
def test_random_class_scenes(shape):
    from animatablegaussians_amd.targets import boundary_mask, prepare_targets
    matte, color = to.class_scene(shape, 0), to.color_scene(shape, 0)
    out = prepare_targets(color, matte, bbox=False)
    want = _check(out, color, matte)
    if shape[0] * shape[1] >= 37 * 70:
        b, m = want["boundary_mask_img"].mean(), want["mask_img"].mean()
        assert min(b, 1 - b, m, 1 - m) >= 0.10, (b, m)
    b, m = boundary_mask(matte)
    assert torch.equal(b, out["boundary_mask_img"]) and torch.equal(m, out["mask_img"]) and b.dtype == m.dtype == torch.bool


@pytest.mark.parametrize("name", sorted(STRUCTURED))
def test_structured_scenes(name):
    from animatablegaussians_amd.targets import prepare_targets
    matte = STRUCTURED[name]
    color = to.color_scene(matte.shape, 3)
    want = _check(prepare_targets(color, matte, bbox=False), color, matte)
    band, mask = want["boundary_mask_img"], want["mask_img"]
    if name in ("all_255", "all_0"):
        assert not band.any() and mask.all() == (name == "all_255")            # the border convention: outside pixels take no part
    elif name.startswith("pixel_"):
        assert mask.sum() == 1 and band.sum() == (9 if "corner" in name else 25)
    else:
        assert band.any() and mask.any() and not band.all() and not mask.all()


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 15])
def test_kernel_sizes(k):
    from animatablegaussians_amd.targets import prepare_targets
    matte, color = to.class_scene((37, 70), 0), to.color_scene((37, 70), 0)
    _check(prepare_targets(color, matte, kernel_size=k, bbox=False), color, matte, k)


def test_batched_equals_single_calls():
    """V = 3 at 19 x 131: H W is odd, so the second view's planes start at an odd address."""
    from animatablegaussians_amd.targets import prepare_targets
    matte = np.stack([to.class_scene((19, 131), s) for s in range(3)])
    color = np.stack([to.color_scene((19, 131), s) for s in range(3)])
    matte[:, 9, 60] = 255                                                      # no view is empty
    out = prepare_targets(color, matte)
    _check(out, color, matte)
    assert isinstance(out["mask_bbox"], list) and len(out["mask_bbox"]) == 3
    for v in range(3):
        one = prepare_targets(color[v], matte[v])
        _same(one, {k: out[k][v] for k in out})


@pytest.mark.parametrize("shape", [(19, 131), (5, 7)])
def test_abi_writes_nothing_outside_its_outputs(shape):
    """Every buffer of the call sits at an odd offset inside a larger one filled with a sentinel; the bytes around the outputs stay."""
    from animatablegaussians_amd import _lib
    V, (H, W) = 2, shape
    n = V * H * W
    matte = np.stack([to.class_scene(shape, 5 + v) for v in range(V)])
    color = np.stack([to.color_scene(shape, 5 + v) for v in range(V)])
    want = to.prepare(color, matte, 5)
    PAD, S = 64, 0xA5
    dev = torch.device("cuda")

    def framed(nbytes, off):
        return torch.full((PAD + off + nbytes + PAD,), S, dtype=torch.uint8, device=dev), PAD + off

    bufs = {"color": framed(3 * n, 3), "matte": framed(n, 1), "color_f": framed(12 * n, 4), "mask": framed(n, 5), "boundary": framed(n, 7),
            "rows": framed(V * H, 2), "cols": framed(V * W, 3)}
    for key, src in (("color", color), ("matte", matte)):
        t, o = bufs[key]
        t[o:o + src.size] = torch.from_numpy(src.reshape(-1)).to(dev)
    p = {k: ctypes.c_void_p(t.data_ptr() + o) for k, (t, o) in bufs.items()}
    assert (bufs["color_f"][0].data_ptr() + bufs["color_f"][1]) % 16 == 4 and p["mask"].value % 2 == 1 and p["boundary"].value % 2 == 1
    _lib.check(_lib.lib().ag_prepare_targets(p["color"], p["matte"], V, H, W, 5, p["color_f"], p["mask"], p["boundary"], p["rows"], p["cols"],
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ag_prepare_targets")
    host = {k: t.cpu().numpy() for k, (t, o) in bufs.items()}
    sizes = {"color": 3 * n, "matte": n, "color_f": 12 * n, "mask": n, "boundary": n, "rows": V * H, "cols": V * W}
    for k, nbytes in sizes.items():
        o = bufs[k][1]
        assert (host[k][:o] == S).all() and (host[k][o + nbytes:] == S).all(), f"bytes around {k} changed"
    body = lambda k: host[k][bufs[k][1]:bufs[k][1] + sizes[k]]  # noqa: E731
    assert np.array_equal(body("color"), color.reshape(-1)) and np.array_equal(body("matte"), matte.reshape(-1))
    assert np.array_equal(body("color_f").view(np.int32), want["color_img"].reshape(-1).view(np.int32))
    assert np.array_equal(body("mask"), want["mask_img"].reshape(-1).astype(np.uint8))
    assert np.array_equal(body("boundary"), want["boundary_mask_img"].reshape(-1).astype(np.uint8))
    assert np.array_equal(body("rows"), want["mask_img"].any(2).reshape(-1).astype(np.uint8))
    assert np.array_equal(body("cols"), want["mask_img"].any(1).reshape(-1).astype(np.uint8))


def _bbox_mattes():
    edges = np.zeros((45, 150), np.uint8)
    edges[0, 70], edges[44, 3], edges[20, 0], edges[7, 149] = 255, 200, 129, 255
    single = np.zeros((45, 150), np.uint8)
    single[31, 137] = 255
    blob = np.zeros((45, 150), np.uint8)
    blob[10:30, 40:135] = 255
    blob[5, 60] = 128                                                          # not in the mask: does not move the box
    return {"edges": edges, "single": single, "blob": blob}


@pytest.mark.parametrize("name", ["edges", "single", "blob"])
def test_mask_bbox_equals_the_host_function(name):
    from animatablegaussians_amd import losses
    from animatablegaussians_amd.targets import prepare_targets
    matte = _bbox_mattes()[name]
    out = prepare_targets(to.color_scene(matte.shape, 1), matte)
    want = losses.mask_bbox(to.get_boundary_mask(matte)[1])
    assert isinstance(out["mask_bbox"], tuple) and out["mask_bbox"] == want
    if name == "edges":
        assert want == (0, 0, 44, 149)


def test_mask_bbox_empty_raises_and_bbox_false_has_no_key():
    from animatablegaussians_amd.targets import prepare_targets
    m = _bbox_mattes()
    color = to.color_scene((45, 150), 1)
    empty = np.full((45, 150), 128, np.uint8)
    with pytest.raises(ValueError, match="view 0"):
        prepare_targets(color, empty)
    with pytest.raises(ValueError, match="view 1"):
        prepare_targets(np.stack([color, color]), np.stack([m["blob"], empty]))
    out = prepare_targets(color, empty, bbox=False)
    assert set(out) == {"color_img", "mask_img", "boundary_mask_img"} and not out["mask_img"].any()


def test_input_forms_and_stream():
    from animatablegaussians_amd.targets import prepare_targets
    matte, color = to.class_scene((37, 70), 2), to.color_scene((37, 70), 2)
    matte[20, 30] = 255
    base = prepare_targets(color, matte)
    _check(base, color, matte)
    tc, tm = torch.from_numpy(color), torch.from_numpy(matte)
    _same(base, prepare_targets(tc, tm))
    _same(base, prepare_targets(tc.pin_memory(), tm.pin_memory()))
    _same(base, prepare_targets(tc.cuda(), tm.cuda()))
    _same(base, prepare_targets(tc.cuda(), matte))                             # one on the device, one on the host
    wide_c = torch.zeros(37, 140, 3, dtype=torch.uint8)
    wide_m = torch.zeros(37, 140, dtype=torch.uint8)
    wide_c[:, ::2], wide_m[:, ::2] = tc, tm
    for dev in ("cpu", "cuda"):
        sc, sm = wide_c.to(dev)[:, ::2], wide_m.to(dev)[:, ::2]
        assert not sc.is_contiguous() and not sm.is_contiguous()
        _same(base, prepare_targets(sc, sm))
    _same(base, prepare_targets(np.asfortranarray(color), np.asfortranarray(matte)))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = prepare_targets(color, matte)
    side.synchronize()
    _same(base, on_side)


def test_training_loss_takes_the_items_as_they_are():
    """losses.training_loss on device-prepared items and on the oracle's items uploaded from the host: the same bits."""
    from animatablegaussians_amd import losses
    from animatablegaussians_amd.targets import prepare_targets
    H, W = 48, 64
    matte = to.disc_scene(48, 14.0, 3.0)
    matte = np.concatenate([matte, np.zeros((48, 16), np.uint8)], 1)
    color = to.color_scene((H, W), 4)
    g = torch.Generator().manual_seed(0)
    render = {"rgb_map": torch.rand(H, W, 3, generator=g).cuda(), "mask_map": torch.rand(H, W, 1, generator=g).cuda(),
              "offset": (0.01 * torch.randn(500, 3, generator=g)).cuda()}
    bg = torch.tensor([1., 1., 1.], device="cuda")
    weights = {"l1": 1.0, "mask": 0.1, "offset": 0.005}
    ours = prepare_targets(color, matte)
    ref = {k: torch.from_numpy(v).cuda() for k, v in to.prepare(color, matte).items()}
    ref["mask_bbox"] = losses.mask_bbox(ref["mask_img"].cpu().numpy())
    assert ours["mask_bbox"] == ref["mask_bbox"]
    la, pa = losses.training_loss(render, ours, bg, weights, lpips=None)
    lb, pb = losses.training_loss(render, ref, bg, weights, lpips=None)
    assert pa.keys() == pb.keys() == {"l1_loss", "mask_loss", "offset_loss"}
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and float(la) > 0
    for k in pa:
        assert torch.equal(pa[k].view(torch.int32), pb[k].view(torch.int32)), k
