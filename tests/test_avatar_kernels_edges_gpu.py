"""The kernels of csrc/ag_avatar.hip -- map gather + activations, linear-blend skinning forward and backward, the joint-matrix gradient, hand fusion -- against
the float64 references of tests/avatar_kernels_oracle.py, at the shapes and values no other test runs them at: the front|back seam and the last canvas pixel,
N = 1 and N off a multiple of 256, the eps branch of the normalize backward, saturated logits, ragged and empty waves of the skinning, even J, J = 1 and J at
the LDS limits, unnormalised and all-zero weight rows, sparse joint indices up to 255, every arg-max candidate of matrix_to_quaternion, and the hand-fusion
rows on the centre line, between overlapping boxes and beyond the range of the fast exponential.

The bar is that of tests/test_pose_grad_gpu.py (4 x the float32 oracle's own deviation from float64 + 2e-6 of the float64 scale, max and L2 norm), per output
tensor and per case; hand fusion (the kernel uses the fast exponential) is held to rtol 1e-5 + atol 2e-6 of tests/test_avatar_gpu.py, against float64.  Every
test prints its worst ratio on a [parity] line.  tests/test_avatar_kernels_oracle_cpu.py asserts that each case reaches what it is here for."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avatar_kernels_oracle as ako  # noqa: E402

pytestmark = pytest.mark.gpu


def _cuda(t, grad=False):
    return t.detach().cuda().requires_grad_(grad)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# gather + activations
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _gather_gpu(d):
    """The fused call and its backward: (outputs, gradient maps, pix)."""
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    maps = [_cuda(d[k], True) for k in ("position_map", "other_map", "color_map")]
    pix = ops.mask_to_pix(d["mask"].cuda())
    raws = [_cuda(d[k]) for k in ("xyz", "opacity_raw", "scaling_raw", "rotation_raw")]
    outs = ops.gather_activate(*maps, pix, *raws)
    torch.autograd.backward(list(outs), [u.cuda() for u in d["ups"]])
    return outs, [m.grad for m in maps], pix, raws


def _check_gather(name):
    """Forward outputs and gradient maps of one case against the bar (zero-quaternion rows and the channel groups of the other map on their own), the
    gradient maps exactly 0 off the mask.  Returns the worst ratio."""
    import torch
    d = ako.gather_case(name)
    (o64, g64), (o32, g32) = ako.gather_reference(name)
    outs, grads, _, _ = _gather_gpu(d)
    z, mask = d["zero_rows"], d["mask"]
    floor = ako.SUBNORMAL_FLOOR if d["kind"] in ("opacity_neg", "scale_small") else 0.0
    worst = 0.0
    for what, got, a, b in zip(ako.GATHER_OUTPUTS, outs, o64, o32):
        got = got.detach().cpu()
        if what == "rotations" and bool(z.any()):
            assert bool((got[z] == 0).all()), f"{name}: a zero quaternion is not normalised to exactly 0"
            got, a, b = got[~z], a[~z], b[~z]
        worst = max(worst, ako.bar(got, a, b, f"{name}: {what}", floor))
    for (what, C, groups), got, a, b in zip(ako.GRAD_GROUPS, grads, g64, g32):
        rows, off = ako.canvas_rows(got.cpu(), C, mask)
        assert bool((off == 0).all()), f"{name}: dL/d{what} is not exactly 0 off the mask"
        ra, rb = ako.canvas_rows(a, C, mask)[0], ako.canvas_rows(b, C, mask)[0]
        for lo, hi, group in groups:
            every = torch.ones_like(z)
            sets = [(every, "")] if group != "rotations" or not bool(z.any()) else [(~z, ""), (z, " (zero-quaternion rows: g * 1e12)")]
            for sel, tag in sets:
                worst = max(worst, ako.bar(rows[sel, lo:hi], ra[sel, lo:hi], rb[sel, lo:hi], f"{name}: dL/d{what}[{group}]{tag}", floor))
    return worst


@pytest.mark.parametrize("name", [n for n, c in ako.GATHER_CASES.items() if c[2] == "plain"])
def test_gather_at_the_seam_the_corners_and_the_workgroup_tails(name):
    worst = _check_gather(name)
    d = ako.gather_case(name)
    print(f"\n[parity] gather {name}: S {d['S']}, N {d['N']}, 5 outputs + 3 gradient maps (5 channel groups): worst ratio to the bar {worst:.3f} (bar 1)")


def test_gather_zero_quaternion_rows():
    """norm <= 1e-12 in both kernels: the forward gives exactly 0, the backward g * 1e12 (F.normalize divides by max(|x|, eps))."""
    worst = _check_gather("zero_quat")
    d = ako.gather_case("zero_quat")
    print(f"\n[parity] gather zero_quat: {int(d['zero_rows'].sum())} of {d['N']} rows with a zero rotation sum: worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("name", sorted(ako.SATURATED))
def test_gather_saturated_logits(name):
    """Forward and backward stay finite (ako.bar asserts it) and within the bar; below fp32's normal range with an absolute floor of 1e-37."""
    worst = _check_gather(name)
    which, lo, hi = ako.SATURATED[name]
    print(f"\n[parity] gather {name}: {which} logits in [{lo:g}, {hi:g}]: worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("name", ["s8_full", "s16_n1_last", "s16_n257", "zero_quat", "scale_big"])
def test_gather_parts_and_canonical_activations_give_the_fused_bits(name):
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    d = ako.gather_case(name)
    outs, grads, pix, (xyz, opa, sca, rot) = _gather_gpu(d)
    maps = [_cuda(d[k], True) for k in ("position_map", "other_map", "color_map")]
    parts = (ops.gather_positions(maps[0], pix, xyz),) + tuple(ops.gather_others(maps[1], pix, opa, sca, rot)) + (ops.gather_colors(maps[2], pix),)
    torch.autograd.backward(list(parts), [u.cuda() for u in d["ups"]])
    for what, a, b in zip(ako.GATHER_OUTPUTS, parts, outs):
        assert torch.equal(a, b), f"{name}: part-wise {what} differs from the fused call"
    for what, a, b in zip(("position_map", "other_map", "color_map"), maps, grads):
        assert torch.equal(a.grad, b), f"{name}: part-wise dL/d{what} differs from the fused call"
    zeros = [torch.zeros_like(m) for m in maps]
    fused0 = ops.gather_activate(*zeros, pix, xyz, opa, sca, rot)
    for what, a, b in zip(("opacity", "scales", "rotations"), ops.canonical_activations(pix, d["S"], opa, sca, rot), fused0[1:4]):
        assert torch.equal(a, b), f"{name}: canonical {what} differs from the fused call on all-zero maps"
    print(f"\n[parity] gather {name}: the three part-wise calls (forward, backward) and canonical_activations are bit-identical to the fused call")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# linear-blend skinning
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _lbs_gpu(d, sparse, joint_grad=False):
    """(live positions, live rotations, dL/dpositions, dL/drotations, dL/dA or None) of ops.lbs_transform."""
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    p, r, A = _cuda(d["pos"], True), _cuda(d["rot"], True), _cuda(d["A"], joint_grad)
    lp, lr = ops.lbs_transform(p, r, d["lbs"].cuda(), A, sparse)
    torch.autograd.backward([lp, lr], [u.cuda() for u in d["ups"]])
    return lp.detach(), lr.detach(), p.grad, r.grad, A.grad


_LBS_WHAT = ("live positions", "live rotations", "dL/dpositions", "dL/drotations", "dL/dA")


def _check_lbs(name, forms=("dense", "sparse"), joint_grad=False):
    """The four (five) tensors of each form against the bar, rotations without the fragile rows, rows marked exact left to the caller; the sparse form
    bit-identical to the dense one.  Returns (worst ratio, results of the first form)."""
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    d = ako.lbs_case(name)
    r64, r32 = ako.lbs_reference(name, joint_grad)
    frag, exact = ako.fragile_rows(name), d["exact_rows"]
    assert int((frag & ~exact).sum()) <= ako.FRAGILE_CAP * d["N"]
    res, worst = {}, 0.0
    for form in forms:
        sp = None
        if form == "sparse":
            sp = ops.SparseLbs.build(d["lbs"].cuda())
            assert sp is not None and sp.K == d["K"], f"{name}: no sparse form"
        res[form] = _lbs_gpu(d, sp, joint_grad)
        for i, what in enumerate(_LBS_WHAT[:5 if joint_grad else 4]):
            keep = ~exact & (~frag if "rotations" in what else True) if i < 4 else slice(None)
            worst = max(worst, ako.bar(res[form][i].cpu()[keep], r64[i][keep], r32[i][keep], f"{name} ({form}): {what}"))
    if len(forms) == 2:
        for what, a, b in zip(_LBS_WHAT, res["dense"], res["sparse"]):
            assert a is None or torch.equal(a, b), f"{name}: sparse {what} differs from dense by {float((a - b).abs().max()):.3e}"
    return worst, res[forms[0]]


@pytest.mark.parametrize("N,J", ako.LBS_NJ, ids=[ako.lbs_name(N, J) for N, J in ako.LBS_NJ])
def test_lbs_forward_backward_dense_and_sparse(N, J):
    """Ragged last waves (stage_rows with rows < 64), whole waves past N, odd / even / single J, J at the dense LDS limit (160), quaternions that are not
    unit and weight rows that do not sum to 1."""
    worst, _ = _check_lbs(ako.lbs_name(N, J))
    print(f"\n[parity] lbs N {N}, J {J}: positions, rotations, dL/dpositions, dL/drotations, dense and sparse (bit-identical): worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("name", [c[0] for c in ako.LBS_SPARSE_ONLY])
def test_lbs_sparse_at_256_joints(name):
    worst, _ = _check_lbs(name, forms=("sparse",))
    d = ako.lbs_case(name)
    print(f"\n[parity] lbs {name}: N {d['N']}, J 256, K {d['K']}, joints 250..255 in use, sparse only: worst ratio to the bar {worst:.3f} (bar 1)")


def test_lbs_all_zero_weight_row():
    import torch
    worst, _ = _check_lbs("zero_row")
    d = ako.lbs_case("zero_row")
    row = int(d["exact_rows"].nonzero())
    from animatablegaussians_amd import avatar_ops as ops
    for form, sp in (("dense", None), ("sparse", ops.SparseLbs.build(d["lbs"].cuda()))):
        lp, lr, dp, dr = (t.cpu() for t in _lbs_gpu(d, sp)[:4])
        assert lp[row].tolist() == [0.0, 0.0, 0.0], f"{form}: live position of the all-zero row is {lp[row].tolist()}"
        assert lr[row].tolist() == [0.5, 0.0, 0.0, 0.0], f"{form}: live rotation of the all-zero row is {lr[row].tolist()}"
        assert bool(torch.isfinite(dp[row]).all()) and bool(torch.isfinite(dr[row]).all())
        assert bool((dr[row] == 0).all()) and bool((dp[row] == 0).all()), f"{form}: gradients of the all-zero row are {dp[row].tolist()}, {dr[row].tolist()}"
    print(f"\n[parity] lbs zero_row: row {row} of {d['N']} exact ((0, 0, 0), (0.5, 0, 0, 0), zero gradients), the rest: worst ratio to the bar {worst:.3f} (bar 1)")


def test_lbs_every_matrix_to_quaternion_branch():
    """The four arg-max candidates at blend weight 1, 0.004 and -0.5 (the positive-part branch of the square root), with both upstream gradients."""
    worst, _ = _check_lbs("branches")
    print(f"\n[parity] lbs branches: {ako.lbs_case('branches')['N']} rows, 4 candidates x blend weights 1 / 0.004 / -0.5, all four tensors: worst ratio to the bar {worst:.3f} (bar 1)")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the limits on J
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_dense_lbs_refuses_j_beyond_the_lds():
    """Dense J = 160 runs (test_lbs_forward_backward_dense_and_sparse asserts its values); dense J = 161 is refused by the argument check, whose message
    names the largest dense J -- that message is what tells the refusal from a launch error.  The sparse form keeps J <= 256."""
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd import avatar_ops as ops
    worst, _ = _check_lbs(ako.lbs_name(65, 160), forms=("dense",))
    N, J = 65, 161
    g = torch.Generator().manual_seed(1)
    lbs = torch.zeros(N, J)
    lbs[:, ::40] = torch.rand(N, 5, generator=g) + 0.1
    pos, rot, A = torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g), ako.joints(J, 2)
    with pytest.raises(_lib.AgNativeError, match=r"largest dense J = \d+") as e:
        ops.lbs_transform(pos.cuda(), rot.cuda(), lbs.cuda(), A.cuda())
    largest = int(re.search(r"largest dense J = (\d+)", str(e.value)).group(1))
    assert largest == 160 and "code -1" in str(e.value), str(e.value)                  # AG_ERR_INVALID_ARGUMENT, not a HIP error
    torch.cuda.synchronize()                                                           # nothing was launched: the device is in order
    with pytest.raises(_lib.AgNativeError, match=r"largest dense J = 160"):            # beyond the sparse limit too, a dense call is told the dense limit
        ops.lbs_transform(pos.cuda(), rot.cuda(), torch.zeros(N, 300).cuda(), ako.joints(300, 2).cuda())
    sp = ops.SparseLbs.build(lbs.cuda())
    lp, lr = ops.lbs_transform(pos.cuda(), rot.cuda(), lbs.cuda(), A.cuda(), sp)        # the same call in the sparse form
    want = ako.ao.transform_cano2live(pos.double(), rot.double(), lbs.double(), A.double())
    f32 = ako.ao.transform_cano2live(pos, rot, lbs, A)
    worst = max(worst, ako.bar(lp, want[0], f32[0], "sparse J = 161: positions"), ako.bar(lr, want[1], f32[1], "sparse J = 161: rotations"))
    print(f"\n[parity] lbs limits: dense J 160 within the bar, dense J 161 refused ('{str(e.value)[-150:]}'), sparse J 161: worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("N,J", ako.JOINT_GRAD_NJ, ids=[ako.lbs_name(N, J) for N, J in ako.JOINT_GRAD_NJ])
def test_lbs_joint_gradient_at_its_largest_j(N, J):
    import torch
    worst, res = _check_lbs(ako.lbs_name(N, J), joint_grad=True)
    assert torch.equal(res[4][:, 3], torch.zeros_like(res[4][:, 3])), "row 3 of dL/dA is not exactly 0"
    print(f"\n[parity] lbs joint gradient N {N}, J {J}: dL/dA and the four other tensors, dense and sparse (bit-identical): worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("name", ako.JOINT_GRAD_EDGE)
def test_lbs_joint_gradient_through_the_shared_chain(name):
    """dL/dA comes from the routine that also gives dL/drotations (lbs_backward_gaussian of csrc/ag_avatar.hip): here on every arg-max candidate and the
    positive-part branch of the square root, at J = 1, with one Gaussian beside three idle waves, with one Gaussian in the second workgroup at the product's
    J, and at J = 64, dense and sparse (bit-identical).  That asking for dL/dA leaves dL/dpositions and dL/drotations the bits of the plain backward is
    asserted by tests/test_pose_grad_gpu.py::test_lbs_joint_gradient_at_full_size_and_bits."""
    import torch
    assert not bool(ako.fragile_rows(name).any()), f"{name}: dL/dA is compared over all rows, none may be fragile"
    worst, res = _check_lbs(name, joint_grad=True)
    assert torch.equal(res[4][:, 3], torch.zeros_like(res[4][:, 3])), "row 3 of dL/dA is not exactly 0"
    d = ako.lbs_case(name)
    print(f"\n[parity] lbs joint gradient {name}: N {d['N']}, J {d['J']}, dL/dA and the four other tensors, dense and sparse (bit-identical): worst ratio to the bar {worst:.3f} (bar 1)")


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_lbs_joint_gradient_refuses_j_141(form):
    import torch
    from animatablegaussians_amd import _lib
    from animatablegaussians_amd import avatar_ops as ops
    N, J = 65, 141
    g = torch.Generator().manual_seed(3)
    lbs = torch.zeros(N, J)
    lbs[:, ::47] = torch.rand(N, 3, generator=g) + 0.1
    A = ako.joints(J, 4).cuda().requires_grad_(True)
    sp = ops.SparseLbs.build(lbs.cuda()) if form == "sparse" else None
    lp, lr = ops.lbs_transform(torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 4, generator=g).cuda(), lbs.cuda(), A, sp)
    with pytest.raises(_lib.AgNativeError, match="140"):
        (lp.sum() + lr.sum()).backward()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hand fusion
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boxes", sorted(ako.HAND_BOXES))
@pytest.mark.parametrize("N", ako.HAND_N)
def test_hand_fuse_against_float64(N, boxes):
    import torch
    from animatablegaussians_amd import avatar_ops as ops
    d = ako.hand_case(N, boxes)
    ref, w = ako.hand_reference(N, boxes)
    keys = ('positions', 'opacity', 'scales', 'rotations')
    cur = [d["cur"][k].cuda() for k in keys]
    hand = [d["hand"][k].cuda() for k in keys]
    xyz, left, right = d["xyz"].cuda(), d["left"].cuda(), d["right"].cuda()
    before = [t.clone() for t in cur + hand + [xyz, left, right]]
    got = ops.hand_fuse(*cur, xyz, left, right, d["centre"], *hand)
    for a, b in zip(cur + hand + [xyz, left, right], before):
        assert torch.equal(a, b), "hand_fuse changed one of its inputs"
    below = d["xyz"][:, 1] < d["centre"][1]
    worst = 0.0
    for k, t in zip(keys, got):
        t = t.cpu()
        assert bool(torch.isfinite(t).all()), k
        assert torch.equal(t[below], d["cur"][k][below]), f"{k}: rows below the centre are not returned bit-identical"
        lim = ako.HAND_ATOL + ako.HAND_RTOL * ref[k].abs()
        ratio = float(((t.double() - ref[k]).abs() / lim).max())
        worst = max(worst, ratio)
    print(f"\n[parity] hand fusion {boxes}, N {N}: worst ratio to rtol {ako.HAND_RTOL:g} + atol {ako.HAND_ATOL:g} against float64: {worst:.3f} (bar 1)")
    assert worst <= 1.0, f"hand fusion {boxes}, N {N}: {worst:.3f} x the tolerance"
