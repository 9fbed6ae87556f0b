"""csrc/ag_linear.hip off the shapes of the workload (tests/test_linear_gpu.py runs the workload's own, which all land on the fast paths): the
loop body of the bilinear backward (candidate ranges of 6 and more: up-sampling factors above 2), both of its bodies in one launch, the scalar
store path and the column stride of select_add_rows, the EqualLinear group at in_features of 4 / no multiple of 256 or 512, at B = 8, at
AG_LINEAR_MAX_JOBS jobs and through PixelNorm at B > 1, the host refusals, and plane sums with ragged, misaligned and one-element slices.
tests/test_style_kernels_oracle_cpu.py asserts which body each resize shape reaches.

Yardstick: the float64 oracles of tests/style_kernels_oracle.py.  Bars (those of test_linear_gpu.py): a deviation of at most 4 x the deviation of
torch's float32 CPU evaluation of the same data from the oracle, the 4 being what the project grants a different summation order, with floors of
2e-6 (forward, EqualLinear) and 4e-6 (resize backward) of the oracle's largest value; plane sums of standard-normal data within
2e-6 sqrt(n) 4.  Every check prints its ratio to the bar (``pytest -s``)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_kernels_oracle as sko  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(what, got, want, ref32, floor):
    """got (GPU), ref32 (torch float32 on the CPU) against want (float64): finite everywhere, and the largest deviation over EVERY element within
    max(4 x torch's, floor) of want's largest value.  Returns the ratio to that bar."""
    got, want, ref32 = got.detach().cpu().double(), want.detach().double(), ref32.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    scale = float(want.abs().max()) + 1e-30
    err, err32 = float((got - want).abs().max()) / scale, float((ref32 - want).abs().max()) / scale
    ratio = err / max(4 * err32, floor)
    print(f"  {what}: {err:.2e} of the scale (torch fp32 {err32:.2e}), {ratio:.3f} of the bar")
    assert ratio <= 1.0, f"{what}: {err:.2e} of the scale (torch fp32: {err32:.2e}, floor {floor:g})"
    return ratio


def _on_offset(t, off):
    """A contiguous GPU copy of t that starts ``off`` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


# ---- bilinear resize ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name,hw,ohw", sko.RESIZE_CASES, ids=[c[0] for c in sko.RESIZE_CASES])
def test_bilinear_resize_beyond_2x_equals_the_float64_matrix_form(name, hw, ohw, off):
    """Forward and backward at up-sampling factors above 2 (the loop body of the backward), just over 2 (both bodies in one launch), on one
    axis only, from a single input, down on one axis and up on the other, and on rows wider than the 64 lanes -- with the input and the
    upstream gradient aligned and one float off a 16-byte boundary (the kernels read with scalar loads: no alignment is assumed).  Both
    parities of OW % 4 occur (40, 12, 300 against 21, 50, 7, 9, 11, 150): the float4 and the guarded scalar store of the forward."""
    from animatablegaussians_amd.linear_ops import bilinear_resize, bilinear_resize_backward
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, *hw, generator=g)
    up = torch.randn(2, 3, *ohw, generator=g)
    want, want_g = sko.resize(x.double(), ohw), sko.resize_adjoint(up.double(), hw)
    xc = x.clone().requires_grad_(True)
    y32 = F.interpolate(xc, ohw, mode="bilinear")
    y32.backward(up)

    xg = _on_offset(x, off).requires_grad_(True)
    upg = _on_offset(up, off)
    got = bilinear_resize(xg, ohw)
    got.backward(upg)
    print(f"\n{name} {hw} -> {ohw}, offset {off}: {int(sko.loop_form(hw, ohw).sum())} of {hw[0] * hw[1]} elements in the loop form")
    _check("forward", got, want, y32, 2e-6)
    _check("backward", xg.grad, want_g, xc.grad, 4e-6)
    # the adjoint called directly (the route of select_add_rows' view-feature gradient) and a second run: a gather in a fixed order, the same bits
    assert torch.equal(bilinear_resize_backward(upg, hw), xg.grad)
    xg2 = _on_offset(x, off).requires_grad_(True)
    got2 = bilinear_resize(xg2, ohw)
    got2.backward(upg)
    assert torch.equal(got2, got) and torch.equal(xg2.grad, xg.grad)


# ---- select_add_rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,src,rows,vf_size", sko.SELECT_CASES, ids=[c[0] for c in sko.SELECT_CASES])
def test_select_add_rows_on_the_scalar_path_and_beyond_2x(name, W, src, rows, vf_size):
    """grouped._SelectAddRows where W % 4 != 0 (guarded scalar stores: the lanes past the end of a row read a clamped column and must write
    nothing -- the kernel allocates x itself, so the check is that EVERY element of x, the first and last column of every row among them,
    equals the oracle), with M = 16 and repeated sources, with the view feature at 3x / 2.4x / 2.5x / 2.875x (``lerp_of`` beyond 2x and its adjoint
    through the loop body of bilinear_resize_backward), at the target's own size, absent, and on rows of more than 64 four-pixel groups."""
    from animatablegaussians_amd.grouped import _SelectAddRows
    H = sko.SELECT_H
    g = torch.Generator().manual_seed(14)
    out = torch.randn(4, 3, H, W, generator=g)
    vf = torch.randn(rows[1] - rows[0], 3, *vf_size, generator=g) if vf_size else None
    up = torch.randn(len(src), 3, H, W, generator=g)

    o64 = out.double().requires_grad_(True)
    v64 = vf.double().requires_grad_(True) if vf is not None else None
    want = sko.select_add(o64, src, v64, rows)
    want.backward(up.double())

    o32 = out.clone().requires_grad_(True)
    v32 = vf.clone().requires_grad_(True) if vf is not None else None
    y32 = o32.index_select(0, torch.tensor(src))
    if v32 is not None:
        f = v32 if vf_size == (H, W) else F.interpolate(v32, (H, W), mode="bilinear")
        y32 = torch.cat([y32[:rows[0]], y32[rows[0]:rows[1]] + f, y32[rows[1]:]], 0)
    y32.backward(up)

    def run():
        og = out.cuda().requires_grad_(True)
        vg = vf.cuda().requires_grad_(True) if vf is not None else None
        y = _SelectAddRows.apply(og, vg, src, rows)
        y.backward(up.cuda())
        return y.detach(), og.grad, vg.grad if vg is not None else None

    got, again = run(), run()
    print(f"\n{name}: W {W}, M {len(src)}, rows {rows}, view feature {vf_size}")
    _check("x", got[0], want, y32, 2e-6)
    _check("g_out", got[1], o64.grad, o32.grad, 2e-6)
    if vf is not None:
        _check("g_vf", got[2], v64.grad, v32.grad, 4e-6)
    assert all(torch.equal(a, b) for a, b in zip(got, again) if a is not None)


# ---- EqualLinear group ----------------------------------------------------------------------------------------------------------------
def _linear_runs(xs_of, n_inputs, B, fin, outs, no_bias, lr_mul, activation, normalize=False, seed=21):
    """The group on the GPU (twice) against the reference formula in float64 and float32 on the CPU.  ``xs_of(inputs)``: the per-job input list.
    Each run returns (ys, input gradients, weight gradients, bias gradients)."""
    from animatablegaussians_amd.linear_ops import equal_linear_group
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, fin, generator=g) for _ in range(n_inputs)]
    ws = [torch.randn(o, fin, generator=g) / lr_mul for o in outs]
    bs = [None if j in no_bias else torch.randn(o, generator=g) for j, o in enumerate(outs)]
    ups = [torch.randn(B, o, generator=g) for o in outs]

    def run(dev, dtype, fn):
        leaf = lambda t: t.detach().clone().to(dev, dtype).requires_grad_(True)      # noqa: E731
        X = [leaf(x) if not normalize else x.to(dev, dtype) for x in xs]
        Wt, Bi = [leaf(w) for w in ws], [leaf(b) if b is not None else None for b in bs]
        ys = fn(xs_of(X), Wt, Bi)
        torch.autograd.backward(list(ys), [u.to(dev, dtype) for u in ups])
        cpu = lambda t: t.detach().cpu().double() if t is not None else None          # noqa: E731
        return ([cpu(y) for y in ys], [cpu(x.grad) for x in X], [cpu(w.grad) for w in Wt], [cpu(b.grad) if b is not None else None for b in Bi])

    ref = lambda X, Wt, Bi: sko.equal_linear_group(X, Wt, Bi, lr_mul, activation, normalize)      # noqa: E731
    dev = lambda X, Wt, Bi: equal_linear_group(X, Wt, Bi, lr_mul=lr_mul, activation=activation, normalize_input=normalize)      # noqa: E731
    return run("cpu", torch.float64, ref), run("cpu", torch.float32, ref), run("cuda", torch.float32, dev), run("cuda", torch.float32, dev)


def _check_linear(want, ref32, got, again, input_grads=True):
    worst = 0.0
    for k, part in enumerate(("y", "g_x", "g_weight", "g_bias")):
        if part == "g_x" and not input_grads:
            assert all(t is None for t in got[k])
            continue
        for j, (a, w, r, a2) in enumerate(zip(got[k], want[k], ref32[k], again[k])):
            if w is None:
                assert a is None
                continue
            worst = max(worst, _check(f"{part}[{j}]", a, w, r, 2e-6))
            assert torch.equal(a, a2), f"{part}[{j}] differs between two runs"
    return worst


@pytest.mark.parametrize("sharing", ["aabb", "aba"])
@pytest.mark.parametrize("activation", [False, True])
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("fin", [4, 36, 260, 516])
def test_equal_linear_group_off_the_512_column_shape(fin, B, activation, sharing):
    """in_features 4 (one busy lane of 64 in the forward, two threads of 256 in the backward), 36, 260 (a second, ragged pass of the forward's
    256-column loop) and 516 (a second pass of the backward's 512-column loop); B = 8, the maximum, where g_weight and g_bias accumulate in
    place over the batch rows; jobs of 1, 16 (exactly one chunk of the backward), 17 and 33 rows; one job without bias; inputs shared as
    [a, a, b, b] (one g_x per group) and as [a, b, a], where the two jobs of ``a`` are not consecutive: they give two g_x that autograd adds."""
    outs = [1, 16, 17, 33] if sharing == "aabb" else [16, 17, 33]
    xs_of = (lambda X: [X[0], X[0], X[1], X[1]]) if sharing == "aabb" else (lambda X: [X[0], X[1], X[0]])
    lr_mul = 0.01 if activation else 1.0
    print(f"\nin {fin}, B {B}, activation {activation}, inputs {sharing}")
    runs = _linear_runs(xs_of, 2, B, fin, outs, () if activation else (1,), lr_mul, activation)
    _check_linear(*runs)


def test_equal_linear_group_with_the_most_jobs_a_call_takes():
    from animatablegaussians_amd.linear_ops import MAX_JOBS
    assert MAX_JOBS == 32
    print(f"\n{MAX_JOBS} jobs of 3 rows")
    # three inputs: 10, 10 and 12 consecutive jobs
    runs = _linear_runs(lambda X: [X[0]] * 10 + [X[1]] * 10 + [X[2]] * (MAX_JOBS - 20), 3, 2, 36, [3] * MAX_JOBS, (5,), 1.0, False)
    _check_linear(*runs)


@pytest.mark.parametrize("activation", [False, True])
def test_equal_linear_group_pixel_norm_of_three_rows(activation):
    """normalize_input (the mapping network's PixelNorm) with B = 3: every row has its own factor, in the forward and in the weight gradient."""
    from animatablegaussians_amd.linear_ops import equal_linear_group
    lr_mul = 0.01 if activation else 1.0
    print(f"\nPixelNorm, B 3, in 260, activation {activation}")
    runs = _linear_runs(lambda X: [X[0], X[0], X[1]], 2, 3, 260, [17, 5, 16], (), lr_mul, activation, normalize=True)
    _check_linear(*runs, input_grads=False)
    x = torch.randn(3, 260, device="cuda", requires_grad=True)
    w = torch.randn(5, 260, device="cuda", requires_grad=True)
    (y,) = equal_linear_group([x], [w], [None], normalize_input=True)
    with pytest.raises(RuntimeError, match="no input gradient through the PixelNorm"):
        y.sum().backward()


def test_equal_linear_group_refusals():
    """Each raised by the host checks that precede the launch (the messages are theirs)."""
    from animatablegaussians_amd.linear_ops import MAX_JOBS, equal_linear_group
    dev = "cuda"
    with pytest.raises(RuntimeError, match="bad job count / batch / in_features"):
        equal_linear_group([torch.randn(9, 8, device=dev)], [torch.randn(4, 8, device=dev)], [None])
    with pytest.raises(RuntimeError, match="bad job count / batch / in_features"):
        equal_linear_group([torch.randn(2, 6, device=dev)], [torch.randn(4, 6, device=dev)], [None])
    x = _on_offset(torch.randn(2, 8), 1)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        equal_linear_group([x], [torch.randn(4, 8, device=dev)], [None])
    x = torch.randn(1, 8, device=dev)
    with pytest.raises(RuntimeError, match=f"1 .. {MAX_JOBS} layers per call"):
        equal_linear_group(x, [torch.randn(2, 8, device=dev) for _ in range(MAX_JOBS + 1)], [None] * (MAX_JOBS + 1))
    # the same calls within the limits pass
    (y,) = equal_linear_group([torch.ones(8, 8, device=dev)], [torch.ones(4, 8, device=dev)], [None])
    assert torch.equal(y.cpu(), torch.full((8, 4), 8 * (1 / math.sqrt(8))))


# ---- plane sums -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 65, 65), (1, 4, 64, 65), (1, 5000, 2, 3), (1, 1, 1, 4097), (2, 3, 1, 3)], ids=str)
def test_plane_sums_with_ragged_misaligned_and_many_planes(shape):
    """(3, 2, 65, 65): two slices of 2116 and 2109 floats, planes 1-3 and 5 start off a 16-byte boundary (the scalar loop on a sliced plane),
    planes 0 and 4 end in a ragged float.  (1, 4, 64, 65): two slices of 2080, aligned, no multiple of the 1024-float pass.  (1, 5000, 2, 3):
    more than 4096 planes, one slice each, every other plane aligned.  (1, 1, 1, 4097): slices of 2052 and 2045 floats, the last float ragged.
    (2, 3, 1, 3): planes shorter than one float4."""
    from animatablegaussians_amd.linear_ops import plane_sums
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(19))
    want = x.double().sum((2, 3))
    got = plane_sums(x.cuda())
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    n = shape[2] * shape[3]
    err, bar = float((got.cpu().double() - want).abs().max()), 2e-6 * math.sqrt(n) * 4
    print(f"\nplane sums {shape}: {err:.2e}, {err / bar:.3f} of the bar")
    assert err <= bar
    assert torch.equal(got, plane_sums(x.cuda()))
    # all ones: every partial sum is a small integer, the result is exact
    ones = plane_sums(torch.ones(*shape, device="cuda"))
    assert torch.equal(ones.cpu(), torch.full(shape[:2], float(n)))
