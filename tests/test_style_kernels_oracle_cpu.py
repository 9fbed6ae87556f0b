"""The float64 oracles of tests/style_kernels_oracle.py against torch's own float64 bilinear interpolation, and the record of WHY
tests/test_style_kernels_edges_gpu.py exists: which body of bilinear_backward_kernel (the unrolled one for candidate ranges below 6, the loop
otherwise) every resize shape of the suite reaches.  Needs no GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_kernels_oracle as sko  # noqa: E402

# every (input size, output size) pair the GPU test resizes at: the resize cases and the select_add_rows view features
PAIRS = [(hw, ohw) for _, hw, ohw in sko.RESIZE_CASES] + sorted({(vf, (sko.SELECT_H, W)) for _, W, _, _, vf in sko.SELECT_CASES if vf is not None})


@pytest.mark.parametrize("hw,ohw", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_resize_matrix_reproduces_float64_interpolate_and_its_adjoint(hw, ohw):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(2, 3, *ohw, generator=g, dtype=torch.float64)
    want = F.interpolate(x, ohw, mode="bilinear")
    want.backward(up)
    assert float((sko.resize(x.detach(), ohw) - want.detach()).abs().max()) <= 1e-12
    assert float((sko.resize_adjoint(up, hw) - x.grad).abs().max()) <= 1e-12
    # rows of the matrix are partitions of one: the resize of a constant is that constant
    for n_in, n_out in zip(hw, ohw):
        A = sko.resize_matrix(n_in, n_out)
        assert A.shape == (n_out, n_in) and float((A.sum(1) - 1).abs().max()) <= 1e-15 and float(A.min()) >= 0


def test_select_add_oracle_reproduces_the_float64_torch_composition():
    for name, W, src, rows, vf_size in sko.SELECT_CASES:
        g = torch.Generator().manual_seed(6)
        out = torch.randn(4, 3, sko.SELECT_H, W, generator=g, dtype=torch.float64).requires_grad_(True)
        vf = torch.randn(rows[1] - rows[0], 3, *vf_size, generator=g, dtype=torch.float64).requires_grad_(True) if vf_size else None
        up = torch.randn(len(src), 3, sko.SELECT_H, W, generator=g, dtype=torch.float64)
        want = out.index_select(0, torch.tensor(src))
        if vf is not None:
            f = vf if vf_size == (sko.SELECT_H, W) else F.interpolate(vf, (sko.SELECT_H, W), mode="bilinear")
            want = torch.cat([want[:rows[0]], want[rows[0]:rows[1]] + f, want[rows[1]:]], 0)
        want.backward(up)
        o2 = out.detach().clone().requires_grad_(True)
        v2 = vf.detach().clone().requires_grad_(True) if vf is not None else None
        got = sko.select_add(o2, src, v2, rows)
        got.backward(up)
        assert float((got - want).detach().abs().max()) <= 1e-12 and float((o2.grad - out.grad).abs().max()) <= 1e-12, name
        assert vf is None or float((v2.grad - vf.grad).abs().max()) <= 1e-12, name


def test_the_wide_cases_reach_the_loop_form_on_the_intended_axis():
    by_name = {n: (hw, ohw) for n, hw, ohw in sko.RESIZE_CASES}
    for name, (wide_y, wide_x) in sko.WIDE_CASES.items():
        hw, ohw = by_name[name]
        sy, sx = sko.reader_span(hw[0], ohw[0]), sko.reader_span(hw[1], ohw[1])
        assert (sy.max() >= sko.BILINEAR_TAPS) == wide_y and (sx.max() >= sko.BILINEAR_TAPS) == wide_x, (name, sy, sx)
        assert sko.loop_form(hw, ohw).any()
    # the one-axis cases keep the other axis at the span of an identity resize
    assert sko.reader_span(50, 50).max() == 2
    # 8x in y: every element of that case is in the loop form, borders included
    assert sko.loop_form(*by_name["wide_both"]).all()


def test_the_straddle_case_has_elements_in_both_forms():
    hw, ohw = {n: (a, b) for n, a, b in sko.RESIZE_CASES}["straddle"]
    m = sko.loop_form(hw, ohw)
    assert m.any() and (~m).any(), m
    sy = sko.reader_span(hw[0], ohw[0])
    assert sy.max() == sko.BILINEAR_TAPS and (sy == sko.BILINEAR_TAPS - 1).any(), sy        # right at the threshold, on both sides


def test_the_shapes_of_test_linear_gpu_reach_the_unrolled_form_only():
    for hw, ohw in sko.OLD_RESIZE_SHAPES:
        assert not sko.loop_form(hw, ohw).any(), (hw, ohw)
        assert max(sko.reader_span(hw[0], ohw[0]).max(), sko.reader_span(hw[1], ohw[1]).max()) < sko.BILINEAR_TAPS


def test_reader_range_covers_every_reader():
    """The range restated from the kernel contains every output that reads the input with a weight above rounding (a range that missed one would
    make the gather wrong, not merely slow): checked against the dense matrix."""
    for hw, ohw in PAIRS + sko.OLD_RESIZE_SHAPES:
        for n_in, n_out in zip(hw, ohw):
            A = sko.resize_matrix(n_in, n_out).numpy()
            lo, hi = sko.reader_range(n_in, n_out)
            for i in range(n_in):
                readers = (A[:, i] > 1e-6).nonzero()[0]
                assert len(readers) == 0 or (lo[i] <= readers.min() and readers.max() <= hi[i]), (n_in, n_out, i)
