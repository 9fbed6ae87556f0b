"""Float64 oracles of the style-path kernels of csrc/ag_linear.hip (bilinear resize, select_add_rows, the EqualLinear group), written from the
definitions, and the shapes at which tests/test_style_kernels_edges_gpu.py runs them.  Not a test module.

The resize oracle is a dense matrix per axis (``resize_matrix``): the forward is ``Ay @ x @ Ax.T`` and the adjoint ``Ay.T @ g @ Ax``, so neither
restates the gather of the kernel's backward.  ``reader_span`` restates one thing of the kernel, the candidate range of ``reader_range``, and only
to say which of the backward's two bodies a shape reaches (tests/test_style_kernels_oracle_cpu.py)."""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

BILINEAR_TAPS = 6            # kBilinearTaps: the unrolled body of bilinear_backward_kernel handles hi - lo < 6 on both axes

# (name, (H, W), (OH, OW)): the cases of the resize test and what each was built to reach
RESIZE_CASES = [
    ("wide_both", (5, 7), (40, 21)),                 # 8x in y, 3x in x: every element in the loop form
    ("wide_y", (3, 50), (7, 50)),                    # y in the loop form (span 6 at iy = 1) while x has span 2
    ("wide_x", (50, 3), (50, 7)),                    # the transpose
    ("straddle", (6, 6), (13, 12)),                  # spans 5 and 6 in y: both bodies in one launch
    ("factor_2_5", (16, 16), (40, 40)),              # a non-integer factor
    ("single_input", (1, 1), (9, 9)),                # every output folds onto one input
    ("down_up", (20, 3), (5, 11)),                   # down in y, up in x
    ("wider_than_64", (4, 70), (10, 150)),           # the ix += 64 stride of the backward (the forward has 38 four-output groups: one pass)
    ("forward_stride", (2, 70), (3, 300)),           # 75 four-output groups per row: the q += 64 stride of the forward
]
WIDE_CASES = {"wide_both": (True, True), "wide_y": (True, False), "wide_x": (False, True)}      # name -> (y reaches the loop form, x does)
# the shapes tests/test_linear_gpu.py runs the resize at (its five cases and the two resizing cases of its select_add_rows test)
OLD_RESIZE_SHAPES = [((128, 128), (256, 256)), ((37, 53), (64, 101)), ((64, 48), (20, 31)), ((9, 9), (9, 9)), ((1, 7), (5, 3)), ((16, 12), (32, 24))]

# select_add_rows: (name, W, src, rows, vf size or None); C = 3, H = 12, the shared state has 4 rows
SELECT_H = 12
SELECT_CASES = [
    ("w23_m16_all_rows", 23, (0, 1, 2, 3, 3, 1, 0, 2, 1, 1, 3, 0, 2, 3, 1, 2), (0, 16), (4, 8)),      # scalar path, M = 16, repeated sources, every row adds
    ("w23_last_row", 23, (0, 1, 2, 3, 3, 1, 0, 2, 1, 1, 3, 0, 2, 3, 1, 2), (15, 16), (4, 8)),         # rows = (M - 1, M)
    ("w23_no_vf", 23, (0, 1, 2, 3), None, None),
    ("w5_3x", 5, (3, 1, 1, 0), (3, 4), (4, 2)),                                                       # scalar path with two groups per row, the second ragged
    ("w5_same", 5, (0, 1, 2, 3), (0, 4), (12, 5)),
    ("w10_3x", 10, (2, 0, 0, 3, 0), (1, 4), (4, 4)),                                                  # 3x in y, 2.5x in x
    ("w10_2_5x", 10, (2, 0, 0, 3, 0), (1, 4), (5, 4)),                                                # 2.4x in y, 2.5x in x
    ("w10_same", 10, (0, 1, 2, 3), (0, 4), (12, 10)),
    ("w10_no_vf", 10, (1, 1, 1), None, None),
    ("w12_3x_vector", 12, (0, 2, 2, 2, 1), (0, 5), (4, 4)),                                           # the float4 path beyond 2x
    ("w12_unused_source", 12, (0, 3, 3), (2, 3), (4, 5)),                                             # a row of the shared state nobody continues
    ("w260_vector_stride", 260, (1, 0), (0, 2), (5, 100)),                                            # 65 groups per row: the q += 64 stride, float4 path
    ("w261_scalar_stride", 261, (1, 0), (1, 2), (5, 100)),                                            # 66 groups, the last one ragged, scalar path
]


def resize_matrix(n_in, n_out):
    """[n_out, n_in] float64: row o holds the two weights with which output o of ``F.interpolate(mode="bilinear", align_corners=False)`` reads
    one axis: source coordinate max(0, n_in / n_out (o + 0.5) - 0.5), lower neighbour its floor, upper neighbour clamped onto the last input."""
    A = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    for o in range(n_out):
        src = max(0.0, scale * (o + 0.5) - 0.5)
        i0 = int(src)
        i1 = min(i0 + 1, n_in - 1)
        A[o, i0] += 1.0 - (src - i0)
        A[o, i1] += src - i0
    return torch.from_numpy(A)


def resize(x, size):
    """Bilinear resize of [..., H, W] float64 to ``size``."""
    return resize_matrix(x.shape[-2], size[0]) @ x @ resize_matrix(x.shape[-1], size[1]).T


def resize_adjoint(g, size):
    """The adjoint of ``resize`` from ``size`` to g's resolution, applied to g [..., OH, OW] float64."""
    return resize_matrix(size[0], g.shape[-2]).T @ g @ resize_matrix(size[1], g.shape[-1])


def reader_range(n_in, n_out):
    """``(lo, hi)`` of the kernel's ``reader_range`` for every input index of one axis, in float32 as there (int64 [n_in] each)."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    inv = f(1.0) / scale
    i = np.arange(n_in, dtype=f)
    lo = np.floor((i - f(0.5)) * inv - f(0.5)).astype(np.int64)
    hi = np.ceil((i + f(1.5)) * inv - f(0.5)).astype(np.int64)
    return np.maximum(lo, 0), np.minimum(hi, n_out - 1)


def reader_span(n_in, n_out):
    """``hi - lo`` of ``reader_range``: below BILINEAR_TAPS on both axes an input element takes the unrolled body of the backward."""
    lo, hi = reader_range(n_in, n_out)
    return hi - lo


def loop_form(in_hw, out_hw):
    """bool [H, W]: the input elements whose gradient bilinear_backward_kernel forms in its loop body."""
    sy, sx = reader_span(in_hw[0], out_hw[0]), reader_span(in_hw[1], out_hw[1])
    return (sy[:, None] >= BILINEAR_TAPS) | (sx[None, :] >= BILINEAR_TAPS)


def select_add(out, src, vf, rows):
    """x[m] = out[src[m]] (+ vf[m - rows[0]] resized to out's resolution for rows[0] <= m < rows[1]); float64, differentiable."""
    x = out.index_select(0, torch.tensor(list(src)))
    if vf is None:
        return x
    f = vf if tuple(vf.shape[-2:]) == tuple(out.shape[-2:]) else resize(vf, out.shape[-2:])
    return torch.cat([x[:rows[0]], x[rows[0]:rows[1]] + f, x[rows[1]:]], 0)


def equal_linear_group(xs, ws, bs, lr_mul, activation, normalize_input=False):
    """[EqualLinear_j(xs[j])] by the reference formula of tests/test_linear_gpu.py (one definition for both files), PixelNorm
    (x / sqrt(mean(x^2) + 1e-8) per row) first when asked."""
    from test_linear_gpu import _ref_equal_linear
    if normalize_input:
        xs = [x * torch.rsqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-8) for x in xs]
    return [_ref_equal_linear(x, w, b, lr_mul, activation) for x, w, b in zip(xs, ws, bs)]
