"""What the wrappers of the fused MLP kernels share: the packed weight layout of ``csrc/ag_mlp_tile.h`` and the ctypes plumbing of a launch."""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import stream  # noqa: F401  (the wrappers take it from here, with ptr)


def pad(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _order(Kp: int, Np: int) -> np.ndarray:
    """Where in a row-major [Kp, Np] each element of the packed block comes from: packed element ``[g][n][j]`` is ``[4 g + j][n]``."""
    return np.arange(Kp * Np).reshape(Kp // 4, 4, Np).transpose(0, 2, 1).reshape(-1)


def pack_rows(rows: np.ndarray, Kp: int, Np: int) -> np.ndarray:
    """``rows`` [K, N] (input column k, output column n; ``K <= Kp``, a multiple of 4, ``N <= Np``) -> float32 [Kp / 4 * Np * 4], zero in
    the padding."""
    full = np.zeros((Kp, Np), np.float32)
    full[:rows.shape[0], :rows.shape[1]] = rows
    return full.reshape(-1)[_order(Kp, Np)]


def unpack_rows(packed: np.ndarray, Kp: int, Np: int) -> np.ndarray:
    """The inverse of ``pack_rows``: -> [Kp, Np], the padding rows and columns included."""
    full = np.empty(Kp * Np, np.float32)
    full[_order(Kp, Np)] = packed
    return full.reshape(Kp, Np)


def ptr(t) -> ctypes.c_void_p:
    """The device pointer of ``t``; NULL for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
