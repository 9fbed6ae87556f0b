"""The packed weight block of the fused MLP kernels (``mlp_blob.py``) against the formula of ``csrc/ag_mlp_tile.h``, written as plain loops.  No GPU."""
import numpy as np
import pytest


@pytest.mark.parametrize("K,N", [(1, 1), (7, 33), (64, 3), (67, 257)])
def test_pack_rows_is_the_headers_formula_and_unpack_rows_its_inverse(K, N):
    from animatablegaussians_amd.mlp_blob import pack_rows, pad, unpack_rows
    Kp, Np = pad(K, 8), pad(N, 32)
    assert Kp % 8 == 0 and Np % 32 == 0 and 0 <= Kp - K < 8 and 0 <= Np - N < 32
    W = np.random.RandomState(K * 1000 + N).normal(size=(N, K)).astype(np.float32)          # [out, in], as a linear's weight
    W[W == 0] = 1.0                                                                         # a zero is the padding's alone
    want = np.zeros((Kp // 4, Np, 4), np.float32)
    for g in range(Kp // 4):
        for n in range(N):
            for j in range(4):
                if 4 * g + j < K:
                    want[g, n, j] = W[n, 4 * g + j]
    packed = pack_rows(W.T, Kp, Np)
    assert packed.dtype == np.float32 and packed.shape == (Kp // 4 * Np * 4,)
    assert np.array_equal(packed, want.reshape(-1))
    rows = unpack_rows(packed, Kp, Np)
    assert rows.dtype == np.float32 and rows.shape == (Kp, Np)
    assert np.array_equal(rows[:K, :N], W.T)
    assert not rows[K:].any() and not rows[:, N:].any() and np.count_nonzero(rows) == K * N
