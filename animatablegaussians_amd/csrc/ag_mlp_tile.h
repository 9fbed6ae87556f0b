// One 32 x 32 output tile of a fused-MLP layer on v_mfma_f32_32x32x2_f32, shared by field_kernel<false>, field_kernel<true>
// (ag_template_field.hip) and hand_fuse_kernel (ag_hand_fusion.hip).  The ONE statement of what their bit-for-bit contracts rest on:
//   blob    a layer's weights as [k / 4][Np][4] floats (Np a multiple of 32, k padded to a multiple of 8), its Np biases behind them;
//   reads   lane l (i = l & 31, h = l >> 5) of the wave that owns output columns n = 32 t + i takes, per group of 8 k from k0, ONE float4 of
//           the tile's row i (k0 + 4 h .. k0 + 4 h + 3) and ONE float4 of the blob (the same k of column n: a wave reads 2 x 512 contiguous bytes);
//   order   4 MFMAs per group, so k runs k0, k0 + 4, k0 + 1, k0 + 5, ... inside it, groups ascending, one fmaf chain per output from `acc`;
//   rows    accumulator element r of lane l is row (r & 3) + 8 (r >> 2) + 4 h, column i.
// Units that include this are compiled WITHOUT fp contraction (build.sh EXACT): sdf_density and sigmoid round op by op as written.
#pragma once

#include "ag_common.h"

#include <cmath>

namespace ag {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mac8(f32x16 acc, const float4 a, const float4 w)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
    return acc;
}

// this lane's first float4 of the weights at `w_off` of `blob`: column n, k = 4 h .. 4 h + 3; group g is `wstep` = 2 Np float4s further each
__device__ __forceinline__ const float4* weights(const float* __restrict__ blob, unsigned w_off, int Np, int n, int h)
{
    return reinterpret_cast<const float4*>(blob + w_off) + (size_t)h * Np + n;
}

// `groups` groups of 8 k; `u`: this lane's row of the input tile in LDS, already at column 4 h.  The same sum with four groups' reads in
// flight (the wide layers of the template field) is field_kernel's own loop in ag_template_field.hip: inlined from a function of this header
// it is scheduled differently and measurably slower ("The shared MLP tile").
__device__ __forceinline__ f32x16 products(f32x16 acc, const float* u, const float4* w, size_t wstep, int groups)
{
    for (int g = 0; g < groups; ++g) acc = mac8(acc, *reinterpret_cast<const float4*>(u + 8 * g), w[g * wstep]);
    return acc;
}

// C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int cd_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// LaplaceDensity of the raw SDF column v (sdf = -v): alpha (0.5 + 0.5 sign(v) expm1(-|v| / b)), alpha = 1 / b
__device__ __forceinline__ float sdf_density(float v, float b, float alpha)
{
    const float sgn = v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
    const float em = expm1f(-fabsf(v) / b);
    return alpha * (0.5f + (0.5f * sgn) * em);
}

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
inline int pad8(int v) { return (v + 7) / 8 * 8; }
inline int pad32(int v) { return (v + 31) / 32 * 32; }

// The point count and the blob size of a call; `what` prefixes the message.  Needs no device, so it stands before the N == 0 return.
inline int check_sizes(const char* what, long long N, long long n_max, size_t blob_floats, size_t total)
{
    if (N < 0 || N > n_max) { set_error("%s: N = %lld must be 0 .. %lld", what, N, n_max); return AG_ERR_INVALID_ARGUMENT; }
    if (blob_floats != total) { set_error("%s: blob of %zu floats, %zu expected for this table", what, blob_floats, total); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

// A blob the kernel will read: the float4 reads of `weights` need 16-byte alignment.
inline int check_blob(const char* what, const float* blob)
{
    if (!blob) { set_error("%s: blob is NULL", what); return AG_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<uintptr_t>(blob) % 16 != 0) { set_error("%s: the blob is not 16-byte aligned", what); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

// Grid of a persistent kernel: a workgroup per tile up to `workgroups_per_cu` x CUs of the current device; the grid-stride loop takes the rest.
inline int persistent_grid(long long n_tiles, int workgroups_per_cu, const char* what, unsigned* grid)
{
    int dev = 0, cus = 0;
    if (int rc = check_hip(hipGetDevice(&dev), what)) return rc;
    if (int rc = check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), what)) return rc;
    const long long cap = (long long)workgroups_per_cu * cus;
    *grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
    return AG_OK;
}

}  // namespace mlp
}  // namespace ag
