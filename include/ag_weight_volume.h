/*
 * ag_weight_volume.h — C ABI of the blend-weight volume sampler (libag_hip.so): trilinear samples of a channel-last
 * [X, Y, Z, C] fp32 volume at N points -> [N, C].
 *
 * It replaces what the reference's CanoBlendWeightVolume.forward_weight / forward_sdf (network/volume.py:72-93,116-130) compute with
 *     F.grid_sample(volume [1, C, X, Y, Z], grid, mode = 'bilinear', padding_mode = 'border', align_corners = True)
 * on a transposed copy of the file's arrays.  Here the volume stays as `cano_weight_volume.npz` stores it: the C values of one grid
 * node are one contiguous row of 4 C bytes.
 * Same conventions as ag_raster.h: device pointers, fp32, contiguous, 0 on success, ag_last_error() on failure.
 */
#ifndef AG_WEIGHT_VOLUME_H
#define AG_WEIGHT_VOLUME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[n, c] for point p = points[n] (p_0 indexes the FIRST volume axis: the reference permutes its grid with [2, 1, 0] because
 * grid_sample's x runs along the last one).  fp32, every operation rounded on its own, in this order, no contraction; R = (X, Y, Z):
 *
 *   per axis d:   u = (p_d - lo_d) / (hi_d - lo_d)             only with bounds (requires_scale); u = p_d without
 *                 g = 2 * u - 1
 *                 x = ((g + 1) / 2) * (R_d - 1)                 grid_sample's un-normalisation with align_corners
 *                 x = min(max(x, 0), R_d - 1)                   padding_mode 'border'; a NaN coordinate samples node 0
 *                 i_d = floor(x),  f_d = x - i_d,  e_d = (i_d + 1) - x              both differences are exact
 *   corner k = 0 .. 7 with (a, b, c) = (k >> 2, (k >> 1) & 1, k & 1):
 *                 w_k = ((c ? f_2 : e_2) * (b ? f_1 : e_1)) * (a ? f_0 : e_0)
 *                 acc = acc + w_k * volume[i_0 + a, i_1 + b, i_2 + c, :]            from acc = 0, k ascending
 *   A corner whose index is R_d on some axis is skipped: it exists only for x = R_d - 1, where its weight is 0.
 *
 * The product and corner order are those of ATen's grid_sampler_3d (its tnw, tne, tsw, tse, bnw, ... corners).
 * No atomics and no reduction across threads: out is a pure function of the inputs, bit-identical between calls.
 *
 * X, Y, Z >= 2 (AG_ERR_INVALID_ARGUMENT otherwise: R_d - 1 = 0 has no cell to interpolate in), C >= 1, N >= 0 (N = 0 launches
 * nothing).  Element offsets are 64-bit: X * Y * Z * C and N * C may exceed 2^31; N * C < 2^39 (one thread per output, 256 per block).
 * `bounds`: HOST pointer to lo[3], hi[3], or NULL for points already in [0, 1] (requires_scale = False).
 * The volume is read only; `out` must not overlap it or `points`.
 */
int ag_weight_volume_sample(const float* volume /*[X,Y,Z,C]*/, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* points /*[N,3]*/,
                            int64_t N, const float* bounds /*host [2,3] or NULL*/, float* out /*[N,C]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_WEIGHT_VOLUME_H */
