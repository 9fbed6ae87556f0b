/*
 * ag_metrics.h — C ABI of the image-quality kernels (libag_hip.so): the squared error and the structural similarity (SSIM) of two
 * image batches in ONE pass over both, for the PSNR / SSIM figures of the reference's eval/score.py:101-108.
 *
 * Same conventions as ag_raster.h: device pointers, contiguous, 0 on success, ag_last_error() on failure.
 *
 * SSIM is skimage.metrics.structural_similarity restated.  Per channel, with a separable window of w = 2p + 1 taps k (sum 1):
 *     ux = k*x, uy = k*y, uxx = k*(x.x), uyy = k*(y.y), uxy = k*(x.y)                 (k* = the 2-D window mean, k (x) k)
 *     vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy)
 *     S  = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2))
 * evaluated at the centres that are at least p from every border (scikit-image filters the border with reflection and then crops
 * exactly those pixels, so only whole windows are ever evaluated and no border rule exists here).  cn, C1 = (K1 R)^2 and
 * C2 = (K2 R)^2 come from the caller.
 *
 * Arithmetic: the inputs are fp32; every product, window sum and S itself are fp64 (a product of two fp32 values is exact in fp64),
 * so the map deviates from the fp64 definition by its own rounding to fp32 only.  The squared error converts both operands to
 * fp64 BEFORE subtracting, as scikit-image's mean_squared_error does.
 *
 * Reduction: one workgroup owns an AG_METRICS_TILE_H x AG_METRICS_TILE_W block of centres of one image (all channels) and, for the
 * squared error, the pixels under those centres (border tiles also own the p-wide border beside them).  It reduces through the
 * wave and the workgroup in a fixed order and writes ONE fp64 pair; a second launch adds each image's pairs in a fixed order
 * (thread t takes pairs t, t + 256, ... in index order, then the same wave / workgroup reduction).  No float atomic: the sums
 * are pure functions of the inputs (bit-identical between runs and between batch sizes).
 */
#ifndef AG_METRICS_H
#define AG_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_METRICS_TILE_H 16
#define AG_METRICS_TILE_W 32
#define AG_METRICS_MAX_TAPS 11

/* Bytes of the per-workgroup partial sums for a [B, H, W, *] pair and a window of n_taps; 0 when the sizes are not admitted. */
size_t ag_psnr_ssim_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_taps);

/*
 * x, y [B, H, W, C] fp32, C in 1..4.  taps: HOST array of n_taps doubles (n_taps odd, 3..11), read before the call returns.
 * sq_err_sum[b] = sum over all H W C elements of ((double)x - (double)y)^2; ssim_sum[b] = sum of S over the (H - 2p)(W - 2p) C
 * centres (the caller divides).  ssim_map: [B, H - 2p, W - 2p, C] fp32 or NULL.
 * AG_ERR_INVALID_ARGUMENT for H < n_taps, W < n_taps, C outside 1..4, an even n_taps or one outside 3..11; B = 0 launches nothing.
 */
int ag_psnr_ssim(const float* x, const float* y, int32_t B, int32_t H, int32_t W, int32_t C, const double* taps, int32_t n_taps,
                 double cov_norm, double C1, double C2, double* sq_err_sum /*[B]*/, double* ssim_sum /*[B]*/, float* ssim_map,
                 void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_METRICS_H */
