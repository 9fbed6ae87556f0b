/*
 * ag_targets.h — C ABI of the training-target kernel (libag_hip.so): from a decoded uint8 frame and its uint8 matte to the three
 * images the loss tail reads (float colour, the subject mask, the boundary band) and the mask's row / column profiles.
 *
 * It replaces what the reference's loader computes on host arrays, per view and per step:
 *   color_img = (color_img / 255.).astype(np.float32)                         dataset/dataset_mv_rgb.py:185
 *   get_boundary_mask(mask, kernel_size = 5): threshold, cv.erode, cv.dilate   dataset/dataset_mv_rgb.py:263-285
 * Same conventions as ag_raster.h: device pointers, contiguous, 0 on success, ag_last_error() on failure.
 * Every output is a pure function of the inputs: no atomics on global memory, bit-identical between calls.
 */
#ifndef AG_TARGETS_H
#define AG_TARGETS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * With k = kernel_size, r = k / 2 and m = matte_u8[v, y, x]:
 *
 *   class      c = 0 if m < 128,  1 if m > 128,  128 if m == 128       the reference's two assignments (`mask[mask < 128] = 0`,
 *                                                                      `mask[mask > 128] = 1`) leave a matte of exactly 128 as it is
 *   mask_u8    = (c == 1)
 *   window     emin, emax = minimum and maximum of c over the k x k window centred on the pixel, CLIPPED TO THE IMAGE: pixels outside
 *              take part in neither (OpenCV's default border value for erode / dilate), so an all-255 matte has an empty band
 *   boundary_u8 = (uint8(emax - emin) == 1) || (5 < m && m < 250)
 *              the reference subtracts in uint8; with the three classes the first term holds exactly when the window contains a 1 and a
 *              0 and no 128
 *   color_f32  = float(color_u8) / 255.0f, one correctly rounded IEEE fp32 division per element.  For all 256 inputs this equals the
 *              reference's float64 division rounded to float32; a multiplication by 1 / 255.f does not (126 of the 256 differ in the
 *              last bit).  Channel order is kept (the reference keeps cv.imread's BGR).
 *   row_any_u8[v, y] = 1 iff any mask_u8[v, y, :] is set, col_any_u8[v, x] = 1 iff any mask_u8[v, :, x] is: what a bounding box of
 *              the mask needs on the host, H + W bytes per view.  Both are cleared on `stream` before the launch.
 *              Pass BOTH as NULL to skip them.
 *   color_u8 and color_f32 may likewise BOTH be NULL: mask, band and profiles only, for a caller that already holds float colour.
 *
 * mask_u8 and boundary_u8 hold 0 or 1.  One launch for all V views.  Nothing is read or written outside the extents below, whatever
 * the alignment of the pointers and whether W or H * W is odd (color_f32 must be aligned to 4 bytes, as a float is).
 * An output must not overlap an input or another output.
 *
 * AG_ERR_INVALID_ARGUMENT: a null matte_u8, mask_u8 or boundary_u8, exactly one of color_u8 / color_f32 or of row_any_u8 / col_any_u8
 * given, V, H or W <= 0, V or ceil(H / 16) > 65535, kernel_size even or outside [1, 15], color_f32 not aligned to 4 bytes.
 */
int ag_prepare_targets(const uint8_t* color_u8 /*[V,H,W,3]*/, const uint8_t* matte_u8 /*[V,H,W]*/, int32_t V, int32_t H, int32_t W,
                       int32_t kernel_size, float* color_f32 /*[V,H,W,3]*/, uint8_t* mask_u8 /*[V,H,W]*/, uint8_t* boundary_u8 /*[V,H,W]*/,
                       uint8_t* row_any_u8 /*[V,H] or NULL*/, uint8_t* col_any_u8 /*[V,W] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_TARGETS_H */
