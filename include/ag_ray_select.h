/*
 * ag_ray_select.h — C ABI of the template stage's ray selection (libag_hip.so): from a frame on the device, a camera and the posed
 * bounding box to the pixel lists a batch is drawn from and to the rays, box near / far and targets of the drawn pixels.
 *
 * It replaces what the reference computes in numpy inside its loader workers (utils/nerf_util.py):
 *   get_bound_2d_mask :35-46     the box's image-space mask           -> ag_ray_classify
 *   uv_img[mask]      :279-281   the inside / outside candidate lists -> ag_ray_classify + ag_ray_compact
 *   get_rays          :83-99     a ray per pixel                      -> ag_ray_build
 *   get_near_far      :49-80     the ray against the padded box       -> ag_ray_build, ag_ray_box_near_far (+ ag_ray_compact of `hit`)
 *   the gather of color_gt / mask_gt / depth_gt and `dist` :305-314   -> ag_ray_build
 * Same conventions as ag_raster.h: device pointers, contiguous, 0 on success, ag_last_error() on failure.  Every output is a pure
 * function of the inputs: no atomics, no order that depends on scheduling, bit-identical between calls.  All kernels are wave64.
 * A count of 0 launches nothing and succeeds.
 */
#ifndef AG_RAY_SELECT_H
#define AG_RAY_SELECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- classify --------------------------------------------------------------------------------------------------------------------
 * corners_xy: the eight corners of the box in get_bound_corners' order (corner i = (x: bit 2, y: bit 1, z: bit 0 of i; 0 = min,
 * 1 = max)), projected BY THE CALLER in float64 as nerf_util.project does and rounded with np.round (half to even), as
 * (x0, y0, x1, y1, ...), passed by value (a host pointer to 16 integers).  |coordinate| <= 2^29.
 *
 * For the pixel (x, y), 0 <= x < W, 0 <= y < H, and a quad (v0, v1, v2, v3) with v4 = v0, in int64:
 *   e_i = (v_{i+1}.x - v_i.x) * (y - v_i.y) - (v_{i+1}.y - v_i.y) * (x - v_i.x)          i = 0 .. 3
 *   in_quad = (all e_i >= 0 or all e_i <= 0)  and  min_i v_i.x <= x <= max_i v_i.x  and  min_i v_i.y <= y <= max_i v_i.y
 * the closed quad in either winding.  The bounding-box term is implied for a convex quad with area; for a quad that degenerated to a
 * segment or a point (every e_i is 0 along the whole line then) it keeps the segment and drops the rest of its line.
 *   bound = in_quad of any of the six faces  [0,1,3,2] [4,5,7,6] [0,1,5,4] [2,3,7,6] [0,2,6,4] [1,3,7,5]
 * THIS RULE IS THE PROJECT'S OWN DEFINITION of what the reference draws with cv2.fillPoly on these integer vertices.  OpenCV was
 * never run beside it: parity with its scan conversion (which pixels of a quad's boundary it sets) is not pinned.
 *
 *   cls_u8[y W + x] = 0  where !bound, or where unsample_u8 is given and non-zero there
 *                     1  else where mask_u8 is NULL or non-zero there  ("inside": a candidate on the subject's matte)
 *                     2  else                                          ("outside")
 * mask_u8 / unsample_u8: [H, W] bytes (a bool image as it lies in memory), either may be NULL.
 * AG_ERR_INVALID_ARGUMENT: a null corners_xy or cls_u8, H or W <= 0, H * W > 2^31 - 1, a coordinate beyond 2^29.
 */
int ag_ray_classify(const int32_t* corners_xy /*host [16]*/, int32_t H, int32_t W, const uint8_t* mask_u8, const uint8_t* unsample_u8,
                    uint8_t* cls_u8 /*[H,W]*/, void* stream);

/*
 * ---- ordered compaction ----------------------------------------------------------------------------------------------------------
 * list1 = the ascending indices i of flags_u8[i] == 1, list2 (may be NULL) those of flags_u8[i] == 2, as int32: np.flatnonzero of each
 * class, the order in which uv_img[mask] enumerates a row-major image.  counts_i32[0 .. 1] = their lengths, written on the device
 * (counts_i32[1] = 0 without list2).  list1 / list2 must hold n entries each; entries past the count are not written.
 * Three launches: every wave counts the two classes of its run of 512 flags with ballots; one workgroup turns the counts into
 * exclusive offsets (in place, in the workspace) and writes counts_i32; every wave walks its run again and stores index i at
 * offset + popcount of the ballot's lower lanes.  The workspace must not be shared with a call in flight on another stream.
 * AG_ERR_INVALID_ARGUMENT: a null flags_u8, list1, counts_i32 or workspace, n < 0 or n > 2^31 - 1, workspace_bytes below the query.
 */
size_t ag_ray_compact_workspace_bytes(int64_t n);
int ag_ray_compact(const uint8_t* flags_u8 /*[n]*/, int64_t n, int32_t* list1, int32_t* list2, int32_t* counts_i32 /*[2]*/, void* workspace,
                   size_t workspace_bytes, void* stream);

/*
 * ---- build -----------------------------------------------------------------------------------------------------------------------
 * The camera, by value.  inv_intr = inv(intr), inv_rot = inv(extr)[:3, :3], cam = inv(extr)[:3, 3]: formed by the caller in float64
 * (np.linalg.inv) and rounded ONCE to float32; row-major.  fx, fy, cx, cy = intr[0,0], intr[1,1], intr[0,2], intr[1,2] as float32.
 * bounds = (min x, y, z, max x, y, z) of the posed box as float32, NOT padded.
 */
typedef struct AgRayCamera {
    float inv_intr[9];
    float inv_rot[9];
    float cam[3];
    float fx, fy, cx, cy;
    float bounds[6];
    int32_t W, H;
} AgRayCamera;
size_t ag_ray_camera_bytes(void);

/*
 * Entry k of n takes its pixel from ONE of
 *   pix_i32[k] = y W + x                        a pixel list (ag_ray_compact's, or a selection of it)
 *   uv_in_i32[2 k], uv_in_i32[2 k + 1] = x, y   explicit coordinates, any integers; no image may be given then and W, H are not used
 *   neither: k itself = y W + x, all W H pixels in row-major order; n must equal W H.
 * A pix_i32 entry outside [0, W H) is a miss: hit = 0 and every other output of the entry 0; nothing is read for it.
 *
 * Every operation below is ONE rounded IEEE float32 operation (no contraction; `/` and sqrt correctly rounded), sums are taken left to
 * right as written, constants carry the suffix they are rounded with.  K = inv_intr, R = inv_rot, c = cam, fl() = int -> float32.
 *
 *   get_rays.  The pixel enters WITHOUT + 0.5:  X = fl(x), Y = fl(y)
 *     p_i = (K[i][0] * X + K[i][1] * Y) + K[i][2]                                 i = 0, 1, 2   (the third coordinate is 1: K[i][2] * 1)
 *     w_i = ((R[i][0] * p_0 + R[i][1] * p_1) + R[i][2] * p_2) + c_i
 *     g_i = w_i - c_i
 *     l   = sqrt((g_0 * g_0 + g_1 * g_1) + g_2 * g_2)
 *     ray_d_i = g_i / (l + 1e-8f)                 ray_o = c
 *
 *   get_near_far (o = ray_o, d = ray_d; ag_ray_box_near_far starts here with the caller's o, d).
 *     lo_a = bounds[a] - 0.01f,  hi_a = bounds[3 + a] + 0.01f                     a = 0, 1, 2
 *     the six planes in the order b = (lo_0, lo_1, lo_2, hi_0, hi_1, hi_2), plane j on axis a = j mod 3:
 *     t_j   = (b_j - o_a) / (d_a + 1e-9f)
 *     q_j,i = t_j * d_i + o_i                                                     i = 0, 1, 2  (a product, then a sum)
 *     in_j  = for all i:  q_j,i >= lo_i - 1e-6f  and  q_j,i <= hi_i + 1e-6f      (false for a NaN)
 *     hit   = EXACTLY two of the six in_j hold.  A ray through an edge or a corner of the box passes three or more and is dropped, as
 *             in the reference.
 *     with j0 < j1 the two planes that pass:
 *     n   = sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2)
 *     s_m = sqrt(((q_jm,0 - o_0)^2 + (q_jm,1 - o_1)^2) + (q_jm,2 - o_2)^2) / n    m = 0, 1
 *     near = min(s_0, s_1), far = max(s_0, s_1);  near = far = 0 where !hit.
 *
 *   targets (only with color_img AND mask_u8; all four outputs are required then):
 *     m = mask_u8[y, x] != 0;  mask_gt = m ? 1.0f : 0.0f;  color_gt = m ? color_img[y, x, :] : 0;  depth_gt = depth_img ? depth_img[y, x] : 0
 *     dist uses the pixel WITH + 0.5:
 *     ex = ((X + 0.5f) - cx) * depth_gt / fx,  ey = ((Y + 0.5f) - cy) * depth_gt / fy     (left to right: a product, then a quotient)
 *     dist = sqrt((ex * ex + ey * ey) + depth_gt * depth_gt)
 *
 * Outputs, any of which may be NULL (near, far and hit: all three or none; the box test is skipped without them):
 *   uv_i32 [n, 2] = (x, y), ray_o [n, 3], ray_d [n, 3], near [n], far [n], hit_u8 [n] (0 / 1),
 *   color_gt [n, 3], mask_gt [n], depth_gt [n], dist [n].
 * AG_ERR_INVALID_ARGUMENT: a null camera, n < 0 or n > 2^31 - 1, both pix_i32 and uv_in_i32, images with uv_in_i32, neither with
 * n != W H, W or H <= 0 where they are used, exactly one of color_img / mask_u8, a depth_img without them, a target output that is
 * null with images or given without, some but not all of near / far / hit_u8.
 */
int ag_ray_build(const AgRayCamera* camera, const int32_t* pix_i32, const int32_t* uv_in_i32, int64_t n, const float* color_img /*[H,W,3]*/,
                 const uint8_t* mask_u8 /*[H,W]*/, const float* depth_img /*[H,W] or NULL*/, int32_t* uv_i32, float* ray_o, float* ray_d, float* near,
                 float* far, uint8_t* hit_u8, float* color_gt, float* mask_gt, float* depth_gt, float* dist, void* stream);

/* get_near_far alone, for rays the caller holds: bounds = host pointer to (min x, y, z, max x, y, z), not padded; ray_o, ray_d [n, 3];
 * near, far [n] and hit_u8 [n] as above, all required. */
int ag_ray_box_near_far(const float* bounds /*host [6]*/, const float* ray_o, const float* ray_d, int64_t n, float* near, float* far,
                        uint8_t* hit_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_RAY_SELECT_H */
