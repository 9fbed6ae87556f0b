/*
 * ag_ray_march.h — C ABI of the template stage's ray renderer (libag_hip.so): near / far of camera rays against the posed body, sample
 * placement along the rays and alpha compositing of the field's density and colour.  Together with ag_template_field.h and
 * ag_inverse_skinning.h these are the steps of the reference's TemplateNet.render (network/template.py:288-405).  Forward only.
 *
 * Same conventions as ag_template_field.h: device pointers, fp32, contiguous, 0 on success, ag_last_error() on failure; every refusal
 * happens before any launch; R == 0 returns 0 without a launch; work is only enqueued on `stream`.  No atomics anywhere: every output
 * is a pure function of the inputs and bit-identical between calls.  The file is compiled with -ffp-contract=off: every operation
 * below is ONE rounded fp32 operation in the order written (sums left to right), sqrtf and `/` are correctly rounded.
 *
 * ag_ray_near_far — the reference's utils/posevocab_custom_ops/near_far_smpl_kernel.cu: a ball of `radius` around every vertex.
 *   Per ray (o, d) and vertex c:
 *       a    = d0*d0 + d1*d1 + d2*d2
 *       b    = 2 * (d0*(o0-c0) + d1*(o1-c1) + d2*(o2-c2))
 *       c    = (o0-c0)*(o0-c0) + (o1-c1)*(o1-c1) + (o2-c2)*(o2-c2) - radius*radius
 *       disc = b*b - 4*a*c                                   (4*a is exact)
 *   The vertex is MISSED when (double)disc < 1e-8 (the reference's comparison: its 1e-8 is a double).  Otherwise
 *       near_v = (-b - sqrtf(disc)) / (2*a),   far_v = (-b + sqrtf(disc)) / (2*a).
 *   near = fminf over the hit vertices of near_v, far = fmaxf over them of far_v, hit = 1 when any vertex was hit, else 0.  A ray
 *   that hits nothing takes fallback_near / fallback_far of its index (template.py:308-309), or 0 / 0 when these are NULL (what the
 *   reference kernel writes).  Minimum and maximum are exact, so the result does not depend on how the kernel splits the vertices
 *   over lanes (it chooses the split from R).  near may be negative (origin inside a ball), both may be (ball behind the origin).
 *   One deliberate difference: the reference starts `far` at -1.0, so a ray whose every hit ball ends more than one unit BEHIND its
 *   origin gets far = -1 there and the largest far_v here.  The reference's kernel is CUDA and has not been run: this function is
 *   pinned to the formulas above, not to recorded outputs of the reference.
 *
 * ag_ray_sample — nerf_util.sample_pts_on_rays (utils/nerf_util.py:102-131) and the view directions of template.py:355-356.
 *   `t` [S] is torch.linspace(0, 1, S) in float32, computed by the caller (its values are torch's, bit for bit).  Per ray and s:
 *       z_s = near*(1 - t_s) + far*t_s
 *   With u != NULL, for every ray when perturb_mask == NULL and for the rays whose perturb_mask is not 0 otherwise
 *   (nerf_util.py:119-127; u [R,S] are the caller's random numbers in [0, 1), read for those rays only):
 *       lower_s = s == 0     ? z_0     : .5*(z_s + z_{s-1})
 *       upper_s = s == S - 1 ? z_{S-1} : .5*(z_{s+1} + z_s)
 *       z_s     = lower_s + (upper_s - lower_s)*u_s
 *   pts[r*S + s][a]      = o_a + d_a*z_s
 *   viewdirs[r*S + s][a] = d_a / sqrtf(d0*d0 + d1*d1 + d2*d2)      (when viewdirs != NULL; the same three values for the ray's S samples)
 *
 * ag_ray_composite — template.py:345-346, 372-374 and nerf_util.raw2outputs (nerf_util.py:197-223).  Per ray:
 *       dist_s  = z_{s+1} - z_s for s < S - 1,   dist_{S-1} = z_{S-1} - z_{S-2}
 *       alpha_s = 1 - expf(-density_s*dist_s)                  (the accurate expf; alpha never reaches memory)
 *       f_s     = (1 - alpha_s) + 1e-10f
 *       T_s     = prod_{k<s} f_k,   T_0 = 1
 *       w_s     = alpha_s*T_s
 *       rgb_a = sum_s w_s*color_s[a],   acc = sum_s w_s,   depth = sum_s w_s*z_s
 *       q = depth / acc;   disp = 1 / (q <= 1e-10f ? 1e-10f : q)     (torch.max: q = 0/0 = NaN of a ray with acc = 0 stays NaN, as in the reference)
 *       white_bkgd != 0:   rgb_a = rgb_a + (1 - acc)
 *   ORDER of the product and of the sums (one of the valid fp32 orders, fixed).  The samples are taken in chunks of 64 consecutive
 *   s; position l of a chunk is sample 64*chunk + l; positions past S - 1 hold f = 1 and w = 0.
 *     Product.  Inside a chunk, P_l = f_0 * .. * f_l by six doubling steps, o = 1, 2, 4, 8, 16, 32: every position l >= o replaces its
 *       value p_l by p_{l-o} * p_l (all positions at once, from the values before the step).  E_0 = 1, E_l = P_{l-1}.
 *       T of position l = carry * E_l;  carry = 1 for the first chunk and carry * P_63 for the next one.
 *     Sums.  Inside a chunk the 64 terms are folded by six butterfly steps, o = 32, 16, 8, 4, 2, 1: v_l = v_l + v_{l xor o}; the chunk's
 *       sum is v_0.  total = chunk sum of the first chunk, then total + chunk sum, chunk after chunk.
 *   A ray's outputs depend on that ray's inputs alone: they do not change with R or with how the caller chunks the rays.
 *   color and rgb_map may be NULL together (a field without a colour MLP).
 *
 * Limits.  2 <= S <= 1024 (dist_{S-1} has no meaning for S = 1), 1 <= V, 0 <= R, radius finite and positive.  One call takes at most
 *   2^31 rays (near_far), 2^25 rays and 2^31 samples R * S (sample, composite); R * S * 3 passes 2^31 long before that and every index
 *   is 64-bit.  Anything else returns AG_ERR_INVALID_ARGUMENT with a message before any launch.  Non-finite rays, vertices or
 *   densities are outside the contract (fminf / fmaxf skip a NaN).
 *
 * Kernel shapes (csrc/ag_ray_march.hip).
 *   near_far: workgroups of 256 threads; a ray is owned by a group of G consecutive lanes, G a power of two 1 .. 64 chosen from R so
 *     that R * G fills the chip (G = 64 up to 4096 rays, 1 from 262 144).  The vertices pass through LDS in tiles of 1024 (12 KiB);
 *     lane j of a group tests vertices j, j + G, .. of the tile; the partial minima / maxima / flags are folded across the group's
 *     lanes by cross-lane moves.  The division by 2*a is applied ONCE per ray to the folded numerators: x -> x / (2*a) is monotone
 *     for a fixed positive divisor under correct rounding, so it commutes with the exact minimum and maximum, bit for bit.
 *     Compute bound: about 40 VALU operations per (ray, vertex) test.
 *   sample: one thread per (ray, sample); a workgroup of 256 stages its 768 point floats (and view-direction floats) in LDS and
 *     writes them as contiguous rows.  Memory bound: 28 bytes written per sample (16 without view directions), 4 read with u.
 *   composite: one wavefront per ray, one lane per sample of a chunk: contiguous reads of density, colour and z.  Memory bound:
 *     20 bytes read per sample (+ 4 written with weights).
 */
#ifndef AG_RAY_MARCH_H
#define AG_RAY_MARCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_RAY_MIN_SAMPLES 2
#define AG_RAY_MAX_SAMPLES 1024

/* near [R], far [R], hit [R] (uint8) of R rays against V balls.  fallback_near / fallback_far [R] may both be NULL (0 / 0). */
int ag_ray_near_far(const float* vertices /*[V,3]*/, int32_t V, const float* ray_o /*[R,3]*/, const float* ray_d /*[R,3]*/, int64_t R, float radius,
                    const float* fallback_near /*[R] or NULL*/, const float* fallback_far /*[R] or NULL*/, float* near /*[R]*/, float* far /*[R]*/,
                    uint8_t* hit /*[R]*/, void* stream);

/* z_vals [R,S], pts [R*S,3] and (optionally) viewdirs [R*S,3].  u [R,S] NULL: no perturbation; perturb_mask [R] (uint8) NULL: every ray. */
int ag_ray_sample(const float* ray_o /*[R,3]*/, const float* ray_d /*[R,3]*/, const float* near /*[R]*/, const float* far /*[R]*/, int64_t R,
                  const float* t /*[S]*/, int32_t S, const float* u /*[R,S] or NULL*/, const uint8_t* perturb_mask /*[R] or NULL*/,
                  float* z_vals /*[R,S]*/, float* pts /*[R*S,3]*/, float* viewdirs /*[R*S,3] or NULL*/, void* stream);

/* rgb_map [R,3] (NULL exactly when color is NULL), acc_map [R]; depth_map [R], disp_map [R] and weights [R,S] may each be NULL. */
int ag_ray_composite(const float* density /*[R*S]*/, const float* color /*[R*S,3] or NULL*/, const float* z_vals /*[R,S]*/, int64_t R, int32_t S,
                     int32_t white_bkgd, float* rgb_map /*[R,3] or NULL*/, float* acc_map /*[R]*/, float* depth_map /*[R] or NULL*/,
                     float* disp_map /*[R] or NULL*/, float* weights /*[R,S] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_RAY_MARCH_H */
