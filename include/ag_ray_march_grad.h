/*
 * ag_ray_march_grad.h — C ABI of the reverse pass of the template stage's ray renderer (libag_hip.so): the gradient of
 * ag_ray_composite (ag_ray_march.h) with respect to density and colour, LaplaceDensity (network/density.py:22-36) of a signed distance
 * with beta read on the device, and its gradient with respect to the signed distance and beta.  Together they carry the gradients of a
 * training step's colour and mask losses (main_template.py:37-51) from rgb_map / acc_map to the field's outputs sdf, color and to beta.
 *
 * Same conventions as ag_ray_march.h: device pointers, fp32, contiguous, 0 on success, ag_last_error() on failure; every refusal
 * happens before any launch; work is only enqueued on `stream`.  No atomics, no LDS, no scratch: every output is a pure function of
 * the inputs and bit-identical between calls.  The file is compiled with -ffp-contract=off: every operation below is ONE rounded
 * fp32 operation in the order written (sums and products left to right), `/` is correctly rounded, expf / expm1f are the accurate ones.
 *
 * ag_ray_composite_backward.  Per ray, with the forward's quantities (ag_ray_march.h; csrc/ag_ray_scan.h states their order once for
 *   both kernels, so T_s and w_s are the forward's bit for bit):
 *       dist_s, e_s = expf(-density_s*dist_s), alpha_s = 1 - e_s, f_s = (1 - alpha_s) + 1e-10f, T_s, w_s = alpha_s*T_s
 *   and the upstream gradients G_rgb[3], G_acc, G_depth, G_w[S] (a NULL pointer is a gradient of +0 and goes through the same
 *   arithmetic, so a gradient given alone equals the same call with zeros for the others, bit for bit):
 *       G_acc' = white_bkgd ? G_acc - ((G_rgb[0] + G_rgb[1]) + G_rgb[2]) : G_acc
 *       g_s    = G_rgb[0]*color_s[0] + G_rgb[1]*color_s[1] + G_rgb[2]*color_s[2] + G_acc' + G_depth*z_s + G_w[s]
 *       B_{S-1} = 0,   B_s = alpha_{s+1}*g_{s+1} + f_{s+1}*B_{s+1}
 *       grad_density_s  = T_s*(g_s - B_s) * dist_s * e_s                (T_s*(g_s - B_s) is dL/dalpha_s)
 *       grad_color_s[a] = w_s*G_rgb[a]
 *   This is the derivative of the forward's text: dL/dalpha_s = g_s*T_s - (1/f_s) * sum_{j>s} g_j*alpha_j*T_j, and the sum divided by
 *   f_s is T_s*B_s.  No division: torch's cumprod derivative divides by f_s, which is 1e-10 wherever a sample saturates (alpha = 1).
 *   There is no gradient to z_vals (the sample positions carry no parameters) and none through disp_map (no loss reads it).
 *   ORDER of the reverse recurrence.  Sample s carries the affine map M_s(x) = f_s*x + alpha_s*g_s, so B_s = M_{s+1}(B_{s+1}).  The
 *   samples are taken in the forward's chunks of 64, back to front; positions past S - 1 hold the identity (f = 1, alpha = 0).
 *     Inside a chunk, Q_l = M_l o M_{l+1} o .. o M_63 as a pair (A_l, C_l), Q_l(x) = A_l*x + C_l, by six doubling steps o = 1, 2, 4, 8,
 *       16, 32: every position l < 64 - o replaces its pair by  C_l = A_l*C_{l+o} + C_l,  A_l = A_l*A_{l+o}  (all positions at once,
 *       from the values before the step; C first, from the A before the step).
 *     With `in` the B of the chunk's last position (0 for the last chunk):  B_63 = in,  B_l = A_{l+1}*in + C_{l+1} for l < 63.
 *     The previous chunk's `in` is A_0*in + C_0.
 *   For S > 64 the forward carries of the chunks (at most 16) are formed first, by the forward's product scan chunk after chunk, and
 *   kept one per lane; density and z_vals are read twice then.
 *   color and g_rgb_map go together (both or neither); grad_color needs both.  At least one of grad_density / grad_color is asked for.
 *   With every upstream pointer NULL the kernel writes +0 to every output element.  A ray's gradients depend on that ray's inputs
 *   alone.  Limits and refusals are ag_ray_composite's: 2 <= S <= 1024, at most 2^25 rays and 2^31 samples, 64-bit indices, R == 0
 *   returns 0 without a launch.  Non-finite inputs are outside the contract.
 *
 * ag_laplace_density.  density_n = sdf_density(-sdf_n, b, 1/b) of csrc/ag_mlp_tile.h, the routine of the fused field, with
 *       b = fabsf(beta[0]) + 1e-4f                                     (LaplaceDensity.get_beta, formed in the kernel: no host read)
 *   so for the same sdf bits it equals the density of ag_template_field_forward bit for bit.  With v = -sdf (the raw network column):
 *       sgn = v > 0 ? 1 : (v < 0 ? -1 : 0),   density = (1/b) * (0.5 + (0.5*sgn)*expm1f(-|v|/b)).
 *
 * ag_laplace_density_backward.  Elementwise, with ex = expf(-|v|/b), inv = 1/b and density as above:
 *       grad_sdf_n = g_n * ((sgn*sgn*ex) / ((2*b)*b))                  (0 at sdf == 0 exactly, as torch's sign / abs give)
 *       term_n     = g_n * (-density/b + (((inv*0.5)*sgn)*ex)*|v| / (b*b))            (g_n * d density / d b)
 *       grad_beta  = sign(beta[0]) * (float)(sum_n term_n),  sign(0) = 0
 *   ORDER of the sum.  Elements are taken in groups of 64 consecutive n (positions past N - 1 hold 0); a group's 64 terms are folded by
 *   the fp32 butterfly of ag_ray_march.h (o = 32 .. 1, v_l = v_l + v_{l xor o}): the only fp32 summation.  Everything after it is
 *   float64 in index order: a wavefront owns AG_LAPLACE_GROUPS_PER_WAVE = 8 consecutive groups and adds their sums to 0.0 in index
 *   order (one float64 partial per 512 elements, in the workspace); a second launch of one wavefront splits the W = ceil(N / 512)
 *   partials into 64 consecutive runs of ceil(W / 64), adds each run to 0.0 in index order, then adds the 64 run sums to 0.0 in
 *   index order.  No float atomics: two calls give the same bits.  N == 0 writes grad_beta = +0 (one launch) and nothing else.
 *   workspace: ag_laplace_density_backward_workspace_bytes(N) = 8 * max(1, ceil(N / 512)) bytes, 8-byte aligned, needed only with
 *   grad_beta.  At least one of grad_sdf / grad_beta is asked for.  0 <= N <= 2^33.
 *
 * Kernel shapes (csrc/ag_ray_march_grad.hip).
 *   composite backward: one wavefront per ray, four rays per workgroup, one lane per sample of a chunk, like the forward: contiguous
 *     reads of density, colour, z and G_w, contiguous writes.  Memory bound: 24 bytes read and 16 written per sample with every
 *     gradient (20 + 16 without G_w).
 *   density: one thread per element, 4 bytes read and 4 written.  density backward: 8 bytes read and 4 written per element.
 */
#ifndef AG_RAY_MARCH_GRAD_H
#define AG_RAY_MARCH_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_LAPLACE_GROUPS_PER_WAVE 8

/* grad_density [R*S] and grad_color [R*S,3] from the upstream gradients of rgb_map [R,3], acc_map [R], depth_map [R], weights [R,S]. */
int ag_ray_composite_backward(const float* density /*[R*S]*/, const float* color /*[R*S,3] or NULL*/, const float* z_vals /*[R,S]*/, int64_t R,
                              int32_t S, int32_t white_bkgd, const float* g_rgb_map /*[R,3] or NULL*/, const float* g_acc_map /*[R] or NULL*/,
                              const float* g_depth_map /*[R] or NULL*/, const float* g_weights /*[R,S] or NULL*/, float* grad_density /*[R*S] or NULL*/,
                              float* grad_color /*[R*S,3] or NULL*/, void* stream);

/* density [N] of sdf [N] (positive inside) with b = |beta[0]| + 1e-4 formed on the device. */
int ag_laplace_density(const float* sdf /*[N]*/, int64_t N, const float* beta /*[1]*/, float* density /*[N]*/, void* stream);

size_t ag_laplace_density_backward_workspace_bytes(int64_t N);

/* grad_sdf [N] and grad_beta [1] from g_density [N]. */
int ag_laplace_density_backward(const float* sdf /*[N]*/, const float* g_density /*[N]*/, int64_t N, const float* beta /*[1]*/,
                                float* grad_sdf /*[N] or NULL*/, float* grad_beta /*[1] or NULL*/, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_RAY_MARCH_GRAD_H */
