/*
 * ag_weight_diffuse.h — C ABI of the blend-weight diffusion (libag_hip.so): the discrete harmonic extension of the values on a set
 * of FIXED nodes of a channel-last [X, Y, Z, C] fp32 grid into all the others, by matrix-free conjugate gradients.
 *
 * This is the project's own definition of `diff_weight_volume`.  The reference obtains that array from an external program
 * (gen_data/gen_weight_volume.py:64-74,114-135, PointInterpolant.exe: values and gradients fitted with B-splines on an adaptive
 * octree); nothing here reproduces that program and no equality with its output is claimed.
 *
 * The operator.  Node spacings h_k, weights w_k = (h_min / h_k)^2 (a cubic grid has w = 1, 1, 1).  For a node n that is NOT fixed
 *
 *     d_k         = (u[n, c] - u[lower neighbour on axis k, c]) + (u[n, c] - u[upper neighbour on axis k, c])
 *     (A u)[n, c] = (w_x * d_x + w_y * d_y) + w_z * d_z
 *
 * and (A u)[n, c] = 0 for a fixed node.  A neighbour outside the grid is dropped (zero flux through the cube's faces): it is read
 * as the node itself, whose difference is an exact 0 for finite values.  Neighbours are read as they are given, fixed or not.
 * fp32, each difference, product and sum rounded on its own, in the order written.
 *
 * The solve.  With u0 = target on the fixed nodes and 0 elsewhere, b = -A u0, and A_ff the operator on vectors that vanish on the
 * fixed nodes (symmetric positive definite as soon as one node is fixed), every channel c runs its own conjugate gradients on
 * A_ff x_c = b_c from x = 0, in lockstep with the others and with its own scalars:
 *
 *     alpha_c = rr_c / (p_c . A p_c)      x_c += alpha_c p_c      r_c -= alpha_c A p_c
 *     beta_c  = rr_c' / rr_c              p_c  = r_c + beta_c p_c           rr_c = r_c . r_c
 *
 * A zero denominator gives alpha_c = 0 (beta_c = 0): a channel with b_c = 0 stays exactly zero and no NaN arises from one.
 * x, r, p and A p are zero on the fixed nodes throughout; the caller assembles u = target on fixed nodes, x elsewhere.
 *
 * Every per-channel sum is taken in a fixed order (per lane, then per workgroup through LDS, then over the workgroups' partial sums
 * in the workspace by a finishing kernel that also forms alpha and beta on the device): no floating-point atomics, and two calls on
 * the same inputs give bit-identical results.  No call synchronises with the host; the scalars stay on the device.
 *
 * Same conventions as ag_weight_volume.h: device pointers, fp32, contiguous, 0 on success, AG_ERR_INVALID_ARGUMENT with
 * ag_last_error() text otherwise.  X, Y, Z >= 2, C >= 1, X * Y * Z < 2^31 nodes; ELEMENT offsets are 64-bit (X * Y * Z * C may
 * exceed 2^31).  `fixed` is one byte per node, non-zero = fixed.  `w` is a HOST pointer to the three weights, each in (0, 1].
 * No two of the arrays of one call may overlap.
 */
#ifndef AG_WEIGHT_DIFFUSE_H
#define AG_WEIGHT_DIFFUSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the device workspace of init / iterate (the workgroups' partial sums and alpha, beta); 0 for sizes the calls refuse. */
size_t ag_weight_diffuse_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t C);

/* out = A in (the operator alone; out is written on every node, 0 on the fixed ones). */
int ag_weight_diffuse_apply(const float* in /*[X,Y,Z,C]*/, const uint8_t* fixed /*[X,Y,Z]*/, int32_t X, int32_t Y, int32_t Z, int32_t C,
                            const float* w /*host [3]*/, float* out /*[X,Y,Z,C]*/, void* stream);

/*
 * x = 0, r = p = b = -A u0, bb[c] = rr[c] = b_c . b_c.  `ap` is scratch (it holds A u0 afterwards); x, r, p, ap are [X,Y,Z,C].
 * bb and rr are device vectors of C floats.
 */
int ag_weight_diffuse_init(const float* target /*[X,Y,Z,C]*/, const uint8_t* fixed, int32_t X, int32_t Y, int32_t Z, int32_t C,
                           const float* w /*host [3]*/, float* x, float* r, float* p, float* ap, void* workspace, size_t workspace_bytes,
                           float* bb /*[C]*/, float* rr /*[C]*/, void* stream);

/* Enqueue n >= 0 iterations on the state init left (or an earlier iterate); rr[c] = r_c . r_c of the recurrence after the last. */
int ag_weight_diffuse_iterate(const uint8_t* fixed, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* w /*host [3]*/, int32_t n,
                              float* x, float* r, float* p, float* ap, void* workspace, size_t workspace_bytes, float* rr /*[C]*/,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_WEIGHT_DIFFUSE_H */
