/*
 * ag_inverse_skinning.h — C ABI of inverse skinning (libag_hip.so): posed point -> canonical point through the blend-weight volume.
 *
 * It replaces what the reference's TemplateNet.transform_live2cano (network/template.py:226-286) runs on the device: the inverse of
 * the blended joint matrix as the initial guess (:247-253), then damped Newton steps through the weight volume and its Sobel
 * gradient (utils/root_finding/root_finding.cu:43-154, network/volume.py:9-39).  The volume stays channel-last [X, Y, Z, J] as
 * `cano_weight_volume.npz` stores it (include/ag_weight_volume.h): the J values of one grid node are one contiguous row.
 *
 * Same conventions as ag_raster.h: device pointers unless marked HOST, fp32, contiguous, 0 on success, ag_last_error() on failure.
 * Element offsets are 64-bit.  Every function is stated as fp32 operations, each rounded on its own, in the order written (no
 * contraction; the file is compiled with -ffp-contract=off).  No atomics: every output is a pure function of the inputs and
 * bit-identical between calls.  A joint matrix A_j is read as its top three rows (12 floats of the 16): a[r][c], r < 3, c < 4.
 */
#ifndef AG_INVERSE_SKINNING_H
#define AG_INVERSE_SKINNING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[x, y, z, c, d] = the 3x3x3 Sobel derivative of channel c along axis d at node (x, y, z): compute_gradient_volume
 * (network/volume.py:9-39; the layout is the reference's [X, Y, Z, J * 3], joint-major).  A node outside the grid counts as 0
 * (conv3d's padding = 1).  ATen's convolution has no stated summation order; this is ours.  With v(a, b, c) the value at
 * (x - 1 + a, y - 1 + b, z - 1 + c), or 0 outside, a, b, c in {0, 1, 2}, and k_d = 1 / (32 * spacing_d):
 *
 *   along z:   t(a, b) = (v(a, b, 0) + 2 * v(a, b, 1)) + v(a, b, 2)          q(a, b) = v(a, b, 2) - v(a, b, 0)
 *   along y:   s(a) = (t(a, 0) + 2 * t(a, 1)) + t(a, 2)      e(a) = t(a, 2) - t(a, 0)      r(a) = (q(a, 0) + 2 * q(a, 1)) + q(a, 2)
 *   out_0 = (s(2) - s(0)) * k_0
 *   out_1 = ((e(0) + 2 * e(1)) + e(2)) * k_1
 *   out_2 = ((r(0) + 2 * r(1)) + r(2)) * k_2
 *
 * (the products by 2 are exact).  In exact arithmetic this is the reference's filter: smoothing weights 1-2-1 x 1-2-1 on the two
 * other axes, central difference, divided by 32 * spacing_d.
 * X, Y, Z >= 2 and 1 <= C <= 128 (AG_ERR_INVALID_ARGUMENT otherwise), spacing_d finite and positive.  X * Y * Z * C < 2^39 (one
 * thread per (node, channel), 256 per block).  `spacing`: HOST pointer to the three node spacings.  `out` must not overlap `volume`.
 */
int ag_weight_volume_gradient(const float* volume /*[X,Y,Z,C]*/, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* spacing /*host [3]*/,
                              float* out /*[X,Y,Z,C,3]*/, void* stream);

/*
 * The initial guess (template.py:247-253), per point n of batch b, with w = weights[b, n, :], p = points[b, n], A_j = jnt_mats[b, j]:
 *
 *   m[r][c] = m[r][c] + w_j * a_j[r][c]                       from 0, j ascending; the 12 entries of the top three rows
 *   R = m[:, :3], t = m[:, 3]
 *   d = m00*m11*m22 - m00*m12*m21 - m01*m10*m22 + m01*m12*m20 + m02*m10*m21 - m02*m11*m20         left to right
 *   adj = [[ (m11*m22 - m12*m21), -(m01*m22 - m02*m21),  (m01*m12 - m02*m11)],
 *          [-(m10*m22 - m12*m20),  (m00*m22 - m02*m20), -(m00*m12 - m02*m10)],
 *          [ (m10*m21 - m11*m20), -(m00*m21 - m01*m20),  (m00*m11 - m01*m10)]]
 *   inv = adj * (1.f / d)                                     one reciprocal, nine products
 *   s_r = -((inv[r][0]*t_0 + inv[r][1]*t_1) + inv[r][2]*t_2)                                       the translation -R^-1 t
 *   out_points_r  = ((inv[r][0]*p_0 + inv[r][1]*p_1) + inv[r][2]*p_2) + s_r
 *   out_normals_r =  (inv[r][0]*n_0 + inv[r][1]*n_1) + inv[r][2]*n_2                               only with normals
 *
 * The reference inverts the blended 4x4 with torch.linalg.inv; its bottom row is (0, 0, 0, sum w), so the two agree for weights
 * that sum to 1.  A singular blend gives what the arithmetic above gives (inf or NaN), not an error.
 * `normals` and `out_normals` are both given or both NULL.  1 <= J <= 128, N >= 0, 0 <= B <= 65535; B = 0 or N = 0 launches nothing.
 * One thread per point; the matrices of the workgroup's batch are staged in LDS once per workgroup.
 */
int ag_inverse_skinning_init(const float* points /*[B,N,3]*/, const float* weights /*[B,N,J]*/, const float* jnt_mats /*[B,J,4,4]*/,
                             const float* normals /*[B,N,3] or NULL*/, float* out_points /*[B,N,3]*/, float* out_normals /*[B,N,3] or NULL*/,
                             int32_t B, int64_t N, int32_t J, void* stream);

/*
 * xc_out[b, n] = xc_init[b, n] after `iterations` damped Newton steps of  sum_j w_j(xc) (A_j xc) = xt  (root_finding.cu:43-154).
 * Per point, with xc = xc_init[b, n], xt = xt[b, n], A_j = jnt_mats[b, j], R = (X, Y, Z), lo = bounds[0], hi = bounds[1]:
 *
 *   per axis d:  u = (xc_d - lo_d) / (hi_d - lo_d);  u = fmaxf(fminf(u, 1.f), 0.f)                 a NaN u becomes 1
 *                node_d = (int)roundf((float)(R_d - 1) * u)                                          halves round away from zero
 *   w = volume[node, :]
 *   g_j = grad[node, j, :] if `grad` is given, else the expression of ag_weight_volume_gradient at (node, j), evaluated from the 26
 *         rows around the node: the same operations in the same order, so both modes return identical bits
 *   lane l = 0 .. 15 of the point's group takes j = l, l + 16, l + 32, ... ascending, each sum from 0:
 *       m_l[r][c] = m_l[r][c] + w_j * a_j[r][c]                                  12 sums
 *       s_r = ((a_j[r][0]*xc_0 + a_j[r][1]*xc_1) + a_j[r][2]*xc_2) + a_j[r][3]
 *       j2_l[r][c] = j2_l[r][c] + s_r * g_j[c]                                   9 sums
 *       f_l[r] = f_l[r] + w_j * s_r                                              3 sums
 *   each of the 24 sums is then folded over the 16 lanes as a tree: p_l + p_(l+8) for l < 8, of those q_l + q_(l+4) for l < 4, of
 *   those r_l + r_(l+2) for l < 2, and last the two.  (A lane without a joint contributes its zeros.  The kernel forms the tree with
 *   row rotations by 8, 4, 2, 1; fp32 addition commutes, so every lane ends with these bits.)
 *   jac[r][c] = m[r][c] + j2[r][c] * lambda
 *   inv = the adjugate of jac times (1.f / d), d and the adjugate as in ag_inverse_skinning_init
 *   delta = f - xt;   update_r = (inv[r][0]*delta_0 + inv[r][1]*delta_1) + inv[r][2]*delta_2
 *   update_r = fmaxf(fminf(update_r, 0.01f), -0.01f)             fminf / fmaxf return the operand that is not a NaN, so a NaN
 *                                                                component (a singular step: d = 0) becomes +0.01, as in the reference
 *   xc_r = xc_r - update_r
 *
 * A point with active[b, n] == 0 copies xc_init to xc_out (the reference compacts such points away; here the mask goes to the
 * kernel).  `active` NULL: every point is active.  iterations = 0 copies.
 * Two differences from the reference, stated: (1) each batch uses ITS OWN matrices jnt_mats[b]; the reference compacts all batches
 * into one and so reads batch 0's matrices for every point.  The two agree for B = 1.  (2) `iterations` is honoured; the reference
 * ignores its argument and always runs 10.
 * `grad` given: [X, Y, Z, J, 3] as ag_weight_volume_gradient writes it (1.38 GB at 128^3 x 55); NULL needs none of it.
 * `bounds`: HOST lo[3], hi[3].  `spacing`: HOST, the three node spacings of the gradient (read only when grad == NULL, never NULL).
 * X, Y, Z >= 2, 1 <= J <= 128, N >= 0, iterations >= 0, 0 <= B <= 65535 (AG_ERR_INVALID_ARGUMENT otherwise); N = 0 or B = 0
 * launches nothing.  xc_out may be xc_init itself (the reference's call); it must not overlap anything else.
 */
int ag_inverse_skinning_root_find(const float* volume /*[X,Y,Z,J]*/, const float* grad /*[X,Y,Z,J,3] or NULL*/, int32_t X, int32_t Y, int32_t Z,
                                  int32_t J, const float* bounds /*host [2,3]*/, const float* spacing /*host [3]*/, const float* xt /*[B,N,3]*/,
                                  const float* xc_init /*[B,N,3]*/, const float* jnt_mats /*[B,J,4,4]*/, const uint8_t* active /*[B,N] or NULL*/,
                                  float* xc_out /*[B,N,3]*/, int32_t B, int64_t N, float lambda, int32_t iterations, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_INVERSE_SKINNING_H */
