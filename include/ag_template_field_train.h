/*
 * ag_template_field_train.h — C ABI of the template field's training path (libag_hip.so): the field of ag_template_field.h evaluated
 * LAYER BY LAYER with every layer's activations kept (the stash), and its reverse pass: the gradient of a loss with respect to every
 * weight and bias, given the gradient with respect to sdf and color.  The fused forward kernel of ag_template_field.h is untouched: it
 * stays the inference path; this one is what a training step calls (template_train.TemplateFieldModule).
 *
 * The plan (AgTemplateFieldDesc), its limits and the forward blob are ag_template_field.h's.  Conventions as there: device pointers
 * unless marked HOST, fp32, contiguous, 0 on success, ag_last_error() on failure.  All arithmetic is fp32, every product sum runs on
 * v_mfma_f32_32x32x2_f32, and there are NO atomics: every output is a pure function of the inputs and bit-identical between calls.
 *
 * Forward.  Per layer one launch: a workgroup owns 32 points, brings the layer's input rows (the previous layer's output, then the
 *   zero-padded embedding where the layer concatenates one) into LDS and forms every 32-column output tile from the bias by the tile
 *   routine of csrc/ag_mlp_tile.h, in the k order ag_template_field.h states; the activations are that header's.  The chain, its
 *   start and its order are the fused kernel's, so sdf and color equal ag_template_field_forward on the same blob BIT FOR BIT.
 *
 * Stash.  [N, C] blocks, row-major, one after the other (a block of C columns starts at float N * (sum of the C before it)):
 *       emb(xyz, multires)            C = Ep = 3 + 6 multires rounded up to a multiple of 8, the padding zero;
 *       emb(viewdirs, multires_view)  C = Ev, likewise; present (Ev > 0) only when some colour layer concatenates it;
 *       per layer, plan order         C = Np (width rounded up to a multiple of 32): the ACTIVATED output in the blob's packed column
 *                                     order (the last geometry layer: features first, the SDF column at Np - 32).
 *   ag_template_field_train_stash_floats returns N * (Ep + Ev + sum Np): 2944 floats (11.8 KB) per point for the reference's networks.
 *   A forward with color == NULL leaves the colour layers' blocks unwritten; a backward with g_color != NULL needs them written.
 *
 * Backward.  With dY the gradient at a layer's activated output and y that output:
 *       dZ = dY * act'      act' = 1 (NONE), [y > 0] (RELU), y (1 - y) (SIGMOID), and for SOFTPLUS  -expm1f(-(beta * y)),  formed from the
 *                           STASHED OUTPUT: where beta z > 20, y = z and the expression rounds to 1; elsewhere it is sigmoid(beta z);
 *       dX = dZ W           for the columns that are the previous layer's output only (nothing here differentiates with respect to the
 *                           points or the view directions), by the forward's tile routine over the TRANSPOSED blob, from zero;
 *       dW = dZ^T X, db = sum_p dZ    X the layer's whole input, embedding columns included.  Points are cut into slabs of
 *                           AG_FIELD_TRAIN_SLAB; per slab a wave forms a 32-row strip of dW over up to 4 tiles of 32 columns as MFMA
 *                           chains over the slab's points in ascending order (pairs p, p + 1) and writes a partial; a second
 *                           launch adds the slabs' partials in ascending order.
 *   The upstream of the last colour layer is g_color; that of the last geometry layer is [-g_sdf, dX of the first colour layer].
 *   A NULL upstream means zeros.  With g_color == NULL the colour MLP is not walked and its gradient slots are written as zeros.
 *
 * Transposed blob.  Layers in plan order; per layer with Ka > 0 previous-output columns (Ka and Np as in ag_template_field.h):
 *       [Np / 4][Ka][4]:  element [g][k][j] = W[n'][k] of packed column n = 4 g + j (zero where n is padding), k = 0 .. Ka - 1,
 *   each layer starting where the previous one ends; layer 0 (Ka = 0) takes nothing.  ag_template_field_train_blob_t_floats returns the total.
 *
 * Gradients.  g_weight and g_bias are one flat buffer each, layers in plan order (geometry first), in the PLAIN layout of the reference's
 *   parameters: layer l's dW is [width_l][K_l] row-major at float  sum_{j < l} width_j * K_j  of g_weight, its db [width_l] at float
 *   sum_{j < l} width_j  of g_bias.  Every element is written; padding never is.
 *
 * Workspace.  2 * N * max_l Np_l floats (dZ of two neighbouring layers) + ceil(N / AG_FIELD_TRAIN_SLAB) * max_l (Np_l * Kp_l + Np_l)
 *   floats (the slabs' partials), Kp = Ka + Ke.  ag_template_field_train_workspace_floats returns it.
 *
 * Refusals.  A plan outside ag_template_field.h's limits, N outside 0 .. 2^31 - 1, a blob, stash or workspace whose float count is
 *   not the one stated, a blob, stash or workspace that is not 16-byte aligned, a NULL required pointer, colour asked of a field
 *   without a colour MLP: AG_ERR_INVALID_ARGUMENT with a message, before any launch.  The size checks come before the N == 0 return
 *   and need no device.  N == 0: forward returns 0 without a launch; backward enqueues the zeroing of g_weight and g_bias only.
 */
#ifndef AG_TEMPLATE_FIELD_TRAIN_H
#define AG_TEMPLATE_FIELD_TRAIN_H

#include "ag_template_field.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AG_FIELD_TRAIN_SLAB 1024

/* AG_FIELD_TRAIN_SLAB, for the binding. */
int64_t ag_template_field_train_slab(void);

/* Floats of the transposed blob / the stash / the workspace as laid out above; 0 (and ag_last_error) when `desc` is outside the limits
 * or N is negative. */
size_t ag_template_field_train_blob_t_floats(const AgTemplateFieldDesc* desc /*HOST*/);
size_t ag_template_field_train_stash_floats(const AgTemplateFieldDesc* desc /*HOST*/, int64_t N);
size_t ag_template_field_train_workspace_floats(const AgTemplateFieldDesc* desc /*HOST*/, int64_t N);

/*
 * The field at N points with the stash.  `sdf` [N] and `stash` are required; with color == NULL the colour MLP is not run.  `viewdirs`
 * may be NULL (zeros).  `blob`: ag_template_field.h's, blob_floats == ag_template_field_blob_floats(desc).  Only enqueues work on `stream`.
 */
int ag_template_field_train_forward(const AgTemplateFieldDesc* desc /*HOST*/, const float* blob, size_t blob_floats, const float* xyz /*[N,3]*/,
                                    const float* viewdirs /*[N,3] or NULL*/, int64_t N, float* stash, size_t stash_floats, float* sdf /*[N]*/,
                                    float* color /*[N,3] or NULL*/, void* stream);

/*
 * The reverse pass from the stash of a forward at the same N: `g_sdf` [N] and `g_color` [N,3] (each may be NULL: zeros) -> `g_weight`,
 * `g_bias` as laid out above.  Only enqueues work on `stream`.
 */
int ag_template_field_train_backward(const AgTemplateFieldDesc* desc /*HOST*/, const float* blob_t, size_t blob_t_floats, const float* stash,
                                     size_t stash_floats, const float* g_sdf /*[N] or NULL*/, const float* g_color /*[N,3] or NULL*/, int64_t N,
                                     float* workspace, size_t workspace_floats, float* g_weight, float* g_bias, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_TEMPLATE_FIELD_TRAIN_H */
