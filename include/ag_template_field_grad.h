/*
 * ag_template_field_grad.h — C ABI of the template field's gradient (libag_hip.so): canonical points -> raw SDF, its gradient with
 * respect to the points, and density, in ONE fused kernel beside ag_template_field.h's forward.
 *
 * It evaluates what the reference's TemplateNet.forward_cano_body_nerf (network/template.py:98-140) returns as 'normal' when
 * compute_grad is set: torch.autograd.grad of the raw SDF with respect to the query points (template.py:129-139), the quantity of the
 * eikonal loss (main_template.py:53-58).  Forward mode, forward only: no gradient with respect to the weights.
 *
 * Same descriptor, same packed blob, same limits, same conventions and same error behaviour as ag_template_field_forward
 * (ag_template_field.h): nothing is repacked.
 *
 * Definition.  With s = column 0 of the last geometry layer (raw), grad_p = d s / d xyz_p.  That is the reference's 'normal': the
 *   gradient of the RAW output, minus the gradient of the returned sdf = -s.  It points out of the body (sdf is positive inside).
 *   It is computed as three tangents, one per axis b, pushed through the geometry MLP beside the value:
 *   Embedding.   The tangent of axis b of emb(x, L), column by column:
 *                x_a:            1 if a == b, else 0;
 *                sinf(x_a f):    f * cosf(x_a f) if a == b, else 0;
 *                cosf(x_a f):    -(f * sinf(x_a f)) if a == b, else 0.
 *                The sine and the cosine are the very values of the value row; f is a power of two, so the product is exact.
 *   Linear.      A tangent row t maps to W t: the same fp32 MFMA chain and the same order over k as the value row of
 *                ag_template_field.h, starting from 0 where the value row starts from the bias.  A skip layer's input tangent is the
 *                previous output's tangent followed by the embedding's.
 *   Activation.  With z the value row's pre-activation, a tangent is multiplied ONCE in fp32 by the derivative:
 *                AG_FIELD_ACT_SOFTPLUS: beta * z > 20 ? 1 : 1 / (1 + expf(-(beta * z)));  AG_FIELD_ACT_RELU: z > 0 ? 1 : 0;
 *                AG_FIELD_ACT_NONE: 1.
 *   Outputs.     sdf_p = -s.  density_p exactly as in ag_template_field.h.  grad_p[b] = the tangent of column 0 for axis b.
 *   Only the SDF tile of the last geometry layer is computed, as in a forward without colour; the colour MLP never runs and there are
 *   no view directions (a table whose geometry layers concatenate the view embedding is refused).
 *   No atomics: every output is bit-identical between calls.  The value rows go through the instruction sequence of the forward
 *   kernel, so sdf -- and density when requested -- are bit-identical to ag_template_field_forward's.
 *
 * Kernel shape (csrc/ag_template_field.hip).  The forward's workgroup, LDS (144 896 bytes, one workgroup per CU) and product loop.  A
 *   tile is 8 points x 4 rows: MFMA row 4 q + c holds point q's value (c = 0) or its tangent along axis c - 1.  In the 32x32 C/D map a
 *   lane then holds a point's value and three tangents in four consecutive accumulator registers, so the derivative needs no
 *   cross-lane traffic, no stored activations and no second pass.  A pass over the weights serves 8 points where the forward's serves 32.
 */
#ifndef AG_TEMPLATE_FIELD_GRAD_H
#define AG_TEMPLATE_FIELD_GRAD_H

#include "ag_template_field.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The SDF and its gradient at N points.  `sdf` [N] and `grad` [N,3] are required; `density` [N] may be NULL.  `blob` must hold
 * blob_floats == ag_template_field_blob_floats(desc) floats, 16-byte aligned.  Validates before any launch; N == 0 returns 0 without a
 * launch; any N works, the last tile of points is masked inside the kernel.  Only enqueues work on `stream`.
 */
int ag_template_field_sdf_grad(const AgTemplateFieldDesc* desc /*HOST*/, const float* blob, size_t blob_floats, const float* xyz /*[N,3]*/, int64_t N,
                               float* sdf /*[N]*/, float* grad /*[N,3]*/, float* density /*[N] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_TEMPLATE_FIELD_GRAD_H */
