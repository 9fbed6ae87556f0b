/*
 * ag_template_field.h — C ABI of the template stage's field (libag_hip.so): canonical points -> raw SDF, density and colour through a
 * positional embedding, a geometry MLP and a colour MLP, in ONE fused forward kernel.
 *
 * It evaluates what the reference's TemplateNet.forward_cano_body_nerf (network/template.py:98-140) evaluates without compute_grad:
 * Embedder.embed (utils/embedder.py), SdfMLP and MLPLinear (network/mlp.py) and LaplaceDensity (network/density.py:22-36).  Forward
 * only: no gradient with respect to the points or the weights.
 *
 * Same conventions as ag_raster.h: device pointers unless marked HOST, fp32, contiguous, 0 on success, ag_last_error() on failure.
 *
 * Definition.  For every point p (viewdirs == NULL means d = 0, template.py:115-116):
 *   Embedding.   emb(x, L) has 3 + 6 L columns: x_0 x_1 x_2, then for f = 1, 2, ..., 2^(L-1) in this order:
 *                sinf(x_0 * f) sinf(x_1 * f) sinf(x_2 * f) cosf(x_0 * f) cosf(x_1 * f) cosf(x_2 * f).  x_a * f is ONE fp32 product (exact: f
 *                is a power of two) and sinf / cosf are the accurate ones (full argument reduction), never the fast intrinsics.
 *                e = emb(xyz_p, multires), v = emb(viewdirs_p, multires_view).
 *   Linear.      A layer of the table maps its input row u [K] to  act(W u + bias)  [width].  Its input is the previous layer's output,
 *                followed -- AFTER it -- by e when concat == AG_FIELD_CONCAT_POSITION or by v when concat == AG_FIELD_CONCAT_VIEW.
 *                The first geometry layer has no previous output: its concat must be POSITION and its input is e alone.  The first
 *                colour layer's "previous output" is columns 1 .. width-1 of the last geometry layer (the features).
 *                Every product sum is an fp32 fused-multiply-add chain that starts from the bias (v_mfma_f32_32x32x2_f32: one rounding per
 *                product, fp32 accumulation, no fp16 / bf16 operand rounding).  The ORDER over k is the kernel's, not ascending: within
 *                each group of 8 consecutive k (groups of the previous output first, then groups of the embedding, whose column count
 *                is padded with zeros to a multiple of 8) it is k0, k0+4, k0+1, k0+5, k0+2, k0+6, k0+3, k0+7.
 *   Activations. AG_FIELD_ACT_NONE: x.  AG_FIELD_ACT_SOFTPLUS (torch's, threshold 20): x when beta * x > 20, else
 *                log1pf(expf(beta * x)) / beta, beta the network's `softplus_beta`.  AG_FIELD_ACT_RELU: x > 0 ? x : 0.
 *                AG_FIELD_ACT_SIGMOID: 1 / (1 + expf(-x)).
 *   Outputs.     s = column 0 of the last geometry layer (raw).   sdf_p = -s (template.py:123).
 *                density_p = alpha * (0.5 + (0.5 * sign(s)) * expm1f(-|s| / b)),  alpha = 1 / b,  b = `density_b` given by the caller
 *                (|beta| + 1e-4 in fp32, density.py:34-36); sign(0) = 0.
 *                color_p = the 3 columns of the last colour layer.
 *   Everything but the product sums is rounded fp32 operations in the order written (the file is compiled with -ffp-contract=off).
 *   No atomics: every output is a pure function of the inputs and bit-identical between calls.  The SDF column is computed by the same
 *   instruction sequence whether or not density and colour are requested, so it is bit-identical between the two requests.
 *
 * Limits.  1 .. 8 layers per MLP.  Every width is a multiple of 32 and at most 512, except the last geometry layer, 1 + 32 m wide
 *   (m >= 0; m >= 1 when a colour MLP follows), and the last colour layer, exactly 3 wide.  multires 0 .. 10, multires_view 0 .. 4.  K of a
 *   layer = previous width (features for the first colour layer) + columns of the concatenated embedding: at most 512 + 63.
 *   Anything else returns AG_ERR_INVALID_ARGUMENT with a message before any launch.  N == 0 returns 0 without a launch; any N works,
 *   the last tile of points is masked inside the kernel.
 *
 * Packed weights.  One fp32 blob, packed once on the host, re-read from L2 by every workgroup (the reference's two networks: 2.8 MB).
 *   Layers in order, geometry first.  Per layer, with Np = width rounded up to a multiple of 32, Ka = previous width (a multiple of 8),
 *   Ke = embedding columns rounded up to a multiple of 8, Kp = Ka + Ke:
 *       weights [Kp / 4][Np][4]:  element [g][n][j] = W[n'][k'] of packed row k = 4 g + j and packed column n (zero where k or n is padding);
 *                                 packed rows: the Ka previous-output columns, then the embedding columns, then zeros up to Ke;
 *       bias    [Np]              (zero in the padding),
 *   each layer starting where the previous one ends (every size is a multiple of 32 floats).  Packed column n is output n, except in
 *   the last geometry layer, where the features come first and the SDF column last: packed n = c - 1 for output c >= 1, and output 0
 *   sits at packed column Np - 32, alone in its 32-column tile.  That tile is the only one computed when colour is not requested.
 *   ag_template_field_blob_floats returns the total.
 *
 * Kernel shape, LDS and occupancy (csrc/ag_template_field.hip).  A workgroup of 512 threads (8 waves) owns a tile of 32 points and
 *   walks over tiles in a grid-stride loop; a wave owns 32-column output tiles (the t-th tile computed -> wave t mod 8), one 32x32 accumulator at a time.
 *   Activations never leave LDS: two buffers [32][512 + 4] fp32 (input and output of the current layer, swapped per layer) and the
 *   embedding tile [32][64 + 32 + 4], resident from the first layer to the skip layer and the colour MLP: 132 096 + 12 800 = 144 896
 *   bytes of the CU's 160 KiB (163 840).  So ONE workgroup per CU, 2 waves per SIMD, 8 of 32 wave slots; with 64 points the two
 *   buffers alone would be 264 192 bytes.  The + 4 in the strides keeps the 16-byte operand reads of 32 rows off each other's banks.
 */
#ifndef AG_TEMPLATE_FIELD_H
#define AG_TEMPLATE_FIELD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_FIELD_MAX_LAYERS 8

enum { AG_FIELD_ACT_NONE = 0, AG_FIELD_ACT_SOFTPLUS = 1, AG_FIELD_ACT_RELU = 2, AG_FIELD_ACT_SIGMOID = 3 };
enum { AG_FIELD_CONCAT_NONE = 0, AG_FIELD_CONCAT_POSITION = 1, AG_FIELD_CONCAT_VIEW = 2 };

typedef struct AgFieldLayer {
    int32_t K;       /* input columns, the concatenated embedding included */
    int32_t width;   /* output columns */
    int32_t act;     /* AG_FIELD_ACT_* */
    int32_t concat;  /* AG_FIELD_CONCAT_*: which embedding follows the previous output in the input */
} AgFieldLayer;

typedef struct AgTemplateFieldDesc {
    int32_t multires, multires_view;      /* L of the two embeddings (L = 0: the three coordinates alone) */
    int32_t n_geo, n_color;               /* layers used of each table; n_color = 0: no colour MLP (colour cannot be requested) */
    float softplus_beta;                  /* > 0 */
    float density_b;                      /* > 0 */
    AgFieldLayer geo[AG_FIELD_MAX_LAYERS];
    AgFieldLayer color[AG_FIELD_MAX_LAYERS];
} AgTemplateFieldDesc;

/* sizeof(AgTemplateFieldDesc), for the binding's layout check. */
size_t ag_template_field_desc_bytes(void);

/* Floats of the packed blob of `desc` as laid out above; 0 (and ag_last_error) when `desc` is outside the limits. */
size_t ag_template_field_blob_floats(const AgTemplateFieldDesc* desc /*HOST*/);

/*
 * Evaluates the field at N points.  `sdf` [N] is required; `density` [N] and `color` [N,3] may each be NULL.  With color == NULL the
 * feature columns of the last geometry layer and the colour MLP are not computed.  `viewdirs` may be NULL (zeros).  `blob` must hold
 * blob_floats == ag_template_field_blob_floats(desc) floats, 16-byte aligned.  Only enqueues work on `stream`.
 */
int ag_template_field_forward(const AgTemplateFieldDesc* desc /*HOST*/, const float* blob, size_t blob_floats, const float* xyz /*[N,3]*/,
                              const float* viewdirs /*[N,3] or NULL*/, int64_t N, float* sdf /*[N]*/, float* density /*[N] or NULL*/,
                              float* color /*[N,3] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_TEMPLATE_FIELD_H */
