/*
 * ag_hand_fusion.h — C ABI of the template stage's hand fusion (libag_hip.so): near the two hands the body field's SDF, density and
 * colour are cross-faded into a signed distance to the MANO mesh and a small per-hand colour MLP, in ONE fused kernel per call.
 *
 * It evaluates what the reference's TemplateNet.fuse_hands (network/template.py:146-202) evaluates for one batch element, with the two
 * HandAvatar colour networks (network/hand_avatar.py) and geo_util.normalize_vert_bbox(per_axis = True) (utils/geo_util.py:104-114).
 * Forward only.  (ag_avatar.h's ag_hand_fuse is another thing: the Gaussian avatar's eval-time cross-fade into the mean hands.)
 *
 * Same conventions as ag_template_field.h: device pointers unless marked HOST, fp32 / int32, contiguous, 0 on success,
 * ag_last_error() on failure.  The file is compiled with -ffp-contract=off: everything below that is not a product sum of the MLP is
 * individually rounded fp32 operations in the order written; (x . y) stands for (x_0 * y_0 + x_1 * y_1) + x_2 * y_2 and
 * sigmoid(x) for 1 / (1 + expf(-x)) with the accurate expf.
 *
 * Definition, per point n (p = points[n], c = cano_xyz[n]; sdf_b, density_b, color_b the body's values) and per hand h (left, right):
 *   Box.         (mn, mx) = the hand's bbox_min / bbox_max [3]: the per-axis minimum and maximum of its canonical vertices, reduced by the
 *                caller (a minimum is exact).  norm_h(x)_a = (2 * (x_a - 0.5 * (mx_a + mn_a))) / (mx_a - mn_a).
 *   Gate.        gl = sigmoid(25 * (norm_left(c)_0 + 0.8)),   gr = sigmoid(-25 * (norm_right(c)_0 - 0.8));
 *                both 0 where c_1 < centre_y (a point AT centre_y keeps its gates).  ag_hand_field_gate writes
 *                active[n] = (gl != 0 || gr != 0) from these operations alone: it needs nothing but cano_xyz and the boxes.
 *   Closest.     (dist2, f, b) = the hand's dist2[n], face_id[n], bary[n] as ag_mesh_closest_point writes them for p on the hand's
 *                vertices / faces.  The hand is MISSING at n when f < 0 (a hand without faces), f >= F, or a corner of face f lies
 *                outside [0, V); nothing of a missing hand is read beyond f and the three indices.
 *   Weights.     wl = missing_left ? 0 : gl,  wr likewise;  s = max(wl + wr, 1);  wl = wl / s;  wr = wr / s;  w = wl + wr.
 *   Inactive.    wl == 0 && wr == 0: the outputs are the body's values, copied bit for bit (the density too: it is not recomputed).
 *                fp32 sigmoid is exactly 0 once expf overflows, i.e. more than about 5 half-widths of the box toward the body.  The
 *                reference's arithmetic gives 0 * hand + 1 * body there, which differs only in the sign of a zero.
 *   Interpolate. with (i0, i1, i2) = faces[f]:  attr(T) = (b_0 * T[i0] + b_1 * T[i1]) + b_2 * T[i2]  per component (the order of
 *                ag_mesh_resolve_attribute).  x = attr(norm_h(cano_vertices)) (each vertex normalised, then interpolated),
 *                q = attr(vertices), nrm = attr(normals)  (vertices / normals in the space of p).
 *   Hand SDF.    t = (nrm . (p - q)),  sg = t > 0 ? 1 : t < 0 ? -1 : 0,  sdf_h = (-sg) * sqrtf(dist2)   (positive inside, like sdf_b).
 *   Colour MLP.  u = [emb(x, multires), sdf_h], emb as in ag_template_field.h (3 + 6 L columns, accurate sinf / cosf, x_a * f one
 *                exact product), 4 + 6 L columns, padded with zeros to a multiple of 8.  Layers 0 .. n_layers-2 are
 *                relu(W u + bias), the last is sigmoid(W u + bias) and 3 wide: color_h.
 *                The reference's layer 0 has 60 more input columns, the quaternions of the 15 joints of hand_pose, constant over
 *                the points.  They are FOLDED INTO THE BIAS on the host, and that folding is the definition:
 *                bias0' = fp32(bias0 + W0[:, 4 + 6 L :] . quat) with the sum in float64, rounded once.  The device never sees them.
 *                Every product sum is an fp32 fused-multiply-add chain that starts from the bias (v_mfma_f32_32x32x2_f32: one
 *                rounding per product, fp32 accumulation).  The ORDER over k is the kernel's: within each group of 8 consecutive
 *                k it is k0, k0+4, k0+1, k0+5, k0+2, k0+6, k0+3, k0+7 (as in ag_template_field.h).
 *   Blend.       A hand with weight 0 contributes the constant 0 and nothing of it is used (its closest point may be +inf):
 *                term_h(v) = w_h != 0 ? w_h * v_h : 0.
 *                sdf     = (term_l(sdf) + term_r(sdf)) + (1 - w) * sdf_b
 *                color_a = (term_l(color_a) + term_r(color_a)) + (1 - w) * color_b,a
 *                density = alpha * (0.5 + (0.5 * sign(s)) * expm1f(-|s| / b)),  s = -sdf,  alpha = 1 / b,  b = density_b, sign(0) = 0
 *                (LaplaceDensity of the raw value, the formula of ag_template_field.h).
 *   No atomics and no reduction across points: every output is a pure function of its point's inputs, two calls agree bit for bit, and
 *   a point's outputs do not depend on which other points share the call (what lets the host compact the active points).
 *
 * In place.  sdf / density / color may be the very pointers sdf_in / density_in / color_in: a point's inputs are read before its
 *   outputs are written and no other point reads them.  Partial overlap is not allowed.
 *
 * Limits.  multires 0 .. 10.  2 .. 8 layers; every hidden width 32 or 64, the last layer exactly 3 wide; K of layer 0 = 4 + 6 L,
 *   of a later layer the previous width.  The boxes must have mx_a > mn_a on every axis, density_b > 0, all finite.  N < 2^31.
 *   Anything else returns AG_ERR_INVALID_ARGUMENT with a message before any launch.  N == 0 returns 0 without a launch; any N works,
 *   the last tile of points is masked inside the kernel.
 *
 * Packed weights.  One fp32 blob PER HAND, packed once on the host.  Layers in order; per layer, with Kp = K rounded up to a multiple
 *   of 8 and Np = width rounded up to a multiple of 32:
 *       weights [Kp / 4][Np][4]:  element [g][n][j] = W[n][k] of k = 4 g + j (zero where k or n is padding);
 *       bias    [Np]              (layer 0: the folded bias0'; zero in the padding),
 *   each layer starting where the previous one ends.  The reference's net (multires 4, 64 x 5, 3): 20 832 floats, 83 328 bytes.
 *   ag_hand_fusion_blob_floats returns the total.
 *
 * Kernel shape, LDS and occupancy (csrc/ag_hand_fusion.hip).  A workgroup of 256 threads (4 waves) owns a tile of 32 points and walks
 *   over tiles in a grid-stride loop.  Waves 0-1 run the left hand's MLP, waves 2-3 the right hand's, at the same time: a layer of
 *   width 64 is two 32x32 accumulators, one per wave of the hand.  Activations stay in LDS: per hand two buffers [32][64 + 4] fp32
 *   (34 816 bytes in all) plus 1 536 bytes of per-point scalars and 256 of the barrier vote: 36 608 bytes, four workgroups (16 waves) per
 *   CU.  A tile in which no (hand, point) has weight skips the embedding and the MLPs (a workgroup-uniform vote; same results).  Weights are read from
 *   L2 as 16-byte loads of the packed blob (both hands: 167 KB, resident in every XCD's 4 MB L2).  Chosen and rejected mappings and the
 *   measured times: DESIGN.md, "Hand fusion".
 */
#ifndef AG_HAND_FUSION_H
#define AG_HAND_FUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_HAND_MAX_LAYERS 8

typedef struct AgHandFusionDesc {
    int32_t multires;                     /* L of the embedding of x */
    int32_t n_layers;                     /* linears of the colour MLP, the last one (3 wide) included */
    int32_t width[AG_HAND_MAX_LAYERS];    /* output columns of each */
} AgHandFusionDesc;

typedef struct AgHandSide {
    const float* dist2;           /* [N]   as written by the closest-point query of `points` on (vertices, faces) */
    const int32_t* face_id;       /* [N] */
    const float* bary;            /* [N,3] */
    const float* vertices;        /* [V,3] the hand in the space of `points` */
    const float* normals;         /* [V,3] its vertex normals in that space */
    const float* cano_vertices;   /* [V,3] the hand in canonical space */
    const int32_t* faces;         /* [F,3] */
    const float* blob;            /* the hand's packed net, 16-byte aligned */
    int32_t V, F;
    float bbox_min[3], bbox_max[3];   /* of cano_vertices, per axis */
} AgHandSide;

typedef struct AgHandFieldFuseArgs {
    int64_t N;
    AgHandFusionDesc desc;        /* both hands' nets have this shape */
    float centre_y;               /* cano_smpl_center's y */
    float density_b;
    const float* points;          /* [N,3] the samples in the space they are rendered in */
    const float* cano_xyz;        /* [N,3] the same samples in canonical space */
    const float* sdf_in;          /* [N]   the body's sdf (positive inside) */
    const float* density_in;      /* [N]   the body's density */
    const float* color_in;        /* [N,3] the body's colour, or NULL: no colour is computed */
    float* sdf;                   /* [N] */
    float* density;               /* [N] */
    float* color;                 /* [N,3]; NULL exactly when color_in is */
    size_t blob_floats;           /* floats of each hand's blob */
    AgHandSide left, right;
} AgHandFieldFuseArgs;

/* sizeof(AgHandFieldFuseArgs), for the binding's layout check. */
size_t ag_hand_field_fuse_args_bytes(void);

/* Floats of one hand's packed blob as laid out above; 0 (and ag_last_error) when `desc` is outside the limits. */
size_t ag_hand_fusion_blob_floats(const AgHandFusionDesc* desc /*HOST*/);

/*
 * active[n] = 1 where a gate of point n is not 0, else 0 (the "Gate" lines above; the missing-hand rule is not applied, so the set is
 * a superset of the points the fusion changes).  left_box / right_box: HOST {min_x, max_x} of the two canonical hands.
 */
int ag_hand_field_gate(const float* cano_xyz /*[N,3]*/, int64_t N, const float* left_box /*HOST [2]*/, const float* right_box /*HOST [2]*/,
                       float centre_y, uint8_t* active /*[N]*/, void* stream);

/* The fusion of N points.  Only enqueues work on `stream`. */
int ag_hand_field_fuse(const AgHandFieldFuseArgs* args /*HOST*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AG_HAND_FUSION_H */
