// The template stage's field (include/ag_template_field.h): embedding -> geometry MLP -> colour MLP -> density, one fused forward kernel,
// field_kernel<false>; the SDF with its gradient (include/ag_template_field_grad.h) is field_kernel<true>, the same tile, layer and
// product loops with its own embedding, accumulator start and epilogue.
//
// Shape.  A workgroup of 8 waves owns a tile of kPoints = 32 points and keeps it in LDS from the embedding to the outputs:
//   emb   [32][kEmbStride]   the positional embedding (columns 0 .. 63) and the view embedding (64 .. 95), padding columns zero;
//   act0 / act1 [32][kActStride]   input and output of the current layer, swapped after every layer.
// A layer is  D[point][n] = bias[n] + sum_k U[point][k] W[n][k]  on v_mfma_f32_32x32x2_f32: the 32 points are the rows of A, a 32-column
// tile of outputs the columns of B, one wave per tile (tile t of a layer goes to wave (t - first tile) mod 8).  Lane l (i = l & 31,
// h = l >> 5) feeds A[i][k] and B[k][i] for one k per instruction; for a group of 8 consecutive k it reads A as ONE 16-byte LDS read
// (k0 + 4 h .. k0 + 4 h + 3 of point i) and B as ONE 16-byte global read of the packed blob ([k / 4][n][4], so a wave reads 2 x 512
// contiguous bytes), then issues 4 MFMAs: the k order inside a group is k0, k0+4, k0+1, k0+5, ... as the header states.  These reads, the
// order and the C/D row map are csrc/ag_mlp_tile.h's, shared with the hand fusion.  The accumulator
// starts from the bias.  Weights come from L2 (2.8 MB for both reference networks); nothing but xyz / viewdirs and the outputs touches HBM.
//
// The SDF column sits alone in the last 32-column tile of the last geometry layer (the blob's column order), so a request without
// colour computes that one tile and stops; with colour the same tile is computed by the same code, hence bit-identical.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states the embedding, the activations and the density op by op.
#include "ag_mlp_tile.h"
#include "../../include/ag_template_field.h"
#include "../../include/ag_template_field_grad.h"

namespace ag {
namespace field {

constexpr int kPoints = 32;                 // points per tile = rows of one 32x32 MFMA
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxWidth = 512;
constexpr int kActStride = kMaxWidth + 4;   // floats; 16-byte rows, 4 banks apart
constexpr int kEmbPos = 64;                 // 3 + 6 * 10 = 63 columns at most, padded to 8
constexpr int kEmbView = 32;                // 3 + 6 * 4 = 27
constexpr int kEmbStride = kEmbPos + kEmbView + 4;
constexpr int kMaxMultires = 10, kMaxMultiresView = 4;
constexpr size_t kLdsBytes = (size_t)(2 * kPoints * kActStride + kPoints * kEmbStride) * sizeof(float);
static_assert(kLdsBytes == 144896 && kLdsBytes <= 160 * 1024, "LDS budget stated in include/ag_template_field.h");

enum { kToLds = 0, kGeoLast = 1, kColorLast = 2 };

struct LayerPlan {
    int Ka;            // columns taken from the previous layer's output (a multiple of 8)
    int Ke;            // columns taken from the embedding tile, padded to a multiple of 8 (0: none)
    int emb_off;       // first of them in a row of `emb`
    int Np;            // packed output columns (a multiple of 32)
    int act;
    int route;
    int first_tile;    // tiles below it are not computed
    unsigned w_off, b_off;   // floats from the start of the blob
};

struct Plan {
    int n_layers;      // layers to run (the geometry layers alone when colour is not requested)
    int L, Lv;
    float beta, b;
    LayerPlan layer[2 * AG_FIELD_MAX_LAYERS];
};

using namespace ag::mlp;

__device__ __forceinline__ float activate(float x, int act, float beta)
{
    if (act == AG_FIELD_ACT_SOFTPLUS) {
        const float bx = beta * x;
        return bx > 20.0f ? x : log1pf(expf(bx)) / beta;
    }
    if (act == AG_FIELD_ACT_RELU) return x > 0.0f ? x : 0.0f;
    if (act == AG_FIELD_ACT_SIGMOID) return sigmoid(x);
    return x;
}

// emb(x, L) of one tile into columns [off, off + pad8(3 + 6 L)) of `emb`; src == nullptr or a point past N reads as zero
__device__ __forceinline__ void embed_tile(float* emb, int off, int L, const float* __restrict__ src, long long p0, long long N)
{
    const int per_point = 3 * (L + 1);
    for (int e = threadIdx.x; e < kPoints * per_point; e += kThreads) {
        const int p = e / per_point, r = e - p * per_point;
        const int fi = r / 3, axis = r - 3 * fi;
        const float x = (src != nullptr && p0 + p < N) ? src[(size_t)(p0 + p) * 3 + axis] : 0.0f;
        float* row = emb + p * kEmbStride + off;
        if (fi == 0) {
            row[axis] = x;
        } else {
            const float v = x * (float)(1 << (fi - 1));
            row[3 + 6 * (fi - 1) + axis] = sinf(v);
            row[6 + 6 * (fi - 1) + axis] = cosf(v);
        }
    }
    const int cols = 3 + 6 * L, pad = (cols + 7) / 8 * 8 - cols;
    for (int e = threadIdx.x; e < kPoints * pad; e += kThreads) emb[(e / pad) * kEmbStride + off + cols + e % pad] = 0.0f;
}

// ---- the SDF with its gradient (include/ag_template_field_grad.h): field_kernel<true> -----------------------------------------------------
// Forward mode: a tile is kGradPoints = 8 points x 4 rows, MFMA row 4 q + c with q the point, c = 0 its value row and c = 1 .. 3 the
// tangent d/dx_{c-1}.  A tangent row goes through the same linear maps as the value row (from 0 instead of the bias) and is multiplied
// by the activation's derivative at the value row's pre-activation.  In the C/D map a lane holds rows (r & 3) + 8 (r >> 2) + 4 h: c = r & 3
// and q = 2 (r >> 2) + h, so acc[4 j .. 4 j + 3] are the value and the three tangents of ONE point and the derivative needs no other lane.
// The value rows see the instructions of field_kernel<false> (a row of an MFMA does not depend on the other rows), so sdf and
// density are that kernel's bit for bit.  Same LDS, same blob, same plan as an SDF-only forward.
constexpr int kGradPoints = kPoints / 4;

__device__ __forceinline__ float activation_slope(float z, int act, float beta)
{
    if (act == AG_FIELD_ACT_SOFTPLUS) {
        const float bz = beta * z;
        return bz > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-bz));
    }
    if (act == AG_FIELD_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
    return 1.0f;
}

// emb(x, L) of 8 points into rows 4 q and its three tangents into rows 4 q + 1 + b, columns [0, pad8(3 + 6 L)); a point past N reads as zero
__device__ __forceinline__ void embed_tile_grad(float* emb, int L, const float* __restrict__ src, long long p0, long long N)
{
    const int per_point = 3 * (L + 1);
    for (int e = threadIdx.x; e < kGradPoints * per_point; e += kThreads) {
        const int q = e / per_point, r = e - q * per_point;
        const int fi = r / 3, axis = r - 3 * fi;
        const float x = p0 + q < N ? src[(size_t)(p0 + q) * 3 + axis] : 0.0f;
        float* row = emb + 4 * q * kEmbStride;
        if (fi == 0) {
            row[axis] = x;
            for (int b = 0; b < 3; ++b) row[(1 + b) * kEmbStride + axis] = b == axis ? 1.0f : 0.0f;
        } else {
            const float f = (float)(1 << (fi - 1));
            const float v = x * f;
            const float s = sinf(v), c = cosf(v);
            const int cs = 3 + 6 * (fi - 1) + axis, cc = cs + 3;
            row[cs] = s;
            row[cc] = c;
            for (int b = 0; b < 3; ++b) {
                row[(1 + b) * kEmbStride + cs] = b == axis ? f * c : 0.0f;
                row[(1 + b) * kEmbStride + cc] = b == axis ? -(f * s) : 0.0f;
            }
        }
    }
    const int cols = 3 + 6 * L, pad = (cols + 7) / 8 * 8 - cols;
    for (int e = threadIdx.x; e < kPoints * pad; e += kThreads) emb[(e / pad) * kEmbStride + cols + e % pad] = 0.0f;
}

// kTangents false: the field (`vec3` = color, may be NULL); true: the SDF with its gradient (`vec3` = grad, `viewdirs` not read).  The tile
// loop, the layer loop and the products are one text; the embedding, the accumulator's start and the epilogue are each kernel's own.
template <bool kTangents>
__global__ void __launch_bounds__(kThreads) field_kernel(Plan plan, const float* __restrict__ blob, const float* __restrict__ xyz,
                                                         const float* __restrict__ viewdirs, long long N, long long n_tiles, float* __restrict__ sdf,
                                                         float* __restrict__ density, float* __restrict__ vec3)
{
    __shared__ __attribute__((aligned(16))) float act_lds[2 * kPoints * kActStride];
    __shared__ __attribute__((aligned(16))) float emb[kPoints * kEmbStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const float alpha = 1.0f / plan.b;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long p0 = tile * (kTangents ? kGradPoints : kPoints);
        if constexpr (kTangents) {
            embed_tile_grad(emb, plan.L, xyz, p0, N);
        } else {
            embed_tile(emb, 0, plan.L, xyz, p0, N);
            if (plan.Lv >= 0) embed_tile(emb, kEmbPos, plan.Lv, viewdirs, p0, N);   // some layer that runs concatenates the view embedding
        }
        __syncthreads();
        float* in = act_lds + kPoints * kActStride;
        float* out = act_lds;
        for (int l = 0; l < plan.n_layers; ++l) {
            const LayerPlan lp = plan.layer[l];
            const int n_col_tiles = lp.Np >> 5;
            const size_t wstep = 2 * (size_t)lp.Np;                    // float4s between two groups of 8 k
            for (int t = lp.first_tile + wave; t < n_col_tiles; t += kWaves) {
                const int n = t * 32 + i;
                const float bias = blob[lp.b_off + n];
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = (!kTangents || (r & 3) == 0) ? bias : 0.0f;
                const float4* w = weights(blob, lp.w_off, lp.Np, n, h);
                const float* a = in + i * kActStride + 4 * h;
                const int ga = lp.Ka >> 3;
                // Ka is a multiple of 32: batches of 4 groups, the next batch's 8 reads in flight under the 16 MFMAs of this one.  This loop
                // stands here and not behind a function of ag_mlp_tile.h: inlined from one, it is scheduled differently and both kernels lose time.
                float4 av[4], wv[4];
                if (ga > 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { av[j] = *reinterpret_cast<const float4*>(a + 8 * j); wv[j] = w[j * wstep]; }
                }
                for (int g = 0; g < ga; g += 4) {
                    float4 an[4], wn[4];
                    const int gn = g + 4 < ga ? g + 4 : g;             // the last batch reads itself again: no branch around the reads
#pragma unroll
                    for (int j = 0; j < 4; ++j) { an[j] = *reinterpret_cast<const float4*>(a + 8 * (gn + j)); wn[j] = w[(gn + j) * wstep]; }
                    __builtin_amdgcn_sched_barrier(0);                 // keep the reads above the MFMAs they overlap with
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = mac8(acc, av[j], wv[j]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { av[j] = an[j]; wv[j] = wn[j]; }
                }
                acc = products(acc, emb + i * kEmbStride + lp.emb_off + 4 * h, w + ga * wstep, wstep, lp.Ke >> 3);
                // the field's epilogue: 16 values of 16 points (no trip when kTangents)
#pragma unroll
                for (int r = 0; r < 16 && !kTangents; ++r) {
                    const int row = cd_row(r, h);
                    const float v = activate(acc[r], lp.act, plan.beta);
                    const long long p = p0 + row;
                    if (lp.route == kGeoLast && t == n_col_tiles - 1) {
                        if (i == 0 && p < N) {
                            sdf[p] = -v;
                            if (density != nullptr) density[p] = sdf_density(v, plan.b, alpha);
                        }
                    } else if (lp.route == kColorLast) {
                        if (i < 3 && p < N) vec3[(size_t)p * 3 + i] = v;
                    } else {
                        out[row * kActStride + n] = v;
                    }
                }
                // the gradient's epilogue: value and three tangents of 4 points (no trip unless kTangents)
#pragma unroll
                for (int j = 0; j < 4 && kTangents; ++j) {
                    const float z = acc[4 * j];
                    const float v = activate(z, lp.act, plan.beta);
                    const float slope = activation_slope(z, lp.act, plan.beta);
                    const float t0 = acc[4 * j + 1] * slope, t1 = acc[4 * j + 2] * slope, t2 = acc[4 * j + 3] * slope;
                    if (lp.route == kGeoLast) {                        // first_tile: only the SDF tile runs
                        const long long p = p0 + 2 * j + h;
                        if (i == 0 && p < N) {
                            sdf[p] = -v;
                            vec3[(size_t)p * 3 + 0] = t0;
                            vec3[(size_t)p * 3 + 1] = t1;
                            vec3[(size_t)p * 3 + 2] = t2;
                            if (density != nullptr) density[p] = sdf_density(v, plan.b, alpha);
                        }
                    } else {
                        float* o = out + (8 * j + 4 * h) * kActStride + n;
                        o[0] = v;
                        o[kActStride] = t0;
                        o[2 * kActStride] = t1;
                        o[3 * kActStride] = t2;
                    }
                }
            }
            __syncthreads();
            float* s = in; in = out; out = s;
        }
    }
}

// Validates `d` against the limits of the header and lays the blob out; returns the blob's floats through `total`.
int make_plan(const AgTemplateFieldDesc* d, bool want_color, Plan& plan, size_t& total)
{
    if (!d) { set_error("template field: desc is NULL"); return AG_ERR_INVALID_ARGUMENT; }
    if (d->n_geo < 1 || d->n_geo > AG_FIELD_MAX_LAYERS || d->n_color < 0 || d->n_color > AG_FIELD_MAX_LAYERS) {
        set_error("template field: n_geo = %d must be 1 .. %d and n_color = %d must be 0 .. %d", d->n_geo, AG_FIELD_MAX_LAYERS, d->n_color, AG_FIELD_MAX_LAYERS);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (d->multires < 0 || d->multires > kMaxMultires || d->multires_view < 0 || d->multires_view > kMaxMultiresView) {
        set_error("template field: multires = %d must be 0 .. %d and multires_view = %d must be 0 .. %d", d->multires, kMaxMultires, d->multires_view,
                  kMaxMultiresView);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (!(d->softplus_beta > 0.f) || !std::isfinite(d->softplus_beta) || !(d->density_b > 0.f) || !std::isfinite(d->density_b)) {
        set_error("template field: softplus_beta = %g and density_b = %g must be finite and positive", (double)d->softplus_beta, (double)d->density_b);
        return AG_ERR_INVALID_ARGUMENT;
    }
    plan = Plan{};
    plan.L = d->multires;
    plan.Lv = -1;
    plan.beta = d->softplus_beta;
    plan.b = d->density_b;
    const int e_pos = 3 + 6 * d->multires, e_view = 3 + 6 * d->multires_view;
    size_t off = 0;
    int prev = 0;
    const int n_all = d->n_geo + d->n_color;
    for (int l = 0; l < n_all; ++l) {
        const bool geo = l < d->n_geo;
        const int li = geo ? l : l - d->n_geo;
        const AgFieldLayer& a = geo ? d->geo[li] : d->color[li];
        const char* net = geo ? "geometry" : "colour";
        const bool last = li == (geo ? d->n_geo : d->n_color) - 1;
        if (a.act < AG_FIELD_ACT_NONE || a.act > AG_FIELD_ACT_SIGMOID || a.concat < AG_FIELD_CONCAT_NONE || a.concat > AG_FIELD_CONCAT_VIEW) {
            set_error("template field: %s layer %d: act = %d or concat = %d is not one of the header's", net, li, a.act, a.concat);
            return AG_ERR_INVALID_ARGUMENT;
        }
        if (l == 0 && a.concat != AG_FIELD_CONCAT_POSITION) {
            set_error("template field: geometry layer 0 must take the positional embedding (concat = %d)", a.concat);
            return AG_ERR_INVALID_ARGUMENT;
        }
        const int e_cols = a.concat == AG_FIELD_CONCAT_POSITION ? e_pos : a.concat == AG_FIELD_CONCAT_VIEW ? e_view : 0;
        if (a.K != prev + e_cols) {
            set_error("template field: %s layer %d: K = %d, but its input has %d + %d columns", net, li, a.K, prev, e_cols);
            return AG_ERR_INVALID_ARGUMENT;
        }
        bool ok;
        if (!last) ok = a.width >= 32 && a.width % 32 == 0 && a.width <= kMaxWidth;
        else if (geo) ok = a.width >= 1 && (a.width - 1) % 32 == 0 && a.width - 1 <= kMaxWidth && (d->n_color == 0 || a.width > 1);
        else ok = a.width == 3;
        if (!ok) {
            set_error("template field: %s layer %d: width = %d (multiples of 32 up to %d; the last geometry layer 1 + 32 m; the last colour layer 3)", net, li,
                      a.width, kMaxWidth);
            return AG_ERR_INVALID_ARGUMENT;
        }
        LayerPlan& lp = plan.layer[l];
        lp.Ka = prev;
        lp.Ke = pad8(e_cols);
        lp.emb_off = a.concat == AG_FIELD_CONCAT_VIEW ? kEmbPos : 0;
        lp.Np = pad32(a.width);
        lp.act = a.act;
        lp.route = !last ? kToLds : geo ? kGeoLast : kColorLast;
        lp.first_tile = (last && geo && !want_color) ? lp.Np / 32 - 1 : 0;
        lp.w_off = (unsigned)off;
        off += (size_t)(lp.Ka + lp.Ke) * lp.Np;
        lp.b_off = (unsigned)off;
        off += (size_t)lp.Np;
        if (a.concat == AG_FIELD_CONCAT_VIEW) plan.Lv = d->multires_view;
        prev = (last && geo) ? a.width - 1 : a.width;
    }
    plan.n_layers = want_color ? n_all : d->n_geo;
    if (!want_color) plan.Lv = -1;
    total = off;
    return AG_OK;
}

}  // namespace field
}  // namespace ag

using namespace ag;
using namespace ag::field;

extern "C" size_t ag_template_field_desc_bytes(void) { return sizeof(AgTemplateFieldDesc); }

extern "C" size_t ag_template_field_blob_floats(const AgTemplateFieldDesc* desc)
{
    Plan plan;
    size_t total = 0;
    if (make_plan(desc, true, plan, total) != AG_OK) return 0;
    return total;
}

extern "C" int ag_template_field_forward(const AgTemplateFieldDesc* desc, const float* blob, size_t blob_floats, const float* xyz, const float* viewdirs,
                                         int64_t N, float* sdf, float* density, float* color, void* stream)
{
    Plan plan;
    size_t total = 0;
    const bool want_color = color != nullptr;
    if (int rc = make_plan(desc, want_color, plan, total)) return rc;
    if (want_color && desc->n_color == 0) { set_error("template field: colour requested from a field without a colour MLP"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_sizes("template field", N, INT64_MAX, blob_floats, total)) return rc;
    if (N == 0) return AG_OK;
    if (!xyz || !sdf) { set_error("null pointer in ag_template_field_forward"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_blob("template field", blob)) return rc;
    const long long n_tiles = (N + kPoints - 1) / kPoints;
    unsigned grid = 0;                                                         // one workgroup fits a CU (LDS); the rest of a tile list is the grid-stride loop
    if (int rc = persistent_grid(n_tiles, 4, "template field device query", &grid)) return rc;
    hipLaunchKernelGGL(field_kernel<false>, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), plan, blob, xyz, viewdirs,
                       (long long)N, n_tiles, sdf, density, color);
    return check_hip(hipGetLastError(), "field_kernel<false>");
}

extern "C" int ag_template_field_sdf_grad(const AgTemplateFieldDesc* desc, const float* blob, size_t blob_floats, const float* xyz, int64_t N, float* sdf,
                                          float* grad, float* density, void* stream)
{
    Plan plan;
    size_t total = 0;
    if (int rc = make_plan(desc, false, plan, total)) return rc;
    for (int l = 0; l < desc->n_geo; ++l) {
        if (desc->geo[l].concat == AG_FIELD_CONCAT_VIEW) {
            set_error("template field gradient: geometry layer %d concatenates the view embedding, and there are no view directions here", l);
            return AG_ERR_INVALID_ARGUMENT;
        }
    }
    if (int rc = check_sizes("template field gradient", N, INT64_MAX, blob_floats, total)) return rc;
    if (N == 0) return AG_OK;
    if (!xyz || !sdf || !grad) { set_error("null pointer in ag_template_field_sdf_grad"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_blob("template field gradient", blob)) return rc;
    const long long n_tiles = (N + kGradPoints - 1) / kGradPoints;
    unsigned grid = 0;                                                         // as ag_template_field_forward
    if (int rc = persistent_grid(n_tiles, 4, "template field gradient device query", &grid)) return rc;
    hipLaunchKernelGGL(field_kernel<true>, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), plan, blob, xyz,
                       static_cast<const float*>(nullptr), (long long)N, n_tiles, sdf, density, grad);
    return check_hip(hipGetLastError(), "field_kernel<true>");
}
