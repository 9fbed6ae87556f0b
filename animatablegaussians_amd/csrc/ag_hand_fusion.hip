// The template stage's hand fusion (include/ag_hand_fusion.h): gates -> per hand (interpolate, signed distance, embedding, colour MLP) ->
// blend -> density, one fused kernel; beside it the gate alone, which marks the points the fusion can change.
//
// Shape.  A workgroup of 4 waves owns a tile of kPoints = 32 points.  Per tile:
//   A  threads 0 .. 63, one per (hand, point): gate, the closest face's three corners, x / q / nrm, sdf_h; x and sdf_h go straight
//      into the hand's layer-0 input row in LDS, the raw weight and sdf_h into s_w / s_sdf;
//   B  all threads: the sin / cos columns of both hands' embeddings from the x just written, zeros in the padding columns;
//   C  the MLP, waves 0-1 on the left hand and waves 2-3 on the right: a layer is D[point][n] = bias[n] + sum_k U[point][k] W[n][k] on
//      v_mfma_f32_32x32x2_f32 with the operand reads, the packed blob and the k order of csrc/ag_mlp_tile.h; a hand's two
//      waves take the layer's 32-column tiles alternately; the last layer writes sigmoid to s_col;
//   D  threads 0 .. 31, one per point: normalise the weights, blend, density, write (or copy the body's values).
// A tile in which no (hand, point) has weight skips B and C.
// Weights come from L2 (167 KB for both reference nets); nothing but the per-point inputs and the outputs touches HBM.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states everything but the product sums op by op.
#include "ag_mlp_tile.h"
#include "../../include/ag_hand_fusion.h"

namespace ag {
namespace handfuse {

constexpr int kPoints = 32;                 // points per tile = rows of one 32x32 MFMA
constexpr int kWavesPerHand = 2;
constexpr int kThreads = 64 * 2 * kWavesPerHand;
constexpr int kMaxWidth = 64;
constexpr int kStride = kMaxWidth + 4;      // floats; 16-byte rows, 4 banks apart
constexpr int kMaxMultires = 10;            // 4 + 6 * 10 = 64 input columns at most
constexpr size_t kLdsBytes = (size_t)(2 * 2 * kPoints * kStride + 2 * kPoints * (1 + 1 + 4)) * sizeof(float);
static_assert(kLdsBytes == 36352, "LDS budget stated in include/ag_hand_fusion.h");

struct LayerPlan {
    int Kp;            // input columns, padded to a multiple of 8
    int Np;            // packed output columns (a multiple of 32)
    int width;
    unsigned w_off, b_off;   // floats from the start of a hand's blob
};

struct Plan {
    int n_layers;
    int L;
    LayerPlan layer[AG_HAND_MAX_LAYERS];
};

struct Side {          // AgHandSide as the kernel reads it
    const float* dist2; const int* face_id; const float* bary; const float* vertices; const float* normals; const float* cano_vertices;
    const int* faces; const float* blob;
    int V, F;
    float mn[3], mx[3];
};

struct Params {
    long long N, n_tiles;
    float centre_y, b;
    const float* points; const float* cano_xyz; const float* sdf_in; const float* density_in; const float* color_in;
    float* sdf; float* density; float* color;
    Side side[2];
};

using namespace ag::mlp;

__device__ __forceinline__ float norm_axis(float x, float mn, float mx) { return (2.0f * (x - 0.5f * (mx + mn))) / (mx - mn); }

// the two gates of a canonical point; the only code that decides whether a point is active, in both kernels
__device__ __forceinline__ void gates(float cx, float cy, float lmn, float lmx, float rmn, float rmx, float centre_y, float& gl, float& gr)
{
    gl = sigmoid(25.0f * (norm_axis(cx, lmn, lmx) + 0.8f));
    gr = sigmoid(-25.0f * (norm_axis(cx, rmn, rmx) - 0.8f));
    if (cy < centre_y) { gl = 0.0f; gr = 0.0f; }
}

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

__global__ void __launch_bounds__(256) hand_gate_kernel(const float* __restrict__ cano_xyz, long long N, float lmn, float lmx, float rmn, float rmx,
                                                        float centre_y, unsigned char* __restrict__ active)
{
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        float gl, gr;
        gates(cano_xyz[(size_t)n * 3], cano_xyz[(size_t)n * 3 + 1], lmn, lmx, rmn, rmx, centre_y, gl, gr);
        active[n] = (gl != 0.0f || gr != 0.0f) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(kThreads) hand_fuse_kernel(Plan plan, Params a)
{
    __shared__ __attribute__((aligned(16))) float act_lds[2 * 2 * kPoints * kStride];   // [hand][buffer][point][kStride]
    __shared__ float s_w[2 * kPoints];                                                     // raw weight (gate, 0 where the hand is missing)
    __shared__ float s_sdf[2 * kPoints];
    __shared__ float s_col[2 * kPoints * 4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int hand_w = wave / kWavesPerHand, wave_h = wave % kWavesPerHand;
    const bool want_color = a.color != nullptr;
    const int e_cols = 3 + 6 * plan.L;                 // sdf_h sits in column e_cols
    const int Kp0 = plan.layer[0].Kp;
    const float alpha = 1.0f / a.b;

    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long p0 = tile * kPoints;
        // ---- A: one thread per (hand, point)
        int has_weight = 0;
        if (tid < 2 * kPoints) {
            const int hd = tid >> 5, pt = tid & 31;
            const long long n = p0 + pt;
            float w = 0.0f, sd = 0.0f, x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
            if (n < a.N) {
                const Side& s = a.side[hd];
                float gl, gr;
                gates(a.cano_xyz[(size_t)n * 3], a.cano_xyz[(size_t)n * 3 + 1], a.side[0].mn[0], a.side[0].mx[0], a.side[1].mn[0], a.side[1].mx[0],
                      a.centre_y, gl, gr);
                const float g = hd == 0 ? gl : gr;
                const int f = s.face_id[n];
                bool ok = f >= 0 && f < s.F;
                int i0 = 0, i1 = 0, i2 = 0;
                if (ok) {
                    i0 = s.faces[(size_t)f * 3]; i1 = s.faces[(size_t)f * 3 + 1]; i2 = s.faces[(size_t)f * 3 + 2];
                    ok = i0 >= 0 && i0 < s.V && i1 >= 0 && i1 < s.V && i2 >= 0 && i2 < s.V;
                }
                if (ok && g != 0.0f) {
                    w = g;
                    const float b0 = s.bary[(size_t)n * 3], b1 = s.bary[(size_t)n * 3 + 1], b2 = s.bary[(size_t)n * 3 + 2];
                    float x[3], q[3], nr[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float c0 = norm_axis(s.cano_vertices[(size_t)i0 * 3 + c], s.mn[c], s.mx[c]);
                        const float c1 = norm_axis(s.cano_vertices[(size_t)i1 * 3 + c], s.mn[c], s.mx[c]);
                        const float c2 = norm_axis(s.cano_vertices[(size_t)i2 * 3 + c], s.mn[c], s.mx[c]);
                        x[c] = (b0 * c0 + b1 * c1) + b2 * c2;
                        q[c] = (b0 * s.vertices[(size_t)i0 * 3 + c] + b1 * s.vertices[(size_t)i1 * 3 + c]) + b2 * s.vertices[(size_t)i2 * 3 + c];
                        nr[c] = (b0 * s.normals[(size_t)i0 * 3 + c] + b1 * s.normals[(size_t)i1 * 3 + c]) + b2 * s.normals[(size_t)i2 * 3 + c];
                    }
                    const float t = dot3(nr[0], nr[1], nr[2], a.points[(size_t)n * 3] - q[0], a.points[(size_t)n * 3 + 1] - q[1],
                                         a.points[(size_t)n * 3 + 2] - q[2]);
                    const float sg = t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : 0.0f);
                    sd = (-sg) * sqrtf(s.dist2[n]);
                    x0 = x[0]; x1 = x[1]; x2 = x[2];
                }
            }
            float* row = act_lds + (size_t)(hd * 2 + 1) * kPoints * kStride + pt * kStride;     // buffer 1 is the first layer's input
            row[0] = x0; row[1] = x1; row[2] = x2;
            row[e_cols] = sd;
            s_w[tid] = w;
            s_sdf[tid] = sd;
            has_weight = w != 0.0f;
        }
        // a tile without any weight (most tiles of an uncompacted call) skips the embedding and both MLPs: D copies the body's values and
        // reads nothing of B and C.  The vote is the barrier's, so the branch is uniform over the workgroup.
        const int tile_active = __syncthreads_or(has_weight);
        // ---- B: the sin / cos columns and the padding of both hands' input rows
        if (want_color && tile_active) {
            const int per_point = 3 * plan.L;
            for (int e = tid; e < 2 * kPoints * per_point; e += kThreads) {
                const int rowi = e / per_point, r = e - rowi * per_point;       // rowi = hand * 32 + point
                const int fi = r / 3, axis = r - 3 * fi;
                float* row = act_lds + (size_t)((rowi >> 5) * 2 + 1) * kPoints * kStride + (rowi & 31) * kStride;
                const float v = row[axis] * (float)(1 << fi);
                row[3 + 6 * fi + axis] = sinf(v);
                row[6 + 6 * fi + axis] = cosf(v);
            }
            const int pad = Kp0 - (e_cols + 1);
            for (int e = tid; e < 2 * kPoints * pad; e += kThreads) {
                const int rowi = e / pad;
                act_lds[(size_t)((rowi >> 5) * 2 + 1) * kPoints * kStride + (rowi & 31) * kStride + e_cols + 1 + e % pad] = 0.0f;
            }
            __syncthreads();
            // ---- C: the colour MLP of hand `hand_w`
            float* in = act_lds + (size_t)(hand_w * 2 + 1) * kPoints * kStride;
            float* out = act_lds + (size_t)(hand_w * 2) * kPoints * kStride;
            const float* __restrict__ blob = a.side[hand_w].blob;
            for (int l = 0; l < plan.n_layers; ++l) {
                const LayerPlan lp = plan.layer[l];
                const bool last = l == plan.n_layers - 1;
                const int n_col_tiles = lp.Np >> 5;
                const size_t wstep = 2 * (size_t)lp.Np;                    // float4s between two groups of 8 k
                for (int t = wave_h; t < n_col_tiles; t += kWavesPerHand) {
                    const int n = t * 32 + i;
                    const float bias = blob[lp.b_off + n];
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = bias;
                    acc = products(acc, in + i * kStride + 4 * h, weights(blob, lp.w_off, lp.Np, n, h), wstep, lp.Kp >> 3);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = cd_row(r, h);
                        if (last) {
                            if (i < 3) s_col[(hand_w * kPoints + row) * 4 + i] = sigmoid(acc[r]);
                        } else {
                            out[row * kStride + n] = acc[r] > 0.0f ? acc[r] : 0.0f;
                        }
                    }
                }
                __syncthreads();
                float* s = in; in = out; out = s;
            }
        }
        // ---- D: one thread per point
        if (tid < kPoints && p0 + tid < a.N) {
            const long long n = p0 + tid;
            float wl = s_w[tid], wr = s_w[kPoints + tid];
            const float sdf_b = a.sdf_in[n];
            if (wl == 0.0f && wr == 0.0f) {
                a.sdf[n] = sdf_b;
                a.density[n] = a.density_in[n];
                if (want_color) {
                    const float c0 = a.color_in[(size_t)n * 3], c1 = a.color_in[(size_t)n * 3 + 1], c2 = a.color_in[(size_t)n * 3 + 2];
                    a.color[(size_t)n * 3] = c0; a.color[(size_t)n * 3 + 1] = c1; a.color[(size_t)n * 3 + 2] = c2;
                }
            } else {
                const float sum = wl + wr;
                const float s = sum > 1.0f ? sum : 1.0f;
                wl = wl / s;
                wr = wr / s;
                const float w = wl + wr;
                const float rest = 1.0f - w;
                const float tl = wl != 0.0f ? wl * s_sdf[tid] : 0.0f;
                const float tr = wr != 0.0f ? wr * s_sdf[kPoints + tid] : 0.0f;
                const float sdf = (tl + tr) + rest * sdf_b;
                float cb[3];
                if (want_color) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) cb[c] = a.color_in[(size_t)n * 3 + c];
                }
                a.sdf[n] = sdf;
                a.density[n] = sdf_density(-sdf, a.b, alpha);
                if (want_color) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float cl = wl != 0.0f ? wl * s_col[tid * 4 + c] : 0.0f;
                        const float cr = wr != 0.0f ? wr * s_col[(kPoints + tid) * 4 + c] : 0.0f;
                        a.color[(size_t)n * 3 + c] = (cl + cr) + rest * cb[c];
                    }
                }
            }
        }
        __syncthreads();      // s_w / s_col / the input rows are rewritten by the next tile
    }
}

// Validates `d` against the limits of the header and lays one hand's blob out; returns its floats through `total`.
int make_plan(const AgHandFusionDesc* d, Plan& plan, size_t& total)
{
    if (!d) { set_error("hand fusion: desc is NULL"); return AG_ERR_INVALID_ARGUMENT; }
    if (d->multires < 0 || d->multires > kMaxMultires) {
        set_error("hand fusion: multires = %d must be 0 .. %d", d->multires, kMaxMultires);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (d->n_layers < 2 || d->n_layers > AG_HAND_MAX_LAYERS) {
        set_error("hand fusion: n_layers = %d must be 2 .. %d", d->n_layers, AG_HAND_MAX_LAYERS);
        return AG_ERR_INVALID_ARGUMENT;
    }
    plan = Plan{};
    plan.n_layers = d->n_layers;
    plan.L = d->multires;
    size_t off = 0;
    int prev = 4 + 6 * d->multires;
    for (int l = 0; l < d->n_layers; ++l) {
        const bool last = l == d->n_layers - 1;
        const int width = d->width[l];
        if (last ? width != 3 : (width != 32 && width != 64)) {
            set_error("hand fusion: layer %d: width = %d (hidden layers 32 or 64, the last layer 3)", l, width);
            return AG_ERR_INVALID_ARGUMENT;
        }
        LayerPlan& lp = plan.layer[l];
        lp.Kp = pad8(prev);
        lp.Np = pad32(width);
        lp.width = width;
        lp.w_off = (unsigned)off;
        off += (size_t)lp.Kp * lp.Np;
        lp.b_off = (unsigned)off;
        off += (size_t)lp.Np;
        prev = width;
    }
    total = off;
    return AG_OK;
}

int fill_side(const AgHandSide& s, const char* what, bool want_color, Side& o)
{
    if (s.V < 0 || s.F < 0) { set_error("%s: V = %d and F = %d must not be negative", what, s.V, s.F); return AG_ERR_INVALID_ARGUMENT; }
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(s.bbox_min[c]) || !std::isfinite(s.bbox_max[c]) || !(s.bbox_max[c] > s.bbox_min[c])) {
            set_error("%s: the canonical box [%g, %g] of axis %d is empty or not finite", what, (double)s.bbox_min[c], (double)s.bbox_max[c], c);
            return AG_ERR_INVALID_ARGUMENT;
        }
    }
    if (!s.face_id) { set_error("%s: face_id is NULL", what); return AG_ERR_INVALID_ARGUMENT; }
    if (s.F > 0 && (!s.dist2 || !s.bary || !s.vertices || !s.normals || !s.cano_vertices || !s.faces)) {
        set_error("%s: null pointer among dist2, bary, vertices, normals, cano_vertices, faces", what);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if (int rc = want_color ? check_blob(what, s.blob) : AG_OK) return rc;
    o.dist2 = s.dist2; o.face_id = s.face_id; o.bary = s.bary; o.vertices = s.vertices; o.normals = s.normals; o.cano_vertices = s.cano_vertices;
    o.faces = s.faces; o.blob = s.blob;
    o.V = s.V; o.F = s.F;
    for (int c = 0; c < 3; ++c) { o.mn[c] = s.bbox_min[c]; o.mx[c] = s.bbox_max[c]; }
    return AG_OK;
}

int check_box(const float* box, const char* name)
{
    if (!box || !std::isfinite(box[0]) || !std::isfinite(box[1]) || !(box[1] > box[0])) {
        set_error("hand fusion gate: the %s box is NULL, empty or not finite", name);
        return AG_ERR_INVALID_ARGUMENT;
    }
    return AG_OK;
}

}  // namespace handfuse
}  // namespace ag

using namespace ag;
using namespace ag::handfuse;

extern "C" size_t ag_hand_field_fuse_args_bytes(void) { return sizeof(AgHandFieldFuseArgs); }

extern "C" size_t ag_hand_fusion_blob_floats(const AgHandFusionDesc* desc)
{
    Plan plan;
    size_t total = 0;
    if (make_plan(desc, plan, total) != AG_OK) return 0;
    return total;
}

extern "C" int ag_hand_field_gate(const float* cano_xyz, int64_t N, const float* left_box, const float* right_box, float centre_y, uint8_t* active,
                                  void* stream)
{
    if (N < 0 || N >= (1ll << 31)) { set_error("hand fusion gate: N = %lld must be 0 .. 2^31 - 1", (long long)N); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_box(left_box, "left")) return rc;
    if (int rc = check_box(right_box, "right")) return rc;
    if (!std::isfinite(centre_y)) { set_error("hand fusion gate: centre_y is not finite"); return AG_ERR_INVALID_ARGUMENT; }
    if (N == 0) return AG_OK;
    if (!cano_xyz || !active) { set_error("null pointer in ag_hand_field_gate"); return AG_ERR_INVALID_ARGUMENT; }
    const long long blocks = (N + 255) / 256;
    hipLaunchKernelGGL(hand_gate_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), cano_xyz,
                       (long long)N, left_box[0], left_box[1], right_box[0], right_box[1], centre_y, active);
    return check_hip(hipGetLastError(), "hand_gate_kernel");
}

extern "C" int ag_hand_field_fuse(const AgHandFieldFuseArgs* args, void* stream)
{
    if (!args) { set_error("hand fusion: args is NULL"); return AG_ERR_INVALID_ARGUMENT; }
    Plan plan;
    size_t total = 0;
    if (int rc = make_plan(&args->desc, plan, total)) return rc;
    const AgHandFieldFuseArgs& g = *args;
    if (int rc = check_sizes("hand fusion", g.N, INT32_MAX, g.blob_floats, total)) return rc;
    if (!(g.density_b > 0.f) || !std::isfinite(g.density_b) || !std::isfinite(g.centre_y)) {
        set_error("hand fusion: density_b = %g must be finite and positive and centre_y = %g finite", (double)g.density_b, (double)g.centre_y);
        return AG_ERR_INVALID_ARGUMENT;
    }
    if ((g.color == nullptr) != (g.color_in == nullptr)) { set_error("hand fusion: color and color_in must both be given or both be NULL"); return AG_ERR_INVALID_ARGUMENT; }
    Params p{};
    const bool want_color = g.color != nullptr;
    if (int rc = fill_side(g.left, "hand fusion: left hand", want_color, p.side[0])) return rc;
    if (int rc = fill_side(g.right, "hand fusion: right hand", want_color, p.side[1])) return rc;
    if (g.N == 0) return AG_OK;
    if (!g.points || !g.cano_xyz || !g.sdf_in || !g.density_in || !g.sdf || !g.density) { set_error("null pointer in ag_hand_field_fuse"); return AG_ERR_INVALID_ARGUMENT; }
    p.N = g.N;
    p.n_tiles = (g.N + kPoints - 1) / kPoints;
    p.centre_y = g.centre_y;
    p.b = g.density_b;
    p.points = g.points; p.cano_xyz = g.cano_xyz; p.sdf_in = g.sdf_in; p.density_in = g.density_in; p.color_in = g.color_in;
    p.sdf = g.sdf; p.density = g.density; p.color = g.color;
    unsigned grid = 0;                                                         // four workgroups fit a CU (LDS); the rest is the grid-stride loop
    if (int rc = persistent_grid(p.n_tiles, 16, "hand fusion device query", &grid)) return rc;
    hipLaunchKernelGGL(hand_fuse_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), plan, p);
    return check_hip(hipGetLastError(), "hand_fuse_kernel");
}
