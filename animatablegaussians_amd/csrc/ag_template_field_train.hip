// The template field's training path (include/ag_template_field_train.h): the field layer by layer with a stash of every layer's
// activations, and the reverse pass to the weights.  Three small kernels beside the fused field_kernel (ag_template_field.hip), all on the
// tile routine of ag_mlp_tile.h:
//   layer_kernel<false>   one layer's forward: 32 points' input rows (previous output | padded embedding) in LDS, every 32-column output
//                         tile from the bias in the fused kernel's k order, activation, stash (and sdf / color from the two last layers);
//   layer_kernel<true>    one layer's data gradient: the same routine with dZ as the rows, the transposed blob as the weights and a zero
//                         start; the epilogue multiplies by the previous layer's act' (from its stashed output) and writes that layer's dZ;
//   wgrad_kernel          dW = dZ^T X and db = sum dZ of one slab of points: a wave owns a 32-row strip of dW and up to 4 tiles of 32
//                         columns, both MFMA operands are coalesced row reads (lane (i, h): dZ[p + h][n0 + i], X[p + h][k0 + i]);
//   wgrad_reduce_kernel   adds the slabs' partials in ascending order into the plain [out][in] layout.
// embed_kernel fills the two embedding blocks of the stash and seed_kernel writes the upstream of a last layer.  No atomics anywhere.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the embedding and the activations must round as in ag_template_field.hip.
#include "ag_mlp_tile.h"
#include "../../include/ag_template_field_train.h"

namespace ag {
namespace field_train {

using namespace ag::mlp;

constexpr int kPoints = 32;
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxRow = 512 + 64;             // previous output (at most 512 + 32 as dZ of the last geometry layer) + padded embedding
constexpr int kRowStride = kMaxRow + 4;       // floats; 16-byte rows, 4 banks apart
static_assert((size_t)kPoints * kRowStride * sizeof(float) == 74240, "two workgroups per CU (160 KiB of LDS)");
constexpr int kSlab = AG_FIELD_TRAIN_SLAB;
constexpr int kWgradWaves = 4;                // independent waves of a wgrad workgroup
constexpr int kWgradTiles = 4;                // 32-column tiles of dW per wave: one dZ read feeds 4 MFMAs
constexpr long long kMaxN = 2147483647LL;

enum { kHidden = 0, kGeoLast = 1, kColorLast = 2 };

struct Layer {
    int Ka, Ke, e_cols, Np, width, K, act, route, concat;
    int prev_cs, prev_cols;     // the stash block of the previous output: columns before it, its row length
    int out_cs;                 // the stash block of this layer's output (row length Np)
    size_t w_off, b_off, wt_off, gw_off, gb_off;
};

struct Table {
    int n_geo, n_all, L, Lv, Ep, Ev, cols, max_np;
    float beta;
    size_t blob, blob_t, gw, gb, max_partial;
    Layer layer[2 * AG_FIELD_MAX_LAYERS];
};

// `desc` is validated by ag_template_field_blob_floats (make_plan of ag_template_field.hip: the limits are stated once, there).
int make_table(const AgTemplateFieldDesc* d, Table& t)
{
    const size_t blob = ag_template_field_blob_floats(d);
    if (blob == 0) return AG_ERR_INVALID_ARGUMENT;
    t = Table{};
    t.n_geo = d->n_geo;
    t.n_all = d->n_geo + d->n_color;
    t.L = d->multires;
    t.Lv = d->multires_view;
    t.beta = d->softplus_beta;
    t.Ep = pad8(3 + 6 * d->multires);
    for (int l = 0; l < d->n_color; ++l)
        if (d->color[l].concat == AG_FIELD_CONCAT_VIEW) t.Ev = pad8(3 + 6 * d->multires_view);
    int cs = t.Ep + t.Ev, prev = 0, prev_cs = 0, prev_cols = 0;
    for (int l = 0; l < t.n_all; ++l) {
        const bool geo = l < d->n_geo;
        const int li = geo ? l : l - d->n_geo;
        const AgFieldLayer& a = geo ? d->geo[li] : d->color[li];
        const bool last = li == (geo ? d->n_geo : d->n_color) - 1;
        Layer& y = t.layer[l];
        y.Ka = prev;
        y.e_cols = a.K - prev;
        y.Ke = pad8(y.e_cols);
        y.Np = pad32(a.width);
        y.width = a.width;
        y.K = a.K;
        y.act = a.act;
        y.concat = a.concat;
        y.route = !last ? kHidden : geo ? kGeoLast : kColorLast;
        y.prev_cs = prev_cs;
        y.prev_cols = prev_cols;
        y.out_cs = cs;
        y.w_off = t.blob;
        y.b_off = t.blob + (size_t)(y.Ka + y.Ke) * y.Np;
        t.blob = y.b_off + y.Np;
        y.wt_off = t.blob_t;
        t.blob_t += (size_t)y.Np * y.Ka;
        y.gw_off = t.gw;
        y.gb_off = t.gb;
        t.gw += (size_t)a.width * a.K;
        t.gb += a.width;
        const size_t partial = (size_t)y.Np * (y.Ka + y.Ke) + y.Np;
        if (partial > t.max_partial) t.max_partial = partial;
        if (y.Np > t.max_np) t.max_np = y.Np;
        prev_cs = cs;
        prev_cols = y.Np;
        cs += y.Np;
        prev = (last && geo) ? a.width - 1 : a.width;
    }
    t.cols = cs;
    if (t.blob != blob) { set_error("template field training: the blob's layout disagrees with ag_template_field_blob_floats"); return AG_ERR_UNSUPPORTED; }
    return AG_OK;
}

inline size_t slabs_of(long long N) { return (size_t)((N + kSlab - 1) / kSlab); }
inline size_t stash_floats(const Table& t, long long N) { return (size_t)N * t.cols; }
inline size_t workspace_floats(const Table& t, long long N) { return 2 * (size_t)N * t.max_np + slabs_of(N) * t.max_partial; }

// ---- device -------------------------------------------------------------------------------------------------------------------------------
// as ag_template_field.hip's
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

// act' from the activated output y (the header's table)
__device__ __forceinline__ float slope_of_output(float y, int act, float beta)
{
    if (act == AG_FIELD_ACT_SOFTPLUS) return -expm1f(-(beta * y));
    if (act == AG_FIELD_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (act == AG_FIELD_ACT_SIGMOID) return y * (1.0f - y);
    return 1.0f;
}

// emb(x, L) of every point into its stash block [N][cols_pad], the padding zero; src == nullptr reads as zero.  One thread per (point,
// frequency, axis), the expressions of embed_tile in ag_template_field.hip.
__global__ void __launch_bounds__(256) embed_kernel(const float* __restrict__ src, long long N, int L, int cols_pad, float* __restrict__ out)
{
    const int per_point = 3 * (L + 1), cols = 3 + 6 * L;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * per_point) return;
    const long long p = e / per_point;
    const int r = (int)(e - p * per_point);
    const int fi = r / 3, axis = r - 3 * fi;
    const float x = src != nullptr ? src[(size_t)p * 3 + axis] : 0.0f;
    float* row = out + (size_t)p * cols_pad;
    if (fi == 0) {
        row[axis] = x;
    } else {
        const float v = x * (float)(1 << (fi - 1));
        row[3 + 6 * (fi - 1) + axis] = sinf(v);
        row[6 + 6 * (fi - 1) + axis] = cosf(v);
    }
    if (r == 0) for (int c = cols; c < cols_pad; ++c) row[c] = 0.0f;      // at most 7 padding columns
}

struct LayerArgs {
    const float* rows;       // [N][rows_stride]: the first Ka columns go to LDS
    int rows_stride, Ka;
    const float* emb;        // [N][emb_stride]: Ke columns behind them (forward only)
    int emb_stride, Ke;
    const float* w;          // the layer's block of the blob (forward) or of the transposed blob (reverse)
    const float* bias;       // forward only
    int n_cols;              // output columns of the block (a multiple of 32): the layer's Np (forward), its Ka (reverse)
    int act, route;          // forward: this layer's; reverse: act of the PREVIOUS layer
    float beta;
    long long N;
    float* out;              // [N][out_stride]: the stash block (forward), the previous layer's dZ (reverse)
    int out_stride;
    const float* y_prev;     // reverse: the previous layer's stashed output [N][out_stride]
    float* sdf;
    float* color;            // forward, the two last layers
};

// kReverse false: a layer's forward; true: its data gradient.  One text for the rows, the tiles and the products.
template <bool kReverse>
__global__ void __launch_bounds__(kThreads) layer_kernel(LayerArgs a)
{
    __shared__ __attribute__((aligned(16))) float rows[kPoints * kRowStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const long long p0 = (long long)blockIdx.x * kPoints;
    const int Kp = a.Ka + a.Ke, stride = Kp + 4;
    const int qa = a.Ka >> 2, qe = a.Ke >> 2;              // float4s per row
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int e = threadIdx.x; e < kPoints * qa; e += kThreads) {
        const int p = e / qa, c = e - p * qa;
        const float4 v = p0 + p < a.N ? *reinterpret_cast<const float4*>(a.rows + (size_t)(p0 + p) * a.rows_stride + 4 * c) : zero4;
        *reinterpret_cast<float4*>(rows + p * stride + 4 * c) = v;
    }
    for (int e = threadIdx.x; e < kPoints * qe; e += kThreads) {
        const int p = e / qe, c = e - p * qe;
        const float4 v = p0 + p < a.N ? *reinterpret_cast<const float4*>(a.emb + (size_t)(p0 + p) * a.emb_stride + 4 * c) : zero4;
        *reinterpret_cast<float4*>(rows + p * stride + a.Ka + 4 * c) = v;
    }
    __syncthreads();
    const int n_col_tiles = a.n_cols >> 5;
    const size_t wstep = 2 * (size_t)a.n_cols;
    for (int t = wave; t < n_col_tiles; t += kWaves) {
        const int n = t * 32 + i;
        const float start = kReverse ? 0.0f : a.bias[n];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = start;
        acc = products(acc, rows + i * stride + 4 * h, weights(a.w, 0, a.n_cols, n, h), wstep, Kp >> 3);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long p = p0 + cd_row(r, h);
            if (p >= a.N) continue;
            const size_t at = (size_t)p * a.out_stride + n;
            if constexpr (kReverse) {
                a.out[at] = acc[r] * slope_of_output(a.act == AG_FIELD_ACT_NONE ? 0.0f : a.y_prev[at], a.act, a.beta);
            } else {
                const float v = activate(acc[r], a.act, a.beta);
                a.out[at] = v;
                if (a.route == kGeoLast && t == n_col_tiles - 1 && i == 0) a.sdf[p] = -v;
                if (a.route == kColorLast && i < 3 && a.color != nullptr) a.color[(size_t)p * 3 + i] = v;
            }
        }
    }
}

// The upstream of a last layer into columns [c0, Np) of its dZ [N][Np].  colour: g_color * y (1 - y) in columns 0 .. 2 (y the stashed
// sigmoid), zero elsewhere; geometry: -g_sdf in column Np - 32, zero elsewhere.  A NULL gradient reads as zero.
__global__ void __launch_bounds__(256) seed_kernel(float* __restrict__ dz, long long N, int Np, int c0, int colour, const float* __restrict__ g,
                                                   const float* __restrict__ y)
{
    const int span = Np - c0;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * span) return;
    const long long p = e / span;
    const int c = c0 + (int)(e - p * span);
    float v = 0.0f;
    if (g != nullptr) {
        if (colour) {
            if (c < 3) v = g[(size_t)p * 3 + c] * slope_of_output(y[(size_t)p * Np + c], AG_FIELD_ACT_SIGMOID, 0.0f);
        } else if (c == Np - 32) {
            v = -g[p];
        }
    }
    dz[(size_t)p * Np + c] = v;
}

struct WgradArgs {
    const float* dz;         // [N][Np]
    int Np;
    const float* xa;         // [N][xa_stride]: the Ka previous-output columns of X
    int xa_stride, Ka;
    const float* xe;         // [N][xe_stride]: the Ke embedding columns behind them
    int xe_stride, Ke;
    long long N;
    float* partial;          // [slab][Np * Kp + Np]
    int n_strips, n_groups;  // 32-row strips of dW, groups of kWgradTiles column tiles
    long long n_items;       // slabs * n_strips * n_groups waves
};

__global__ void __launch_bounds__(64 * kWgradWaves) wgrad_kernel(WgradArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const long long item = (long long)blockIdx.x * kWgradWaves + (threadIdx.x >> 6);
    if (item >= a.n_items) return;                          // a whole wave leaves
    const int group = (int)(item % a.n_groups);
    const int strip = (int)((item / a.n_groups) % a.n_strips);
    const long long slab = item / ((long long)a.n_groups * a.n_strips);
    const int Kp = a.Ka + a.Ke, n0 = strip * 32;
    const float* x[kWgradTiles];
    int xs[kWgradTiles];
#pragma unroll
    for (int j = 0; j < kWgradTiles; ++j) {
        const int k = (group * kWgradTiles + j) * 32 + i;
        if (k < a.Ka) { x[j] = a.xa + k; xs[j] = a.xa_stride; }
        else if (k < Kp) { x[j] = a.xe + (k - a.Ka); xs[j] = a.xe_stride; }
        else { x[j] = a.dz + n0 + i; xs[j] = a.Np; }          // a tile column past Kp: any readable address, its products are never stored
    }
    const long long p_begin = slab * kSlab, p_end = p_begin + kSlab < a.N ? p_begin + kSlab : a.N;
    f32x16 acc[kWgradTiles];
#pragma unroll
    for (int j = 0; j < kWgradTiles; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    float bsum = 0.0f;
    const float* dz = a.dz + n0 + i;
    const int n_pairs = (int)((p_end - p_begin + 1) / 2);
    for (int q = 0; q < n_pairs; ++q) {
        const long long p = p_begin + 2 * q + h;
        const bool in = p < p_end;                          // only the odd half of a ragged slab's last pair is outside
        const size_t pc = (size_t)(in ? p : p_end - 1);     // read a point of the slab anyway, count it as zero: no branch around the loads
        const float dr = dz[pc * a.Np];
        float v[kWgradTiles];
#pragma unroll
        for (int j = 0; j < kWgradTiles; ++j) v[j] = x[j][pc * xs[j]];
        const float d = in ? dr : 0.0f;
#pragma unroll
        for (int j = 0; j < kWgradTiles; ++j) v[j] = in ? v[j] : 0.0f;
#pragma unroll
        for (int j = 0; j < kWgradTiles; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(d, v[j], acc[j], 0, 0, 0);
        bsum += d;
    }
    float* part = a.partial + (size_t)slab * ((size_t)a.Np * Kp + a.Np);
#pragma unroll
    for (int j = 0; j < kWgradTiles; ++j) {
        const int k = (group * kWgradTiles + j) * 32 + i;
        if (k >= Kp) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[(size_t)(n0 + cd_row(r, h)) * Kp + k] = acc[j][r];
    }
    const float other = __shfl_xor(bsum, 32);
    if (group == 0 && h == 0) part[(size_t)a.Np * Kp + n0 + i] = bsum + other;      // even points + odd points
}

// One thread per element of the plain dW [width][K] and db [width]: the slabs' partials in ascending order.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ partial, int n_slabs, int Np, int Kp, int width, int K, int geo_last,
                                                           float* __restrict__ gw, float* __restrict__ gb)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_w = width * K;
    if (e >= n_w + width) return;
    const int o = e < n_w ? e / K : e - n_w;
    const int n = geo_last ? (o == 0 ? Np - 32 : o - 1) : o;       // the blob's packed column of output o
    const size_t stride = (size_t)Np * Kp + Np;
    const size_t at = e < n_w ? (size_t)n * Kp + (e - o * K) : (size_t)Np * Kp + n;
    float s = 0.0f;
    for (int b = 0; b < n_slabs; ++b) s += partial[b * stride + at];
    if (e < n_w) gw[e] = s; else gb[o] = s;
}

int check_buffer(const char* what, const void* p, size_t floats, size_t expected)
{
    if (floats != expected) { set_error("template field training: %s of %zu floats, %zu expected", what, floats, expected); return AG_ERR_INVALID_ARGUMENT; }
    if (expected != 0 && !p) { set_error("template field training: %s is NULL", what); return AG_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) { set_error("template field training: the %s is not 16-byte aligned", what); return AG_ERR_INVALID_ARGUMENT; }
    return AG_OK;
}

inline unsigned blocks_of(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace field_train
}  // namespace ag

using namespace ag;
using namespace ag::field_train;

extern "C" int64_t ag_template_field_train_slab(void) { return kSlab; }

extern "C" size_t ag_template_field_train_blob_t_floats(const AgTemplateFieldDesc* desc)
{
    Table t;
    return make_table(desc, t) == AG_OK ? t.blob_t : 0;
}

static bool table_for(const AgTemplateFieldDesc* desc, int64_t N, Table& t)
{
    if (make_table(desc, t) != AG_OK) return false;
    if (N < 0 || N > kMaxN) { set_error("template field training: N = %lld must be 0 .. %lld", (long long)N, kMaxN); return false; }
    return true;
}

extern "C" size_t ag_template_field_train_stash_floats(const AgTemplateFieldDesc* desc, int64_t N)
{
    Table t;
    return table_for(desc, N, t) ? stash_floats(t, N) : 0;
}

extern "C" size_t ag_template_field_train_workspace_floats(const AgTemplateFieldDesc* desc, int64_t N)
{
    Table t;
    return table_for(desc, N, t) ? workspace_floats(t, N) : 0;
}

extern "C" int ag_template_field_train_forward(const AgTemplateFieldDesc* desc, const float* blob, size_t blob_floats, const float* xyz, const float* viewdirs,
                                               int64_t N, float* stash, size_t stash_fl, float* sdf, float* color, void* stream)
{
    Table t;
    if (int rc = make_table(desc, t)) return rc;
    if (color != nullptr && desc->n_color == 0) { set_error("template field training: colour requested from a field without a colour MLP"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_sizes("template field training", N, kMaxN, blob_floats, t.blob)) return rc;
    if (int rc = check_buffer("stash", stash, stash_fl, stash_floats(t, N))) return rc;
    if (N == 0) return AG_OK;
    if (!xyz || !sdf) { set_error("null pointer in ag_template_field_train_forward"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_blob("template field training", blob)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* emb_pos = stash;
    float* emb_view = stash + (size_t)N * t.Ep;
    hipLaunchKernelGGL(embed_kernel, dim3(blocks_of((long long)N * 3 * (t.L + 1), 256)), dim3(256), 0, s, xyz, (long long)N, t.L, t.Ep, emb_pos);
    const int n_run = color != nullptr ? t.n_all : t.n_geo;
    if (t.Ev > 0 && color != nullptr)
        hipLaunchKernelGGL(embed_kernel, dim3(blocks_of((long long)N * 3 * (t.Lv + 1), 256)), dim3(256), 0, s, viewdirs, (long long)N, t.Lv, t.Ev, emb_view);
    for (int l = 0; l < n_run; ++l) {
        const Layer& y = t.layer[l];
        LayerArgs a{};
        a.rows = stash + (size_t)N * y.prev_cs;
        a.rows_stride = y.prev_cols;
        a.Ka = y.Ka;
        a.emb = y.concat == AG_FIELD_CONCAT_VIEW ? emb_view : emb_pos;
        a.emb_stride = y.concat == AG_FIELD_CONCAT_VIEW ? t.Ev : t.Ep;
        a.Ke = y.Ke;
        a.w = blob + y.w_off;
        a.bias = blob + y.b_off;
        a.n_cols = y.Np;
        a.act = y.act;
        a.route = y.route;
        a.beta = t.beta;
        a.N = N;
        a.out = stash + (size_t)N * y.out_cs;
        a.out_stride = y.Np;
        a.sdf = sdf;
        a.color = color;
        hipLaunchKernelGGL(layer_kernel<false>, dim3(blocks_of(N, kPoints)), dim3(kThreads), 0, s, a);
    }
    return check_hip(hipGetLastError(), "template field training forward");
}

extern "C" int ag_template_field_train_backward(const AgTemplateFieldDesc* desc, const float* blob_t, size_t blob_t_floats, const float* stash, size_t stash_fl,
                                                const float* g_sdf, const float* g_color, int64_t N, float* workspace, size_t workspace_fl, float* g_weight,
                                                float* g_bias, void* stream)
{
    Table t;
    if (int rc = make_table(desc, t)) return rc;
    if (g_color != nullptr && desc->n_color == 0) { set_error("template field training: a colour gradient for a field without a colour MLP"); return AG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_sizes("template field training (transposed blob)", N, kMaxN, blob_t_floats, t.blob_t)) return rc;
    if (int rc = check_buffer("stash", stash, stash_fl, stash_floats(t, N))) return rc;
    if (int rc = check_buffer("workspace", workspace, workspace_fl, workspace_floats(t, N))) return rc;
    if (!g_weight || !g_bias) { set_error("null pointer in ag_template_field_train_backward"); return AG_ERR_INVALID_ARGUMENT; }
    if (t.blob_t != 0) { if (int rc = check_blob("template field training (transposed blob)", blob_t)) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_run = (g_color != nullptr && N > 0) ? t.n_all : (N > 0 ? t.n_geo : 0);
    if (n_run < t.n_all) {                                  // the layers not walked: zeros
        const size_t w0 = n_run == 0 ? 0 : t.layer[n_run].gw_off, b0 = n_run == 0 ? 0 : t.layer[n_run].gb_off;
        if (int rc = check_hip(hipMemsetAsync(g_weight + w0, 0, (t.gw - w0) * sizeof(float), s), "template field training: zero weight gradients")) return rc;
        if (int rc = check_hip(hipMemsetAsync(g_bias + b0, 0, (t.gb - b0) * sizeof(float), s), "template field training: zero bias gradients")) return rc;
    }
    if (N == 0) return AG_OK;
    float* cur = workspace;
    float* nxt = workspace + (size_t)N * t.max_np;
    float* partial = workspace + 2 * (size_t)N * t.max_np;
    const int n_slabs = (int)slabs_of(N);
    const Layer& top = t.layer[n_run - 1];
    if (g_color != nullptr)
        hipLaunchKernelGGL(seed_kernel, dim3(blocks_of((long long)N * top.Np, 256)), dim3(256), 0, s, cur, (long long)N, top.Np, 0, 1, g_color,
                           stash + (size_t)N * top.out_cs);
    else
        hipLaunchKernelGGL(seed_kernel, dim3(blocks_of((long long)N * top.Np, 256)), dim3(256), 0, s, cur, (long long)N, top.Np, 0, 0, g_sdf,
                           static_cast<const float*>(nullptr));
    for (int l = n_run - 1; l >= 0; --l) {
        const Layer& y = t.layer[l];
        if (l == t.n_geo - 1 && g_color != nullptr)         // the features' columns came from the first colour layer: the SDF tile beside them
            hipLaunchKernelGGL(seed_kernel, dim3(blocks_of((long long)N * 32, 256)), dim3(256), 0, s, cur, (long long)N, y.Np, y.Np - 32, 0, g_sdf,
                               static_cast<const float*>(nullptr));
        const float* emb = y.concat == AG_FIELD_CONCAT_VIEW ? stash + (size_t)N * t.Ep : stash;
        const int emb_stride = y.concat == AG_FIELD_CONCAT_VIEW ? t.Ev : t.Ep;
        const int Kp = y.Ka + y.Ke;
        WgradArgs w{};
        w.dz = cur;
        w.Np = y.Np;
        w.xa = stash + (size_t)N * y.prev_cs;
        w.xa_stride = y.prev_cols;
        w.Ka = y.Ka;
        w.xe = emb;
        w.xe_stride = emb_stride;
        w.Ke = y.Ke;
        w.N = N;
        w.partial = partial;
        w.n_strips = y.Np / 32;
        w.n_groups = (Kp + 32 * kWgradTiles - 1) / (32 * kWgradTiles);
        w.n_items = (long long)n_slabs * w.n_strips * w.n_groups;
        hipLaunchKernelGGL(wgrad_kernel, dim3(blocks_of(w.n_items, kWgradWaves)), dim3(64 * kWgradWaves), 0, s, w);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks_of((long long)y.width * y.K + y.width, 256)), dim3(256), 0, s, partial, n_slabs, y.Np, Kp,
                           y.width, y.K, y.route == kGeoLast ? 1 : 0, g_weight + y.gw_off, g_bias + y.gb_off);
        if (l == 0) break;
        const Layer& below = t.layer[l - 1];
        LayerArgs a{};
        a.rows = cur;
        a.rows_stride = y.Np;
        a.Ka = y.Np;
        a.w = blob_t + y.wt_off;
        a.n_cols = y.Ka;
        a.act = below.act;
        a.beta = t.beta;
        a.N = N;
        a.out = nxt;
        a.out_stride = below.Np;
        a.y_prev = stash + (size_t)N * below.out_cs;
        hipLaunchKernelGGL(layer_kernel<true>, dim3(blocks_of(N, kPoints)), dim3(kThreads), 0, s, a);
        float* swap = cur; cur = nxt; nxt = swap;
    }
    return check_hip(hipGetLastError(), "template field training backward");
}
