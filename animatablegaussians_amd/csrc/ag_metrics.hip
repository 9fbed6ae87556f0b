// Image-quality sums of two image batches in one pass (include/ag_metrics.h): per image the fp64 sum of squared errors and the fp64
// sum of the SSIM map, optionally the map itself.
//
// One workgroup of 256 threads owns a kTileH x kTileW block of window centres of one image, all channels:
//   1. it loads the block plus the p-wide halo of both images once into LDS, walking the interleaved W*C row so that consecutive
//      lanes read consecutive floats, and takes the squared error of the pixels it owns on the way;
//   2. per channel: the horizontal pass writes the five window moments of every row into LDS (fp64), the vertical pass reads them
//      back down the columns (consecutive lanes, consecutive doubles) and evaluates S;
//   3. it reduces its two sums through the wave (shuffles) and the four waves (LDS, fixed order) and stores one pair.
// A second launch adds the pairs of each image in a fixed order.  No atomics anywhere.
//
// fp64 throughout: a product of two fp32 values is exact in fp64, so the window sums carry fp64 rounding only and the variances
// uxx - ux^2 (differences of nearly equal numbers on the flat white background of an evaluation frame) lose nothing that matters.
// Per 512-centre tile and channel that is ~47 000 fp64 FMAs against 12 KiB of algorithmic traffic.

#include "ag_common.h"
#include "../../include/ag_metrics.h"

namespace ag {
namespace {

constexpr int kTileH = AG_METRICS_TILE_H, kTileW = AG_METRICS_TILE_W, kThreads = 256;
static_assert(kTileW == 32 && kTileH * kTileW == 2 * kThreads, "the vertical pass gives each thread the centres (i, j) and (i + 8, j)");

struct Taps { double k[AG_METRICS_MAX_TAPS]; };

__host__ __device__ inline size_t metrics_lds_bytes(int p, int C)
{
    const size_t rh = kTileH + 2 * p;
    return (5 * rh * kTileW + 8) * sizeof(double) + 2 * rh * (size_t)(kTileW + 2 * p) * C * sizeof(float);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0
}

template <int P>
__global__ __launch_bounds__(kThreads) void psnr_ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int C,
                                                                  Taps taps, double cn, double C1, double C2, int ntx, int nty,
                                                                  float* __restrict__ ssim_map, double* __restrict__ partial)
{
    constexpr int kW = 2 * P + 1, kRH = kTileH + 2 * P;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* mom = reinterpret_cast<double*>(smem);                 // [5][kRH][kTileW]
    double* red = mom + 5 * kRH * kTileW;                          // [4 waves][2]
    const int RS = (kTileW + 2 * P) * C;                           // floats per LDS row
    float* sx = reinterpret_cast<float*>(red + 8);                 // [kRH][RS]
    float* sy = sx + kRH * RS;

    const int t = threadIdx.x;
    const int per_image = ntx * nty;
    const int b = blockIdx.x / per_image, rem = blockIdx.x - b * per_image;
    const int tyi = rem / ntx, txi = rem - tyi * ntx;
    const int Ho = H - 2 * P, Wo = W - 2 * P;
    const int ty0 = tyi * kTileH, tx0 = txi * kTileW;              // first centre of the tile, in map coordinates
    const int th = min(kTileH, Ho - ty0), tw = min(kTileW, Wo - tx0);
    const int rows = th + 2 * P, rowlen = (tw + 2 * P) * C;        // the block read: image rows ty0 .. ty0 + rows - 1, all inside the image
    // squared error: the pixels under the tile's centres, plus the border beside a tile that touches it
    const int own_r0 = tyi == 0 ? 0 : P, own_r1 = tyi == nty - 1 ? rows : th + P;
    const int own_k0 = txi == 0 ? 0 : P * C, own_k1 = txi == ntx - 1 ? rowlen : (tw + P) * C;

    const size_t image = (size_t)b * H * W * C;
    double sq = 0.0;
    for (int r = t >> 6; r < rows; r += kThreads / 64) {           // one wave per row segment: consecutive lanes, consecutive floats
        const size_t g = image + ((size_t)(ty0 + r) * W + tx0) * C;
        const bool own_row = r >= own_r0 && r < own_r1;
        for (int k = t & 63; k < rowlen; k += 64) {
            const float a = x[g + k], c = y[g + k];
            sx[r * RS + k] = a;
            sy[r * RS + k] = c;
            if (own_row && k >= own_k0 && k < own_k1) {
                const double d = (double)a - (double)c;
                sq += d * d;
            }
        }
    }
    __syncthreads();

    double ss = 0.0;
    const int j = t & (kTileW - 1), i0 = t >> 5;
    for (int c = 0; c < C; ++c) {
        for (int idx = t; idx < rows * kTileW; idx += kThreads) {
            const int r = idx >> 5, jj = idx & (kTileW - 1);
            if (jj >= tw) continue;
            const float* px = sx + r * RS + jj * C + c;
            const float* py = sy + r * RS + jj * C + c;
            double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
            for (int q = 0; q < kW; ++q) {
                const double a = px[q * C], d = py[q * C], k = taps.k[q];
                ax += k * a; ay += k * d; axx += k * (a * a); ayy += k * (d * d); axy += k * (a * d);
            }
            double* m = mom + r * kTileW + jj;
            m[0] = ax; m[kRH * kTileW] = ay; m[2 * kRH * kTileW] = axx; m[3 * kRH * kTileW] = ayy; m[4 * kRH * kTileW] = axy;
        }
        __syncthreads();
        if (j < tw) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int i = i0 + half * (kTileH / 2);
                if (i >= th) continue;
                const double* m = mom + i * kTileW + j;
                double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
                for (int q = 0; q < kW; ++q) {
                    const double k = taps.k[q];
                    ux += k * m[q * kTileW]; uy += k * m[(kRH + q) * kTileW]; uxx += k * m[(2 * kRH + q) * kTileW];
                    uyy += k * m[(3 * kRH + q) * kTileW]; uxy += k * m[(4 * kRH + q) * kTileW];
                }
                const double vx = cn * (uxx - ux * ux), vy = cn * (uyy - uy * uy), vxy = cn * (uxy - ux * uy);
                const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
                ss += S;
                if (ssim_map) ssim_map[(((size_t)b * Ho + (ty0 + i)) * Wo + (tx0 + j)) * C + c] = (float)S;
            }
        }
        __syncthreads();
    }

    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if ((t & 63) == 0) { red[2 * (t >> 6)] = sq; red[2 * (t >> 6) + 1] = ss; }
    __syncthreads();
    if (t == 0) {
        partial[2 * (size_t)blockIdx.x] = ((red[0] + red[2]) + red[4]) + red[6];
        partial[2 * (size_t)blockIdx.x + 1] = ((red[1] + red[3]) + red[5]) + red[7];
    }
}

// one workgroup per image: thread t adds pairs t, t + 256, ... in that order, then the same fixed wave / workgroup reduction
__global__ __launch_bounds__(kThreads) void psnr_ssim_sum_kernel(const double* __restrict__ partial, int per_image, double* __restrict__ sq_err_sum,
                                                                 double* __restrict__ ssim_sum)
{
    __shared__ double red[8];
    const int t = threadIdx.x;
    const double* p = partial + 2 * (size_t)blockIdx.x * per_image;
    double sq = 0.0, ss = 0.0;
    for (int i = t; i < per_image; i += kThreads) { sq += p[2 * (size_t)i]; ss += p[2 * (size_t)i + 1]; }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if ((t & 63) == 0) { red[2 * (t >> 6)] = sq; red[2 * (t >> 6) + 1] = ss; }
    __syncthreads();
    if (t == 0) {
        sq_err_sum[blockIdx.x] = ((red[0] + red[2]) + red[4]) + red[6];
        ssim_sum[blockIdx.x] = ((red[1] + red[3]) + red[5]) + red[7];
    }
}

bool sizes_ok(long long B, long long H, long long W, int n_taps)
{
    return B >= 0 && n_taps >= 3 && n_taps <= AG_METRICS_MAX_TAPS && (n_taps & 1) && H >= n_taps && W >= n_taps;
}

long long tiles_per_image(int H, int W, int n_taps)
{
    const long long Ho = H - (n_taps - 1), Wo = W - (n_taps - 1);
    return ((Ho + kTileH - 1) / kTileH) * ((Wo + kTileW - 1) / kTileW);
}

template <int P>
int launch_tiles(long long tiles, size_t lds, hipStream_t s, const float* x, const float* y, int H, int W, int C, const Taps& taps, double cn,
                 double C1, double C2, int ntx, int nty, float* ssim_map, double* partial)
{
    if (lds > 64 * 1024) {   // a workgroup may hold up to 160 KiB of LDS on gfx950, beyond 64 KiB only on request
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&psnr_ssim_tile_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds), "hipFuncSetAttribute");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(psnr_ssim_tile_kernel<P>, dim3((unsigned)tiles), dim3(kThreads), lds, s, x, y, H, W, C, taps, cn, C1, C2, ntx, nty, ssim_map,
                       partial);
    return check_hip(hipGetLastError(), "psnr_ssim_tile_kernel");
}

}  // namespace
}  // namespace ag

using namespace ag;

extern "C" {

size_t ag_psnr_ssim_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_taps)
{
    if (!sizes_ok(B, H, W, n_taps)) return 0;
    return (size_t)B * (size_t)tiles_per_image(H, W, n_taps) * 2 * sizeof(double) + 256;
}

int ag_psnr_ssim(const float* x, const float* y, int32_t B, int32_t H, int32_t W, int32_t C, const double* taps, int32_t n_taps,
                 double cov_norm, double C1, double C2, double* sq_err_sum, double* ssim_sum, float* ssim_map, void* workspace,
                 size_t workspace_bytes, void* stream)
{
    if (n_taps < 3 || n_taps > AG_METRICS_MAX_TAPS || !(n_taps & 1)) { set_error("psnr_ssim: the window needs an odd tap count in 3..11, got %d", n_taps); return AG_ERR_INVALID_ARGUMENT; }
    if (C < 1 || C > 4) { set_error("psnr_ssim: 1 to 4 channels, got %d", C); return AG_ERR_INVALID_ARGUMENT; }
    if (!sizes_ok(B, H, W, n_taps)) { set_error("psnr_ssim: images of %d x %d are smaller than the window of %d (or B < 0)", H, W, n_taps); return AG_ERR_INVALID_ARGUMENT; }
    if (B == 0) return AG_OK;
    if (!x || !y || !taps || !sq_err_sum || !ssim_sum || !workspace) { set_error("null pointer in ag_psnr_ssim"); return AG_ERR_INVALID_ARGUMENT; }
    const int p = (n_taps - 1) / 2;
    const int Ho = H - 2 * p, Wo = W - 2 * p;
    const int nty = (Ho + kTileH - 1) / kTileH, ntx = (Wo + kTileW - 1) / kTileW;
    const long long per_image = (long long)nty * ntx, tiles = per_image * B;
    if (per_image > 0x7fffffffll || tiles > 0x7fffffffll) { set_error("psnr_ssim: more than 2^31 tiles"); return AG_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < ag_psnr_ssim_workspace_bytes(B, H, W, n_taps)) { set_error("psnr_ssim workspace too small"); return AG_ERR_SCRATCH_TOO_SMALL; }
    Taps k{};
    for (int i = 0; i < n_taps; ++i) k.k[i] = taps[i];
    double* partial = reinterpret_cast<double*>(aligned_base(workspace));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = metrics_lds_bytes(p, C);
    int rc;
    switch (p) {
        case 1: rc = launch_tiles<1>(tiles, lds, s, x, y, H, W, C, k, cov_norm, C1, C2, ntx, nty, ssim_map, partial); break;
        case 2: rc = launch_tiles<2>(tiles, lds, s, x, y, H, W, C, k, cov_norm, C1, C2, ntx, nty, ssim_map, partial); break;
        case 3: rc = launch_tiles<3>(tiles, lds, s, x, y, H, W, C, k, cov_norm, C1, C2, ntx, nty, ssim_map, partial); break;
        case 4: rc = launch_tiles<4>(tiles, lds, s, x, y, H, W, C, k, cov_norm, C1, C2, ntx, nty, ssim_map, partial); break;
        default: rc = launch_tiles<5>(tiles, lds, s, x, y, H, W, C, k, cov_norm, C1, C2, ntx, nty, ssim_map, partial); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(psnr_ssim_sum_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, partial, (int)per_image, sq_err_sum, ssim_sum);
    return check_hip(hipGetLastError(), "psnr_ssim_sum_kernel");
}

}  // extern "C"
