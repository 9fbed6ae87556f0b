// Trilinear sampler of a channel-last [X, Y, Z, C] volume (include/ag_weight_volume.h): the per-point skinning weights of a clothed
// template (CanoBlendWeightVolume.forward_weight) and its SDF.  Init-time, memory bound: 8 rows of 4 C bytes in, one row out per point.
//
// One thread per OUTPUT element (n, c): consecutive lanes hold consecutive channels of one point and, where a row ends, the first
// channels of the next point, so every corner read of a wave is one or two contiguous runs of the volume's rows and the output write
// is fully coalesced whatever C is (55 and 1 in the product).  Every lane recomputes its point's cell and weights (about 40 VALU
// operations against 9 memory instructions); sharing them through LDS would add a barrier to save arithmetic nobody waits for.
//
// Compiled WITHOUT fp contraction (build.sh EXACT): the header states the result as individually rounded fp32 operations, which is
// what the test oracle's float32 restatement (numpy has no FMA) evaluates.
#include "ag_common.h"
#include "../../include/ag_weight_volume.h"

namespace ag {
namespace {

struct VolumeArgs {
    int X, Y, Z, C;
    int scale;              // 1: u = (p - lo) / (hi - lo)
    float lo[3], hi[3];
    long long total;        // N * C
};

// cell index in [0, R - 1] and the two weights of one axis
__device__ __forceinline__ void axis_cell(float p, float lo, float hi, int scale, int R, int& i, float& f, float& e)
{
    float u = p;
    if (scale) u = (p - lo) / (hi - lo);
    const float g = 2.f * u - 1.f;
    float x = ((g + 1.f) / 2.f) * (float)(R - 1);
    x = fminf(fmaxf(x, 0.f), (float)(R - 1));        // fmaxf(NaN, 0) = 0
    const float fl = floorf(x);
    i = (int)fl;
    f = x - fl;
    e = (fl + 1.f) - x;
}

__global__ void __launch_bounds__(256) weight_volume_sample_kernel(VolumeArgs a, const float* __restrict__ volume, const float* __restrict__ points,
                                                                   float* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total) return;
    const long long n = (long long)((unsigned long long)t / (unsigned)a.C);
    const int c = (int)(t - n * a.C);
    int i0, i1, i2;
    float f0, f1, f2, e0, e1, e2;
    axis_cell(points[3 * n], a.lo[0], a.hi[0], a.scale, a.X, i0, f0, e0);
    axis_cell(points[3 * n + 1], a.lo[1], a.hi[1], a.scale, a.Y, i1, f1, e1);
    axis_cell(points[3 * n + 2], a.lo[2], a.hi[2], a.scale, a.Z, i2, f2, e2);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int da = k >> 2, db = (k >> 1) & 1, dc = k & 1;
        const int j0 = i0 + da, j1 = i1 + db, j2 = i2 + dc;
        const float w = ((dc ? f2 : e2) * (db ? f1 : e1)) * (da ? f0 : e0);
        if (j0 < a.X && j1 < a.Y && j2 < a.Z) {       // i_d >= 0 by the clamp; j_d = R_d only with weight 0
            const long long node = ((long long)j0 * a.Y + j1) * a.Z + j2;
            acc = acc + w * volume[node * a.C + c];
        }
    }
    out[t] = acc;
}

}  // namespace
}  // namespace ag

using namespace ag;

extern "C" int ag_weight_volume_sample(const float* volume, int32_t X, int32_t Y, int32_t Z, int32_t C, const float* points, int64_t N,
                                       const float* bounds, float* out, void* stream)
{
    if (X < 2 || Y < 2 || Z < 2) { set_error("weight volume: every resolution must be at least 2, got %d x %d x %d", X, Y, Z); return AG_ERR_INVALID_ARGUMENT; }
    if (C < 1 || N < 0) { set_error("weight volume: bad sizes C = %d, N = %lld", C, (long long)N); return AG_ERR_INVALID_ARGUMENT; }
    if (N == 0) return AG_OK;
    if (!volume || !points || !out) { set_error("null pointer in ag_weight_volume_sample"); return AG_ERR_INVALID_ARGUMENT; }
    if (N > (0x7fffffffll * 256) / C) { set_error("weight volume: N * C = %lld * %d outputs exceed one launch", (long long)N, C); return AG_ERR_INVALID_ARGUMENT; }
    VolumeArgs a;
    a.X = X; a.Y = Y; a.Z = Z; a.C = C;
    a.scale = bounds ? 1 : 0;
    for (int d = 0; d < 3; ++d) { a.lo[d] = bounds ? bounds[d] : 0.f; a.hi[d] = bounds ? bounds[3 + d] : 1.f; }
    a.total = (long long)N * C;
    hipLaunchKernelGGL(weight_volume_sample_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       a, volume, points, out);
    return check_hip(hipGetLastError(), "weight_volume_sample_kernel");
}
