// The per-ray cross-lane pieces of the template renderer's compositing, shared by ray_composite_kernel (ag_ray_march.hip) and
// ray_composite_backward_kernel (ag_ray_march_grad.hip).  The ONE statement of what makes the backward's T_s and w_s the forward's bit
// for bit (include/ag_ray_march.h, "ORDER of the product and of the sums"):
//   samples   one wavefront per ray; lane l of chunk k is sample 64 k + l; positions past S - 1 hold f = 1 and alpha = 0;
//   dist      dist_s = z_{s+1} - z_s, dist_{S-1} = z_{S-1} - z_{S-2};
//   product   P_l = f_0 * .. * f_l by six doubling steps o = 1, 2, 4, 8, 16, 32: every lane l >= o replaces p_l by p_{l-o} * p_l;
//   T         T of lane l = carry * (l == 0 ? 1 : P_{l-1});  carry = 1 for the first chunk, carry * P_63 for the next one;
//   sums      six butterfly steps o = 32, 16, 8, 4, 2, 1: v_l = v_l + v_{l xor o}, every lane ends with the chunk's sum
//             (wave_sum of ag_common.h).
// Every lane of the wavefront must call these (cross-lane moves).  Units that include this are compiled WITHOUT fp contraction.
#pragma once

#include "ag_common.h"
#include "../../include/ag_ray_march.h"

namespace ag {
namespace ray {

constexpr int kRayThreads = 256;                   // four rays (wavefronts) per workgroup

// z_s and dist_s of a valid sample s of the ray whose samples start at z_vals[row]
__device__ __forceinline__ float sample_dist(const float* __restrict__ z_vals, long long row, int s, int S, float& z)
{
    z = z_vals[row + s];
    const float zn = z_vals[row + min(s + 1, S - 1)];
    const float zl = s == S - 1 ? z_vals[row + S - 2] : z;
    return zn - zl;
}

// P_l of the chunk from f_l
__device__ __forceinline__ float product_scan(float p, int lane)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const float q = __shfl_up(p, o, 64);
        if (lane >= o) p = q * p;
    }
    return p;
}

__device__ __forceinline__ float transmittance(float p, float carry, int lane)
{
    const float before = __shfl_up(p, 1, 64);
    return carry * (lane == 0 ? 1.f : before);
}

__device__ __forceinline__ float next_carry(float p, float carry) { return carry * __shfl(p, 63, 64); }

// The counts ag_ray_sample, ag_ray_composite and ag_ray_composite_backward take (host)
inline bool bad_counts(const char* what, long long R, int S)
{
    if (R < 0) { set_error("%s: R = %lld is negative", what, R); return true; }
    if (S < AG_RAY_MIN_SAMPLES || S > AG_RAY_MAX_SAMPLES) {
        set_error("%s: S = %d is outside %d .. %d", what, S, AG_RAY_MIN_SAMPLES, AG_RAY_MAX_SAMPLES);
        return true;
    }
    if (R > (1ll << 31) / S || R > (1ll << 25)) { set_error("%s: R = %lld rays of %d samples exceed one launch (2^25 rays, 2^31 samples)", what, R, S); return true; }
    return false;
}

}  // namespace ray
}  // namespace ag
