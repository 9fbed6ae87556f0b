// Host walk of the inverse-skinning kernels (csrc/ag_inverse_skinning.hip): what one lane does is a host-callable function there, so
// this program runs every thread of ag_weight_volume_gradient and ag_inverse_skinning_init and every lane of every 16-lane group of
// ag_inverse_skinning_root_find on the CPU, in both gradient modes, and compares each BIT FOR BIT with the float32 run of
// tests/inverse_skinning_oracle.py.  The fold of the 24 lane sums across the group is the one step that cannot be walked as written
// (the kernel does it with DPP row rotations); it is restated here as the rotations 8, 4, 2, 1 over an array of 16 lanes, every lane
// kept, and all 16 lanes then take the step, so the walk also checks that they end with the same bits.  Arrays are malloc'ed at
// their exact sizes, so a host sanitizer sees every index the kernels form; it needs no GPU:
//   python tests/inverse_skinning_oracle.py /tmp/inverse_skinning_cases.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Ianimatablegaussians_amd/csrc profiles/ub/inverse_skinning_host_walk.hip -o profiles/ub/inverse_skinning_host_walk
//   profiles/ub/inverse_skinning_host_walk /tmp/inverse_skinning_cases.bin
// Prints one line per case and "TOTAL bad 0"; exit status 1 on any mismatch.
#define AG_INVERSE_SKINNING_HOST_ONLY
#include "../../animatablegaussians_amd/csrc/ag_inverse_skinning.hip"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ag::invskin;

namespace ag {
void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace ag

template <typename T>
static T* read_array(FILE* fh, size_t n)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (fread(p, sizeof(T), n, fh) != n) { fprintf(stderr, "truncated case file\n"); exit(2); }
    return p;
}

static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a == 0.f && b == 0.f) || (a != a && b != b); }     // +0 and -0 are one value

static long long compare(const char* what, const float* got, const float* want, size_t n)
{
    long long bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (!same(got[i], want[i])) { if (bad < 5) printf("  %s element %zu: %.9g / %.9g\n", what, i, got[i], want[i]); ++bad; }
    return bad;
}

// the group's fold as the kernel's four row rotations, every lane kept
static void row_fold_host(float v[kGroup])
{
    for (int rot = 8; rot > 0; rot >>= 1) {
        float read[kGroup];
        for (int l = 0; l < kGroup; ++l) read[l] = v[(l + kGroup - rot) % kGroup];          // row_ror: lane l reads lane l - rot
        for (int l = 0; l < kGroup; ++l) v[l] = v[l] + read[l];
    }
}

template <bool PRE>
static long long walk_root_find(const VolArgs& a, int B, const float* vol, const float* grad, const float* zero, const float* jnt_mats, const float* xt,
                                const float* xc_init, const uint8_t* active, float* out)
{
    long long disagree = 0;
    float* mats = (float*)malloc((size_t)12 * a.J * 4);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < 12 * a.J; ++i) mats[i] = jnt_mats[((size_t)b * a.J + i / 12) * 16 + i % 12];             // stage_matrices
        for (long long n = 0; n < a.N; ++n) {
            const long long i = b * a.N + n;
            float xc[kGroup][3];
            for (int l = 0; l < kGroup; ++l) for (int d = 0; d < 3; ++d) xc[l][d] = xc_init[3 * i + d];
            if (active[i])
                for (int it = 0; it < a.iterations; ++it) {
                    float acc[kGroup][24], col[kGroup];
                    for (int l = 0; l < kGroup; ++l) lane_partial<PRE>(a, vol, grad, zero, mats, xc[l], l, acc[l]);
                    for (int k = 0; k < 24; ++k) {
                        for (int l = 0; l < kGroup; ++l) col[l] = acc[l][k];
                        row_fold_host(col);
                        for (int l = 0; l < kGroup; ++l) acc[l][k] = col[l];
                    }
                    for (int l = 0; l < kGroup; ++l) newton_step(a, acc[l], xt + 3 * i, xc[l]);
                }
            for (int l = 1; l < kGroup; ++l) for (int d = 0; d < 3; ++d) if (!same(xc[l][d], xc[0][d])) ++disagree;
            for (int d = 0; d < 3; ++d) out[3 * i + d] = xc[0][d];
        }
    }
    free(mats);
    return disagree;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, fh) != 1) return 2;
    long long total_bad = 0;
    float* zero = (float*)malloc(4);
    *zero = 0.f;
    for (int cs = 0; cs < n_cases; ++cs) {
        int32_t* dims = read_array<int32_t>(fh, 7);
        const int X = dims[0], Y = dims[1], Z = dims[2], J = dims[3], B = dims[4], N = dims[5], iterations = dims[6];
        const size_t nodes = (size_t)X * Y * Z, P = (size_t)B * N;
        float* lam = read_array<float>(fh, 1);
        float* bounds = read_array<float>(fh, 6);
        float* spacing = read_array<float>(fh, 3);
        float* vol = read_array<float>(fh, nodes * J);
        float* jnt = read_array<float>(fh, (size_t)B * J * 16);
        float* xt = read_array<float>(fh, P * 3);
        float* xc_init = read_array<float>(fh, P * 3);
        uint8_t* active = read_array<uint8_t>(fh, P);
        float* weights = read_array<float>(fh, P * J);
        float* normals = read_array<float>(fh, P * 3);
        float* want_grad = read_array<float>(fh, nodes * J * 3);
        float* want_xc = read_array<float>(fh, P * 3);
        float* want_ip = read_array<float>(fh, P * 3);
        float* want_in = read_array<float>(fh, P * 3);
        VolArgs a = {};
        if (make_root_args(X, Y, Z, J, bounds, spacing, B, N, *lam, iterations, a)) return 2;
        long long bad = 0;
        // gradient_kernel: one thread per (node, channel)
        float* grad = (float*)malloc(nodes * J * 3 * 4);
        for (size_t t = 0; t < nodes * J; ++t) {
            const long long node = (long long)(t / J);
            const int j = (int)(t - node * J);
            const long long xy = node / Z;
            sobel_node(a, vol, zero, (int)(xy / Y), (int)(xy % Y), (int)(node - xy * Z), j, grad + 3 * t);
        }
        bad += compare("gradient", grad, want_grad, nodes * J * 3);
        // root_find_kernel in both modes
        float* out = (float*)malloc(P * 3 * 4);
        long long disagree = walk_root_find<false>(a, B, vol, nullptr, zero, jnt, xt, xc_init, active, out);
        bad += compare("root_find (on the fly)", out, want_xc, P * 3);
        memset(out, 0xff, P * 3 * 4);
        disagree += walk_root_find<true>(a, B, vol, grad, zero, jnt, xt, xc_init, active, out);
        bad += compare("root_find (gradient volume)", out, want_xc, P * 3);
        bad += disagree;
        // init_kernel: one thread per point
        float* ip = (float*)malloc(P * 3 * 4); float* in = (float*)malloc(P * 3 * 4);
        float* mats = (float*)malloc((size_t)12 * J * 4);
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < 12 * J; ++i) mats[i] = jnt[((size_t)b * J + i / 12) * 16 + i % 12];
            for (int n = 0; n < N; ++n) {
                const size_t i = (size_t)b * N + n;
                init_point(J, weights + i * J, mats, xt + 3 * i, normals + 3 * i, ip + 3 * i, in + 3 * i);
            }
        }
        bad += compare("init points", ip, want_ip, P * 3);
        bad += compare("init normals", in, want_in, P * 3);
        printf("case %d: %d x %d x %d x %d, B %d, N %d, iterations %d: lanes that disagree %lld, bad %lld\n", cs, X, Y, Z, J, B, N, iterations, disagree, bad);
        total_bad += bad;
        free(dims); free(lam); free(bounds); free(spacing); free(vol); free(jnt); free(xt); free(xc_init); free(active); free(weights); free(normals);
        free(want_grad); free(want_xc); free(want_ip); free(want_in); free(grad); free(out); free(ip); free(in); free(mats);
    }
    free(zero);
    fclose(fh);
    printf("TOTAL bad %lld\n", total_bad);
    return total_bad != 0;
}
