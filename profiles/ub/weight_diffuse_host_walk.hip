// Host walk of the diffusion kernels (csrc/ag_weight_diffuse.hip): what one thread of one workgroup does is a host-callable function
// there, so this program runs every (workgroup, thread) of every launch of ag_weight_diffuse_apply / _init / _iterate on the CPU, with
// the launch plan of the library itself (make_plan), the workgroup sums through a 256-float array and the finishing wave's fold
// written out.  It compares the operator BIT FOR BIT with the float32 run of tests/weight_diffuse_oracle.py and the solve with the
// oracle's direct solution.  Arrays are malloc'ed at their exact sizes, so a host sanitizer sees every index the kernels form; it
// needs no GPU:
//   python tests/weight_diffuse_oracle.py /tmp/weight_diffuse_cases.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Ianimatablegaussians_amd/csrc profiles/ub/weight_diffuse_host_walk.hip -o profiles/ub/weight_diffuse_host_walk
//   profiles/ub/weight_diffuse_host_walk /tmp/weight_diffuse_cases.bin
// Prints one line per case and "TOTAL bad 0"; exit status 1 on any mismatch.
#define AG_WEIGHT_DIFFUSE_HOST_ONLY
#include "../../animatablegaussians_amd/csrc/ag_weight_diffuse.hip"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ag::wdiff;

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

static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a == 0.f && b == 0.f); }     // +0 and -0 are one value

// one launch: f(block, tid, c0) -> the thread's share of the sum; SUM: the workgroup's partial sums as block_sum forms them
template <bool SUM, typename F>
static void launch(const DiffArgs& a, int blocks, float* partial, F f)
{
    float s_part[kThreads];
    for (int b = 0; b < blocks; ++b)
        for (int c0 = 0; c0 < a.C; c0 += 64) {
            for (int tid = 0; tid < kThreads; ++tid) s_part[tid] = f((unsigned)b, tid, c0);
            if (SUM)
                for (int t = 0; t < kThreads; ++t)
                    if (t < a.CP && c0 + t < a.C) partial[(long long)b * a.C + c0 + t] = block_sum_thread(a, s_part, t);
        }
}

static void finish(int mode, const float* partial, int nb, int C, float* rr, float* bb, float* alpha, float* beta)
{
    for (int c = 0; c < C; ++c) {
        float s[64];
        for (int l = 0; l < 64; ++l) s[l] = finish_lane_sum(partial, nb, C, c, l);
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) s[l] = s[l] + s[l + o];          // what lane 0 ends with after the shuffles
        finish_write(mode, s[0], c, rr, bb, alpha, beta);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, fh) != 1) return 2;
    long long total_bad = 0;
    for (int cs = 0; cs < n_cases; ++cs) {
        int32_t* dims = read_array<int32_t>(fh, 5);
        const int X = dims[0], Y = dims[1], Z = dims[2], C = dims[3], want_iterations = dims[4];
        const size_t N = (size_t)X * Y * Z, E = N * C;
        float* w = read_array<float>(fh, 3);
        uint8_t* fixed = read_array<uint8_t>(fh, N);
        float* target = read_array<float>(fh, E);
        float* probe = read_array<float>(fh, E);
        float* want_apply = read_array<float>(fh, E);
        double* direct = read_array<double>(fh, E);
        Plan pl;
        if (make_plan("host walk", X, Y, Z, C, w, pl)) return 2;
        const DiffArgs a = pl.a;
        float* x = (float*)malloc(E * 4); float* r = (float*)malloc(E * 4); float* p = (float*)malloc(E * 4); float* ap = (float*)malloc(E * 4);
        const size_t n_partial = (size_t)(pl.stencil_blocks > pl.vector_blocks ? pl.stencil_blocks : pl.vector_blocks) * C;
        float* partial = (float*)malloc(n_partial * 4);
        float* rr = (float*)malloc(C * 4); float* bb = (float*)malloc(C * 4); float* alpha = (float*)malloc(C * 4); float* beta = (float*)malloc(C * 4);
        long long bad = 0;
        // ag_weight_diffuse_apply on the probe
        memset(ap, 0xff, E * 4);
        launch<false>(a, pl.stencil_blocks, partial, [&](unsigned b, int tid, int c0) {
            return stencil_thread<false>(a, pl.stencil_items, b, pl.stencil_blocks, tid, c0, probe, fixed, ap); });
        for (size_t e = 0; e < E; ++e)
            if (!same(ap[e], want_apply[e])) { if (bad < 5) printf("  apply element %zu: %.9g / %.9g\n", e, ap[e], want_apply[e]); ++bad; }
        // the same with 2 workgroups, so that every wave strides over several runs
        memset(ap, 0xff, E * 4);
        launch<false>(a, 2, partial, [&](unsigned b, int tid, int c0) { return stencil_thread<false>(a, pl.stencil_items, b, 2, tid, c0, probe, fixed, ap); });
        for (size_t e = 0; e < E; ++e)
            if (!same(ap[e], want_apply[e])) ++bad;
        // ag_weight_diffuse_init
        memset(x, 0xff, E * 4); memset(r, 0xff, E * 4); memset(p, 0xff, E * 4); memset(ap, 0xff, E * 4);
        launch<false>(a, pl.vector_blocks, partial, [&](unsigned b, int tid, int c0) {
            return vector_thread<M_MASK>(a, pl.vector_items, b, pl.vector_blocks, tid, c0, target, fixed, x, r, p, nullptr, nullptr); });
        launch<false>(a, pl.stencil_blocks, partial, [&](unsigned b, int tid, int c0) {
            return stencil_thread<false>(a, pl.stencil_items, b, pl.stencil_blocks, tid, c0, x, fixed, ap); });
        launch<true>(a, pl.vector_blocks, partial, [&](unsigned b, int tid, int c0) {
            return vector_thread<M_INIT>(a, pl.vector_items, b, pl.vector_blocks, tid, c0, nullptr, fixed, x, r, p, ap, nullptr); });
        finish(F_INIT, partial, pl.vector_blocks, C, rr, bb, alpha, beta);
        // ag_weight_diffuse_iterate, one iteration at a time, to the tolerance of the tests
        int it = 0;
        for (; it < 4000; ++it) {
            bool done = true;
            for (int c = 0; c < C; ++c) done = done && (double)rr[c] <= 1e-10 * (double)bb[c];
            if (done) break;
            launch<true>(a, pl.stencil_blocks, partial, [&](unsigned b, int tid, int c0) {
                return stencil_thread<true>(a, pl.stencil_items, b, pl.stencil_blocks, tid, c0, p, fixed, ap); });
            finish(F_ALPHA, partial, pl.stencil_blocks, C, rr, nullptr, alpha, beta);
            launch<true>(a, pl.vector_blocks, partial, [&](unsigned b, int tid, int c0) {
                return vector_thread<M_XR>(a, pl.vector_items, b, pl.vector_blocks, tid, c0, nullptr, fixed, x, r, p, ap, alpha); });
            finish(F_BETA, partial, pl.vector_blocks, C, rr, nullptr, alpha, beta);
            launch<false>(a, pl.vector_blocks, partial, [&](unsigned b, int tid, int c0) {
                return vector_thread<M_P>(a, pl.vector_items, b, pl.vector_blocks, tid, c0, nullptr, fixed, x, r, p, nullptr, beta); });
        }
        double worst = 0;
        for (size_t n = 0; n < N; ++n)
            for (int c = 0; c < C; ++c) {
                const size_t e = n * C + c;
                if (fixed[n] && !(x[e] == 0.f && r[e] == 0.f && p[e] == 0.f)) ++bad;            // the invariant of the header
                const double u = fixed[n] ? (double)target[e] : (double)x[e];
                const double d = std::fabs(u - direct[e]);
                if (!(d <= worst)) worst = d;
            }
        if (!(worst <= 1e-4) || it > want_iterations + want_iterations / 2) ++bad;
        printf("case %d: %d x %d x %d x %d, blocks %d / %d, iterations %d (float64 oracle %d), worst |u - direct| %.3e, bad %lld\n", cs, X, Y, Z, C,
               pl.stencil_blocks, pl.vector_blocks, it, want_iterations, worst, bad);
        total_bad += bad;
        free(dims); free(w); free(fixed); free(target); free(probe); free(want_apply); free(direct); free(x); free(r); free(p); free(ap); free(partial);
        free(rr); free(bb); free(alpha); free(beta);
    }
    fclose(fh);
    printf("TOTAL bad %lld\n", total_bad);
    return total_bad != 0;
}
