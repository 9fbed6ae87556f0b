// Host walk of the iso-surface kernels (csrc/ag_isosurface.hip): what one thread does is a host-callable function there, so this
// program runs every thread of classify_kernel, edge_kernel, vertex_kernel and face_kernel on the CPU and compares vertices and faces
// BIT FOR BIT with the float32 run of tests/isosurface_oracle.py.  The scans are the one step that cannot be walked as written (wave
// shuffles); they only add integers, whose order cannot change the result, and are restated here as one serial exclusive scan with the
// total in the extra last item, which is what the kernels leave.  Arrays are malloc'ed at the sizes of the workspace layout, so a host
// sanitizer sees every index the kernels form; it needs no GPU:
//   python tests/isosurface_oracle.py /tmp/isosurface_cases.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Ianimatablegaussians_amd/csrc profiles/ub/isosurface_host_walk.hip -o profiles/ub/isosurface_host_walk
//   profiles/ub/isosurface_host_walk /tmp/isosurface_cases.bin
// Prints one line per case and "TOTAL bad 0"; exit status 1 on any mismatch.
#define AG_ISOSURFACE_HOST_ONLY
#include "../../animatablegaussians_amd/csrc/ag_isosurface.hip"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ag::iso;

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

static void exclusive_scan(uint32_t* data, size_t len)
{
    uint32_t run = 0;
    for (size_t i = 0; i < len; ++i) { const uint32_t v = data[i]; data[i] = run; run += v; }
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
        int32_t* dims = read_array<int32_t>(fh, 6);
        const int X = dims[0], Y = dims[1], Z = dims[2], has_mask = dims[3], want_V = dims[4], want_F = dims[5];
        float* par = read_array<float>(fh, 7);
        Grid g = {};
        if (check_sizes("walk", X, Y, Z, g) || check_iso("walk", par[0], g) || check_placement("walk", par + 1, par + 4, g)) return 2;
        const size_t N = (size_t)g.N;
        float* vol = read_array<float>(fh, N);
        uint8_t* mask = has_mask ? read_array<uint8_t>(fh, N) : nullptr;
        float* want_v = read_array<float>(fh, (size_t)want_V * 3);
        int32_t* want_f = read_array<int32_t>(fh, (size_t)want_F * 3);
        uint8_t* cases = (uint8_t*)malloc(N);
        uint32_t* escan = (uint32_t*)malloc((3 * N + 1) * 4);
        uint32_t* tscan = (uint32_t*)malloc((N + 1) * 4);
        for (size_t n = 0; n < N; ++n) classify_node(g, vol, mask, (long long)n, cases, tscan);
        tscan[N] = 0;
        for (size_t n = 0; n < N; ++n) flag_node(g, vol, cases, (long long)n, escan);
        escan[3 * N] = 0;
        exclusive_scan(escan, 3 * N + 1);
        exclusive_scan(tscan, N + 1);
        const long long V = escan[3 * N], F = tscan[N];
        long long bad = (V != want_V) + (F != want_F);
        if (!bad) {
            float* v = (float*)malloc(V ? (size_t)V * 12 : 1);
            int32_t* f = (int32_t*)malloc(F ? (size_t)F * 12 : 1);
            memset(v, 0xff, (size_t)V * 12);
            memset(f, 0xff, (size_t)F * 12);
            for (size_t n = 0; n < N; ++n) emit_node(g, vol, escan, (long long)n, v);
            for (size_t n = 0; n < N; ++n) emit_cell(g, cases, escan, tscan, (long long)n, f);
            for (long long i = 0; i < 3 * V; ++i)
                if (memcmp(v + i, want_v + i, 4) != 0 && !(v[i] == 0.f && want_v[i] == 0.f)) { if (bad < 5) printf("  vertex element %lld: %.9g / %.9g\n", i, v[i], want_v[i]); ++bad; }
            for (long long i = 0; i < 3 * F; ++i)
                if (f[i] != want_f[i]) { if (bad < 5) printf("  face element %lld: %d / %d\n", i, f[i], want_f[i]); ++bad; }
            free(v); free(f);
        }
        printf("case %d: %d x %d x %d%s, iso %g: V %lld / %d, F %lld / %d, bad %lld\n", cs, X, Y, Z, has_mask ? " masked" : "", (double)par[0], V, want_V, F, want_F, bad);
        total_bad += bad;
        free(dims); free(par); free(vol); free(mask); free(want_v); free(want_f); free(cases); free(escan); free(tscan);
    }
    fclose(fh);
    printf("TOTAL bad %lld\n", total_bad);
    return total_bad != 0;
}
