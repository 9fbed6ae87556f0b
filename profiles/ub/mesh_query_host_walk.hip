// Host walk of the closest-point kernels (csrc/ag_mesh_query.hip): the face record, the pair test, the winner's detail pass and the
// pseudonormal sign are host-callable functions, so this program runs them query by query over the CPU test shapes and compares
// every output BIT FOR BIT with the float32 run of tests/mesh_query_oracle.py.  Faces are walked backwards, the oracle scans them
// forwards: the tie rule makes the order immaterial.  Arrays are malloc'ed at their exact sizes, so a host sanitizer sees every
// index the kernels form; it needs no GPU:
//   python tests/mesh_query_oracle.py /tmp/mesh_query_cases.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Ianimatablegaussians_amd/csrc profiles/ub/mesh_query_host_walk.hip -o profiles/ub/mesh_query_host_walk
//   profiles/ub/mesh_query_host_walk /tmp/mesh_query_cases.bin
// Prints one line per case and "TOTAL bad 0"; exit status 1 on any mismatch.
#define AG_MESH_QUERY_HOST_ONLY
#include "../../animatablegaussians_amd/csrc/ag_mesh_query.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ag::meshq;

template <typename T>
static T* read_array(FILE* fh, size_t n)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (fread(p, sizeof(T), n, fh) != n) { fprintf(stderr, "truncated case file\n"); exit(2); }
    return p;
}

static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a == 0.f && b == 0.f); }     // +0 and -0 are one value

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, fh) != 1) return 2;
    long long total_bad = 0;
    for (int c = 0; c < n_cases; ++c) {
        int32_t* dims = read_array<int32_t>(fh, 3);
        const int V = dims[0], F = dims[1], N = dims[2];
        float* v = read_array<float>(fh, 3 * (size_t)V);
        int32_t* f = read_array<int32_t>(fh, 3 * (size_t)F);
        float* p = read_array<float>(fh, 3 * (size_t)N);
        float* fn = read_array<float>(fh, 3 * (size_t)F);
        float* en = read_array<float>(fh, 9 * (size_t)F);
        float* vn = read_array<float>(fh, 3 * (size_t)V);
        float* want_d2 = read_array<float>(fh, N);
        int32_t* want_face = read_array<int32_t>(fh, N);
        float* want_bary = read_array<float>(fh, 3 * (size_t)N);
        int32_t* want_feat = read_array<int32_t>(fh, N);
        float* want_sign = read_array<float>(fh, N);
        FaceRec* recs = (FaceRec*)malloc(F ? F * sizeof(FaceRec) : 1);
        for (int i = 0; i < F; ++i) recs[i] = face_record(v, f, V, i);
        float* d2 = (float*)malloc(N * sizeof(float));
        int32_t* face = (int32_t*)malloc(N * sizeof(int32_t));
        float* bary = (float*)malloc(3 * (size_t)N * sizeof(float));
        int32_t* feat = (int32_t*)malloc(N * sizeof(int32_t));
        Query a;
        a.N = N; a.V = V; a.F = F; a.gx = a.gy = a.gz = 0;
        a.points = p; a.axis_x = a.axis_y = a.axis_z = nullptr;
        long long bad = 0;
        for (int n = 0; n < N; ++n) {
            float qx, qy, qz;
            load_query(a, n, qx, qy, qz);
            float best = INFINITY;
            int best_f = -1;
            for (int i = F - 1; i >= 0; --i) {
                const float d = pair_dist2(recs[i], qx, qy, qz);
                if (wins(d, i, best, best_f)) { best = d; best_f = i; }
            }
            store_result(recs, n, qx, qy, qz, best_f, d2, face, bary, feat);
            const float sg = pseudonormal_sign(a, n, v, f, face, bary, feat, fn, en, vn);
            const bool ok = same(d2[n], want_d2[n]) && same(d2[n], best) && face[n] == want_face[n] && same(bary[3 * n], want_bary[3 * n])
                            && same(bary[3 * n + 1], want_bary[3 * n + 1]) && same(bary[3 * n + 2], want_bary[3 * n + 2])
                            && feat[n] == want_feat[n] && same(sg, want_sign[n]);
            if (!ok) {
                if (bad < 5) printf("  query %d: d2 %.9g/%.9g face %d/%d bary %.9g %.9g %.9g / %.9g %.9g %.9g feature %d/%d sign %g/%g\n", n, d2[n],
                                    want_d2[n], face[n], want_face[n], bary[3 * n], bary[3 * n + 1], bary[3 * n + 2], want_bary[3 * n],
                                    want_bary[3 * n + 1], want_bary[3 * n + 2], feat[n], want_feat[n], sg, want_sign[n]);
                ++bad;
            }
        }
        // grid mode: the node decode of a 2 x 3 x 4 grid whose axes are cut from the first coordinates
        if (N >= 9) {
            Query g = a;
            g.points = nullptr; g.gx = 2; g.gy = 3; g.gz = 4; g.N = 24;
            float ax[2] = {p[0], p[3]}, ay[3] = {p[1], p[4], p[7]}, az[4] = {p[2], p[5], p[8], p[11]};
            g.axis_x = ax; g.axis_y = ay; g.axis_z = az;
            for (int n = 0; n < 24; ++n) {
                float qx, qy, qz;
                load_query(g, n, qx, qy, qz);
                if (qx != ax[n / 12] || qy != ay[(n / 4) % 3] || qz != az[n % 4]) ++bad;
            }
        }
        printf("case %d: V %d F %d N %d bad %lld\n", c, V, F, N, bad);
        total_bad += bad;
        free(dims); free(v); free(f); free(p); free(fn); free(en); free(vn); free(want_d2); free(want_face); free(want_bary); free(want_feat);
        free(want_sign); free(recs); free(d2); free(face); free(bary); free(feat);
    }
    fclose(fh);
    printf("TOTAL bad %lld\n", total_bad);
    return total_bad != 0;
}
