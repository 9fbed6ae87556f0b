// Host walk of the training-target kernel (csrc/ag_targets.hip): its phases are host-callable functions of the thread index, so this
// program runs them thread by thread, workgroup by workgroup, over malloc'ed planes at every pointer alignment and compares with a
// brute-force window (uint8 subtraction kept) and the float64 division.  Meant for a host sanitizer, which sees every index the
// kernel forms; it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Ianimatablegaussians_amd/csrc \
//         profiles/ub/targets_host_walk.hip -o profiles/ub/targets_host_walk && profiles/ub/targets_host_walk
// Prints one line per case and "TOTAL bad 0"; exit status 1 on any mismatch or changed guard byte.
#define AG_TARGETS_HOST_ONLY
#include "../../animatablegaussians_amd/csrc/ag_targets.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cmath>
using namespace ag::targets;

template <int R>
static void run_block(const Args& a, int bx, int by, int v, int gx, int gy)
{
    std::vector<uint32_t> cls(kClsWords, 0xdeadbeef), hor(kHorWords, 0xdeadbeef), res(kResWords, 0xdeadbeef), col(kTW / 4, 0);
    const int Y0 = by * kTH, X0 = bx * kTW;
    const long long block = ((long long)v * gy + by) * gx + bx;
    for (int tid = 0; tid < kThreads; ++tid) convert_colour(a, tid, block);
    for (int tid = 0; tid < kThreads; ++tid) load_flags<R>(a, tid, v, Y0, X0, cls.data());
    for (int tid = 0; tid < kThreads; ++tid) row_pass<R>(tid, cls.data(), hor.data());
    for (int tid = 0; tid < kThreads; ++tid) {
        const int t = tid & 31, ty = tid / 32;
        for (int half = 0; half < 2; ++half) {
            const int oy = ty + 8 * half;
            uint32_t m = column_pass<R>(oy, t, cls.data(), hor.data(), res.data());
            col[t] |= m;
            if (a.row_any && m) a.row_any[(long long)v * a.H + Y0 + oy] = 1;
        }
    }
    if (a.col_any)
        for (int tid = 0; tid < 32; ++tid)
            for (int k = 0; k < 4; ++k)
                if ((col[tid] >> (8 * k)) & 1u) a.col_any[(long long)v * a.W + X0 + 4 * tid + k] = 1;
    for (int tid = 0; tid < kThreads; ++tid) store_plane(a, tid, v, Y0, X0, res.data(), a.mask, 0);
    for (int tid = 0; tid < kThreads; ++tid) store_plane(a, tid, v, Y0, X0, res.data(), a.boundary, 1);
}

static int cls_of(int m) { return m < 128 ? 0 : m > 128 ? 1 : 128; }

static long long run_case(int V, int H, int W, int R, int o_col, int o_mat, int o_cf, int o_mask, int o_bnd, unsigned seed)
{
    const long long n = (long long)V * H * W;
    srand(seed);
    static const int vals[10] = {0, 3, 5, 6, 127, 128, 129, 249, 250, 255};
    static const int cum[10] = {30, 32, 34, 36, 38, 43, 45, 47, 49, 100};
    auto mk = [](size_t off, size_t bytes) { uint8_t* p = (uint8_t*)malloc(off + bytes); memset(p, 0xA5, off + bytes); return p; };
    uint8_t* bcol = mk(o_col, n * 3); uint8_t* bmat = mk(o_mat, n);
    uint8_t* bcf = mk(o_cf * 4, n * 12); uint8_t* bmask = mk(o_mask, n); uint8_t* bbnd = mk(o_bnd, n);
    uint8_t* row = mk(0, (size_t)V * H); uint8_t* colp = mk(0, (size_t)V * W);
    memset(row, 0, (size_t)V * H); memset(colp, 0, (size_t)V * W);
    // a block structure so that classes form regions as well as noise
    for (long long i = 0; i < n; ++i) {
        int r = rand() % 100, k = 0; while (cum[k] <= r) ++k;
        long long x = i % W, y = (i / W) % H;
        int base = (((x / 9) + (y / 7)) & 1) ? 255 : 0;
        bmat[o_mat + i] = (rand() % 4 == 0) ? vals[k] : base;
    }
    for (long long i = 0; i < 3 * n; ++i) bcol[o_col + i] = (uint8_t)(rand() & 255);
    Args a;
    a.color = bcol + o_col; a.matte = bmat + o_mat; a.color_f = (float*)(bcf) + o_cf; a.mask = bmask + o_mask; a.boundary = bbnd + o_bnd;
    a.row_any = row; a.col_any = colp; a.V = V; a.H = H; a.W = W; a.n_matte = n; a.n_color = 3 * n;
    a.color_shift = (int)(((uintptr_t)a.color_f >> 2) & 3u);
    a.groups = (a.n_color + a.color_shift + 3) / 4;
    const int gx = (W + kTW - 1) / kTW, gy = (H + kTH - 1) / kTH;
    a.per_block = (a.groups + (long long)gx * gy * V - 1) / ((long long)gx * gy * V);
    for (int v = 0; v < V; ++v) for (int by = 0; by < gy; ++by) for (int bx = 0; bx < gx; ++bx) {
        switch (R) {
            case 0: run_block<0>(a, bx, by, v, gx, gy); break; case 1: run_block<1>(a, bx, by, v, gx, gy); break;
            case 2: run_block<2>(a, bx, by, v, gx, gy); break; case 3: run_block<3>(a, bx, by, v, gx, gy); break;
            case 4: run_block<4>(a, bx, by, v, gx, gy); break; case 5: run_block<5>(a, bx, by, v, gx, gy); break;
            case 6: run_block<6>(a, bx, by, v, gx, gy); break; default: run_block<7>(a, bx, by, v, gx, gy); break;
        }
    }
    long long bad = 0, nb = 0, nm = 0;
    for (int v = 0; v < V; ++v) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const long long i = ((long long)v * H + y) * W + x;
        int m = a.matte[i], emin = 255, emax = 0;
        for (int dy = -R; dy <= R; ++dy) for (int dx = -R; dx <= R; ++dx) {
            int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            int c = cls_of(a.matte[((long long)v * H + yy) * W + xx]);
            emin = c < emin ? c : emin; emax = c > emax ? c : emax;
        }
        int b = ((uint8_t)(emax - emin) == 1) || (m > 5 && m < 250);
        int mk_ = cls_of(m) == 1;
        nb += b; nm += mk_;
        if (a.mask[i] != mk_ || a.boundary[i] != b) { if (bad < 5) printf("  mismatch v%d y%d x%d: mask %d/%d band %d/%d\n", v, y, x, a.mask[i], mk_, a.boundary[i], b); ++bad; }
    }
    for (long long i = 0; i < 3 * n; ++i) {
        float want = (float)((double)a.color[i] / 255.);
        if (memcmp(&want, &a.color_f[i], 4)) { if (bad < 5) printf("  colour mismatch at %lld\n", i); ++bad; }
    }
    for (int v = 0; v < V; ++v) {
        for (int y = 0; y < H; ++y) { int any = 0; for (int x = 0; x < W; ++x) any |= a.mask[((long long)v * H + y) * W + x]; if (any != row[v * H + y]) ++bad; }
        for (int x = 0; x < W; ++x) { int any = 0; for (int y = 0; y < H; ++y) any |= a.mask[((long long)v * H + y) * W + x]; if (any != colp[v * W + x]) ++bad; }
    }
    auto guard = [&](uint8_t* p, int off) { for (int i = 0; i < off; ++i) if (p[i] != 0xA5) ++bad; };
    guard(bcf, o_cf * 4); guard(bmask, o_mask); guard(bbnd, o_bnd);
    printf("V%d %dx%d R%d offs %d %d %d %d %d: band %.1f%% mask %.1f%% bad %lld\n", V, H, W, R, o_col, o_mat, o_cf, o_mask, o_bnd, 100. * nb / n, 100. * nm / n, bad);
    free(bcol); free(bmat); free(bcf); free(bmask); free(bbnd); free(row); free(colp);
    return bad;
}

int main()
{
    long long bad = 0;
    const int shapes[][2] = {{1, 3}, {4, 4}, {5, 7}, {37, 70}, {19, 131}, {70, 203}, {9, 9}, {67, 523}, {33, 128}, {16, 257}};
    unsigned seed = 1;
    for (auto& s : shapes)
        for (int R = 0; R <= 7; ++R)
            for (int V = 1; V <= 3; V += 2)
                bad += run_case(V, s[0], s[1], R, (seed * 7) & 3, (seed * 5) & 3, (seed * 3) & 3, seed & 3, (seed >> 2) & 3, seed), ++seed;
    for (int o = 0; o < 4; ++o) for (int p = 0; p < 4; ++p) bad += run_case(2, 19, 131, 2, o, p, (o + p) & 3, p, o, 100 + 4 * o + p);
    printf("TOTAL bad %lld\n", bad);
    return bad != 0;
}
