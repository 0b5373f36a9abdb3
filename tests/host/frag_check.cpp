// frag_check.cpp - stand-alone check of fastenhancer_amd/csrc/fe_fragments.h against the written definition of the two fragment
// orders (tests/test_cpu_pack.py compiles it with the host compiler and -fsanitize=address,undefined, and runs it).
#include <cstdio>
#include <vector>

#include "fe_fragments.h"

using namespace fe::frag;

static int g_bad = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

// a value that names its (row / column, k): no two differ by chance
static float val(int rn, int k) { return (float)(1 + rn * 1000 + k); }

template <class IndexFn>
static void check_bijection(int NT, int KS, IndexFn index) {
    std::vector<int> seen((size_t)NT * KS * 64, 0);
    for (int t = 0; t < NT; ++t)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const size_t i = index(t, KS, ks, lane);
                CHECK(i < seen.size());
                if (i < seen.size()) ++seen[i];
            }
    for (int c : seen) CHECK(c == 1);
}

int main() {
    // both index functions are bijections onto [0, NT * KS * 64)
    check_bijection(3, 9, [](int t, int KS, int ks, int lane) { return plain_index(t, KS, ks, lane); });
    check_bijection(1, 1, [](int t, int KS, int ks, int lane) { return plain_index(t, KS, ks, lane); });
    check_bijection(3, 8, [](int t, int KS, int ks, int lane) { return k4_index(t, KS, ks, lane); });
    check_bijection(2, 4, [](int t, int KS, int ks, int lane) { return k4_index(t, KS, ks, lane); });

    // pack_a / pack_b at K = 36, N = 24 against the definition: dst[(tile * KS + ks) * 64 + lane] holds (r = lane % 16, k = 4 ks + lane / 16);
    // the second tile is half full (zero fill), the ninth k-step is a group of four that is not full
    const int K = 36, N = 24, KS = K / 4, NT = 2;
    {
        Buffer b((size_t)NT * KS * 64 + 7);
        for (size_t i = 0; i < b.size(); ++i) b[i] = -1.0f;
        b.pack_b(7, K, N, [](int k, int n) { return val(n, k); });
        Buffer a((size_t)NT * KS * 64);
        a.pack_a(0, N, K, [](int m, int k) { return val(m, k); });
        Buffer a4((size_t)NT * 8 * 64);
        a4.pack_a<kK4>(0, N, 32, [](int m, int k) { return val(m, k); });
        for (int i = 0; i < 7; ++i) CHECK(b[i] == -1.0f);
        for (int t = 0; t < NT; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = 16 * t + lane % 16, k = 4 * ks + lane / 16;
                    const float want = r < N ? val(r, k) : 0.0f;
                    CHECK(b[7 + ((size_t)t * KS + ks) * 64 + lane] == want);
                    CHECK(a[((size_t)t * KS + ks) * 64 + lane] == want);
                    if (ks < 8) CHECK(a4[(((size_t)t * 2 + ks / 4) * 64 + lane) * 4 + ks % 4] == want);
                }
    }

    // regrouping a copy at KS = 9: the first eight k-steps move to k4 order within their tile, the ninth stays plain where it was
    {
        Buffer b((size_t)2 * NT * KS * 64);
        const size_t copy = (size_t)NT * KS * 64;
        b.pack_b(0, K, N, [](int k, int n) { return val(n, k); });
        for (size_t i = 0; i < copy; ++i) b[copy + i] = b[i];
        b.regroup_k4(copy, 0, NT, KS, 0, KS);
        for (int t = 0; t < NT; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const float want = b[((size_t)t * KS + ks) * 64 + lane];
                    const size_t tile = copy + (size_t)t * KS * 64;
                    if (ks < 8) CHECK(b[tile + (size_t)(ks / 4) * 256 + lane * 4 + ks % 4] == want);
                    else CHECK(b[tile + (size_t)ks * 64 + lane] == want);
                }
    }

    // the sub-range form into a fresh allocation: k-steps [k0, k0 + nk) of tiles [tile][kst][64] as [tile][nk / 4][lane][4], tiles permuted
    {
        const int ntiles = 3, kst = 12, k0 = 4, nk = 8;
        Buffer b;
        const int src = b.alloc((size_t)ntiles * kst * 64 + 5);
        for (int i = 0; i < ntiles * kst * 64; ++i) b[src + i] = (float)(i + 1);
        const int dst = b.alloc((size_t)ntiles * nk * 64), perm = b.alloc((size_t)ntiles * nk * 64);
        CHECK(dst % 64 == 0 && perm % 64 == 0 && dst >= src + ntiles * kst * 64 + 5);
        b.regroup_k4(dst, src, ntiles, kst, k0, nk);
        b.regroup_k4(perm, src, ntiles, kst, k0, nk, [](int t) { return (t + 1) % 3; });
        for (int t = 0; t < ntiles; ++t)
            for (int q = 0; q < nk / 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const size_t at = (((size_t)t * (nk / 4) + q) * 64 + lane) * 4 + j;
                        CHECK(b[dst + at] == b[src + ((size_t)t * kst + k0 + 4 * q + j) * 64 + lane]);
                        CHECK(b[perm + at] == b[src + ((size_t)((t + 1) % 3) * kst + k0 + 4 * q + j) * 64 + lane]);
                    }
    }

    // alloc: multiples of 64, zero-filled, earlier contents kept; the per-row tables and rep4
    {
        Buffer b;
        const int a0 = b.alloc(3), a1 = b.alloc(70), a2 = b.alloc(0), a3 = b.alloc(64);
        CHECK(a0 == 0 && a1 == 64 && a2 == 192 && a3 == 192 && b.size() == 256);
        for (size_t i = 0; i < b.size(); ++i) CHECK(b[i] == 0.0f);
        b.rows(a1, 2, [](int t, int r) { return val(t, r); });
        for (int t = 0; t < 2; ++t)
            for (int r = 0; r < 16; ++r) CHECK(b[a1 + t * 16 + r] == val(t, r));
        const float s[3] = {1.5f, -2.0f, 4.0f};
        b.rep4(a3, 3, s);
        for (int i = 0; i < 12; ++i) CHECK(b[a3 + i] == s[i / 4]);
        CHECK(b[a3 + 12] == 0.0f && b[a1 + 32] == 0.0f);
        const int a4 = b.alloc(1);
        CHECK(a4 == 256 && b[a1] == val(0, 0) && b[a4] == 0.0f);
    }

    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("frag_check: ok\n");
    return 0;
}
