// fe_fragments.h - host side of the weight buffers: the operand order of the 16x16x4 fp32 MFMA, written once (plain C++17, no HIP).
//
// A matrix operand is cut into tiles of 16 rows (A operand; columns of a B operand) and k-steps of 4: one k-step of one tile is
// the 64 floats a wavefront feeds to one v_mfma_f32_16x16x4_f32, lane by lane:
//
//     lane  <->  (r = lane % 16, k = 4 * ks + lane / 16)        r: row / column within the tile, k: index along the product's K
//
// and a matrix of NT tiles x KS k-steps is stored in one of two orders:
//
//     plain   dst[(tile * KS + ks) * 64 + lane]                              one 4-byte fetch per lane and k-step
//     k4      dst[((tile * (KS / 4) + ks / 4) * 64 + lane) * 4 + ks % 4]     four k-steps per lane side by side: 16-byte fetches
//
// What r and k MEAN (gate order and pre-scaling, channel groups, taps, permuted features) is each packer's business: it hands a
// function f(tile, r, k) to Buffer::tiles.  Everything that writes or reorders fragments goes through this file.
#pragma once

#include <cstddef>
#include <vector>

namespace fe {
namespace frag {

enum Order { kPlain, kK4 };

constexpr size_t plain_index(int tile, int KS, int ks, int lane) { return ((size_t)tile * KS + ks) * 64 + lane; }
constexpr size_t k4_index(int tile, int KS, int ks, int lane) { return (((size_t)tile * (KS / 4) + ks / 4) * 64 + lane) * 4 + ks % 4; }
constexpr int lane_r(int lane) { return lane % 16; }
constexpr int lane_k(int ks, int lane) { return 4 * ks + lane / 16; }

// The packed buffer.  Fixed size with offsets known at compile time (Buffer(total)), or growing (alloc); zero-filled either way.
// Every access is v[...]: a build with -D_GLIBCXX_ASSERTIONS bounds-checks all of the packing.
struct Buffer {
    std::vector<float> v;
    explicit Buffer(size_t floats = 0) : v(floats, 0.0f) {}
    float& operator[](size_t i) { return v[i]; }
    size_t size() const { return v.size(); }
    // n more zeros, starting at a multiple of 64 floats: returns where
    int alloc(size_t n) {
        const size_t off = (v.size() + 63) & ~(size_t)63;
        v.resize(off + n, 0.0f);
        return (int)off;
    }
    void raw(size_t off, size_t n, const float* src) {
        for (size_t i = 0; i < n; ++i) v[off + i] = src[i];
    }
    void rep4(size_t off, size_t n, const float* src) {   // [n][4]: each value four times (16-byte accumulator initialisers)
        for (size_t i = 0; i < n; ++i)
            for (int r = 0; r < 4; ++r) v[off + 4 * i + r] = src[i];
    }
    // NT tiles x KS k-steps of f(tile, r, k) at off (k4: KS % 4 == 0)
    template <Order O = kPlain, class F>
    void tiles(size_t off, int NT, int KS, F&& f) {
        for (int t = 0; t < NT; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    v[off + (O == kK4 ? k4_index(t, KS, ks, lane) : plain_index(t, KS, ks, lane))] = f(t, lane_r(lane), lane_k(ks, lane));
    }
    // A operand of A(m, k), Mrows x K: rows = r, zero beyond Mrows
    template <Order O = kPlain, class F>
    void pack_a(size_t off, int Mrows, int K, F&& Amk) {
        tiles<O>(off, (Mrows + 15) / 16, K / 4, [&](int t, int r, int k) { return 16 * t + r < Mrows ? Amk(16 * t + r, k) : 0.0f; });
    }
    // B operand of B(k, n), K x Ncols: columns = r, zero beyond Ncols
    template <Order O = kPlain, class F>
    void pack_b(size_t off, int K, int Ncols, F&& Bkn) {
        tiles<O>(off, (Ncols + 15) / 16, K / 4, [&](int t, int r, int k) { return 16 * t + r < Ncols ? Bkn(k, 16 * t + r) : 0.0f; });
    }
    // per-row values [tile][16] of f(tile, r): the tiles' start values / biases (a lane of the accumulator reads rows 4 (lane / 16) .. + 3)
    template <class F>
    void rows(size_t off, int NT, F&& f) {
        for (int t = 0; t < NT; ++t)
            for (int r = 0; r < 16; ++r) v[off + (size_t)t * 16 + r] = f(t, r);
    }
    // plain -> k4: the k-steps [k0, k0 + nk) of ntiles plain tiles of KS k-steps at src, written as tiles of nk k-steps at dst (the two
    // ranges apart); dst tile t is src tile src_tile(t).  The k-steps beyond the last full group of four keep their plain place, so with
    // k0 = 0, nk = KS a tile stays where it is in a copy of its region and only its full groups change order.
    template <class TileMap>
    void regroup_k4(size_t dst, size_t src, int ntiles, int KS, int k0, int nk, TileMap&& src_tile) {
        for (int t = 0; t < ntiles; ++t)
            for (int ks = 0; ks < nk; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    v[dst + (size_t)t * nk * 64 + (ks < nk / 4 * 4 ? k4_index(0, nk, ks, lane) : plain_index(0, nk, ks, lane))] =
                        v[src + plain_index(src_tile(t), KS, k0 + ks, lane)];
    }
    void regroup_k4(size_t dst, size_t src, int ntiles, int KS, int k0, int nk) { regroup_k4(dst, src, ntiles, KS, k0, nk, [](int t) { return t; }); }
};

}  // namespace frag
}  // namespace fe
