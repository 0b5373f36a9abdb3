// resample_kernels.hip.h — polyphase resampling sr_in -> sr_out (fe_resample / fe_resample_streams / fe_resample_rings of the C ABI): one
// template, three forms.
//
// The contract ("Audio at another sample rate"): up = sr_out / g, down = sr_in / g, R = max(up, down), hl = 10 R, L = 2 hl + 1
// taps h = up * firwin(L, 1 / R, kaiser 5.0), K = ceil(L / up) taps per output.  Output m:  c = m down + hl, kmax = c div up, r = c mod up,
//   y[m] = sum over j = 0 .. K - 1 with r + j up <= 2 hl of h[r + j up] x[kmax - j],     x = 0 outside the signal,
// accumulated in fp32 from +0, j ascending, one fused multiply-add per tap - the same sequence of operations for an output whichever form,
// tile or packetisation computes it, so a stream's outputs are the bits of the whole-signal call's.
//
// A workgroup of 256 threads keeps in LDS: the phase-major tap table T[r][j] = h[r + j up] (row stride KP = K | 1: the lanes of a wave read
// one j of different rows r, and an odd stride spreads rows over the 32 banks of a 4-byte read; up = 1 is one row, read as a broadcast), one
// tile of input as floats (the tile's oldest tap to its newest sample: xcap floats) and the tile's outputs (tile_out floats).  One thread per
// output of the tile.  The host chooses tile_out so that a tile advances at most 4096 input samples (fe_api_resample.inc).
//
// !STRM (whole signals): grid (tiles, B), rows addressed by strides, no state.
// STRM (packet streams): one workgroup per call stream walks the stream's tiles, so the LDS footprint does not depend on n_in_max.  The
// descriptor is read wave-uniformly (as fe_kernels.hip.h::stream_view reads fe_stream_desc) and checked before anything is read or
// written; samples before the packet come from the slot's history; the new history and count are written after a barrier behind the last tile.
// No atomics, no waiting on other workgroups, no cooperative launch.
// RING (packet streams whose samples live in rings; implies STRM): the STRM form with another descriptor and other addresses, nothing else -
// sample i of the packet is element in_base + (in_pos + i) mod in_len of a.in, output m of the call element out_base + (out_pos + m) mod
// out_len of a.out.  A tile's outputs go out as at most two contiguous segments (the split is wave-uniform), each through
// stream_store_row; the history update reads the packet's last K - 1 samples through the ring index, since they may straddle the wrap.
// G711 (any form): the instantiations the host launches where either format of the call is a G.711 law (FE_AUDIO_ULAW / FE_AUDIO_ALAW, one
// byte per sample).  They load and store through helpers of this file that dispatch over all four formats; the instantiations without it
// keep stream_sample / stream_store_row, their argument blocks and their code.
#pragma once
#include <hip/hip_runtime.h>

#include "fe_kernels.hip.h"
#include "fe_launch.h"

namespace fe {

constexpr int kResampleThreads = 256;

struct ResampleDesc {         // = fe_resample_desc of the C ABI (24 bytes)
    int slot, n_in;
    long long in_offset, out_offset;
};

struct ResampleRingDesc {     // = fe_resample_ring_desc of the C ABI (40 bytes)
    int slot, n_in;
    long long in_base, out_base;
    int in_len, in_pos, out_len, out_pos;
};

struct ResampleArgs {
    const float* table;       // [up][KP] device copy of the tap table (zeros where r + j up > 2 hl: never multiplied)
    int up, down, hl, K, KP;
    int tile_out, xcap;       // outputs per tile (<= 1024), floats of the input tile
    const void* in;
    void* out;
    int in_format, out_format;   // FE_AUDIO_*
    // whole signals
    long long n_in, n_out;
    size_t in_stride, out_stride;
    // packet streams
    int n_in_max;             // (the grid is one workgroup per call stream)
    const ResampleDesc* desc; // [n] device memory, read when the kernel runs
    size_t in_count, out_count;   // elements of in / out: no access outside [0, count)
    float* state;             // [capacity][state_floats]: hist[K - 1] oldest first, the consumed count as two 32-bit words, padding
    int capacity, state_floats;
    int* produced;            // [n] or null
};

// The ring form's argument block: ResampleArgs with one field at the end (a.desc is unused).  A type of its own, so that the other two
// instantiations keep their kernel-argument block - and their code - as they were.
struct ResampleRingArgs : ResampleArgs {
    const ResampleRingDesc* ring_desc;   // [n] device memory, read when the kernel runs
};
template <bool RING> struct ResampleKernelArgs { using type = ResampleArgs; };
template <> struct ResampleKernelArgs<true> { using type = ResampleRingArgs; };

// outputs a stream that has consumed N samples has emitted: every output whose newest input has arrived
__device__ __forceinline__ long long resample_emitted(long long N, int up, int down, int hl) {
    const long long a = N * up - hl;
    return a > 0 ? (a + down - 1) / down : 0;
}

// position l places behind `pos` in a ring of `len` elements, for 0 <= pos < len and 0 <= l <= len
__device__ __forceinline__ long long ring_index(int pos, int len, long long l) {
    const long long p = (long long)pos + l;
    return p >= len ? p - len : p;
}

// ---- G.711 (FE_AUDIO_ULAW / FE_AUDIO_ALAW of the C ABI: one unsigned byte per sample).  The formulas are the contract's (INTEGRATION.md,
// "Audio at another sample rate"), in integer ALU operations: no table, no LDS, no barrier.
constexpr int kAudioUlaw = 4, kAudioAlaw = 5;

__device__ __forceinline__ int g711_ulaw_dec(int b) {
    const int u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15;
    const int mag = (((m << 3) + 0x84) << e) - 0x84;
    return (u & 0x80) ? -mag : mag;
}
__device__ __forceinline__ int g711_alaw_dec(int b) {
    const int a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15;
    const int mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (a & 0x80) ? mag : -mag;
}
// q: an int16 value (pcm16_out).  hibit(v) = 31 - clz(v) of a value that is never 0: v >= 33 here, n | 256 >= 256 below (where n < 256
// the exponent so computed is not used)
__device__ __forceinline__ int g711_ulaw_enc(int q) {
    int v = q >> 2;
    const int mask = v < 0 ? 0x7F : 0xFF;
    v = v < 0 ? -v : v;
    v = (v < 8159 ? v : 8159) + 33;
    const int seg = 31 - __builtin_clz((unsigned)v) - 5;
    const int t = seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 15);
    return t ^ mask;
}
__device__ __forceinline__ int g711_alaw_enc(int q) {
    const int n = q >= 0 ? q : ~q, sign = q >= 0 ? 0x80 : 0;
    const int eh = 31 - __builtin_clz((unsigned)(n | 256)) - 7;
    const int e = n < 256 ? 0 : eh;
    const int m = n < 256 ? n >> 4 : (n >> (eh + 3)) & 15;
    return (sign | (e << 4) | m) ^ 0x55;
}
template <bool ALAW>
__device__ __forceinline__ int g711_enc(float y) { return ALAW ? g711_alaw_enc(pcm16_out(y)) : g711_ulaw_enc(pcm16_out(y)); }

// sample `idx` of the input in any of the four formats (a wave-uniform branch); a G.711 byte is the int16 sample it decodes to
__device__ __forceinline__ float resample_sample_g711(const void* base, int format, long long idx) {
    if (format == kAudioUlaw) return (float)g711_ulaw_dec(static_cast<const unsigned char*>(base)[idx]) * (1.0f / 32768.0f);
    if (format == kAudioAlaw) return (float)g711_alaw_dec(static_cast<const unsigned char*>(base)[idx]) * (1.0f / 32768.0f);
    return stream_sample(base, format, idx);
}

// n samples from src (LDS) to the BYTES out .. out + n of a G.711 output, as head / body / tail: single bytes up to the first 16-byte
// boundary of the destination, then sixteen samples per lane packed into one non-temporal 16-byte store, then single bytes.  A one-byte
// store per lane is a one-byte write on the bus where the destination is page-locked host memory; with byte elements a row's base is
// 16-byte aligned one time in sixteen, hence the head.  The split depends on the address and the length only (wave-uniform), and no store
// covers a byte outside [out, out + n).  (Vector stores only.)
template <bool ALAW>
__device__ __forceinline__ void g711_store_row(unsigned char* out, const float* src, int n, int tid, int nth) {
    const int to_boundary = (int)((16u - (unsigned)(reinterpret_cast<size_t>(out) & 15)) & 15u);
    const int head = to_boundary < n ? to_boundary : n;
    for (int i = tid; i < head; i += nth) __builtin_nontemporal_store((unsigned char)g711_enc<ALAW>(src[i]), out + i);
#ifdef FE_G711_BYTE_BODY       // (a side build for tools/gpu_g711_timing.py: the whole row as single bytes)
    const int n16 = 0;
#else
    const int n16 = (n - head) >> 4;
#endif
    i32x4* o4 = reinterpret_cast<i32x4*>(out + head);
    for (int i = tid; i < n16; i += nth) {
        const float* s = src + head + 16 * i;
        i32x4 v;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = g711_enc<ALAW>(s[4 * w]) | (g711_enc<ALAW>(s[4 * w + 1]) << 8) | (g711_enc<ALAW>(s[4 * w + 2]) << 16) | (g711_enc<ALAW>(s[4 * w + 3]) << 24);
        __builtin_nontemporal_store(v, o4 + i);
    }
    for (int i = head + 16 * n16 + tid; i < n; i += nth) __builtin_nontemporal_store((unsigned char)g711_enc<ALAW>(src[i]), out + i);
}
// ... to elements idx .. of an output in any of the four formats (a wave-uniform branch)
__device__ __forceinline__ void resample_store_row_g711(void* base, int format, long long idx, const float* src, int n, int tid, int nth) {
    if (format == kAudioUlaw) return g711_store_row<false>(static_cast<unsigned char*>(base) + idx, src, n, tid, nth);
    if (format == kAudioAlaw) return g711_store_row<true>(static_cast<unsigned char*>(base) + idx, src, n, tid, nth);
    stream_store_row(base, format, idx, src, n, tid, nth);
}
// the load and the store of an instantiation: G711 - launched only where either format of the call is a G.711 law - dispatches over the
// four formats, the others are stream_sample / stream_store_row as before
template <bool G711>
__device__ __forceinline__ float resample_sample(const void* base, int format, long long idx) {
    if constexpr (G711) return resample_sample_g711(base, format, idx);
    else return stream_sample(base, format, idx);
}
template <bool G711>
__device__ __forceinline__ void resample_store_row(void* base, int format, long long idx, const float* src, int n, int tid, int nth) {
    if constexpr (G711) resample_store_row_g711(base, format, idx, src, n, tid, nth);
    else stream_store_row(base, format, idx, src, n, tid, nth);
}

template <bool STRM, bool RING = false, bool G711 = false>
__global__ __launch_bounds__(kResampleThreads) void fe_resample_kernel(typename ResampleKernelArgs<RING>::type a) {
    static_assert(STRM || !RING, "the ring form is a form of the packet-stream form");
    extern __shared__ float rs_lds[];
    const int tid = (int)threadIdx.x;
    const int up = a.up, down = a.down, K = a.K, KP = a.KP;
    float* T = rs_lds;                          // [up][KP]
    float* X = T + ((up * KP + 3) & ~3);        // [xcap]
    float* Y = X + ((a.xcap + 3) & ~3);         // [tile_out]

    // what this workgroup resamples: outputs [m_begin, m_end) of a signal whose sample g is element in_base + g - g0 of a.in for
    // g0 <= g < g0 + n (STRM: g0 = the stream's consumed count, and hist holds g0 - (K - 1) .. g0 - 1; else g0 = 0 and there is no history)
    long long m_begin = 0, m_end = 0, g0 = 0, in_base = 0, out_base = 0;
    int n = 0;
    float* row = nullptr;
    [[maybe_unused]] int in_len = 0, in_pos = 0, out_len = 0, out_pos = 0;       // RING
    if constexpr (RING) {
        const int b = (int)blockIdx.x;
        const int* p = reinterpret_cast<const int*>(a.ring_desc + b);
        int w[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) w[i] = __builtin_amdgcn_readfirstlane(p[i]);
        const int slot = w[0];
        n = w[1] < 0 ? 0 : (w[1] > a.n_in_max ? a.n_in_max : w[1]);
        in_base = (long long)(((unsigned long long)(unsigned)w[3] << 32) | (unsigned)w[2]);
        out_base = (long long)(((unsigned long long)(unsigned)w[5] << 32) | (unsigned)w[4]);
        in_len = w[6]; in_pos = w[7]; out_len = w[8]; out_pos = w[9];
        long long made = 0;
        bool ok = (unsigned)slot < (unsigned)a.capacity && in_len >= 1 && out_len >= 1 && (unsigned)in_pos < (unsigned)in_len &&
                  (unsigned)out_pos < (unsigned)out_len && n <= in_len;
        if (ok) {
            row = a.state + (size_t)slot * a.state_floats;
            const unsigned* cw = reinterpret_cast<const unsigned*>(row + (K - 1));
            const unsigned lo = __builtin_amdgcn_readfirstlane(cw[0]), hi = __builtin_amdgcn_readfirstlane(cw[1]);
            g0 = (long long)(((unsigned long long)hi << 32) | lo);
            ok = g0 >= 0 && g0 < (1ll << 40);                      // (the rule of the STRM form, below)
        }
        if (ok) {
            m_begin = resample_emitted(g0, up, down, a.hl);
            m_end = resample_emitted(g0 + n, up, down, a.hl);
            made = m_end - m_begin;
            // the whole of each ring inside its buffer: then every index base + (pos + i) mod len is
            const bool in_ok = in_base >= 0 && (unsigned long long)in_base <= a.in_count && a.in_count - (unsigned long long)in_base >= (unsigned long long)in_len;
            const bool out_ok = out_base >= 0 && (unsigned long long)out_base <= a.out_count && a.out_count - (unsigned long long)out_base >= (unsigned long long)out_len;
            ok = made <= (long long)out_len && in_ok && out_ok;
        }
        if (a.produced != nullptr && tid == 0) a.produced[b] = ok ? (int)made : 0;
        if (!ok || n == 0) return;              // skipped, or nothing new: nothing read, nothing written, the row as it was
    } else if constexpr (STRM) {
        const int b = (int)blockIdx.x;
        const int* p = reinterpret_cast<const int*>(a.desc + b);
        int w[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = __builtin_amdgcn_readfirstlane(p[i]);
        const int slot = w[0];
        n = w[1] < 0 ? 0 : (w[1] > a.n_in_max ? a.n_in_max : w[1]);
        in_base = (long long)(((unsigned long long)(unsigned)w[3] << 32) | (unsigned)w[2]);
        out_base = (long long)(((unsigned long long)(unsigned)w[5] << 32) | (unsigned)w[4]);
        long long made = 0;
        bool ok = (unsigned)slot < (unsigned)a.capacity;
        if (ok) {
            row = a.state + (size_t)slot * a.state_floats;
            const unsigned* cw = reinterpret_cast<const unsigned*>(row + (K - 1));
            const unsigned lo = __builtin_amdgcn_readfirstlane(cw[0]), hi = __builtin_amdgcn_readfirstlane(cw[1]);
            g0 = (long long)(((unsigned long long)hi << 32) | lo);
            // (a count that is no count - a row is plain data - must not become an access: beyond 2^40 samples the stream is skipped)
            ok = g0 >= 0 && g0 < (1ll << 40);
        }
        if (ok) {
            m_begin = resample_emitted(g0, up, down, a.hl);
            m_end = resample_emitted(g0 + n, up, down, a.hl);
            made = m_end - m_begin;
            const unsigned long long len_in = (unsigned long long)n, len_out = (unsigned long long)made;
            const bool in_ok = in_base >= 0 && (unsigned long long)in_base <= a.in_count && a.in_count - (unsigned long long)in_base >= len_in;
            const bool out_ok = out_base >= 0 && (unsigned long long)out_base <= a.out_count && a.out_count - (unsigned long long)out_base >= len_out;
            ok = in_ok && out_ok;
        }
        if (a.produced != nullptr && tid == 0) a.produced[b] = ok ? (int)made : 0;
        if (!ok || n == 0) return;              // skipped, or nothing new: nothing read, nothing written, the row as it was
    } else {
        const int b = (int)blockIdx.y;
        n = 0;                                  // (unused: the whole-signal bound is a.n_in)
        m_begin = (long long)blockIdx.x * a.tile_out;
        m_end = m_begin + a.tile_out < a.n_out ? m_begin + a.tile_out : a.n_out;
        in_base = (long long)((size_t)b * a.in_stride);
        out_base = (long long)((size_t)b * a.out_stride) + m_begin;
    }
    const long long n_sig = STRM ? (long long)n : a.n_in;

    for (int i = tid; i < up * KP; i += kResampleThreads) T[i] = a.table[i];

    for (long long m0 = m_begin; m0 < m_end; m0 += a.tile_out) {
        const int cnt = (int)(m_end - m0 < a.tile_out ? m_end - m0 : a.tile_out);
        const long long c0 = m0 * down + a.hl;
        const long long kmax0 = c0 / up;
        const int r0 = (int)(c0 - kmax0 * up);
        // the tile's inputs: signal samples x_lo .. x_lo + span - 1, the oldest tap of its first output to the newest of its last
        const long long x_lo = kmax0 - (K - 1);
        const int span = (r0 + (cnt - 1) * down) / up + K;         // <= xcap (the host's bound is this expression at r0 = up - 1, cnt = tile_out)
        for (int i = tid; i < span; i += kResampleThreads) {
            const long long l = x_lo + i - g0;                     // index into this call's samples
            float v = 0.0f;
            if constexpr (RING) {
                if (l >= 0 && l < n_sig) v = resample_sample<G711>(a.in, a.in_format, in_base + ring_index(in_pos, in_len, l));
            } else {
                if (l >= 0 && l < n_sig) v = resample_sample<G711>(a.in, a.in_format, in_base + l);
            }
            if constexpr (STRM) {
                if (l < 0 && l >= -(long long)(K - 1)) v = row[(K - 1) + (int)l];
            }
            X[i] = v;
        }
        __syncthreads();
        for (int t = tid; t < cnt; t += kResampleThreads) {
            const int c = r0 + t * down;
            const int q = c / up, r = c - q * up;
            const float* tr = T + r * KP;
            const float* xr = X + q + (K - 1);                     // x[kmax], then backwards
            float acc = 0.0f;
            for (int j = 0; j < K - 1; ++j) acc = __builtin_fmaf(tr[j], xr[-j], acc);
            if (r + (K - 1) * up <= 2 * a.hl) acc = __builtin_fmaf(tr[K - 1], xr[-(K - 1)], acc);
            Y[t] = acc;
        }
        __syncthreads();
        if constexpr (RING) {
            // outputs m0 - m_begin .. of this call: up to the ring's end, then from its start (o and first are wave-uniform)
            const long long o = ring_index(out_pos, out_len, m0 - m_begin);
            const int first = (long long)cnt < out_len - o ? cnt : (int)(out_len - o);
            resample_store_row<G711>(a.out, a.out_format, out_base + o, Y, first, tid, kResampleThreads);
            if (first < cnt) resample_store_row<G711>(a.out, a.out_format, out_base, Y + first, cnt - first, tid, kResampleThreads);
        } else {
            resample_store_row<G711>(a.out, a.out_format, out_base + (STRM ? m0 - m_begin : 0), Y, cnt, tid, kResampleThreads);
        }
        // (no barrier here: the next tile overwrites X only behind the barrier above, and Y only behind its own first barrier, which no
        // thread passes before every thread has left this store)
    }

    if constexpr (STRM) {
        // the new history: samples g0 + n - (K - 1) .. g0 + n - 1, from the packet or - a packet shorter than K - 1 - the old history
        // shifted; staged in LDS so that every old value is read before any is overwritten
        for (int i = tid; i < K - 1; i += kResampleThreads) {
            const long long l = (long long)n - (K - 1) + i;
            if constexpr (RING) X[i] = l >= 0 ? resample_sample<G711>(a.in, a.in_format, in_base + ring_index(in_pos, in_len, l)) : row[(K - 1) + (int)l];
            else X[i] = l >= 0 ? resample_sample<G711>(a.in, a.in_format, in_base + l) : row[(K - 1) + (int)l];
        }
        __syncthreads();
        for (int i = tid; i < K - 1; i += kResampleThreads) row[i] = X[i];
        if (tid == 0) {
            const unsigned long long g1 = (unsigned long long)(g0 + n);
            unsigned* cw = reinterpret_cast<unsigned*>(row + (K - 1));
            cw[0] = (unsigned)g1;
            cw[1] = (unsigned)(g1 >> 32);
        }
    }
}

// LDS floats of a launch (the three regions, each rounded up to 4 floats)
inline size_t resample_lds_floats(int up, int KP, int xcap, int tile_out) {
    return (size_t)((up * KP + 3) & ~3) + (size_t)((xcap + 3) & ~3) + (size_t)((tile_out + 3) & ~3);
}

// The launchers, defined in fe_resample.hip - the one translation unit that instantiates the kernels (three forms, each with and without G711), so that the C-ABI unit, which
// includes this header for the argument blocks, carries no device code of them.  Every resampler of the process shares the kernels, and
// the opt-in for dynamic LDS is made once per kernel and device: for the most any ratio needs (160 KiB), not for one handle's footprint.
// g711: the G711 instantiation of the form.
hipError_t launch_resample(bool strm, bool g711, dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleArgs& a);
hipError_t launch_resample_rings(bool g711, dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleRingArgs& a);

}  // namespace fe
