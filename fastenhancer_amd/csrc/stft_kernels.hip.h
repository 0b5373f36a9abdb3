// stft_kernels.hip.h — the STFT front / back ends of the path as stand-alone launches (gfx950).
//
// Inside fe_step / fe_offline the transforms are fused into the frame kernel (fe_kernels.hip.h).  The reference also
// exposes them as modules of their own, which scripts/export_onnx.py:55-57 composes line by line:
//   ONNXSTFT.forward(x, cache) / .inverse(spec, cache)        functional/audio_modules.py:243-303   (streaming, one hop)
//   CompressedSTFT.forward(x) / .inverse(spec)                functional/audio_modules.py:124-164   (offline, centered)
// These kernels back the mirrors of those methods (fe_stft_step, fe_istft_step, fe_stft_offline, fe_istft_offline) and
// the time-parallel overlap-add of fe_offline.  One workgroup = one frame of one stream; radix-2 Stockham FFT in LDS
// (fe::fft_lds).  They are HBM / latency-bound element-wise work around a 512- or 1024-point FFT, not GEMMs.
#pragma once
#include "fe_kernels.hip.h"

namespace fe {

template <int N_>
struct FftShape {
    static constexpr int NFFT = N_;
    static constexpr int LOG2N = (N_ == 512) ? 9 : (N_ == 1024 ? 10 : -1);
    static_assert(LOG2N > 0, "n_fft must be 512 or 1024");
};

// tables: [window N | window_istft N | twiddle N (N/2 float2)]
struct StftArgs {
    const float* tables;
    const float* wav_in;      // streaming: [b*in_stride + n], n < H;  offline: [b*in_stride + n], n < Tw
    size_t in_stride;
    const float* cache_in;    // [B][N-H]
    float* cache_out;         // [B][N-H] (may alias cache_in)
    float* spec;              // streaming: [B][N/2+1][1][2];  offline: [B][F][T][2]
    float* wav_out;           // streaming: [b*out_stride + n], n < H
    size_t out_stride;
    float* frames;            // offline inverse: [B][T][N] windowed frames before the overlap-add
    int B, T, H, Tw;
    int F;                    // offline: number of bins kept (N/2 with discard_last_freq_bin, else N/2+1)
    float compression;        // offline: |X|^(c-1) (forward) / |X|^(1/c-1) (inverse); 1 = none
    float eps;
};

// ONNXSTFT.forward (functional/audio_modules.py:243-257): x = cat(cache, new); cache' = x[-(N-H):]; rfft(x * window)
template <int N>
__global__ void __launch_bounds__(kThreads) stft_step_kernel(StftArgs a) {
    using S = FftShape<N>;
    __shared__ float2 fa[N], fb[N], tw[N / 2];
    const int b = blockIdx.x, tid = threadIdx.x, H = a.H, OVL = N - H;
    const float* win = a.tables;
    const float2* twg = reinterpret_cast<const float2*>(a.tables + 2 * N);
    for (int i = tid; i < N / 2; i += kThreads) tw[i] = twg[i];
    const float* cin = a.cache_in + (size_t)b * OVL;
    const float* xin = a.wav_in + (size_t)b * a.in_stride;
    for (int n = tid; n < N; n += kThreads) {
        const float v = n < OVL ? cin[n] : xin[n - OVL];
        fb[n] = make_float2(v, 0.0f);
        fa[n] = make_float2(v * win[n], 0.0f);
    }
    __syncthreads();
    float* cout = a.cache_out + (size_t)b * OVL;
    for (int m = tid; m < OVL; m += kThreads) cout[m] = fb[m + H].x;
    __syncthreads();
    const float2* X = fft_lds<S, false>(fa, fb, tw);
    float2* out = reinterpret_cast<float2*>(a.spec) + (size_t)b * (N / 2 + 1);
    for (int f = tid; f <= N / 2; f += kThreads) out[f] = X[f];
}

// ONNXSTFT.inverse (functional/audio_modules.py:259-303): irfft (Im X[0], Im X[N/2] ignored), * window_istft,
// x[:N-H] += cache, out = x[:H], cache' = x[H:]
template <int N>
__global__ void __launch_bounds__(kThreads) istft_step_kernel(StftArgs a) {
    using S = FftShape<N>;
    __shared__ float2 fa[N], fb[N], tw[N / 2];
    const int b = blockIdx.x, tid = threadIdx.x, H = a.H, OVL = N - H;
    const float* wi = a.tables + N;
    const float2* twg = reinterpret_cast<const float2*>(a.tables + 2 * N);
    for (int i = tid; i < N / 2; i += kThreads) tw[i] = twg[i];
    const float2* X = reinterpret_cast<const float2*>(a.spec) + (size_t)b * (N / 2 + 1);
    for (int f = tid; f <= N / 2; f += kThreads) {
        const float2 v = X[f];
        if (f == 0 || f == N / 2) fa[f] = make_float2(v.x, 0.0f);
        else { fa[f] = v; fa[N - f] = make_float2(v.x, -v.y); }
    }
    __syncthreads();
    const float2* y = fft_lds<S, true>(fa, fb, tw);
    float* xo = reinterpret_cast<float*>((y == fa) ? fb : fa);
    const float* cin = a.cache_in + (size_t)b * OVL;
    const float invN = 1.0f / (float)N;
    for (int n = tid; n < N; n += kThreads) {
        float v = y[n].x * invN * wi[n];
        if (n < OVL) v += cin[n];
        xo[n] = v;
    }
    __syncthreads();
    float* out = a.wav_out + (size_t)b * a.out_stride;
    for (int n = tid; n < H; n += kThreads) out[n] = xo[n];
    float* cout = a.cache_out + (size_t)b * OVL;
    for (int m = tid; m < OVL; m += kThreads) cout[m] = xo[m + H];
}

// CompressedSTFT.forward (functional/audio_modules.py:146-155 over STFT.forward :70-95): torch.stft(center=True,
// pad_mode="reflect"), keep F bins, X *= max(|X|, eps)^(c-1).  grid (T, B).
template <int N>
__global__ void __launch_bounds__(kThreads) stft_frames_kernel(StftArgs a) {
    using S = FftShape<N>;
    __shared__ float2 fa[N], fb[N], tw[N / 2];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* win = a.tables;
    const float2* twg = reinterpret_cast<const float2*>(a.tables + 2 * N);
    for (int i = tid; i < N / 2; i += kThreads) tw[i] = twg[i];
    const float* xin = a.wav_in + (size_t)b * a.in_stride;
    for (int n = tid; n < N; n += kThreads) {
        int idx = t * a.H + n - N / 2;
        idx = idx < 0 ? -idx : idx;
        idx = idx >= a.Tw ? 2 * (a.Tw - 1) - idx : idx;
        fa[n] = make_float2(xin[idx] * win[n], 0.0f);
    }
    __syncthreads();
    const float2* X = fft_lds<S, false>(fa, fb, tw);
    float2* out = reinterpret_cast<float2*>(a.spec) + (size_t)b * a.F * a.T;
    for (int f = tid; f < a.F; f += kThreads) {
        float2 v = X[f];
        if (a.compression != 1.0f) {
            const float g = pow_f(fmaxf(sqrtf(v.x * v.x + v.y * v.y), a.eps), a.compression - 1.0f);
            v.x *= g; v.y *= g;
        }
        out[(size_t)f * a.T + t] = v;
    }
}

// CompressedSTFT.inverse (functional/audio_modules.py:157-164), first half: un-compress, zero-pad the dropped bin,
// irfft of frame t, * window -> frames[b][t][N].  grid (T, B).
template <int N>
__global__ void __launch_bounds__(kThreads) istft_frames_kernel(StftArgs a) {
    using S = FftShape<N>;
    __shared__ float2 fa[N], fb[N], tw[N / 2];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* win = a.tables;
    const float2* twg = reinterpret_cast<const float2*>(a.tables + 2 * N);
    for (int i = tid; i < N / 2; i += kThreads) tw[i] = twg[i];
    const float2* X = reinterpret_cast<const float2*>(a.spec) + (size_t)b * a.F * a.T;
    for (int f = tid; f <= N / 2; f += kThreads) {
        float2 v = f < a.F ? X[(size_t)f * a.T + t] : make_float2(0.0f, 0.0f);
        if (a.compression != 1.0f) {
            const float g = pow_f(sqrtf(v.x * v.x + v.y * v.y), 1.0f / a.compression - 1.0f);
            v.x *= g; v.y *= g;
        }
        if (f == 0 || f == N / 2) fa[f] = make_float2(v.x, 0.0f);
        else { fa[f] = v; fa[N - f] = make_float2(v.x, -v.y); }
    }
    __syncthreads();
    const float2* y = fft_lds<S, true>(fa, fb, tw);
    float* fr = a.frames + ((size_t)b * a.T + t) * N;
    const float invN = 1.0f / (float)N;
    for (int n = tid; n < N; n += kThreads) fr[n] = y[n].x * invN * win[n];
}

// torch.istft(center=True) tail (functional/audio_modules.py:117-119): y[pos] = sum_t frames[t][n - tH] / sum_t w^2[n - tH],
// n = pos + N/2, for pos < H (T-1).  One thread per output sample; frames stay L2-resident between the two launches.
// Tw_b != nullptr (ragged batch, fe_offline_ragged): utterance b has Tw_b[b] samples = Tb = 1 + Tw_b[b] / H frames of the T the batch is
// laid out for; its output is H (Tb - 1) samples from its own frames only (the rest of its row is left untouched).
__global__ void __launch_bounds__(kThreads) istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win,
                                                            float* __restrict__ wav_out, size_t out_stride, int N, int H, int T,
                                                            const int* __restrict__ Tw_b = nullptr) {
    const int b = blockIdx.y;
    const int pos = blockIdx.x * kThreads + threadIdx.x;
    const int Tb = Tw_b != nullptr ? 1 + Tw_b[b] / H : T;
    const int n_out = H * (Tb - 1);
    if (pos >= n_out) return;
    const int n = pos + N / 2;
    int t_lo = (n - N + H) / H;            // ceil((n - N + 1) / H)
    t_lo = t_lo < 0 ? 0 : t_lo;
    int t_hi = n / H;
    t_hi = t_hi > Tb - 1 ? Tb - 1 : t_hi;
    const float* fr = frames + (size_t)b * T * N;
    float acc = 0.0f, env = 0.0f;
    for (int tt = t_lo; tt <= t_hi; ++tt) {
        const float wv = win[n - tt * H];
        acc += fr[(size_t)tt * N + (n - tt * H)];
        env += wv * wv;
    }
    wav_out[(size_t)b * out_stride + pos] = acc / env;
}

// The audio side of fe_step_chunk after its time-pipelined launch: the STREAMING overlap-add (scripts/export_onnx.py:48-58 hop after hop) of
// the chunk's windowed frames [B][T][N], and the two STFT caches the chunk leaves.  Position p of the chunk's overlap-add, p < T H + OVL
// (OVL = N - H), is the old cache_istft[p] (p < OVL, else 0) plus frames[t][p - t H] of every frame of the chunk that covers p, added OLDEST
// FIRST - the order in which the hop-by-hop walk adds them (its tail carries the older frames' sum into the newer frame).  p < T H goes to
// wav_out, the rest is the new cache_istft; the new cache_stft is the last OVL input samples.  Needs T H >= OVL (the host side checks it):
// then the new caches depend on no old cache value, and thread p < OVL, the only reader of the old cache_istft[p], is also the only writer
// of the new one - no ordering between threads or workgroups is needed.  One thread per output sample; wav_in and wav_out do not overlap.
__global__ void __launch_bounds__(kThreads) stream_ola_kernel(const float* __restrict__ frames, const float* __restrict__ wav_in, size_t in_stride,
                                                             float* __restrict__ cache_stft, float* __restrict__ cache_istft,
                                                             float* __restrict__ wav_out, size_t out_stride, int N, int H, int T) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int OVL = N - H, n_out = T * H;
    if (p >= n_out) return;
    const float* fr = frames + (size_t)b * T * N;
    // the sum at position q: frames ceil((q - N + 1) / H) .. min(q / H, T - 1) on top of `acc`
    auto ola = [&](int q, float acc) {
        int t_lo = (q - N + H) / H;
        t_lo = t_lo < 0 ? 0 : t_lo;
        int t_hi = q / H;
        t_hi = t_hi > T - 1 ? T - 1 : t_hi;
        for (int tt = t_lo; tt <= t_hi; ++tt) acc = fr[(size_t)tt * N + (q - tt * H)] + acc;
        return acc;
    };
    float* cis = cache_istft + (size_t)b * OVL;
    wav_out[(size_t)b * out_stride + p] = ola(p, p < OVL ? cis[p] : 0.0f);
    if (p < OVL) {
        cis[p] = ola(n_out + p, 0.0f);
        cache_stft[(size_t)b * OVL + p] = wav_in[(size_t)b * in_stride + (n_out - OVL + p)];
    }
}

// stream_view (fe_kernels.hip.h) with the hop a run-time value: this file's kernels are not compiled per shape.  The same clamp and the same
// bounds check, word for word - the frame kernel's workgroups and the audio kernel below must make the same stream of a descriptor.
// (A: the packet argument block of any family - StreamFrameArgs, BStreamArgs, FStreamArgs, LStreamArgs: a.B, a.T, a.desc and the two counts.)
template <class A>
__device__ __forceinline__ StreamView stream_view_rt(const A& a, int b, int H) {
    StreamView v{-1, 0, 0, 0};
    if (b < a.B) {
        const int* p = reinterpret_cast<const int*>(a.desc + b);
        int w[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = __builtin_amdgcn_readfirstlane(p[i]);
        v.slot = w[0];
        const int hops = w[1] < 0 ? 0 : (w[1] > a.T ? a.T : w[1]);
        v.in_off = (long long)(((unsigned long long)(unsigned)w[3] << 32) | (unsigned)w[2]);
        v.out_off = (long long)(((unsigned long long)(unsigned)w[5] << 32) | (unsigned)w[4]);
        const unsigned long long len = (unsigned long long)hops * (unsigned long long)H;
        const bool in_ok = v.in_off >= 0 && (unsigned long long)v.in_off <= a.in_count && a.in_count - (unsigned long long)v.in_off >= len;
        const bool out_ok = v.out_off >= 0 && (unsigned long long)v.out_off <= a.out_count && a.out_count - (unsigned long long)v.out_off >= len;
        v.hops = (in_ok && out_ok) ? hops : 0;
    }
    return v;
}

// The frame counters of fe_step_streams_chunk's pipelined launch, zeroed by a launch of their own ahead of it.  Not a memset: captured into
// a graph, the memset node of n x counters words (36 bytes for three streams of FastEnhancer_B) left the counters of later replays unzeroed
// or holding other values on the runtime this was developed on - the frames then ran ahead of their predecessors' state - while a kernel
// node replays as it was captured.
__global__ void __launch_bounds__(kThreads) zero_counters_kernel(unsigned int* __restrict__ flags, int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) flags[i] = 0u;
}

// The audio side of fe_step_streams_chunk after its time-pipelined launch: stream_ola_kernel for the packet step - every stream at its own hop
// count T = hops, its own element offsets, float32 or int16, at its state slot.  One workgroup per call stream, looping over the stream's
// T H + OVL overlap-add positions (OVL = N - H): position p is the old cache_istft[p] (p < OVL, else 0) plus frames[t][p - t H] of every
// frame that covers p, added OLDEST FIRST as the hop-by-hop walk adds them; p < T H is output, the rest the new cache_istft; the new
// cache_stft is the last OVL samples of [old cache_stft | the stream's T H input samples].  ANY T >= 1: with T H < OVL the new caches hold
// shifted old cache values, so the workgroup loads both old caches into LDS, meets at a barrier and only then stores - every read of a
// stream's old caches is ordered before every write of its new ones.  Output goes through the packet step's quantiser and row stores
// (stream_store_row) in tiles of kOlaTile positions, a multiple of 16 bytes in either format, so every tile has the alignment of the first.
// A stream without a hop (0 hops, or skipped by the bounds check) writes nothing; one without state (slot or bank out of range) gets zero
// rows.  The level row: per-thread partials over the thread's own positions in a fixed order, the wave reductions of the frame kernels, the
// waves' words through LDS, wave 0 first, one 16-byte store (levels_put / levels_store) - no atomics, the same bits on every run.
// a: the frame kernel's argument block (a.frames [B][a.T][N], a.T = T_max).  wav_in and wav_out do not overlap.
// A template over that block: FastEnhancer's StreamFrameArgs (fe_step_streams_chunk - the only one with a bank table), and the packet blocks of
// the families whose time pipeline carries the streaming state (fe_step_pool_streams_chunk: BStreamArgs, FStreamArgs, and LStreamArgs for
// LiSenNet's launch on request), which name the same fields - audio, the two STFT caches, descriptors, counts, format, capacity, levels, frames.
constexpr int kOlaTile = 4 * kThreads;
template <class A>
__device__ __forceinline__ int stream_ola_bank(const A& a, const StreamView& sv) {
    if constexpr (std::is_same<A, StreamFrameArgs>::value) return stream_bank<true>(a, sv);
    else return 0;
}
template <class A>
__global__ void __launch_bounds__(kThreads) stream_ola_streams_kernel(A a, int N, int H) {
    __shared__ float old_cis[1024], old_cst[1024], tile[kOlaTile], red[4 * kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const StreamView sv = stream_view_rt(a, b, H);
    if (sv.hops == 0) return;                                   // (wave-uniform, as the two below)
    const int sb = sv.slot;
    if ((unsigned)sb >= (unsigned)a.capacity || stream_ola_bank(a, sv) < 0) {
        stream_zero_row(a.wav_out, a.format, sv.out_off, sv.hops * H, tid, kThreads);
        return;
    }
    const int OVL = N - H, T = sv.hops, n_out = T * H, total = n_out + OVL;
    float* cis = a.cache_istft + (size_t)sb * OVL;
    float* cst = a.cache_stft + (size_t)sb * OVL;
    for (int m = tid; m < OVL; m += kThreads) { old_cis[m] = cis[m]; old_cst[m] = cst[m]; }
    __syncthreads();
    // the new cache_stft: chunk positions n_out - OVL + m, below 0 the old cache
    for (int m = tid; m < OVL; m += kThreads) {
        const int q = n_out - OVL + m;
        cst[m] = q < 0 ? old_cst[q + OVL] : stream_sample(a.wav_in, a.format, sv.in_off + q);
    }
    const bool meters = a.levels != nullptr;
    LevelAcc lv;
    if (meters) {
        float ss = 0.0f, pk = 0.0f;
        for (int i = tid; i < n_out; i += kThreads) {
            const float x = stream_sample(a.wav_in, a.format, sv.in_off + i);
            ss += x * x;
            pk = fmaxf(pk, fabsf(x));
        }
        lv.in_ss = wave_sum(0.0f, ss);
        lv.in_pk = wave_max(0.0f, pk);
    }
    const float* fr = a.frames + (size_t)b * a.T * N;
    // the sum at position q: frames ceil((q - N + 1) / H) .. min(q / H, T - 1) on top of `acc`
    auto ola = [&](int q, float acc) {
        int t_lo = (q - N + H) / H;
        t_lo = t_lo < 0 ? 0 : t_lo;
        int t_hi = q / H;
        t_hi = t_hi > T - 1 ? T - 1 : t_hi;
        for (int tt = t_lo; tt <= t_hi; ++tt) acc = fr[(size_t)tt * N + (q - tt * H)] + acc;
        return acc;
    };
    float oss = 0.0f, opk = 0.0f;
    for (int p0 = 0; p0 < total; p0 += kOlaTile) {              // (the trip count is the workgroup's: the barriers are uniform)
#pragma unroll
        for (int j = 0; j < kOlaTile / kThreads; ++j) {
            const int p = p0 + tid + j * kThreads;
            if (p < total) {
                const float y = ola(p, p < OVL ? old_cis[p] : 0.0f);
                if (p < n_out) {
                    tile[p - p0] = y;
                    oss += y * y;
                    opk = fmaxf(opk, fabsf(y));
                } else {
                    cis[p - n_out] = y;
                }
            }
        }
        __syncthreads();
        const int cnt = n_out - p0 < kOlaTile ? n_out - p0 : kOlaTile;
        if (cnt > 0) stream_store_row(a.wav_out, a.format, sv.out_off + p0, tile, cnt, tid, kThreads);
        __syncthreads();
    }
    if (meters) {
        lv.out_ss = wave_sum(0.0f, oss);
        lv.out_pk = wave_max(0.0f, opk);
        levels_put(red, lv, tid >> 6, tid & 63);
        __syncthreads();
        if (tid == 0) levels_store<kWaves>(a.levels + sb, red);
    }
}

}  // namespace fe
