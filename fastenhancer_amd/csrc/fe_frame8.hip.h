// fe_frame8.hip.h — the per-hop streaming step (scripts/export_onnx.py:48-58, one hop per launch) on a 512-THREAD workgroup:
// eight wavefronts per stream, TWO per SIMD of the CU.
//
// fe_frame_kernel (fe_kernels.hip.h) runs a stream on four waves, one per SIMD: a frame is a chain of ~38 barrier-bounded
// phases, and with a lone wave per SIMD nothing hides a wave's own latencies - the pipeline fill after each barrier, the LDS
// write -> read turn-around, the dependent transcendental chains of the epilogues (52 % MFMA-busy, 42 % of the wave cycles
// waiting, profiles/r3k_*).  Here every phase's tiles are split once more so that each SIMD holds two waves (w and w + 4)
// that issue into each other's stalls:
//   conv-type GEMMs  [F1 x C1] (M = 4 row tiles, N = NTC channel tiles): wave (ws, wh) = row tile ws, channel tiles
//                    [0, NTA) for wh = 0 and [NTA, NTC) for wh = 1 - unequal halves (2 : 1 for FastEnhancer_B) on purpose:
//                    the lighter wave reaches its epilogue while the heavier one still feeds the matrix pipe
//   token GEMMs      [F2P x C2] (M = 2 row tiles): wave (ws, wh) = row tile wh x the column tiles ws, ws + 4 - the
//                    register-resident weight fragments are fetched by both waves of a pair (L1 / L2 hits)
//   attention        wave (ws, wh) = head ws, query tile wh
//   element-wise     512 threads
//   DFT / iDFT       the four-wave transform of Dft<S> on waves 0-3 (one per SIMD), the other four run the
//                    element-wise work next to it (cache shift, constant prefetch)
// Same LDS plan (Lds<S>), same packed weights (Pack<S>), same state and the same arithmetic per output element as
// fe_frame_kernel: the two kernels agree to fp32 rounding (the order of the additions inside a GEMM is the same; tests
// compare both with the oracle and with each other).
// Reference: models/fastenhancer/default/model.py:266-290 (RNNFormer block), 620-675 (model_forward), 677-710 (ONNXModel.forward),
// functional/audio_modules.py:243-303 (ONNXSTFT).
#pragma once
#include "fe_kernels.hip.h"

namespace fe {

constexpr int kThreads8 = 512;
constexpr int kWaves8 = 8;

template <class S>
struct Wg8 {
    using L = Lds<S>;
    static constexpr bool MDFT = (S::NFFT == 512) || (S::C1 < 128);
    // built for the B-type plan: staged conv weights, LDS-resident skips, register-resident block weights with flat GRU gates
    static constexpr bool OK0 = L::STAGED && L::SKIPS_LDS && S::GFLAT && S::KT == 1 && S::LOW == 0 && !S::FRNN && !S::TATT && !S::LN && !S::BIDIR &&
                               S::G8P && S::MTC == 4 && S::MT2 == 2 && MDFT && !L::PERHEAD && S::NFFT == kThreads8 && S::NTPW2 == 1;
    static constexpr int NTA = (S::NTC + 1) / 2, NTB = S::NTC - NTA;        // conv channel tiles of the wh = 0 / wh = 1 wave
    static constexpr int N2A = (S::NT2 + 1) / 2, N2B = S::NT2 - N2A;        // rf_post's token-channel tiles likewise
    static constexpr int NPW = ceil_div(ceil_div(Pack<S>::umax(), 256), kWaves8);
    static constexpr int HPT = ceil_div(S::F2 * S::C2, kThreads8);          // hidden-state elements per thread
    // Weight staging region: FOUR slots of U8_SLOT floats.  The conv units use them as the two buffers of fe_frame_kernel (WB0 = slots
    // 0-1, WB1 = slots 2-3); during the RNNFormer blocks - where fe_frame_kernel's staging buffers sit idle and its waves fetch their
    // private weight fragments from L2 - the BLOCK weights go through the four slots as well: eight waves would fetch every fragment
    // twice (the two waves of a SIMD work on the same columns), 240 wave-level loads per block at ~16 cycles of the CU's vector-memory
    // path each (measured: 3.5 us of the 32.7 us frame, profiles/r4a_wg8_steps.txt); staged, a block is 64 one-KiB pieces.
    //   slot 1: GRU input weights   slot 3: GRU hidden weights   slot 0: rnn_fc, then attn_fc   slot 2: qkv
    static constexpr int SLOT = S::U8_SLOT;
    static constexpr int WB0 = L::NOSTAGE_TOTAL, WB1 = WB0 + 2 * SLOT;
    // The new GRU states of the KB blocks wait in LDS for the end of the frame and leave as whole lines (HST, when it fits): stored from the GRU
    // epilogues - 64-byte pieces of [F2][C2] rows - their acknowledgements were charged to the next vmcnt wait of the weight staging
    // (vmcnt counts loads and stores in order): 0.6 us of the 31.6 us frame (same-box timing experiment, profiles/r4a_wg8_steps.txt)
    // r6: the mixed gate tile's x half and h half are computed by different waves (4 / 5: x, 6 / 7: h - 63 MFMAs per SIMD instead
    // of 72 / 72 / 54 / 54); both write their raw sums here, [half][row tile][16 rows][LDM], and the h-half wave finishes the tile's gate math
    // one element per lane.  + 8 words: the x-half waves' "written" counter of each row tile (monotonic: frame * KB + block + 1), the rest padding
    static constexpr int LDM = 13;
    static constexpr int MXB = L::NOSTAGE_TOTAL + 4 * SLOT, MX_FLOATS = round_up(4 * 16 * LDM + 8, 4), MXF = MXB + 4 * 16 * LDM;
    static constexpr int HST = MXB + MX_FLOATS;
    static constexpr bool HSTASH = (size_t)(HST + S::KB * S::F2 * S::C2) * 4 <= 160 * 1024;
    static constexpr size_t BYTES = (size_t)(HST + (HSTASH ? S::KB * S::F2 * S::C2 : 0)) * 4;
    static constexpr int NPWB = ceil_div(ceil_div(SLOT, 256), kWaves8);      // pieces per wave of a block unit
    static constexpr bool PLAN_OK = 2 * SLOT >= Pack<S>::umax() && BYTES <= 160 * 1024 && (S::NU & 1) == 0;
    static constexpr bool OK = OK0 && PLAN_OK;
};

// Address windows.  fp32 MFMAs and the vector ALU share the SIMD's datapath, so every v_add / v_mul / v_or that forms an LDS address is
// paid in matrix time.  The per-lane part of the frame's few address patterns is therefore formed ONCE, as a 32-bit LDS pointer
// the compiler cannot take apart again (the empty asm: otherwise it re-derives lane * 4 | constant, row * LDC, ... next to every use); a
// phase then reaches its operands as window + compile-time constant, which the ds instructions carry as their 16-bit immediate offset.
using LdsF = __attribute__((address_space(3))) float;
using LdsV4 = __attribute__((address_space(3))) f32x4;
__device__ __forceinline__ LdsF* lds_ptr(const float* p) { return (LdsF*)p; }          // (p points into LDS)
__device__ __forceinline__ LdsF* lds_window(const float* p) {
    LdsF* q = lds_ptr(p);
    asm volatile("" : "+v"(q));
    return q;
}
__device__ __forceinline__ f32x4 lds_v4(const LdsF* p) { return *reinterpret_cast<const LdsV4*>(p); }
// StageSide (the weight-staging side job of a GEMM) whose commit() writes through a window: w = &destination[wave * 256 + lane * 4] of piece 0
template <int NPW, int NP>
struct Stage8 : StageSide<NPW, NP, kWaves8> {
    LdsF* w;
    __device__ __forceinline__ void commit() const {
        using B = StageSide<NPW, NP, kWaves8>;
#pragma unroll
        for (int i = 0; i < B::NPI; ++i) {
            const int p = this->j->wave + kWaves8 * i;
            if (kWaves8 * i + kWaves8 - 1 < NP || p < NP) *reinterpret_cast<LdsV4*>(w + i * (kWaves8 * 256)) = this->j->r[i];
        }
    }
};
// An accumulator that starts as the splat of one LDS word: one read and three v_mov.  (Four reads of the word straight into the
// accumulator's registers - no vector ALU instruction at all - were measured: 31.25 us against 30.65 us, the LDS pipe is the dearer one here.)
__device__ __forceinline__ f32x4 lds_splat(const float* p) {
    const float b = *p;
    return f32x4{b, b, b, b};
}

// One conv-layout GEMM job of a wave: row tile mt x the NT channel tiles J0 .. J0 + NT - 1, K = 4 KS.
//   af(ks) -> A fragment element, bf(j, ks) -> B fragment element of ABSOLUTE tile j, bias(j) -> accumulator start.
// Epilogue: optional activation (Shape::EPA, scaled trunk; ap: its constant), store to out[(row0 + m)][col] for col < NCOLS:
//   dst = &out[row0 + 16 mt + 4 lg][li], this lane's first element (the C-store window of the frame plus a constant, or formed in place).
template <class S, int NT, int J0, int KS, int NCOLS, int LDO, bool ACT, class AF, class BF, class BI, class SIDE>
__device__ __forceinline__ void conv8(AF&& af, BF&& bf, BI&& bias, const SIDE& side, LdsF* dst, int lane, float ap = 0.0f) {
    if constexpr (NT > 0) {
        const int li = lane & 15;
        f32x4 acc[1][NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[0][j] = bias(J0 + j);
        mma_panel<1, NT, KS, Lds<S>::PDK>(acc, [&](int, int ks) { return af(ks); }, [&](int j, int ks) { return bf(J0 + j, ks); }, side);
        side.commit();
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = 16 * (J0 + j) + li;
            if (col < NCOLS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[0][j][r];
                    if (ACT) v = act_scaled_f<S::EPA>(v, ap);
                    dst[r * LDO + 16 * (J0 + j)] = v;
                }
            }
        }
    } else {
        // a wave without a tile still moves its share of the next weight unit
        constexpr int NSG = (KS + 3) / 4;
#pragma unroll
        for (int g = 0; g < NSG; ++g) side(g, NSG);
        side.commit();
    }
}
// the pair split: wh = 0 takes the tiles [0, NA), wh = 1 the tiles [NA, NA + NB)
template <class S, int NA, int NB, int KS, int NCOLS, int LDO, bool ACT, class AF, class BF, class BI, class SIDE>
__device__ __forceinline__ void conv8_pair(int wh, AF&& af, BF&& bf, BI&& bias, const SIDE& side, LdsF* dst, int lane, float ap = 0.0f) {
    // (with the store addresses window + constant, the last activation + store of the two roles differ in operands only and the compiler
    // sinks that chain into a common tail behind the epilogue; keeping it in the roles was measured 0.2 us slower)
    if (wh == 0) conv8<S, NA, 0, KS, NCOLS, LDO, ACT>(af, bf, bias, side, dst, lane, ap);
    else conv8<S, NB, NA, KS, NCOLS, LDO, ACT>(af, bf, bias, side, dst, lane, ap);
}

// DBG: per-stage dumps (fe_debug_step) and the phase cycle probes (fe_profile_step).  PERSIST: more streams than CUs,
// each workgroup walks the streams blockIdx.x, blockIdx.x + gridDim.x, ...  SLOT (fe_step_slots): stream b's state is slot a.slots[b] of a
// state sized for a.capacity streams, as in fe_frame_kernel.  HIO (fe_step_slots_pinned; SLOT only): the audio is page-locked host
// memory - the hop sample of each thread is requested ahead into hv (the first stream's before any other load of the kernel, the next
// stream's once the current one's has been taken), and the output row goes out in non-temporal 16-byte stores.  STRM (fe_step_streams /
// fe_step_streams_pinned; HIO only): slot, hop count (0 or 1 here) and audio offsets come from the stream's descriptor (stream_view), the audio is
// float32 or int16 PCM (a.format, wave-uniform); a stream without a hop is skipped and no hop of it is requested, as in fe_frame_kernel
// BANK (fe_step_streams_banked[_pinned] with a bank table; STRM only): the stream's weights are bank a.bank[slot] of the handle's banks, in an
// instantiation of its own as in fe_frame_kernel
template <class S, bool DBG, bool PERSIST, bool SLOT = false, bool HIO = false, bool STRM = false, bool BANK = false>
__global__ void __launch_bounds__(kThreads8) __attribute__((amdgpu_waves_per_eu(2, 2))) fe_frame8_kernel(typename KernelArgs<SLOT, STRM>::type a_in) {
    static_assert(Wg8<S>::OK, "fe_frame8_kernel: shape outside the 512-thread kernel's plan");
    static_assert(!BANK || STRM, "weight banks: the packet-audio instantiations only");
    static_assert(!HIO || (SLOT && !DBG), "host audio: slotted production instantiations only");
    static_assert(!STRM || HIO, "packet audio: the host-audio instantiations only");
    typename KernelArgs<SLOT, STRM>::type a = a_in;
    if constexpr (STRM) a.T = 1;                     // (one hop per launch: what stream_view clamps the hop counts to)
#ifdef FE_PROBE_HOT
    if constexpr (!DBG) a.dbg = nullptr;
#else
    if constexpr (!DBG) { a.dbg = nullptr; a.clk = nullptr; }
#endif
    FE_CLK(62);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = Lds<S>;
    using W8 = Wg8<S>;
    constexpr int N = S::NFFT, H = S::HOP, OVL = S::OVL, F0 = S::F0, F1 = S::F1;
    constexpr int C1 = S::C1, C2 = S::C2, F2 = S::F2, HD = S::HD;
    constexpr int LDC = S::LDC, LDX = S::LDX, LDG = L::LDGX;
    constexpr int NTH = kThreads8;
#ifndef FE_WG8_PDK
#define FE_WG8_PDK 3      // software-pipeline depth of the token GEMMs (A and B both from LDS)
#endif
    constexpr int PDK = FE_WG8_PDK;

    const int tid0 = threadIdx.x;
    const int tid = tid0;
    const int lane = tid & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = wave0;
    float hv = 0.0f;                                 // (HIO) this thread's hop sample of the next stream the workgroup runs
    auto hop_issue = [&](int bb) {
        if constexpr (STRM) {
            const StreamView v = stream_view<H>(a, bb);
            if (v.hops && tid0 >= OVL) hv = stream_sample(a.wav_in, a.format, v.in_off + (tid0 - OVL));
        } else
        if constexpr (HIO) { if (bb < a.B && tid0 >= OVL) hv = a.wav_in[(size_t)bb * a.in_stride + tid0 - OVL]; }
    };
    hop_issue((int)blockIdx.x);
    const float* __restrict__ wp = a.wp;
    // (BANK) the bank whose unit 0 is staged for the stream to come, as in fe_frame_kernel: the prologue's requests - units 0 and 1 - follow
    // the first stream's bank (descriptor -> bank[slot] -> weight request, in the banked instantiations only)
    int bank_staged = 0;
    if constexpr (BANK) {
        if (a.bank != nullptr) {       // (the run-time test stays: the note at fe_frame_kernel's BANK)
            const int k0 = stream_bank<BANK>(a, stream_view<S::HOP>(a, (int)blockIdx.x));
            bank_staged = k0 < 0 ? 0 : k0;
            wp = a.wp + (size_t)bank_staged * a.bank_stride;
        }
    }
    WSrc<true> wb;
    constexpr PackedOffsets o = Pack<S>::v;
    wb.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wp), 0, o.total * 4, 0x00020000);
    wb.lane4 = lane * 4;
    wb.li4 = (lane & 15) * 4;
    wb.lds = nullptr;
    wb.base = 0;
    wb.k4d = 0;
    float ap = 0.0f;                                 // the activation's constant (Shape::EPP)
    if constexpr (S::EPP) ap = wp[o.act_p];
    // ---- the frame's address windows (lds_window), formed here while the prologue's loads are in flight:
    //   wl0 / wl1  staged B (or A) fragment `+ lane` of the weight buffers WB0 / WB1 - every unit, and every block slot, lies within 64 KB of
    //              its buffer's start                        wq0 / wq1  their 4x replicated bias tables, `+ 4 (lane & 15)`
    //   stC        C / D store of the conv-layout GEMMs, &[16 ws + 4 lg][li] of an [..][LDC] buffer at LDS offset 0: the skips and both decoder
    //              buffers end below 64 KB                   stX  the token GEMMs' store into X, &X[16 wh + 4 lg][min(col, C2)] (tok_dst)
    LdsF* const wl0 = lds_window(smem + W8::WB0 + lane);
    LdsF* const wl1 = lds_window(smem + W8::WB1 + lane);
    //   stG / stS  the GRU epilogue of waves 0 - 3 (row tile wave & 1, channel group wave >> 1): &Hl[16 g_rt + 4 lg][ch] - Hs lies a constant
    //              behind it - and the same element of block 0 in the state stash
    LdsF* const stG = lds_window(smem + L::HL + (16 * (wave0 & 1) + 4 * (lane >> 4)) * LDX + 16 * (wave0 >> 1) + (lane & 15));
    LdsF* const stS = lds_window(smem + W8::HST + (16 * (wave0 & 1) + 4 * (lane >> 4)) * C2 + 16 * (wave0 >> 1) + (lane & 15));
    //   sw0 / sw1  this thread's 16 bytes of piece `wave` of a unit staged into WB0 / WB1 (Stage8::commit)
    LdsF* const sw0 = lds_window(smem + W8::WB0 + wave0 * 256 + lane * 4);
    LdsF* const sw1 = lds_window(smem + W8::WB1 + wave0 * 256 + lane * 4);
    auto swin = [&](int dst_floats) { return dst_floats >= W8::WB1 ? sw1 + (dst_floats - W8::WB1) : sw0 + (dst_floats - W8::WB0); };
    LdsF* const wq0 = lds_window(smem + W8::WB0 + 4 * (lane & 15));
    LdsF* const wq1 = lds_window(smem + W8::WB1 + 4 * (lane & 15));
    LdsF* const stC = lds_window(smem + (16 * (wave0 & 3) + 4 * (lane >> 4)) * LDC + (lane & 15));
    LdsF* const stX = lds_window(smem + L::X + (16 * (wave0 >> 2) + 4 * (lane >> 4)) * LDX +
                                 (16 * (wave0 & 3) + (lane & 15) < C2 ? 16 * (wave0 & 3) + (lane & 15) : C2));

    // ---- one-time: the zero halos (compressed spectrum, skip buffers), twiddles, weight unit 0.
    // !PERSIST (one stream per workgroup): everything the front of the frame waits for is requested HERE, in one memory round trip
    // with the prologue's own loads - the frame and its window, the DFT constants, and weight unit 1 as well (both staging
    // buffers are free at this point), so that enc_pre, a 12-MFMA phase, does not wait for 28 KiB of the next layer's weights.
    float* sc = smem + L::SC;
    float* Ebuf = smem + L::E;
    float* W0 = smem + L::W0;
    float* W1 = smem + L::W1;
    float2* tw = reinterpret_cast<float2*>(smem + L::TW);
    constexpr int NPW = W8::NPW;
    DmaJobT<NPW> job;
    job.l = smem + W8::WB0;
    job.rsrc = wb.rsrc;
    job.soff = (o.u_off[0] + wave * 256) * 4;
    job.wave = wave;
    job.lane = lane;
    typename Dft<S>::FwdConst dc;
    float fv = 0.0f, fw = 0.0f;
    {
        const StageSide<NPW, o.u_size[0] / 256, kWaves8> st0{&job};
        st0(0, 1);
        float2 twv = make_float2(0.0f, 0.0f);
        if (tid < N / 2) twv = reinterpret_cast<const float2*>(wp + o.twiddle)[tid];
        // (r6: committing unit 1 after the forward DFT instead of here - vmcnt completes in order, the first barrier waits for its 28 KiB - measured neutral: 30.76 / 30.76 us)
        DmaJobT<NPW> job1 = job;
        job1.l = smem + W8::WB1;
        job1.soff = (o.u_off[1] + wave * 256) * 4;
        const StageSide<NPW, PERSIST ? 0 : o.u_size[1] / 256, kWaves8> st1{&job1};
        if constexpr (!PERSIST) {
            const int b0 = (int)blockIdx.x;
            if constexpr (SLOT) {
                int s0;
                bool live;
                if constexpr (STRM) {
                    const StreamView v0 = stream_view<H>(a, b0);
                    s0 = v0.slot;
                    live = v0.hops != 0 && (unsigned)s0 < (unsigned)a.capacity;
                } else {
                    s0 = a.slots[b0];
                    live = (unsigned)s0 < (unsigned)a.capacity;
                }
                if constexpr (HIO) fv = (tid < OVL) ? (live ? a.cache_stft[(size_t)s0 * OVL + tid] : 0.0f) : hv;
                else fv = (tid < OVL) ? (live ? a.cache_stft[(size_t)s0 * OVL + tid] : 0.0f) : a.wav_in[(size_t)b0 * a.in_stride + tid - OVL];
            } else {
                fv = (tid < OVL) ? a.cache_stft[(size_t)b0 * OVL + tid] : a.wav_in[(size_t)b0 * a.in_stride + tid - OVL];
            }
            fw = wp[o.window + tid];
            if (wave < 4) Dft<S>::load(dc, wb, o, wave);
            st1(0, 1);
        }
        for (int i = tid; i < 2 * S::LDS_S; i += NTH) smem[L::SC + i] = 0.0f;
        for (int i = tid; i < (S::NL + 1) * 2 * LDC; i += NTH) {
            const int e = i / (2 * LDC), q = i - e * (2 * LDC);
            smem[L::E + e * S::ACT + (q >= LDC ? (F1 + 1) * LDC + (q - LDC) : q)] = 0.0f;
        }
        if (tid < N / 2) tw[tid] = twv;
        if (tid < 8) smem[W8::MXF + tid] = 0.0f;          // (the mixed tile's hand-over counters and the padding behind them: ints, 0)
        st0.commit();
        if constexpr (!PERSIST) {
            st1.commit();
            smem[L::FFT_A + tid] = fv * fw;
        }
    }
    __syncthreads();

    int b = (int)blockIdx.x;
    int fc = 0;
    StreamView sv{-1, 0, 0, 0};                          // (STRM) the stream this workgroup is running
#pragma unroll 1
    do {
        int sb = b;                                      // the stream's state slot
        int nst = a.B;                                   // streams the state is sized for
        if constexpr (SLOT) {
            static_assert(!DBG, "slotted step: production instantiations only");
            if constexpr (STRM) {
                sv = stream_view<H>(a, b);
                sb = sv.slot;
            } else
            sb = a.slots[b];
            nst = a.capacity;
            if constexpr (STRM) {
                const int bk = stream_bank<BANK>(a, sv);       // (!BANK: 0; -1: a bank out of range - the stream is one without state)
                if (sv.hops == 0 || (unsigned)sb >= (unsigned)nst || bk < 0) {      // (wave-uniform) no hop: nothing; no state: the stream's output row is zero
                    if (sv.hops) stream_zero_row(a.wav_out, a.format, sv.out_off, H, tid0, NTH);
                    __builtin_amdgcn_s_waitcnt(0);       // (the weight stages issued for this stream have landed before the next one or the end)
                    b += (int)gridDim.x;
                    hop_issue(b);
                    continue;
                }
                if (BANK && a.bank != nullptr) {
                    // the stream's own bank from here on: wp, the resource of every weight fetch and of the staging jobs (jb1 / jb2 copy it below)
                    wp = a.wp + (size_t)bk * a.bank_stride;
                    wb.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wp), 0, o.total * 4, 0x00020000);
                    job.rsrc = wb.rsrc;
                    if constexpr (PERSIST) {
                        if (bk != bank_staged) {
                            // unit 0 was staged from another bank (the last phase of the stream before, or the prologue): fetch this bank's into the
                            // buffer stream fc consumes it from - nothing reads that buffer since the stage that filled it; the barrier orders these
                            // LDS stores before enc_pre's reads.  (Unit 1 rides in enc_pre, with the resource set above.)
                            DmaJobT<NPW> jr = job;
                            jr.l = smem + (((S::NU & 1) && (fc & 1)) ? W8::WB1 : W8::WB0);
                            jr.soff = (o.u_off[0] + wave0 * 256) * 4;
                            const StageSide<NPW, o.u_size[0] / 256, kWaves8> str{&jr};
                            str(0, 1);
                            str.commit();
                            __syncthreads();
                        }
                    }
                    bank_staged = bk;
                }
            } else
            if ((unsigned)sb >= (unsigned)nst) {         // (wave-uniform) no state: the stream's output row is zero
                if constexpr (HIO) { if (tid0 < H) __builtin_nontemporal_store(0.0f, a.wav_out + (size_t)b * a.out_stride + tid0); }
                else
                if (tid0 < H) a.wav_out[(size_t)b * a.out_stride + tid0] = 0.0f;
                __builtin_amdgcn_s_waitcnt(0);           // (the weight stages issued for this stream have landed before the next one or the end)
                b += (int)gridDim.x;
                hop_issue(b);
                continue;
            }
        }
        // PERSIST: a loop-variant zero keeps the wave-uniform / per-lane offsets of a frame from being hoisted out of the stream loop
        // (hoisted, they stay live through the whole frame and spill - see fe_frame_kernel)
        int lz = 0, lzv = 0;
        if constexpr (PERSIST) { asm volatile("" : "+s"(lz)); asm volatile("" : "+v"(lzv)); }
        const int wave = wave0 + lz;
        const int tid = tid0 + lzv;
        const int lane = tid & 63;
        const int ws = wave & 3, wh = wave >> 2;          // SIMD slot, half
        const int li = lane & 15, lg = lane >> 4;
        StreamCtl<STRM> ctl;                              // (STRM) the limit and the meters' partials of this stream
        // (the meters' hand-over uses the head of PT while other waves may still read the iSTFT's quarters: PT lies beyond them)
        static_assert(!STRM || (L::PT - L::FFT_A >= L::END_FFT && S::F1 * S::LDP >= 4 * kWaves8), "levels_put / levels_store: PT clear of the FFT buffers");
        float* cst = a.cache_stft + (size_t)sb * OVL;
        float* cis = a.cache_istft + (size_t)sb * OVL;
        const int fpar = (S::NU & 1) ? (fc & 1) : 0;
#define FE8_BEGIN_UNIT(U)                                                                          \
        constexpr int fe_un_ = ((U) + 1 == S::NU) ? 0 : (U) + 1;                                   \
        /* (NU is even - Wg8::PLAN_OK -, so unit U is read from WB0 / WB1 by its parity: a compile-time choice of window) */ \
        constexpr int ub_ = o.u_off[(U)];                                                          \
        LdsF* const wl_ = ((U) & 1) ? wl1 : wl0;                                                   \
        LdsF* const wq_ = ((U) & 1) ? wq1 : wq0;                                                   \
        (void)ub_; (void)wl_; (void)wq_;                                                           \
        {                                                                                          \
            const int slot_ = ((U) & 1) ^ fpar;                                                    \
            job.l = smem + (slot_ ? W8::WB0 : W8::WB1);                                            \
            job.soff = (o.u_off[fe_un_] + wave * 256) * 4;                                         \
            wb.lds = smem + (slot_ ? W8::WB1 : W8::WB0);                                           \
            wb.base = o.u_off[(U)];                                                                \
        }                                                                                          \
        const Stage8<NPW, ((!PERSIST && ((U) + 1 == S::NU || (U) == 0)) || (U) == S::U_RFPRE + 1) ? 0 : o.u_size[fe_un_] / 256> stage{{&job}, ((U) & 1) ? sw0 : sw1}
        FE_CLK(0);
        // =========================== STFT (a1-a3) ===========================
        // LDS quarters of the FFT arena: q0 windowed frame / iSTFT partial sums, q1 iSTFT partial sums, q3 spectrum {Re[N/2], Im[N/2]}
        float* q0 = smem + L::FFT_A;
        float* q1 = q0 + N;
        float* q3 = smem + L::FFT_B + N;
        {
            if constexpr (PERSIST) {
                if (wave < 4) Dft<S>::load(dc, wb, o, wave);             // in flight while the frame is fetched
                const float* xin = a.wav_in + (size_t)b * a.in_stride;
                if constexpr (HIO) {
                    fv = (tid < OVL) ? cst[tid] : hv;                      // (requested ahead) and the next stream's, under this frame
                    hop_issue(b + (int)gridDim.x);
                } else
                fv = (tid < OVL) ? cst[tid] : xin[tid - OVL];            // one sample per thread
                fw = wp[o.window + tid];
                q0[tid] = fv * fw;
                __syncthreads();
            }
            // cache' = frame[H:], straight from the registers (every load of the old cache has landed: its value went to LDS above)
            if (tid >= H) cst[tid - H] = fv;
            if constexpr (STRM) {
                // the meters' input side: the hop is the frame's samples n >= OVL (on the waves that hold one; the others go on to the DFT)
                if (a.levels != nullptr && 64 * (wave + 1) > OVL) {
                    const float x = tid >= OVL ? fv : 0.0f;
                    ctl.lv.in_ss = wave_sum(0.0f, x * x);
                    ctl.lv.in_pk = wave_max(0.0f, fabsf(x));
                }
            }
            FE_CLK(1);
            float* nyq = a.dbg ? a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(0) + 2 * F0 : nullptr;
            if (wave < 4) Dft<S>::template forward<false>(q0, q3, tw, dc, wave, lane, nyq);
            __syncthreads();
            FE_CLK(2);
            const float* Xr = q3;
            const float* Xi = q3 + N / 2;
            if (a.dbg) {
                float* dst = a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(0);
                for (int f = tid; f < F0; f += NTH) { dst[2 * f] = Xr[f]; dst[2 * f + 1] = Xi[f]; }
            }
            // =========================== compress (a4) ===========================
            for (int f = tid; f < F0; f += NTH) {
                const float re = Xr[f], im = Xi[f];
                const float mag = fmaxf(sqrtf(re * re + im * im), 1.0e-5f);
                const float g = pow_f(mag, a.compression - 1.0f);
                sc[2 + f] = re * g;
                sc[S::LDS_S + 2 + f] = im * g;
            }
        }
        __syncthreads();
        if (a.dbg) {
            float* dst = a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(1);
            for (int f = tid; f < F0; f += NTH) { dst[2 * f] = sc[2 + f]; dst[2 * f + 1] = sc[S::LDS_S + 2 + f]; }
        }

        FE_CLK(3);
        // =========================== enc_pre (a5): strided conv as a K = 16 GEMM ===========================
        {
            FE8_BEGIN_UNIT(0);
            // A[row][kk] = sc[c][4 (row + tp) + s] with kk = 4 ks + lg = 8 tp + 2 s + c: lg gives c and the low bit of s, ks the rest - a
            // per-lane base and a compile-time offset per k-step
            const float* const a0 = sc + (lg & 1) * S::LDS_S + 4 * (16 * ws + li) + (lg >> 1);
            conv8_pair<S, W8::NTA, W8::NTB, 4, C1, LDC, true>(
                wh, [&](int ks) { return a0[4 * (ks >> 1) + 2 * (ks & 1)]; },
                [&](int j, int ks) -> float { return wl_[o.enc_pre_w - ub_ + (j * 4 + ks) * 64]; },
                [&](int j) { return lds_v4(wq_ + (o.enc_pre_b - ub_ + j * 64)); }, stage, stC + (L::E + LDC), lane, ap);
        }
        __syncthreads();
        dbg_dump<S, NTH>(a, b, 2, Ebuf + LDC, LDC);

        FE_CLK(4);
        // =========================== encoder (a6): k = 3 convs ===========================
        static_for<S::NL>([&](auto l_) {
            constexpr int l = decltype(l_)::value;
            const float* in = Ebuf + l * S::ACT;
            float* out = Ebuf + (l + 1) * S::ACT;
            if (l == 0) FE_CLK(40);
            {
                FE8_BEGIN_UNIT(S::U_ENC + l);
                const float* const t0 = in + (16 * ws + li) * LDC + lg;
                conv8_pair<S, W8::NTA, W8::NTB, 3 * S::KS_C, C1, LDC, true>(
                    wh, [&](int ks) { return t0[(ks / S::KS_C) * LDC + 4 * (ks % S::KS_C)]; },
                    [&](int j, int ks) -> float { return wl_[o.enc_w[l] - ub_ + (j * (3 * S::KS_C) + ks) * 64]; },
                    [&](int j) { return lds_v4(wq_ + (o.enc_b[l] - ub_ + j * 64)); }, stage, stC + (L::E + (l + 1) * S::ACT + LDC), lane, ap);
            }
            if (l == 0) FE_CLK(42);
            __syncthreads();
            if (l == 0) FE_CLK(43);
            dbg_dump<S, NTH>(a, b, 3 + l, out + LDC, LDC);
        });

        float* Xb = smem + L::X;
        float* Hl = smem + L::HL;
        float* Hs = smem + L::HS;
        float* Gi = smem + L::GI;
        float* Y1 = smem + L::Y1;
        float* Y2 = smem + L::Y2;

        FE_CLK(5);
        // =========================== rf_pre (a7) ===========================
        constexpr int NTPW3 = S::NTPW3;
        constexpr int HPT = W8::HPT;
        constexpr int K2 = S::KS_2;
        f32x4 xr;                                      // residual stream x: row tile wh, channel tile ws
        // GRU: (channel group, row tile) jobs - waves 0-3 a 16-channel group x a row tile (three gate tiles: 54 MFMAs), waves 4 / 5
        // (SIMDs 0 and 1) the x half and waves 6 / 7 (SIMDs 2 and 3) the h half of a row tile's mixed tile of the left-over channels (9 MFMAs
        // each): 63 MFMAs per SIMD, and the three gates of a (row, channel) meet in one lane
        const int g_rt = wave & 1;                                         // row tile of this wave's GRU job
        const int g_t0 = wave < 4 ? 3 * (wave >> 1) : 3 * S::G8_NG;        // its first gate tile
        // block weights in LDS (W8 slots): B fragment (tile, k-step) of a unit at u[(tile * K2 + ks) * 64 + lane], start value of a tile's
        // column at u[NT * K2 * 64 + tile * 16 + li]
        const float* const sGx = smem + W8::WB0 + 1 * W8::SLOT;
        const float* const sGh = smem + W8::WB0 + 3 * W8::SLOT;
        const float* const sF = smem + W8::WB0 + 0 * W8::SLOT;
        static_assert(W8::WB1 == W8::WB0 + 2 * W8::SLOT, "slots 2 (qkv) and 3 are reached through WB1's window");
        constexpr int NPWB = W8::NPWB;
        DmaJobT<NPWB> jb1, jb2;                        // staging jobs of the block units (two may ride in one GEMM)
        jb1.rsrc = wb.rsrc; jb1.wave = wave; jb1.lane = lane; jb1.l = smem; jb1.soff = 0;
        jb2 = jb1;
        auto stage_to = [&](DmaJobT<NPWB>& j, int src_floats, int dst_floats) { j.l = smem + dst_floats; j.soff = (src_floats + wave * 256) * 4; };
        constexpr int u8_stride = S::KB > 1 ? o.u8_gx[1] - o.u8_gx[0] : 0;
        using StG = Stage8<NPWB, S::U8_G / 256>;
        using StF = Stage8<NPWB, S::U8_F / 256>;
        using StQ = Stage8<NPWB, S::U8_Q / 256>;
        float pe_r[4];
        // unpredicated epilogue stores into the [F2P][C2 + 2] token buffer X (pad rows are real rows, lanes past C2 aim at the pad column):
        // stX, the prologue's window &X[16 wh + 4 lg][min(16 ws + li, C2)]
        int hs_off[HPT];
#pragma unroll
        for (int q = 0; q < HPT; ++q) {
            const int i = tid + q * NTH, f = i / C2;
            hs_off[q] = i < F2 * C2 ? f * LDX + (i - f * C2) : C2;
        }
        {
            // Y1[f2][c1] = sum_f1 Wf[f2][f1] E[f1][c1]      (A = packed filterbank rows of tile wh, B = LDS, channel tile ws)
            constexpr int KS = F1 / 4;
            const float* Ein = Ebuf + S::NL * S::ACT + LDC;   // row 0 = bin 0
            FE8_BEGIN_UNIT(S::U_RFPRE);
            stage_to(jb1, o.u8_gx[0], W8::WB0 + 1 * W8::SLOT);          // block 0's GRU input weights -> slot 1
            const StG stg{{&jb1}, swin(W8::WB0 + 1 * W8::SLOT)};
            f32x4 acc[1][1];
            acc_init_zero<1, 1>(acc);
            const int nt = ws < S::NTC ? ws : S::NTC - 1;
            mma_panel<1, 1, KS, PDK>(
                acc, [&](int, int ks) -> float { return wl_[o.rfpre_lin - ub_ + (wh * KS + ks) * 64]; },
                [&](int, int ks) { return Ein[(4 * ks + lg) * LDC + 16 * nt + li]; }, side2(stage, stg));
            stage.commit();
            stg.commit();
            const int col = 16 * ws + li;
            if (ws < S::NTC && col < C1 && 16 * wh + 4 * lg < F2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Y1[(16 * wh + 4 * lg + r) * LDC + col] = acc[0][0][r];
            }
        }
        __syncthreads();
        {
            // X[f2][c2] = Y1[f2][:] . Wc[c2][:] + b
            FE8_BEGIN_UNIT(S::U_RFPRE + 1);
            stage_to(jb1, o.u8_gh[0], W8::WB0 + 3 * W8::SLOT);          // ... and the hidden weights -> slot 3
            const StG stg{{&jb1}, swin(W8::WB0 + 3 * W8::SLOT)};
            float hpre[HPT];
            const float* hg0 = a.h + (size_t)sb * (F2 * C2);
#pragma unroll
            for (int q = 0; q < HPT; ++q) { const int i = tid + q * NTH; hpre[q] = hg0[i < F2 * C2 ? i : F2 * C2 - 1]; }
            f32x4 acc[1][1];
            const int nt = ws < S::NT2 ? ws : S::NT2 - 1;
            acc[0][0] = lds_v4(wq_ + (o.rfpre_b - ub_ + nt * 64));
            const float* ya = Y1 + (16 * wh + li) * LDC + lg;
            const LdsF* const wt = wl_ + (o.rfpre_w - ub_ + nt * (S::KS_C * 64));
            mma_panel<1, 1, S::KS_C, PDK>(
                acc, [&](int, int ks) { return ya[4 * ks]; },
                [&](int, int ks) -> float { return wt[ks * 64]; }, stg);
            (void)stage;
            stg.commit();
            xr = acc[0][0];
#pragma unroll
            for (int r = 0; r < 4; ++r) stX[r * LDX] = acc[0][0][r];
#pragma unroll
            for (int q = 0; q < HPT; ++q) Hs[hs_off[q]] = hpre[q];
        }
        __syncthreads();
        dbg_dump<S, NTH>(a, b, 3 + S::NL, Xb, LDX);

        FE_CLK(6);
        // =========================== RNNFormer blocks (a9-a11) ===========================
#pragma unroll
        for (int k = 0; k < S::KB; ++k) {
            float* hg = a.h + ((size_t)k * nst + sb) * (F2 * C2);
            const int ub = k * u8_stride;
            if (k == 0) FE_CLK(20);
            {
                // GRU (nn.GRU gate order r, z, n; model.py:187, 271) over (channel group, row tile) jobs, the gate math in the GEMM
                // epilogue - r, z, n of a (row, channel) sit in one lane: no exchange through LDS, one barrier for the phase.
                // Staged meanwhile: this block's rnn_fc -> slot 0 and qkv -> slot 2.
                stage_to(jb1, o.u8_f1[0] + ub, W8::WB0 + 0 * W8::SLOT);
                stage_to(jb2, o.u8_q[0] + ub, W8::WB0 + 2 * W8::SLOT);
                const StF st1{{&jb1}, swin(W8::WB0 + 0 * W8::SLOT)};
                const StQ st2{{&jb2}, swin(W8::WB0 + 2 * W8::SLOT)};
                const auto sideg = side2(st1, st2);
                if (k == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * wh + 4 * lg + r, col = 16 * ws + li;
                        pe_r[r] = wb.gather_g(o.blk_pe + (row < F2 ? row : F2 - 1) * C2 + (col < C2 ? col : C2 - 1));
                    }
                }
                const float* xa = Xb + (16 * g_rt + li) * LDX + lg;
                const float* ha = Hs + (16 * g_rt + li) * LDX + lg;
                const LdsF* const wx = wl0 + (1 * W8::SLOT + g_t0 * (K2 * 64));         // = sGx + .. + lane
                const LdsF* const wh_ = wl1 + (1 * W8::SLOT + g_t0 * (K2 * 64));        // = sGh + .. + lane (slot 3 = WB1 + SLOT)
                const float* bx = sGx + S::G8_NT * K2 * 64 + g_t0 * 16 + li;
                const float* bh = sGh + S::G8_NT * K2 * 64 + g_t0 * 16 + li;
                __builtin_amdgcn_sched_barrier(0);
                if (k == 0) FE_CLK(45);
                if (wave < 4) {
                    // a 16-channel group: tiles r, z (x and h halves in one accumulator), n (separate halves)
                    const int ch = 16 * (wave >> 1) + li;
                    float hprev[4];                      // previous state of this lane's outputs: in flight under the GEMM
#pragma unroll
                    for (int r = 0; r < 4; ++r) hprev[r] = stG[(L::HS - L::HL) + r * LDX];           // = Hs[(16 g_rt + 4 lg + r) LDX + ch]
                    f32x4 ar = lds_splat(bx), az = lds_splat(bx + 16);
                    f32x4 anx = lds_splat(bx + 32), anh = lds_splat(bh + 32);
                    mma_panel_sel<1, 3, 2 * K2, PDK>(
                        [&](int, int j, int ks) -> f32x4& { return j == 0 ? ar : (j == 1 ? az : (ks < K2 ? anx : anh)); },
                        [&](int, int ks) { return ks < K2 ? xa[4 * ks] : ha[4 * (ks - K2)]; },
                        [&](int j, int ks) -> float { return ks < K2 ? wx[(j * K2 + ks) * 64] : wh_[(j * K2 + (ks - K2)) * 64]; }, sideg);
                    __builtin_amdgcn_sched_barrier(0);
                    if (k == 0) FE_CLK(46);
                    float hn[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float rr = sigmoid_pre(ar[r]);        // (the packer scales the gate rows: -log2 e / 2 log2 e)
                        const float zz = sigmoid_pre(az[r]);
                        const float nn = tanh_pre(__builtin_fmaf(rr, anh[r], anx[r]));
                        hn[r] = __builtin_fmaf(zz, hprev[r] - nn, nn);          // (1 - z) n + z h
                    }
                    if (16 * g_rt + 4 * lg < F2) {       // (F2 % 4 == 0: the four rows of a lane are valid together)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * g_rt + 4 * lg + r;
                            stG[r * LDX] = hn[r];                                                    // = Hl[row * LDX + ch]
                            if constexpr (W8::HSTASH) stS[k * (F2 * C2) + r * C2] = hn[r];              // = stash[k][row][ch]
                            else hg[row * C2 + ch] = hn[r];
                        }
                    }
                } else {
                    // r6: the mixed tile (the left-over R channels' r | z | n columns) of row tile g_rt, x half on waves 4 / 5, h half on waves
                    // 6 / 7: 9 MFMAs each next to the 54 of their SIMD's channel-group job - 63 MFMAs per SIMD.  Each half goes to LDS as a
                    // [16 rows][3 R columns] matrix; the h-half wave waits for its partner's counter (a wave's LDS operations execute in order)
                    // and finishes the R channels one (row, channel) per lane.  Same chains, same summation order and gate arithmetic as ONE wave
                    // running the tile's x and h halves as a single 2 K2-step panel.
                    constexpr int R = S::G8_R, LDM = W8::LDM;
                    const bool hhalf = wave >= 6;
                    float* mx = smem + W8::MXB + ((hhalf ? 2 : 0) + g_rt) * (16 * LDM);
                    int* mflag = reinterpret_cast<int*>(smem + W8::MXF) + g_rt;
                    const int seq = fc * S::KB + k + 1;
                    f32x4 s0, s1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    __builtin_amdgcn_s_setprio(3);
                    if (!hhalf) {
                        s0 = lds_splat(bx);
                        mma_panel_sel<1, 1, K2, PDK>([&](int, int, int ks) -> f32x4& { return (ks & 1) ? s1 : s0; },
                                                     [&](int, int ks) { return xa[4 * ks]; }, [&](int, int ks) -> float { return wx[ks * 64]; }, sideg);
                    } else {
                        s0 = lds_splat(bh);
                        // (the chains go by the parity of the k-step of the whole 2 K2-step x | h panel: K2 is odd here, so the biased chain takes
                        // the h half's odd local steps)
                        mma_panel_sel<1, 1, K2, PDK>([&](int, int, int ks) -> f32x4& { return ((ks + K2) & 1) ? s1 : s0; },
                                                     [&](int, int ks) { return ha[4 * ks]; }, [&](int, int ks) -> float { return wh_[ks * 64]; }, sideg);
                    }
                    // (the priority stays raised through the hand-over and the gate math: at priority 0 every instruction of this dependent chain
                    // waited for a gap between the MFMAs of the SIMD's 54-MFMA job - 1.5 k cycles for ~35 instructions, and this wave arrived last)
                    s0 += s1;
                    __builtin_amdgcn_sched_barrier(0);
                    if (k == 0) FE_CLK(46);
                    if (li < 3 * R) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx[(4 * lg + r) * LDM + li] = s0[r];
                    }
                    if (!hhalf) {
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): the writes above are in LDS
                        if (lane == 0) __hip_atomic_store(mflag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                    } else {
                        const int row = lane >> 2, c = lane & 3;
                        static_assert(R == 4, "one (row, channel) per lane: sixteen rows x four channels");
                        const int ch = 16 * S::G8_NG + c;
                        const bool live = 16 * g_rt + row < F2;
                        const float hprev = Hs[(16 * g_rt + row) * LDX + ch];
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(mflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < seq) {}
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        const float* mxx = smem + W8::MXB + g_rt * (16 * LDM) + row * LDM + c;
                        const float* mxh = mx + row * LDM + c;
                        const float sxr = mxx[0], sxz = mxx[R], sxn = mxx[2 * R];
                        const float shr = mxh[0], shz = mxh[R], shn = mxh[2 * R];
                        const float rr = sigmoid_pre(sxr + shr);
                        const float zz = sigmoid_pre(sxz + shz);
                        const float nn = tanh_pre(__builtin_fmaf(rr, shn, sxn));
                        const float hn = __builtin_fmaf(zz, hprev - nn, nn);          // (1 - z) n + z h
                        if (live) {
                            Hl[(16 * g_rt + row) * LDX + ch] = hn;
                            if constexpr (W8::HSTASH) smem[W8::HST + k * (F2 * C2) + (16 * g_rt + row) * C2 + ch] = hn;
                            else hg[(16 * g_rt + row) * C2 + ch] = hn;
                        }
                    }
                    __builtin_amdgcn_s_setprio(0);
                }
                st1.commit();
                st2.commit();
            }
            if (k == 0) FE_CLK(47);
            __syncthreads();
            if (k == 0) FE_CLK(21);
            if (k == 0) FE_CLK(22);
            const int ntf = ws < S::NT2 ? ws : S::NT2 - 1;           // this wave's channel tile of the fc layers (ws = 3: a shadow of the last)
            {
                // x += rnn_fc(h') (+ pe in block 0); staged meanwhile: the next block's GRU input weights -> slot 1
                stage_to(jb1, o.u8_gx[0] + ub + u8_stride, W8::WB0 + 1 * W8::SLOT);
                const StG stn{{&jb1}, swin(W8::WB0 + 1 * W8::SLOT)};
                f32x4 acc[1][1];
                acc[0][0] = lds_splat(sF + S::NT2 * K2 * 64 + ntf * 16 + li);
                const float* hla = Hl + (16 * wh + li) * LDX + lg;
                const LdsF* const wf = wl0 + ntf * (K2 * 64);                           // = sF + .. + lane
                if (k + 1 < S::KB) {
                    mma_panel<1, 1, K2, PDK>(acc, [&](int, int ks) { return hla[4 * ks]; }, [&](int, int ks) -> float { return wf[ks * 64]; }, stn);
                    stn.commit();
                } else
                    mma_panel<1, 1, K2, PDK>(acc, [&](int, int ks) { return hla[4 * ks]; }, [&](int, int ks) -> float { return wf[ks * 64]; }, NoSide{});
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[0][0][r] + xr[r];
                    if (k == 0) v += pe_r[r];
                    xr[r] = v;
                    stX[r * LDX] = v;
                }
            }
            __syncthreads();
            dbg_dump<S, NTH>(a, b, 4 + S::NL + 2 * k, Xb, LDX);
            if (k == 0) FE_CLK(23);
            {
                // qkv = x W_qkv^T -> Gi (columns per head interleaved [h][q|k|v][hd]); staged meanwhile: attn_fc -> slot 0
                stage_to(jb1, o.u8_f2[0] + ub, W8::WB0 + 0 * W8::SLOT);
                const StF st1{{&jb1}, swin(W8::WB0 + 0 * W8::SLOT)};
                f32x4 acc[1][NTPW3];
                acc_init_zero<1, NTPW3>(acc);
                __builtin_amdgcn_sched_barrier(0);
                if (k == 0) FE_CLK(50);
                const float* xa = Xb + (16 * wh + li) * LDX + lg;
                mma_panel<1, NTPW3, K2, PDK>(acc, [&](int, int ks) { return xa[4 * ks]; },
                                             [&](int j, int ks) -> float {
                                                 int nt = ws + 4 * j;
                                                 nt = nt < S::NT3 ? nt : S::NT3 - 1;
                                                 return wl1[(nt * K2 + ks) * 64];                // = sQ[.. + lane] (slot 2 = WB1)
                                             }, st1);
                st1.commit();
                __builtin_amdgcn_sched_barrier(0);
                if (k == 0) FE_CLK(51);
                float* gdst = Gi + (16 * wh + 4 * lg) * LDG + 16 * ws + li;
#pragma unroll
                for (int j = 0; j < NTPW3; ++j)
                    if (ws + 4 * j < S::NT3) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) gdst[r * LDG + 64 * j] = acc[0][j][r];
                    }
                __builtin_amdgcn_sched_barrier(0);
                if (k == 0) FE_CLK(52);
            }
            __syncthreads();
            if (k == 0) FE_CLK(24);
            // attention: wave (ws, wh) = head ws, query tile wh
            attention_head<S, 1, LDG>(Gi, Hl, ws * 3 * HD, ws, wh, 1, lane);
            __syncthreads();
            if (k == 0) FE_CLK(25);
            {
                // x += attn_fc(o); staged meanwhile: the next block's GRU hidden weights -> slot 3 (last block: rf_post's filterbank -> WB1);
                // the next block's hidden state is fetched now and parked after the GEMM
                float hpre[HPT];
                if (k + 1 < S::KB) {
                    const float* hgn = hg + (size_t)nst * (F2 * C2);
#pragma unroll
                    for (int q = 0; q < HPT; ++q) { const int i = tid + q * NTH; hpre[q] = hgn[i < F2 * C2 ? i : F2 * C2 - 1]; }
                }
                f32x4 acc[1][1];
                acc[0][0] = lds_splat(sF + S::NT2 * K2 * 64 + ntf * 16 + li);
                const float* hla = Hl + (16 * wh + li) * LDX + lg;
                const LdsF* const wf = wl0 + ntf * (K2 * 64);                           // = sF + .. + lane
                if (k + 1 < S::KB) {
                    stage_to(jb1, o.u8_gh[0] + ub + u8_stride, W8::WB0 + 3 * W8::SLOT);
                    const StG stn{{&jb1}, swin(W8::WB0 + 3 * W8::SLOT)};
                    mma_panel<1, 1, K2, PDK>(acc, [&](int, int ks) { return hla[4 * ks]; }, [&](int, int ks) -> float { return wf[ks * 64]; }, stn);
                    stn.commit();
                } else {
                    stage_to(jb1, o.u_off[S::U_RFPOST], W8::WB1);
                    const Stage8<NPWB, o.u_size[S::U_RFPOST] / 256> stn{{&jb1}, swin(W8::WB1)};
                    mma_panel<1, 1, K2, PDK>(acc, [&](int, int ks) { return hla[4 * ks]; }, [&](int, int ks) -> float { return wf[ks * 64]; }, stn);
                    stn.commit();
                }
                if (k + 1 < S::KB) {
#pragma unroll
                    for (int q = 0; q < HPT; ++q) Hs[hs_off[q]] = hpre[q];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[0][0][r] + xr[r];
                    xr[r] = v;
                    stX[r * LDX] = v;
                }
            }
            __syncthreads();
            if (k == 0) FE_CLK(26);
            dbg_dump<S, NTH>(a, b, 5 + S::NL + 2 * k, Xb, LDX);
        }

        FE_CLK(7);
        // =========================== rf_post (a13) ===========================
        {
            // Y2[f1][c2] = sum_f2 Wp[f1][f2] X[f2][c2]      (A = packed filterbank rows of tile ws, B = LDS tokens)
            constexpr int KS = F2 / 4;
            FE8_BEGIN_UNIT(S::U_RFPOST);
            conv8_pair<S, W8::N2A, W8::N2B, KS, C2, LDX, false>(
                wh, [&](int ks) -> float { return wl_[o.rfpost_lin - ub_ + (ws * KS + ks) * 64]; },
                [&](int j, int ks) { return Xb[(4 * ks + lg) * LDX + 16 * j + li]; },
                [&](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }, stage, lds_ptr(Y2 + (16 * ws + 4 * lg) * LDX + li), lane);
        }
        __syncthreads();
        // rf_post's 1x1 conv is folded into decoder layer 0's 1x1 on the host (fe_api.hip::pack_weights): that layer reads Y2 as its
        // first K-segment.  Wy (= W0) takes the 1x1 outputs, Wx (= W1, whose first rows Y2 occupies until layer 0 has consumed it)
        // the k = 3 outputs.
        float* const Wx = W1;
        float* const Wy = W0;
        for (int i = tid; i < 2 * LDC; i += NTH) {                // Wy lay under the token arena: zero its halo rows 0 and F1 + 1
            const int r = i / LDC, c = i - r * LDC;
            Wy[(r ? F1 + 1 : 0) * LDC + c] = 0.0f;
        }
        if (a.dbg != nullptr) {                                   // the rf_post stage no longer exists: recompute it for the dump
            float* dst = a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(4 + S::NL + 2 * S::KB);
            for (int i = tid; i < F1 * C1; i += NTH) {
                const int f = i / C1, n = i - f * C1;
                float v = wp[o.rfpost_b + n];
                for (int kk = 0; kk < C2; ++kk) v += Y2[f * LDX + kk] * wp[o.rfpost_w + n * C2 + kk];
                dst[i] = v;
            }
        }

        FE_CLK(8);
        // =========================== decoder (a14) ===========================
        static_for<S::NL>([&](auto l_) {
            constexpr int l = decltype(l_)::value;
            const float* skip = Ebuf + (S::NL - l) * S::ACT;
            {
                // 1x1 conv on cat([x, skip]): two K-segments, never materialised
                FE8_BEGIN_UNIT(S::U_DEC + l * 2);
                constexpr bool FOLD0 = (l == 0);
                constexpr int K0 = FOLD0 ? S::KS_2 : S::KS_C;
                const float* xa = FOLD0 ? Y2 + (16 * ws + li) * LDX + lg : Wx + (16 * ws + li + 1) * LDC + lg;
                const float* sk = skip + (16 * ws + li + 1) * LDC + lg;
                conv8_pair<S, W8::NTA, W8::NTB, K0 + S::KS_C, C1, LDC, true>(
                    wh, [&](int ks) { return ks < K0 ? xa[4 * ks] : sk[4 * (ks - K0)]; },
                    [&](int j, int ks) -> float { return wl_[o.dec1_w[l] - ub_ + (j * (K0 + S::KS_C) + ks) * 64]; },
                    [&](int j) { return lds_v4(wq_ + (o.dec1_b[l] - ub_ + j * 64)); }, stage, stC + (L::W0 + LDC), lane, ap);
            }
            __syncthreads();
            {
                FE8_BEGIN_UNIT(S::U_DEC + l * 2 + 1);
                const float* const t0 = Wy + (16 * ws + li) * LDC + lg;
                conv8_pair<S, W8::NTA, W8::NTB, 3 * S::KS_C, C1, LDC, true>(
                    wh, [&](int ks) { return t0[(ks / S::KS_C) * LDC + 4 * (ks % S::KS_C)]; },
                    [&](int j, int ks) -> float { return wl_[o.dec3_w[l] - ub_ + (j * (3 * S::KS_C) + ks) * 64]; },
                    [&](int j) { return lds_v4(wq_ + (o.dec3_b[l] - ub_ + j * 64)); }, stage, stC + (L::W1 + LDC), lane, ap);
            }
            __syncthreads();
            dbg_dump<S, NTH>(a, b, 5 + S::NL + 2 * S::KB + l, Wx + LDC, LDC);
        });

        FE_CLK(9);
        // =========================== dec_post (a15) ===========================
        float* PT = smem + L::PT;
        typename Dft<S>::InvConst idc;
        float mb0 = 0.0f, mb1 = 0.0f;                  // the mask's two biases
        if constexpr (STRM) { if (a.min_gain != nullptr) ctl.graw = a.min_gain[sb]; }     // (the suppression limit, in flight across dec_post)
        {
            FE8_BEGIN_UNIT(S::U_POST);
            const float* xa = Wx + (16 * ws + li + 1) * LDC + lg;
            const float* sk = Ebuf + (16 * ws + li + 1) * LDC + lg;
            conv8_pair<S, W8::NTA, W8::NTB, 2 * S::KS_C, C1, LDC, true>(
                wh, [&](int ks) { return ks < S::KS_C ? xa[4 * ks] : sk[4 * (ks - S::KS_C)]; },
                [&](int j, int ks) -> float { return wl_[o.post1_w - ub_ + (j * (2 * S::KS_C) + ks) * 64]; },
                [&](int j) { return lds_v4(wq_ + (o.post1_b - ub_ + j * 64)); }, stage, stC + (L::W0 + LDC), lane, ap);
        }
        __syncthreads();
        {
            // transposed conv as a GEMM: P[i][co * 8 + j] = sum_ci x[i][ci] w[ci][co][j]   (one channel tile: the wh = 0 waves)
            FE8_BEGIN_UNIT(S::U_POST + 1);
            const float* xa = Wy + (16 * ws + li + 1) * LDC + lg;
            conv8_pair<S, 1, 0, S::KS_C, 16, S::LDP, false>(
                wh, [&](int ks) { return xa[4 * ks]; }, [&](int j, int ks) -> float { return wl_[o.post_t_w - ub_ + (j * S::KS_C + ks) * 64]; },
                [&](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }, stage, lds_ptr(PT + (16 * ws + 4 * lg) * S::LDP + li), lane);
            if (wave < 4) Dft<S>::load(idc, wb, o, wave);         // iSTFT constants, in flight during the mask phase
            mb0 = wb.scalar(o.post_t_b);
            mb1 = wb.scalar(o.post_t_b + 1);
        }
        __syncthreads();

        FE_CLK(10);
        // =========================== mask, un-compress (a16, a17) ===========================
        {
            const float b0 = mb0, b1 = mb1;
            for (int f = tid; f < F0; f += NTH) {
                const int q = f + 2, j1 = q & 3, i1 = q >> 2;
                float m0 = b0, m1 = b1;
                if (i1 < F1) { m0 += PT[i1 * S::LDP + j1]; m1 += PT[i1 * S::LDP + 8 + j1]; }
                if (i1 >= 1) { m0 += PT[(i1 - 1) * S::LDP + j1 + 4]; m1 += PT[(i1 - 1) * S::LDP + 8 + j1 + 4]; }
                if constexpr (S::EPM != kMaskNone) { m0 = mask_f<S::EPM>(m0); m1 = mask_f<S::EPM>(m1); }
                const float xr_ = sc[2 + f], xi_ = sc[S::LDS_S + 2 + f];
                float yr = xr_ * m0 - xi_ * m1;
                float yi = xr_ * m1 + xi_ * m0;
                if (a.dbg) {
                    float* dst = a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(5 + 2 * S::NL + 2 * S::KB);
                    dst[2 * f] = m0; dst[2 * f + 1] = m1;
                }
                const float mag = sqrtf(yr * yr + yi * yi);
                const float g = pow_f(mag, 1.0f / a.compression - 1.0f);
                yr *= g; yi *= g;
                if (a.dbg) {
                    float* dst = a.dbg + (size_t)b * a.dbg_stride + DebugLayout<S>::offset(6 + 2 * S::NL + 2 * S::KB);
                    dst[2 * f] = yr; dst[2 * f + 1] = yi;
                    if (f == 0) { dst[2 * F0] = 0.0f; dst[2 * F0 + 1] = 0.0f; }
                }
                q3[f] = yr;
                q3[N / 2 + f] = yi;
            }
            // (STRM) the suppression limit: a stream that has one does its bins again with the lifted mask, each thread over the values it has
            // just written, through one wave-uniform branch.  The loop above stays as every other instantiation compiles it, contraction for
            // contraction, so a stream without a limit keeps the bits of fe_step_slots.
            if constexpr (STRM) {
                static_assert(!DBG, "the second pass writes the iSTFT's input only: no debug dump");
                if (a.min_gain != nullptr) ctl.m_min = stream_mask_floor(ctl.graw, a.compression);
                if (ctl.m_min > 0.0f) {
                    const float e = 1.0f / a.compression - 1.0f;
                    for (int f = tid; f < F0; f += NTH) {
                        float yr, yi;
                        limited_bin<S>(PT, sc, f, b0, b1, ctl.m_min, e, yr, yi);
                        q3[f] = yr;
                        q3[N / 2 + f] = yi;
                    }
                }
            }
        }
        __syncthreads();

        FE_CLK(11);
        // =========================== iSTFT (a18) ===========================
        {
            // synthesis window w / sum_k w^2 and the overlap tail: fetched across the inverse DFT
            const float ow = wp[o.window_istft + tid];
            const float oc = tid < OVL ? cis[tid] : 0.0f;
            if (wave < 4) Dft<S>::template inverse<WSrc<true>, false>(q3, q0, q1, tw, idc, wb, o, wave, lane);
            __syncthreads();
            FE_CLK(12);
            const int pi = Dft<S>::pidx(tid & (Dft<S>::N1 - 1), tid / Dft<S>::N1);
            const float xo = (q0[pi] + q1[pi]) * ow + oc;
            // one sample per thread: the first H go out, the rest is the new overlap tail (the old tail was read before the barrier)
            if constexpr (STRM) {
                // the meters' output side: the H samples that go out, as floats; then the waves' partials meet in the transposed-conv buffer,
                // idle since the mask phase
                if (a.levels != nullptr) {
                    if (64 * wave < H) {
                        const float x = tid < H ? xo : 0.0f;
                        ctl.lv.out_ss = wave_sum(0.0f, x * x);
                        ctl.lv.out_pk = wave_max(0.0f, fabsf(x));
                    }
                    levels_put(PT, ctl.lv, wave, lane);
                }
                if (a.format) {
                    // int16 PCM: even lanes pack two samples, lane 8j gathers the four words of lanes 8j, 8j + 2, 8j + 4, 8j + 6 (every lane shuffles)
                    const int qv = pcm16_out(xo);
                    const int pw = pcm16_pair(qv, __shfl_down(qv, 1));
                    const int p1 = __shfl_down(pw, 2), p2 = __shfl_down(pw, 4), p3 = __shfl_down(pw, 6);
                    short* orow = reinterpret_cast<short*>(a.wav_out) + sv.out_off;
                    if (tid < H) {
                        if (H % 8 == 0 && (reinterpret_cast<size_t>(orow) & 15) == 0) {
                            if ((tid & 7) == 0) __builtin_nontemporal_store(i32x4{pw, p1, p2, p3}, reinterpret_cast<i32x4*>(orow + tid));
                        } else {
                            __builtin_nontemporal_store((short)qv, orow + tid);
                        }
                    }
                } else {
                    const float x1 = __shfl_down(xo, 1), x2 = __shfl_down(xo, 2), x3 = __shfl_down(xo, 3);
                    float* orow = a.wav_out + sv.out_off;
                    if (tid < H) {
                        if (H % 4 == 0 && (reinterpret_cast<size_t>(orow) & 15) == 0) {
                            if ((tid & 3) == 0) __builtin_nontemporal_store(f32x4{xo, x1, x2, x3}, reinterpret_cast<f32x4*>(orow + tid));
                        } else {
                            __builtin_nontemporal_store(xo, orow + tid);
                        }
                    }
                }
                if (tid >= H) cis[tid - H] = xo;
            } else
            if constexpr (HIO) {
                // whole 16-byte pieces to host memory: lane 4j gathers the samples of lanes 4j + 1 .. 4j + 3 (every lane of the wave shuffles)
                const float x1 = __shfl_down(xo, 1), x2 = __shfl_down(xo, 2), x3 = __shfl_down(xo, 3);
                float* orow = a.wav_out + (size_t)b * a.out_stride;
                if (tid < H) {
                    if (H % 4 == 0 && (reinterpret_cast<size_t>(orow) & 15) == 0) {
                        if ((tid & 3) == 0) __builtin_nontemporal_store(f32x4{xo, x1, x2, x3}, reinterpret_cast<f32x4*>(orow + tid));
                    } else {
                        __builtin_nontemporal_store(xo, orow + tid);
                    }
                }
                else cis[tid - H] = xo;
            } else {
            if (tid < H) a.wav_out[(size_t)b * a.out_stride + tid] = xo;
            else cis[tid - H] = xo;
            }
            if constexpr (W8::HSTASH) {       // the frame's new GRU states: [KB][B][F2 * C2], 16 bytes per thread and store
                constexpr int N4 = F2 * C2 / 4;
                static_assert((F2 * C2) % 4 == 0 && W8::HST % 4 == 0, "16-byte state rows");
                const f32x4* hst = reinterpret_cast<const f32x4*>(smem + W8::HST);
#pragma unroll
                for (int k = 0; k < S::KB; ++k) {
                    f32x4* dst = reinterpret_cast<f32x4*>(a.h + ((size_t)k * nst + sb) * (F2 * C2));
                    for (int e = tid; e < N4; e += NTH) dst[e] = hst[k * N4 + e];
                }
            }
            if constexpr (PERSIST) __syncthreads();               // (the next stream's frame load reuses q0)
            else if constexpr (STRM) { if (a.levels != nullptr) __syncthreads(); }      // (one stream per workgroup: a barrier for the meters alone)
            if constexpr (STRM) { if (a.levels != nullptr && tid0 == 0) levels_store<kWaves8>(a.levels + sb, PT); }
        }
        FE_CLK(13);
        b += (int)gridDim.x;
        ++fc;
    } while (PERSIST && b < a.B);
#undef FE8_BEGIN_UNIT
    FE_CLK(63);
}

}  // namespace fe
