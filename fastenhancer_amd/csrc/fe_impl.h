// fe_impl.h — per-shape dispatch record shared by fe_api.hip and the per-shape translation units
// (one fe_shape_<name>.hip per compiled shape, so that the shapes build in parallel).  Every launch of a shape's frame kernels goes through one
// pointer of the record - Impl::launch_step: flavour -> launch_impl<S, SLOT, HIO, STRM> - but the cooperative time-pipelined one (launch_pipe).
#pragma once
#include <hip/hip_runtime.h>

#include "fe_kernels.hip.h"
#include "fe_frame8.hip.h"
#include "tb_kernels.hip.h"

namespace fe {

struct Impl {
    int C1, NL, C2, F2, KB, NFFT, HOP, KT, LOW, FR, TA, LN, BD;
    const tb::TbImpl* tb;   // time-batched engine (tb_kernels.hip.h) or nullptr
    size_t lds_bytes;
    int occ;              // resident workgroups per CU
    bool many_persist;    // companion: also used beyond occ x #CUs streams (persistent workgroups)
    bool wg8;             // the 512-thread per-hop kernel (fe_frame8.hip.h) is built for this shape
    int n_units, u_max;
    bool staged;
    size_t skip_floats;   // per stream, 0 when the skips stay in LDS
    size_t dbg_floats;
    int dbg_stages;
    const PackedOffsets* off;
    // every launch of the frame kernels but the time-pipelined one: launch_impl's choice for a.B streams, made with the flavour's instantiations,
    // which take the prefix of the argument block they were compiled for; nullptr without a frame kernel (the noncausal shapes)
    void (*launch_step)(const StreamFrameArgs&, StepFlavour, int max_wgs, hipStream_t, hipError_t*);
    void (*launch_pipe)(const FrameArgs&, hipStream_t, hipError_t*);     // time-pipelined offline / spec launch (a.pipe_p workgroups per stream)
    void (*dbg_stage)(int, int*, int*, size_t*);
    const char* name = nullptr;      // the line of fe_shapes.def this record was compiled from (fe_shape.hip.in): part of fe_last_step_kernel's answer
    bool many_one_round = true;      // companion: used from the first stream above the shape's own plan (false: only beyond occ x #CUs streams, as persistent workgroups)
    int EP = 0;                      // Shape::EP: activation + 8 * mask (FE_ACT_* / FE_MASK_*); 0 = SiLU, no mask function
    // the packet step's time-pipelined launch (fe_step_streams_chunk: a.pipe_p workgroups per call stream; cooperative, a refusal leaves no
    // error behind and notes no kernel); nullptr for the shapes it is not built for (TATT, KT > 1, BIDIR, the low-LDS companions)
    hipError_t (*launch_streams_pipe)(const StreamFrameArgs&, hipStream_t) = nullptr;
};

// The texts of the frame kernels (kernel_names, fe_launch.h).  HIO says where a slotted step's audio lives; for the STRM instantiations that, the
// audio's format and a bank table are run-time facts of the call: s[pinned + 2 * s16 + 4 * banks].
static_assert(same_text(kernel_names("fe_frame8_kernel", 0, "", "").s[0], "fe_frame8_kernel") &&
              same_text(kernel_names("fe_frame8_kernel", 0, "persistent", "slots").s[1], "fe_frame8_kernel<persistent, slots, pinned>") &&
              same_text(kernel_names("fe_frame_kernel", 2, "per-hop, persistent", "streams").s[3], "fe_frame_kernel<LOW=2, per-hop, persistent, streams, pinned, s16>") &&
              same_text(kernel_names("fe_frame_kernel", 2, "per-hop, persistent", "streams").s[7], "fe_frame_kernel<LOW=2, per-hop, persistent, streams, pinned, s16, banks>"),
              "the texts fe_last_step_kernel has always reported, and the banked call's (the last one is the longest: 72 characters)");
template <bool WG8, int LOW, bool DBG, bool T1, bool PERSIST, bool SLOT, bool HIO, bool STRM, class Args>
const char* kernel_name_of(const Args& a) {      // WG8: fe_frame8_kernel (no LOW shapes, no generic form), else fe_frame_kernel
    static constexpr KernelNames names = kernel_names(WG8 ? "fe_frame8_kernel" : "fe_frame_kernel", LOW,
        DBG ? "debug" : WG8 ? (PERSIST ? "persistent" : "") : !T1 ? "generic" : PERSIST ? "per-hop, persistent" : "per-hop", STRM ? "streams" : SLOT ? "slots" : "");
    if constexpr (STRM) return names.s[(a.pinned != 0) + 2 * (a.format != 0) + 4 * (a.bank != nullptr)];
    else return names.s[HIO];
}

// (STRM: a call with a bank table runs the BANK instantiation of the same choice - a.bank decides here, per launch)
template <class S, bool DBG, int MODE, bool T1, bool PERSIST, bool SLOT = false, bool HIO = false, bool STRM = false>
void launch_one(const typename KernelArgs<SLOT, STRM>::type& a, int grid_x, hipStream_t st, hipError_t* err) {
    const char* name = kernel_name_of<false, S::LOW, DBG, T1, PERSIST, SLOT, HIO, STRM>(a);
    if constexpr (STRM) {
        if (a.bank != nullptr) {
            *err = launch<&fe_frame_kernel<S, DBG, MODE, T1, PERSIST, false, SLOT, HIO, STRM, true>>(name, dim3(grid_x), dim3(kThreads), Lds<S>::BYTES, st, a);
            return;
        }
    }
    *err = launch<&fe_frame_kernel<S, DBG, MODE, T1, PERSIST, false, SLOT, HIO, STRM>>(name, dim3(grid_x), dim3(kThreads), Lds<S>::BYTES, st, a);
}

// a.step_kernel (fe_set_step_kernel; the handle's default comes from the environment variable FE_WG8, else 1):
//   0 = the four-wave kernel everywhere; 1 = the 512-thread kernel (fe_frame8.hip.h: two waves per SIMD, channel-grouped GRU gates)
//   for the per-hop step of the shapes it is built for, up to one stream per CU; 2 = also above that (persistent workgroups)
template <class S, bool DBG, bool PERSIST, bool SLOT = false, bool HIO = false, bool STRM = false>
void launch_one8(const typename KernelArgs<SLOT, STRM>::type& a, int grid_x, hipStream_t st, hipError_t* err) {
    const char* name = kernel_name_of<true, 0, DBG, true, PERSIST, SLOT, HIO, STRM>(a);
    if constexpr (STRM) {
        if (a.bank != nullptr) {
            *err = launch<&fe_frame8_kernel<S, DBG, PERSIST, SLOT, HIO, STRM, true>>(name, dim3(grid_x), dim3(kThreads8), Wg8<S>::BYTES, st, a);
            return;
        }
    }
    *err = launch<&fe_frame8_kernel<S, DBG, PERSIST, SLOT, HIO, STRM>>(name, dim3(grid_x), dim3(kThreads8), Wg8<S>::BYTES, st, a);
}

// max_wgs: workgroups that are resident at once (one per CU: 129+ KiB of LDS and waves_per_eu(1,1)); a batch with more
// streams runs on a grid of max_wgs PERSISTENT workgroups, each walking its streams b, b + grid, ...
// SLOT (fe_step_slots): the same choice, made with the slotted instantiations (streaming mode; no debug dumps or cycle probes)
// HIO (fe_step_slots_pinned; SLOT only): ... with the instantiations that read and write the audio in page-locked host memory
// STRM (fe_step_streams / fe_step_streams_pinned; HIO only): ... with the packet-audio instantiations (a.T = T_max picks per-hop or generic)
template <class S, bool SLOT = false, bool HIO = false, bool STRM = false>
void launch_impl(const typename KernelArgs<SLOT, STRM>::type& a, int max_wgs, hipStream_t st, hipError_t* err) {
    static_assert(SLOT || !HIO, "host audio: slotted instantiations only");
    static_assert(HIO || !STRM, "packet audio: the host-audio instantiations only");
    // the choice: debug instantiation (fe_debug_step / fe_profile_step; never slotted), per-hop or generic kernel, 512-thread or four-wave, grid
#ifdef FE_PROBE_HOT
    const bool dbg = !SLOT && a.dbg != nullptr;
#else
    const bool dbg = !SLOT && (a.dbg != nullptr || a.clk != nullptr);
#endif
    const bool per_hop = a.mode == FE_MODE_STREAM && a.T == 1;       // (the slotted steps are always streaming steps)
    const int resident = max_wgs * Lds<S>::OCC;
    int grid = a.B < resident ? a.B : resident;
    if constexpr (Wg8<S>::OK) {
        // one 512-thread workgroup per CU; more streams than that: persistent workgroups at step_kernel 2 (no debug form), else the four-wave kernel
        if (a.step_kernel > 0 && per_hop && (a.B <= max_wgs || (a.step_kernel > 1 && !dbg))) {
            if constexpr (!SLOT)
                if (dbg) return launch_one8<S, true, false>(a, a.B, st, err);
            if (a.B <= max_wgs) return launch_one8<S, false, false, SLOT, HIO, STRM>(a, a.B, st, err);
            return launch_one8<S, false, true, SLOT, HIO, STRM>(a, max_wgs, st, err);
        }
    }
    if constexpr (!SLOT)
        if (dbg) return launch_one<S, true, -1, false, true>(a, grid, st, err);
    if (per_hop) {                                                                       // the per-hop hot path
        if (grid == a.B) return launch_one<S, false, FE_MODE_STREAM, true, false, SLOT, HIO, STRM>(a, grid, st, err);
        return launch_one<S, false, FE_MODE_STREAM, true, true, SLOT, HIO, STRM>(a, grid, st, err);
    }
    launch_one<S, false, -1, false, true, SLOT, HIO, STRM>(a, grid, st, err);                    // chunked streaming, fe_spec_step, fe_offline
}

template <class S>
void launch_step_impl(const StreamFrameArgs& a, StepFlavour flavour, int max_wgs, hipStream_t st, hipError_t* err) {
    switch (flavour) {       // (each instantiation's launcher binds the prefix of a that is its kernels' argument block)
    case STEP_PLAIN: return launch_impl<S>(a, max_wgs, st, err);
    case STEP_SLOTS: return launch_impl<S, true>(a, max_wgs, st, err);
    case STEP_SLOTS_PINNED: return launch_impl<S, true, true>(a, max_wgs, st, err);
    case STEP_STREAMS: return launch_impl<S, true, true, true>(a, max_wgs, st, err);
    }
}

// Time-pipelined launch: B * pipe_p workgroups that wait on each other inside the kernel - a cooperative launch, so
// that the runtime guarantees (or refuses) their co-residency instead of a spin-wait deadlock.
template <class S>
void launch_pipe_impl(const FrameArgs& a, hipStream_t st, hipError_t* err) {
    // (one instantiation, the mode a run-time fact: fe_step_chunk's launch is named apart)
    const char* name = a.mode == FE_MODE_STREAM ? "fe_frame_kernel<time-pipelined, streaming>" : "fe_frame_kernel<time-pipelined>";
    *err = launch_coop<&fe_frame_kernel<S, false, -1, false, true, true>>(name, dim3(a.B * a.pipe_p), dim3(kThreads), Lds<S>::BYTES, st, a);
}

// The packet step on the time pipeline (PIPE + SLOT + STRM; the BANK instantiation for a call with a bank table, as launch_one chooses).  The
// name is the packet step's with "time-pipelined" for what it is: fe_frame_kernel<time-pipelined, streams[, pinned][, s16][, banks]>.
template <class S>
hipError_t launch_streams_pipe_impl(const StreamFrameArgs& a, hipStream_t st) {
    static constexpr KernelNames names = kernel_names("fe_frame_kernel", S::LOW, "time-pipelined", "streams");
    const char* name = names.s[(a.pinned != 0) + 2 * (a.format != 0) + 4 * (a.bank != nullptr)];
    const dim3 grid(a.B * a.pipe_p), block(kThreads);
    if (a.bank != nullptr)
        return launch_coop<&fe_frame_kernel<S, false, FE_MODE_STREAM, false, true, true, true, false, true, true>, true>(name, grid, block, Lds<S>::BYTES, st, a);
    return launch_coop<&fe_frame_kernel<S, false, FE_MODE_STREAM, false, true, true, true, false, true, false>, true>(name, grid, block, Lds<S>::BYTES, st, a);
}

template <class S>
void dbg_stage_impl(int s, int* rows, int* cols, size_t* off) {
    *rows = DebugLayout<S>::rows(s);
    *cols = DebugLayout<S>::cols(s);
    *off = DebugLayout<S>::offset(s);
}

template <class S>
Impl make_impl() {
    const tb::TbImpl* tbp = nullptr;
    if constexpr (S::TB) {
        static const tb::TbImpl tbi = tb::make_tb_impl<S>();
        tbp = &tbi;
    }
    if constexpr (S::BIDIR) {       // noncausal: no frame-by-frame kernel (the reverse-time scan needs all frames): time-batched engine only
        Impl im{S::C1, S::NL, S::C2, S::F2, S::KB, S::NFFT, S::HOP, S::KT, S::LOW, 0, 0, 0, 1, tbp, (size_t)0, 1, false, false, S::NU, Pack<S>::umax(), false,
                (size_t)0, DebugLayout<S>::total(), DebugLayout<S>::n_stages, &Pack<S>::v, nullptr, nullptr, &dbg_stage_impl<S>};
        im.EP = S::EP;
        return im;
    } else {
    Impl im{S::C1, S::NL, S::C2, S::F2, S::KB, S::NFFT, S::HOP, S::KT, S::LOW, S::FRNN ? 1 : 0, S::LB, S::LN ? 1 : 0, 0, tbp, Lds<S>::BYTES, Lds<S>::OCC, Lds<S>::MANY_PERSIST, Wg8<S>::OK, S::NU, Pack<S>::umax(), Lds<S>::STAGED,
            Lds<S>::SKIPS_LDS ? (size_t)0 : (size_t)(S::NL + 1) * S::F1 * S::C1,
            DebugLayout<S>::total(), DebugLayout<S>::n_stages, &Pack<S>::v, &launch_step_impl<S>, &launch_pipe_impl<S>, &dbg_stage_impl<S>};
    im.many_one_round = Lds<S>::MANY_ONE_ROUND;
    im.EP = S::EP;
    if constexpr (!S::TATT && S::KT == 1 && S::LOW == 0) im.launch_streams_pipe = &launch_streams_pipe_impl<S>;
    return im;
    }
}


}  // namespace fe
