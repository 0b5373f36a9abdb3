// fe_launch.h — the one host-side way to enqueue a model kernel: opt in to its dynamic LDS once per (kernel, device), name it for
// fe_last_step_kernel, launch, report the error; and what the launchers of the four families share - the flavour a streaming step was asked
// for (StepFlavour) and the texts fe_last_step_kernel reports (kernel_names).  Every launcher of fe_impl.h, tb_kernels.hip.h, fe_resample.hip and
// the BSRNN / FSPEN / LiSenNet headers goes through launch / launch_coop.  Launched where they stand, by hand, are only the helper kernels
// around the models: in fe_api.hip istft_ola_kernel, stream_ola_kernel, stream_ola_streams_kernel, zero_counters_kernel, ring_in_kernel,
// ring_out_kernel, state_reset_slots_kernel, poison_lds_kernel and the stand-alone STFT kernels of stft_kernels.hip.h (FE_STFT_LAUNCH); in
// tb_kernels.hip.h tb_scan_kernel / tb_scan4_kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace fe {

constexpr int kMaxDevices = 64;

// fe_last_step_kernel (C ABI, r6): every host-side launcher names the kernel it enqueues (a string literal: family + instantiation);
// the compute entry points of fe_api.hip collect the names of one call in the handle.  Defined in fe_api.hip (thread-local log).
void note_kernel(const char* name);

// How a streaming step was asked for = the instantiations that run it and the prefix of the family's widest argument block (StreamFrameArgs;
// BStreamArgs, FStreamArgs, LStreamArgs) they take as theirs: plain (fe_step, the debug / profile steps, fe_spec_step, fe_offline: XArgs), SLOT
// (fe_step_slots, fe_step_pool: XSlotArgs, a.slots / a.capacity), HIO (FastEnhancer only - fe_step_pinned / fe_step_slots_pinned: wav_in / wav_out
// are device views of page-locked host memory; a baseline family's launcher refuses it) or STRM (fe_step_streams[_pinned],
// fe_step_pool_streams[_pinned]: all of it - a.desc, a.T = T_max; float32 or int16 audio in device or page-locked host memory)
enum StepFlavour { STEP_PLAIN, STEP_SLOTS, STEP_SLOTS_PINNED, STEP_STREAMS };

// What fe_last_step_kernel reports for the instantiation a launcher picked: the kernel's name, then in angle brackets and joined by ", " whichever
// apply of "LOW=n", what it is (debug, per-hop, PART 1, ...), the flavour ("slots"; "streams" for FastEnhancer's STRM instantiations, "slots, streams"
// for the other families'), "pinned", "s16", "banks" and what comes after those (BSRNN: "two workgroups per CU") - put together at compile time, so
// that note_kernel still gets a constant string.  Where a packet step's audio lives, its format and a bank table (fe_step_streams_banked) are
// run-time facts of the call (a.pinned, a.format, a.bank), hence a name for each of the eight: s[pinned + 2 * s16 + 4 * banks].
struct KernelNames { char s[8][96] = {}; };
constexpr KernelNames kernel_names(const char* kernel, int low, const char* what, const char* flavour, const char* after = "") {
    KernelNames n;
    for (int v = 0; v < 8; ++v) {
        const char* parts[] = {low == 2 ? "LOW=2" : low == 1 ? "LOW=1" : "", what, flavour, v & 1 ? "pinned" : "", v & 2 ? "s16" : "", v & 4 ? "banks" : "", after};
        int k = 0;
        auto put = [&](const char* p) { while (*p) n.s[v][k++] = *p++; };
        put(kernel);
        bool open = false;
        for (const char* p : parts)
            if (*p) { put(open ? ", " : "<"); put(p); open = true; }
        if (open) put(">");
    }
    return n;
}
constexpr bool same_text(const char* a, const char* b) { for (; *a == *b; ++a, ++b) if (!*a) return true; return false; }
// the flavour part of a BSRNN / FSPEN / LiSenNet name, and the one of a table's names that a launch of that flavour reports
constexpr const char* baseline_flavour(bool slot, bool strm) { return strm ? "slots, streams" : slot ? "slots" : ""; }
template <bool STRM, class Args>
const char* baseline_name(const KernelNames& names, const Args& a) {
    if constexpr (STRM) return names.s[(a.pinned != 0) + 2 * (a.format != 0)];
    else return names.s[0];
}

// The opt-in for more than 64 KiB of dynamic LDS is a per-device function attribute: set once per kernel and device (an engine may
// live on any GPU of the process; relaxed atomics - setting it twice is harmless; a device index out of range counts as device 0).
// Keyed by the kernel itself, not by its type: kernels of one signature (every tb_*_kernel is a void(TbArgs)) each have their own flags.
template <auto Kern>
hipError_t lds_opt_in(size_t lds_bytes) {
    static std::atomic<bool> done[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    if (done[dev].load(std::memory_order_relaxed)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) done[dev].store(true, std::memory_order_relaxed);
    return e;
}

// name: what fe_last_step_kernel reports, noted before the launch (nullptr: the caller has noted it)
// (a kernel with static LDS only - lds_bytes = 0 - has nothing to opt in to)
template <auto Kern, class Args>
hipError_t launch(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args& a) {
    const hipError_t e = lds_bytes ? lds_opt_in<Kern>(lds_bytes) : hipSuccess;
    if (e != hipSuccess) return e;
    if (name) note_kernel(name);
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, a);
    return hipGetLastError();
}

// Cooperative launch: the workgroups wait on each other inside the kernel, so the runtime guarantees their co-residency or refuses.
// OPTIONAL = the caller has separate launches to fall back on: the kernel is noted only when the launch was accepted, and a refusal
// leaves no sticky error behind.
template <auto Kern, bool OPTIONAL = false, class Args>
hipError_t launch_coop(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args& a) {
    hipError_t e = lds_bytes ? lds_opt_in<Kern>(lds_bytes) : hipSuccess;
    if (e != hipSuccess) return e;
    Args args = a;
    void* kargs[] = {&args};
    if (!OPTIONAL) note_kernel(name);
    e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(Kern), grid, block, kargs, (unsigned int)lds_bytes, st);
    if (OPTIONAL && e == hipSuccess) note_kernel(name);
    if (OPTIONAL && e != hipSuccess) (void)hipGetLastError();
    return e;
}

}  // namespace fe
