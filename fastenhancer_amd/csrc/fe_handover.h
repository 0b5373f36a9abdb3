// The hand-over between the workgroups of a time-pipelined launch (the PIPE instantiations of fe_frame_kernel, bsrnn_frame_kernel,
// fspen_frame_kernel and lisennet_frame_kernel), written once.  Device code only; fe_kernels.hip.h includes it.
//
// PIPE (offline / spec -> spec / fe_step_chunk with T >> 1): the frames of ONE stream are spread over P co-resident workgroups (one per
// CU, cooperative launch), workgroup p running frames p, p + P, ...  Everything in a frame but the recurrent state is independent of
// the other frames, so the workgroups run their frames concurrently, staggered by the one true dependency: a site of frame t needs what
// the same site of frame t - 1 left (FastEnhancer: the GRU state of a block, the K / V rings, the time_kernel conv rings; BSRNN: the
// time-LSTM's (h, c) of a layer; FSPEN: a block's inter-GRU states; LiSenNet: nine caches).  The producer publishes it through global
// memory in four steps:
//   1. agent-scope (sc1) stores of the data                                                    st()
//   2. s_waitcnt vmcnt(0) in every thread that stored, then the phase barrier                  drain(), __syncthreads()
//   3. a RELAXED agent-scope store of a per-(stream, site) frame counter, t + 1, by thread 0   signal()
//   4. the consumer polls the counter (relaxed, agent scope) until it reaches t, meets at a
//      barrier, and then fetches the data with agent-scope loads                               wait(), ld()
// INVARIANT: every datum handed from one workgroup to another goes through st() / ld() - a plain load or store added to a ring or state
// would be a silent stale read, served from a stale L1 / L2 line: no release / acquire fence covers it (on this part a fence writes back /
// invalidates whole caches, which is why there is none).  The serial chain is T x (state round trip + one recurrent phase) instead of
// T x (whole frame): ~12 frames in flight for FastEnhancer_B.
// publish() is steps 2 and 3 in one piece.  A site whose drain or barrier is placed by other work - weight loads issued ahead of the
// drain so that one wait covers both, a barrier that is there in some instantiations only - calls drain() and signal() apart with its
// own barrier in between.
// ov_group_barrier (bsrnn_ov_kernels.hip.h) moves its data by steps 1, 2 and 4 as well; its counter arithmetic (fetch-add arrivals) and
// the LDS counters of ov_signal / ov_wait are protocols of their own.
#pragma once

namespace fe {

// Polls of a counter (one relaxed agent-scope load of global memory + s_sleep 1 each) after which wait() gives a producer up and traps
// the launch instead of running on stale state: it bounds how long a lost producer can hold a cooperative launch on the card (BSRNN,
// FSPEN, LiSenNet; FastEnhancer's waits have no bound, see wait_unbounded).  How long
// 2^24 such polls take on this part has not been measured; the one figure on record (2^22 polls in 0.1 - 0.2 s) is of LDS polls without
// a sleep, a different kind of poll.  The limit has to outlast every legitimate wait (a producer that is preempted or takes its first
// page faults), so it errs on the long side.  Reporting the time-out instead of trapping would be an edit of wait() alone.
constexpr int kHandOverSpinLimit = 1 << 24;

// PIPE = false: the same calls in the kernels' other instantiations - plain accesses, no waits, no counters.
// A counter is named by the stream's (or the launch's) counter array and the site's index in it, not by its address: the address is
// formed where it is used, inside the lead thread's branch, as the kernels did when they wrote these steps out.
template <bool PIPE>
struct HandOver {
    static __device__ __forceinline__ float ld(const float* p) {
        if constexpr (PIPE) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else return *p;
    }
    static __device__ __forceinline__ void st(float* p, float v) {
        if constexpr (PIPE) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *p = v;
    }
    // this thread's st() stores have left the CU
    static __device__ __forceinline__ void drain() {
        if constexpr (PIPE) __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0) (gfx9 encoding: lgkmcnt / expcnt left alone)
    }
    // frame t's data of the site are in place: count it.  After drain() and a barrier; all threads call.  (tid: the caller's thread
    // index - a kernel that hides its thread index from the optimiser inside its frame loop tests that copy to keep its code.)
    static __device__ __forceinline__ void signal(unsigned int* flags, int site, int t, int tid = threadIdx.x) {
        if constexpr (PIPE) {
            if (tid == 0) __hip_atomic_store(flags + site, (unsigned int)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    static __device__ __forceinline__ void publish(unsigned int* flags, int site, int t) {
        drain();
        if constexpr (PIPE) __syncthreads();
        signal(flags, site, t);
    }
    // frame t - 1's data of the site are in place (all threads call; the lead thread polls, the barrier holds the others)
    static __device__ __forceinline__ void wait(unsigned int* flags, int site, int t, int tid = threadIdx.x) {
        if constexpr (PIPE) {
            if (t > 0) {
                if (tid == 0) {
                    int spins = 0;
                    while (__hip_atomic_load(flags + site, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)t && ++spins < kHandOverSpinLimit) __builtin_amdgcn_s_sleep(1);
                    if (spins >= kHandOverSpinLimit) __builtin_trap();      // (a producer that never shows up: fail the launch loudly, never run on stale state)
                }
                __syncthreads();
            }
        }
    }
    // wait() without the limit: a lost producer is an endless poll.  FastEnhancer's two waits (a block's state, the time_kernel conv rings)
    // use it: with the spin count in their poll loops the pipelined launches of FastEnhancer_B / T / L and dptransformer B measured
    // 2 - 8 % slower than without, three alternating rounds each (profiles/handover_timing.txt) - the wait is on the serial chain of the
    // pipeline.  A bound for them has to come in a form that costs nothing there.
    static __device__ __forceinline__ void wait_unbounded(unsigned int* flags, int site, int t) {
        if constexpr (PIPE) {
            if (t > 0) {
                if (threadIdx.x == 0) {
                    while (__hip_atomic_load(flags + site, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)t) __builtin_amdgcn_s_sleep(1);
                }
                __syncthreads();
            }
        }
    }
};

}  // namespace fe
