// fe_launch.h — the one host-side way to enqueue a kernel: opt in to its dynamic LDS once per (kernel, device), name it for
// fe_last_step_kernel, launch, report the error.  Every launcher of the library (fe_impl.h, tb_kernels.hip.h, the BSRNN / FSPEN /
// LiSenNet headers) goes through it; kernels without dynamic LDS need no opt-in and are launched where they stand.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace fe {

constexpr int kMaxDevices = 64;

// fe_last_step_kernel (C ABI, r6): every host-side launcher names the kernel it enqueues (a string literal: family + instantiation);
// the compute entry points of fe_api.hip collect the names of one call in the handle.  Defined in fe_api.hip (thread-local log).
void note_kernel(const char* name);

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
template <auto Kern, class Args>
hipError_t launch(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args& a) {
    const hipError_t e = lds_opt_in<Kern>(lds_bytes);
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
    hipError_t e = lds_opt_in<Kern>(lds_bytes);
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
