// fe_resample.hip - the translation unit of the polyphase resampler's kernels (resample_kernels.hip.h): the three instantiations of
// fe_resample_kernel and their launchers.  The host side - filter design, argument checks - is fe_api_resample.inc in the C-ABI unit.
#include "resample_kernels.hip.h"

namespace fe {

template <bool STRM>
static hipError_t launch_resample_form(dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleArgs& a) {
    const hipError_t e = lds_opt_in<fe_resample_kernel<STRM>>(160 * 1024);
    if (e != hipSuccess) return e;
    return launch<fe_resample_kernel<STRM>>(nullptr, grid, dim3(kResampleThreads), lds_bytes, st, a);      // (the handle names the kernel: fe_resampler_last_kernel)
}

hipError_t launch_resample(bool strm, dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleArgs& a) {
    return strm ? launch_resample_form<true>(grid, lds_bytes, st, a) : launch_resample_form<false>(grid, lds_bytes, st, a);
}

hipError_t launch_resample_rings(dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleRingArgs& a) {
    const hipError_t e = lds_opt_in<fe_resample_kernel<true, true>>(160 * 1024);
    if (e != hipSuccess) return e;
    return launch<fe_resample_kernel<true, true>>(nullptr, grid, dim3(kResampleThreads), lds_bytes, st, a);
}

}  // namespace fe
