// fe_resample.hip - the translation unit of the polyphase resampler's kernels (resample_kernels.hip.h): the instantiations of
// fe_resample_kernel - whole, streams and ring, each as it was and once more for calls with a G.711 format - and their launchers.  The host
// side - filter design, argument checks - is fe_api_resample.inc in the C-ABI unit.
#include "resample_kernels.hip.h"

namespace fe {

template <bool STRM, bool G711>
static hipError_t launch_resample_form(dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleArgs& a) {
    const hipError_t e = lds_opt_in<fe_resample_kernel<STRM, false, G711>>(160 * 1024);
    if (e != hipSuccess) return e;
    return launch<fe_resample_kernel<STRM, false, G711>>(nullptr, grid, dim3(kResampleThreads), lds_bytes, st, a);      // (the handle names the kernel: fe_resampler_last_kernel)
}

hipError_t launch_resample(bool strm, bool g711, dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleArgs& a) {
    if (g711) return strm ? launch_resample_form<true, true>(grid, lds_bytes, st, a) : launch_resample_form<false, true>(grid, lds_bytes, st, a);
    return strm ? launch_resample_form<true, false>(grid, lds_bytes, st, a) : launch_resample_form<false, false>(grid, lds_bytes, st, a);
}

template <bool G711>
static hipError_t launch_resample_ring_form(dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleRingArgs& a) {
    const hipError_t e = lds_opt_in<fe_resample_kernel<true, true, G711>>(160 * 1024);
    if (e != hipSuccess) return e;
    return launch<fe_resample_kernel<true, true, G711>>(nullptr, grid, dim3(kResampleThreads), lds_bytes, st, a);
}

hipError_t launch_resample_rings(bool g711, dim3 grid, size_t lds_bytes, hipStream_t st, const ResampleRingArgs& a) {
    return g711 ? launch_resample_ring_form<true>(grid, lds_bytes, st, a) : launch_resample_ring_form<false>(grid, lds_bytes, st, a);
}

}  // namespace fe
