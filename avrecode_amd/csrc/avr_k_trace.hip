// parallel slice kernel, MODE_TRACE (decode-only bin trace for the hooks layer) (one translation unit per kernel: see avr_walker.h).
// the layout hints (avr_engine.h) are off here: no A/B of this unit's kernels has been run with them
#define AVR_NO_LAYOUT_HINTS
#include "avr_prof.h"
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_parallel_trace(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                    uint8_t* out, avr_slice_result* res, uint16_t* est, const int* order, uint32_t flags, hipStream_t stream) {
  hipLaunchKernelGGL((slices_parallel_kernel<MODE_TRACE, false>), dim3(n), dim3(slice_threads<MODE_TRACE>()), lds, stream, T, descs, n, in, out, res, est, order, flags);
  // field pictures / MBAFF frames: a second launch over the batch (its workgroups for progressive
  // slices return at once)
  if (flags & kFlagFields) {
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL((slices_parallel_kernel<MODE_TRACE, true>), dim3(n), dim3(slice_threads<MODE_TRACE>()), lds, stream, T, descs, n, in, out, res, est, order, flags);
  }
  return hipGetLastError();
}

// AVR_PROFILE builds: read (and clear) this kernel's section cycle counters; zeros otherwise.
hipError_t profile_parallel_trace(unsigned long long* out16) { return read_clear_prof(AVR_PROF_SYM, out16); }

}  // namespace avr
