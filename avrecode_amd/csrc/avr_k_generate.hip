// parallel slice kernel, MODE_GENERATE (one translation unit per kernel: see avr_walker.h).
#include "avr_prof.h"
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_parallel_generate(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                    uint8_t* out, avr_slice_result* res, uint16_t* est, const int* order, uint32_t flags, hipStream_t stream) {
  hipLaunchKernelGGL((slices_parallel_kernel<MODE_GENERATE, false>), dim3(n), dim3(slice_threads<MODE_GENERATE>()), lds, stream, T, descs, n, in, out, res, est, order, flags);
  // field pictures / MBAFF frames: a second launch over the batch (its workgroups for progressive
  // slices return at once)
  if (flags & kFlagFields) {
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL((slices_parallel_kernel<MODE_GENERATE, true>), dim3(n), dim3(slice_threads<MODE_GENERATE>()), lds, stream, T, descs, n, in, out, res, est, order, flags);
  }
  return hipGetLastError();
}

// AVR_PROFILE builds: read (and clear) this kernel's section cycle counters; zeros otherwise.
hipError_t profile_parallel_generate(unsigned long long* out16) { return read_clear_prof(AVR_PROF_SYM, out16); }

}  // namespace avr
