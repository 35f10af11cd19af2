// sequential slice kernel, MODE_COMPRESS (one translation unit per kernel: see avr_walker.h).
// the layout hints (avr_engine.h) are off here: this kernel family's A/B (the reference model's
// whole-file decompress) has not been run with them
#define AVR_NO_LAYOUT_HINTS
#include "avr_prof.h"
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_sequential_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                    uint8_t* out, avr_slice_result* res, uint16_t* est, uint8_t* frames, int* frame_meta,
                    const int* file_first, int n_files, uint64_t frame_stride, uint32_t flags,
                    hipStream_t stream) {
  if (flags & kFlagFields)
    hipLaunchKernelGGL((slices_sequential_kernel<MODE_COMPRESS, true>), dim3(n_files), dim3(slice_threads<MODE_COMPRESS>()), lds, stream, T, descs, n, in, out, res, est,
                     frames, frame_meta, file_first, frame_stride, flags);
  else
    hipLaunchKernelGGL((slices_sequential_kernel<MODE_COMPRESS, false>), dim3(n_files), dim3(slice_threads<MODE_COMPRESS>()), lds, stream, T, descs, n, in, out, res, est,
                     frames, frame_meta, file_first, frame_stride, flags);
  return hipGetLastError();
}

// AVR_PROFILE builds: read (and clear) this kernel's section cycle counters; zeros otherwise.
hipError_t profile_sequential_compress(unsigned long long* out16) { return read_clear_prof(AVR_PROF_SYM, out16); }

}  // namespace avr
