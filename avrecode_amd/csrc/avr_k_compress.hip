// parallel slice kernel, MODE_COMPRESS, the reference's arithmetic_code<uint64_t, uint8_t> coder (one
// translation unit per kernel: see avr_walker.h).
#include "avr_prof.h"
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_parallel_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                    uint8_t* out, avr_slice_result* res, uint16_t* est, const int* order, uint32_t flags, hipStream_t stream, uint32_t* qhead, int qgrid, int qgrid_fld, size_t lds_fld, const FieldLane* lane) {
#ifdef AVR_PROFILE   // the section counters are this unit's: a profiled build keeps every kernel here
  return launch_parallel<MODE_COMPRESS, false>(T, descs, n, lds, in, out, res, est, order, flags, stream, QueueLaunch{qhead, qgrid, qgrid_fld, lds_fld, lane});
#else
  if (qhead) return launch_queue_compress(T, descs, n, lds, in, out, res, est, order, flags, stream, qhead, qgrid, qgrid_fld, lds_fld, lane);
  return launch_parallel<MODE_COMPRESS, false, kLaunchResident>(T, descs, n, lds, in, out, res, est, order, flags, stream, QueueLaunch{nullptr, qgrid, qgrid_fld, lds_fld, lane});
#endif
}

// AVR_PROFILE builds: read (and clear) this kernel's section cycle counters; zeros otherwise.
hipError_t profile_parallel_compress(unsigned long long* out16) { return read_clear_prof(AVR_PROF_SYM, out16); }

// AVR_PROFILE builds: per-slice wave placement (see avr_place); zeros otherwise.
hipError_t placement_parallel_compress(uint32_t* out, int n) { return read_placement(AVR_PLACE_SYM, out, n); }

}  // namespace avr
