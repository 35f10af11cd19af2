// persistent queue kernels, MODE_COMPRESS, the reference's arithmetic_code<uint64_t, uint8_t> coder: a
// unit of their own (its own CU board, reset by its launch), because the layout hints (avr_engine.h)
// are off here -- with them the persistent compress kernel has one VGPR spill and 16 B of scratch
// more than without.  The resident kernels are in avr_k_compress.hip.
#define AVR_NO_LAYOUT_HINTS
#include "avr_prof.h"
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_queue_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                    uint8_t* out, avr_slice_result* res, uint16_t* est, const int* order, uint32_t flags, hipStream_t stream, uint32_t* qhead, int qgrid, int qgrid_fld, size_t lds_fld, const FieldLane* lane) {
  return launch_parallel<MODE_COMPRESS, false, kLaunchQueue>(T, descs, n, lds, in, out, res, est, order, flags, stream, QueueLaunch{qhead, qgrid, qgrid_fld, lds_fld, lane});
}

}  // namespace avr
