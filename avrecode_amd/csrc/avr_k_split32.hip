// The long-slice split's kernels on the P32 coder (avr_slice_kernels.h slices_split_kernel<MODE, true>;
// avr_engine.h PEncoder / PDecoder, tags avrecode-amd:P32S / P32SE): compress (whole slices, cut as
// they are walked) and decompress (the pieces), in a translation unit of their own with its own CU
// board, as avr_k_compress32.hip / avr_k_decompress32.hip are.  launch_split (avr_k_split.hip) sizes
// the launch and comes here when the flags carry kFlagP32.
// The layout hints (avr_engine.h) stay on, as in avr_k_split.hip: both kernels of this unit fit
// __launch_bounds__(192, 4) either way with the same VGPR spills and scratch (7 / 32 B compress, 0 /
// 0 B decompress), and without the hints they spill more SGPRs (180 / 412 against 174 / 330).
#include "avr_slice_kernels.h"

namespace avr {

hipError_t launch_split32(int mode, const EngineTables* T, const avr_slice_desc* descs, int n, int grid, size_t lds,
                          const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est, const SplitArgs& sp,
                          uint32_t flags, hipStream_t stream) {
  if (hipError_t e = reset_cu_board(stream); e != hipSuccess) return e;
  if (mode == MODE_COMPRESS)
    hipLaunchKernelGGL((slices_split_kernel<MODE_COMPRESS, true>), dim3(grid), dim3(slice_threads<MODE_COMPRESS>()), lds,
                       stream, T, descs, n, in, out, res, est, sp, flags);
  else
    hipLaunchKernelGGL((slices_split_kernel<MODE_DECOMPRESS, true>), dim3(grid), dim3(slice_threads<MODE_DECOMPRESS>()),
                       lds, stream, T, descs, n, in, out, res, est, sp, flags);
  return hipGetLastError();
}

}  // namespace avr
