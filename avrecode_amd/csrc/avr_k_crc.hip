// avr_crc_spans: the CRC-32 (ISO-HDLC / zlib: reflected 0xEDB88320, init and xorout 0xFFFFFFFF) of a
// batch of byte spans of one device buffer -- the slice payloads of a compress, the regenerated
// slices or packed units of a decompress -- where they lie, so that a checked container
// (Recoded.Metadata field 16, include/avrecode.h) costs the host 4 bytes per span and a fold
// (avr_crc32_combine) instead of a pass over the file.  No reference counterpart (recode.proto has
// no checksum).
//
// The variant built is the chunked one: each thread runs a table CRC over a contiguous chunk and
// the 256 partial values are folded pairwise, crc(AB) = crc(A) x^(8 |B|) + crc(B) in GF(2)[x]/P.  The
// chunks are right-aligned in the span -- thread 255's ends at the span's end, every chunk is C bytes
// and only the first non-empty one is shorter -- so one multiplier x^(8 C 2^level) serves every pair of
// a level: a short or empty operand can only be a left one, and the empty ones are zero (the init
// value goes to the first non-empty chunk alone), which any multiplier leaves zero.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_crc_device.h"   // crc_span
#include "avr_kernels.h"

namespace avr {

// One workgroup per span, as verify_kernel (avr_kernels.hip) and pack_pieces_kernel.
__global__ __launch_bounds__(256) void crc_spans_kernel(const uint8_t* buf, uint64_t buf_len, const uint64_t* off,
                                                        const uint32_t* len, int n, uint32_t* crc, int32_t* status) {
  __shared__ CrcLds s;
  const int k = blockIdx.x;
  if (k >= n) return;
  crc_span(s, buf, buf_len, off[k], len[k], &crc[k], &status[k]);
}

// The spans of a slice batch read from its descriptors: the payloads of a compress batch (regen = 0:
// payload_offset, payload_size), or what a decompress batch regenerated (regen = 1: out_offset,
// res.out_len; a slice that failed keeps its status and gets crc 0).
__global__ __launch_bounds__(256) void crc_slices_kernel(const avr_slice_desc* d, const avr_slice_result* res, int n,
                                                         int regen, const uint8_t* buf, uint64_t buf_len, uint32_t* crc,
                                                         int32_t* status) {
  __shared__ CrcLds s;
  const int k = blockIdx.x;
  if (k >= n) return;
  if (regen && res[k].status != 0) {
    if (threadIdx.x == 0) crc[k] = 0, status[k] = res[k].status;
    return;
  }
  crc_span(s, buf, buf_len, regen ? d[k].out_offset : d[k].payload_offset, regen ? res[k].out_len : d[k].payload_size,
           &crc[k], &status[k]);
}

hipError_t launch_crc_spans(const uint8_t* buf, uint64_t buf_len, const uint64_t* off, const uint32_t* len, int n,
                            uint32_t* crc, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crc_spans_kernel, dim3(n), dim3(256), 0, stream, buf, buf_len, off, len, n, crc, status);
  return hipGetLastError();
}

hipError_t launch_crc_slices(const avr_slice_desc* descs, const avr_slice_result* res, int n, bool regen,
                             const uint8_t* buf, uint64_t buf_len, uint32_t* crc, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crc_slices_kernel, dim3(n), dim3(256), 0, stream, descs, res, n, regen ? 1 : 0, buf, buf_len, crc,
                     status);
  return hipGetLastError();
}

}  // namespace avr
