// avr_check_units: the unit check of a range read (include/avrecode.h, ABI 13).  A container written
// with unit checksums carries one CRC-32 per unit -- a whole coded slice, or one piece of a cut one --
// over the unit's share of the slice's payload (Block field 18).  After the units of a window are
// regenerated and the tails have run (avr_k_gather.hip), each selected unit's share is CRC'd where it
// lies, in the unit's output space, the last-byte rule (recode.cpp:1345-1356) goes onto the value
// instead of onto bytes, and the value is compared with the container's: a flipped bit that
// regenerates a slice of the right length with wrong bytes -- which neither the unit's status nor the
// tails' length check can see -- fails the read, and only the reads that touch that unit.
// No reference counterpart (recode.proto has no checksum, and decompressor::run no partial read).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_crc_device.h"   // crc_span
#include "avr_kernels.h"

namespace avr {

// One workgroup per selected unit, after range_tails_kernel on the same stream (stream order is the
// only synchronisation).  Everything that decides whether the workgroup works is uniform over it.
__global__ __launch_bounds__(256) void check_units_kernel(const avr_range_tail* tails, const avr_unit_check* checks,
                                                          const avr_slice_result* res, int n, const uint8_t* src,
                                                          uint64_t src_len, int32_t* status) {
  __shared__ CrcLds s;
  const int k = blockIdx.x;
  if (k >= n) return;
  const avr_unit_check ck = checks[k];
  const avr_slice_result r = res[k];
  if (status[k] != 0 || r.status != 0 || !ck.have) return;   // the status stays as it is
  const avr_range_tail t = tails[k];
  // the unit's share of its slice: a piece that is not the last keeps `keep` bytes even when it
  // regenerated more; a last piece or whole slice all it regenerated, and the rule on top, decided as
  // range_tails_kernel decides it
  uint32_t len = r.out_len;
  int rule = 0;   // 0 keep, 1 replace, 2 append
  if (t.keep != 0xffffffffu) {
    len = t.keep;
  } else if (t.has_rule) {
    const uint64_t total = (uint64_t)t.q_last + r.out_len;
    rule = (uint32_t)(total & 1) != (uint32_t)(t.length_parity & 1) ? 2 : len ? 1 : 0;
  }
  uint32_t crc = 0;
  int32_t st = 0;
  crc_span(s, src, src_len, ck.src_off, len, &crc, &st);   // thread 0 holds the result
  if (threadIdx.x != 0) return;
  if (st != 0) {   // the span does not lie inside src_len: nothing of it was read
    status[k] = st;
    return;
  }
  // the rule on the value, fold_file_crc's arithmetic (avr_host.cpp): two messages of one length that
  // differ in the last byte differ by the raw byte table's entry for the difference; an appended byte
  // goes through the register (the empty message's register is the init value)
  if (rule == 1) {
    crc ^= crc_shift8((uint32_t)(src[ck.src_off + len - 1] ^ t.last_byte));
  } else if (rule == 2) {
    const uint32_t reg = ~crc;
    crc = ~(crc_shift8((reg ^ t.last_byte) & 0xffu) ^ (reg >> 8));
  }
  if (crc != ck.crc) status[k] = AVR_SLICE_CHECKSUM;
}

hipError_t launch_check_units(const avr_range_tail* tails, const avr_unit_check* checks, const avr_slice_result* res,
                              int n, const uint8_t* src, uint64_t src_len, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(check_units_kernel, dim3(n), dim3(256), 0, stream, tails, checks, res, n, src, src_len, status);
  return hipGetLastError();
}

}  // namespace avr
