// avr_gather_spans / avr_range_tails: the device side of a range read (include/avrecode.h, ABI 12).
// A window of the file is laid out in its final form from the planner's copy spans (avr_plan.cpp,
// plan_range) -- literal bytes and crops of the regenerated units, both standing in one source
// buffer -- and then every selected unit's result is checked against its tail record, the unit that
// ends a slice applying the last-byte rule (recode.cpp:1345-1356) where the slice's final byte lies
// in the window.  No reference counterpart (decompressor::run regenerates the whole file,
// recode.cpp:1312-1357).  A unit of its own: pack_pieces_kernel (avr_k_pieces.hip) has no crop at
// the front, no literals and no patch, and its code object stays what it is.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_kernels.h"
#include "avr_load16.h"   // load16_shifted

namespace avr {

// One workgroup per span, any alignment on either side: bytes up to the destination's first 16-byte
// boundary, then 16-byte stores, each made of the two aligned 16-byte source blocks that hold its
// bytes, then the rest by bytes.  A 16-byte load is made only of aligned blocks that lie wholly inside
// [src, src + src_len): the stores whose blocks would reach before the buffer's first byte or past
// its last one go by bytes too (a span that starts at the first byte of a buffer that is not itself
// aligned, one that ends flush with the buffer's end).  A span outside src_len or dst_len is refused:
// nothing of it is read or written.
__global__ __launch_bounds__(256) void gather_spans_kernel(const avr_span* spans, int n, const uint8_t* src,
                                                           uint64_t src_len, uint8_t* dst, uint64_t dst_len,
                                                           int32_t* status) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const avr_span sp = spans[k];
  const uint32_t t = threadIdx.x, nt = blockDim.x, len = sp.len;
  if (sp.src_off > src_len || len > src_len - sp.src_off || sp.dst_off > dst_len || len > dst_len - sp.dst_off) {
    if (t == 0) status[k] = AVR_SLICE_OVERFLOW;
    return;
  }
  if (t == 0) status[k] = 0;
  if (!len) return;
  const uint8_t* s = src + sp.src_off;
  uint8_t* d = dst + sp.dst_off;
  const uint32_t head = min(len, (uint32_t)((16 - ((uintptr_t)d & 15)) & 15));
  // store j writes d[head + 16 j, + 16) from the aligned source blocks j and (a != 0) j + 1 of s4
  const uint32_t nv = (len - head) / 16;
  const uintptr_t sv = (uintptr_t)(s + head);
  const uint32_t a = (uint32_t)(sv & 15);
  const uintptr_t base = sv - a;                      // block 0; may start before src
  const uintptr_t lo = (uintptr_t)src, hi = lo + src_len;
  const uint32_t reach = a ? 32 : 16;                 // bytes of aligned blocks one store loads
  uint32_t j0 = base < lo ? 1 : 0, j1 = 0;
  if (hi >= base + reach) j1 = (uint32_t)min((uint64_t)nv, (uint64_t)((hi - base - reach) / 16 + 1));
  if (j0 > nv) j0 = nv;
  if (j1 < j0) j1 = j0;
  const uint4* s4 = (const uint4*)base;
  uint4* d4 = (uint4*)(d + head);
  for (uint32_t j = j0 + t; j < j1; j += nt) d4[j] = load16_shifted(s4, j, a, true);
  // by bytes: the head, the stores left out at either edge, the tail
  const uint32_t b0 = head + 16 * j0, b1 = head + 16 * j1;
  for (uint32_t i = t; i < b0; i += nt) d[i] = s[i];
  for (uint32_t i = b1 + t; i < len; i += nt) d[i] = s[i];
}

// One thread per selected unit, after the gather on the same stream (stream order is the only
// synchronisation).  status = the unit's own when non-zero; AVR_SLICE_NO_END for a piece that came
// out shorter than its share of the slice, or a slice whose regenerated length does not restore
// exactly the block's size -- stricter than the whole-file splice, which never compares the two: a
// range read's coordinates are the container's sizes.  Then the last-byte rule: replaced, or appended
// over the byte of slack the gather copied there.
__global__ __launch_bounds__(256) void range_tails_kernel(const avr_range_tail* tails, const avr_slice_result* res, int n,
                                                          uint8_t* dst, uint64_t dst_len, int32_t* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const avr_range_tail t = tails[k];
  const avr_slice_result r = res[k];
  int32_t st = r.status;
  if (st == 0) {
    if (t.keep != 0xffffffffu) {
      if (r.out_len < t.keep) st = AVR_SLICE_NO_END;
    } else {
      const uint64_t total = (uint64_t)t.q_last + r.out_len;
      const bool append = t.has_rule && (uint32_t)(total & 1) != (uint32_t)(t.length_parity & 1);
      if (total + (append ? 1 : 0) != t.size) {
        st = AVR_SLICE_NO_END;
      } else if (t.has_rule && t.final_pos != AVR_RANGE_NO_POS) {
        if (t.final_pos < dst_len) dst[t.final_pos] = t.last_byte;
        else st = AVR_SLICE_OVERFLOW;
      }
    }
  }
  status[k] = st;
}

hipError_t launch_gather_spans(const avr_span* spans, int n, const uint8_t* src, uint64_t src_len, uint8_t* dst,
                               uint64_t dst_len, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_spans_kernel, dim3(n), dim3(256), 0, stream, spans, n, src, src_len, dst, dst_len, status);
  return hipGetLastError();
}

hipError_t launch_range_tails(const avr_range_tail* tails, const avr_slice_result* res, int n, uint8_t* dst,
                              uint64_t dst_len, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(range_tails_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tails, res, n, dst, dst_len, status);
  return hipGetLastError();
}

}  // namespace avr
