// The device CRC-32 (ISO-HDLC / zlib) of one byte span by one workgroup of 256 threads, shared by the
// kernels that CRC where the bytes lie: avr_k_crc.hip (avr_crc_spans, the slice batches' CRCs) and
// avr_k_check.hip (avr_check_units).  The method -- per-thread table CRCs over right-aligned chunks,
// folded pairwise -- is described in avr_k_crc.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_kernels.h"
#include "avr_load16.h"   // load16_shifted

namespace avr {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;   // x^0: reflected, bit 31 - k is the coefficient of x^k

// r x^8 mod P: one zero byte through the register
__device__ __forceinline__ uint32_t crc_shift8(uint32_t r) {
#pragma unroll
  for (int i = 0; i < 8; i++) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1)));
  return r;
}

// a b mod P: 32 steps, b times x at each
__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1)));
  }
  return p;
}

struct CrcLds {
  uint32_t tab[4][256];   // tab[k][b]: byte b, then k zero bytes (slice-by-4)
  uint32_t part[256];
};

__device__ __forceinline__ uint32_t crc_byte(const CrcLds& s, uint32_t r, uint8_t b) {
  return s.tab[0][(r ^ b) & 0xff] ^ (r >> 8);
}
__device__ __forceinline__ uint32_t crc_word(const CrcLds& s, uint32_t r, uint32_t w) {
  r ^= w;
  return s.tab[3][r & 0xff] ^ s.tab[2][(r >> 8) & 0xff] ^ s.tab[1][(r >> 16) & 0xff] ^ s.tab[0][r >> 24];
}

// One workgroup of 256 threads: the CRC of buf[off, off + len), any alignment.  A 16-byte load is
// made only of aligned 16-byte blocks that lie wholly inside the buffer (it may touch bytes of such a
// block outside the span); what is left at the buffer's ends goes by bytes.  A span that does not lie
// inside buf_len is refused before anything of it is read.
__device__ __forceinline__ void crc_span(CrcLds& s, const uint8_t* buf, uint64_t buf_len, uint64_t off, uint32_t len,
                                         uint32_t* crc, int32_t* status) {
  const uint32_t t = threadIdx.x;
  const bool outside = off > buf_len || len > buf_len - off;
  if (outside || !len) {   // the empty span's CRC is 0
    if (t == 0) {
      *crc = 0;
      *status = outside ? AVR_SLICE_OVERFLOW : 0;
    }
    return;
  }
  // the tables from the polynomial, one entry of each per thread
  uint32_t e = crc_shift8(t);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    s.tab[k][t] = e;
    e = crc_shift8(e);
  }
  __syncthreads();
  // chunk t = the span's bytes [hi - C, hi), hi = len - (255 - t) C, cut at the span's start
  // (lengths are uint32_t: len + 15 and 256 C need 64 bits)
  const uint32_t per = (uint32_t)((((uint64_t)len + 15) / 16 + 255) / 256);   // 16-byte words per chunk
  const int64_t C = 16 * (int64_t)per;
  const int64_t hi = (int64_t)len - (int64_t)(255 - t) * C;
  const int64_t lo = hi - C > 0 ? hi - C : 0;
  uint32_t r = 0;
  if (hi > 0) {
    if (lo == 0) r = 0xffffffffu;   // the init value: the first non-empty chunk only
    const uint8_t* q = buf + off + lo;
    const uint32_t n = (uint32_t)(hi - lo);
    const uint32_t a = (uint32_t)((uintptr_t)q & 15);
    const uintptr_t base = (uintptr_t)q - a;
    const uintptr_t safe_lo = ((uintptr_t)buf + 15) & ~(uintptr_t)15, safe_hi = ((uintptr_t)buf + buf_len) & ~(uintptr_t)15;
    // words [j0, j1) of the chunk by 16-byte loads: word j reads blocks j and (a != 0) j + 1 from base
    const uint32_t need = a ? 2 : 1;
    const uint64_t avail = safe_hi > base ? (safe_hi - base) / 16 : 0;
    const uint32_t j0 = base < safe_lo ? 1 : 0;
    uint32_t j1 = (uint32_t)(avail >= need ? (avail - need + 1 < n / 16 ? avail - need + 1 : n / 16) : 0);
    if (j1 < j0) j1 = j0;
    const uint32_t head = 16 * j0 < n ? 16 * j0 : n;
    for (uint32_t i = 0; i < head; i++) r = crc_byte(s, r, q[i]);
    const uint4* s4 = (const uint4*)base;
    for (uint32_t j = j0; j < j1; j++) {
      const uint4 w = load16_shifted(s4, j, a, true);
      r = crc_word(s, r, w.x);
      r = crc_word(s, r, w.y);
      r = crc_word(s, r, w.z);
      r = crc_word(s, r, w.w);
    }
    for (uint32_t i = 16 * j1 > head ? 16 * j1 : head; i < n; i++) r = crc_byte(s, r, q[i]);
  }
  s.part[t] = r;
  // the level's multiplier: x^(8 C) = (x^128)^per at level 0, squared at each level
  uint32_t m = kCrcOne >> 8;
#pragma unroll
  for (int i = 0; i < 4; i++) m = crc_mulmod(m, m);
  uint32_t mult = kCrcOne;
  for (uint32_t x = per; x; x >>= 1) {
    if (x & 1) mult = crc_mulmod(mult, m);
    m = crc_mulmod(m, m);
  }
  __syncthreads();
  for (uint32_t step = 1; step < 256; step <<= 1) {
    if ((t & (2 * step - 1)) == 0) {
      const uint32_t left = s.part[t];
      s.part[t] = (left ? crc_mulmod(left, mult) : 0u) ^ s.part[t + step];
    }
    mult = crc_mulmod(mult, mult);
    __syncthreads();
  }
  if (t == 0) {
    *crc = ~s.part[0];
    *status = 0;
  }
}

}  // namespace avr
