// 16-byte loads at any byte alignment, from aligned 16-byte loads: what the kernels that read packed
// units (avr_k_pieces.hip, avr_k_crc.hip) share.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace avr {

// bytes [8 bs, 8 bs + 32) of the 64-bit window hi:lo (bs < 4)
__device__ __forceinline__ uint32_t window32(uint32_t lo, uint32_t hi, uint32_t bs) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bs));
}

// 16 bytes from byte offset 16 j + a (a < 16) of the 16-byte aligned blocks s4: blocks j and, when the
// bytes reach into it (a != 0 and `next`), j + 1 -- the caller clears `next` where block j + 1 lies
// past the block of the last byte it may read (the bytes from there then read as zero).
__device__ __forceinline__ uint4 load16_shifted(const uint4* s4, uint32_t j, uint32_t a, bool next) {
  const uint4 x = s4[j];
  if (!a) return x;
  const uint4 y = next ? s4[j + 1] : make_uint4(0, 0, 0, 0);
  const uint32_t bs = a & 3;
  switch (a >> 2) {
    case 0:
      return make_uint4(window32(x.x, x.y, bs), window32(x.y, x.z, bs), window32(x.z, x.w, bs), window32(x.w, y.x, bs));
    case 1:
      return make_uint4(window32(x.y, x.z, bs), window32(x.z, x.w, bs), window32(x.w, y.x, bs), window32(y.x, y.y, bs));
    case 2:
      return make_uint4(window32(x.z, x.w, bs), window32(x.w, y.x, bs), window32(y.x, y.y, bs), window32(y.y, y.z, bs));
    default:
      return make_uint4(window32(x.w, y.x, bs), window32(y.x, y.y, bs), window32(y.y, y.z, bs), window32(y.z, y.w, bs));
  }
}

}  // namespace avr
