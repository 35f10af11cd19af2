// avr_pack_pieces: the packing of a batch of units (whole slices and the pieces of split slices,
// include/avrecode.h avr_piece) for the gather of a sharded decompress.  A unit keeps the first
// `keep` bytes it regenerated (a piece's bytes up to the next cut's first byte; everything for a last
// piece or a whole slice), so the consecutive units of a slice pack into the slice's bytes without
// gaps.  A scan kernel and a copy kernel, as scan_lengths_kernel / pack_kernel (avr_kernels.hip); no
// reference counterpart (the reference decodes a slice as one chain, recode.cpp:1411-1520).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_kernels.h"

namespace avr {

// what unit k keeps and the status it reports: a failed unit keeps nothing; a piece that came out
// shorter than its share of the slice fails as splice_pieces fails its block (AVR_SLICE_NO_END)
__device__ __forceinline__ uint32_t unit_kept(const avr_piece& p, const avr_slice_result& r, int32_t* status) {
  if (r.status != 0) {
    *status = r.status;
    return 0;
  }
  if (p.keep != 0xffffffffu && r.out_len < p.keep) {
    *status = AVR_SLICE_NO_END;
    return 0;
  }
  *status = 0;
  return p.keep == 0xffffffffu ? r.out_len : p.keep;
}

__global__ __launch_bounds__(1024) void scan_kept_kernel(const avr_piece* pieces, const avr_slice_result* res, int n,
                                                         uint64_t* offsets, uint32_t* kept, int32_t* status) {
  // single workgroup exclusive scan (n is a few thousand at most)
  __shared__ uint64_t part[1024];
  const int t = threadIdx.x, nt = blockDim.x;
  const int per = (n + nt - 1) / nt;
  const int lo = min(n, t * per), hi = min(n, (t + 1) * per);
  uint64_t sum = 0;
  for (int i = lo; i < hi; i++) {
    int32_t st;
    const uint32_t k = unit_kept(pieces[i], res[i], &st);
    kept[i] = k;
    status[i] = st;
    sum += k;
  }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < nt; off <<= 1) {
    uint64_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t run = t ? part[t - 1] : 0;
  for (int i = lo; i < hi; i++) {
    offsets[i] = run;
    run += kept[i];
  }
  if (t == nt - 1) offsets[n] = part[nt - 1];
}

// bytes [8 bs, 8 bs + 32) of the 64-bit window hi:lo (bs < 4)
__device__ __forceinline__ uint32_t window32(uint32_t lo, uint32_t hi, uint32_t bs) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bs));
}

// One workgroup per unit.  The source (a unit's output in the work buffer) is 16-byte aligned, the
// destination wherever the prefix sum put it: bytes up to the destination's first 16-byte boundary,
// then 16-byte stores, each made of the two aligned 16-byte loads that hold its bytes, then the
// rest by bytes.  A load never reaches past the 16-byte block of the unit's last kept byte.
__global__ __launch_bounds__(256) void pack_pieces_kernel(const avr_slice_desc* descs, int n, const uint8_t* out,
                                                          uint8_t* packed, const uint64_t* offsets,
                                                          const uint32_t* kept) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const uint32_t len = kept[k];
  if (!len) return;
  const uint8_t* src = out + descs[k].out_offset;
  uint8_t* dst = packed + offsets[k];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  if ((uintptr_t)src & 15) {   // not a plan's layout: by bytes
    for (uint32_t i = t; i < len; i += nt) dst[i] = src[i];
    return;
  }
  const uint32_t head = min(len, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
  for (uint32_t i = t; i < head; i += nt) dst[i] = src[i];
  // store j writes dst[head + 16 j, + 16) from src's aligned blocks j and (head != 0) j + 1
  const uint32_t blocks = (len + 15) / 16;                  // aligned source blocks holding kept bytes
  uint32_t nv = (len - head) / 16;
  if (head && nv + 1 > blocks) nv = blocks - 1;
  const uint4* s4 = (const uint4*)src;
  uint4* d4 = (uint4*)(dst + head);
  const uint32_t ws = head >> 2, bs = head & 3;
  for (uint32_t j = t; j < nv; j += nt) {
    const uint4 a = s4[j];
    uint4 o = a;
    if (head) {
      const uint4 b = s4[j + 1];
      switch (ws) {
        case 0:
          o = make_uint4(window32(a.x, a.y, bs), window32(a.y, a.z, bs), window32(a.z, a.w, bs), window32(a.w, b.x, bs));
          break;
        case 1:
          o = make_uint4(window32(a.y, a.z, bs), window32(a.z, a.w, bs), window32(a.w, b.x, bs), window32(b.x, b.y, bs));
          break;
        case 2:
          o = make_uint4(window32(a.z, a.w, bs), window32(a.w, b.x, bs), window32(b.x, b.y, bs), window32(b.y, b.z, bs));
          break;
        default:
          o = make_uint4(window32(a.w, b.x, bs), window32(b.x, b.y, bs), window32(b.y, b.z, bs), window32(b.z, b.w, bs));
          break;
      }
    }
    d4[j] = o;
  }
  for (uint32_t i = head + 16 * nv + t; i < len; i += nt) dst[i] = src[i];
}

hipError_t launch_pack_pieces(const avr_slice_desc* descs, const avr_piece* pieces, const avr_slice_result* res, int n,
                              const uint8_t* out, uint8_t* packed, uint64_t* offsets, uint32_t* kept, int32_t* status,
                              hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scan_kept_kernel, dim3(1), dim3(1024), 0, stream, pieces, res, n, offsets, kept, status);
  hipLaunchKernelGGL(pack_pieces_kernel, dim3(n), dim3(256), 0, stream, descs, n, out, packed, offsets, kept);
  return hipGetLastError();
}

}  // namespace avr
