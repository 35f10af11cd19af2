// avr_pack_pieces: the packing of a batch of units (whole slices and the pieces of split slices,
// include/avrecode.h avr_piece) for the gather of a sharded decompress.  A unit keeps the first
// `keep` bytes it regenerated (a piece's bytes up to the next cut's first byte; everything for a last
// piece or a whole slice), so the consecutive units of a slice pack into the slice's bytes without
// gaps.  A scan kernel and a copy kernel, as scan_lengths_kernel / pack_kernel (avr_kernels.hip); no
// reference counterpart (the reference decodes a slice as one chain, recode.cpp:1411-1520).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "avr_kernels.h"
#include "avr_load16.h"   // window32, load16_shifted

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

// ------------------------------------------------------------------ avr_stage_pieces / avr_verify_units
// The compress side of the split for slice batches (include/avrecode.h, ABI 8): a split walk leaves a
// slice's pieces one after the other in the work buffer, at any alignment; to check them on the
// device they are staged into the layout the pieces' decompress reads, regenerated, packed
// (pack_pieces_kernel above) and compared with the payload.  No reference counterpart.

// a unit's room in the staging arena: its stream, at least 16 zero bytes, rounded up to 16
__device__ __forceinline__ uint64_t staged_room(uint32_t len) { return ((uint64_t)len + 16 + 15) & ~15ull; }

// Single workgroup exclusive scan of the units' rooms (n is a few thousand at most): per-thread
// runs, a shuffle scan inside each wave, the 16 wave totals through LDS.  It also places each unit
// (payload_offset, read_limit) and refuses the ones that do not fit their buffers.
__global__ __launch_bounds__(1024) void scan_stage_kernel(avr_slice_desc* descs, const uint64_t* src, int n,
                                                          uint64_t out_len, uint64_t cap, uint64_t* offsets,
                                                          int32_t* status) {
  __shared__ uint64_t wave_sum[16];
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6;
  const int per = (n + nt - 1) / nt;
  const int lo = min(n, t * per), hi = min(n, (t + 1) * per);
  uint64_t sum = 0;
  for (int i = lo; i < hi; i++) sum += staged_room(descs[i].payload_size);
  unsigned long long incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint64_t run = incl - sum;
  for (int w = 0; w < wave; w++) run += wave_sum[w];
  for (int i = lo; i < hi; i++) {
    const uint32_t len = descs[i].payload_size;
    const uint64_t room = staged_room(len);
    offsets[i] = run;
    descs[i].payload_offset = run;
    descs[i].read_limit = len;
    status[i] = src[i] > out_len || len > out_len - src[i] || run + room > cap ? AVR_SLICE_OVERFLOW : 0;
    run += room;
  }
  if (t == nt - 1) offsets[n] = run;
}

// One workgroup per unit.  pack_pieces_kernel turned round: the source wherever the split walk left
// the piece, the destination 16-byte aligned.  Every store is 16 bytes -- the stream, its last
// bytes filled up with zeros, then the zero bytes after it -- made of the two aligned 16-byte loads
// that hold its bytes; a load never reaches past the 16-byte block of the piece's last byte.
__global__ __launch_bounds__(256) void stage_pieces_kernel(const avr_slice_desc* descs, const uint64_t* src, int n,
                                                           const uint8_t* out, uint8_t* arena, const uint64_t* offsets,
                                                           const int32_t* status) {
  const int k = blockIdx.x;
  if (k >= n || status[k] != 0) return;
  const uint32_t len = descs[k].payload_size;
  const uint8_t* s = out + src[k];
  uint8_t* dst = arena + offsets[k];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  const uint32_t room = (uint32_t)(offsets[k + 1] - offsets[k]);
  if ((uintptr_t)dst & 15) {   // not a staging arena's alignment: by bytes
    for (uint32_t i = t; i < room; i += nt) dst[i] = i < len ? s[i] : (uint8_t)0;
    return;
  }
  const uint32_t a = (uint32_t)((uintptr_t)s & 15);
  const uint4* s4 = (const uint4*)(s - a);
  const uint32_t last = len ? (a + len - 1) / 16 : 0;   // the aligned source block of the last byte
  uint4* d4 = (uint4*)dst;
  for (uint32_t j = t; j < room / 16; j += nt) {
    uint4 o = make_uint4(0, 0, 0, 0);
    const uint32_t b = 16 * j;
    if (b < len) {
      o = load16_shifted(s4, j, a, j + 1 <= last);
      const uint32_t left = len - b;   // bytes of this store that are the stream's
      if (left < 16) {
        const uint32_t w = left >> 2, m = (1u << (8 * (left & 3))) - 1;
        o.x = w > 0 ? o.x : o.x & m;
        o.y = w > 1 ? o.y : w == 1 ? o.y & m : 0;
        o.z = w > 2 ? o.z : w == 2 ? o.z & m : 0;
        o.w = w == 3 ? o.w & m : 0;
      }
    }
    d4[j] = o;
  }
}

// One workgroup per slice, as verify_kernel (avr_kernels.hip): the slice's regenerated bytes are its
// units' kept bytes, contiguous in `packed` from offsets[first[k]] at any alignment; the payload is
// 16-byte aligned.  The last-byte rule: size or size - 1 bytes, the final byte not compared.
__global__ __launch_bounds__(256) void verify_units_kernel(const avr_slice_desc* d, const avr_slice_result* rc, int n,
                                                           const uint32_t* first, int n_units, const uint8_t* in,
                                                           const uint8_t* packed, const uint64_t* offsets,
                                                           const uint32_t* kept, const int32_t* ustatus,
                                                           int32_t* verdict) {
  const int k = blockIdx.x;
  if (k >= n) return;
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  if (!d[k].coded || rc[k].status != 0) {
    if (threadIdx.x == 0) verdict[k] = 2;
    return;
  }
  const uint32_t u0 = first[k], u1 = first[k + 1], size = d[k].payload_size;
  // every unit done, and their kept bytes one after the other: the lengths add up
  int local = u1 <= u0 || u1 > (uint32_t)n_units;
  uint64_t total = 0;
  for (uint32_t u = u0; u < u1 && !local; u++) {
    local |= ustatus[u] != 0 || offsets[u] + kept[u] != offsets[u + 1];
    total += kept[u];
  }
  if (local || size == 0 || !(total == size || total + 1 == size)) {
    if (threadIdx.x == 0) verdict[k] = 0;
    return;
  }
  const uint8_t* p = in + d[k].payload_offset;
  const uint8_t* r = packed + offsets[u0];
  const uint32_t m = size - 1;   // total >= m bytes stand at r
  uint32_t m16 = 0;
  if (m && !((uintptr_t)p & 15)) {
    const uint32_t a = (uint32_t)((uintptr_t)r & 15);
    const uint4* r4 = (const uint4*)(r - a);
    const uint4* p4 = (const uint4*)p;
    const uint32_t last = (a + m - 1) / 16;   // the aligned block of the last compared byte
    m16 = m / 16;
    for (uint32_t j = threadIdx.x; j < m16; j += blockDim.x) {
      const uint4 x = p4[j], y = load16_shifted(r4, j, a, j + 1 <= last);
      local |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
  }
  for (uint32_t i = m16 * 16 + threadIdx.x; i < m; i += blockDim.x) local |= p[i] != r[i];
  if (local) atomicOr(&bad, 1);
  __syncthreads();
  if (threadIdx.x == 0) verdict[k] = bad ? 0 : 1;
}

hipError_t launch_stage_pieces(avr_slice_desc* descs, const uint64_t* src, int n, const uint8_t* out, uint64_t out_len,
                               uint8_t* arena, uint64_t cap, uint64_t* offsets, int32_t* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scan_stage_kernel, dim3(1), dim3(1024), 0, stream, descs, src, n, out_len, cap, offsets, status);
  hipLaunchKernelGGL(stage_pieces_kernel, dim3(n), dim3(256), 0, stream, descs, src, n, out, arena, offsets, status);
  return hipGetLastError();
}

hipError_t launch_verify_units(const avr_slice_desc* descs, const avr_slice_result* rc, int n, const uint32_t* first,
                               int n_units, const uint8_t* in, const uint8_t* packed, const uint64_t* offsets, const uint32_t* kept,
                               const int32_t* ustatus, int32_t* verdict, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(verify_units_kernel, dim3(n), dim3(256), 0, stream, descs, rc, n, first, n_units, in, packed, offsets,
                     kept, ustatus, verdict);
  return hipGetLastError();
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
