// What the waves of one slice's workgroup share: the modes and flag bits, the constant tables, the
// LDS records and layout (MbRec, EdgeRec / EdgeCore, Shared), the encodings of the ring operations,
// the ring protocol itself, wave priority and the per-CU board, and the SIG / NZ estimator hash.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/avrecode.h"
#include "avr_engine.h"
#include "avr_kernels.h"
#include "avr_prof.h"

namespace avr {

// MODE_TRACE: the compress-side CABAC decode + parse alone, recording every bin in decode order
// (2 bytes: bin | kind << 1, the context's state byte before the bin) -- the bin sequence the
// libavcodec-hooks layer (avr_hook_*) serves to its caller -- and, between the bins, the model
// events that decide the model keys (kind 3 records, TRACE_EV_*): where each significance map
// begins and ends, with the model coordinates (mb_xy) and sub-macroblock (begin_sub_mb) it runs
// under; the hooks layer checks the caller's begin/end_coding_type(SIG_MAP), mb_xy and
// begin_sub_mb against them (recode.cpp:166-207, 951-974).
enum { MODE_COMPRESS = 0, MODE_DECOMPRESS = 1, MODE_GENERATE = 2, MODE_TRACE = 3 };
enum { F_DEC = 1, F_SKIP = 2, F_INTRA = 4, F_I16 = 8, F_D16 = 16, F_T8 = 32, F_CPRED = 64 };
enum { SE_OTHER = 0, SE_REF, SE_QPDELTA, SE_MVD_SUFFIX, SE_LEVEL_SUFFIX, SE_EOS, SE_PCM };
// MODE_TRACE event records: 0x06 (kind 3), type, payload.  MAP_BEGIN: mb_x, model row (u16 LE
// each), cat, scan8 index, max_coeff, is_dc | chroma422 << 1 (10 bytes); MAP_END: 2 bytes.
enum { TRACE_EV_MAP_BEGIN = 1, TRACE_EV_MAP_END = 2 };

static __constant__ uint8_t c_scan8[51] = {
  4 + 1 * 8,  5 + 1 * 8,  4 + 2 * 8,  5 + 2 * 8,  6 + 1 * 8,  7 + 1 * 8,  6 + 2 * 8,  7 + 2 * 8,
  4 + 3 * 8,  5 + 3 * 8,  4 + 4 * 8,  5 + 4 * 8,  6 + 3 * 8,  7 + 3 * 8,  6 + 4 * 8,  7 + 4 * 8,
  4 + 6 * 8,  5 + 6 * 8,  4 + 7 * 8,  5 + 7 * 8,  6 + 6 * 8,  7 + 6 * 8,  6 + 7 * 8,  7 + 7 * 8,
  4 + 8 * 8,  5 + 8 * 8,  4 + 9 * 8,  5 + 9 * 8,  6 + 8 * 8,  7 + 8 * 8,  6 + 9 * 8,  7 + 9 * 8,
  4 + 11 * 8, 5 + 11 * 8, 4 + 12 * 8, 5 + 12 * 8, 6 + 11 * 8, 7 + 11 * 8, 6 + 12 * 8, 7 + 12 * 8,
  4 + 13 * 8, 5 + 13 * 8, 4 + 14 * 8, 5 + 14 * 8, 6 + 13 * 8, 7 + 13 * 8, 6 + 14 * 8, 7 + 14 * 8,
  0 + 0 * 8,  0 + 5 * 8,  0 + 10 * 8,
};
static __constant__ uint8_t c_b_pairs[9][2] = {{1, 1}, {2, 2}, {1, 2}, {2, 1}, {1, 3}, {2, 3}, {3, 1}, {3, 2}, {3, 3}};
constexpr int kSigEst = 229376;
constexpr int kNzEst = 63 * 2 * 3 * 3 * 57;
constexpr int kEstDefault = 1026;
static_assert(kEstTable >= kSigEst + kNzEst, "estimator table size");

struct MbRec {
  uint8_t flags, is8x8;
  uint16_t cbp;         // FFmpeg cbp_table layout: luma b0-3, chroma b4-5, chroma DC b6-7, luma DC b8-10
  uint8_t nnz[3][16];   // coefficient count per 4x4, raster per plane
  uint8_t mvd[2][16][2];
  int8_t ref[2][4];
  uint8_t direct8[4];
  uint8_t mnnz[52];     // model BlockMeta.num_nonzeros[51]
};
// bottom edge of the macroblock above, dword j gathered from MbRec dword Walker::edge_src (lane j)
// at the publish; 92 B keeps four 1080p workgroups within a CU's LDS
struct EdgeRec {
  uint8_t flags, pad;
  uint16_t cbp;
  uint8_t nnz[3][4];    // bottom row of each plane
  uint8_t mvd[2][4][2]; // bottom row
  int8_t ref[2][2];     // bottom two 8x8 of each list
  uint8_t direct8[2], pad2[2];
  uint8_t mnnz[52];
};
static_assert(sizeof(EdgeRec) == 92, "EdgeRec layout");
// The progressive walkers' ring holds EdgeRec's first ten dwords only (the parse's neighbour
// fields); the model bytes of each column (EdgeRec::mnnz, read by the NZ-tree keys of the parallel
// model) live in a row of their own, `mring`: in LDS after the ring, or -- when that is what lets
// four wide workgroups share a CU's LDS (4K: 240 columns x 92 B would leave room for three) -- in
// the workgroup's global scratch (kFlagMringGlobal).  Only the upper macroblock's bottom-row
// blocks and DC entries are ever read there (get_neighbor_sub_mb's upper neighbours: mnnz bytes
// 8-15, 24-31, 40-50, i.e. dwords 2, 3, 6, 7, 10, 11, 12 -- tests/test_oracle_geometry.py checks
// the table), so a column keeps those 7 dwords, dword d at ((d >> 2) << 1) | (d & 1): 28 B instead
// of 52 (round 6: the 4K stream's model-row write-backs were most of its HBM writes).
struct EdgeCore {
  uint8_t flags, pad;
  uint16_t cbp;
  uint8_t nnz[3][4];
  uint8_t mvd[2][4][2];
  int8_t ref[2][2];
  uint8_t direct8[2], pad2[2];
};
static_assert(sizeof(EdgeCore) == 40 && offsetof(EdgeRec, mnnz) == 40, "EdgeCore = EdgeRec's first ten dwords");
constexpr int kMringDwords = 7;      // per column: the read dwords of EdgeRec::mnnz
constexpr uint32_t kEdgeMringNz = 0x200u;   // EdgeCore dword 0: the column's model row was stored (global row)
constexpr uint32_t kMringUsed = 0x1CCCu;   // those dwords (2, 3, 6, 7, 10, 11, 12) of the 13
AVR_FI uint32_t mring_dword(uint32_t d) { return (d >> 2) << 1 | (d & 1); }
static_assert(sizeof(MbRec) == 180, "MbRec layout (dword map in Walker::edge_src)");

// LDS layout (per workgroup = one slice); the ring is sized by mb_width at launch.
// SIG + NZ estimators: an LDS hash table (4096 slots, 16 KB) in front of the dense per-model
// table in HBM (kEstTable u16 entries).  A slice touches ~3.5-5.5 K distinct SIG/NZ keys out of
// 294 K, so the first ones seen get an LDS slot for the rest of the model's life and only the
// keys that find their probe window full live in HBM (0.4 % of lookups at QP 22, none at QP 30,
// vs ~11 % misses for the direct-mapped write-back cache this replaces).  Keys never leave the
// table, so "not in the window and the window has a free slot" means "never seen": a new key
// starts at the default estimator without any HBM access.
//   key p = idx * kEstKeyMul mod 2^19 (a bijection), home slot p >> 7, tag p & 127; one probe is
//   one LDS read per lane over the 64 slots home .. home + 63; slot = (0x8000 | disp << 7 | tag)
//   << 16 | estimator, 0 = free.
// The HBM table is cleared lazily and sparsely: an entry stored there carries bit 15 (estimators
// use 15 bits: neg - 1 <= 0x60), so its first store is recognised and its index appended to the
// table's write log; the next model using the table zeroes the logged entries (the whole table
// only if the log overflowed) instead of clearing 588 KB per slice.
constexpr int kEtabBits = 12;
constexpr int kEtabSize = 1 << kEtabBits;
constexpr uint32_t kEstKeyMul = 0x4F1BBu;   // odd: multiplication mod 2^19 is a bijection
constexpr uint32_t kEstWritten = 0x8000u;
static_assert(kEstTable < (1 << 19), "estimator key space");

// Producer -> consumer ring of coding operations (see "Two waves per slice" below).
constexpr int kFifo = 512;

struct Shared {
  HotTables tab;          // copy of EngineTables::hot (per-bin lookups stay in LDS)
  uint32_t fifo[2][kFifo];   // [0] walker -> next wave, [1] modeler -> coder (compress only)
  uint32_t fifo_head[2];     // operations published by the ring's producer (monotonic)
  uint32_t fifo_tail[2];     // operations retired by the ring's consumer (monotonic)
  int32_t p_status, p_stop_ok, c_err;  // slice results of the two waves
  uint32_t elog_n;           // entries appended to the HBM table's write log by this model
  uint32_t prio;             // the slice's current wave priority (walker -> modeler / coder)
  uint32_t qnext;            // persistent launches: the queue entry this workgroup drew
  uint32_t c_len, c_last;
  uint32_t bill[6];          // the coder's h264_model billing by CodingType (kFlagBill launches)
  uint32_t blk[64];       // residual blocks of the current macroblock (packed, see push_block)
  uint8_t state[1024];
  uint16_t est[kEstDefault + 2];
  uint8_t in_stage[kStage];
  MbRec cur, left;
  union {
    uint32_t etab[kEtabSize + 64]; // compress/decompress: LDS hash table of the SIG + NZ estimators
                                   //   (home slots 0 .. kEtabSize - 1, probe windows do not wrap)
    uint16_t gen_p[1024];          // generator: P(bin = 1) in 1/65536 per context
  };
};

// ---------------------------------------------------------------------------------------
// Several waves per slice.  The hot path is a chain of serial recurrences that only meet in the
// bin value, so each runs on its own wave and they overlap on the SIMD instead of adding up:
//   compress:   walker (CABAC decode + slice_data parse + model keys)  --ring 0-->
//               modeler (estimator lookup/update, recode.cpp:816-820, 1030-1047)  --ring 1-->
//               coder (arithmetic_code<uint64_t,uint8_t> encoder, recode.cpp:1074, 1092-1094)
//   decompress: walker (recoded decode + model + parse: the parse needs each bin at once)
//               --ring 0--> coder (cabac::encoder, cabac_code.h:33-67)
// Consumers retire a ring in batches of up to 64 ops (one entry per lane, plus whatever table
// record that lane can gather), then run their serial chain over the batch from registers.
//
// ring 0, compress (model ops): bit 0 bin, bit 1 SIG/NZ estimator (else per-context), bit 2
//   significance-map threshold 0x50 (else 0x60), bits 3-21 estimator index.
// ring 1, compress (coder ops): bit 0 bin, bits 1-7 pos, bits 8-14 pos+neg of the estimator
//   before its update.
// ring 0, decompress: bit 0 bin, bits 1-2 kind (0 decision, 1 bypass, 2 terminate), bits 3-12
//   ctxIdx.
// Billing classes (h264_model::coding_type at the put, recode.cpp:615-661): compress coder ops
//   carry it in bits 15-16 (0 UNKNOWN, 1 SIGNIFICANCE_MAP, 2 SIGNIFICANCE_NZ), decompress walker
//   ops in bits 13-14 (0 UNKNOWN, 1 SIGNIFICANCE_MAP, 2 SIGNIFICANCE_EOB).
// OP_FINISH = arithmetic_code::encoder::finish (terminate = 1); OP_END closes a slice's stream.
enum { PIPC_UNKNOWN = 0, PIPC_UNREACHABLE, PIPC_SIG_MAP, PIPC_SIG_EOB, PIPC_SIG_NZ, PIPC_RESIDUALS };
constexpr uint32_t OPC_SHIFT_C = 15, OPC_SHIFT_D = 13;
__host__ __device__ inline int op_class_pip_c(uint32_t c) { return c == 1 ? PIPC_SIG_MAP : c == 2 ? PIPC_SIG_NZ : PIPC_UNKNOWN; }
__host__ __device__ inline int op_class_pip_d(uint32_t c) { return c == 1 ? PIPC_SIG_MAP : c == 2 ? PIPC_SIG_EOB : PIPC_UNKNOWN; }
constexpr uint32_t OP_FINISH = 1u << 30;
constexpr uint32_t OP_END = 1u << 31;
// compress rings of the long-slice split (SPL): with OP_FINISH at a cut -- the modeler starts a fresh
// model after it, the coder a fresh stream (bit 29: no model or coder op reaches it)
constexpr uint32_t OP_RESTART = 1u << 29;
enum { OPK_DECISION = 0, OPK_BYPASS = 1, OPK_TERMINATE = 2, OPK_MACRO = 3 };

constexpr uint32_t OPM_CACHE = 2, OPM_THR50 = 4;
AVR_FI uint32_t op_model(int bin, uint32_t flags, uint32_t idx) { return (uint32_t)bin | flags | idx << 3; }
AVR_FI uint32_t op_recode(int bin, uint32_t est) {
  const uint32_t pos = (est & 0xff) + 1, tot = pos + (est >> 8) + 1;
  return (uint32_t)bin | pos << 1 | tot << 8;
}
// Decompress macro ops (kind OPK_MACRO, progressive walkers): the coder expands them into the bins
// and contexts the walker would have sent one by one.  Bits 3-4 select the op:
//   0 map segment: ctxBlockCat bits 5-8, positions coded in this 16-position segment - 1 bits 9-12,
//     bit 13 = the map ended on a last_significant_coeff_flag of 1 at its highest significant
//     position (else: a full segment, or the map ran to max - 1), bits 14-29 the
//     significant_coeff_flag of each position.  The coder tracks the segment's first position; a
//     map's last segment resets it and the level counters (gt1 / eq1 of residual_block_cabac);
//   1 level: ctxBlockCat bits 5-8, sign bit 9, min(coeff_abs_level_minus1 + 1, 15) bits 10-13 (15:
//     the prefix only; the escape's suffix and the sign follow as bypass ops);
//   2 mvd component: vertical bit 5 (ctxIdxOffset 47, else 40), ctxIdxInc of the first bin bits 6-7,
//     sign bit 8, min(|mvd|, 9) bits 9-12 (9: the prefix only; the UEG3 suffix and the sign follow
//     as bypass ops).
AVR_FI uint32_t op_map(int cat, int npos, int ended, uint32_t mask) {
  return OPK_MACRO << 1 | (uint32_t)cat << 5 | (uint32_t)(npos - 1) << 9 | (uint32_t)ended << 13 | mask << 14;
}
AVR_FI uint32_t op_level(int cat, int absl, int sign) {
  return OPK_MACRO << 1 | 1u << 3 | (uint32_t)cat << 5 | (uint32_t)sign << 9 | (uint32_t)absl << 10;
}
AVR_FI uint32_t op_mvd(int comp, int inc, int amvd, int sign) {
  return OPK_MACRO << 1 | 2u << 3 | (uint32_t)comp << 5 | (uint32_t)inc << 6 | (uint32_t)sign << 8 | (uint32_t)amvd << 9;
}
// Ring counters: plain LDS accesses.  LDS is one memory per CU and executes each wave's accesses
// in program order, so a counter store issued after the entry stores cannot be seen before them;
// the asm statements only keep the compiler from reordering (an acquire/release fence would
// also wait for, or write back, this wave's outstanding global stores).
// The casts to address space 3 matter: a volatile access through a generic pointer stays a
// flat access with cache-bypass bits and a vmcnt(0) wait (the address-space inference pass does
// not rewrite volatile accesses), which costs a global-memory round trip per counter update.
typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;
AVR_FI uint32_t ld_volatile(const uint32_t* p) {
  const uint32_t v = *(lds_vu32*)p;
  asm volatile("" ::: "memory");
  return __builtin_amdgcn_readfirstlane(v);
}
AVR_FI void st_volatile(uint32_t* p, uint32_t v) {
  asm volatile("" ::: "memory");
  *(lds_vu32*)p = v;
}
// LDS hand-offs between the lanes of ONE wave need no barrier (a wave's LDS operations execute in
// order); only the compiler must not move memory operations across the hand-off.
AVR_FI void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// Wave priority (s_setprio): the SQ issues from higher-priority waves first, then the oldest.
// A batch's time is its longest slice's, and the slices sharing a CU compete for the issue slots,
// so every wave of a slice runs at a priority that grows with the slice's remaining input
// (longest-remaining-first); the walker sets it once per macroblock and publishes it in LDS,
// the modeler and coder follow it once per ring batch.
AVR_FI void set_prio(uint32_t p) {
  switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
// The slices that share a CU (up to 4 resident workgroups) rank themselves by remaining input on
// a per-CU board in global memory (one copy per kernel): each walker registers a cell of its CU
// (HW_ID / XCC_ID registers), posts its remaining bytes there once per macroblock and takes
// priority 3 - (number of CU neighbours with more input left), so the CU's issue slots go to the
// longest remaining slice first and the co-resident slices tend to finish together.  The board
// is shared by waves of one CU only, so workgroup-scope accesses (through the CU's own vector
// cache and the XCD's L2) suffice; agent scope would send every post to memory.  A stale read
// only delays a priority change.
constexpr int kCuIds = 2048;   // XCC (3 bits) x SE (3) x SH (1) x CU (4)
static __device__ uint32_t avr_cu_count[kCuIds];
static __device__ uint32_t avr_cu_rem[kCuIds * 4];
AVR_FI uint32_t cu_cell() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_REG_HW_ID
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (15 << 11));  // HW_REG_XCC_ID
  const uint32_t cu = (((xcc & 7) * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 15);
  uint32_t slot = 0;
  if (__lane_id() == 0) slot = atomicAdd(&avr_cu_count[cu], 1u);
  return cu * 4 + (__builtin_amdgcn_readfirstlane(slot) & 3);
}
// Host side: zero this translation unit's board before a launch (stream-ordered).
static inline hipError_t reset_cu_board(hipStream_t stream) {
  void *cnt = nullptr, *rem = nullptr;
  hipError_t e = hipGetSymbolAddress(&cnt, HIP_SYMBOL(avr_cu_count));
  if (e == hipSuccess) e = hipGetSymbolAddress(&rem, HIP_SYMBOL(avr_cu_rem));
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(avr_cu_count), stream);
  if (e == hipSuccess) e = hipMemsetAsync(rem, 0, sizeof(avr_cu_rem), stream);
  return e;
}
constexpr uint32_t kNoCell = 0xffffffffu;   // Walker::prio_cell not assigned yet
AVR_FI void cu_post(uint32_t cell, uint32_t rem) {
  if (__lane_id() == 0) __hip_atomic_store(&avr_cu_rem[cell], rem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
AVR_FI uint32_t cu_rank_prio(uint32_t cell, uint32_t rem) {
  const uint32_t lane = __lane_id(), me = cell & 3;
  uint32_t v = 0;
  if (lane < 4) v = __hip_atomic_load(&avr_cu_rem[(cell & ~3u) + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  const uint64_t ahead = __ballot(lane < 4 && lane != me && (v > rem || (v == rem && lane < me)));
  return 3u - (uint32_t)__builtin_popcountll(ahead);
}

AVR_FI void follow_prio(Shared* sh, uint32_t* cur) {
  const uint32_t p = __builtin_amdgcn_readfirstlane(*(volatile __attribute__((address_space(3))) uint32_t*)&sh->prio);
  if (p != *cur) {
    *cur = p;
    set_prio(p);
  }
}

AVR_FI uint64_t readlane64(uint64_t v, uint32_t j) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, j);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), j);
  return (uint64_t)hi << 32 | lo;
}

// v_writelane_b32 (clang has no builtin for it; the LLVM intrinsic by its name)
extern "C" __device__ int avr_llvm_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// Producer end of ring r: entries go to LDS at once, the head counter every 32 entries (and on
// demand), the tail is re-read only when the ring looks full.
template <bool STAGED>
struct RingOutT {
  Shared* sh;
  int r;
  uint32_t head, room;
  AVR_FI void init(Shared* s, int ring) {
    sh = s;
    r = ring;
    head = 0;
    room = kFifo;
    stage_v = 0;
    stage_n = 0;
  }
  AVR_FI void publish() {
    flush();
    st_volatile(&sh->fifo_head[r], head);
  }
#ifdef AVR_PROFILE
  uint64_t wait_cycles = 0;
#endif
  // STAGED: single ops are staged in a VGPR (lane k = k-th op) and stored 64 at a time (fewer
  // instructions per op on the producer; measured 1 % faster for the decompress walker, 2 %
  // slower for the compress walker, whose consumer then waits in bursts)
  uint32_t stage_v, stage_n;
  AVR_FI void flush() {
    if (STAGED && stage_n) {
      const uint32_t k = stage_n;
      stage_n = 0;
      push_v_raw(stage_v, k);
    }
  }
  AVR_FI void push_v(uint32_t op_v, uint32_t n) {
    flush();
    push_v_raw(op_v, n);
  }
  // a staged run of ops on either ring kind (stage, then flush_stage before any other push)
  AVR_FI void stage(uint32_t op) {
    stage_v = __lane_id() == stage_n ? op : stage_v;
    if (AVR_UNLIKELY(++stage_n == 64)) flush_stage();
  }
  AVR_FI void flush_stage() {
    if (stage_n) {
      const uint32_t k = stage_n;
      stage_n = 0;
      push_v_raw(stage_v, k);
    }
  }
  AVR_FI void push(uint32_t op) {
    if (STAGED) {
      stage_v = __lane_id() == stage_n ? op : stage_v;
      if (AVR_UNLIKELY(++stage_n == 64)) flush();
      return;
    }
    if (AVR_UNLIKELY(room == 0)) {
      st_volatile(&sh->fifo_head[r], head);
#ifdef AVR_PROFILE
      const uint64_t tw = PROF_T();
#endif
      for (;;) {
        const uint32_t used = head - ld_volatile(&sh->fifo_tail[r]);
        if (used < (uint32_t)kFifo) { room = kFifo - used; break; }
        __builtin_amdgcn_s_sleep(1);
      }
#ifdef AVR_PROFILE
      wait_cycles += PROF_T() - tw;
#endif
    }
    sh->fifo[r][head & (kFifo - 1)] = op;
    head++;
    room--;
    if (AVR_UNLIKELY((head & 31) == 0)) st_volatile(&sh->fifo_head[r], head);
  }
  // n <= 64 ops at once, op k in lane k (one vector store)
  AVR_FI void push_v_raw(uint32_t op_v, uint32_t n) {
    if (AVR_UNLIKELY(room < n)) {
      st_volatile(&sh->fifo_head[r], head);
#ifdef AVR_PROFILE
      const uint64_t tw = PROF_T();
#endif
      for (;;) {
        const uint32_t used = head - ld_volatile(&sh->fifo_tail[r]);
        if (used + n <= (uint32_t)kFifo) { room = kFifo - used; break; }
        __builtin_amdgcn_s_sleep(1);
      }
#ifdef AVR_PROFILE
      wait_cycles += PROF_T() - tw;
#endif
    }
    if (__lane_id() < n) sh->fifo[r][(head + __lane_id()) & (kFifo - 1)] = op_v;
    const uint32_t h0 = head;
    head += n;
    room -= n;
    if ((h0 ^ head) & ~31u) st_volatile(&sh->fifo_head[r], head);
  }
};
// Consumer end: wait for a batch, load it one entry per lane.  Returns the batch size.
AVR_FI uint32_t ring_take(Shared* sh, int r, uint32_t tail, uint32_t* op_v, uint64_t* waited) {
  uint32_t head;
#ifdef AVR_PROFILE
  const uint64_t tw = PROF_T();
#endif
  for (;;) {
    head = ld_volatile(&sh->fifo_head[r]);
    if (head != tail) break;
    __builtin_amdgcn_s_sleep(1);
  }
#ifdef AVR_PROFILE
  *waited += PROF_T() - tw;
#endif
  const uint32_t n = min(head - tail, 64u);
  const uint32_t lane = __lane_id();
  *op_v = lane < n ? sh->fifo[r][(tail + lane) & (kFifo - 1)] : 0u;
  return n;
}
AVR_FI void ring_retire(Shared* sh, int r, uint32_t tail) { st_volatile(&sh->fifo_tail[r], tail); }

// SIG / NZ estimators: probe the LDS hash table (see kEtabBits).  Returns the estimator and in
// *slot where est_store writes it back (0: the HBM table).  Called by a whole wave.
AVR_FI uint32_t est_load(Shared* sh, const uint16_t* est_g, uint32_t idx, uint32_t* slot, bool claim = false) {
  const uint32_t p = (idx * kEstKeyMul) & ((1u << 19) - 1);
  const uint32_t home = p >> 7, tag = p & 127;
  const uint32_t lane = __lane_id();
  const uint32_t ent = sh->etab[home + lane];
  const uint64_t hit = __ballot((ent >> 16) == (0x8000u | lane << 7 | tag));
#ifdef AVR_PROFILE_EST   // with AVR_PROFILE: estimator lookups that go to HBM (scripts/diag_est.py)
  if (lane == 0) atomicAdd(&avr_prof[22], 1ull);
  if (lane == 0 && !hit && !__ballot(ent == 0)) atomicAdd(&avr_prof[23], 1ull);
#endif
  if (AVR_LIKELY(hit != 0)) {
    // the entry's upper half is the slot's tag word already
    const uint32_t j = (uint32_t)__builtin_ctzll(hit);
    const uint32_t ej = __builtin_amdgcn_readlane(ent, j);
    *slot = (ej & 0xffff0000u) | (home + j);
    return ej & 0xffff;
  }
  const uint64_t free_v = __ballot(ent == 0);
  if (AVR_LIKELY(free_v != 0)) {   // of the misses: a new key (the HBM table holds 0.4 % of lookups)
    const uint32_t j = (uint32_t)__builtin_ctzll(free_v);
    *slot = (0x8000u | j << 7 | tag) << 16 | (home + j);
    // a caller that defers its store claims the slot now (a later key of the window must not take it)
    if (claim && lane == j) sh->etab[home + j] = *slot & 0xffff0000u;
    return 0;
  }
  // HBM: slot 1 marks the entry's first store (to be logged), 0 a stored one
  const uint32_t raw = __builtin_amdgcn_readfirstlane(est_g[idx]);
  *slot = __builtin_amdgcn_readfirstlane((raw >> 15 & 1u) ^ 1u);   // a scalar, like the LDS slots
  return raw & (kEstWritten - 1);
}
AVR_FI void est_store(Shared* sh, uint16_t* est_g, uint32_t idx, uint32_t slot, uint32_t e) {
  if (AVR_LIKELY(slot >> 31)) {
    sh->etab[slot & 0xffff] = (slot & 0xffff0000u) | e;
  } else if (__lane_id() == 0) {
    est_g[idx] = (uint16_t)(e | kEstWritten);
    if (slot) {
      const uint32_t n = sh->elog_n;
      sh->elog_n = n + 1;
      uint32_t* lg = (uint32_t*)(est_g + kEstLog);
      if (n < (uint32_t)kEstLogCap) lg[n] = idx;
      *(uint32_t*)(est_g + kEstLogN) = n < (uint32_t)kEstLogCap ? n + 1 : kEstLogOverflow;
    }
  }
}
// Lane-parallel lookup of each lane's key in the first four slots of its window: true (with the
// estimator and its slot) when found there.  A key found stays where it is, so a hit is final;
// a miss (new key, deeper or HBM-resident one) goes through est_load.
AVR_FI bool est_probe4(const Shared* sh, uint32_t idx, uint32_t* e, uint32_t* slot) {
  const uint32_t p = (idx * kEstKeyMul) & ((1u << 19) - 1);
  const uint32_t home = p >> 7, t0 = 0x8000u | (p & 127);
  const uint32_t s0 = sh->etab[home], s1 = sh->etab[home + 1], s2 = sh->etab[home + 2], s3 = sh->etab[home + 3];
  // branch-free (selects): callers run it on every lane
  const bool h0 = (s0 >> 16) == t0, h1 = (s1 >> 16) == (t0 | 1u << 7);
  const bool h2 = (s2 >> 16) == (t0 | 2u << 7), h3 = (s3 >> 16) == (t0 | 3u << 7);
  const uint32_t d = h0 ? 0u : h1 ? 1u : h2 ? 2u : 3u;
  *e = (h0 ? s0 : h1 ? s1 : h2 ? s2 : s3) & 0xffff;
  *slot = (t0 | d << 7) << 16 | (home + d);
  return h0 | h1 | h2 | h3;
}

// A fresh model on a table the last model may have written: zero the logged entries (or the
// whole table), reset the log.  Called by the whole workgroup; ends with a barrier.
AVR_FI void est_table_reset(uint16_t* est_g, Shared* sh) {
  const uint32_t n = *(volatile uint32_t*)(est_g + kEstLogN);
  __syncthreads();   // every thread has read the count before it is reset
  if (n == kEstLogOverflow) {
    uint4* e4 = (uint4*)est_g;
    for (int i = threadIdx.x; i < kEstTable / 8; i += blockDim.x) e4[i] = make_uint4(0, 0, 0, 0);
  } else if (n) {
    const uint32_t* lg = (const uint32_t*)(est_g + kEstLog);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) est_g[lg[i]] = 0;
  }
  if (threadIdx.x == 0) {
    *(uint32_t*)(est_g + kEstLogN) = 0;
    sh->elog_n = 0;
  }
  __syncthreads();
}

}  // namespace avr
