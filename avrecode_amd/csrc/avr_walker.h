// The per-slice walker shared by the slice kernels (included through avr_slice_kernels.h by the
// avr_k_*.hip units only; each instantiates one kernel so the kernels compile in parallel).
//
// One wavefront (64 lanes) owns one CABAC slice and runs the whole hot path for it:
//   compress:    CABAC decode (fork ff_get_cabac*) -> H.264 slice_data() parse (the fork's
//                caller of the hooks) -> h264_model keys/estimators (recode.cpp:615-1059)
//                -> recoded arithmetic encode (arithmetic_code.h, recode.cpp:1061-1100, 1134-1268)
//   decompress:  recoded decode -> parse -> model -> CABAC re-encode (recode.cpp:1411-1520,
//                cabac_code.h)
//   generate:    seeded bins -> parse -> CABAC encode (synthetic benchmark slices)
// The serial part runs redundantly on all lanes (wave-uniform values); the lanes cooperate on
// staging the byte streams through LDS and on clearing the model tables.  Everything is inlined
// into the kernel (no calls, no private arrays) so the walker state lives in registers: a
// non-inlined member call would put the whole Walker in scratch memory.
//
// Model modes: RM = true reproduces recode.cpp exactly (estimators and frame metadata persist
// across slices; one wavefront walks all slices in file order).  RM = false applies the same
// model to each slice from a fresh state (independent slices, one wavefront per slice).
//
// This header: struct Walker (the parse, the model keys, the per-bin engines) and the walk of one
// slice.  The other waves' bodies are in avr_coder.h, the kernels in avr_slice_kernels.h.
#pragma once
#include <type_traits>

#include "avr_slice_lds.h"

// The rare exits of the macroblock loop and of the block list (used where MODE is a template
// parameter): hinted in the decompress walkers only.  With them the batch decompress kernel measured
// 1.4 % faster and the compress kernel 1.6 % slower than without.  Macros, not functions:
// __builtin_expect has to stand in the branch's own condition.  They read the template parameter MODE
// of the scope they are used in and are this header's alone (#undef at its end).
#define AVR_MB_LIKELY(x) (MODE == MODE_DECOMPRESS ? AVR_LIKELY(x) : (x))
#define AVR_MB_UNLIKELY(x) (MODE == MODE_DECOMPRESS ? AVR_UNLIKELY(x) : (x))

// Components of the frame walkers' block state kept in VGPR lanes (Walker::BS, 0-3; 0: the LDS
// records).  A build knob only so that each component can be measured alone.
#ifndef AVR_BLOCK_STATE
#define AVR_BLOCK_STATE 3
#endif

namespace avr {

// FLD: field-coded slices (PAFF, MBAFF) -- a second instantiation (kernels of their own, launched
// only when a batch may hold such slices: kFlagFields), so that the progressive walker carries no
// field tests in its per-bin and per-macroblock code

// SPL: the long-slice split's kernels (slices_split_kernel): a piece may start from a seam record
// and stop after n macroblocks, and compress takes the cut records (avr_kernels.h SeamRec)
// SRD: keep the recoded decoder's interval scalar (RecodedDecoder) where VD below would choose
// VDecoder: the persistent queue kernel, whose registers have no room for it
template <int MODE, bool RM, bool FLD = false, bool P32 = false, bool SPL = false, bool SRD = false>
struct Walker {
  static constexpr bool DEC = MODE == MODE_COMPRESS || MODE == MODE_TRACE;  // CABAC decoding side
  const HotTables* T;     // LDS copy
  const EngineTables* G;  // global (init-only tables)
  const avr_slice_desc* d;
  Shared* sh;
  // the upper row's edge records: full EdgeRecs for the field walkers (their MBAFF views and pair
  // records), EdgeCore plus the separate model row (mring) for the progressive ones
  typedef typename std::conditional<FLD, EdgeRec, EdgeCore>::type ERec;
  ERec* ring;
  uint32_t* mring;        // progressive, parallel model: 13 dwords per column (LDS or global)
  bool mring_global;
  uint16_t* est_g;        // SIG + NZ estimators (global)
  uint8_t* frames;        // RM: 2 frames of W*H*52 model bytes
  int64_t cur_off, prev_off;   // RM: byte offsets of the current / previous frame's model bytes (prev < 0: zeros)
  // RM scan (rscan_kernel): model ops go to global memory instead of the modeler's ring
  bool gmode;
  uint32_t* gsink;        // nullptr: count only
  uint32_t gcount;
  // engines
  InStream in;
  OutStream out;
  CabacDecoder cd;
  CabacEncoder ce;
  RecodedEncoder re;
  // the model's decisions go through the reference's arithmetic_code<uint64_t, uint8_t> (both
  // models' default containers); P32 = the parallel model's optional 32-bit coder (avr_engine.h,
  // PDecoder; container tag avrecode-amd:P32)
  // VD: the slice batch's resident and split kernels (frame and field walkers) keep that
  // decoder's interval in VGPRs (avr_engine.h, VDecoder); the sequential kernels, built for a lone
  // wave's latency with another scheduler, and the queue kernel (SRD) keep the scalar one
  static constexpr bool VD = MODE == MODE_DECOMPRESS && !P32 && !RM && !SRD;
  typename std::conditional<P32, PDecoder, typename std::conditional<VD, VDecoder, RecodedDecoder>::type>::type rd;
  uint64_t rng;
  // slice state
  int W, H, mb_x, mb_y, slice_type, is_b, cat_, t8mode;
  // field coding: fld = the current macroblocks are field coded (their significance contexts use
  // the field tables); my = the model's row of the current macroblock, FFmpeg's sl->mb_y (frame
  // rows: a field picture's row r is frame row 2 r + bottom), stepped by ystep per parse row
  int fld, fld_pic, my, ystep;
  // RM parallel compress (rscan_kernel): this slice belongs to the first-coded field of its frame,
  // so the other field's rows -- already in the frame buffer, which that kernel fills before it
  // reads -- must read as the zeros the sequential model still sees there
  int top_pending;
  AVR_FI int mrow() const { return FLD ? my : mb_y; }   // the model's row (progressive: the parse row)
  // MBAFF frame (AVR_STRUCT_MBAFF): macroblock pairs; pst = the pair's state (PST_*); ring_cols =
  // EdgeRec slots the launch gave the LDS ring (an MBAFF slice needs 3 W + 7, see pair_edge)
  int mbaff;
  uint32_t pst, ring_cols;
  int left_ok, top_ok, last_dqp_nz;
  // flags (bits 0-6, F_*) and coded_block_pattern (bits 16-31) of the current macroblock and of
  // its left / upper neighbours, in one scalar register each for the whole macroblock (the
  // neighbours' read once at its start): context selection reads no LDS for them.  Bit 7 of cf:
  // the current macroblock has an 8x8 residual block (finished_queueing's is_8x8).
  uint32_t cf, lf, tf;
  static constexpr uint32_t CF_8X8 = 0x80;
  uint32_t edge_src;      // lane j < 23: the MbRec dword that becomes EdgeRec dword j (set per slice)

  // ------------------------------------------------------------------ block state in VGPR lanes
  // The frame walkers of the parallel model keep what a residual block needs before its first bin
  // in VGPR lanes, so that a block starts on v_readlane instead of a chain of LDS round trips
  // (DESIGN §4.5).  BS counts the components in use, each on top of the one before:
  //   1  blk_v:  the macroblock's block list, lane j = record j in bitstream order (list_build)
  //   2  nz_v / nzn_v: the parse's nnz grid and its neighbours (coded_block_flag contexts)
  //   3  mz_v / mzl_v / mzt_v: the model's nnz (the NZ tree's neighbours), blk2_v bits 16-31
  // (A fourth, the ctxBlockCat bases in two registers with lane = cat, measured slower in the
  // decompress kernel and is not kept: DESIGN §4.5.)
  // The field / MBAFF and the R-mode walkers keep the LDS records (BS = 0).  So do the persistent
  // queue kernels (SRD) and the split kernels (SPL): with these registers their listings spill more
  // VGPRs than without, and a spilling kernel is not shipped.
  static constexpr int BS = (!RM && !FLD && !SPL && !SRD) ? AVR_BLOCK_STATE : 0;
  // blk_v, lane j < nb: cat bits 0-3, n (scan8 index) 4-9, max 10-16, is_dc 17, c422 18, then the
  // block's lane g = p * 16 + y4 * 4 + x4 of the nnz grid as x4 19-20, y4 21-22, p 23-24, and pw 25-27.
  // blk2_v, lane j < nb: the lanes of the block's left (bits 0-5) and upper (8-13) nnz neighbour
  // with bit 6 / 14 set when that lane is nzn_v's, not nz_v's; the block's nb_left / nb_up table
  // bytes in bits 16-23 / 24-31 (0 for the DC blocks, n >= 48, which do not use them).
  // residual() reads lanes j < nb only, the lanes list_build has just written.
  uint32_t blk_v, blk2_v;
  // nz_v, lane g < 48: MbRec::nnz[p][y4 * 4 + x4] of the current macroblock (0 at its start).  Read
  // at g - 1 (x4 > 0) and g - 4 (y4 > 0) of a block's own g and stored by lane to sh->cur.nnz at the
  // macroblock's end: lanes 48-63 are never touched.
  // nzn_v, lane p * 8 + y4: what nnz_left gives for row y4 of plane p at x4 = 0; lane p * 8 + 4 + x4:
  // what nnz_top gives for column x4 at y4 = 0 (edge_load: unavailable defaults, the plane's width
  // and the 4:4:4 override folded in).  Lanes 0-23 are all loaded; lanes 24-63 are never read.
  uint32_t nz_v, nzn_v;
  // mz_v, lane n < 52: MbRec::mnnz[n] of the current macroblock; mzl_v, lane idx < 52: mnnz_left(idx);
  // mzt_v, lane idx < 52: mnnz_top(idx) -- the upper macroblock's kept model bytes (kMringUsed; the
  // other lanes hold 0 and, like the bytes the row does not keep, are never read).  Lanes 52-63: 0.
  uint32_t mz_v, mzl_v, mzt_v;
  int err, finished;
  uint32_t bins;
  int target_mbs, mbs_done, last_mb;
  int nref0, nref1, d8x8inf, x264_build, first_mb;
  // the long-slice split (SPL): the piece's start record (nullptr: the slice's own start) and
  // macroblock count (0: to end_of_slice); compress: where the cut records go (snap, snap_cap of
  // them, rec_stride apart; snap_n made, count to *snap_count), a candidate every split_bits decoded
  // bits (snap_last: the previous one; snap_q: the previous cut's first byte)
  const SeamRec* seam;
  uint8_t* snap;
  uint32_t* snap_count;
  uint32_t snap_cap, snap_n, snap_last, snap_q, split_bits, rec_stride, piece_mbs;
  int cut;                // the walk stopped at the piece's end (not at end_of_slice)
  // The re-encoder's state where the decoder stands (the oracle's avr_seam_encoder): L = V - offset,
  // V the payload's first bitpos bits, as bytes Z = F[sb..e) - (offset << r) (r = 8 e - bitpos pad
  // bits); q = the last byte below m = (bitpos - 10) / 8 that is not 0xFF, the 0xFF bytes after it
  // outstanding, the bits of L from byte m on in low.  A dozen scalar byte loads, at a cut candidate.
  AVR_FI bool seam_place(uint32_t bitpos, uint32_t offset, uint32_t* ce) const {
    if (bitpos < 26) return false;
    const uint32_t m = (bitpos - 10) >> 3, sb = m > 12 ? m - 12 : 0, e = (bitpos + 7) >> 3, r = 8 * e - bitpos;
    const uint32_t sub = offset << r;
    uint32_t borrow = 0, low = 0, q = ~0u, cache = 0;
    for (uint32_t j = e; j-- > sb;) {
      const uint32_t t = e - 1 - j;
      const uint32_t sbyte = t < 4 ? (sub >> (8 * t)) & 0xff : 0u;
      const uint32_t f = j < in.limit ? (uint32_t)in.g[j] : 0u;
      const uint32_t v = f - sbyte - borrow;
      borrow = v >> 31;
      const uint32_t z = v & 0xff;
      if (j >= m) low |= z << (8 * t);
      else if (q == ~0u && z != 0xff) q = j, cache = z;
    }
    if (borrow || q == ~0u) return false;
    const uint32_t lowbits = bitpos - 8 * m;
    ce[0] = (low >> r) & ((1u << lowbits) - 1);    // ce_low
    ce[1] = cd.range;                               // ce_range
    ce[2] = m - 1 - q;                              // ce_outstanding
    ce[3] = cache;                                  // ce_cache
    ce[4] = lowbits - 18;                           // ce_queue
    ce[5] = q;
    return true;
  }
  // A cut candidate at this row start (compress, SPL; the rule of oracle/oracle_recode.c
  // c_row_start): at least split_bits decoded bits since the last candidate, half of that still ahead
  // in the payload.  Where the re-encoder's state can be placed (and moves forward), the slice is cut
  // here: the record (decoder, re-encoder, contexts with the cached lanes written back, last_dqp_nz,
  // the ring's upper-row edges), then the piece's re-coded stream ends (encoder::finish) and the
  // modeler starts a fresh model (OP_RESTART, taken alone: the walker waits until the modeler has
  // retired it), and the model row reads zero for the new piece's first row.
  AVR_FI void seam_cut(int addr) {
    const uint32_t pos = cd_bitpos(cd);
    if (pos - snap_last < split_bits || (uint64_t)pos + split_bits / 2 > 8ull * d->payload_size) return;
    snap_last = pos;
    if (snap_n >= snap_cap) return;
    uint32_t ce[6];
    if (!seam_place(pos, cd.low >> cd.k, ce) || (snap_n && ce[5] <= snap_q)) return;
    snap_q = ce[5];
    rc_writeback();
    mc_store();
    uint32_t* r32 = (uint32_t*)(snap + (size_t)snap_n * rec_stride);
    const uint32_t lane = __lane_id();
    if (lane < 16) {
      const uint32_t v = lane == 0 ? (uint32_t)addr : lane == 1 ? (uint32_t)last_dqp_nz : lane == 2 ? cd.low
                       : lane == 3 ? cd.range : lane == 4 ? (uint32_t)cd.k : lane == 5 ? cd.next
                       : lane == 6 ? ce[0] : lane == 7 ? ce[1] : lane == 8 ? ce[2] : lane == 9 ? ce[3]
                       : lane == 10 ? ce[4] : lane == 11 ? ce[5] : 0u;
      r32[lane] = v;
    }
    const uint32_t* st = (const uint32_t*)sh->state;
    for (uint32_t i = lane; i < 256; i += 64) r32[16 + i] = st[i];
    const uint32_t* e = (const uint32_t*)ring;
    for (uint32_t i = lane; i < (uint32_t)W * 10; i += 64) r32[16 + 256 + i] = i % 10 ? e[i] : e[i] & ~kEdgeMringNz;
    snap_n++;
    if constexpr (MODE == MODE_COMPRESS) {
      push(OP_FINISH | OP_RESTART);
      publish();
      while (ld_volatile(&sh->fifo_tail[0]) != ring0.head) {
        __builtin_amdgcn_s_sleep(1);
      }
      for (uint32_t i = lane; i < (uint32_t)W * kMringDwords; i += 64) mring[i] = 0;
      wave_sync();
    }
  }
  uint32_t prio_cell, prio_cur;   // this slice's cell on the CU board, current priority
  AVR_FI void update_prio() {
    const uint32_t pos = MODE == MODE_DECOMPRESS ? rd.next : cd.next;
    const uint32_t size = d->payload_size;
    const uint32_t rem = pos < size ? size - pos : 0u;
    cu_post(prio_cell, rem);
    const uint32_t p = cu_rank_prio(prio_cell, rem);
    if (p != prio_cur) {
      prio_cur = p;
      set_prio(p);
      if (__lane_id() == 0) *(volatile __attribute__((address_space(3))) uint32_t*)&sh->prio = p;
    }
  }
  RingOutT<MODE == MODE_DECOMPRESS> ring0;   // walker -> modeler (compress) / coder (decompress)
  // compress: a residual block's level ops are staged in a VGPR and stored together after the
  // block (measured: batch compress -0.4 %, profiles/r04h_lstage_ab.log)
  static constexpr bool kStageLevels = true;
  VTab vt;                // CABAC state records (compress / generate: the walker's engine)

  // ------------------------------------------------------------------ residual context registers
  // The residual contexts of one ctxBlockCat (significant_coeff_flag lanes 0-15,
  // last_significant lanes 16-31, coeff_abs_level_minus1 lanes 32-41, coded_block_flag lanes
  // 42-45) live in one VGPR, lane j
  // holding the walker's per-context value for ctx rc_addr(j): the CABAC state byte (compress,
  // generate) or the estimator (decompress).  A residual bin then costs a v_readlane /
  // v_writelane instead of an LDS round trip.  Switching category writes the lanes back.
  uint32_t rc_v;
  int rc_cat;
  uint32_t sig8_v, last8_v;   // 8x8 significant / last ctxIdxInc tables, lane = scan position
  uint32_t byp_e;         // decompress: the estimator of &bypass_context (recode.cpp:1049), Shared::est[1024] while walking
  // lane L of v := x (L and x wave-uniform).  Decompress: one v_writelane, no lane-mask compare
  // to keep live (R-mode decompress -1 %); compress keeps the select (v_writelane there: +2 %).
  AVR_FI static uint32_t wlane(uint32_t v, uint32_t L, uint32_t x) {
    return (uint32_t)avr_llvm_writelane((int)x, (int)L, (int)v);
  }
  AVR_FI int rc_addr(int cat, uint32_t j) const {
    // Only the contexts the category can use: a lane past them would alias another syntax
    // element's context and write a stale copy back over it at rc_writeback -- within the
    // category (8x8 sig ctxIdxInc 0-14 / last 0-8 then the next element) or, with the field
    // offsets, transform_size_8x8_flag (ctxIdx 399-400 = chroma AC's last lanes 30-31), which
    // bin() updates in LDS while the category stays loaded across macroblocks.
    const bool c8 = cat == 5 || cat == 9 || cat == 13;
    if (!FLD) {   // frame offsets: only the 8x8 categories' lanes alias (within the category)
      if (c8 && (j == 15 || (j >= 25 && j < 32))) return -1;
      return j < 16 ? T->sig_base[cat] + (int)j : j < 32 ? T->last_base[cat] + (int)j - 16
           : j < 42 ? T->abs_base[cat] + (int)j - 32 : j < 46 ? T->cbf_base[cat] + (int)j - 42 : -1;
    }
    const int ns = c8 ? 15 : cat == 3 ? 3 : (cat == 1 || cat == 4 || cat == 7 || cat == 11) ? 14 : 15;
    const int nl = c8 ? 9 : ns;
    if (j < 16) return (int)j < ns ? T->sig_base[cat] + (int)j : -1;
    if (j < 32) return (int)j - 16 < nl ? T->last_base[cat] + (int)j - 16 : -1;
    return j < 42 ? T->abs_base[cat] + (int)j - 32 : j < 46 ? T->cbf_base[cat] + (int)j - 42 : -1;
  }
  AVR_FI void rc_writeback() {
    if (rc_cat < 0) return;
    const int a = rc_addr(rc_cat, __lane_id());
    if (a >= 0) {
      if (MODE == MODE_DECOMPRESS) sh->est[a] = (uint16_t)rc_v;
      else sh->state[a] = (uint8_t)rc_v;
    }
    wave_sync();
    rc_cat = -1;
  }
  AVR_FI void rc_select(int cat) {
    if (cat == rc_cat) return;
    rc_writeback();
    const int a = rc_addr(cat, __lane_id());
    rc_v = a < 0 ? 0u : MODE == MODE_DECOMPRESS ? (uint32_t)sh->est[a] : (uint32_t)sh->state[a];
    rc_cat = cat;
  }
  // compress: one CABAC decision on cached context lane L (no op pushed)
  AVR_FI int rdecide(uint32_t L) {
    bins++;
    const uint32_t s = __builtin_amdgcn_readlane(rc_v, L);
    uint32_t ns;
    const int b = cd_decide(cd, in, s, crec(s), &ns);
    rc_v = wlane(rc_v, L, ns);
    if (MODE == MODE_TRACE) trace(b, OPK_DECISION, s);
    return b;
  }
  AVR_FI void trace(int b, uint32_t kind, uint32_t s) {
    out_byte(out, (uint32_t)b | kind << 1);
    out_byte(out, s);
  }
  AVR_FI void trace_map_begin(int cat, int n, int max, int is_dc, int c422) {
    const uint32_t y = (uint32_t)mrow();
    out_byte(out, 3u << 1);
    out_byte(out, TRACE_EV_MAP_BEGIN);
    out_byte(out, (uint32_t)mb_x & 0xff);
    out_byte(out, (uint32_t)mb_x >> 8);
    out_byte(out, y & 0xff);
    out_byte(out, y >> 8);
    out_byte(out, (uint32_t)cat);
    out_byte(out, (uint32_t)n);
    out_byte(out, (uint32_t)max);
    out_byte(out, (uint32_t)is_dc | (uint32_t)c422 << 1);
  }
  AVR_FI void trace_map_end() {
    out_byte(out, 3u << 1);
    out_byte(out, TRACE_EV_MAP_END);
  }
  // a residual bin through the model on cached lane L; ctx = rc_addr(rc_cat, L)
  AVR_FI int rbin(uint32_t L, int ctx) {
    if (DEC) {
      const int b = rdecide(L);
      if (MODE == MODE_COMPRESS) push(op_model(b, 0, ctx));
      return b;
    } else if (MODE == MODE_DECOMPRESS) {
      bins++;
      const uint32_t e = __builtin_amdgcn_readlane(rc_v, L);
      const int b = rdec(e);
      rc_v = wlane(rc_v, L, est_update(e, b, 0x60));
      push((uint32_t)b | OPK_DECISION << 1 | (uint32_t)ctx << 3);
      return b;
    } else {
      bins++;
      const uint32_t s = __builtin_amdgcn_readlane(rc_v, L);
      const int b = rnd() < sh->gen_p[ctx];
      uint32_t ns;
      ce_encode(ce, out, b, s, vtab_rec(vt, s), &ns);
      rc_v = wlane(rc_v, L, ns);
      return b;
    }
  }

  // decompress: a residual bin / a bypass bin without its coder op (the macro ops below carry it)
  AVR_FI int rdec_lane(uint32_t L) {
    bins++;
    const uint32_t e = __builtin_amdgcn_readlane(rc_v, L);
    const int b = rdec(e);
    rc_v = wlane(rc_v, L, est_update(e, b, 0x60));
    return b;
  }
  AVR_FI int rdec_mc(int ctx) {   // a macroblock-layer context bin (kMcBase .. + 63)
    bins++;
    const uint32_t L = (uint32_t)(ctx - kMcBase);
    const uint32_t e = __builtin_amdgcn_readlane(mc_v, L);
    const int b = rdec(e);
    mc_v = wlane(mc_v, L, est_update(e, b, 0x60));
    return b;
  }
  AVR_FI int rdec_bypass() {
    bins++;
    const uint32_t e = byp_e;
    const int b = rdec(e);
    byp_e = est_update(e, b, 0x60);
    return b;
  }

  // recoded-decoder probability (recode.cpp:816-820).  The reciprocal comes by a scalar load
  // from the constant table (s_load_dwordx4 into SGPRs, scalar-cache hit): fewer instructions on
  // the walker than three v_readlane pairs and selects from a VGPR table (measured 10 % slower).
  typedef const __attribute__((address_space(4))) uint64_t cu64;
  typedef const __attribute__((address_space(4))) uint32_t cu32;
  AVR_FI auto p1(uint32_t e) const {
    const uint32_t pos = (e & 0xff) + 1, tot = (e & 0xff) + (e >> 8) + 2;   // the sum est_update tests
    if constexpr (!P32) {
      cu64* dv = (cu64*)&G->hot.div[tot][0];
      return (__umul64hi(rd.range, dv[0]) >> (uint32_t)dv[1]) * pos;
    } else {
      return __umulhi(rd.range, ((cu32*)G->hot.rcp32)[tot]) * pos;   // the P-format rule
    }
  }
  // One decision of the model's coder with estimator e (recode.cpp:1435-1449).
  AVR_FI int rdec(uint32_t e) { return rd_get(rd, in, p1(e)); }
  // CABAC state record of state byte s: VGPR table (two v_readlane)
  AVR_FI CabacRec crec(uint32_t s) const {
    return vtab_rec(vt, s);
  }
  AVR_FI void publish() {
    if (RM && gmode) return;
    ring0.publish();
  }
  AVR_FI void push(uint32_t op) {
    if (RM && gmode) {
      if (gsink && __lane_id() == 0) gsink[gcount] = op;
      gcount++;
      return;
    }
    ring0.push(op);
  }
  AVR_FI void push_v(uint32_t op_v, uint32_t n) {
    if (RM && gmode) {
      if (gsink && __lane_id() < n) gsink[gcount + __lane_id()] = op_v;
      gcount += n;
      return;
    }
    ring0.push_v(op_v, n);
  }
#ifdef AVR_PROFILE
  uint64_t prof[8], sprof[8];
  uint32_t profb[8], sprofb[8];
#endif

  // Frame or field significance contexts for the macroblocks that follow: the walker's LDS copy of
  // the ctxIdx bases (rc_addr, sig_map) and the 8x8 ctxIdxInc map in sig8_v (for decompress also
  // the frame map in bits 8-15: the model keys 8x8 positions by the frame map, recode.cpp:703-704,
  // as does T->sig8x8, which is never patched).  Only this wave reads the patched entries.
  AVR_FI void set_fld(int f) {
    if (f == fld) return;
    rc_writeback();
    fld = f;
    const uint32_t L = __lane_id();
    HotTables* t = &sh->tab;
    if (L < 16) t->sig_base[L] = f ? G->sig_base_fld[L] : G->hot.sig_base[L];
    else if (L < 32) t->last_base[L - 16] = f ? G->last_base_fld[L - 16] : G->hot.last_base[L - 16];
    const uint32_t fr = T->sig8x8[L];
    const uint32_t cm = f ? (uint32_t)G->sig8x8_fld[L] : fr;
    sig8_v = (MODE == MODE_DECOMPRESS && FLD) ? (cm | fr << 8) : cm;
    wave_sync();
  }

  // ------------------------------------------------------------------ bins through the model
  // Macroblock-layer contexts kMcBase .. kMcBase + 63 (sub_mb_type, B mb_type, mvd, ref_idx,
  // mb_qp_delta, intra_chroma_pred_mode, prev/rem_intra_pred_mode, coded_block_pattern) stay in
  // one VGPR for the whole slice, lane ctx - kMcBase, like the residual contexts.
  static constexpr int kMcBase = 21;
  uint32_t mc_v;
  AVR_FI void mc_load() {
    const int a = kMcBase + (int)__lane_id();
    mc_v = MODE == MODE_DECOMPRESS ? (uint32_t)sh->est[a] : (uint32_t)sh->state[a];
  }
  AVR_FI void mc_store() {
    const int a = kMcBase + (int)__lane_id();
    if (MODE == MODE_DECOMPRESS) sh->est[a] = (uint16_t)mc_v;
    else sh->state[a] = (uint8_t)mc_v;
    wave_sync();
  }
  AVR_FI int mbin(int se, int k, int ctx) {
    bins++;
    const uint32_t L = (uint32_t)(ctx - kMcBase);
    if (DEC) {
      const uint32_t s = __builtin_amdgcn_readlane(mc_v, L);
      uint32_t ns;
      const int b = cd_decide(cd, in, s, crec(s), &ns);
      mc_v = wlane(mc_v, L, ns);
      if (MODE == MODE_TRACE) trace(b, OPK_DECISION, s);
      else push(op_model(b, 0, ctx));
      return b;
    } else if (MODE == MODE_DECOMPRESS) {
      const uint32_t e = __builtin_amdgcn_readlane(mc_v, L);
      const int b = rdec(e);
      mc_v = wlane(mc_v, L, est_update(e, b, 0x60));
      push((uint32_t)b | OPK_DECISION << 1 | (uint32_t)ctx << 3);
      return b;
    } else {
      const uint32_t s = __builtin_amdgcn_readlane(mc_v, L);
      const int b = gen_bin(se, k, ctx);
      uint32_t ns;
      ce_encode(ce, out, b, s, vtab_rec(vt, s), &ns);
      mc_v = wlane(mc_v, L, ns);
      return b;
    }
  }
  AVR_FI int bin(int se, int k, int ctx) {
    if ((uint32_t)(ctx - kMcBase) < 64u) return mbin(se, k, ctx);
    bins++;
    if (DEC) {
      const uint32_t s = sh->state[ctx];
      uint32_t ns;
      const int b = cd_decide(cd, in, s, crec(s), &ns);
      sh->state[ctx] = (uint8_t)ns;
      if (MODE == MODE_TRACE) trace(b, OPK_DECISION, s);
      else push(op_model(b, 0, ctx));
      return b;
    } else if (MODE == MODE_DECOMPRESS) {
      const uint32_t e = sh->est[ctx];
      const int b = rdec(e);
      sh->est[ctx] = (uint16_t)est_update(e, b, 0x60);
      push((uint32_t)b | OPK_DECISION << 1 | (uint32_t)ctx << 3);
      return b;
    } else {
      int b = gen_bin(se, k, ctx);
      ce_decision(ce, out, b, &sh->state[ctx], T);
      return b;
    }
  }
  AVR_FI int bypass(int se, int k) {
    bins++;
    if (DEC) {
      const int b = cd_bypass(cd, in);
      if (MODE == MODE_TRACE) trace(b, OPK_BYPASS, 0);
      else push(op_model(b, 0, 1024));
      return b;
    } else if (MODE == MODE_DECOMPRESS) {
      const uint32_t e = byp_e;   // the bypass estimator lives in a scalar register
      const int b = rdec(e);
      byp_e = est_update(e, b, 0x60);
      push((uint32_t)b | OPK_BYPASS << 1);
      return b;
    } else {
      int b = gen_bypass(se, k);
      ce_bypass(ce, out, b);
      return b;
    }
  }
  AVR_FI int terminate(int se) {
    bins++;
    int b;
    if (DEC) {
      b = cd_terminate(cd, in);
      if (MODE == MODE_TRACE) {
        trace(b, OPK_TERMINATE, 0);
      } else {
        push(op_model(b, 0, 1025));
        if (b) push(OP_FINISH);
      }
    } else if (MODE == MODE_DECOMPRESS) {
      const uint32_t e = sh->est[1025];
      b = rdec(e);
      sh->est[1025] = (uint16_t)est_update(e, b, 0x60);
      push((uint32_t)b | OPK_TERMINATE << 1);
    } else {
      b = se == SE_EOS ? (mbs_done >= target_mbs || last_mb) : 0;
      ce_terminate(ce, out, b);
    }
    if (b && se == SE_EOS) finished = 1;
    return b;
  }

  // ------------------------------------------------------------------ synthetic bin policy
  AVR_FI uint32_t rnd() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)(rng >> 16) & 0xffff;
  }
  AVR_FI int gen_bin(int se, int k, int ctx) {
    if (se == SE_REF && k >= avr_limit) return 0;
    if (se == SE_QPDELTA && k >= 2) return 0;
    return rnd() < sh->gen_p[ctx];
  }
  AVR_FI int gen_bypass(int se, int k) {
    if ((se == SE_MVD_SUFFIX || se == SE_LEVEL_SUFFIX) && k >= 5 && k < 100) return 0;
    return rnd() & 1;
  }
  int avr_limit;

  // ------------------------------------------------------------------ neighbours (parser)
  AVR_FI const ERec& top() const { return ring[mb_x]; }
  AVR_FI uint16_t nb_cbp_left() const {
    return left_ok ? (lf >> 16) : ((cf & F_INTRA) ? 0x7CF : 0x00F);
  }
  AVR_FI uint16_t nb_cbp_top() const {
    return top_ok ? (tf >> 16) : ((cf & F_INTRA) ? 0x7CF : 0x00F);
  }
  // FFmpeg 4:4:4 8x8 coded_block_flag quirk for x264 < r151 (see oracle_walker.c)
  AVR_FI int nnz_override(uint32_t nbflags, int* v) const {
    if (cat_ != 3 || !(cf & F_T8) || (nbflags & F_T8)) return 0;
    *v = (uint32_t)x264_build < 151u ? ((cf & F_INTRA) ? 64 : 0) : 0;
    return 1;
  }
  AVR_FI int nnz_left(int p, int pw, int x4, int y4) const {
    if (x4 > 0) return sh->cur.nnz[p][y4 * 4 + x4 - 1];
    if (!left_ok) return (cf & F_INTRA) ? 64 : 0;
    int v;
    // MBAFF: rows of one left macroblock come from both macroblocks of the left pair; the view's
    // flags byte holds each row's source 8x8-transform flag
    if (nnz_override((FLD && mbaff) ? (((uint32_t)sh->left.flags >> y4) & 1u) * (uint32_t)F_T8 : lf, &v)) return v;
    return sh->left.nnz[p][y4 * 4 + pw - 1];
  }
  AVR_FI int nnz_top(int p, int x4, int y4) const {
    if (y4 > 0) return sh->cur.nnz[p][(y4 - 1) * 4 + x4];
    if (!top_ok) return (cf & F_INTRA) ? 64 : 0;
    int v;
    if (nnz_override(tf, &v)) return v;
    return ring[mb_x].nnz[p][x4];
  }

  // ------------------------------------------------------------------ MBAFF (field / frame pairs)
  // The per-bin code reads its neighbours from sh->left (the left macroblock), ring[mb_x] (the
  // bottom edge of the upper one) and lf / tf / left_ok / top_ok.  In an MBAFF frame the
  // neighbours of a macroblock follow ITU-T H.264 Table 6-4 (6.4.12.2): rows of the left one may
  // come from either macroblock of the left pair, the upper one depends on the field / frame
  // coding of both pairs, and vertical mvd / ref_idx of a neighbour of the other kind are scaled
  // (9.3.3.1.1.6-7, FFmpeg fill_decode_caches MAP_F2F).  mbaff_view writes exactly that view into
  // sh->left and ring[mb_x] before each coded macroblock, so the per-bin code is the same.
  // LDS of an MBAFF launch (ring_cols >= 3 W + 7): ring[0, W) the views, ring[W + x] /
  // ring[2 W + x] the bottom edges of the last top / bottom macroblock of column x, then three
  // MbRec (this pair's top, the left pair's top and bottom, dword 0 = their cf) and four words:
  // the dword 0 of the left pair's top / bottom and of the upper pair's top / bottom edges.
  static constexpr uint32_t F_FLD = 0x100;   // cf: field macroblock
  static constexpr uint32_t PST_FLD = 1, PST_SKIPT = 2, PST_SKIPB = 4, PST_BOT = 8;
  AVR_FI ERec* pair_edge(int bot) const { return ring + (1 + bot) * W; }
  AVR_FI MbRec* pair_rec() const { return (MbRec*)(ring + 3 * W); }
  AVR_FI uint32_t* pair_nb() const { return (uint32_t*)(pair_rec() + 3); }
  AVR_FI uint32_t lds_u32(const uint32_t* p) const { return __builtin_amdgcn_readfirstlane(*p); }

  // top macroblock of a pair: the neighbour pairs' words and the inferred field flag (7.4.4: the
  // left pair's in the slice, else the upper pair's, else frame)
  AVR_FI void mbaff_pair_start() {
    const uint32_t L = __lane_id();
    uint32_t v = 0;
    if (L < 2) v = mb_x > 0 ? *(const uint32_t*)&pair_rec()[1 + L] : 0u;
    else if (L < 4) v = *(const uint32_t*)&pair_edge((int)L - 2)[mb_x];
    if (L < 4) pair_nb()[L] = v;
    wave_sync();
    const uint32_t lt = __builtin_amdgcn_readlane(v, 0), at = __builtin_amdgcn_readlane(v, 2);
    pst = ((lt & F_DEC) ? (lt & F_FLD) : (at & F_DEC) ? (at & F_FLD) : 0u) ? PST_FLD : 0u;
  }
  // mb_skip_flag ctxIdx (FFmpeg decode_cabac_mb_skip); top_d0 = this pair's top macroblock's cf
  AVR_FI int mbaff_skip_ctx(int bottom, uint32_t fld, uint32_t top_d0) const {
    const uint32_t* nb = pair_nb();
    const uint32_t lt = lds_u32(nb), lb = lds_u32(nb + 1), at = lds_u32(nb + 2), ab = lds_u32(nb + 3);
    uint32_t a = 0, b = 0;
    if (lt & F_DEC) a = (bottom && fld == ((lt & F_FLD) ? 1u : 0u)) ? lb : lt;
    if (fld) {
      if (at & F_DEC) b = (!bottom && (at & F_FLD)) ? at : ab;
    } else {
      b = bottom ? top_d0 : ab;
    }
    return (is_b ? 24 : 11) + ((a & F_DEC) && !(a & F_SKIP)) + ((b & F_DEC) && !(b & F_SKIP));
  }
  // mb_field_decoding_flag, ctxIdx 70-72 (FFmpeg decode_cabac_field_decoding_flag)
  AVR_FI uint32_t mbaff_field_flag(uint32_t inferred) {
    const uint32_t at = lds_u32(pair_nb() + 2);
    return (uint32_t)bin(SE_OTHER, 0, 70 + (mb_x > 0 && inferred) + ((at & F_DEC) && (at & F_FLD)));
  }
  // FFmpeg's order: a skipped top macroblock takes the bottom's skip flag next and, when the bottom
  // is coded, the pair's field flag; a coded top reads the field flag after its skip flag
  AVR_FI int mbaff_skip() {
    const int bottom = (pst & PST_BOT) != 0;
    uint32_t fld = pst & PST_FLD;
    int skip;
    if (bottom && (pst & PST_SKIPT)) skip = (pst & PST_SKIPB) != 0;
    else skip = bin(SE_OTHER, 0, mbaff_skip_ctx(bottom, fld, lds_u32((const uint32_t*)&pair_rec()[0])));
    if (skip && !bottom) {
      pst |= PST_SKIPT;
      if (bin(SE_OTHER, 0, mbaff_skip_ctx(1, fld, F_DEC | F_SKIP))) {
        pst |= PST_SKIPB;
      } else {
        fld = mbaff_field_flag(fld);
        pst = (pst & ~PST_FLD) | fld;
      }
    }
    if (skip && fld) cf |= F_FLD;
    return skip;
  }
  // Table 6-4, xN < 0: the left pair's macroblock (s: 0 top, 1 bottom) and 4x4 row r holding row y4
  // of a plane maxH samples high, for a field (fld) or frame current macroblock and a frame
  // (afrm) or field left pair
  AVR_FI static void left_src(uint32_t fld, int afrm, int bottom, int y4, int maxH, int* s, int* r) {
    const int yN = 4 * y4;
    if (!fld) {
      if (afrm) { *s = bottom; *r = y4; return; }
      *s = 0;
      *r = (bottom ? (yN + maxH) >> 1 : yN >> 1) >> 2;
      return;
    }
    if (afrm) {
      const int y2 = 2 * yN + bottom;
      if (yN < maxH / 2) { *s = 0; *r = y2 >> 2; }
      else { *s = 1; *r = (y2 - maxH) >> 2; }
      return;
    }
    *s = bottom;
    *r = y4;
  }
  // vertical |mvd| bytes (1, 3) and ref_idx bytes of a neighbour of the other coding: a field
  // neighbour of a frame macroblock counts double motion and half the references, and vice versa
  AVR_FI static uint32_t scale_mvd(uint32_t v, uint32_t fld) {
    return fld ? ((v & 0x00ff00ffu) | ((v >> 1) & 0x7f007f00u)) : ((v & 0x00ff00ffu) | ((v & 0xff00ff00u) << 1));
  }
  AVR_FI static uint32_t scale_ref(uint32_t v, uint32_t fld) {
    uint32_t o = 0;
    for (int k = 0; k < 4; k++) {
      int r = (int8_t)(v >> (8 * k));
      if (r >= 0) r = fld ? r * 2 : r >> 1;
      o |= (uint32_t)(uint8_t)r << (8 * k);
    }
    return o;
  }
  AVR_FI void mbaff_view(int bottom, uint32_t fld) {
    set_fld((int)fld);
    nref0 = d->num_ref_idx_l0 << fld;   // a field macroblock addresses fields: twice the references
    nref1 = d->num_ref_idx_l1 << fld;
    const uint32_t L = __lane_id();
    const uint32_t* nb = pair_nb();
    const uint32_t lt = lds_u32(nb), lb = lds_u32(nb + 1), at = lds_u32(nb + 2);
    // ---- left: sh->left, lane j = dword j, gathered from the left pair's records
    left_ok = (lt & F_DEC) != 0;
    if (left_ok) {
      const int afrm = !(lt & F_FLD);
      const MbRec* lp = pair_rec() + 1;
      int s0, r0, s2, r2;
      left_src(fld, afrm, bottom, 0, 16, &s0, &r0);
      left_src(fld, afrm, bottom, 2, 16, &s2, &r2);
      const uint32_t A = s0 ? lb : lt, C = s2 ? lb : lt;
      const uint32_t cbpA = A >> 16, cbpC = C >> 16;
      const uint32_t cbp = (cbpA & 0x7F0u) | (((cbpA >> ((r0 >> 1) * 2 + 1)) & 1u) << 1) |
                           (((cbpC >> ((r2 >> 1) * 2 + 1)) & 1u) << 3);
      lf = (A & 0xffffu) | cbp << 16;
      uint32_t t8rows = 0;
      for (int y4 = 0; y4 < 4; y4++) {
        int sy, ry;
        left_src(fld, afrm, bottom, y4, 16, &sy, &ry);
        t8rows |= (((sy ? lb : lt) & F_T8) ? 1u : 0u) << y4;
      }
      int s = 0, dw = 0;
      if (L >= 1 && L < 13) {          // nnz rows
        const int p = ((int)L - 1) >> 2;
        int r;
        left_src(fld, afrm, bottom, ((int)L - 1) & 3, (cat_ == 1 && p) ? 8 : 16, &s, &r);
        dw = 1 + p * 4 + min(r, 3);
      } else if (L >= 13 && L < 29) {  // mvd rows (two dwords per row)
        const int k = ((int)L - 13) & 7;
        int r;
        left_src(fld, afrm, bottom, k >> 1, 16, &s, &r);
        dw = 13 + (((int)L - 13) >> 3) * 8 + r * 2 + (k & 1);
      } else if (L == 29 || L == 30 || L == 31) {
        s = s0;
        dw = (int)L;
      } else if (L >= 32 && L < 45) {  // model bytes: the left macroblock in the same row
        s = bottom;
        dw = (int)L;
      }
      uint32_t v = L < 45 ? ((const uint32_t*)&lp[s])[dw] : 0u;
      const uint32_t v2 = (L >= 29 && L < 32) ? ((const uint32_t*)&lp[s2])[L] : 0u;
      if (L == 0) {
        v = t8rows | cbp << 16;
      } else if (L >= 13 && L < 29) {
        if (fld != (uint32_t)(!afrm)) v = scale_mvd(v, fld);
      } else if (L == 29 || L == 30 || L == 31) {
        // b8 1 <- row 0's source, b8 3 <- row 2's (the only left 8x8 blocks read: ref_idx / direct
        // of partitions at y4 = 0 and 2)
        const uint32_t b1 = (v >> (8 * ((r0 >> 1) * 2 + 1))) & 0xff, b3 = (v2 >> (8 * ((r2 >> 1) * 2 + 1))) & 0xff;
        v = (L == 31 ? 0u : 0xff00ffu) | b1 << 8 | b3 << 24;
        if (L != 31 && fld != (uint32_t)(!afrm)) v = scale_ref(v, fld);
      }
      if (L < 45) ((uint32_t*)&sh->left)[L] = v;
    }
    // ---- upper: ring[mb_x] from the pair edges (parse neighbour B) + the model's upper macroblock
    const int above = (at & F_DEC) != 0;
    const int sel = !fld ? (bottom ? 1 : above ? 2 : 0) : above ? ((!bottom && (at & F_FLD)) ? 1 : 2) : 0;
    const int msel = bottom ? 1 : above ? 2 : 0;
    uint32_t v = 0;
    if (L < 10 && sel) v = ((const uint32_t*)&pair_edge(sel - 1)[mb_x])[L];
    else if (L >= 10 && L < 23 && msel) v = ((const uint32_t*)&pair_edge(msel - 1)[mb_x])[L];
    const uint32_t t0 = __builtin_amdgcn_readlane(v, 0);
    if (sel && ((t0 & F_FLD) ? 1u : 0u) != fld) {
      if (L >= 4 && L < 8) v = scale_mvd(v, fld);
      else if (L == 8) v = scale_ref(v, fld);
    }
    if (L < 23) ((uint32_t*)&ring[mb_x])[L] = v;
    tf = t0;
    top_ok = sel != 0;
    wave_sync();
  }
  AVR_FI void mbaff_layer_begin() {
    const int bottom = (pst & PST_BOT) != 0;
    uint32_t fld = pst & PST_FLD;
    if (!bottom) {
      fld = mbaff_field_flag(fld);
      pst = (pst & ~PST_FLD) | fld;
    }
    if (fld) cf |= F_FLD;
    mbaff_view(bottom, fld);
  }

  // ------------------------------------------------------------------ model neighbours
  // model num_nonzeros of a neighbouring macroblock (get_neighbor_sub_mb, recode.cpp:419-471)
  AVR_FI int mnnz_left(int idx) const {
    if (RM) return frames[cur_off + ((int64_t)mrow() * W + mb_x - 1) * 52 + idx];
    return left_ok ? sh->left.mnnz[idx] : 0;
  }
  AVR_FI int mnnz_top(int idx) const {
    if (RM) return (FLD && top_pending) ? 0 : frames[cur_off + ((int64_t)(mrow() - 1) * W + mb_x) * 52 + idx];
    // fresh model per slice: in a field picture the model's upper row belongs to the other field
    if (FLD && fld_pic) return 0;
    if constexpr (FLD) {
      return (top_ok | mbaff) ? ring[mb_x].mnnz[idx] : 0;   // MBAFF: the view holds the model's upper macroblock
    } else {
      if (!top_ok) return 0;
      const uint32_t at = (uint32_t)mb_x * (kMringDwords * 4) + mring_dword((uint32_t)idx >> 2) * 4 + ((uint32_t)idx & 3);
      if (mring_global) return (tf & kEdgeMringNz) ? ((const __attribute__((address_space(1))) uint8_t*)mring)[at] : 0;
      return ((const __attribute__((address_space(3))) uint8_t*)mring)[at];
    }
  }
  AVR_FI int mnnz_prev(int idx) const {
    if (RM) return prev_off < 0 ? 0 : frames[prev_off + ((int64_t)mrow() * W + mb_x) * 52 + idx];
    return 0;
  }

  // finished_queueing (recode.cpp:845-930): the 2/4/6 nnz bits, LSB first
  // b2: the block's blk2_v record (BS >= 3: its nb_left / nb_up bytes)
  AVR_FI int nz_bits(int cat, int n, int max, int is_dc, int c422, int count, uint32_t b2 = 0) {
    const int bits = max > 16 ? 6 : max > 4 ? 4 : 2;
    // the R-mode compress's count pass (rscan without a sink) needs the number of ops only: skip
    // the neighbours' frame loads (measured: R-mode compress -2 % clip, -4 % cockatoo)
    if (MODE == MODE_COMPRESS && RM && gmode && !gsink) {
      gcount += (uint32_t)bits;
      return count & ((1 << bits) - 1);
    }
    int has_left, has_above, lv = 0, av = 0;
    if constexpr (BS >= 3) {
      // the same rules on registers: no LDS load before the probe.  A value read for a neighbour
      // that does not exist (mb_x == 0, row 0) is 0 as in the LDS version: mzl_v / mzt_v hold 0
      // where left_ok / top_ok fail, and has_left alone selects lb's third value.
      if (n >= 48) {
        has_left = mb_x > 0;
        lv = (int)__builtin_amdgcn_readlane(mzl_v, (uint32_t)n);
        av = (int)__builtin_amdgcn_readlane(mzt_v, (uint32_t)n);
      } else {
        const uint32_t L = (b2 >> 16) & 0xff, U = b2 >> 24;
        uint32_t li = L & 63, ui = U & 63;
        if (max >= 32) { li &= ~3u; ui &= ~3u; }
        has_left = !(L & 128) || mb_x > 0;
        const uint32_t lc = __builtin_amdgcn_readlane(mz_v, li), ln = __builtin_amdgcn_readlane(mzl_v, li);
        const uint32_t uc = __builtin_amdgcn_readlane(mz_v, ui), un = __builtin_amdgcn_readlane(mzt_v, ui);
        lv = (int)((L & 128) ? ln : lc);
        av = (int)((U & 128) ? un : uc);   // row 0 has no top_ok: un = 0, as av must be without has_above
      }
    } else
    if (n >= 48) {
      has_left = mb_x > 0;
      has_above = mrow() > 0;
      if (has_left) lv = mnnz_left(n);
      if (has_above) av = mnnz_top(n);
    } else {
      uint8_t L = T->nb_left[n], U = T->nb_up[n];
      int li = L & 63, ui = U & 63;
      if (max >= 32) { li &= ~3; ui &= ~3; }
      has_left = !(L & 128) || mb_x > 0;
      has_above = !(U & 128) || mrow() > 0;
      if (has_left) lv = (L & 128) ? mnnz_left(li) : sh->cur.mnnz[li];
      if (has_above) av = (U & 128) ? mnnz_top(ui) : sh->cur.mnnz[ui];
    }
    const int pv = mnnz_prev(n);
    const int t = (((cf & CF_8X8) || max > 32) ? 1 : 0) + 2 * is_dc + c422 + 4 * cat;
    if (MODE == MODE_COMPRESS) {
      // all bits at once, bit i in lane i (so_far = the count's bits below i)
      const int i = (int)__lane_id();
      const int cur_bit = 1 << (i & 7);
      const int so_far = count & (cur_bit - 1);
      const int lb = has_left ? (lv >= cur_bit) : 2;
      const int ab = av ? (av >= cur_bit) : 2;
      const int pb = pv >= cur_bit;
      const int idx = kSigEst + (((((cur_bit - 1 + so_far) * 2 + pb) * 3 + lb) * 3 + ab) * 57 + t);
      push_v(op_model((count >> (i & 7)) & 1, OPM_CACHE, idx), (uint32_t)bits);
      return count & ((1 << bits) - 1);
    }
    if (MODE == MODE_DECOMPRESS) {
      // every key of the bit tree at once (lane (1 << i) - 1 + so_far: bit i after so_far; the
      // keys are distinct), then the bits in order with the estimators already in registers
      const uint32_t L = __lane_id();
      const int i = 31 - __clz((int)L + 1);
      const int cur_bit = 1 << i;
      const int lb = has_left ? (lv >= cur_bit) : 2;
      const int ab = av ? (av >= cur_bit) : 2;
      const int pb = pv >= cur_bit;
      const uint32_t idx_v = kSigEst + ((((L * 2 + pb) * 3 + lb) * 3 + ab) * 57 + t);
      uint32_t e_v = 0, slot_v = 0;
      const bool hit = est_probe4(sh, idx_v, &e_v, &slot_v);   // lanes past the tree are never read
      const uint64_t hit_m = __ballot(hit);
      int so_far = 0;
      for (int k = 0; k < bits; k++) {
        const uint32_t j = (1u << k) - 1 + (uint32_t)so_far;
        const uint32_t idx = __builtin_amdgcn_readlane(idx_v, j);
        uint32_t e, slot;
        if ((hit_m >> j) & 1) {
          e = __builtin_amdgcn_readlane(e_v, j);
          slot = __builtin_amdgcn_readlane(slot_v, j);
        } else {
          e = est_load(sh, est_g, idx, &slot);
        }
        const int b = rdec(e);
        est_store(sh, est_g, idx, slot, est_update(e, b, 0x60));
        so_far |= b << k;
      }
      return so_far;
    }
    int so_far = 0;
    for (int i = 0; i < bits; i++) {
      const int cur_bit = 1 << i;
      const int lb = has_left ? (lv >= cur_bit) : 2;
      const int ab = av ? (av >= cur_bit) : 2;
      const int pb = pv >= cur_bit;
      const int idx = kSigEst + (((((cur_bit - 1 + so_far) * 2 + pb) * 3 + lb) * 3 + ab) * 57 + t);
      int b;
      if (MODE == MODE_COMPRESS) {
        b = (count >> i) & 1;
        push(op_model(b, OPM_CACHE, idx));
      } else {
        uint32_t slot;
        const uint32_t e = est_load(sh, est_g, idx, &slot);
        b = rdec(e);
        est_store(sh, est_g, idx, slot, est_update(e, b, 0x60));
      }
      if (b) so_far |= cur_bit;
    }
    return so_far;
  }

  AVR_FI int sig_est_index(int seb, int max, int is_dc, int c422, int zz, int nnz_m, int obs) const {
    if (max == 64) return seb + (T->sig8x8[zz] * 64 + nnz_m) * 64 + obs;
    int zo = (is_dc && c422) ? (zz < 2 ? 0 : zz < 4 ? 1 : 2) : zz;
    return seb + (zo * 16 + nnz_m) * 16 + obs;
  }

  // significance map of one residual block; returns the coefficient count (b2: the block's blk2_v
  // record, see BS)
  AVR_FI int sig_map(int cat, int n, int max, int is_dc, int c422, uint32_t b2 = 0) {
    const int numc8x8 = cat_ == 2 ? 2 : 1;
    const int sb = T->sig_base[cat], lb = T->last_base[cat], seb = (int)opaque_u32((uint32_t)T->sig_est_base[cat]);
    const int bits = max > 16 ? 6 : max > 4 ? 4 : 2;
    const int mask = (1 << bits) - 1;
    int cnt = 0;
    if (DEC) {
      uint64_t sigmask = 0;
      int pos, end = max - 2;
      PROF_BEGIN(t3);
      if (MODE == MODE_TRACE) trace_map_begin(cat, n, max, is_dc, c422);
      // the loop once per block kind (K: 0 4x4-class, 1 chroma DC, 2 8x8), so that no per-bin
      // code selects between them (one call site, kinds known only at run time)
      auto map_loop = [&](auto K) {
        constexpr int k = decltype(K)::value;
        for (pos = 0; pos < max - 1; pos++) {
          int sc, lc;
          if constexpr (k == 2) {
            sc = (int)__builtin_amdgcn_readlane(sig8_v, (uint32_t)pos);
            lc = (int)__builtin_amdgcn_readlane(last8_v, (uint32_t)pos);
          } else if constexpr (k == 1) {
            sc = lc = min(pos / numc8x8, 2);
          } else {
            sc = lc = pos;
          }
          if (rdecide(sc)) {
            sigmask |= 1ull << pos;
            cnt++;
            if (rdecide(16 + lc)) { end = pos; break; }
          }
        }
      };
      if (max == 64) map_loop(std::integral_constant<int, 2>());
      else if (cat == 3) map_loop(std::integral_constant<int, 1>());
      else map_loop(std::integral_constant<int, 0>());
      if (pos == max - 1) cnt++;
      if (MODE == MODE_TRACE) trace_map_end();
      PROF_END(3, t3);
      if (MODE == MODE_COMPRESS) {
        // model: nnz first (recode.cpp:1208-1221), then the buffered map (1244-1255)
        PROF_BEGIN(t4);
        nz_bits(cat, n, max, is_dc, c422, cnt, b2);
        PROF_END(4, t4);
        PROF_BEGIN(t5);
        const int nnz_m = cnt & mask;
        // positions 0..end at once, position zz in lane zz (obs = significant positions before it)
        const int zz = (int)__lane_id();
        const int b = (int)((sigmask >> zz) & 1);
        const int obs = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(sigmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sigmask, 0u));
        const int idx = sig_est_index(seb, max, is_dc, c422, zz, nnz_m, obs);
        push_v(op_model(b, OPM_CACHE | OPM_THR50, idx), (uint32_t)end + 1);
        PROF_END(5, t5);
      }
    } else if (MODE == MODE_DECOMPRESS) {
      PROF_BEGIN(t4);
      const int nnz_m = nz_bits(cat, n, max, is_dc, c422, 0, b2);   // recode.cpp:1476-1486
      PROF_END(4, t4);
      PROF_BEGIN(t3);
      int pos;
      // the coder ops of the map's bins: scalar bases, one add of (ctxIdxInc << 3) + bin each
      const uint32_t sop = opaque_u32((uint32_t)sb << 3 | OPK_DECISION << 1 | 1u << OPC_SHIFT_D);
      const uint32_t lop = opaque_u32((uint32_t)lb << 3 | OPK_DECISION << 1 | 2u << OPC_SHIFT_D);
      // one loop per block kind (K: 0 4x4-class, 1 chroma DC, 2 8x8; see the DEC side)
      auto map_loop = [&](auto K) {
        constexpr int k = decltype(K)::value;
        constexpr int stride = k == 2 ? 64 : 16;
        uint32_t mk = 0;   // progressive walker: the significance bits of this 16-position segment
        // 4x4-class maps key each position's estimator by the position itself, so no key repeats
        // within the map: the LDS write-backs wait in two VGPRs (lane = position) for one store
        // after the loop (a new key claims its slot at once, est_load).  Chroma DC and 8x8 maps
        // reuse keys within the map and store at once.
        constexpr bool defer = k == 0;
        uint32_t dslot_v = 0, de_v = 0;
        for (pos = 0; pos < max - 1; pos++) {
          int sc, lc, zo;
          if constexpr (k == 2) {
            const uint32_t v = __builtin_amdgcn_readlane(sig8_v, (uint32_t)pos);   // CABAC inc | key inc << 8 (FLD)
            sc = FLD ? (int)(v & 0xff) : (int)v;
            zo = FLD ? (int)(v >> 8) : (int)v;
            lc = (int)__builtin_amdgcn_readlane(last8_v, (uint32_t)pos);
          } else if constexpr (k == 1) {
            sc = lc = min(pos / numc8x8, 2);
            zo = (is_dc && c422) ? (pos < 2 ? 0 : pos < 4 ? 1 : 2) : pos;
          } else {
            sc = lc = zo = pos;
          }
          const int idx = seb + (zo * stride + nnz_m) * stride + cnt;   // sig_est_index
          uint32_t slot;
          uint32_t e = est_load(sh, est_g, idx, &slot, defer);
          int b = rdec(e);
          const uint32_t ne = est_update(e, b, 0x50);
          if (defer && AVR_LIKELY(slot >> 31)) {
            dslot_v = wlane(dslot_v, (uint32_t)pos, slot);
            de_v = wlane(de_v, (uint32_t)pos, ne);
          } else {
            est_store(sh, est_g, idx, slot, ne);
          }
          bins++;
          if constexpr (FLD) push(sop + ((uint32_t)sc << 3) + (uint32_t)b);
          else mk |= (uint32_t)b << (pos & 15);
          if (b) {
            cnt++;
            int last = nnz_m == cnt;   // derived EOB (recode.cpp:1437-1438)
            bins++;
            if constexpr (FLD) push(lop + ((uint32_t)lc << 3) + (uint32_t)last);
            if (last) break;
          }
          if constexpr (!FLD && k == 2) {
            if ((pos & 15) == 15) {
              push(op_map(cat, 16, 0, mk));
              mk = 0;
            }
          }
        }
        if constexpr (defer) {
          if (dslot_v >> 31) sh->etab[dslot_v & 0xffff] = (dslot_v & 0xffff0000u) | de_v;
          wave_sync();
        }
        if constexpr (!FLD) {
          const int ended = pos < max - 1;
          push(op_map(cat, (pos & 15) + ended, ended, mk));
        }
      };
      if (max == 64) map_loop(std::integral_constant<int, 2>());
      else if (cat == 3) map_loop(std::integral_constant<int, 1>());
      else map_loop(std::integral_constant<int, 0>());
      if (pos == max - 1) cnt++;
      PROF_END(3, t3);
    } else {
      int pos;
      for (pos = 0; pos < max - 1; pos++) {
        int sc, lc;
        if (max == 64) {
          sc = (int)__builtin_amdgcn_readlane(sig8_v, (uint32_t)pos);
          lc = (int)__builtin_amdgcn_readlane(last8_v, (uint32_t)pos);
        }
        else if (cat == 3) { sc = lc = min(pos / numc8x8, 2); }
        else sc = lc = pos;
        if (rbin(sc, sb + sc)) {
          cnt++;
          if (rbin(16 + lc, lb + lc)) break;
        }
      }
      if (pos == max - 1) cnt++;
    }
    return cnt;
  }

  // residual_block_cabac() of one block; p/x4/y4 locate it in the walker's nnz grid
  // (b2: the block's blk2_v record, BS >= 2)
  AVR_FI void residual_block(int cat, int n, int max, int is_dc, int c422, int p, int pw, int x4, int y4, uint32_t b2 = 0) {
    if (AVR_MB_UNLIKELY(err)) return;
    MbRec& cur = sh->cur;
    int coded = 1;
    if (max != 64 || cat_ == 3) {
      int nza, nzb;
      if (is_dc) {
        int bit = cat == 3 ? (0x40 << (n - 49)) : (0x100 << (n - 48));
        nza = (nb_cbp_left() & bit) != 0;
        nzb = (nb_cbp_top() & bit) != 0;
      } else if constexpr (BS >= 2) {
        // both registers at the neighbour's lane, then the one the record names
        const uint32_t ll = b2 & 63, tl = (b2 >> 8) & 63;
        const uint32_t lc = __builtin_amdgcn_readlane(nz_v, ll), ln = __builtin_amdgcn_readlane(nzn_v, ll);
        const uint32_t tc = __builtin_amdgcn_readlane(nz_v, tl), tn = __builtin_amdgcn_readlane(nzn_v, tl);
        nza = ((b2 & 0x40) ? ln : lc) > 0;
        nzb = ((b2 & 0x4000) ? tn : tc) > 0;
      } else {
        nza = nnz_left(p, pw, x4, y4) > 0;
        nzb = nnz_top(p, x4, y4) > 0;
      }
      rc_select(cat);
      coded = rbin(42 + nza + 2 * nzb, T->cbf_base[cat] + nza + 2 * nzb);
    }
    int cnt = 0;
    if (coded) {
      rc_select(cat);
      cnt = sig_map(cat, n, max, is_dc, c422, b2);
      // coeff_abs_level_minus1 + sign, reverse scan order
      const int ab = (int)opaque_u32((uint32_t)T->abs_base[cat]);   // scalar: the coder ops' base
      int gt1 = 0, eq1 = 0;
      PROF_BEGIN(t6);
      if constexpr (MODE == MODE_DECOMPRESS && !FLD) {
        // one coder op per coefficient (op_level): the coder derives the level bins' contexts
        for (int i = cnt - 1; i >= 0 && !err; i--) {
          int absl;
          const int i0 = gt1 ? 0 : min(4, 1 + eq1);
          if (!rdec_lane(32 + i0)) {
            absl = 1;
          } else {
            const int i1 = 5 + min(4 - (cat == 3), gt1);
            absl = 2;
            while (absl < 15 && rdec_lane(32 + i1)) absl++;
          }
          if (absl < 15) {
            push(op_level(cat, absl, rdec_bypass()));
          } else {   // escape: the prefix as one op, suffix and sign bin by bin
            push(op_level(cat, 15, 0));
            int k = 0;
            while (bypass(SE_LEVEL_SUFFIX, k)) {
              if (++k > 30) { err = AVR_SLICE_BAD_LEVEL; break; }
            }
            while (k-- > 0) bypass(SE_LEVEL_SUFFIX, 100);
            bypass(SE_OTHER, 0);
          }
          if (absl == 1) eq1++;
          else gt1++;
        }
      } else if constexpr (MODE == MODE_COMPRESS && kStageLevels) {
        // the block's level ops staged in a VGPR and stored together after the block
        const bool st = !(RM && gmode);
        auto lpush = [&](uint32_t op) {
          if (st) ring0.stage(op);
          else push(op);
        };
        auto lbyp = [&]() {
          bins++;
          const int b = cd_bypass(cd, in);
          lpush(op_model(b, 0, 1024));
          return b;
        };
        for (int i = cnt - 1; i >= 0 && !err; i--) {
          int absl;
          const int i0 = gt1 ? 0 : min(4, 1 + eq1);
          int b = rdecide(32 + i0);
          lpush(op_model(b, 0, ab + i0));
          if (!b) {
            absl = 1;
          } else {
            const int i1 = 5 + min(4 - (cat == 3), gt1);
            absl = 2;
            while (absl < 15) {
              b = rdecide(32 + i1);
              lpush(op_model(b, 0, ab + i1));
              if (!b) break;
              absl++;
            }
            if (absl >= 15) {
              int k = 0;
              while (lbyp()) {
                if (++k > 30) { err = AVR_SLICE_BAD_LEVEL; break; }
              }
              while (k-- > 0) lbyp();
            }
          }
          lbyp();
          if (absl == 1) eq1++;
          else gt1++;
        }
        if (st) ring0.flush_stage();
      } else
      for (int i = cnt - 1; i >= 0 && !err; i--) {
        int absl;
        const int i0 = gt1 ? 0 : min(4, 1 + eq1);
        if (!rbin(32 + i0, ab + i0)) {
          absl = 1;
        } else {
          const int i1 = 5 + min(4 - (cat == 3), gt1);
          absl = 2;
          while (absl < 15 && rbin(32 + i1, ab + i1)) absl++;
          if (absl >= 15) {
            int k = 0;
            while (bypass(SE_LEVEL_SUFFIX, k)) {
              if (++k > 30) { err = AVR_SLICE_BAD_LEVEL; break; }
            }
            int v = 1;
            while (k-- > 0) v += v + bypass(SE_LEVEL_SUFFIX, 100);
            absl = 14 + v;
          }
        }
        bypass(SE_OTHER, 0);
        if (absl == 1) eq1++;
        else gt1++;
      }
      PROF_END(6, t6);
      // end_coding_type recount (recode.cpp:935-947)
      if constexpr (BS >= 3) mz_v = wlane(mz_v, (uint32_t)n, (uint32_t)cnt);
      else cur.mnnz[n] = (uint8_t)cnt;
      if (max > 32) cf |= CF_8X8;
    }
    if (is_dc) {
      if (cnt) cf |= (uint32_t)(cat == 3 ? (0x40 << (n - 49)) : (0x100 << (n - 48))) << 16;
    } else if constexpr (BS >= 2) {
      // an uncoded block leaves its lanes at the macroblock's initial 0 (each block is coded once)
      if (cnt) {
        const uint32_t g = (uint32_t)(p * 16 + y4 * 4 + x4);
        nz_v = wlane(nz_v, g, (uint32_t)cnt);
        if (max == 64) {
          nz_v = wlane(nz_v, g + 1, (uint32_t)cnt);
          nz_v = wlane(nz_v, g + 4, (uint32_t)cnt);
          nz_v = wlane(nz_v, g + 5, (uint32_t)cnt);
        }
      }
    } else if (max == 64) {
      cur.nnz[p][y4 * 4 + x4] = cur.nnz[p][y4 * 4 + x4 + 1] = (uint8_t)cnt;
      cur.nnz[p][y4 * 4 + 4 + x4] = cur.nnz[p][y4 * 4 + 4 + x4 + 1] = (uint8_t)cnt;
    } else {
      cur.nnz[p][y4 * 4 + x4] = (uint8_t)cnt;
    }
  }

  AVR_FI void blk_pos(int n, int* x4, int* y4) const {
    int s = c_scan8[n];
    int row = s >> 3;
    *x4 = (s & 7) - 4;
    *y4 = row <= 4 ? row - 1 : row <= 9 ? row - 6 : row - 11;
  }

  // The macroblock's residual blocks in bitstream order (residual(), 7.3.5.3) are listed in LDS
  // first and then coded through ONE inlined residual_block site, so the per-bin code exists
  // once in the kernel instead of once per block kind.
  AVR_FI int push_block(int nb, int cat, int n, int max, int is_dc, int c422, int p, int pw, int x4, int y4) {
    sh->blk[nb] = (uint32_t)cat | (uint32_t)n << 4 | (uint32_t)max << 10 | (uint32_t)is_dc << 17 |
                  (uint32_t)c422 << 18 | (uint32_t)p << 19 | (uint32_t)pw << 21 | (uint32_t)x4 << 24 |
                  (uint32_t)y4 << 26;
    return nb + 1;
  }
  AVR_FI int list_luma(int nb, int p, int i16, int cbp) {
    const int cat_dc = p == 0 ? 0 : p == 1 ? 6 : 10;
    const int cat_ac = cat_dc + 1, cat_4 = cat_dc + 2, cat_8 = p == 0 ? 5 : p == 1 ? 9 : 13;
    int x4, y4;
    if (i16) {
      nb = push_block(nb, cat_dc, 48 + p, 16, 1, 0, p, 4, 0, 0);
      if (cbp & 15)
        for (int i = 0; i < 16; i++) {
          blk_pos(16 * p + i, &x4, &y4);
          nb = push_block(nb, cat_ac, 16 * p + i, 15, 0, 0, p, 4, x4, y4);
        }
      return nb;
    }
    for (int i8 = 0; i8 < 4; i8++) {
      if (!(cbp & (1 << i8))) continue;
      if (cf & F_T8) {
        blk_pos(16 * p + 4 * i8, &x4, &y4);
        nb = push_block(nb, cat_8, 16 * p + 4 * i8, 64, 0, 0, p, 4, x4, y4);
      } else {
        for (int i4 = 0; i4 < 4; i4++) {
          int n = 16 * p + 4 * i8 + i4;
          blk_pos(n, &x4, &y4);
          nb = push_block(nb, cat_4, n, 16, 0, 0, p, 4, x4, y4);
        }
      }
    }
    return nb;
  }

  // BS >= 1: the same list, record j computed by lane j (blk_v / blk2_v; returns the block count).
  // Per luma-like plane (plane 0, or 0-2 in 4:4:4) the list holds np records: Intra16x16 its DC
  // block and, with cbp & 15, its 16 AC blocks; else one 8x8 block (F_T8) or four 4x4 blocks per set
  // bit of cbp & 15.  Then, 4:2:0 / 4:2:2: two chroma DC blocks (cbp & 0x30) and 2 x 4 or 2 x 8 chroma
  // AC blocks (cbp & 0x20).  A block's position in its plane is blk_pos's: with i = n & 15 the c_scan8
  // entries give x4 = (i & 1) | (i >> 1 & 2), y4 = (i >> 1 & 1) | (i >> 2 & 2) in every plane.
  AVR_FI int list_build(int i16, int cbp) {
    const int j = (int)__lane_id();
    const int t8 = (cf & F_T8) != 0, m4 = cbp & 15;
    const int np = i16 ? (m4 ? 17 : 1) : __builtin_popcount((uint32_t)m4) << (t8 ? 0 : 2);
    const int nluma = cat_ == 3 ? 3 * np : np;
    const int c422 = cat_ == 2, chroma = cat_ == 1 || cat_ == 2;
    const int ndc = (chroma && (cbp & 0x30)) ? 2 : 0, per = c422 ? 8 : 4;
    const int nac = (chroma && (cbp & 0x20)) ? 2 * per : 0;
    // a luma-like lane
    const int p = (j >= np) + (j >= 2 * np), k = j - p * np;
    const int cat_dc = p == 0 ? 0 : p == 1 ? 6 : 10;
    int cat, i, max, is_dc = 0;
    if (i16) {
      is_dc = k == 0;
      i = is_dc ? 0 : k - 1;
      cat = cat_dc + !is_dc;
      max = is_dc ? 16 : 15;
    } else {
      const int q = t8 ? k : k >> 2;   // the block's 8x8 is the q-th set bit of cbp & 15
      int i8 = 0;
      for (int b = 1; b < 4; b++)
        if (((m4 >> b) & 1) && __builtin_popcount((uint32_t)(m4 & ((1 << b) - 1))) == q) i8 = b;
      i = 4 * i8 + (t8 ? 0 : (k & 3));
      cat = t8 ? (p == 0 ? 5 : p == 1 ? 9 : 13) : cat_dc + 2;
      max = t8 ? 64 : 16;
    }
    int n = is_dc ? 48 + p : 16 * p + i, pl = p, pw = 4, dc422 = 0;
    // a chroma lane
    if (j >= nluma) {
      const int jc = j - nluma;
      if (jc < ndc) {
        cat = 3; n = 49 + jc; max = per; is_dc = 1; dc422 = c422; pl = 1 + jc; i = 0;
      } else {
        const int ja = jc - ndc, c = ja >= per, jp = ja - c * per;
        i = (jp & 3) + 8 * (jp >> 2);   // 4:2:2: the plane's second 8x8 is blocks 8-11
        cat = 4; n = 16 + 16 * c + i; max = 15; is_dc = 0; pl = 1 + c;
      }
      pw = 2;
    }
    const int x4 = (i & 1) | ((i >> 1) & 2), y4 = ((i >> 1) & 1) | ((i >> 2) & 2);
    blk_v = (uint32_t)cat | (uint32_t)n << 4 | (uint32_t)max << 10 | (uint32_t)is_dc << 17 | (uint32_t)dc422 << 18 |
            (uint32_t)x4 << 19 | (uint32_t)y4 << 21 | (uint32_t)pl << 23 | (uint32_t)pw << 25;
    if constexpr (BS >= 2) {
      const int g = pl * 16 + y4 * 4 + x4;
      const uint32_t l = x4 > 0 ? (uint32_t)(g - 1) : 0x40u | (uint32_t)(pl * 8 + y4);
      const uint32_t u = y4 > 0 ? (uint32_t)(g - 4) : 0x40u | (uint32_t)(pl * 8 + 4 + x4);
      uint32_t v = l | u << 8;
      if constexpr (BS >= 3) {
        const int nt = n < 48 ? n : 0;   // the DC blocks do not use the tables (48 entries)
        const uint32_t tb = (uint32_t)T->nb_left[nt] << 16 | (uint32_t)T->nb_up[nt] << 24;
        v |= n < 48 ? tb : 0u;
      }
      blk2_v = v;
    }
    return nluma + ndc + nac;
  }

  // BS >= 2: the neighbours of the macroblock's nnz grids, once per macroblock.  Called at the entry
  // of residual(), after the macroblock's transform_size_8x8_flag is known (both of the macroblock
  // layer's places for it precede residual()): nnz_override depends on the current F_T8.  Everything
  // else read here (sh->left, ring[mb_x], the model row, lf / tf, left_ok / top_ok) was final at the
  // macroblock's start; a macroblock without residual() needs none of it.
  AVR_FI void edge_load() {
    const uint32_t L = __lane_id();
    {
      const uint32_t pl = (L >> 3) < 3 ? L >> 3 : 2, r = L & 7;   // lanes >= 24: plane 2 again, never read
      const int dflt = (cf & F_INTRA) ? 64 : 0;
      const int pwp = (pl && (cat_ == 1 || cat_ == 2)) ? 2 : 4;
      int ov_l = 0, ov_t = 0;
      const int has_ov_l = nnz_override(lf, &ov_l), has_ov_t = nnz_override(tf, &ov_t);
      const int lval = sh->left.nnz[pl][(r & 3) * 4 + pwp - 1], tval = ring[mb_x].nnz[pl][r & 3];
      const int lres = !left_ok ? dflt : has_ov_l ? ov_l : lval;
      const int tres = !top_ok ? dflt : has_ov_t ? ov_t : tval;
      nzn_v = (uint32_t)(r < 4 ? lres : tres);
    }
    if constexpr (BS >= 3) {
      const uint32_t idx = L < 52 ? L : 51;
      const uint32_t lval = sh->left.mnnz[idx];
      mzl_v = (left_ok && L < 52) ? lval : 0u;
      // the upper macroblock's model bytes (mnnz_top): the kept dwords of the column's row
      const bool kept = L < 52 && ((kMringUsed >> (L >> 2)) & 1);
      const uint32_t at = (uint32_t)mb_x * (kMringDwords * 4) + mring_dword(idx >> 2) * 4 + (idx & 3);
      uint32_t tval = 0;
      if (kept && top_ok) {
        if (mring_global) {
          if (tf & kEdgeMringNz) tval = ((const __attribute__((address_space(1))) uint8_t*)mring)[at];
        } else {
          tval = ((const __attribute__((address_space(3))) uint8_t*)mring)[at];
        }
      }
      mzt_v = tval;
    }
  }

  AVR_FI void residual(int i16, int cbp) {
    if constexpr (BS >= 1) {
      const int nb = list_build(i16, cbp);
      if constexpr (BS >= 2) edge_load();
      PROF_BEGIN(t2);
      for (int j = 0; j < nb && AVR_MB_LIKELY(!err); j++) {
        const uint32_t b = __builtin_amdgcn_readlane(blk_v, (uint32_t)j);
        const uint32_t b2 = BS >= 2 ? __builtin_amdgcn_readlane(blk2_v, (uint32_t)j) : 0u;
        // BS >= 2: residual_block needs the block's grid lane g only, passed whole as x4
        if constexpr (BS >= 2)
          residual_block(b & 15, (b >> 4) & 63, (b >> 10) & 127, (b >> 17) & 1, (b >> 18) & 1, 0, 0, (b >> 19) & 63, 0, b2);
        else
          residual_block(b & 15, (b >> 4) & 63, (b >> 10) & 127, (b >> 17) & 1, (b >> 18) & 1, (b >> 23) & 3,
                         (b >> 25) & 7, (b >> 19) & 3, (b >> 21) & 3);
      }
      PROF_END(2, t2);
      return;
    }
    int nb = list_luma(0, 0, i16, cbp);
    if (cat_ == 3) {
      nb = list_luma(nb, 1, i16, cbp);
      nb = list_luma(nb, 2, i16, cbp);
    } else if (cat_ == 1 || cat_ == 2) {
      const int c422 = cat_ == 2;
      if (cbp & 0x30)
        for (int c = 0; c < 2; c++) nb = push_block(nb, 3, 49 + c, c422 ? 8 : 4, 1, c422, 1 + c, 2, 0, 0);
      if (cbp & 0x20)
        for (int c = 0; c < 2; c++)
          for (int i8 = 0; i8 < (c422 ? 2 : 1); i8++)
            for (int i = 0; i < 4; i++) {
              int n = 16 + 16 * c + 8 * i8 + i, x4, y4;
              blk_pos(n, &x4, &y4);
              nb = push_block(nb, 4, n, 15, 0, 0, 1 + c, 2, x4, y4);
            }
    }
    PROF_BEGIN(t2);
    for (int j = 0; j < nb && AVR_MB_LIKELY(!err); j++) {
      const uint32_t b = sh->blk[j];
      residual_block(b & 15, (b >> 4) & 63, (b >> 10) & 127, (b >> 17) & 1, (b >> 18) & 1, (b >> 19) & 3,
                     (b >> 21) & 7, (b >> 24) & 3, (b >> 26) & 3);
    }
    PROF_END(2, t2);
  }

  // ------------------------------------------------------------------ prediction syntax
  AVR_FI int ref_gt0(int list, int x4, int y4, int use_left) const {
    uint8_t dir;
    int r;
    if (use_left) {
      if (x4 > 0) {
        int b8 = (y4 >> 1) * 2 + ((x4 - 1) >> 1);
        dir = sh->cur.direct8[b8]; r = sh->cur.ref[list][b8];
      } else {
        if (!left_ok) return 0;
        int b8 = (y4 >> 1) * 2 + 1;
        dir = sh->left.direct8[b8]; r = sh->left.ref[list][b8];
      }
    } else {
      if (y4 > 0) {
        int b8 = ((y4 - 1) >> 1) * 2 + (x4 >> 1);
        dir = sh->cur.direct8[b8]; r = sh->cur.ref[list][b8];
      } else {
        if (!top_ok) return 0;
        dir = ring[mb_x].direct8[x4 >> 1]; r = ring[mb_x].ref[list][x4 >> 1];
      }
    }
    if (is_b && dir) return 0;
    return r > 0;
  }
  AVR_FI int decode_ref(int list, int x4, int y4) {
    int ctx = ref_gt0(list, x4, y4, 1) + 2 * ref_gt0(list, x4, y4, 0);
    int ref = 0;
    avr_limit = (list ? nref1 : nref0) - 1;
    while (bin(SE_REF, ref, 54 + ctx)) {
      ref++;
      ctx = (ctx >> 2) + 4;
      if (ref >= 32) { err = AVR_SLICE_BAD_REF_IDX; return 0; }
    }
    return ref;
  }
  AVR_FI int mvd_nb(int list, int comp, int x4, int y4, int use_left) const {
    if (use_left) {
      if (x4 > 0) return sh->cur.mvd[list][y4 * 4 + x4 - 1][comp];
      return left_ok ? sh->left.mvd[list][y4 * 4 + 3][comp] : 0;
    }
    if (y4 > 0) return sh->cur.mvd[list][(y4 - 1) * 4 + x4][comp];
    return top_ok ? ring[mb_x].mvd[list][x4][comp] : 0;
  }
  AVR_FI int decode_mvd(int list, int comp, int x4, int y4) {
    const int base = comp ? 47 : 40;
    const int amvd = mvd_nb(list, comp, x4, y4, 1) + mvd_nb(list, comp, x4, y4, 0);
    const int inc = amvd < 3 ? 0 : amvd <= 32 ? 1 : 2;
    if constexpr (MODE == MODE_DECOMPRESS && !FLD) {   // one op_mvd (+ an escape's bins)
      if (!rdec_mc(base + inc)) {
        push(op_mvd(comp, inc, 0, 0));
        return 0;
      }
      int mvd = 1, ctx = base + 3;
      while (mvd < 9 && rdec_mc(ctx)) {
        if (mvd < 4) ctx++;
        mvd++;
      }
      if (mvd < 9) {
        push(op_mvd(comp, inc, mvd, rdec_bypass()));
        return mvd;
      }
      push(op_mvd(comp, inc, 9, 0));
      int k = 3;
      while (bypass(SE_MVD_SUFFIX, k - 3)) {
        mvd += 1 << k;
        if (++k > 24) { err = AVR_SLICE_BAD_MVD; return 0; }
      }
      while (k--) mvd += bypass(SE_MVD_SUFFIX, 100) << k;
      bypass(SE_OTHER, 0);
      return mvd < 70 ? mvd : 70;
    }
    if (!bin(SE_OTHER, 0, base + inc)) return 0;
    int mvd = 1, ctx = base + 3;
    while (mvd < 9 && bin(SE_OTHER, 0, ctx)) {
      if (mvd < 4) ctx++;
      mvd++;
    }
    if (mvd >= 9) {
      int k = 3;
      while (bypass(SE_MVD_SUFFIX, k - 3)) {
        mvd += 1 << k;
        if (++k > 24) { err = AVR_SLICE_BAD_MVD; return 0; }
      }
      while (k--) mvd += bypass(SE_MVD_SUFFIX, 100) << k;
    }
    bypass(SE_OTHER, 0);
    return mvd < 70 ? mvd : 70;
  }
  AVR_FI void mvd_part(int list, int px, int py, int pw, int ph) {
    int mx = decode_mvd(list, 0, px, py);
    int my = decode_mvd(list, 1, px, py);
    for (int y = py; y < py + ph; y++)
      for (int x = px; x < px + pw; x++) {
        sh->cur.mvd[list][y * 4 + x][0] = (uint8_t)mx;
        sh->cur.mvd[list][y * 4 + x][1] = (uint8_t)my;
      }
  }

  AVR_FI int intra_mb_type(int base, int intra_slice, int* i16_cbp) {
    // returns 0 = I_NxN, 1 = I_16x16, 2 = I_PCM
    int ctx = 0;
    if (intra_slice) {
      if (left_ok && (lf & F_I16)) ctx++;
      if (top_ok && (tf & F_I16)) ctx++;
      if (!bin(SE_OTHER, 0, base + ctx)) return 0;
      base += 2;
    } else {
      if (!bin(SE_OTHER, 0, base)) return 0;
    }
    if (terminate(SE_PCM)) return 2;
    int luma = bin(SE_OTHER, 0, base + 1) ? 15 : 0;
    int chroma = 0;
    if (bin(SE_OTHER, 0, base + 2)) chroma = 1 + bin(SE_OTHER, 0, base + 2 + intra_slice);
    bin(SE_OTHER, 0, base + 3 + intra_slice);
    bin(SE_OTHER, 0, base + 3 + 2 * intra_slice);
    *i16_cbp = luma | (chroma << 4);
    return 1;
  }

  // ------------------------------------------------------------------ one macroblock
  AVR_FI void decode_mb() {
    MbRec& cur = sh->cur;
    const int nlists = is_b ? 2 : 1;
    PROF_BEGIN(ps1);
    if (slice_type != 2) {
      int skip;
      if (FLD && mbaff) skip = mbaff_skip();
      else skip = bin(SE_OTHER, 0, (is_b ? 24 : 11) + (left_ok && !(lf & F_SKIP)) + (top_ok && !(tf & F_SKIP)));
      if (skip) {
        cf |= F_SKIP;
        if (is_b) {
          cf |= F_D16;
          cur.direct8[0] = cur.direct8[1] = cur.direct8[2] = cur.direct8[3] = 1;
        } else {
          cur.ref[0][0] = cur.ref[0][1] = cur.ref[0][2] = cur.ref[0][3] = 0;
        }
        last_dqp_nz = 0;
        SPROF_END(1, ps1);
        return;
      }
    }
    if (FLD && mbaff) mbaff_layer_begin();
    SPROF_END(1, ps1);
    PROF_BEGIN(ps2);
    // mb_type
    int intra = 0, kind = 0, i16_cbp = 0, nparts = 0, vertical = 0, pred0 = 0, pred1 = 0, direct16 = 0;
    if (slice_type == 2) {
      intra = 1;
      kind = intra_mb_type(3, 1, &i16_cbp);
    } else if (slice_type == 0) {
      if (!bin(SE_OTHER, 0, 14)) {
        int mt;
        if (!bin(SE_OTHER, 0, 15)) mt = 3 * bin(SE_OTHER, 0, 16);
        else mt = 2 - bin(SE_OTHER, 0, 17);
        if (mt == 0) { nparts = 1; pred0 = 1; }
        else if (mt == 1) { nparts = 2; pred0 = pred1 = 1; }
        else if (mt == 2) { nparts = 2; vertical = 1; pred0 = pred1 = 1; }
        else nparts = 4;
      } else {
        intra = 1;
        kind = intra_mb_type(17, 0, &i16_cbp);
      }
    } else {
      int ctx = (left_ok && !(lf & F_D16)) + (top_ok && !(tf & F_D16));
      if (!bin(SE_OTHER, 0, 27 + ctx)) {
        direct16 = 1;
        nparts = 4;
      } else if (!bin(SE_OTHER, 0, 27 + 3)) {
        nparts = 1;
        pred0 = 1 + bin(SE_OTHER, 0, 27 + 5);
      } else {
        int bits = bin(SE_OTHER, 0, 27 + 4) << 3;
        bits |= bin(SE_OTHER, 0, 27 + 5) << 2;
        bits |= bin(SE_OTHER, 0, 27 + 5) << 1;
        bits |= bin(SE_OTHER, 0, 27 + 5);
        int mt = -1;
        if (bits < 8) mt = bits + 3;
        else if (bits == 13) { intra = 1; kind = intra_mb_type(32, 0, &i16_cbp); }
        else if (bits == 14) mt = 11;
        else if (bits == 15) mt = 22;
        else mt = ((bits << 1) | bin(SE_OTHER, 0, 27 + 5)) - 4;
        if (!intra) {
          if (mt == 3) { nparts = 1; pred0 = 3; }
          else if (mt == 22) nparts = 4;
          else {
            int k = mt - 4;
            nparts = 2;
            vertical = k & 1;
            pred0 = c_b_pairs[k >> 1][0];
            pred1 = c_b_pairs[k >> 1][1];
          }
        }
      }
    }
    SPROF_END(2, ps2);
    if (err) return;
    if (intra && kind == 2) { err = AVR_SLICE_PCM; return; }  // I_PCM (skip_bytes hook, recode.cpp:161-163)
    int no_sub_lt8x8 = 1;
    int t8 = 0;
    PROF_BEGIN(ps3);
    if (intra) {
      cf |= F_INTRA;
      if (kind == 1) cf |= F_I16;
      if (kind == 0) {
        if (t8mode) {
          t8 = bin(SE_OTHER, 0, 399 + (left_ok && (lf & F_T8)) + (top_ok && (tf & F_T8)));
          if (t8) cf |= F_T8;
        }
        const int nmodes = t8 ? 4 : 16;
        for (int i = 0; i < nmodes; i++)
          if (!bin(SE_OTHER, 0, 68)) {
            bin(SE_OTHER, 0, 69);
            bin(SE_OTHER, 0, 69);
            bin(SE_OTHER, 0, 69);
          }
      }
      if (cat_ == 1 || cat_ == 2) {
        int ctx = (left_ok && (lf & F_INTRA) && (lf & F_CPRED)) +
                  (top_ok && (tf & F_INTRA) && (tf & F_CPRED));
        if (bin(SE_OTHER, 0, 64 + ctx)) {
          cf |= F_CPRED;
          if (bin(SE_OTHER, 0, 67)) bin(SE_OTHER, 0, 67);
        }
      }
      SPROF_END(3, ps3);
    } else if (nparts == 4) {
      if (direct16) {
        cf |= F_D16;
        cur.direct8[0] = cur.direct8[1] = cur.direct8[2] = cur.direct8[3] = 1;
        if (!d8x8inf) no_sub_lt8x8 = 0;
      } else {
        uint32_t sub = 0;  // per 8x8: parts b0-2, vertical b3, pred b4-5 (no private arrays)
        for (int i = 0; i < 4; i++) {
          int t, sp, sv, spr;
          if (!is_b) {
            if (bin(SE_OTHER, 0, 21)) t = 0;
            else if (!bin(SE_OTHER, 0, 22)) t = 1;
            else if (bin(SE_OTHER, 0, 23)) t = 2;
            else t = 3;
            sp = t == 0 ? 1 : t == 3 ? 4 : 2;
            sv = t == 2;
            spr = 1;
          } else {
            if (!bin(SE_OTHER, 0, 36)) t = 0;
            else if (!bin(SE_OTHER, 0, 37)) t = 1 + bin(SE_OTHER, 0, 39);
            else {
              t = 3;
              if (bin(SE_OTHER, 0, 38)) {
                if (bin(SE_OTHER, 0, 39)) t = 11 + bin(SE_OTHER, 0, 39);
                else {
                  t += 4;
                  t += 2 * bin(SE_OTHER, 0, 39);
                  t += bin(SE_OTHER, 0, 39);
                }
              } else {
                t += 2 * bin(SE_OTHER, 0, 39);
                t += bin(SE_OTHER, 0, 39);
              }
            }
            if (t == 0) { sp = 0; sv = 0; spr = 0; }
            else if (t <= 3) { sp = 1; sv = 0; spr = t; }
            else if (t <= 9) { int k = t - 4; sp = 2; sv = k & 1; spr = (k >> 1) + 1; }
            else { sp = 4; sv = 0; spr = t - 9; }
          }
          sub |= (uint32_t)(sp | sv << 3 | spr << 4) << (8 * i);
          if (sp == 0) {
            cur.direct8[i] = 1;
            if (!d8x8inf) no_sub_lt8x8 = 0;
          } else if (sp > 1) {
            no_sub_lt8x8 = 0;
          }
        }
        SPROF_END(2, ps3);
        PROF_BEGIN(ps4);
        for (int list = 0; list < nlists; list++)
          for (int i = 0; i < 4; i++) {
            const int sp = (sub >> (8 * i)) & 7, spr = (sub >> (8 * i + 4)) & 3;
            if (!sp || !(spr & (1 << list))) continue;
            int nref = list ? nref1 : nref0;
            cur.ref[list][i] = (int8_t)(nref > 1 ? decode_ref(list, 2 * (i & 1), 2 * (i >> 1)) : 0);
          }
        SPROF_END(4, ps4);
        PROF_BEGIN(ps5);
        for (int list = 0; list < nlists; list++)
          for (int i = 0; i < 4; i++) {
            const int sp = (sub >> (8 * i)) & 7, sv = (sub >> (8 * i + 3)) & 1, spr = (sub >> (8 * i + 4)) & 3;
            if (!sp || !(spr & (1 << list))) continue;
            const int x0 = 2 * (i & 1), y0 = 2 * (i >> 1);
            for (int j = 0; j < sp; j++) {
              if (sp == 1) mvd_part(list, x0, y0, 2, 2);
              else if (sp == 4) mvd_part(list, x0 + (j & 1), y0 + (j >> 1), 1, 1);
              else if (!sv) mvd_part(list, x0, y0 + j, 2, 1);
              else mvd_part(list, x0 + j, y0, 1, 2);
            }
          }
        SPROF_END(5, ps5);
      }
    } else {
      SPROF_END(4, ps3);
      PROF_BEGIN(ps4);
      for (int list = 0; list < nlists; list++)
        for (int i = 0; i < nparts; i++) {
          const int pr = i ? pred1 : pred0;
          if (!(pr & (1 << list))) continue;
          const int px = (nparts == 2 && vertical) ? 2 * i : 0, py = (nparts == 2 && !vertical) ? 2 * i : 0;
          const int nref = list ? nref1 : nref0;
          const int ref = nref > 1 ? decode_ref(list, px, py) : 0;
          if (nparts == 1) cur.ref[list][0] = cur.ref[list][1] = cur.ref[list][2] = cur.ref[list][3] = (int8_t)ref;
          else if (!vertical) cur.ref[list][2 * i] = cur.ref[list][2 * i + 1] = (int8_t)ref;
          else cur.ref[list][i] = cur.ref[list][i + 2] = (int8_t)ref;
        }
      SPROF_END(4, ps4);
      PROF_BEGIN(ps5);
      for (int list = 0; list < nlists; list++)
        for (int i = 0; i < nparts; i++) {
          const int pr = i ? pred1 : pred0;
          if (!(pr & (1 << list))) continue;
          if (nparts == 1) mvd_part(list, 0, 0, 4, 4);
          else if (vertical) mvd_part(list, 2 * i, 0, 2, 4);
          else mvd_part(list, 0, 2 * i, 4, 2);
        }
      SPROF_END(5, ps5);
    }
    if (err) return;
    PROF_BEGIN(ps6);
    int cbp;
    if (intra && kind == 1) {
      cbp = i16_cbp;
    } else {
      const uint16_t ca = nb_cbp_left(), cb = nb_cbp_top();
      int c = 0;
      c |= bin(SE_OTHER, 0, 73 + !(ca & 0x02) + 2 * !(cb & 0x04));
      c |= bin(SE_OTHER, 0, 73 + !(c & 0x01) + 2 * !(cb & 0x08)) << 1;
      c |= bin(SE_OTHER, 0, 73 + !(ca & 0x08) + 2 * !(c & 0x01)) << 2;
      c |= bin(SE_OTHER, 0, 73 + !(c & 0x04) + 2 * !(c & 0x02)) << 3;
      if (cat_ == 1 || cat_ == 2) {
        const int a = (ca >> 4) & 3, b = (cb >> 4) & 3;
        if (bin(SE_OTHER, 0, 77 + (a > 0) + 2 * (b > 0)))
          c |= (1 + bin(SE_OTHER, 0, 77 + 4 + (a == 2) + 2 * (b == 2))) << 4;
      }
      cbp = c;
      if ((cbp & 15) && t8mode && !intra && no_sub_lt8x8 && (!direct16 || d8x8inf)) {
        if (bin(SE_OTHER, 0, 399 + (left_ok && (lf & F_T8)) + (top_ok && (tf & F_T8))))
          cf |= F_T8;
      }
    }
    cf |= (uint32_t)cbp << 16;
    if ((cbp & 0x3f) || (intra && kind == 1)) {
      int ctx = last_dqp_nz ? 1 : 0, val = 0;
      while (bin(SE_QPDELTA, val, 60 + ctx)) {
        ctx = ctx < 2 ? 2 : 3;
        if (++val > 102) { err = AVR_SLICE_BAD_QP_DELTA; return; }
      }
      last_dqp_nz = val != 0;
      SPROF_END(6, ps6);
      residual(intra && kind == 1, cbp);
    } else {
      last_dqp_nz = 0;
      SPROF_END(6, ps6);
    }
  }
};

// ---------------------------------------------------------------------------------------
template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void init_slice_state(Walker<MODE, RM, FLD, P32, SPL, SRD>& w, const EngineTables* T) {
  const int lane = threadIdx.x, nt = blockDim.x;  // every wave of the workgroup takes part
  const avr_slice_desc* d = w.d;
  // cabac contexts: 9.3.1.1
  const int tbl = d->slice_type == 2 ? 0 : 1 + d->cabac_init_idc;
  const int qp = d->slice_qp < 0 ? 0 : d->slice_qp > 51 ? 51 : d->slice_qp;
  const SeamRec* seam = nullptr;
  if constexpr (SPL) seam = w.seam;
  if (seam) {   // a piece after a cut: the contexts as they stood there
    const uint32_t* s32 = (const uint32_t*)seam->state;
    uint32_t* st32 = (uint32_t*)w.sh->state;
    for (int i = lane; i < 256; i += nt) st32[i] = s32[i];
  }
  for (int i = seam ? 1024 : lane; i < 1024; i += nt) {
    int m = T->mn[tbl][i][0], n = T->mn[tbl][i][1];
    int pre = ((m * qp) >> 4) + n;
    pre = pre < 1 ? 1 : pre > 126 ? 126 : pre;
    uint8_t s = pre <= 63 ? (uint8_t)((63 - pre) << 1) : (uint8_t)(((pre - 64) << 1) | 1);
    w.sh->state[i] = s;
    if (MODE == MODE_GENERATE) {
      // P(bin = 1) of the initial state: p_LPS = 0.5 * alpha^pStateIdx
      uint32_t plps = T->gen_plps[s >> 1];
      w.sh->gen_p[i] = (uint16_t)((s & 1) ? 65536 - plps : plps);
    }
  }
  if (!RM) {
    for (int i = lane; i < kEstDefault + 2; i += nt) w.sh->est[i] = 0;
    if (MODE != MODE_GENERATE)
      for (int i = lane; i < kEtabSize + 64; i += nt) w.sh->etab[i] = 0;
  }
  uint32_t* ring32 = (uint32_t*)w.ring;
  // MBAFF: the pair edges and records too (walk_slice refuses the slice when they do not fit).  The
  // progressive model row needs no clear: a column's model bytes are read only under a decoded
  // upper macroblock of this slice (top_ok), which wrote them.
  const int cols = (FLD && d->structure == AVR_STRUCT_MBAFF && (int)w.ring_cols >= 3 * w.W + 7) ? 3 * w.W + 7 : w.W;
  if (seam) {   // the upper row's edges from the cut, and a model row of zeros (a fresh model sees none)
    const uint32_t* e32 = (const uint32_t*)(seam + 1);
    for (int i = lane; i < w.W * kEdgeBytes / 4; i += nt) ring32[i] = i % 10 ? e32[i] : e32[i] & ~kEdgeMringNz;
    if (!w.mring_global)
      for (int i = lane; i < w.W * kMringDwords; i += nt) w.mring[i] = 0;
  } else {
    for (int i = lane; i < cols * (int)sizeof(typename Walker<MODE, RM, FLD, P32, SPL, SRD>::ERec) / 4; i += nt) ring32[i] = 0;
  }
  if (lane < 2) {
    w.sh->fifo_head[lane] = 0;
    w.sh->fifo_tail[lane] = 0;
  }
  __syncthreads();
}

template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void walk_slice(Walker<MODE, RM, FLD, P32, SPL, SRD>& w) {
  const avr_slice_desc* d = w.d;
  w.W = d->mb_width;
  // a field picture is a picture of half the frame's rows (d->mb_height is the frame's)
  w.H = (FLD && w.fld_pic) ? d->mb_height >> 1 : d->mb_height;
  w.slice_type = d->slice_type;
  w.is_b = d->slice_type == 1;
  w.cat_ = d->chroma_array_type;
  w.t8mode = d->transform_8x8_mode;
  w.nref0 = d->num_ref_idx_l0;   // descriptor fields used while parsing: kept in registers
  w.nref1 = d->num_ref_idx_l1;
  w.d8x8inf = d->direct_8x8_inference;
  w.x264_build = d->x264_build;
  w.first_mb = d->first_mb;
  w.last_dqp_nz = 0;
  if constexpr (SPL) {
    if (w.seam) w.last_dqp_nz = (int)w.seam->last_dqp_nz;
  }
  w.err = 0;
  w.finished = 0;
  w.bins = 0;
  w.mbs_done = 0;
  int addr = d->first_mb;
  const int lane = threadIdx.x;
  const int npic = w.W * w.H;
  w.mb_x = addr % w.W;   // then stepped: no integer division per macroblock
  w.mb_y = addr / w.W;
  w.ystep = (FLD && w.fld_pic) ? 2 : 1;
  w.my = w.mb_y * w.ystep + (d->structure == AVR_STRUCT_BOTTOM_FIELD ? 1 : 0);
  w.mbaff = FLD && d->structure == AVR_STRUCT_MBAFF;
  w.pst = 0;
  if ((FLD && w.mbaff)) {   // pairs in raster order: mb_y = pair row, my = 2 mb_y + bottom
    if ((int)w.ring_cols < 3 * w.W + 7 || (addr & 1)) { w.err = AVR_SLICE_MBAFF_RING; return; }
    w.mb_x = (addr >> 1) % w.W;
    w.mb_y = (addr >> 1) / w.W;
    w.ystep = 2;
    w.my = 2 * w.mb_y;
  }
  {
    const int j = lane, ph_c = (w.cat_ == 2 || w.cat_ == 3) ? 4 : 2;
    int src = 0;
    if (j >= 1 && j < 4) src = 1 + (j - 1) * 4 + (j == 1 ? 3 : ph_c - 1);   // nnz: bottom row of plane j - 1
    else if (j >= 4 && j < 8) src = 13 + ((j - 4) >> 1) * 8 + 6 + ((j - 4) & 1);   // mvd[l][12..15]
    else if (j == 8) src = 29;                       // ref[0][2..3] (| ref[1][2..3] from dword 30)
    else if (j == 9) src = 31;                       // direct8[2..3]
    else if (j >= 10 && j < 23) src = 32 + (j - 10); // mnnz[52]
    w.edge_src = (uint32_t)src;
  }
  for (;;) {
    if (AVR_MB_UNLIKELY(addr >= npic)) { w.err = AVR_SLICE_BAD_MB_ADDR; break; }
    if constexpr (SPL && MODE == MODE_COMPRESS) {
      if (AVR_MB_UNLIKELY(w.snap && w.mb_x == 0 && w.mbs_done > 0)) w.seam_cut(addr);
    }
    PROF_BEGINW(ps0);
    if (!(FLD && w.mbaff)) {
      w.left_ok = w.mb_x > 0 && addr - 1 >= w.first_mb;
      // the upper neighbour's flags + cbp: the first dword of its edge record
      w.tf = *(const uint32_t*)&w.ring[w.mb_x];
      w.top_ok = (w.tf & F_DEC) != 0;
    } else if (!(w.pst & Walker<MODE, RM, FLD, P32, SPL, SRD>::PST_BOT)) {
      w.mbaff_pair_start();
    }
    w.cf = 0;
    // clear the current record (one dword per lane; ref[2][4] = dwords 29-30 to -1)
    {
      uint32_t* c32 = (uint32_t*)&w.sh->cur;
      if (lane < (int)sizeof(MbRec) / 4) c32[lane] = (lane == 29 || lane == 30) ? 0xffffffffu : 0u;
      wave_sync();
    }
    // the grids of the record that live in registers start from zero like the record
    if constexpr (Walker<MODE, RM, FLD, P32, SPL, SRD>::BS >= 2) w.nz_v = 0;
    if constexpr (Walker<MODE, RM, FLD, P32, SPL, SRD>::BS >= 3) w.mz_v = 0;
    SPROF_ENDW(0, ps0);
#ifdef AVR_PROFILE
    w.sprofb[0]++;   // sub-section 0 counts macroblocks
#endif
    PROF_BEGINW(t1);
    w.decode_mb();
    PROF_ENDW(1, t1);
    PROF_BEGINW(t7);
    if (AVR_MB_UNLIKELY(w.err)) break;
    w.cf |= F_DEC;
    w.mbs_done++;
    w.last_mb = addr + 1 >= npic;
    // publish: bottom edge to the ring, full record to `left`, model bytes to the frame (RM) --
    // two lane-parallel LDS reads of the record (whole, and the edge's dwords), then the stores
    // (BS >= 2: first the grids kept in registers into the record, one byte per lane)
    if constexpr (Walker<MODE, RM, FLD, P32, SPL, SRD>::BS >= 2) {
      if (lane < 48) ((uint8_t*)w.sh->cur.nnz)[lane] = (uint8_t)w.nz_v;
    }
    if constexpr (Walker<MODE, RM, FLD, P32, SPL, SRD>::BS >= 3) {
      if (lane < 52) w.sh->cur.mnnz[lane] = (uint8_t)w.mz_v;
    }
    wave_sync();
    {
      const uint32_t* c32 = (const uint32_t*)&w.sh->cur;
      const uint32_t v = c32[lane < 45 ? lane : 44];
      const uint32_t ve = c32[w.edge_src], ref1 = c32[30];
      const uint32_t ev = lane == 8 ? (ve >> 16) | (ref1 & 0xffff0000u) : lane == 9 ? ve >> 16 : ve;
      if (!(FLD && w.mbaff)) {
        uint32_t* l32 = (uint32_t*)&w.sh->left;
        if (lane < 45) l32[lane] = v;
        uint32_t* e32 = (uint32_t*)&w.ring[w.mb_x];
        if constexpr (FLD) {
          if (lane < 23) e32[lane] = lane == 0 ? (w.cf & 0xffff017fu) : ev;   // dword 0: flags, pad, cbp
        } else {
          // a model row in global scratch: a column whose kept model bytes are all zero (a skipped or
          // residual-free bottom row) is not stored; bit 9 of the edge's dword 0 (EdgeCore::pad)
          // says which, and the lookups under it read zero without a load (4K P-slices: most rows)
          const bool mz = !RM && w.mring_global &&
                          __ballot(lane >= 10 && lane < 23 && ((kMringUsed >> (lane - 10)) & 1) && ev != 0) != 0;
          if (lane < 10) e32[lane] = lane == 0 ? ((w.cf & 0xffff017fu) | (mz ? kEdgeMringNz : 0u)) : ev;
          else if (!RM && lane < 23 && ((kMringUsed >> (lane - 10)) & 1)) {   // the model row (RM reads the frame)
            const uint32_t at = (uint32_t)w.mb_x * kMringDwords + mring_dword((uint32_t)lane - 10);
            if (w.mring_global) {
              if (mz) ((__attribute__((address_space(1))) uint32_t*)w.mring)[at] = ev;
            } else {
              ((__attribute__((address_space(3))) uint32_t*)w.mring)[at] = ev;
            }
          }
        }
        w.lf = w.cf;
      } else {   // the pair edge of this macroblock; the pair's records move left after its bottom
        const int bot = (w.pst & Walker<MODE, RM, FLD, P32, SPL, SRD>::PST_BOT) != 0;
        uint32_t* e32 = (uint32_t*)&w.pair_edge(bot)[w.mb_x];
        if (lane < 23) e32[lane] = lane == 0 ? (w.cf & 0xffff017fu) : ev;
        uint32_t* pr = (uint32_t*)w.pair_rec();
        const uint32_t t = pr[lane < 45 ? lane : 44];
        if (!bot) {
          if (lane < 45) pr[lane] = lane == 0 ? w.cf : v;
        } else if (lane < 45) {
          pr[45 + lane] = t;
          pr[90 + lane] = lane == 0 ? w.cf : v;
        }
      }
      if (RM) {   // MbRec dwords 32-44 are the 52 model bytes
        uint32_t* f32 = (uint32_t*)(w.frames + w.cur_off + ((int64_t)w.mrow() * w.W + w.mb_x) * 52);
        if (lane >= 32 && lane < 45) f32[lane - 32] = v;
      }
      wave_sync();
    }
    PROF_ENDW(7, t7);
    PROF_BEGINW(ps7);
    if (MODE == MODE_COMPRESS || MODE == MODE_DECOMPRESS) {
      w.publish();
      if (!RM) w.update_prio();
    }
    // MBAFF: end_of_slice_flag follows the bottom macroblock of a pair only (7.3.4)
    const int eos = (!(FLD && w.mbaff) || (w.pst & Walker<MODE, RM, FLD, P32, SPL, SRD>::PST_BOT)) ? w.terminate(SE_EOS) : 0;
    SPROF_ENDW(7, ps7);
    if (AVR_MB_UNLIKELY(eos)) break;
    if constexpr (SPL) {   // the piece ends at the next cut (its last macroblock's end_of_slice_flag was 0)
      if (AVR_MB_UNLIKELY(w.piece_mbs && (uint32_t)w.mbs_done >= w.piece_mbs)) {
        w.finished = 1;
        w.cut = 1;
        break;
      }
    }
    if (Walker<MODE, RM, FLD, P32, SPL, SRD>::DEC && AVR_MB_UNLIKELY(w.in.limit && w.cd.next > w.in.limit + 8)) { w.err = AVR_SLICE_OVERREAD; break; }
    // a parallel-model decoder reads at most 8 bytes past its stream (the recoded decoder's 63-bit
    // window; P32: 4): a damaged stream is stopped within a macroblock of running off its end
    if (MODE == MODE_DECOMPRESS && !RM && AVR_MB_UNLIKELY(w.in.limit && w.rd.next > w.in.limit + 16)) { w.err = AVR_SLICE_OVERREAD; break; }
    addr++;
    if ((FLD && w.mbaff) && !(w.pst & Walker<MODE, RM, FLD, P32, SPL, SRD>::PST_BOT)) {
      w.pst |= Walker<MODE, RM, FLD, P32, SPL, SRD>::PST_BOT;
      w.my++;
      continue;
    }
    if ((FLD && w.mbaff)) {
      w.pst = 0;
      w.my--;
    }
    if (++w.mb_x == w.W) {
      w.mb_x = 0;
      w.mb_y++;
      if (FLD) w.my += w.ystep;
    }
  }
}

// Run f on the walker instantiation of the slice's structure: w itself for a progressive frame,
// a field-capable copy (FLD = true, set up from w) for field pictures and MBAFF frames.
// --------------------------------------------------------------------------- kernel bodies
template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void begin_slice(Walker<MODE, RM, FLD, P32, SPL, SRD>& w, const avr_slice_desc* d, const uint8_t* in, uint8_t* out) {
  w.d = d;
  w.in.g = in + d->payload_offset;
  w.in.limit = MODE == MODE_GENERATE ? 0 : d->read_limit;
  w.in.lds = w.sh->in_stage;
  w.in.win = 0xffffffffu - kStage;  // force a fill on first use
  w.out.g = out + d->out_offset;
  w.out.cap = d->out_capacity;
  w.out.n = 0;
  w.out.last = 0;
  w.ring0.init(w.sh, 0);
  vtab_load(w.vt, w.T);
  w.rc_cat = -1;
  w.rc_v = 0;
  w.fld_pic = FLD && (d->structure == AVR_STRUCT_TOP_FIELD || d->structure == AVR_STRUCT_BOTTOM_FIELD);
  w.fld = -1;
  // the progressive kernels never run a field slice: their LDS tables are the frame ones
  if (FLD) w.set_fld(w.fld_pic);
  else w.sig8_v = w.T->sig8x8[__lane_id()];
  w.top_pending = 0;
  w.last8_v = w.T->last8x8[__lane_id()];
  w.blk_v = w.blk2_v = w.nz_v = w.nzn_v = w.mz_v = w.mzl_v = w.mzt_v = 0;
  if (MODE == MODE_DECOMPRESS) w.byp_e = w.sh->est[1024];
  w.mc_load();
  if (!RM && (MODE == MODE_COMPRESS || MODE == MODE_DECOMPRESS)) {
    if (w.prio_cell == kNoCell) w.prio_cell = cu_cell();
    w.prio_cur = 0xffffffffu;   // set on the first macroblock
  }
  if (MODE == MODE_COMPRESS || MODE == MODE_TRACE) {
    cd_init(w.cd, w.in);
    if constexpr (SPL) {
      if (w.seam) {   // a piece after a cut: the decoder where the cut left it
        w.cd.low = w.seam->cd_low;
        w.cd.range = w.seam->cd_range;
        w.cd.k = (int)w.seam->cd_k;
        w.cd.next = w.seam->cd_next;
      }
    }
  } else if (MODE == MODE_DECOMPRESS) {
    // A piece (SPL) starts its decoder like a slice.  The P32 decoder's window runs up to 4 bytes
    // past its stream, the u64 one's up to 8: in_fill_call loads no byte at or past in.limit (the
    // piece's own length, read_limit) and gives zeros there, and every layout a piece comes from
    // (append_pieces, avr_stage_pieces, the piece plans' arena) follows each stream with >= 16 zero
    // bytes besides -- so a piece reads what the encoder's finish assumed, never its neighbour's
    // bytes, and the AVR_SLICE_OVERREAD check below stops a damaged piece at its own end.
    rd_init(w.rd, w.in);
  } else {
    ce_init(w.ce);
    w.rng = d->payload_offset * 0x9E3779B97F4A7C15ull + 0x1234567ull + (uint64_t)d->picture_id;
    w.target_mbs = d->payload_size ? (int)d->payload_size : 1 << 30;
  }
#ifdef AVR_PROFILE
  for (int i = 0; i < 8; i++) w.prof[i] = 0, w.profb[i] = 0, w.sprof[i] = 0, w.sprofb[i] = 0;
#endif
}

template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void profile_slice(Walker<MODE, RM, FLD, P32, SPL, SRD>& w) {
#ifdef AVR_PROFILE
  w.bins = 0;
  const uint64_t t0 = PROF_T();
  const uint32_t t0_b = 0;
  walk_slice(w);
  PROF_ENDW(0, t0);
  if (__lane_id() == 0) {
    for (int i = 0; i < 8; i++) {
      atomicAdd(&avr_prof[i], (unsigned long long)w.prof[i]);
      atomicAdd(&avr_prof[8 + i], (unsigned long long)w.profb[i]);
      atomicAdd(&avr_prof[32 + i], (unsigned long long)w.sprof[i]);
      atomicAdd(&avr_prof[40 + i], (unsigned long long)w.sprofb[i]);
    }
  }
#else
  walk_slice(w);
#endif
}

// The walker wave of a pipelined slice: parse + model, one op per bin into the ring, OP_END at
// the end whatever happened.  Leaves its status in LDS for finish_slice.
template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void walker_slice(Walker<MODE, RM, FLD, P32, SPL, SRD>& w, const avr_slice_desc* d, const uint8_t* in, avr_slice_result* res) {
  begin_slice(w, d, in, nullptr);
  profile_slice(w);
  if constexpr (SPL) {
    if (MODE == MODE_COMPRESS && w.snap && __lane_id() == 0) *w.snap_count = w.snap_n;
  }
  if (!RM) cu_post(w.prio_cell, 0);   // leave the CU board
  w.rc_writeback();  // estimators persist across slices in the reference model
  w.mc_store();
  if (MODE == MODE_DECOMPRESS && __lane_id() == 0) w.sh->est[1024] = (uint16_t)w.byp_e;
  w.push(OP_END);
#ifdef AVR_PROFILE
  if (__lane_id() == 0) atomicAdd(&avr_prof[16], (unsigned long long)w.ring0.wait_cycles);
#endif
  w.publish();
  int status = w.err;
  if (!status && !w.finished) status = AVR_SLICE_NO_END;
  bool cut = false;
  if constexpr (SPL) {
    cut = w.cut;
    if (!status && w.piece_mbs && !cut) status = AVR_SLICE_NO_END;   // end_of_slice inside a non-last piece
    // A P32 piece has to have used up its stream.  The decoder reads 4 bytes at rd_init and one per
    // renormalisation: next = 4 + R.  The encoder made a digit at each of the same R renormalisations
    // and its finish k more, 0 <= k <= 4 (re_finish shifts while low != 0, and low has 32 bits), all of
    // them written out by the end: the stream is L = R + k bytes.  So next - L = 4 - k is in [0, 4]
    // for a stream the encoder made, whether the piece ends at a cut or at end_of_slice.  A damaged
    // piece decodes other decisions and stops, by macroblock count or at the picture's end, somewhere
    // else in its stream (the format has no checksum of a stream; this is the check it allows).
    if constexpr (P32 && MODE == MODE_DECOMPRESS) {
      if (!status && w.in.limit && w.rd.next - w.in.limit > 4u) status = AVR_SLICE_CODER;
    }
  }
  int stop_ok = 1;
  if (MODE == MODE_COMPRESS && !status && !cut) {
    // predicted decompressor output (recode.cpp:1345-1356, 1503-1505): the regenerated CABAC
    // bytes equal the payload through the stop bit, then zero bits
    const uint32_t sbi = cd_bitpos(w.cd) - 1;
    const uint32_t k = sbi >> 3, size = d->payload_size;
    const uint32_t b = in_byte(w.in, k);
    const uint32_t masked = b & (0xffu << (7 - (sbi & 7))) & 0xff;
    if (masked == 0x80) stop_ok = (k == size) || (k + 1 == size);
    else stop_ok = (k + 1 == size) || (k + 2 == size && b == masked);
  }
  if (__lane_id() == 0) {
    w.sh->p_status = status;
    w.sh->p_stop_ok = stop_ok;
    res->bins = w.bins;
    res->mbs = (uint32_t)w.mbs_done;
  }
}

}  // namespace avr

#undef AVR_MB_LIKELY
#undef AVR_MB_UNLIKELY
