// The waves beside the walker (avr_slice_lds.h "Several waves per slice"): the modeler (compress)
// and the coder, each retiring its ring in batches, and the combination of their results.
#pragma once
#include <type_traits>

#include "avr_slice_lds.h"

namespace avr {

AVR_FI uint32_t vgpr_zero() {
  uint32_t z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}
// The modeler wave (compress): the estimator recurrences (recode.cpp:816-820, 1030-1047),
// lane-parallel over each batch of ring-0 ops (lane j = op j):
//  1. every lane loads its op's estimator at once: per-context ones from Shared::est, SIG/NZ
//     ones by probing the first four slots of the key's window in the LDS hash table; keys not
//     resolved there (new keys, deep or HBM-resident ones) go through est_load one key at a time,
//     a new key claiming its slot immediately;
//  2. a scalar loop walks the batch key by key (ballot of equal keys) and, within a key, op by op
//     in order: the recurrence runs in a scalar register and each op's estimator before its update
//     goes into its lane of the output vector -- no memory access on this chain;
//  3. the last op of each key writes the estimator back (lane-parallel), and the whole batch
//     goes to ring 1 as one vector store.
// Ops of one key stay in order, different keys are independent, so this equals processing the
// ops one by one.
// lane L of v := x (x, L wave-uniform)
AVR_FI uint32_t writelane(uint32_t v, uint32_t L, uint32_t x) { return __lane_id() == L ? x : v; }
// SPL: a batch that holds OP_RESTART (the walker's cut, the batch's last op) ends with a fresh model:
// the HBM table's logged entries, the LDS hash and the per-context estimators cleared
template <bool SPL = false>
AVR_FI void model_slice(Shared* sh, uint16_t* est_g) {
  uint32_t tail = 0, head1 = 0, tail1 = 0;
  uint64_t waited = 0;
  uint32_t prio = 0;
  const uint32_t lane = __lane_id();
#ifdef AVR_PROFILE
  uint64_t out_wait = 0;
  const uint64_t t_start = PROF_T();
#endif
  for (bool done = false; !done;) {
    uint32_t op_v;
    const uint32_t n = ring_take(sh, 0, tail, &op_v, &waited);
    follow_prio(sh, &prio);
    asm volatile("; MARK_MODEL_BEGIN");
    const bool live = lane < n;
    const bool ctrl = (op_v & (OP_END | OP_FINISH)) != 0;
    const bool est_op = live && !ctrl;
    if (__ballot(live && (op_v & OP_END))) done = true;
    const uint32_t idx = (op_v >> 3) & 0x7ffffu;
    const bool cache = (op_v & OPM_CACHE) != 0;
    // ---- 1. loads
    uint32_t e_v = 0, slot_v = 0;
    bool resolved = true;
    if (est_op && !cache) e_v = sh->est[idx];
    if (est_op && cache) resolved = est_probe4(sh, idx, &e_v, &slot_v);
    // keys the short probe did not find: one at a time through the wave-wide probe
    uint64_t slow = __ballot(est_op && !resolved);
    while (slow) {
      const uint32_t l = (uint32_t)__builtin_ctzll(slow);
      const uint32_t idx_l = __builtin_amdgcn_readlane(idx, l);
      uint32_t slot;
      const uint32_t e = est_load(sh, est_g, idx_l, &slot);
      if (slot >> 31) {
        if (lane == 0) sh->etab[slot & 0xffff] = (slot & 0xffff0000u) | e;   // claim / keep the slot
        wave_sync();
      }
      const uint64_t same = __ballot(est_op && cache && idx == idx_l);
      if ((same >> lane) & 1) { e_v = e; slot_v = slot; }
      slow &= ~same;
    }
    // ---- 2. the recurrences, key by key, ops in order
    const uint32_t key_v = (op_v >> 1) & 0xfffffdu;            // cache bit + index (bin, threshold excluded)
    const uint64_t bins_m = __ballot(op_v & 1), thr_m = __ballot(op_v & OPM_THR50);
    // billing class of op j: significance map (threshold 0x50), nnz bits (the other SIG/NZ
    // estimators), or anything else
    const uint64_t nz_m = __ballot(cache && !(op_v & OPM_THR50));
    auto cls_of = [&](uint32_t j) -> uint32_t { return ((thr_m >> j) & 1) ? 1u : ((nz_m >> j) & 1) ? 2u : 0u; };
    uint32_t out_v = op_v;                                     // control ops pass through
    uint32_t fin_v = 0;
    uint64_t last_m = 0;
    uint64_t todo = __ballot(est_op);
    while (todo) {
      const uint32_t l = (uint32_t)__builtin_ctzll(todo);
      const uint32_t k = __builtin_amdgcn_readlane(key_v, l);
      uint64_t m = __ballot(key_v == k) & todo;
      todo &= ~m;
      uint32_t e = __builtin_amdgcn_readlane(e_v, l);
      uint32_t j = l;
      for (;;) {
        const uint32_t b = (uint32_t)(bins_m >> j) & 1u;
        out_v = writelane(out_v, j, op_recode((int)b, e) | cls_of(j) << OPC_SHIFT_C);
        e = est_update(e, (int)b, ((thr_m >> j) & 1) ? 0x50u : 0x60u);
        m &= m - 1;
        if (!m) break;
        j = (uint32_t)__builtin_ctzll(m);
      }
      fin_v = writelane(fin_v, j, e);
      last_m |= 1ull << j;
    }
    // ---- 3. write-back by the last op of each key
    const bool is_last = (last_m >> lane) & 1;
    if (is_last && !cache) sh->est[idx] = (uint16_t)fin_v;
    if (is_last && cache && (slot_v >> 31)) sh->etab[slot_v & 0xffff] = (slot_v & 0xffff0000u) | fin_v;
    const bool hbm = is_last && cache && !(slot_v >> 31);
    if (__ballot(hbm)) {
      if (hbm) est_g[idx] = (uint16_t)(fin_v | kEstWritten);
      const uint64_t first = __ballot(hbm && slot_v == 1);
      if (first) {   // append first stores to the table's write log (est_store)
        const uint32_t base = __builtin_amdgcn_readfirstlane(sh->elog_n);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(first);
        const uint32_t pos = base + (uint32_t)__builtin_popcountll(first & ((1ull << lane) - 1));
        uint32_t* lg = (uint32_t*)(est_g + kEstLog);
        if (((first >> lane) & 1) && pos < (uint32_t)kEstLogCap) lg[pos] = idx;
        if (lane == 0) {
          sh->elog_n = base + cnt;
          *(uint32_t*)(est_g + kEstLogN) = base + cnt <= (uint32_t)kEstLogCap ? base + cnt : kEstLogOverflow;
        }
      }
    }
    asm volatile("; MARK_MODEL_END");
    // ---- the batch to ring 1 (room for n entries), then retire it from ring 0
    if (head1 + n - tail1 > (uint32_t)kFifo) {
#ifdef AVR_PROFILE
      const uint64_t tw = PROF_T();
#endif
      for (;;) {
        tail1 = ld_volatile(&sh->fifo_tail[1]);
        if (head1 + n - tail1 <= (uint32_t)kFifo) break;
        __builtin_amdgcn_s_sleep(1);
      }
#ifdef AVR_PROFILE
      out_wait += PROF_T() - tw;
#endif
    }
    if (live) sh->fifo[1][(head1 + lane) & (kFifo - 1)] = out_v;
    head1 += n;
    st_volatile(&sh->fifo_head[1], head1);
    if constexpr (SPL) {
      if (__ballot(live && (op_v & OP_RESTART))) {
        const uint32_t nl = *(volatile uint32_t*)(est_g + kEstLogN);
        if (nl == kEstLogOverflow) {
          uint4* e4 = (uint4*)est_g;
          for (uint32_t i = lane; i < (uint32_t)kEstTable / 8; i += 64) e4[i] = make_uint4(0, 0, 0, 0);
        } else {
          const uint32_t* lg = (const uint32_t*)(est_g + kEstLog);
          for (uint32_t i = lane; i < nl; i += 64) est_g[lg[i]] = 0;
        }
        if (lane == 0) {
          *(uint32_t*)(est_g + kEstLogN) = 0;
          sh->elog_n = 0;
        }
        for (uint32_t i = lane; i < (uint32_t)kEstDefault + 2; i += 64) sh->est[i] = 0;
        for (uint32_t i = lane; i < (uint32_t)kEtabSize + 64; i += 64) sh->etab[i] = 0;
        __threadfence_block();
        wave_sync();
      }
    }
    tail += n;
    ring_retire(sh, 0, tail);
  }
#ifdef AVR_PROFILE
  if (__lane_id() == 0) {
    atomicAdd(&avr_prof[17], (unsigned long long)waited);
    atomicAdd(&avr_prof[18], (unsigned long long)out_wait);
    atomicAdd(&avr_prof[20], (unsigned long long)(PROF_T() - t_start));
  }
#endif
}

// The coder wave: compress retires ring 1 (arithmetic_code<uint64_t,uint8_t>::encoder::put /
// finish, recode.cpp:1074, 1092-1094), gathering each op's reciprocal record with its lane;
// decompress retires ring 0 (cabac::encoder::put / put_bypass / put_terminate,
// recode.cpp:1443-1474, cabac_code.h:33-67).
// SEQ: the reference model's per-file kernels (one slice chain per CU, where the coder can hold the
// walker up): the level / mvd prefixes on one context with the state in a register, and the map
// loops unswitched by block kind.  The slice batch keeps the plain loops (measured: the variants
// cost the batch 0.3-0.8 % and gain R-mode 1-2 %, profiles/r04o_coder2_ab.log, r04q_crunmvd_ab.log).
// SPL (decompress): a piece after a cut starts the re-encoder from the seam record; a piece that ends
// at a cut (seam_end) writes its pending bytes out at the end instead of a flush (the oracle's
// avr_ce_seam_flush): the bytes of the arithmetic's low up to the next piece's first byte
// SPL (compress): every OP_FINISH ends a piece's stream -- its length goes to piece_end[k] and a fresh
// encoder starts the next piece's
template <int MODE, bool P32, bool SEQ = false, bool SPL = false>
AVR_FI void coder_slice(Shared* sh, const HotTables* T, const avr_slice_desc* d, uint8_t* out, uint32_t flags,
                        const SeamRec* seam = nullptr, bool seam_end = false, uint32_t* piece_end = nullptr) {
  uint32_t pieces = 0;
  const bool billing = (flags & kFlagBill) != 0;
  uint32_t bill[6] = {0, 0, 0, 0, 0, 0};
  uint32_t bill_pend = 0;
  CabacBill cbill;
  cb_init(cbill);
  OutStream o;
  o.g = out + d->out_offset;
  o.cap = d->out_capacity;
  o.n = 0;
  o.last = 0;
  typename std::conditional<P32, PEncoder, RecodedEncoder>::type re;   // see Walker::rd
  CabacEncoder ce;
  VTab vt;
  if (MODE == MODE_COMPRESS) {
    re_init(re);
    // Keep the coder's interval in VGPRs: every wave of the CU shares one scalar unit, and the
    // walker wave (the critical path) is scalar-bound; 64-bit multiply-adds are also cheaper on
    // the vector unit (v_mad_u64_u32).  A value the compiler cannot prove uniform stays vector.
    const uint32_t z = vgpr_zero();
    re.range += z;
    re.low += z;
  } else {
    ce_init(ce);
    if constexpr (SPL) {
      if (seam) {
        ce.low = seam->ce_low;
        ce.range = seam->ce_range;
        ce.queue = seam->ce_queue;
        ce.outstanding = seam->ce_outstanding;
        ce.cache = seam->ce_cache;
        ce.have_cache = 1;
      }
    }
    vtab_load(vt, T);
  }
  const int r = MODE == MODE_COMPRESS ? 1 : 0;
  uint32_t gt1 = 0, eq1 = 0;   // decompress: level counters of the block in progress (op_level)
  uint32_t mpos = 0;           // decompress: first position of the next op_map segment
  const uint32_t numc = d->chroma_array_type == 2 ? 2u : 1u;   // chroma DC: NumC8x8
  uint32_t tail = 0;
  uint64_t waited = 0;
#ifdef AVR_PROFILE
  const uint64_t t_start = PROF_T();
#endif
  uint32_t prio = 0;
  for (bool done = false; !done;) {
    uint32_t op_v;
    const uint32_t n = ring_take(sh, r, tail, &op_v, &waited);
    follow_prio(sh, &prio);
    if (MODE == MODE_COMPRESS) {
      const uint32_t tot_v = (op_v >> 8) & 127;
      const uint64_t m_v = !P32 ? T->div[tot_v][0] : T->rcp32[tot_v];
      const uint32_t s_v = !P32 ? (uint32_t)T->div[tot_v][1] : 0u;
      // r1 of op j: the reference coder's exact quotient, or the P-format rule (avr_engine.h)
      auto r1_of = [&](uint32_t j, uint32_t op) {
        if constexpr (!P32) {
          const uint64_t m = readlane64(m_v, j);
          const uint32_t shift = __builtin_amdgcn_readlane(s_v, j);
          return (__umul64hi(re.range, m) >> shift) * ((op >> 1) & 127);
        } else {
          return __umulhi(re.range, __builtin_amdgcn_readlane((uint32_t)m_v, j)) * ((op >> 1) & 127);
        }
      };
      asm volatile("; MARK_CODER_BEGIN");
      // control ops (FINISH, END: once per slice) located up front, so the put loop has no checks
      uint64_t ctrl = __ballot(__lane_id() < n && (op_v & (OP_END | OP_FINISH)));
      for (uint32_t j = 0;;) {
        const uint32_t stop = ctrl ? (uint32_t)__builtin_ctzll(ctrl) : n;
        if (billing) {
          for (; j < stop; j++) {
            const uint32_t op = __builtin_amdgcn_readlane(op_v, j);
            const uint32_t bytes = re_put_billed(re, o, op & 1, r1_of(j, op), &bill_pend);
            const int c = op_class_pip_c((op >> OPC_SHIFT_C) & 3);
            if (bytes) bill[c] += bytes;
          }
        } else {
          for (; j < stop; j++) {
            const uint32_t op = __builtin_amdgcn_readlane(op_v, j);
            re_put(re, o, op & 1, r1_of(j, op));
          }
        }
        if (j >= n) break;
        const uint32_t op = __builtin_amdgcn_readlane(op_v, j);
        if (op & OP_END) { done = true; break; }
        re_finish(re, o);
        if constexpr (SPL) {
          if (piece_end && __lane_id() == 0) piece_end[pieces] = out_total(o);
          pieces++;
          re_init(re);
          const uint32_t z = vgpr_zero();
          re.range += z;
          re.low += z;
        }
        ctrl &= ctrl - 1;
        j++;
      }
      asm volatile("; MARK_CODER_END");
    } else {
      // billing: the generic coder's emission counts beside the re-encode, bin by bin
      auto run = [&](auto BILL) {
        constexpr bool bl = decltype(BILL)::value;
        auto put_dec = [&](int b, uint32_t ctx, uint32_t cls) {
          uint8_t* stp = &sh->state[ctx];
          if constexpr (bl) {
            const uint32_t st = *stp;
            const uint32_t bytes = cb_decision(cbill, b, st, vtab_rec(vt, st));
            if (bytes) bill[op_class_pip_d(cls)] += bytes;
          }
          ce_decision_v(ce, o, b, stp, vt);
        };
        // n ones then (if zero) a zero on one context, class 0 (level / mvd prefixes)
        auto put_run = [&](uint32_t ctx, uint32_t n, bool zero) {
          uint8_t* stp = &sh->state[ctx];
          uint32_t st = *stp;
          for (uint32_t k = 0; k < n + (zero ? 1u : 0u); k++) {
            const int b = k < n;
            const CabacRec r = vtab_rec(vt, st);
            if constexpr (bl) {
              const uint32_t bytes = cb_decision(cbill, b, st, r);
              if (bytes) bill[0] += bytes;
            }
            uint32_t ns;
            ce_encode(ce, o, b, st, r, &ns);
            st = ns;
          }
          *stp = (uint8_t)st;
        };
        auto put_byp = [&](int b, uint32_t cls) {
          if constexpr (bl) {
            const uint32_t bytes = cb_bypass(cbill, b);
            if (bytes) bill[op_class_pip_d(cls)] += bytes;
          }
          ce_bypass(ce, o, b);
        };
        for (uint32_t j = 0; j < n; j++) {
          const uint32_t op = __builtin_amdgcn_readlane(op_v, j);
          if (op & OP_END) { done = true; break; }
          const int b = op & 1;
          const uint32_t kind = (op >> 1) & 3;
          const uint32_t cls = (op >> OPC_SHIFT_D) & 3;
          if (kind == OPK_DECISION) {
            put_dec(b, (op >> 3) & 1023, cls);
          } else if (kind == OPK_BYPASS) {
            put_byp(b, cls);
          } else if (kind == OPK_MACRO) {
            const uint32_t sub = (op >> 3) & 3, cat = (op >> 5) & 15;
            if (sub == 0) {   // op_map: significant / last_significant_coeff_flag of one segment
              const uint32_t npos = ((op >> 9) & 15) + 1, ended = (op >> 13) & 1;
              const uint32_t mask = op >> 14, lastq = ended ? npos - 1 : 16u;
              const uint32_t sb = (uint32_t)T->sig_base[cat], lb = (uint32_t)T->last_base[cat];
              // one loop per block kind (K: 0 4x4-class, 1 chroma DC, 2 8x8), as the walker's
              auto seg_loop = [&](auto K) {
                constexpr int k = decltype(K)::value;
                for (uint32_t q = 0; q < npos; q++) {
                  const uint32_t p = mpos + q;
                  uint32_t sc, lc;
                  if constexpr (k == 2) {
                    sc = T->sig8x8[p];
                    lc = T->last8x8[p];
                  } else if constexpr (k == 1) {
                    sc = lc = min(p / numc, 2u);
                  } else {
                    sc = lc = p;
                  }
                  const int sig = (mask >> q) & 1;
                  put_dec(sig, sb + sc, 1);
                  if (sig) put_dec(q == lastq, lb + lc, 2);
                }
              };
              if constexpr (!SEQ) {
                const bool c8 = cat == 5 || cat == 9 || cat == 13;
                for (uint32_t q = 0; q < npos; q++) {
                  const uint32_t p = mpos + q;
                  uint32_t sc, lc;
                  if (c8) {
                    sc = T->sig8x8[p];
                    lc = T->last8x8[p];
                  } else if (cat == 3) {
                    sc = lc = min(p / numc, 2u);
                  } else {
                    sc = lc = p;
                  }
                  const int sig = (mask >> q) & 1;
                  put_dec(sig, sb + sc, 1);
                  if (sig) put_dec(q == lastq, lb + lc, 2);
                }
              } else if (cat == 5 || cat == 9 || cat == 13) {
                seg_loop(std::integral_constant<int, 2>());
              } else if (cat == 3) {
                seg_loop(std::integral_constant<int, 1>());
              } else {
                seg_loop(std::integral_constant<int, 0>());
              }
              if (npos != 16 || ended) {   // the map's last segment: its block's levels follow
                mpos = 0;
                gt1 = eq1 = 0;
              } else {
                mpos += 16;
              }
            } else if (sub == 1) {   // op_level: coeff_abs_level_minus1 prefix (+ sign)
              const uint32_t sg = (op >> 9) & 1, absl = (op >> 10) & 15;
              const uint32_t ab = (uint32_t)T->abs_base[cat];
              put_dec(absl > 1, ab + (gt1 ? 0u : min(4u, 1 + eq1)), 0);
              if (absl > 1) {
                const uint32_t c1 = ab + 5 + min(4u - (cat == 3), gt1);
                if constexpr (SEQ) {
                  put_run(c1, absl - 2, absl < 15);   // one context: its state stays in a register
                } else {
                  for (uint32_t a = 2; a < 15; a++) {
                    const int more = a < absl;
                    put_dec(more, c1, 0);
                    if (!more) break;
                  }
                }
              }
              if (absl < 15) put_byp((int)sg, 0);
              if (absl == 1) eq1++;
              else gt1++;
            } else {   // op_mvd: mvd_lX[][][comp] prefix (+ sign), 9.3.3.1.1.7 / 9.3.3.1.2
              const uint32_t base = (op & 32) ? 47u : 40u, sg = (op >> 8) & 1, am = (op >> 9) & 15;
              put_dec(am > 0, base + ((op >> 6) & 3), 0);
              if (am > 0) {
                // bins m = 1, 2, 3 on contexts base + 3, 4, 5, then m = 4 .. 8 on base + 6
                uint32_t m = 1;
                for (; m < 4; m++) {
                  const int more = m < am;
                  put_dec(more, base + m + 2, 0);
                  if (!more) break;
                }
                if (m == 4) {
                  if constexpr (SEQ) {
                    put_run(base + 6, min(am, 9u) - 4, am < 9);
                  } else {
                    for (; m < 9; m++) {
                      const int more = m < am;
                      put_dec(more, base + 6, 0);
                      if (!more) break;
                    }
                  }
                }
                if (am < 9) put_byp((int)sg, 0);
              }
            }
          } else {
            if constexpr (bl) {
              const uint32_t bytes = cb_terminate(cbill, b);
              if (bytes) bill[op_class_pip_d(cls)] += bytes;
            }
            ce_terminate(ce, o, b);
          }
        }
      };
      if (billing) run(std::true_type());
      else run(std::false_type());
    }
    tail += n;
    ring_retire(sh, r, tail);
  }
#ifdef AVR_PROFILE
  if (__lane_id() == 0) {
    atomicAdd(&avr_prof[19], (unsigned long long)waited);
    atomicAdd(&avr_prof[21], (unsigned long long)(PROF_T() - t_start));
  }
#endif
  if constexpr (SPL) {
    if (MODE == MODE_DECOMPRESS && seam_end) {
      const uint32_t carry = ce.low >> (ce.queue + 18);
      if (ce.have_cache) {
        if (ce.cache + carry > 0xff) ce.err = 1;
        out_byte(o, ce.cache + carry);
      } else if (carry) {
        ce.err = 1;
      }
      if (ce.outstanding) out_repeat(o, (0xff + carry) & 0xff, ce.outstanding);
    }
  }
  if (__lane_id() == 0) {
    sh->c_err = MODE == MODE_COMPRESS ? re.err : ce.err;
    sh->c_len = out_total(o);
    sh->c_last = o.last;
    for (int i = 0; i < 6; i++) sh->bill[i] = bill[i];
  }
}

// Combine the two waves' results (after a workgroup barrier), with run_slice_inline's semantics.
// seam_end: a piece that ends at a cut (its last byte is not the slice's)
template <int MODE>
AVR_FI void finish_slice(const Shared* sh, const avr_slice_desc* d, avr_slice_result* res, bool seam_end = false) {
  int status = sh->p_status;
  if (sh->c_err) status = AVR_SLICE_CODER;
  if (MODE == MODE_COMPRESS && !status && !sh->p_stop_ok) status = AVR_SLICE_NO_STOP;
  uint32_t len = sh->c_len;
  if (len > d->out_capacity) {   // nothing past the capacity was written: report what was
    status = AVR_SLICE_OVERFLOW;
    len = d->out_capacity;
  }
  if (MODE == MODE_DECOMPRESS && !status && len && sh->c_last == 0x80 && !seam_end) len--;  // recode.cpp:1503-1505
  res->out_len = len;
  res->status = status;
  for (int i = 0; i < 6; i++) res->bill[i] = sh->bill[i];
}

}  // namespace avr
