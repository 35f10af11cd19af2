// C ABI of avrecode-amd (include/avrecode.h), the device side: the context, and the orchestration
// of every launch around the device kernels.
//
//   compress file   demux + headers (avr_front.cpp) -> payload arena in HBM -> slice kernel
//                   (one wavefront per slice) -> segmentation + Recoded protobuf
//                   (avr_assemble.cpp; recode.cpp:1102-1132, 1275-1297)
//   decompress file Recoded -> literal + surrogate stream (avr_plan.cpp; recode.cpp:1359-1409,
//                   1527-1544) -> headers -> slice kernel -> last-byte patch (recode.cpp:1345-1356)
//
// The host-only entry points (plans, assembly, stream parse) live in avr_plan.cpp and
// avr_assemble.cpp, the seams codec in avr_seams.cpp, the libavcodec-hooks surface in avr_hooks.cpp.
// The hot path has no host implementation: without a GPU every entry point here fails with
// AVR_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/avrecode.h"
#include "avr_ctx.h"
#include "avr_engine.h"
#include "avr_synth.h"
#include "h264_tables.h"

using namespace avr_host;

namespace {

constexpr uint64_t kMaxSynthBytes = (uint64_t)1 << 35;   // avr_synthesize_stream's output cap (32 GiB)

// Engine tables: FFmpeg-layout CABAC tables, (m,n) init, exact reciprocals for the recoded
// coder's (range/(pos+neg)) and the model's neighbour geometry.
void build_tables(avr::EngineTables* t) {
  memset(t, 0, sizeof(*t));
  // FFmpeg-layout LPS range [q*128 + state] and transitions ([128+s] MPS, [127-s] LPS), state =
  // 2*pStateIdx + valMPS; packed per state into one 64-bit record (HotTables::cabac)
  uint8_t lps[512], mlps[256];
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < 64; i++) lps[q * 128 + 2 * i] = lps[q * 128 + 2 * i + 1] = avr::kRangeTabLPS[i][q];
  for (int i = 0; i < 64; i++) {
    int mps = i < 62 ? i + 1 : i;
    mlps[128 + 2 * i] = (uint8_t)(2 * mps);
    mlps[128 + 2 * i + 1] = (uint8_t)(2 * mps + 1);
    mlps[127 - 2 * i] = (uint8_t)(i == 0 ? 1 : 2 * avr::kTransIdxLPS[i]);
    mlps[127 - (2 * i + 1)] = (uint8_t)(i == 0 ? 0 : 2 * avr::kTransIdxLPS[i] + 1);
  }
  for (int st = 0; st < 128; st++) {
    uint64_t r = 0;
    for (int q = 0; q < 4; q++) r |= (uint64_t)lps[q * 128 + st] << (8 * q);
    r |= (uint64_t)mlps[128 + st] << 32;
    r |= (uint64_t)mlps[127 - st] << 40;
    t->hot.cabac[st] = r;
  }
  for (int tbl = 0; tbl < 4; tbl++)
    for (int c = 0; c < 1024; c++) {
      int m, n;
      avr::mn_for_ctx(tbl - 1, c, &m, &n);
      t->mn[tbl][c][0] = (int8_t)m;
      t->mn[tbl][c][1] = (int8_t)n;
    }
  for (uint32_t d = 2; d < 128; d++) {
    int l = 0;
    while ((1u << l) < d) l++;
    unsigned __int128 num = (unsigned __int128)1 << (63 + l);
    t->hot.div[d][0] = (uint64_t)((num + d - 1) / d);
    t->hot.div[d][1] = (uint64_t)(l - 1);
    t->hot.rcp32[d] = (uint32_t)((1ull << 32) / d);   // P-format coder (avr_engine.h, PEncoder)
  }
  // reverse_scan_8 neighbours (recode.cpp:279-312, 444-447)
  static const uint8_t scan8[48] = {
    4 + 1 * 8,  5 + 1 * 8,  4 + 2 * 8,  5 + 2 * 8,  6 + 1 * 8,  7 + 1 * 8,  6 + 2 * 8,  7 + 2 * 8,
    4 + 3 * 8,  5 + 3 * 8,  4 + 4 * 8,  5 + 4 * 8,  6 + 3 * 8,  7 + 3 * 8,  6 + 4 * 8,  7 + 4 * 8,
    4 + 6 * 8,  5 + 6 * 8,  4 + 7 * 8,  5 + 7 * 8,  6 + 6 * 8,  7 + 6 * 8,  6 + 7 * 8,  7 + 7 * 8,
    4 + 8 * 8,  5 + 8 * 8,  4 + 9 * 8,  5 + 9 * 8,  6 + 8 * 8,  7 + 8 * 8,  6 + 9 * 8,  7 + 9 * 8,
    4 + 11 * 8, 5 + 11 * 8, 4 + 12 * 8, 5 + 12 * 8, 6 + 11 * 8, 7 + 11 * 8, 6 + 12 * 8, 7 + 12 * 8,
    4 + 13 * 8, 5 + 13 * 8, 4 + 14 * 8, 5 + 14 * 8, 6 + 13 * 8, 7 + 13 * 8, 6 + 14 * 8, 7 + 14 * 8};
  auto cell_block = [&](int row, int col, bool* crossed) {
    const int top = row <= 4 ? 1 : row <= 9 ? 6 : 11;
    *crossed = false;
    if (row == top - 1) row = top + 3, *crossed = true;
    if (col == 3) col = 7, *crossed = true;
    for (int k = 0; k < 48; k++)
      if (scan8[k] == row * 8 + col) return k;
    return 0;
  };
  for (int n = 0; n < 48; n++) {
    bool cr;
    int s = scan8[n];
    int l = cell_block(s >> 3, (s & 7) - 1, &cr);
    t->hot.nb_left[n] = (uint8_t)(l | (cr ? 128 : 0));
    int u = cell_block((s >> 3) - 1, s & 7, &cr);
    t->hot.nb_up[n] = (uint8_t)(u | (cr ? 128 : 0));
  }
  // ctxIdx bases per ctxBlockCat (9.3.3.1.1.9, frame coded) and the 8x8 ctxIdxInc maps
  static const int16_t cbf[14] = {85, 89, 93, 97, 101, 1012, 460, 464, 468, 1016, 472, 476, 480, 1020};
  static const int16_t sig[14] = {105, 120, 134, 149, 152, 402, 484, 499, 513, 660, 528, 543, 557, 718};
  static const int16_t last[14] = {166, 181, 195, 210, 213, 417, 572, 587, 601, 690, 616, 631, 645, 748};
  static const int16_t abs_[14] = {227, 237, 247, 257, 266, 426, 952, 962, 972, 708, 982, 992, 1002, 766};
  // dense SIG estimator base per ctxBlockCat: 4096 per 4x4-class cat, 61440 for 8x8 cats (5, 9, 13)
  static const int32_t seb[14] = {0, 4096, 8192, 12288, 16384, 20480, 81920, 86016, 90112,
                                  94208, 155648, 159744, 163840, 167936};
  static const uint8_t sig8[63] = {
    0, 1, 2, 3, 4, 5, 5, 4, 4, 3, 3, 4, 4, 4, 5, 5, 4, 4, 4, 4, 3, 3, 6, 7, 7, 7, 8, 9, 10, 9, 8, 7,
    7, 6, 11, 12, 13, 11, 6, 7, 8, 9, 14, 10, 9, 8, 6, 11, 12, 13, 11, 6, 9, 14, 10, 9, 11, 12, 13, 11, 14, 10, 12};
  static const uint8_t last8[63] = {
    0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,
    3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8};
  for (int c = 0; c < 14; c++) {
    t->hot.cbf_base[c] = cbf[c];
    t->hot.sig_base[c] = sig[c];
    t->hot.last_base[c] = last[c];
    t->hot.abs_base[c] = abs_[c];
    t->hot.sig_est_base[c] = seb[c];
  }
  for (int i = 0; i < 63; i++) {
    t->hot.sig8x8[i] = sig8[i];
    t->hot.last8x8[i] = last8[i];
  }
  // field coded (FFmpeg significant_coeff_flag_offset[1], last_coeff_flag_offset[1],
  // significant_coeff_flag_offset_8x8[1] == recode.cpp:691-694)
  static const int16_t sig_f[14] = {277, 292, 306, 321, 324, 436, 776, 791, 805, 675, 820, 835, 849, 733};
  static const int16_t last_f[14] = {338, 353, 367, 382, 385, 451, 864, 879, 893, 699, 908, 923, 937, 757};
  static const uint8_t sig8_f[63] = {
    0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 7, 7, 8, 4, 5, 6, 9, 10, 10, 8, 11, 12, 11, 9, 9, 10, 10, 8, 11, 12, 11,
    9, 9, 10, 10, 8, 11, 12, 11, 9, 9, 10, 10, 8, 13, 13, 9, 9, 10, 10, 8, 13, 13, 9, 9, 10, 10, 14, 14, 14, 14, 14};
  for (int c = 0; c < 14; c++) {
    t->sig_base_fld[c] = sig_f[c];
    t->last_base_fld[c] = last_f[c];
  }
  for (int i = 0; i < 63; i++) t->sig8x8_fld[i] = sig8_f[i];
  const double alpha = std::pow(0.01875 / 0.5, 1.0 / 63.0);
  for (int s = 0; s < 64; s++) t->gen_plps[s] = (uint16_t)std::lround(65536.0 * 0.5 * std::pow(alpha, s));
}

bool check_reciprocals(const avr::EngineTables& t) {
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (uint32_t d = 2; d < 128; d++) {
    auto q = [&](uint64_t v) -> uint64_t {
      return (uint64_t)(((unsigned __int128)v * t.hot.div[d][0]) >> 64) >> t.hot.div[d][1];
    };
    const uint64_t edge[] = {0, 1, d - 1, d, d + 1, (1ull << 63) - 1, 1ull << 63, (1ull << 62) + 12345};
    for (uint64_t v : edge)
      if (q(v) != v / d) return false;
    for (int k = 0; k < 4000; k++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      uint64_t v = x >> 1;
      uint64_t m = (v / d) * d;
      if (q(v) != v / d || q(m) != m / d || (m && q(m - 1) != (m - 1) / d)) return false;
    }
  }
  return true;
}

constexpr int kRModeFallback = 1;

// Reference-model compress of a plan (file order) in parallel over slices (avr_k_rmode.hip), the
// device half: the frame generations are rmode_generations' (avr_cplan.cpp), which also leaves a
// plan to the sequential kernel (kRModeFallback), as does a plan too large for one pass.
int run_rmode_compress(avr_ctx* c, Plan& plan, uint32_t flags) {
  const int n = (int)plan.descs.size();
  const int nf = plan.n_files();
  std::vector<int64_t> goff;
  int64_t fbytes = 0;
  if (nf > avr::rmode_max_files_per_pass() || !rmode_generations(plan, &goff, &fbytes)) return kRModeFallback;
  const size_t lds = avr::shared_bytes(plan.max_w);
  HIP_TRY(c, c->frames.reserve((size_t)fbytes + 64));
  HIP_TRY(c, hipMemsetAsync(c->frames.p, 0, (size_t)fbytes + 64, c->stream));
  HIP_TRY(c, c->rm_goff.reserve(sizeof(int64_t) * goff.size()));
  HIP_TRY(c, hipMemcpyAsync(c->rm_goff.p, goff.data(), sizeof(int64_t) * goff.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, c->rm_counts.reserve(sizeof(uint32_t) * n));
  HIP_TRY(c, c->rm_stop.reserve(sizeof(int32_t) * n));
  HIP_TRY(c, c->rm_off.reserve(sizeof(uint64_t) * (n + 1)));
  // 1) count the model ops (and fill the frame metadata)
  HIP_TRY(c, avr::launch_rscan(c->tables.as<avr::EngineTables>(), c->descs.as<avr_slice_desc>(), n, lds,
                               c->in.as<uint8_t>(), c->frames.as<uint8_t>(), c->rm_goff.as<int64_t>(),
                               c->rm_counts.as<uint32_t>(), nullptr, nullptr, c->res.as<avr_slice_result>(),
                               c->rm_stop.as<int32_t>(), plan.fields(), c->stream));
  std::vector<uint32_t> counts(n);
  HIP_TRY(c, hipMemcpyAsync(counts.data(), c->rm_counts.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<uint64_t> off(n + 1, 0);
  for (int k = 0; k < n; k++) off[k + 1] = off[k] + counts[k];
  const uint64_t N = off[n];
  if (getenv("AVR_RMODE_STATS")) {
    uint64_t pay = 0;
    uint32_t mx = 0;
    double mxr = 0;
    for (int k = 0; k < n; k++) {
      pay += plan.descs[k].payload_size;
      mx = std::max(mx, counts[k]);
      if (plan.descs[k].payload_size > 0) mxr = std::max(mxr, (double)counts[k] / plan.descs[k].payload_size);
    }
    fprintf(stderr, "rmode: %d slices, %llu ops, %llu payload bytes (%.2f ops/B, max slice %u ops, max %.1f ops/B)\n",
            n, (unsigned long long)N, (unsigned long long)pay, pay ? (double)N / pay : 0.0, mx, mxr);
  }
  if (N >= (1ull << 31) - 1) return kRModeFallback;   // hipCUB's item count is an int
  HIP_TRY(c, hipMemcpyAsync(c->rm_off.p, off.data(), sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
  std::vector<uint64_t> fop(nf + 1);
  for (int f = 0; f <= nf; f++) fop[f] = off[f < nf ? plan.file_begin(f) : n];
  HIP_TRY(c, c->file_op_off.reserve(sizeof(uint64_t) * (nf + 1)));
  HIP_TRY(c, hipMemcpyAsync(c->file_op_off.p, fop.data(), sizeof(uint64_t) * (nf + 1), hipMemcpyHostToDevice,
                            c->stream));
  const size_t tb = avr::rmode_sort_temp_bytes(N, nf);
  // ops, keys, skeys, rops: 4 B per op; vals, svals: 8 B (op index << 2 | flags)
  HIP_TRY(c, c->rm_ops.reserve(sizeof(uint32_t) * (N + 1) * 8 + tb + 256));
  uint32_t* ops = c->rm_ops.as<uint32_t>();
  uint32_t* keys = ops + (N + 1);
  uint32_t* skeys = keys + (N + 1);
  uint32_t* rops = skeys + (N + 1);
  uint64_t* vals = (uint64_t*)(rops + (N + 1));
  uint64_t* svals = vals + (N + 1);
  void* temp = (void*)(((uintptr_t)(svals + (N + 1)) + 255) & ~(uintptr_t)255);
  // 2) write the ops, 3) estimator chains, 4) per-slice coder
  HIP_TRY(c, avr::launch_rscan(c->tables.as<avr::EngineTables>(), c->descs.as<avr_slice_desc>(), n, lds,
                               c->in.as<uint8_t>(), c->frames.as<uint8_t>(), c->rm_goff.as<int64_t>(),
                               c->rm_counts.as<uint32_t>(), ops, c->rm_off.as<uint64_t>(),
                               c->res.as<avr_slice_result>(), c->rm_stop.as<int32_t>(), plan.fields(), c->stream));
  HIP_TRY(c, avr::launch_rmode_estimators(ops, N, c->file_op_off.as<uint64_t>(), nf, keys, vals, skeys, svals, temp,
                                          tb, rops, c->stream));
  HIP_TRY(c, avr::launch_rcode(c->tables.as<avr::EngineTables>(), c->descs.as<avr_slice_desc>(), n, rops,
                               c->rm_off.as<uint64_t>(), c->rm_counts.as<uint32_t>(), c->out.as<uint8_t>(),
                               c->res.as<avr_slice_result>(), c->rm_stop.as<int32_t>(), flags, c->stream));
  return AVR_OK;
}

// Device scratch of a parallel launch of n slices: the estimator tables (one per slice of a resident
// batch, one per workgroup of a persistent one: avr::est_slots), the CU schedule and the slice queue.
hipError_t reserve_parallel(avr_ctx* c, int n, int max_w, bool field_lane = false) {
  const int slots = std::max(1, avr::est_slots(n, max_w, field_lane));
  hipError_t e = c->est.reserve(sizeof(uint16_t) * (size_t)avr::kEstGlobal * slots, true);
  if (e == hipSuccess) e = c->order.reserve(sizeof(int) * (size_t)std::max(1, n));
  if (e == hipSuccess) e = c->queue.reserve(std::max<size_t>(256, avr::queue_scratch_bytes(n)));
  return e;
}

// ------------------------------------------------------------------------ the long-slice split
// The parallel model (on arithmetic_code<uint64_t, uint8_t>; on the P32 coder with avr_set_split_p32)
// cuts a long progressive slice at macroblock-row starts into pieces re-coded with fresh models, so
// its decompress runs one workgroup per piece instead of one chain (the reference decodes a slice as
// one chain, recode.cpp:1411-1520).
// The format is this library's own, restated and checked by the oracle (oracle/oracle_seams.c,
// avr_oracle.h):
//   - a cut candidate every 8 split_bytes CABAC bits decoded (at a row start, half a piece still
//     ahead); it becomes a cut where the re-encoder's state can be placed (seam_encoder) -- the
//     byte form of the arithmetic's low L = V - codIOffset, V the payload's first bitpos bits;
//   - each piece has its own re-coded stream (Block.cabac holds them one after the other) and starts
//     with a fresh model whose upper row of model bytes is zero;
//   - Block field 16 ("seams", zlib) carries, per cut, what the piece after it needs: its first
//     macroblock, its first output byte q, the re-encoder state, the CABAC contexts, last_dqp_nz
//     and the upper row's edges (the parse's neighbour fields).
// Compress takes the long slices through the split kernel once (avr_k_split.hip, mode 0), on its
// own stream beside the rest of the batch: each whole slice is cut as it is walked -- the cut
// records, the pieces' streams one after the other and their ends come out of that single walk (a
// slice without a cut: one piece).  Decompress runs the pieces side by side and splices them: piece
// i's bytes up to cut i's q.
constexpr size_t kSplitBytesDefault = 98304;

// The two timing events around a split launch, owned by the job they time: destroyed with it on
// every path out, the failed ones included.
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  int create(avr_ctx* c) {
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    return AVR_OK;
  }
};

// The launches of the split kernel, each stated once for the whole-file calls (split_begin,
// split_launch: the context's sp_* buffers on split_stream) and for the ABI's calls on a caller's
// device buffers and stream (avr_compress_split_slices, avr_decompress_pieces).  Everything but ctl
// is device memory.  ctl is the launch's host PieceCtl array, uploaded to ctl_dev on st: the caller
// keeps it alive while that is in flight.  ev (optional): recorded directly around the kernel.
// Mode 1, the pieces: piece k starts at record ctl[k].seam of d_recs (null: no piece does).
int launch_split_ctl(avr_ctx* c, int mode, const avr_slice_desc* d_desc, int n, int max_w, const uint8_t* d_in,
                     uint8_t* d_out, avr_slice_result* d_res, const avr::PieceCtl* ctl, DevBuf* ctl_dev,
                     avr::SplitArgs sa, uint32_t flags, hipStream_t st, const EventPair* ev) {
  HIP_TRY(c, ctl_dev->reserve(sizeof(avr::PieceCtl) * n));
  HIP_TRY(c, c->sp_est.reserve(sizeof(uint16_t) * (size_t)avr::kEstGlobal * std::max(1, avr::split_grid(n, max_w)), true));
  if (!sa.recs) {   // a batch without records: none is read or written
    HIP_TRY(c, c->sp_recs.reserve(64));
    sa.recs = c->sp_recs.as<uint8_t>();
  }
  HIP_TRY(c, hipMemcpyAsync(ctl_dev->p, ctl, sizeof(avr::PieceCtl) * n, hipMemcpyHostToDevice, st));
  sa.ctl = ctl_dev->as<avr::PieceCtl>();
  if (ev) HIP_TRY(c, hipEventRecord(ev->e0, st));
  HIP_TRY(c, avr::launch_split(mode, c->tables.as<avr::EngineTables>(), d_desc, n, max_w, d_in, d_out, d_res,
                               c->sp_est.as<uint16_t>(), sa, flags, st));
  if (ev) HIP_TRY(c, hipEventRecord(ev->e1, st));
  return AVR_OK;
}
// Mode 0, the split walk: slice k may write the records of its slot (avr_split_plan's; {-1, 0}: it is
// not cut), its cut count to d_cuts[k] and its pieces' ends to d_piece_end from slots[k].first, both
// zeroed here first.  The kernel is offered cap - 1 records of a slot, not cap: a walk that filled
// its slot would write its last piece's end one entry past it, into the next slice's or past the
// array.  The rule leaves that one to spare: cut candidates are at least split_bits apart and need
// split_bits / 2 still ahead (Walker::seam_cut), so cuts <= 8 size / split_bits - 1/2 <= cap - 1.
int launch_split_walk(avr_ctx* c, const avr_slice_desc* d_desc, int n, int max_w, const uint8_t* d_in, uint8_t* d_out,
                      avr_slice_result* d_res, const avr_split_slot* slots, uint8_t* d_recs, int n_recs, size_t rec_stride,
                      uint32_t* d_cuts, uint32_t* d_piece_end, size_t split_bytes, uint32_t flags, hipStream_t st,
                      std::vector<avr::PieceCtl>* ctl, DevBuf* ctl_dev, const EventPair* ev) {
  ctl->resize(n);
  for (int k = 0; k < n; k++)
    (*ctl)[k] = slots[k].first < 0 ? avr::PieceCtl{-1, 0, -1, 0} : avr::PieceCtl{-1, 0, slots[k].first, slots[k].cap - 1};
  HIP_TRY(c, hipMemsetAsync(d_cuts, 0, sizeof(uint32_t) * n, st));
  if (n_recs) HIP_TRY(c, hipMemsetAsync(d_piece_end, 0, sizeof(uint32_t) * n_recs, st));
  avr::SplitArgs sa;
  sa.recs = d_recs;
  sa.rec_stride = (uint32_t)rec_stride;
  sa.split_bits = (uint32_t)(8 * split_bytes);
  sa.snap_n = d_cuts;
  sa.piece_end = n_recs ? d_piece_end : nullptr;
  return launch_split_ctl(c, 0, d_desc, n, max_w, d_in, d_out, d_res, ctl->data(), ctl_dev, sa, flags, st, ev);
}

// Compress of the long slices, in two calls around the rest of the batch: begin uploads them and
// launches the split compress on the split stream (each slice cut as it is walked: the records,
// the pieces' streams one after the other, their ends); finish checks every cut against the host's
// restatement of the re-encoder state, and (verify) decompresses the pieces and compares.
struct SplitOut {
  int32_t status = 0;
  std::vector<uint8_t> recoded, seams;   // seams empty: no cut
  avr_slice_result bill{};
  uint32_t crc = 0;   // SplitJob::crc: the payload's CRC-32
  std::vector<uint32_t> unit_crcs;   // SplitJob::unit_crc: one per unit (Block field 18), the payload's own when uncut
};
struct SplitJob {
  std::vector<const avr::SliceInfo*> sl;
  std::vector<avr_slice_desc> d;      // compress_files: the header's fields and payload_size
  std::vector<avr_split_slot> slots;
  std::vector<avr::PieceCtl> ctl;     // the walk's upload
  Bytes arena;
  uint64_t out_total = 0;
  uint32_t nrec = 0;
  size_t stride = 0;
  int max_w = 1;
  uint32_t coder = 0;   // coder_flag(model): the walk's and the verify launch's coder
  bool crc = false;     // a checked container: the payloads' CRCs too, over the uploaded arena
  bool unit_crc = false;   // unit checksums (implies crc): the cut slices' units too, once the cuts are known
  EventPair ev;   // around the split compress kernel
};

int split_begin(avr_ctx* c, SplitJob* j, size_t split_bytes, uint32_t flags) {
  const int n = (int)j->sl.size();
  if (!n) return AVR_OK;
  j->slots.resize(n);
  for (int k = 0; k < n; k++) {
    const avr::SliceInfo& s = *j->sl[k];
    avr_slice_desc& d = j->d[k];
    append_aligned(&j->arena, s.payload(), s.read_limit, 16, &d.payload_offset);
    d.read_limit = (uint32_t)s.read_limit;
    uint64_t cap = 0, oc = 0;
    if (!split_slot(d, split_bytes, &cap, &oc) || oc > UINT32_MAX || j->nrec + cap > INT32_MAX)
      return fail(c, AVR_ERR_INVALID_ARGUMENT, "split: a slice too long for its cut records");
    d.out_capacity = (uint32_t)oc;
    place_output(&d, &j->out_total);
    j->max_w = std::max(j->max_w, d.mb_width);
    j->slots[k] = avr_split_slot{(int32_t)j->nrec, (uint32_t)cap};
    j->nrec += (uint32_t)cap;
  }
  j->stride = avr::seam_rec_bytes(j->max_w);
  HIP_TRY(c, c->sp_in.reserve(j->arena.size() + 4096));
  HIP_TRY(c, c->sp_out.reserve(j->out_total + 4096));
  HIP_TRY(c, c->sp_descs.reserve(sizeof(avr_slice_desc) * n));
  HIP_TRY(c, c->sp_res.reserve(sizeof(avr_slice_result) * n));
  HIP_TRY(c, c->sp_recs.reserve(j->stride * j->nrec + 64));
  HIP_TRY(c, c->sp_snapn.reserve(sizeof(uint32_t) * ((size_t)n + j->nrec)));
  if (int r = j->ev.create(c)) return r;
  hipStream_t st = c->split_stream;
  HIP_TRY(c, hipMemcpyAsync(c->sp_in.p, j->arena.data(), j->arena.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->sp_descs.p, j->d.data(), sizeof(avr_slice_desc) * n, hipMemcpyHostToDevice, st));
  uint32_t* cuts = c->sp_snapn.as<uint32_t>();   // then the piece ends
  if (j->crc) {
    HIP_TRY(c, c->sp_crc.reserve(2 * sizeof(uint32_t) * n));
    HIP_TRY(c, avr::launch_crc_slices(c->sp_descs.as<avr_slice_desc>(), nullptr, n, false, c->sp_in.as<uint8_t>(),
                                      j->arena.size(), c->sp_crc.as<uint32_t>(), c->sp_crc.as<int32_t>() + n, st));
  }
  return launch_split_walk(c, c->sp_descs.as<avr_slice_desc>(), n, j->max_w, c->sp_in.as<uint8_t>(),
                           c->sp_out.as<uint8_t>(), c->sp_res.as<avr_slice_result>(), j->slots.data(),
                           c->sp_recs.as<uint8_t>(), (int)j->nrec, j->stride, cuts, cuts + n, split_bytes,
                           (flags & avr::kFlagBill) | j->coder, st, &j->ctl, &c->sp_ctl, &j->ev);
}

// One launch of pieces on the split stream: descs / ctl uploaded, records already in sp_recs,
// results and outputs downloaded -- waited for, or (pending != nullptr) left in flight for
// split_wait, so the rest of a batch runs beside it.
// (The downloads wait for split_wait: a copy into pageable host memory would block the host until
// the kernel before it is done, and with it the launches meant to run beside it.)
struct SplitPending {
  EventPair ev;   // around the pieces kernel; e0 set: a launch is in flight
  void* res = nullptr;
  void* out = nullptr;
  const void* res_dev = nullptr;
  const void* out_dev = nullptr;
  size_t res_bytes = 0, out_bytes = 0;
};
// The device buffers of a pieces launch besides its input and output: the context's first set, or the
// second (a decompress call with split blocks of both coders: one launch per coder, avr_ctx.h)
struct SplitLane {
  DevBuf *descs, *res, *ctl, *recs;
};
SplitLane split_lane(avr_ctx* c, int second) {
  return second ? SplitLane{&c->sp2_descs, &c->sp2_res, &c->sp2_ctl, &c->sp2_recs}
                : SplitLane{&c->sp_descs, &c->sp_res, &c->sp_ctl, &c->sp_recs};
}
bool split_timing() { return getenv("AVR_SPLIT_TIMING") != nullptr; }
int split_wait(avr_ctx* c, SplitPending* pend) {
  if (!pend->ev.e0) return AVR_OK;
  HIP_TRY(c, hipStreamSynchronize(c->split_stream));
  HIP_TRY(c, hipMemcpy(pend->res, pend->res_dev, pend->res_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(pend->out, pend->out_dev, pend->out_bytes, hipMemcpyDeviceToHost));
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, pend->ev.e0, pend->ev.e1));
  if (split_timing()) fprintf(stderr, "split: pieces kernel %.3f s\n", 1e-3 * ms);
  c->phase.kernel_s += 1e-3 * ms;
  return AVR_OK;
}
int split_launch(avr_ctx* c, std::vector<avr_slice_desc>& d, const std::vector<avr::PieceCtl>& ctl, const uint8_t* in_dev,
                 int max_w, size_t stride, uint32_t flags, std::vector<avr_slice_result>* res, Bytes* out,
                 DevBuf* out_dev, SplitPending* pending = nullptr, int second = 0) {
  const int n = (int)d.size();
  uint64_t total = 0;
  for (auto& x : d) place_output(&x, &total);
  res->assign(n, avr_slice_result{});
  out->resize(total);
  if (!n) return AVR_OK;
  hipStream_t st = c->split_stream;
  HIP_TRY(c, out_dev->reserve(total + 4096));
  const SplitLane ln = split_lane(c, second);
  HIP_TRY(c, ln.descs->reserve(sizeof(avr_slice_desc) * n));
  HIP_TRY(c, ln.res->reserve(sizeof(avr_slice_result) * n));
  HIP_TRY(c, hipMemcpyAsync(ln.descs->p, d.data(), sizeof(avr_slice_desc) * n, hipMemcpyHostToDevice, st));
  avr::SplitArgs sa;
  sa.recs = ln.recs->as<uint8_t>();
  sa.rec_stride = (uint32_t)stride;
  SplitPending local;
  SplitPending* pend = pending ? pending : &local;
  if (int r = pend->ev.create(c)) return r;
  if (int r = launch_split_ctl(c, 1, ln.descs->as<avr_slice_desc>(), n, max_w, in_dev, out_dev->as<uint8_t>(),
                               ln.res->as<avr_slice_result>(), ctl.data(), ln.ctl, sa, flags, st, &pend->ev))
    return r;
  pend->res = res->data();
  pend->res_dev = ln.res->p;
  pend->res_bytes = sizeof(avr_slice_result) * n;
  pend->out = out->data();
  pend->out_dev = out_dev->p;
  pend->out_bytes = total;
  return pending ? AVR_OK : split_wait(c, pend);
}

int split_finish(avr_ctx* c, SplitJob* j, bool verify, std::vector<SplitOut>* out) {
  const int n = (int)j->sl.size();
  out->assign(n, SplitOut());
  if (!n) return AVR_OK;
  hipStream_t st = c->split_stream;
  // 1) the split compress: statuses, streams, cut records, piece ends
  std::vector<avr_slice_result> r1(n);
  std::vector<uint32_t> cnt((size_t)n + j->nrec);
  Bytes out1(j->out_total), recs((size_t)j->stride * j->nrec);
  HIP_TRY(c, hipMemcpyAsync(r1.data(), c->sp_res.p, sizeof(avr_slice_result) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->sp_snapn.p, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out1.data(), c->sp_out.p, j->out_total, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(recs.data(), c->sp_recs.p, recs.size(), hipMemcpyDeviceToHost, st));
  std::vector<uint32_t> crcs(j->crc ? 2 * (size_t)n : 0);   // then the statuses
  if (j->crc) HIP_TRY(c, hipMemcpyAsync(crcs.data(), c->sp_crc.p, sizeof(uint32_t) * crcs.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int k = 0; j->crc && k < n; k++)   // a payload inside the arena is never refused
    (*out)[k].crc = crcs[n + k] == 0 ? crcs[k] : avr_crc32(0, j->sl[k]->payload(), j->sl[k]->size);
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, j->ev.e0, j->ev.e1));
  if (split_timing()) fprintf(stderr, "split: compress kernel %.3f s (%d slices)\n", 1e-3 * ms, n);
  c->phase.kernel_s += 1e-3 * ms;
  // 2) the seams step (seams_build): every cut checked against the host's restatement, the pieces'
  //    lengths, the fields.  What the device wrote and does not fit fails its slice.
  std::vector<SliceSeams> ss;
  if (seams_build(j->d.data(), n, j->arena.data(), j->arena.size(), r1.data(), j->slots.data(), cnt.data(),
                  cnt.data() + n, (int)j->nrec, recs.data(), j->stride, true, AVR_SLICE_CODER, &ss))
    return fail(c, AVR_ERR_DEVICE, "zlib failed");
  for (int k = 0; k < n; k++) {
    SplitOut& so = (*out)[k];
    so.status = ss[k].status;
    so.bill = r1[k];
    if (so.status) continue;
    so.recoded.assign(out1.begin() + j->d[k].out_offset, out1.begin() + j->d[k].out_offset + r1[k].out_len);
    so.seams.swap(ss[k].field);
  }
  // 2b) unit checksums: the units of the cut slices are known now -- one avr_crc_spans launch over the
  //     payload arena, which still lies in sp_in (an uncut slice's one unit is its payload)
  if (j->unit_crc) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    for (int k = 0; k < n; k++) {
      if ((*out)[k].status || ss[k].q.empty()) continue;
      const uint32_t size = j->d[k].payload_size;
      for (size_t u = 0; u <= ss[k].q.size(); u++) {
        const uint32_t lo = u ? ss[k].q[u - 1] : 0u, hi = u < ss[k].q.size() ? ss[k].q[u] : size;
        if (lo > hi || hi > size) return fail(c, AVR_ERR_DEVICE, "split: cuts that do not ascend inside the slice");
        off.push_back(j->d[k].payload_offset + lo);
        len.push_back(hi - lo);
      }
    }
    const size_t N = off.size();
    std::vector<uint32_t> got(2 * N);   // the values, then the statuses
    if (N) {
      if (N > (size_t)INT32_MAX) return fail(c, AVR_ERR_INVALID_ARGUMENT, "split: too many units");
      HIP_TRY(c, c->sp_ucrc.reserve(20 * N));
      uint64_t* d_off = c->sp_ucrc.as<uint64_t>();
      uint32_t* d_len = (uint32_t*)(d_off + N);
      uint32_t* d_crc = d_len + N;
      HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), 8 * N, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(d_len, len.data(), 4 * N, hipMemcpyHostToDevice, st));
      HIP_TRY(c, avr::launch_crc_spans(c->sp_in.as<uint8_t>(), j->arena.size(), d_off, d_len, (int)N, d_crc,
                                       (int32_t*)(d_crc + N), st));
      HIP_TRY(c, hipMemcpyAsync(got.data(), d_crc, 8 * N, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
    }
    size_t at = 0;
    for (int k = 0; k < n; k++) {
      SplitOut& so = (*out)[k];
      if (so.status) continue;
      if (ss[k].q.empty()) {
        so.unit_crcs.assign(1, so.crc);
        continue;
      }
      for (size_t u = 0; u <= ss[k].q.size(); u++, at++)   // a span inside the arena is never refused
        so.unit_crcs.push_back(got[N + at] == 0 ? got[at]
                                                : avr_crc32(0, j->arena.data() + off[at], len[at]));
    }
  }
  // 3) verify: the pieces decompressed from the records as a container gives them, spliced, compared
  Plan vp;
  std::vector<avr::PieceCtl> pc;
  std::vector<int> first(n, -1);
  for (int k = 0; verify && k < n; k++) {
    if ((*out)[k].status) continue;
    first[k] = (int)vp.descs.size();
    append_pieces(&vp, &pc, j->d[k], (*out)[k].recoded.data(), ss[k].piece_len, ss[k].first_mb,
                  (uint32_t)j->slots[k].first, [&](size_t) { return (uint32_t)j->sl[k]->size + 4096; });
  }
  if (vp.descs.empty()) return AVR_OK;
  HIP_TRY(c, c->sp_in2.reserve(vp.arena.size() + 4096));
  HIP_TRY(c, hipMemcpyAsync(c->sp_in2.p, vp.arena.data(), vp.arena.size(), hipMemcpyHostToDevice, st));
  std::vector<avr_slice_result> r3;
  Bytes out3;
  if (int e = split_launch(c, vp.descs, pc, c->sp_in2.as<uint8_t>(), j->max_w, j->stride, j->coder, &r3, &out3,
                           &c->sp_out2))
    return e;
  for (int k = 0; k < n; k++) {
    if (first[k] < 0) continue;
    const avr::SliceInfo& s = *j->sl[k];
    std::vector<uint8_t> regen;
    bool ok = splice_pieces(&vp.descs[first[k]], &r3[first[k]], out3.data(), ss[k].q, &regen);
    if (ok) {
      last_byte_patch(&regen, s.payload(), s.size);
      ok = regen.size() == s.size && memcmp(regen.data(), s.payload(), s.size) == 0;
    }
    if (!ok) (*out)[k].status = AVR_SLICE_NO_ROUNDTRIP;
  }
  return AVR_OK;
}

// compressor::run (recode.cpp:1102-1132) for several files at once.  The device work of every
// file is batched: one parallel launch checks every candidate slice of every file (parse, restore,
// device roundtrip), and the reference model runs all files in one pass (the parallel R-mode
// pipeline over all their slices with per-file estimators, or one workgroup per file).  out[f] is
// malloc'd; status[f] (optional) is file f's result; the return value is the first failure.
// Host side of avr_phase_times for one whole-file call: the time before the first device pass is
// demux, the wall time inside run_plan is the device passes (split by their HIP events, the rest
// of it overhead), everything else container work.
struct PhaseClock {
  avr_ctx* c;
  double t0, t_demux = -1;
  explicit PhaseClock(avr_ctx* ctx) : c(ctx), t0(now_s()) {
    c->phase = avr_phase_times{};
    c->plan_wall = 0;
  }
  void mark_demux() {
    if (t_demux < 0) t_demux = now_s() - t0;
  }
  void finish() {
    mark_demux();
    avr_phase_times& p = c->phase;
    const double wall = now_s() - t0, dev = p.upload_s + p.kernel_s + p.download_s;
    p.demux_s = t_demux;
    p.container_s = std::max(0.0, wall - t_demux - c->plan_wall);
    p.other_s = std::max(0.0, c->plan_wall - dev);
  }
};

typedef std::array<uint64_t, 6> Bill;   // h264_model::bill / cabac_bill by avr_pip_coding_type
void add_bill(Bill* b, const avr_slice_result& r) {
  for (int i = 0; i < 6; i++) (*b)[i] += r.bill[i];
}

// ------------------------------------------------------------------------ whole-file compress
// Per file f and slice i of it, compress_files keeps: ok (offered to the segmentation), found
// (where the segmentation found it; null: not coded) and recoded (what its block holds).

// The reference-model pass: the coded slices of every file in file order, estimators per file (per
// chain: reference_plan); a slice that fails there is demoted to skip_coded and its file's pass
// repeated.
int reference_pass(avr_ctx* c, int nf, const uint8_t* const* in, const size_t* in_len, int model,
                   const std::vector<ParsedFile>& pf, std::vector<Bill>* bills, std::vector<int32_t>& st,
                   std::vector<std::vector<char>>& ok, std::vector<std::vector<const uint8_t*>>& found,
                   std::vector<std::vector<std::vector<uint8_t>>>& recoded) {
  std::vector<char> todo(nf, 0), coded;
  for (int f = 0; f < nf; f++) todo[f] = st[f] == AVR_OK;
  for (int attempt = 0;; attempt++) {
    Plan rp;
    std::vector<std::pair<int, int>> idx;   // (file, slice) per desc
    for (int f = 0; f < nf; f++) {
      if (!todo[f]) continue;
      if (bills) (*bills)[f] = Bill{};   // this pass re-codes the whole file
      coded.assign(found[f].size(), 0);
      for (size_t i = 0; i < found[f].size(); i++) coded[i] = found[f][i] != nullptr;
      reference_plan(&rp, pf[f], 0, (int)coded.size(), coded, model == AVR_MODEL_CHAINED, f, &idx);
    }
    if (rp.file_first.empty()) break;
    rp.file_first.push_back((int)rp.descs.size());
    std::vector<avr_slice_result> rr;
    Bytes ro;
    if (int r = run_plan(c, 0, true, rp, &rr, &ro, false, bills ? avr::kFlagBill : 0)) return r;
    std::fill(todo.begin(), todo.end(), 0);
    for (size_t k = 0; k < idx.size(); k++) {
      const int f = idx[k].first, i = idx[k].second;
      if (!found[f][i]) continue;
      if (rr[k].status != 0) {
        found[f][i] = nullptr;
        todo[f] = 1;
        continue;
      }
      recoded[f][i].assign(ro.begin() + rp.descs[k].out_offset, ro.begin() + rp.descs[k].out_offset + rr[k].out_len);
      if (bills) add_bill(&(*bills)[f], rr[k]);
    }
    bool again = false;
    for (int f = 0; f < nf; f++) {
      if (!todo[f]) continue;
      again = true;
      // a demoted slice changes the literal gaps of later ones: redo the segmentation
      for (size_t i = 0; i < pf[f].slices.size(); i++) ok[f][i] = ok[f][i] && found[f][i] != nullptr;
      found[f] = segment(in[f], in_len[f], pf[f], ok[f]);
      if (attempt == 7) {
        st[f] = fail(c, AVR_ERR_DEVICE, "reference-model pass did not converge");
        todo[f] = 0;
      }
    }
    if (!again) break;
  }
  return AVR_OK;
}

// verify (parallel model): decompress every candidate slice on the device and code only those that
// regenerate their payload.  avr_roundtrip_file skips it on a first attempt -- its own whole-file
// decompress and compare check the same thing, as the reference's roundtrip() does with a
// compressor that never verifies (recode.cpp:1594-1624) -- and repeats with it on a mismatch.
int compress_files(avr_ctx* c, int nf, const uint8_t* const* in, const size_t* in_len, int model, uint8_t** out,
                   size_t* out_len, int32_t* status, std::vector<Bill>* bills = nullptr, bool verify = true) {
  if (bills) bills->assign(nf, Bill{});
  HIP_TRY(c, hipSetDevice(c->device));
  PhaseClock pc(c);
  std::vector<int32_t> st(nf, AVR_OK);
  std::vector<ParsedFile> pf(nf);
  for (int f = 0; f < nf; f++) {
    out[f] = nullptr;
    out_len[f] = 0;
    st[f] = parse_file(c, in[f], in_len[f], &pf[f], /*views=*/true);
  }
  // 1) plan, parallel model: every candidate slice of every file goes through the parallel kernel
  //    -- per-slice parse, restore check, device roundtrip and the model's output -- the long ones
  //    (split_slot) through the split job.  Reference model: nothing here; the reference-model
  //    pass below parses and checks every candidate itself (its statuses carry the same parse /
  //    restore verdict) and demotes the failures, so a well-formed file costs one reference-model
  //    pass, not a parallel-model pass before it.
  Plan plan;
  SplitJob sj;
  std::vector<std::vector<Route>> route;
  const size_t split_bytes =
      model == AVR_MODEL_PARALLEL || (model == AVR_MODEL_PARALLEL32 && c->split_p32) ? c->split_bytes : 0;
  sj.coder = coder_flag(model);
  // a checked container (avr_set_checksums): the candidates' payload CRCs from the device, where the
  // uploads put them; the reference models' pass re-plans, and its payloads are CRC'd by emit_container
  const bool checks = c->checksums;
  // unit checksums (avr_set_unit_checksums): the parallel models' coded blocks carry their units' CRCs
  // (Block field 18) -- an uncut slice's is that same payload CRC, a cut slice's units follow its cuts
  const bool units = c->unit_checksums && parallel_model(model);
  sj.crc = checks || units;
  sj.unit_crc = units;
  SliceCrcs crcs_dev;
  if (parallel_model(model)) plan_candidates(pf, st, split_bytes, &plan, &sj.sl, &sj.d, &route);
  // 2) launch the split job's first pass on the split stream, then the batch beside it; collect
  std::vector<avr_slice_result> res;
  Bytes outb;
  pc.mark_demux();
  const uint32_t bill_flag = bills ? avr::kFlagBill : 0u;
  if (int r = split_begin(c, &sj, split_bytes, bill_flag)) return r;
  if (int r = run_plan(c, 0, false, plan, &res, &outb, verify, bill_flag | coder_flag(model),
                       checks || units ? &crcs_dev : nullptr)) {
    (void)hipStreamSynchronize(c->split_stream);   // its first pass still reads sj's buffers
    return r;
  }
  std::vector<SplitOut> so;
  {
    const double t = now_s();
    if (int r = split_finish(c, &sj, verify, &so)) return r;
    c->plan_wall += now_s() - t;
  }
  // 3) segmentation (find_next_coded_block_and_emit_literal, recode.cpp:1275-1297)
  std::vector<std::vector<char>> ok(nf);
  std::vector<std::vector<const uint8_t*>> found(nf);
  for (int f = 0; f < nf; f++) {
    ok[f].assign(pf[f].slices.size(), 0);
    for (size_t i = 0; i < pf[f].slices.size(); i++) {
      const Route r = reference_model(model) ? Route{} : route[f][i];
      ok[f][i] = reference_model(model) ? st[f] == AVR_OK && recodable_candidate(pf[f].slices[i])
                 : r.kind == Route::kBatch ? res[r.index].status == 0
                                           : r.kind == Route::kSplit && so[r.index].status == 0;
    }
  }
  // the parallel models' option (avr_set_recode_escaped): a slice the search misses is searched
  // once more by its escaped payload, and kept with Block field 17
  const bool escaped = parallel_model(model) && c->recode_escaped;
  std::vector<std::vector<uint32_t>> escapes(nf);
  parallel_files(nf, [&](int f) { found[f] = segment(in[f], in_len[f], pf[f], ok[f], escaped ? &escapes[f] : nullptr); });
  // 4) the blocks of the coded slices: the reference-model pass, or what step 2 left
  std::vector<std::vector<std::vector<uint8_t>>> recoded(nf);
  for (int f = 0; f < nf; f++) recoded[f].resize(pf[f].slices.size());
  std::vector<std::vector<std::pair<const uint8_t*, size_t>>> seams_of(nf);
  for (int f = 0; f < nf; f++) seams_of[f].assign(pf[f].slices.size(), {nullptr, 0});
  std::vector<std::vector<uint32_t>> crc_of(nf);
  for (int f = 0; f < nf && checks && parallel_model(model); f++) crc_of[f].assign(pf[f].slices.size(), 0);
  std::vector<std::vector<std::vector<uint32_t>>> ucrc_of(nf);
  for (int f = 0; f < nf && units; f++) ucrc_of[f].resize(pf[f].slices.size());
  if (reference_model(model)) {
    if (int r = reference_pass(c, nf, in, in_len, model, pf, bills, st, ok, found, recoded)) return r;
  } else {
    for (int f = 0; f < nf; f++)
      for (size_t i = 0; i < pf[f].slices.size(); i++) {
        if (!found[f][i]) continue;
        const Route r = route[f][i];
        if (r.kind == Route::kSplit) {   // its pieces' streams and seams
          SplitOut& x = so[r.index];
          recoded[f][i].swap(x.recoded);
          seams_of[f][i] = {x.seams.data(), x.seams.size()};
          if (checks) crc_of[f][i] = x.crc;
          if (units) ucrc_of[f][i] = x.unit_crcs;
          if (bills) add_bill(&(*bills)[f], x.bill);
          continue;
        }
        if (checks || units) {
          const uint32_t crc = crcs_dev.have(r.index) ? crcs_dev.crc[r.index]
                                                      : avr_crc32(0, pf[f].slices[i].payload(), pf[f].slices[i].size);
          if (checks) crc_of[f][i] = crc;
          if (units) ucrc_of[f][i].assign(1, crc);
        }
        recoded[f][i].assign(outb.begin() + plan.descs[r.index].out_offset,
                             outb.begin() + plan.descs[r.index].out_offset + res[r.index].out_len);
        if (bills) add_bill(&(*bills)[f], res[r.index]);
      }
  }
  // 5) containers (compressor::run, recode.cpp:1115-1125)
  int first_err = AVR_OK;
  parallel_files(nf, [&](int f) {
    if (st[f] != AVR_OK) return;
    std::vector<std::pair<const uint8_t*, size_t>> blobs(pf[f].slices.size(), {nullptr, 0});
    for (size_t i = 0; i < pf[f].slices.size(); i++) blobs[i] = {recoded[f][i].data(), recoded[f][i].size()};
    st[f] = emit_container(in[f], in_len[f], views_of(pf[f]), found[f], blobs, model, &out[f], &out_len[f], nullptr, 0,
                           &seams_of[f], escaped ? &escapes[f] : nullptr,
                           FileCrcArg{checks, crc_of[f].empty() ? nullptr : crc_of[f].data()},
                           UnitCrcArg{units, units ? &ucrc_of[f] : nullptr});
  });
  for (int f = 0; f < nf; f++) {
    if (status) status[f] = st[f];
    if (st[f] && !first_err) first_err = st[f];
  }
  pc.finish();
  return status ? AVR_OK : first_err;
}

// ------------------------------------------------------------------------ whole-file decompress
// The pieces of split blocks on the split stream, beside the other plans: the two coders' launches
// one after the other there, each with its own input / output / record buffers.  A failure leaves
// nothing in flight.
int launch_pieces(avr_ctx* c, SplitPlan* sps, uint32_t flags, std::vector<avr_slice_result>* prs, Bytes* pos,
                  SplitPending* pends, double* t_split) {
  for (int i = 0; i < 2; i++) {
    SplitPlan& sp = sps[i];
    if (sp.plan.descs.empty()) continue;
    const double t = now_s();
    hipStream_t ss = c->split_stream;
    DevBuf* in_dev = i ? &c->sp_in2 : &c->sp_in;
    DevBuf* recs_dev = split_lane(c, i).recs;
    auto launch = [&]() -> int {
      HIP_TRY(c, in_dev->reserve(sp.plan.arena.size() + 4096));
      HIP_TRY(c, recs_dev->reserve(sp.recs.size() + 64));
      HIP_TRY(c, hipMemcpyAsync(in_dev->p, sp.plan.arena.data(), sp.plan.arena.size(), hipMemcpyHostToDevice, ss));
      HIP_TRY(c, hipMemcpyAsync(recs_dev->p, sp.recs.data(), sp.recs.size(), hipMemcpyHostToDevice, ss));
      return split_launch(c, sp.plan.descs, sp.ctl, in_dev->as<uint8_t>(), sp.plan.max_w, sp.stride,
                          flags | (i ? avr::kFlagP32 : 0u), &prs[i], &pos[i], i ? &c->sp_out2 : &c->sp_out, &pends[i], i);
    };
    if (int r = launch()) {   // what is in flight still reads this call's host buffers
      (void)hipStreamSynchronize(ss);
      return r;
    }
    *t_split += now_s() - t;
  }
  return AVR_OK;
}

// decompressor::run (recode.cpp:1312-1357) for several files at once: the slices of every
// parallel-model file go to one parallel launch, every reference-model file to one workgroup of a
// sequential launch.
int decompress_files(avr_ctx* c, int nf, const uint8_t* const* in, const size_t* in_len, uint8_t** out,
                     size_t* out_len, int32_t* status, std::vector<Bill>* bills = nullptr) {
  HIP_TRY(c, hipSetDevice(c->device));
  PhaseClock pc(c);
  if (bills) bills->assign(nf, Bill{});
  const uint32_t flags = bills ? avr::kFlagBill : 0;
  std::vector<int32_t> st(nf, AVR_OK);
  std::vector<DecJob> jobs(nf);
  // 1) plan.  plans[AVR_MODEL_*]: reference-model files (one workgroup each); parallel-model slices
  //    on the u64 coder; on the P32 coder
  Plan plans[3];   // indexed by plan_of(model): the chained model's chains go to the reference plan
  Plan& rp = plans[AVR_MODEL_REFERENCE];
  // the pieces of split blocks, one plan per coder (the coder is a compile-time parameter of the
  // split kernel, so one launch cannot hold both): [0] the u64 coder's, [1] the P32 coder's
  SplitPlan sps[2];
  auto plan_of = [](int m) { return parallel_model(m) ? m : (int)AVR_MODEL_REFERENCE; };
  for (int f = 0; f < nf; f++) {
    out[f] = nullptr;
    out_len[f] = 0;
    std::string version;
    std::vector<avr::PbBlock> probe;
    const int m = avr::pb_parse(in[f], in_len[f], &probe, &version) ? std::max(0, avr::model_of_version(version)) : 0;
    Plan* plan = &plans[plan_of(m)];
    const size_t n0 = plan->descs.size();
    SplitPlan& sp = sps[m == AVR_MODEL_PARALLEL32];
    const size_t s_descs = sp.plan.descs.size(), s_recs = sp.recs.size(), s_arena = sp.plan.arena.size();
    st[f] = decompress_setup(c, in[f], in_len[f], &jobs[f], plan, &sp);
    if (st[f]) {   // drop whatever the failed file left
      plan->descs.resize(n0);
      sp.plan.descs.resize(s_descs);
      sp.ctl.resize(s_descs);
      sp.recs.resize(s_recs);
      sp.plan.arena.resize(s_arena);
    } else if (!parallel_model(m)) {
      // one workgroup per file, or per chain (the compress side's boundaries)
      append_file_chains(&rp, n0, jobs[f].model == AVR_MODEL_CHAINED);
    }
  }
  std::vector<avr_slice_result> res_of[3];
  std::vector<uint8_t> out_of[3];
  // checked containers: the regenerated slices' CRCs from the device, before the download (the pieces
  // of split blocks are spliced on the host, and CRC'd there by the fold)
  SliceCrcs crcs_of[3];
  bool checks[3] = {false, false, false};
  for (int f = 0; f < nf; f++)
    if (st[f] == AVR_OK && jobs[f].has_crc) checks[plan_of(jobs[f].model)] = true;
  pc.mark_demux();
  // 2) launch the pieces, then the slice plans beside them
  std::vector<avr_slice_result> prs[2];
  Bytes pos[2];
  SplitPending pends[2];
  double t_split = 0;
  if (int r = launch_pieces(c, sps, flags, prs, pos, pends, &t_split)) return r;
  auto drain = [&]() { (void)hipStreamSynchronize(c->split_stream); };
  for (int m = AVR_MODEL_PARALLEL; m <= AVR_MODEL_PARALLEL32; m++)
    if (!plans[m].descs.empty())
      if (int r = run_plan(c, 1, false, plans[m], &res_of[m], &out_of[m], false, flags | coder_flag(m),
                           checks[m] ? &crcs_of[m] : nullptr)) {
        drain();
        return r;
      }
  if (!rp.file_first.empty()) {
    rp.file_first.push_back((int)rp.descs.size());
    if (int r = run_plan(c, 1, true, rp, &res_of[0], &out_of[0], false, flags, checks[0] ? &crcs_of[0] : nullptr)) {
      drain();
      return r;
    }
  }
  // 3) collect the pieces of split blocks, then each block spliced
  if (!sps[0].plan.descs.empty() || !sps[1].plan.descs.empty()) {
    const double t = now_s();
    for (SplitPending& pend : pends)
      if (int r = split_wait(c, &pend)) {
        drain();
        return r;
      }
    for (int f = 0; f < nf; f++) {
      if (st[f]) continue;
      const int i = jobs[f].model == AVR_MODEL_PARALLEL32;   // the file's blocks are in its coder's plan
      const SplitPlan& sp = sps[i];
      const std::vector<avr_slice_result>& pr = prs[i];
      const Bytes& po = pos[i];
      for (SplitBlock& x : jobs[f].splits) {
        for (int k = x.first; k < x.first + x.pieces; k++)
          if (pr[k].status == 0)
            for (int b = 0; b < 6; b++) x.bill.bill[b] += pr[k].bill[b];
        x.status = splice_pieces(&sp.plan.descs[x.first], &pr[x.first], po.data(), x.q, &x.regen) ? 0 : AVR_SLICE_NO_END;
      }
    }
    c->plan_wall += t_split + (now_s() - t);
  }
  // 4) the files written out (decompressor::run, recode.cpp:1338-1357)
  int first_err = AVR_OK;
  for (int f = 0; f < nf; f++) {
    DecJob& j = jobs[f];
    const Plan& plan = plans[plan_of(j.model)];
    const std::vector<avr_slice_result>& res = res_of[plan_of(j.model)];
    const std::vector<uint8_t>& outb = out_of[plan_of(j.model)];
    std::vector<uint8_t> o;
    if (st[f] == AVR_OK)
      st[f] = splice_job(c, j, [&](Route r, const uint8_t** p, size_t* len) {
        if (r.kind == Route::kSplit) {   // spliced from its pieces
          const SplitBlock& x = j.splits[r.index];
          *p = x.regen.data();
          *len = x.regen.size();
          if (bills && x.status == 0) add_bill(&(*bills)[f], x.bill);
          return (int)x.status;
        }
        *p = outb.data() + plan.descs[r.index].out_offset;
        *len = res[r.index].out_len;
        if (bills && res[r.index].status == 0) add_bill(&(*bills)[f], res[r.index]);
        return res[r.index].status;
      }, &o, [&](Route r, uint32_t* crc) {
        const SliceCrcs& cs = crcs_of[plan_of(j.model)];
        if (r.kind != Route::kBatch || !cs.have(r.index)) return false;
        *crc = cs.crc[r.index];
        return true;
      });
    if (st[f] == AVR_OK) {
      out[f] = (uint8_t*)malloc(o.size() ? o.size() : 1);
      if (!out[f]) {
        st[f] = AVR_ERR_OUT_OF_MEMORY;
      } else {
        if (!o.empty()) memcpy(out[f], o.data(), o.size());
        out_len[f] = o.size();
      }
    }
    if (status) status[f] = st[f];
    if (st[f] && !first_err) first_err = st[f];
  }
  pc.finish();
  return status ? AVR_OK : first_err;
}

// ------------------------------------------------------------ the chained model across GPUs
// The chained model's chains are independent by construction (a fresh model -- estimators, frames --
// before every AVR_CHAIN_SLICES-th coded slice of a file: chain_starts), so one file's chains can
// run on several GPUs: each rank takes a contiguous range of chains, balanced by payload bytes, and
// the re-coded (or regenerated) slices are gathered to rank 0, which assembles (splices) them as for
// the parallel model.

// This rank's slices [lo, hi): its share (partition_range) of the chains that start at `first`,
// weighted by their coded payload bytes (size(i): slice i's, 0 when it is not coded).
template <class Size>
std::pair<int, int> rank_slices(const std::vector<int>& first, int world, int rank, Size&& size) {
  const int nc = (int)first.size() - 1;
  std::vector<double> w(nc, 0.0);
  for (int ch = 0; ch < nc; ch++)
    for (int i = first[ch]; i < first[ch + 1]; i++) w[ch] += (double)size(i);
  const auto [clo, chi] = partition_range(w, world, rank);
  return {first[clo], first[std::max(clo, chi)]};
}

// compressor::run (recode.cpp:1102-1132) of the chained model, this rank's chains only: the parse
// and the segmentation of the whole file (the coded slices, hence the chains, depend on every block
// before them), then the reference-model pass over this rank's chains (run_plan: one workgroup
// per chain, or the parallel reference-model compress when it pays).  status: 0 coded (bytes),
// -1 not coded, -2 a coded slice the pass failed (the whole-file call would demote it and
// re-segment, moving every later chain: the caller compresses the file whole instead).
int compress_chain_range(avr_ctx* c, const uint8_t* in, size_t n, int world, int rank, ChainRangeOut* o) {
  HIP_TRY(c, hipSetDevice(c->device));
  ParsedFile pf;
  if (int r = parse_file(c, in, n, &pf, /*views=*/true)) return r;
  const size_t ns = pf.slices.size();
  std::vector<char> ok(ns), coded(ns);
  for (size_t i = 0; i < ns; i++) ok[i] = recodable_candidate(pf.slices[i]);
  const std::vector<const uint8_t*> found = segment(in, n, pf, ok);
  for (size_t i = 0; i < ns; i++) coded[i] = found[i] != nullptr;
  const auto [lo, hi] =
      rank_slices(chain_starts(coded), world, rank, [&](int i) { return coded[i] ? pf.slices[i].size : 0; });
  Plan rp;
  std::vector<avr_slice_result> rr;
  Bytes ro;
  if (hi > lo) {
    reference_plan(&rp, pf, lo, hi, coded, /*chained=*/true);
    rp.file_first.push_back((int)rp.descs.size());
    if (int r = run_plan(c, 0, true, rp, &rr, &ro, false, 0)) return r;
  }
  pack_range(lo, rp.descs, rr, ro.data(), -1, [](int32_t) { return (int32_t)-2; }, o);
  return AVR_OK;
}

// decompressor::run (recode.cpp:1312-1357) of a chained-model container, this rank's chains only:
// the container planned as the whole-file call plans it (every slice, coded or not: the reference
// model turns frames over on uncoded ones), the chains cut by the same rule, and the plan's slices
// [lo, hi) of this rank's chains regenerated on the device (one workgroup per chain).  status per
// plan slice: 0 regenerated (bytes), 1 not coded, < 0 failed.  The caller splices the gathered
// slices with avr_dec_plan_splice (rank 0's plan of the same container).
int decompress_chain_range(avr_ctx* c, const uint8_t* avrc, size_t n, int world, int rank, ChainRangeOut* o) {
  HIP_TRY(c, hipSetDevice(c->device));
  DecJob j;
  Plan full;
  full.layout_only = true;
  if (int r = decompress_setup(c, avrc, n, &j, &full)) return r;
  if (!reference_model(j.model)) return fail(c, AVR_ERR_UNSUPPORTED, "not a reference- or chained-model container");
  const int ns = (int)full.descs.size();
  const bool chained = j.model == AVR_MODEL_CHAINED;
  std::vector<char> coded(ns);
  for (int k = 0; k < ns; k++) coded[k] = full.descs[k].coded != 0;
  // the reference model (one chain per file) is a single unit; the chained model's chains
  const auto [lo, hi] = rank_slices(chained ? chain_starts(coded) : std::vector<int>{0, ns}, world, rank,
                                    [&](int k) { return coded[k] ? full.descs[k].payload_size : 0u; });
  // the range's re-coded streams: decompress_setup listed every coded slice's copy in plan order
  Plan sub;
  size_t ci = 0;
  for (int k = 0; k < hi; k++) {
    avr_slice_desc d = full.descs[k];
    const avr::PbCopy* cp = d.coded ? &full.arena_copies[ci++] : nullptr;
    if (k < lo) continue;
    if (cp) {
      append_aligned(&sub.arena, cp->src, cp->len, 16, &d.payload_offset);
      sub.max_w = std::max(sub.max_w, ring_cols(d));
    }
    sub.descs.push_back(d);
  }
  std::vector<avr_slice_result> rr;
  Bytes ro;
  if (hi > lo) {
    append_file_chains(&sub, 0, chained);   // the range starts at a chain's start: the file's cuts
    sub.file_first.push_back(hi - lo);
    if (int r = run_plan(c, 1, true, sub, &rr, &ro, false, 0)) return r;
  }
  pack_range(lo, sub.descs, rr, ro.data(), 1, [](int32_t s) { return std::min((int32_t)-1, s); }, o);
  return AVR_OK;
}

// a ChainRangeOut to the caller's malloc'd buffers (avr_free)
int export_range(const ChainRangeOut& o, int* lo, int* hi, int32_t** status, uint8_t** blob, size_t* blob_len,
                 uint64_t** offsets, uint32_t** lens) {
  const size_t nr = (size_t)(o.hi - o.lo);
  *status = (int32_t*)malloc(sizeof(int32_t) * std::max<size_t>(1, nr));
  *offsets = (uint64_t*)malloc(sizeof(uint64_t) * std::max<size_t>(1, nr));
  *lens = (uint32_t*)malloc(sizeof(uint32_t) * std::max<size_t>(1, nr));
  *blob = host_alloc(std::max<size_t>(1, o.blob.size()));
  if (!*status || !*offsets || !*lens || !*blob) {
    free(*status), free(*offsets), free(*lens), free(*blob);
    *status = nullptr, *offsets = nullptr, *lens = nullptr, *blob = nullptr;
    return AVR_ERR_OUT_OF_MEMORY;
  }
  if (nr) {
    memcpy(*status, o.status.data(), sizeof(int32_t) * nr);
    memcpy(*offsets, o.offsets.data(), sizeof(uint64_t) * nr);
    memcpy(*lens, o.lens.data(), sizeof(uint32_t) * nr);
  }
  if (!o.blob.empty()) memcpy(*blob, o.blob.data(), o.blob.size());
  *blob_len = o.blob.size();
  *lo = o.lo;
  *hi = o.hi;
  return AVR_OK;
}

}  // namespace

namespace avr_host {

// run_plan (avr_ctx.h; the hooks surface calls it too): defined after its callers above, and
// instantiated below for the two host buffers it is used with
template <class HostBuf>
int run_plan(avr_ctx* c, int mode, bool sequential, Plan& plan, std::vector<avr_slice_result>* res,
             HostBuf* out_host, bool verify, uint32_t flags, SliceCrcs* crcs) {
  const int n = (int)plan.descs.size();
  if (crcs) crcs->crc.clear(), crcs->status.clear();
  if (plan.fields()) flags |= avr::kFlagFields;
  // a parallel batch of progressive and field slices: the two kernels side by side
  const avr::FieldLane lane = !sequential && plan.mixed() ? c->field_lane() : avr::FieldLane();
  res->assign(n, avr_slice_result{0, 0, 0, 0, {0, 0, 0, 0, 0, 0}});
  uint64_t out_total = 0;
  for (auto& d : plan.descs) place_output(&d, &out_total);
  out_host->resize(out_total);
  if (!n) return AVR_OK;
  const double t_wall = now_s();
  HIP_TRY(c, c->in.reserve(plan.arena.size() + 4096));
  HIP_TRY(c, c->out.reserve(out_total + 4096));
  HIP_TRY(c, c->descs.reserve(sizeof(avr_slice_desc) * n));
  HIP_TRY(c, c->res.reserve(sizeof(avr_slice_result) * n));
  for (auto& e : c->ev)
    if (!e) HIP_TRY(c, hipEventCreate(&e));
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->in.p, plan.arena.data(), plan.arena.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->descs.p, plan.descs.data(), sizeof(avr_slice_desc) * n, hipMemcpyHostToDevice,
                            c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  int rm = kRModeFallback;
  if (sequential && mode == 0 && !getenv("AVR_RMODE_SEQUENTIAL") && rmode_parallel_pays(plan)) {
    rm = run_rmode_compress(c, plan, flags);
    if (rm < 0) return rm;
  }
  if (sequential && rm == AVR_OK) {
    // done: the parallel reference-model compress
  } else if (sequential) {
    // one workgroup per file (the reference model is sequential within a file only)
    const int nf = plan.n_files();
    avr::SeqFiles sf;
    sf.n_files = nf;
    size_t fbytes = 0;
    for (auto& d : plan.descs) fbytes = std::max(fbytes, (size_t)2 * d.mb_width * d.mb_height * 52);
    sf.frame_stride = (fbytes + 255) & ~(size_t)255;
    HIP_TRY(c, c->est.reserve(sizeof(uint16_t) * avr::kEstGlobal * (size_t)nf, true));
    HIP_TRY(c, c->frames.reserve(sf.frame_stride * nf + 64));
    HIP_TRY(c, c->frame_meta.reserve(sizeof(int) * (size_t)nf + 64));
    if (!plan.file_first.empty()) {
      HIP_TRY(c, c->file_first.reserve(sizeof(int) * plan.file_first.size()));
      HIP_TRY(c, hipMemcpyAsync(c->file_first.p, plan.file_first.data(), sizeof(int) * plan.file_first.size(),
                                hipMemcpyHostToDevice, c->stream));
      sf.file_first = c->file_first.as<int>();
    }
    HIP_TRY(c, avr::launch_slices(mode, true, c->tables.as<avr::EngineTables>(), c->descs.as<avr_slice_desc>(), n,
                                  plan.max_w, c->in.as<uint8_t>(), c->out.as<uint8_t>(), c->res.as<avr_slice_result>(),
                                  c->est.as<uint16_t>(), c->frames.as<uint8_t>(), c->frame_meta.as<int>(), nullptr,
                                  c->stream, sf, flags));
  } else {
    HIP_TRY(c, reserve_parallel(c, n, plan.max_w, lane.stream != nullptr));
    HIP_TRY(c, avr::launch_slices(mode, false, c->tables.as<avr::EngineTables>(), c->descs.as<avr_slice_desc>(), n,
                                  plan.max_w, c->in.as<uint8_t>(), c->out.as<uint8_t>(), c->res.as<avr_slice_result>(),
                                  c->est.as<uint16_t>(), nullptr, nullptr, c->order_or_null(), c->stream,
                                  avr::SeqFiles(), flags, c->queue.p, &lane));
  }
  std::vector<int32_t> verdict;
  if (verify && mode == 0 && !sequential) {
    HIP_TRY(c, c->regen.reserve(plan.arena.size() + 4096));
    HIP_TRY(c, c->dec_descs.reserve(sizeof(avr_slice_desc) * n));
    HIP_TRY(c, c->res_d.reserve(sizeof(avr_slice_result) * n));
    HIP_TRY(c, c->verdict.reserve(sizeof(int32_t) * n));
    avr_slice_desc* dd = c->dec_descs.as<avr_slice_desc>();
    avr_slice_result* rd = c->res_d.as<avr_slice_result>();
    HIP_TRY(c, avr::launch_derive_decompress(c->descs.as<avr_slice_desc>(), c->res.as<avr_slice_result>(), n, dd,
                                             c->stream));
    HIP_TRY(c, avr::launch_slices(1, false, c->tables.as<avr::EngineTables>(), dd, n, plan.max_w, c->out.as<uint8_t>(),
                                  c->regen.as<uint8_t>(), rd, c->est.as<uint16_t>(), nullptr, nullptr,
                                  c->order_or_null(), c->stream, avr::SeqFiles(),
                                  (plan.fields() ? avr::kFlagFields : 0u) | (flags & avr::kFlagP32), c->queue.p,
                                  &lane));
    HIP_TRY(c, avr::launch_verify(c->descs.as<avr_slice_desc>(), c->res.as<avr_slice_result>(), rd, n,
                                  c->in.as<uint8_t>(), c->regen.as<uint8_t>(), c->verdict.as<int32_t>(), c->stream));
    verdict.resize(n);
    HIP_TRY(c, hipMemcpyAsync(verdict.data(), c->verdict.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  }
  if (crcs) {
    // the payloads where the upload put them, or the regenerated bytes where the kernel left them
    HIP_TRY(c, c->crc.reserve(2 * sizeof(uint32_t) * n));
    crcs->crc.resize(n);
    crcs->status.resize(n);
    HIP_TRY(c, avr::launch_crc_slices(c->descs.as<avr_slice_desc>(), c->res.as<avr_slice_result>(), n, mode == 1,
                                      mode == 1 ? c->out.as<uint8_t>() : c->in.as<uint8_t>(),
                                      mode == 1 ? out_total : plan.arena.size(), c->crc.as<uint32_t>(),
                                      c->crc.as<int32_t>() + n, c->stream));
  }
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  if (crcs) {
    HIP_TRY(c, hipMemcpyAsync(crcs->crc.data(), c->crc.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(crcs->status.data(), c->crc.as<int32_t>() + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost,
                              c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(res->data(), c->res.p, sizeof(avr_slice_result) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_host->data(), c->out.p, out_total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  float ms[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++) HIP_TRY(c, hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
  c->phase.upload_s += 1e-3 * ms[0];
  c->phase.kernel_s += 1e-3 * ms[1];
  c->phase.download_s += 1e-3 * ms[2];
  c->plan_wall += now_s() - t_wall;
  for (int k = 0; k < (int)verdict.size(); k++)
    if ((*res)[k].status == 0 && verdict[k] != 1) (*res)[k].status = AVR_SLICE_NO_ROUNDTRIP;
  return AVR_OK;
}

template int run_plan(avr_ctx*, int, bool, Plan&, std::vector<avr_slice_result>*, Bytes*, bool, uint32_t, SliceCrcs*);
template int run_plan(avr_ctx*, int, bool, Plan&, std::vector<avr_slice_result>*, std::vector<uint8_t>*, bool, uint32_t,
                      SliceCrcs*);

}  // namespace avr_host

// ================================================================================ C ABI
extern "C" {

int avr_create(int device, avr_ctx** out) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return AVR_ERR_DEVICE;
  std::unique_ptr<avr_ctx> c(new avr_ctx());
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) return AVR_ERR_DEVICE;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return AVR_ERR_DEVICE;
  if (hipStreamCreateWithFlags(&c->split_stream, hipStreamNonBlocking) != hipSuccess) return AVR_ERR_DEVICE;
  {
    const char* e = getenv("AVR_SPLIT_BYTES");
    c->split_bytes = e ? (size_t)strtoull(e, nullptr, 10) : kSplitBytesDefault;
  }
  if (const char* e = getenv("AVR_RECODE_ESCAPED")) c->recode_escaped = strtol(e, nullptr, 10) != 0;
  if (const char* e = getenv("AVR_SPLIT_P32")) c->split_p32 = strtol(e, nullptr, 10) != 0;
  if (const char* e = getenv("AVR_CHECKSUMS")) c->checksums = strtol(e, nullptr, 10) != 0;
  if (const char* e = getenv("AVR_UNIT_CHECKSUMS")) c->unit_checksums = strtol(e, nullptr, 10) != 0;
  if (const char* e = getenv("AVR_FIELD_LANE"); !e || strcmp(e, "0") != 0) {
    if (hipStreamCreateWithFlags(&c->fld_stream, hipStreamNonBlocking) != hipSuccess) return AVR_ERR_DEVICE;
    for (auto& ev : c->fld_ev)
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return AVR_ERR_DEVICE;
  }
  avr::EngineTables t;
  build_tables(&t);
  if (!check_reciprocals(t)) return AVR_ERR_DEVICE;
  if (c->tables.reserve(sizeof(t)) != hipSuccess) return AVR_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(c->tables.p, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess) return AVR_ERR_DEVICE;
  // CU grouping of the slice kernels only where the dispatcher deals workgroups round-robin
  if (avr::probe_round_robin(avr::shared_bytes(120), &c->round_robin) != hipSuccess) return AVR_ERR_DEVICE;
  if (getenv("AVR_NO_SCHEDULE")) c->round_robin = false;
  *out = c.release();
  return AVR_OK;
}

void avr_destroy(avr_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;   // every DevBuf frees itself
}

const char* avr_last_error(const avr_ctx* c) { return c ? c->err.c_str() : "no context"; }

int avr_set_split_bytes(avr_ctx* c, size_t bytes) {
  if (!c || bytes >= ((size_t)1 << 28)) return AVR_ERR_INVALID_ARGUMENT;
  c->split_bytes = bytes;
  return AVR_OK;
}
size_t avr_get_split_bytes(const avr_ctx* c) { return c ? c->split_bytes : 0; }

int avr_set_split_p32(avr_ctx* c, int on) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  c->split_p32 = on != 0;
  return AVR_OK;
}
int avr_get_split_p32(const avr_ctx* c) { return c && c->split_p32; }

int avr_set_recode_escaped(avr_ctx* c, int on) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  c->recode_escaped = on != 0;
  return AVR_OK;
}
int avr_get_recode_escaped(const avr_ctx* c) { return c && c->recode_escaped; }

int avr_set_checksums(avr_ctx* c, int on) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  c->checksums = on != 0;
  return AVR_OK;
}
int avr_get_checksums(const avr_ctx* c) { return c && c->checksums; }

int avr_set_unit_checksums(avr_ctx* c, int on) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  c->unit_checksums = on != 0;
  return AVR_OK;
}
int avr_get_unit_checksums(const avr_ctx* c) { return c && c->unit_checksums; }

void avr_free(void* p) { free(p); }

int avr_last_phase_times(const avr_ctx* c, avr_phase_times* out) {
  if (!c || !out) return AVR_ERR_INVALID_ARGUMENT;
  *out = c->phase;
  return AVR_OK;
}

int avr_neighbor_tables(avr_ctx* c, uint8_t out[96]) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  static_assert(offsetof(avr::HotTables, nb_up) == offsetof(avr::HotTables, nb_left) + 48, "nb_left, nb_up adjacent");
  if (!c) {
    std::unique_ptr<avr::EngineTables> t(new avr::EngineTables());
    build_tables(t.get());
    memcpy(out, t->hot.nb_left, 96);
    return AVR_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t off = offsetof(avr::EngineTables, hot) + offsetof(avr::HotTables, nb_left);
  HIP_TRY(c, hipMemcpy(out, c->tables.as<uint8_t>() + off, 96, hipMemcpyDeviceToHost));
  return AVR_OK;
}

int avr_compress_file(avr_ctx* c, const uint8_t* in, size_t n, int model, uint8_t** out, size_t* out_len) {
  if (!c || !in || !out || !out_len || !valid_model(model)) return AVR_ERR_INVALID_ARGUMENT;
  int32_t st = 0;
  const int r = guarded(c, [&] { return compress_files(c, 1, &in, &n, model, out, out_len, &st); });
  return r ? r : st;
}

int avr_compress_files(avr_ctx* c, int n_files, const uint8_t* const* in, const size_t* in_len, int model,
                       uint8_t** out, size_t* out_len, int32_t* status) {
  if (!c || n_files < 0 || (n_files && (!in || !in_len || !out || !out_len)) || !valid_model(model))
    return AVR_ERR_INVALID_ARGUMENT;
  for (int f = 0; f < n_files; f++)
    if (!in[f]) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(c, [&] { return compress_files(c, n_files, in, in_len, model, out, out_len, status); });
}

int avr_decompress_file(avr_ctx* c, const uint8_t* in, size_t n, uint8_t** out, size_t* out_len) {
  if (!c || !in || !out || !out_len) return AVR_ERR_INVALID_ARGUMENT;
  int32_t st = 0;
  const int r = guarded(c, [&] { return decompress_files(c, 1, &in, &n, out, out_len, &st); });
  return r ? r : st;
}

int avr_decompress_files(avr_ctx* c, int n_files, const uint8_t* const* in, const size_t* in_len, uint8_t** out,
                         size_t* out_len, int32_t* status) {
  if (!c || n_files < 0 || (n_files && (!in || !in_len || !out || !out_len))) return AVR_ERR_INVALID_ARGUMENT;
  for (int f = 0; f < n_files; f++)
    if (!in[f]) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(c, [&] { return decompress_files(c, n_files, in, in_len, out, out_len, status); });
}

static int roundtrip_file(avr_ctx* c, const uint8_t* in, size_t n, int model, uint8_t** compressed,
                          size_t* compressed_len, avr_file_stats* stats) {
  if (!c || !in) return AVR_ERR_INVALID_ARGUMENT;
  if (!valid_model(model)) return AVR_ERR_INVALID_ARGUMENT;
  uint8_t *comp = nullptr, *dec = nullptr;
  size_t cn = 0, dn = 0;
  std::vector<Bill> cbill, dbill;
  int32_t st = 0;
  double tc = 0, td = 0;
  avr_phase_times pcomp{}, pdec{};
  uint32_t attempts = 0;
  auto add_phases = [](avr_phase_times* a, const avr_phase_times& b) {
    a->demux_s += b.demux_s, a->upload_s += b.upload_s, a->kernel_s += b.kernel_s;
    a->download_s += b.download_s, a->container_s += b.container_s, a->other_s += b.other_s;
  };
  bool same = false;
  // the parallel model's per-slice device check is left to the whole-file compare below; a file
  // that does not come back is compressed again with it (every slice that fails it stored as is)
  for (int attempt = parallel_model(model) ? 0 : 1; attempt < 2; attempt++) {
    free(comp);
    comp = nullptr;
    cn = 0;
    attempts++;
    const double t0 = now_s();
    if (int r = compress_files(c, 1, &in, &n, model, &comp, &cn, &st, &cbill, /*verify=*/attempt > 0)) {
      free(comp);
      return r;
    }
    if (st) {
      free(comp);
      return st;
    }
    const double t1 = now_s();
    add_phases(&pcomp, c->phase);
    const uint8_t* cp = comp;
    int r = decompress_files(c, 1, &cp, &cn, &dec, &dn, &st, &dbill);
    if (!r) r = st;
    const double t2 = now_s();
    add_phases(&pdec, c->phase);
    tc += t1 - t0;
    td += t2 - t1;
    same = !r && dn == n && memcmp(dec, in, n) == 0;
    free(dec);
    dec = nullptr;
    if (attempt == 0 && getenv("AVR_ROUNDTRIP_FORCE_VERIFY")) continue;   // tests: the second path
    if (same) break;
    if (attempt == 1 && r) {
      free(comp);
      return r;
    }
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->file_bytes = n;
    stats->compress_s = tc;
    stats->decompress_s = td;
    stats->attempts = attempts;
    stats->compress_phases = pcomp;
    stats->decompress_phases = pdec;
    for (int i = 0; i < 6; i++) {
      stats->bill[i] = cbill[0][i];
      stats->cabac_bill[i] = dbill[0][i];
    }
    std::vector<avr::PbBlock> blocks;
    std::string v;
    if (avr::pb_parse(comp, cn, &blocks, &v)) {
      for (auto& b : blocks) {
        if (b.has_cabac) stats->coded_slices++, stats->payload_bytes += (uint64_t)b.size, stats->recoded_bytes += b.cabac_len;
        if (b.has_skip) stats->skipped_slices++;
      }
      stats->slices = stats->coded_slices + stats->skipped_slices;
    }
  }
  if (compressed && compressed_len) {
    *compressed = comp;
    *compressed_len = cn;
  } else {
    free(comp);
  }
  if (!same) return fail(c, AVR_ERR_ROUNDTRIP, "Compress-decompress roundtrip failed.");
  return AVR_OK;
}
int avr_roundtrip_file(avr_ctx* c, const uint8_t* in, size_t n, int model, uint8_t** compressed,
                       size_t* compressed_len, avr_file_stats* stats) {
  return guarded(c, [&] { return roundtrip_file(c, in, n, model, compressed, compressed_len, stats); });
}

// roundtrip_file's two attempts over a corpus: each attempt is one batched compress_files and one
// batched decompress_files over the files still open.
static int roundtrip_files(avr_ctx* c, int nf, const uint8_t* const* in, const size_t* in_len, int model,
                           uint8_t** out, size_t* out_len, int32_t* status, double* times) {
  for (int f = 0; f < nf; f++) out[f] = nullptr, out_len[f] = 0, status[f] = AVR_ERR_ROUNDTRIP;
  double tc = 0, td = 0;
  std::vector<int> open(nf);
  for (int f = 0; f < nf; f++) open[f] = f;
  const bool force_verify = getenv("AVR_ROUNDTRIP_FORCE_VERIFY") != nullptr;   // tests: the second path
  for (int attempt = parallel_model(model) ? 0 : 1; attempt < 2 && !open.empty(); attempt++) {
    const int k = (int)open.size();
    std::vector<const uint8_t*> ins(k);
    std::vector<size_t> lens(k), clen(k, 0), dlen(k, 0);
    std::vector<uint8_t*> comp(k, nullptr), dec(k, nullptr);
    std::vector<int32_t> cst(k, AVR_OK), dst(k, AVR_OK);
    for (int j = 0; j < k; j++) ins[j] = in[open[j]], lens[j] = in_len[open[j]];
    auto free_all = [&] {
      for (int j = 0; j < k; j++) free(comp[j]), free(dec[j]);
    };
    const double t0 = now_s();
    if (int r = compress_files(c, k, ins.data(), lens.data(), model, comp.data(), clen.data(), cst.data(), nullptr,
                               /*verify=*/attempt > 0)) {
      free_all();
      return r;
    }
    const double t1 = now_s();
    // decompress the containers that came out (a file whose compress failed keeps its status)
    std::vector<int> idx;
    std::vector<const uint8_t*> cin;
    std::vector<size_t> cn;
    for (int j = 0; j < k; j++)
      if (cst[j] == AVR_OK) idx.push_back(j), cin.push_back(comp[j]), cn.push_back(clen[j]);
    std::vector<uint8_t*> dout(idx.size(), nullptr);
    std::vector<size_t> dn(idx.size(), 0);
    std::vector<int32_t> ds(idx.size(), AVR_OK);
    if (!idx.empty()) {
      if (int r = decompress_files(c, (int)idx.size(), cin.data(), cn.data(), dout.data(), dn.data(), ds.data())) {
        for (uint8_t* p : dout) free(p);
        free_all();
        return r;
      }
    }
    for (size_t q = 0; q < idx.size(); q++) dec[idx[q]] = dout[q], dlen[idx[q]] = dn[q], dst[idx[q]] = ds[q];
    const double t2 = now_s();
    tc += t1 - t0;
    td += t2 - t1;
    std::vector<int> again;
    for (int j = 0; j < k; j++) {
      const int f = open[j];
      const bool same = cst[j] == AVR_OK && dst[j] == AVR_OK && dlen[j] == in_len[f] &&
                        (in_len[f] == 0 || memcmp(dec[j], in[f], in_len[f]) == 0);
      free(out[f]);
      out[f] = nullptr, out_len[f] = 0;
      if (same && !(attempt == 0 && force_verify)) {
        out[f] = comp[j], out_len[f] = clen[j], comp[j] = nullptr;
        status[f] = AVR_OK;
      } else if (attempt == 0) {
        again.push_back(f);
      } else {
        status[f] = cst[j] != AVR_OK ? cst[j] : AVR_ERR_ROUNDTRIP;
      }
    }
    free_all();
    open.swap(again);
  }
  if (times) times[0] = tc, times[1] = td;
  for (int f = 0; f < nf; f++)
    if (status[f] != AVR_OK) fail(c, status[f], "file " + std::to_string(f) + ": compress-decompress roundtrip failed");
  return AVR_OK;
}
int avr_roundtrip_files(avr_ctx* c, int n_files, const uint8_t* const* in, const size_t* in_len, int model,
                        uint8_t** out, size_t* out_len, int32_t* status, double* times) {
  if (!c || n_files < 0 || (n_files && (!in || !in_len || !out || !out_len || !status)) || !valid_model(model))
    return AVR_ERR_INVALID_ARGUMENT;
  for (int f = 0; f < n_files; f++)
    if (!in[f]) return AVR_ERR_INVALID_ARGUMENT;
  const int r = guarded(c, [&] { return roundtrip_files(c, n_files, in, in_len, model, out, out_len, status, times); });
  if (r != AVR_OK) {
    // a batch that failed as a whole leaves no partial outputs: every file gets the error
    for (int f = 0; f < n_files; f++) {
      free(out[f]);
      out[f] = nullptr;
      out_len[f] = 0;
      status[f] = r;
    }
  }
  return r;
}

static int batch(avr_ctx* c, int mode, const avr_slice_desc* d_desc, int n, int max_w, int max_h,
                 const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, int model, void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_in || !d_out || !d_res)) || max_w <= 0 || max_h <= 0 || !valid_model(model) ||
      model == AVR_MODEL_CHAINED)   // a slice batch has no file to chain over: whole-file calls only
    return AVR_ERR_INVALID_ARGUMENT;
  if (avr::shared_bytes(max_w) > 160 * 1024) return fail(c, AVR_ERR_UNSUPPORTED, "picture too wide for the LDS ring");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  if (model == AVR_MODEL_REFERENCE) {
    HIP_TRY(c, c->est.reserve(sizeof(uint16_t) * avr::kEstGlobal, true));
    HIP_TRY(c, c->frames.reserve((size_t)2 * max_w * max_h * 52 + 64));
    HIP_TRY(c, c->frame_meta.reserve(64));
    HIP_TRY(c, avr::launch_slices(mode, true, c->tables.as<avr::EngineTables>(), d_desc, n, max_w, d_in, d_out, d_res,
                                  c->est.as<uint16_t>(), c->frames.as<uint8_t>(), c->frame_meta.as<int>(), nullptr, s,
                                  avr::SeqFiles(), avr::kFlagFields));
    return AVR_OK;
  }
  HIP_TRY(c, reserve_parallel(c, n, max_w));
  HIP_TRY(c, avr::launch_slices(mode, false, c->tables.as<avr::EngineTables>(), d_desc, n, max_w, d_in, d_out, d_res,
                                c->est.as<uint16_t>(), nullptr, nullptr, c->order_or_null(), s, avr::SeqFiles(),
                                avr::kFlagFields | coder_flag(model), c->queue.p));
  return AVR_OK;
}

int avr_compress_slices(avr_ctx* c, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                        const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, int model, void* stream) {
  return batch(c, 0, d_desc, n, max_mb_width, max_mb_height, d_in, d_out, d_res, model, stream);
}

int avr_decompress_slices(avr_ctx* c, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                          const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, int model, void* stream) {
  return batch(c, 1, d_desc, n, max_mb_width, max_mb_height, d_in, d_out, d_res, model, stream);
}

int avr_roundtrip_slices(avr_ctx* c, const avr_slice_desc* d_desc, int n, int max_w, int max_h, const uint8_t* d_in,
                         uint8_t* d_work, uint8_t* d_regen, avr_slice_desc* d_dec_desc, avr_slice_result* d_res_c,
                         avr_slice_result* d_res_d, int32_t* d_verdict, int model, void* stream) {
  if (!c || n < 0 || (n && (!d_regen || !d_dec_desc || !d_res_d || !d_verdict))) return AVR_ERR_INVALID_ARGUMENT;
  if (int r = batch(c, 0, d_desc, n, max_w, max_h, d_in, d_work, d_res_c, model, stream)) return r;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(c, avr::launch_derive_decompress(d_desc, d_res_c, n, d_dec_desc, s));
  if (int r = batch(c, 1, d_dec_desc, n, max_w, max_h, d_work, d_regen, d_res_d, model, stream)) return r;
  HIP_TRY(c, avr::launch_verify(d_desc, d_res_c, d_res_d, n, d_in, d_regen, d_verdict, s));
  return AVR_OK;
}

int avr_derive_decompress_descs(avr_ctx* c, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c, int n,
                                avr_slice_desc* d_dec_desc, void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_res_c || !d_dec_desc))) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_derive_decompress(d_desc, d_res_c, n, d_dec_desc, (hipStream_t)stream));
  return AVR_OK;
}

int avr_verify_slices(avr_ctx* c, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c,
                      const avr_slice_result* d_res_d, int n, const uint8_t* d_in, const uint8_t* d_regen,
                      int32_t* d_verdict, void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_res_c || !d_res_d || !d_in || !d_regen || !d_verdict)))
    return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_verify(d_desc, d_res_c, d_res_d, n, d_in, d_regen, d_verdict, (hipStream_t)stream));
  return AVR_OK;
}

// the two chain-range calls: range = compress_chain_range or decompress_chain_range
static int chain_range(decltype(compress_chain_range)* range, avr_ctx* c, const uint8_t* in, size_t n, int world, int rank,
                       int* lo, int* hi, int32_t** status, uint8_t** blob, size_t* blob_len, uint64_t** offsets,
                       uint32_t** lens) {
  if (!c || !in || world < 1 || rank < 0 || rank >= world || !lo || !hi || !status || !blob || !blob_len || !offsets ||
      !lens)
    return AVR_ERR_INVALID_ARGUMENT;
  *status = nullptr, *blob = nullptr, *offsets = nullptr, *lens = nullptr;
  return guarded(c, [&]() -> int {
    ChainRangeOut o;
    if (int r = range(c, in, n, world, rank, &o)) return r;
    return export_range(o, lo, hi, status, blob, blob_len, offsets, lens);
  });
}
int avr_compress_chain_range(avr_ctx* c, const uint8_t* file, size_t n, int world, int rank, int* lo, int* hi,
                             int32_t** status, uint8_t** recoded, size_t* recoded_len, uint64_t** offsets,
                             uint32_t** lens) {
  return chain_range(compress_chain_range, c, file, n, world, rank, lo, hi, status, recoded, recoded_len, offsets, lens);
}
int avr_decompress_chain_range(avr_ctx* c, const uint8_t* avrc, size_t n, int world, int rank, int* lo, int* hi,
                               int32_t** status, uint8_t** regen, size_t* regen_len, uint64_t** offsets,
                               uint32_t** lens) {
  return chain_range(decompress_chain_range, c, avrc, n, world, rank, lo, hi, status, regen, regen_len, offsets, lens);
}

int avr_slice_kernel(avr_ctx* c, int decompress, int n, int max_mb_width, int* kind) {
  if (!c || !kind || n < 0 || max_mb_width <= 0) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  *kind = avr::parallel_kernel_kind(decompress ? 1 : 0, n, max_mb_width);
  return AVR_OK;
}

int avr_pack_outputs(avr_ctx* c, const avr_slice_desc* d_desc, const avr_slice_result* d_res, int n,
                     const uint8_t* d_out, uint8_t* d_packed, uint64_t* d_offsets, void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_res || !d_out || !d_packed || !d_offsets))) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_pack(d_desc, d_res, n, d_out, d_packed, d_offsets, (hipStream_t)stream));
  return AVR_OK;
}

int avr_crc_spans(avr_ctx* c, const uint8_t* d_buf, size_t buf_len, const uint64_t* d_off, const uint32_t* d_len, int n,
                  uint32_t* d_crc, int32_t* d_status, void* stream) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  if (n <= 0) return AVR_OK;
  if (!d_buf || !d_off || !d_len || !d_crc || !d_status) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_crc_spans(d_buf, buf_len, d_off, d_len, n, d_crc, d_status, (hipStream_t)stream));
  return AVR_OK;
}

// The units of a piece plan on the device: the split kernel (one workgroup per unit) on the caller's
// stream, from the caller's device-resident descriptors, streams and seam records.  The piece array
// is checked here, before anything is launched: a record index outside d_recs would be read.
// model: which of the two split kernels (the coder is a template parameter of the kernel).
int avr_decompress_pieces_m(avr_ctx* c, int model, const avr_slice_desc* d_desc, const avr_piece* pieces, int n,
                            int max_w, int max_h, const uint8_t* d_recs, int n_recs, size_t rec_stride,
                            const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, void* stream) {
  if (!c || !parallel_model(model) || n < 0 || n_recs < 0 || (n && (!d_desc || !pieces || !d_in || !d_out || !d_res)) || (n_recs && !d_recs) ||
      max_w <= 0 || max_h <= 0)
    return AVR_ERR_INVALID_ARGUMENT;
  if (max_w > avr::kMringCols || rec_stride < avr::seam_rec_bytes(max_w) || rec_stride > UINT32_MAX)
    return fail(c, AVR_ERR_INVALID_ARGUMENT, "avr_decompress_pieces: picture wider than a seam record");
  for (int k = 0; k < n; k++)
    if (pieces[k].seam < -1 || pieces[k].seam >= n_recs)
      return fail(c, AVR_ERR_INVALID_ARGUMENT,
                  "avr_decompress_pieces: unit " + std::to_string(k) + " starts at a seam record outside the batch's");
  if (!n) return AVR_OK;
  return guarded(c, [&]() -> int {
    HIP_TRY(c, hipSetDevice(c->device));
    c->pc_host.resize(n);
    for (int k = 0; k < n; k++) c->pc_host[k] = avr::PieceCtl{pieces[k].seam, pieces[k].n_mbs, -1, 0};
    avr::SplitArgs sa;
    sa.recs = const_cast<uint8_t*>(d_recs);
    sa.rec_stride = (uint32_t)rec_stride;
    return launch_split_ctl(c, 1, d_desc, n, max_w, d_in, d_out, d_res, c->pc_host.data(), &c->pc_ctl, sa,
                            coder_flag(model), (hipStream_t)stream, nullptr);
  });
}
int avr_decompress_pieces(avr_ctx* c, const avr_slice_desc* d_desc, const avr_piece* pieces, int n, int max_w,
                          int max_h, const uint8_t* d_recs, int n_recs, size_t rec_stride, const uint8_t* d_in,
                          uint8_t* d_out, avr_slice_result* d_res, void* stream) {
  return avr_decompress_pieces_m(c, AVR_MODEL_PARALLEL, d_desc, pieces, n, max_w, max_h, d_recs, n_recs, rec_stride, d_in,
                                 d_out, d_res, stream);
}

int avr_pack_pieces(avr_ctx* c, const avr_slice_desc* d_desc, const avr_piece* d_pieces, const avr_slice_result* d_res,
                    int n, const uint8_t* d_out, uint8_t* d_packed, uint64_t* d_offsets, uint32_t* d_kept,
                    int32_t* d_status, void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_pieces || !d_res || !d_out || !d_packed || !d_offsets || !d_kept || !d_status)))
    return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_pack_pieces(d_desc, d_pieces, d_res, n, d_out, d_packed, d_offsets, d_kept, d_status,
                                     (hipStream_t)stream));
  return AVR_OK;
}

// The split walk (launch_split_walk) for a caller's device-resident batch (include/avrecode.h, ABI 8):
// on the caller's stream into the caller's records, cut counts and piece ends.  The slots are checked
// here, before anything is launched: a record outside d_recs would be written.
int avr_compress_split_slices_m(avr_ctx* c, int model, const avr_slice_desc* d_desc, int n, int max_w, int max_h,
                                const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res,
                                const avr_split_slot* slots, size_t split_bytes, uint8_t* d_recs, int n_recs,
                                size_t rec_stride, uint32_t* d_cuts, uint32_t* d_piece_end, void* stream) {
  if (!c || !parallel_model(model) || n < 0 || n_recs < 0 || (n && (!d_desc || !d_in || !d_out || !d_res || !slots || !d_cuts)) ||
      (n_recs && (!d_recs || !d_piece_end)) || max_w <= 0 || max_h <= 0)
    return AVR_ERR_INVALID_ARGUMENT;
  if (max_w > avr::kMringCols || rec_stride < avr::seam_rec_bytes(max_w) || rec_stride > UINT32_MAX)
    return fail(c, AVR_ERR_INVALID_ARGUMENT, "avr_compress_split_slices: picture wider than a seam record");
  if (!split_bytes || split_bytes >= ((size_t)1 << 28))
    return fail(c, AVR_ERR_INVALID_ARGUMENT, "avr_compress_split_slices: split_bytes outside (0, 2^28)");
  for (int k = 0; k < n; k++) {
    const avr_split_slot& s = slots[k];
    if (s.first == -1 && s.cap == 0) continue;
    if (s.first < 0 || s.cap == 0 || (uint64_t)s.first + s.cap > (uint64_t)n_recs)
      return fail(c, AVR_ERR_INVALID_ARGUMENT,
                  "avr_compress_split_slices: slice " + std::to_string(k) + " has its cut records outside the batch's");
  }
  if (!n) return AVR_OK;
  return guarded(c, [&]() -> int {
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_split_walk(c, d_desc, n, max_w, d_in, d_out, d_res, slots, d_recs, n_recs, rec_stride, d_cuts,
                             d_piece_end, split_bytes, coder_flag(model), (hipStream_t)stream, &c->sc_host, &c->sc_ctl,
                             nullptr);
  });
}
int avr_compress_split_slices(avr_ctx* c, const avr_slice_desc* d_desc, int n, int max_w, int max_h,
                              const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res,
                              const avr_split_slot* slots, size_t split_bytes, uint8_t* d_recs, int n_recs,
                              size_t rec_stride, uint32_t* d_cuts, uint32_t* d_piece_end, void* stream) {
  return avr_compress_split_slices_m(c, AVR_MODEL_PARALLEL, d_desc, n, max_w, max_h, d_in, d_out, d_res, slots,
                                     split_bytes, d_recs, n_recs, rec_stride, d_cuts, d_piece_end, stream);
}

int avr_stage_pieces(avr_ctx* c, avr_slice_desc* d_desc, const uint64_t* d_src, int n, const uint8_t* d_out,
                     size_t out_len, uint8_t* d_arena, size_t arena_cap, uint64_t* d_offsets, int32_t* d_status,
                     void* stream) {
  if (!c || n < 0 || (n && (!d_desc || !d_src || !d_out || !d_arena || !d_offsets || !d_status)) ||
      ((uintptr_t)d_arena & 15))
    return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_stage_pieces(d_desc, d_src, n, d_out, out_len, d_arena, arena_cap, d_offsets, d_status,
                                      (hipStream_t)stream));
  return AVR_OK;
}

int avr_verify_units(avr_ctx* c, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c, int n,
                     const uint32_t* d_first, int n_units, const uint8_t* d_in, const uint8_t* d_packed,
                     const uint64_t* d_offsets, const uint32_t* d_kept, const int32_t* d_unit_status,
                     int32_t* d_verdict, void* stream) {
  if (!c || n < 0 || n_units < 0 ||
      (n && (!d_desc || !d_res_c || !d_first || !d_in || !d_packed || !d_offsets || !d_kept || !d_unit_status ||
             !d_verdict)))
    return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_verify_units(d_desc, d_res_c, n, d_first, n_units, d_in, d_packed, d_offsets, d_kept,
                                      d_unit_status, d_verdict, (hipStream_t)stream));
  return AVR_OK;
}

// ------------------------------------------------------------------ range reads (ABI 12)
int avr_gather_spans(avr_ctx* c, const avr_span* d_spans, int n, const uint8_t* d_src, size_t src_len, uint8_t* d_dst,
                     size_t dst_len, int32_t* d_status, void* stream) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  if (n <= 0) return AVR_OK;
  if (!d_spans || !d_src || !d_dst || !d_status) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_gather_spans(d_spans, n, d_src, src_len, d_dst, dst_len, d_status, (hipStream_t)stream));
  return AVR_OK;
}

int avr_range_tails(avr_ctx* c, const avr_range_tail* d_tails, const avr_slice_result* d_res, int n, uint8_t* d_dst,
                    size_t dst_len, int32_t* d_status, void* stream) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  if (n <= 0) return AVR_OK;
  if (!d_tails || !d_res || !d_dst || !d_status) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_range_tails(d_tails, d_res, n, d_dst, dst_len, d_status, (hipStream_t)stream));
  return AVR_OK;
}

int avr_check_units(avr_ctx* c, const avr_range_tail* d_tails, const avr_unit_check* d_checks, const avr_slice_result* d_res,
                    int n, const uint8_t* d_src, size_t src_len, int32_t* d_status, void* stream) {
  if (!c) return AVR_ERR_INVALID_ARGUMENT;
  if (n <= 0) return AVR_OK;
  if (!d_tails || !d_checks || !d_res || !d_src || !d_status) return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, avr::launch_check_units(d_tails, d_checks, d_res, n, d_src, src_len, d_status, (hipStream_t)stream));
  return AVR_OK;
}

// One window of a random-access container (include/avrecode.h): planned on the host, then on the
// context's stream the upload of what the window needs, the selected units regenerated -- the pieces
// through avr_decompress_pieces_m, the whole slices through avr_decompress_slices, one launch after
// the other on rows grouped that way -- the gather into dst (the reader's window buffer, or the
// caller's device buffer) and the tails.  The statuses come back before any byte does.
static int reader_window(avr_reader* r, uint64_t off, size_t len, uint8_t* out, bool device, size_t* got) {
  avr_ctx* c = r->c;
  const avr_dec_plan* h = r->plan;
  const double t0 = now_s();
  if (int e = plan_range(h, off, len, 0, &r->rp)) return fail(c, e, "avr_reader_read: the window cannot be planned");
  const avr_range_info in = r->rp.info;
  if (!in.len) return AVR_OK;
  const int lo = in.unit_lo, nu = in.unit_hi - in.unit_lo, nsp = in.n_spans;
  if (h->plan.arena_copies.size() != h->units.size()) return fail(c, AVR_ERR_FORMAT, "avr_reader_read: not a piece plan");
  auto is_piece = [&](int u) {
    const avr_piece& p = h->unit_pieces[u];
    return p.seam >= 0 || p.n_mbs > 0 || p.keep != UINT32_MAX;
  };
  int np = 0;
  for (int k = 0; k < nu; k++) np += is_piece(lo + k);
  // the rows of the two launches: pieces first, then whole slices; the streams re-placed compactly
  // (16-byte aligned, >= 16 zero bytes after each), the outputs too
  r->descs.resize(nu);
  r->pieces.resize(nu);
  r->tails.resize(nu);
  std::vector<int> row(nu);
  uint64_t at = 0, work = 0;
  int ip = 0, iw = np, w_pieces = 1, w_whole = 1, mh = 1;
  for (int k = 0; k < nu; k++) {
    avr_slice_desc d = h->units[lo + k];
    if (h->plan.arena_copies[lo + k].len != d.payload_size)
      return fail(c, AVR_ERR_FORMAT, "avr_reader_read: not a piece plan");
    d.payload_offset = at;
    at = (at + d.payload_size + 16 + 15) & ~(uint64_t)15;
    place_output(&d, &work);
    const bool pc = is_piece(lo + k);
    row[k] = pc ? ip++ : iw++;
    (pc ? w_pieces : w_whole) = std::max(pc ? w_pieces : w_whole, pc ? d.mb_width : ring_cols(d));
    mh = std::max(mh, d.mb_height);
    r->descs[row[k]] = d;
    r->pieces[row[k]] = h->unit_pieces[lo + k];
    r->tails[row[k]] = r->rp.tails[k];
  }
  // the selected units' checksums (Block field 18), where their blocks carry them
  bool any_check = false;
  if (nu && !h->job.block_checked.empty()) {
    r->rp_checks.resize(nu);
    if (int e = avr_dec_plan_unit_crcs(h, lo, lo + nu, r->rp_checks.data()))
      return fail(c, e, "avr_reader_read: the units' checksums cannot be read");
    for (int k = 0; k < nu; k++) any_check |= r->rp_checks[k].have != 0;
  }
  const uint64_t upload = at + in.literal_bytes, work_base = (upload + 255) & ~(uint64_t)255;
  const uint64_t buf_len = work_base + work + 16;
  if (upload > r->stage_cap) {
    if (r->stage) (void)hipHostFree(r->stage);
    r->stage = nullptr;
    r->stage_cap = 0;
    const size_t cap = (size_t)((upload + 65535) & ~(uint64_t)65535);
    HIP_TRY(c, hipHostMalloc((void**)&r->stage, cap, hipHostMallocDefault));
    r->stage_cap = cap;
  }
  for (int k = 0; k < nu; k++) {
    const avr_slice_desc& d = r->descs[row[k]];
    const uint64_t end = (d.payload_offset + d.payload_size + 16 + 15) & ~(uint64_t)15;
    if (d.payload_size) memcpy(r->stage + d.payload_offset, h->plan.arena_copies[lo + k].src, d.payload_size);
    memset(r->stage + d.payload_offset + d.payload_size, 0, end - d.payload_offset - d.payload_size);
  }
  // the spans' sources in the read's buffer: the literals one after the other behind the streams, a
  // unit's bytes where its output was placed
  uint64_t lit = at;
  for (avr_span& s : r->rp.spans) {
    if (s.source == AVR_SPAN_LITERAL) {
      memcpy(r->stage + lit, r->avrc + s.src_off, s.len);   // plan_range has checked it inside the container
      s.src_off = lit;
      lit += s.len;
    } else {
      s.src_off += work_base + r->descs[row[s.source]].out_offset;
    }
  }
  HIP_TRY(c, r->buf.reserve(buf_len));
  HIP_TRY(c, r->d_descs.reserve(sizeof(avr_slice_desc) * std::max(1, nu)));
  HIP_TRY(c, r->d_res.reserve(sizeof(avr_slice_result) * std::max(1, nu)));
  HIP_TRY(c, r->d_tails.reserve(sizeof(avr_range_tail) * std::max(1, nu)));
  HIP_TRY(c, r->d_spans.reserve(sizeof(avr_span) * nsp));
  HIP_TRY(c, r->d_status.reserve(sizeof(int32_t) * ((size_t)nsp + nu)));
  if (!device) HIP_TRY(c, r->d_win.reserve(in.len));
  uint8_t* dst = device ? out : r->d_win.as<uint8_t>();
  uint8_t* d_in = r->buf.as<uint8_t>();
  uint8_t* d_work = d_in + work_base;
  avr_slice_desc* dd = r->d_descs.as<avr_slice_desc>();
  avr_slice_result* dr = r->d_res.as<avr_slice_result>();
  int32_t* d_st = r->d_status.as<int32_t>();
  hipStream_t st = c->stream;
  const double t1 = now_s();
  HIP_TRY(c, hipEventRecord(r->ev[0], st));
  HIP_TRY(c, hipMemcpyAsync(d_in, r->stage, upload, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(r->d_spans.p, r->rp.spans.data(), sizeof(avr_span) * nsp, hipMemcpyHostToDevice, st));
  if (nu) {
    HIP_TRY(c, hipMemcpyAsync(dd, r->descs.data(), sizeof(avr_slice_desc) * nu, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(r->d_tails.p, r->tails.data(), sizeof(avr_range_tail) * nu, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(dr, 0, sizeof(avr_slice_result) * nu, st));
  }
  HIP_TRY(c, hipEventRecord(r->ev[1], st));
  const int model = r->info.model;
  if (np)
    if (int e = avr_decompress_pieces_m(c, model, dd, r->pieces.data(), np, w_pieces, mh, r->d_recs.as<uint8_t>(),
                                        (int)(h->rec_stride ? h->recs.size() / h->rec_stride : 0), h->rec_stride, d_in,
                                        d_work, dr, st))
      return e;
  if (nu > np)
    if (int e = avr_decompress_slices(c, dd + np, nu - np, w_whole, mh, d_in, d_work, dr + np, model, st)) return e;
  HIP_TRY(c, avr::launch_gather_spans(r->d_spans.as<avr_span>(), nsp, d_in, buf_len, dst, in.len, d_st, st));
  HIP_TRY(c, avr::launch_range_tails(r->d_tails.as<avr_range_tail>(), dr, nu, dst, in.len, d_st + nsp, st));
  if (any_check) {   // each unit's share of its slice where it was regenerated, against the container's value
    r->checks.resize(nu);
    for (int k = 0; k < nu; k++) {
      r->checks[row[k]] = r->rp_checks[k];
      r->checks[row[k]].src_off = work_base + r->descs[row[k]].out_offset;
    }
    HIP_TRY(c, r->d_checks.reserve(sizeof(avr_unit_check) * nu));
    HIP_TRY(c, hipMemcpyAsync(r->d_checks.p, r->checks.data(), sizeof(avr_unit_check) * nu, hipMemcpyHostToDevice, st));
    HIP_TRY(c, avr::launch_check_units(r->d_tails.as<avr_range_tail>(), r->d_checks.as<avr_unit_check>(), dr, nu, d_in,
                                       buf_len, d_st + nsp, st));
  }
  HIP_TRY(c, hipEventRecord(r->ev[2], st));
  r->status.assign((size_t)nsp + nu, 0);
  r->res.assign(nu, avr_slice_result{});
  HIP_TRY(c, hipMemcpyAsync(r->status.data(), d_st, sizeof(int32_t) * r->status.size(), hipMemcpyDeviceToHost, st));
  if (nu) HIP_TRY(c, hipMemcpyAsync(r->res.data(), dr, sizeof(avr_slice_result) * nu, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const double t2 = now_s();
  for (int k = 0; k < nsp; k++)
    if (r->status[k])
      return fail(c, AVR_ERR_FORMAT, "avr_reader_read: span " + std::to_string(k) + " lies outside its buffers");
  for (int k = 0; k < nu; k++)
    if (int32_t s = r->status[nsp + row[k]]) {
      if (s == AVR_SLICE_CHECKSUM)
        return fail(c, AVR_ERR_CHECKSUM,
                    "avr_reader_read: unit " + std::to_string(lo + k) +
                        " of the container regenerated bytes that are not the ones its checksum was made from (CRC-32)");
      return fail(c, AVR_ERR_FORMAT,
                  "avr_reader_read: unit " + std::to_string(lo + k) + " of the container failed to decode (" +
                      std::to_string(s) + ")");
    }
  if (!device) HIP_TRY(c, hipMemcpy(out, dst, in.len, hipMemcpyDeviceToHost));
  const double t3 = now_s();
  avr_read_stats& ls = r->last;
  ls = avr_read_stats{};
  ls.units = (uint64_t)nu;
  ls.pieces = (uint64_t)np;
  for (const avr_slice_result& x : r->res) ls.regenerated_bytes += x.out_len;
  ls.literal_bytes = in.literal_bytes;
  ls.spans = (uint64_t)nsp;
  float up = 0, kn = 0;
  HIP_TRY(c, hipEventElapsedTime(&up, r->ev[0], r->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&kn, r->ev[1], r->ev[2]));
  ls.phases.demux_s = t1 - t0;
  ls.phases.upload_s = up * 1e-3;
  ls.phases.kernel_s = kn * 1e-3;
  ls.phases.download_s = t3 - t2;
  ls.phases.other_s = std::max(0.0, (t3 - t0) - ls.phases.demux_s - ls.phases.upload_s - ls.phases.kernel_s -
                                        ls.phases.download_s);
  *got = (size_t)in.len;
  return AVR_OK;
}

static int reader_read(avr_reader* r, uint64_t off, size_t len, uint8_t* out, bool device, size_t* got) {
  if (!r || !got) return AVR_ERR_INVALID_ARGUMENT;
  *got = 0;
  avr_ctx* c = r->c;
  if (off + len < off) return fail(c, AVR_ERR_INVALID_ARGUMENT, "avr_reader_read: off + len overflows");
  if (!len || off >= r->info.file_size) return AVR_OK;
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(c, [&]() -> int {
    HIP_TRY(c, hipSetDevice(c->device));
    if (r->info.random_access) {
      const int e = reader_window(r, off, len, out, device, got);
      if (e) (void)hipStreamSynchronize(c->stream);   // nothing of a failed read stays in flight over the reader's buffers
      return e;
    }
    // no random access: the whole file once, through the whole-file call (a checked container is checked)
    if (!r->file) {
      uint8_t* f = nullptr;
      size_t fl = 0;
      if (int e = avr_decompress_file(c, r->avrc, r->n, &f, &fl)) return e;
      r->file = f;
      r->file_len = fl;
      r->last = avr_read_stats{};
      r->last.phases = c->phase;
    }
    if (off >= r->file_len) return AVR_OK;
    const size_t m = (size_t)std::min<uint64_t>(len, r->file_len - off);
    if (device) HIP_TRY(c, hipMemcpy(out, r->file + off, m, hipMemcpyHostToDevice));
    else memcpy(out, r->file + off, m);
    *got = m;
    return AVR_OK;
  });
}

int avr_reader_open(avr_ctx* c, const uint8_t* avrc, size_t n, avr_reader** out) {
  if (!c || !avrc || !out) return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(c, [&]() -> int {
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<avr_reader> r(new avr_reader());
    r->c = c;
    r->avrc = avrc;
    r->n = n;
    if (int e = avr_dec_plan_new(&r->plan)) return fail(c, e, "avr_reader_open: no plan handle");
    int ns = 0, nu = 0, mw = 0, mh = 0, nr = 0;
    size_t al = 0, wl = 0, rs = 0;
    int e = avr_dec_plan_load_pieces(r->plan, avrc, n, &ns, &nu, &al, &wl, &mw, &mh, &nr, &rs);
    const bool pieces = e == AVR_OK;
    // the reference and chained models chain their slices: no units, the sizes from a slice plan
    if (e == AVR_ERR_UNSUPPORTED) e = avr_dec_plan_load(r->plan, avrc, n, &ns, &al, &wl, &mw, &mh);
    if (e) return fail(c, e, "avr_reader_open: not a container this library reads");
    const avr_dec_plan* h = r->plan;
    r->info.file_size = h->block_off.back();
    r->info.model = h->job.model;
    r->info.random_access = pieces && !h->escapes;
    r->info.n_blocks = (int32_t)h->job.blocks.size();
    r->info.n_units = r->info.random_access ? nu : 0;
    r->info.checked = h->job.has_crc;
    {   // every coded block carries unit checksums (Block field 18)
      bool coded = false, all = true;
      for (size_t i = 0; i < h->job.blocks.size(); i++)
        if (h->job.blocks[i].has_cabac) coded = true, all = all && h->job.unit_checked(i);
      r->info.unit_checked = coded && all;
    }
    if (r->info.random_access) {
      for (auto& ev : r->ev) HIP_TRY(c, hipEventCreate(&ev));
      HIP_TRY(c, r->d_recs.reserve(std::max<size_t>(64, h->recs.size())));
      if (!h->recs.empty()) HIP_TRY(c, hipMemcpy(r->d_recs.p, h->recs.data(), h->recs.size(), hipMemcpyHostToDevice));
    }
    *out = r.release();
    return AVR_OK;
  });
}

int avr_reader_info(const avr_reader* r, avr_reader_info_t* info) {
  if (!r || !info) return AVR_ERR_INVALID_ARGUMENT;
  *info = r->info;
  return AVR_OK;
}

int avr_reader_read(avr_reader* r, uint64_t off, size_t len, uint8_t* out, size_t* got) {
  return reader_read(r, off, len, out, false, got);
}

int avr_reader_read_device(avr_reader* r, uint64_t off, size_t len, uint8_t* d_out, size_t* got) {
  return reader_read(r, off, len, d_out, true, got);
}

int avr_reader_span(const avr_reader* r, uint64_t off, uint64_t* lo, uint64_t* hi, int* coded) {
  if (!r || !lo || !hi || !coded || off >= r->info.file_size) return AVR_ERR_INVALID_ARGUMENT;
  const avr_dec_plan* h = r->plan;
  const size_t i = block_of_offset(h, off);
  *lo = h->block_off[i];
  *hi = h->block_off[i + 1];
  *coded = h->job.blocks[i].has_cabac ? 1 : 0;
  return AVR_OK;
}

int avr_reader_last(const avr_reader* r, avr_read_stats* out) {
  if (!r || !out) return AVR_ERR_INVALID_ARGUMENT;
  *out = r->last;
  return AVR_OK;
}

void avr_reader_close(avr_reader* r) {
  if (!r) return;
  (void)hipSetDevice(r->c->device);
  if (r->c->stream) (void)hipStreamSynchronize(r->c->stream);
  delete r;   // its events, pinned buffer, plan and device buffers go with it
}

static int synthesize_stream(avr_ctx* c, const avr_synth_params* p, int n, uint8_t** out, size_t* out_len) {
  if (!c || !p || n <= 0 || !out || !out_len || p->mb_width <= 0 || p->mb_height <= 0 || p->slice_type < 0 ||
      p->slice_type > 2 || p->chroma_format_idc < 1 || p->chroma_format_idc > 3 || p->gop_length < 0 ||
      p->repeat < 0 || p->structure < 0 || p->structure > 3 || (p->structure && (p->mb_height & 1)))
    return AVR_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  Plan plan;
  // a coded picture: the frame, or (field pictures) each of its two fields in turn, the top
  // field first (structure 1) or the bottom field first (3)
  const bool paff = p->structure == 1 || p->structure == 3;
  const int fields = paff ? 2 : 1;
  const int mbs = p->mb_width * p->mb_height / fields;
  // MBAFF slices start on a macroblock pair
  const int unit = p->structure == 2 ? 2 : 1;
  const int spp = std::max(1, std::min(p->slices_per_picture, mbs / unit));
  std::vector<int> pic_of, first_of;
  for (int i = 0; i < n * fields * spp; i++) {
    const int pic = i / (spp * fields), fi = (i / spp) % fields, j = i % spp;
    const int first = unit * (int)((int64_t)j * (mbs / unit) / spp);
    const int next = unit * (int)((int64_t)(j + 1) * (mbs / unit) / spp);
    pic_of.push_back(pic);
    first_of.push_back(first);
    avr_slice_desc d;
    memset(&d, 0, sizeof(d));
    // GOP: an IDR I picture every gop_length pictures; with slice_type B the pictures between
    // follow B B P B B P ... (decode order), with P every picture between
    const int g = p->gop_length > 0 ? pic % p->gop_length : -1;
    const int st = g == 0 ? 2 : (g > 0 && p->slice_type == 1 && g % 3 == 0) ? 0 : p->slice_type;
    d.slice_type = st;
    d.slice_qp = p->slice_qp;
    d.cabac_init_idc = st == 2 ? -1 : 0;
    d.mb_width = p->mb_width;
    d.mb_height = p->mb_height;
    d.num_ref_idx_l0 = st == 2 ? 0 : std::max(1, p->num_ref_idx_l0);
    d.num_ref_idx_l1 = st == 1 ? std::max(1, p->num_ref_idx_l1) : 0;
    d.chroma_array_type = p->chroma_format_idc;
    d.transform_8x8_mode = p->transform_8x8_mode;
    d.direct_8x8_inference = 1;
    d.x264_build = -1;
    d.picture_id = pic;
    d.first_mb = first;
    d.coded = 1;
    d.structure = paff ? ((fi ^ (p->structure == 3)) ? AVR_STRUCT_BOTTOM_FIELD : AVR_STRUCT_TOP_FIELD)
                : p->structure == 2 ? AVR_STRUCT_MBAFF : AVR_STRUCT_FRAME;
    d.payload_offset = p->seed * 0x100000001B3ull + (uint64_t)i;  // generator seed
    d.payload_size = (uint32_t)(next - first);                    // generator: macroblocks to emit
    d.out_capacity = (uint32_t)std::min<uint64_t>((uint64_t)mbs * 384 + 4096, 0x7fffffffu);
    plan.descs.push_back(d);
  }
  plan.max_w = p->structure == 2 ? 3 * p->mb_width + 7 : p->mb_width;
  plan.arena.assign(16, 0);
  std::vector<avr_slice_result> res;
  std::vector<uint8_t> outb;
  if (int r = run_plan(c, 2, false, plan, &res, &outb)) return r;
  std::vector<uint8_t> stream;
  avr::synth_write_parameter_sets(&stream, *p);
  for (int i = 0; i < (int)plan.descs.size(); i++)
    if (res[i].status != 0) return fail(c, AVR_ERR_DEVICE, "generator failed on slice " + std::to_string(i));
  const int reps = std::max(1, p->repeat);
  // the tiled stream goes straight into the caller's buffer (one copy of it in host memory): each
  // NAL unit is written to a scratch vector and appended; 64 B per slice bound its header and
  // start code (checked at every append)
  size_t bytes = 0;
  for (int i = 0; i < (int)plan.descs.size(); i++) bytes += res[i].out_len + 64;
  if ((uint64_t)bytes * reps > kMaxSynthBytes) return fail(c, AVR_ERR_INVALID_ARGUMENT, "stream too large");
  const size_t cap = stream.size() + bytes * reps;
  uint8_t* o = (uint8_t*)malloc(cap);
  if (!o) return fail(c, AVR_ERR_OUT_OF_MEMORY, "synthetic stream: host allocation failed");
  memcpy(o, stream.data(), stream.size());
  size_t at = stream.size();
  std::vector<uint8_t> nal;
  for (int t = 0; t < reps; t++)
    for (int i = 0; i < (int)plan.descs.size(); i++) {
      nal.clear();
      avr::synth_write_slice(&nal, *p, plan.descs[i].slice_type, t * n + pic_of[i], plan.descs[i].structure,
                             paff && (i / spp) % 2 == 1, first_of[i], outb.data() + plan.descs[i].out_offset,
                             res[i].out_len);
      if (at + nal.size() > cap) {
        free(o);
        return fail(c, AVR_ERR_DEVICE, "synthetic stream: slice header larger than its bound");
      }
      memcpy(o + at, nal.data(), nal.size());
      at += nal.size();
    }
  *out = o;
  *out_len = at;
  return AVR_OK;
}
int avr_synthesize_stream(avr_ctx* c, const avr_synth_params* p, int n, uint8_t** out, size_t* out_len) {
  return guarded(c, [&] { return synthesize_stream(c, p, n, out, out_len); });
}

}  // extern "C"

// Debug only (not part of include/avrecode.h): section cycle counters (32 slots) of an AVR_PROFILE build of
// the slice kernels (mode 0 compress, 1 decompress, 2 generate, 3/4 sequential compress/decompress), read and cleared.
// Diagnostic (AVR_PROFILE builds): 8 u32 per slice of the last parallel compress (mode 0) or
// decompress (1) launch: HW_ID of waves 0-2, XCC_ID, walker start/end cycle counters.
extern "C" int avr_debug_placement(int mode, uint32_t* out8n, int n) {
  hipError_t e = mode == 0 ? avr::placement_parallel_compress(out8n, n) : avr::placement_parallel_decompress(out8n, n);
  return e == hipSuccess ? AVR_OK : AVR_ERR_DEVICE;
}

extern "C" int avr_debug_profile(int mode, unsigned long long* out16) {
  hipError_t e = mode == 0 ? avr::profile_parallel_compress(out16)
               : mode == 1 ? avr::profile_parallel_decompress(out16)
               : mode == 3 ? avr::profile_sequential_compress(out16)
               : mode == 4 ? avr::profile_sequential_decompress(out16)
                           : avr::profile_parallel_generate(out16);
  return e == hipSuccess ? AVR_OK : AVR_ERR_DEVICE;
}
