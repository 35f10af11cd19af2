// The device context of the C ABI and what the translation units that launch device work share
// (internal; includes HIP -- the host-only side is avr_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include "avr_host.h"
#include "avr_kernels.h"

namespace avr_host {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  // zero: a fresh allocation starts zeroed (the estimator tables rely on it, see kEstLogN)
  hipError_t reserve(size_t n, bool zero = false) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess && zero) e = hipMemset(p, 0, n);
    if (e == hipSuccess && zero) e = hipDeviceSynchronize();
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  ~DevBuf() { release(); }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

}  // namespace avr_host

struct avr_ctx : avr_host::ErrSink {
  using DevBuf = avr_host::DevBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf tables, est, frames, frame_meta, in, out, descs, res, packed, offsets, order;
  DevBuf queue;                                          // largest-first slice queue (launch_slices)
  DevBuf rm_goff, rm_counts, rm_stop, rm_off, rm_ops;   // parallel reference-model compress
  DevBuf regen, dec_descs, res_d, verdict;               // compress-side roundtrip check
  DevBuf file_first, file_op_off;                        // reference model over several files
  // the parallel model's long-slice split (split_compress / split_decompress): its own stream, so the
  // long slices' first pass overlaps the rest of the batch, and its own estimator scratch
  hipStream_t split_stream = nullptr;
  DevBuf sp_in, sp_out, sp_descs, sp_res, sp_ctl, sp_recs, sp_snapn, sp_est, sp_in2, sp_out2;
  // the second pieces launch of a decompress call that holds split blocks of both coders (one kernel
  // runs one coder): its input and output are sp_in2 / sp_out2, its descriptors, results, piece
  // controls and records these; sp_est is shared, the two launches being ordered on split_stream
  DevBuf sp2_descs, sp2_res, sp2_ctl, sp2_recs;
  size_t split_bytes = 0;   // avr_set_split_bytes / AVR_SPLIT_BYTES (0: no split)
  bool split_p32 = false;   // avr_set_split_p32 / AVR_SPLIT_P32: AVR_MODEL_PARALLEL32 reads split_bytes too
  bool recode_escaped = false;   // avr_set_recode_escaped / AVR_RECODE_ESCAPED (Block field 17)
  bool checksums = false;        // avr_set_checksums / AVR_CHECKSUMS (Metadata field 16: the file's CRC-32)
  DevBuf crc, sp_crc;            // per-slice CRCs, then their statuses: run_plan's batch, the split job's slices
  bool unit_checksums = false;   // avr_set_unit_checksums / AVR_UNIT_CHECKSUMS (Block field 18: a CRC-32 per unit)
  DevBuf sp_ucrc;                // the cut slices' unit spans (offsets, lengths), then their CRCs and statuses
  // avr_decompress_pieces: the batch's PieceCtl array, host (alive while its upload is in flight) and device
  std::vector<avr::PieceCtl> pc_host;
  DevBuf pc_ctl;
  // avr_compress_split_slices: the same for its batch (its own pair: the two calls may be in flight together)
  std::vector<avr::PieceCtl> sc_host;
  DevBuf sc_ctl;
  // a batch holding both progressive and field slices runs its field kernel beside the progressive
  // one (avr::FieldLane); AVR_FIELD_LANE=0 keeps the two in one stream, one after the other
  hipStream_t fld_stream = nullptr;
  hipEvent_t fld_ev[2] = {nullptr, nullptr};
  avr::FieldLane field_lane() const {
    avr::FieldLane l;
    if (fld_stream) l.stream = fld_stream, l.fork = fld_ev[0], l.join = fld_ev[1];
    return l;
  }
  bool round_robin = false;   // placement probe passed: the CU schedule (order) may be used
  int* order_or_null() { return round_robin ? order.as<int>() : nullptr; }
  // phase breakdown of the current / last whole-file call (avr_phase_times): run_plan adds the
  // device phases (HIP events ev[0..3] around its uploads, kernels and downloads) and its own wall
  // time (plan_wall); the file paths add the host phases
  avr_phase_times phase{};
  double plan_wall = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~avr_ctx() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (split_stream) (void)hipStreamDestroy(split_stream);
    for (auto& e : fld_ev)
      if (e) (void)hipEventDestroy(e);
    if (fld_stream) (void)hipStreamDestroy(fld_stream);
  }
};

// A reader (include/avrecode.h, ABI 12): an opened container that serves byte ranges of its file.
// Random access: the piece plan loaded once, the seam records on the device, and the buffers of a
// read -- all its own, sized by the largest window read so far, none proportional to the file and none
// shared with the whole-file calls.  Otherwise: the whole file, regenerated at the first read.
struct avr_reader {
  using DevBuf = avr_host::DevBuf;
  avr_ctx* c = nullptr;
  const uint8_t* avrc = nullptr;
  size_t n = 0;
  avr_dec_plan* plan = nullptr;
  avr_reader_info_t info{};
  // one device buffer per read: the selected units' streams and the window's literal bytes (the
  // upload), then the units' output space; gather_spans' source is the whole of it
  DevBuf buf, d_descs, d_res, d_spans, d_tails, d_status, d_recs, d_win, d_checks;
  std::vector<avr_unit_check> rp_checks, checks;   // a read's unit checks (Block field 18): in plan order, in launch-row order
  uint8_t* stage = nullptr;   // pinned: what a read uploads
  size_t stage_cap = 0;
  avr_host::RangePlan rp;
  std::vector<avr_slice_desc> descs;
  std::vector<avr_piece> pieces;
  std::vector<avr_range_tail> tails;
  std::vector<avr_slice_result> res;
  std::vector<int32_t> status;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the upload, the kernels, the downloads
  uint8_t* file = nullptr;    // without random access: the file, after the first read (avr_free)
  size_t file_len = 0;
  avr_read_stats last{};
  ~avr_reader() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stage) (void)hipHostFree(stage);
    if (plan) avr_dec_plan_free(plan);
    free(file);
  }
};

#define HIP_TRY(c, expr)                                                                             \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) return avr_host::fail(c, AVR_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

namespace avr_host {

// Upload plan, run the slice kernel over it (one launch, see launch_slices), download results and outputs.
// verify (parallel compress only): also decompress every slice's output on the device, apply the
// last-byte rule and compare with the payload (avr_roundtrip_slices); a slice whose output does not
// regenerate its payload gets status AVR_SLICE_NO_ROUNDTRIP, so no container ever holds a block that
// cannot be decompressed.
// out_host: a std::vector<uint8_t> or a Bytes (not zero-filled first: the download overwrites it)
// (defined in avr_api.cpp and instantiated there for both)
// crcs (checked containers): the CRC-32 of every slice's payload (compress) or regenerated bytes
// (decompress), computed on the device where they lie and read back with the results.
struct SliceCrcs {
  std::vector<uint32_t> crc;
  std::vector<int32_t> status;   // != 0: no value (the slice failed, or its span was refused)
  bool have(size_t k) const { return k < crc.size() && status[k] == 0; }
};
template <class HostBuf>
int run_plan(avr_ctx* c, int mode, bool sequential, Plan& plan, std::vector<avr_slice_result>* res,
             HostBuf* out_host, bool verify = false, uint32_t flags = 0, SliceCrcs* crcs = nullptr);

}  // namespace avr_host
