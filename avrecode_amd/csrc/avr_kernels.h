// Host-visible entry points of avr_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/avrecode.h"
#include "avr_records.h"

namespace avr {

struct EngineTables;

// Per model instance (u16 units): the dense SIG + NZ estimator table (kEstTable entries), then
// the write log that lets the next user clear only what was written (see avr_slice_lds.h): a u32
// count at kEstLogN (kEstLogOverflow: clear the whole table) and kEstLogCap u32 entry indices.
constexpr int kEstTable = 294016;
constexpr int kEstLogN = kEstTable;
constexpr int kEstLog = kEstTable + 2;
constexpr int kEstLogCap = 8191;
constexpr uint32_t kEstLogOverflow = 0xffffffffu;
// then, for the progressive parallel kernels of wide launches (kFlagMringGlobal), the upper row's
// model bytes (Walker::mring: 28 B per macroblock column -- 52 reserved -- up to kMringCols columns)
constexpr int kEstMring = kEstLog + 2 * kEstLogCap;
constexpr int kEstGlobal = kEstMring + kMringCols * 26;
static_assert(kEstGlobal % 8 == 0 && kEstTable % 8 == 0, "16-byte clears");

// LDS of one slice workgroup: the field / reference-model walkers' layout (full EdgeRecs), and the
// progressive parallel kernels' (EdgeCore ring, plus the model row in LDS unless mring_global)
size_t shared_bytes(int max_mb_width);
size_t shared_bytes_progressive(int max_mb_width, bool mring_global);
// the progressive parallel kernels of a launch of this width keep the model row in global memory:
// it fits one more workgroup per CU (and the row fits the scratch)
bool mring_global_for(int max_mb_width);
// does workgroup b of a 4G-workgroup launch land on CU group b mod G (schedule_kernel's assumption)?
hipError_t probe_round_robin(size_t lds, bool* ok);
// mode: 0 compress, 1 decompress, 2 generate, 3 trace (decode-only bin trace).  sequential = reference model (single wavefront).
// Sequential (reference-model) launches walk n_files files at once, one workgroup each: file f is
// the slices [file_first[f], file_first[f + 1]) (device array; nullptr = one file of all n slices)
// with est + f kEstGlobal, frames + f frame_stride and frame_meta[f] of its own.
struct SeqFiles {
  const int* file_first = nullptr;
  int n_files = 1;
  uint64_t frame_stride = 0;
};
// The field-capable kernel of a parallel launch beside the progressive one instead of after it (a
// batch holding both, e.g. a corpus with interlaced files): launch_parallel records `fork` on the
// launch's stream once the shared setup (queue, CU board) is queued, runs the field kernel on
// `stream` after it, and makes the launch's stream wait for `join` recorded there.  The persistent
// field kernel then takes the estimator scratches after the progressive kernel's (est_slots with
// fields).  Null stream: the field kernel follows the progressive one on the launch's stream.
struct FieldLane {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
// the arguments of a split launch (SeamRec, PieceCtl: avr_records.h)
struct SplitArgs {
  const PieceCtl* ctl = nullptr;
  uint8_t* recs = nullptr;      // rec_stride bytes per record
  uint32_t rec_stride = 0;
  uint32_t split_bits = 0;      // compress: a cut candidate every split_bits decoded bits
  uint32_t* snap_n = nullptr;   // compress: cuts made (records written) per descriptor
  uint32_t* piece_end = nullptr;   // compress: the re-coded stream's length at the end of each piece,
                                   //   one entry per record (from PieceCtl::snap)
};
// compress (mode 0: whole long slices, cut as they are walked) / decompress (1: the pieces) with the
// parallel model on arithmetic_code<uint64_t, uint8_t> (avr_k_split.hip) or, with kFlagP32 in flags,
// on the P32 coder (avr_k_split32.hip): one workgroup per descriptor, min(n, resident slots)
// workgroups; est holds that many estimator scratches
int split_grid(int n, int max_mb_width);
hipError_t launch_split(int mode, const EngineTables* T, const avr_slice_desc* descs, int n, int max_mb_width,
                        const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est, const SplitArgs& sp,
                        uint32_t flags, hipStream_t stream);
// the P32 kernels of launch_split, which has sized the launch (grid, lds) and set the flags
hipError_t launch_split32(int mode, const EngineTables* T, const avr_slice_desc* descs, int n, int grid, size_t lds,
                          const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est, const SplitArgs& sp,
                          uint32_t flags, hipStream_t stream);
// flags: kFlagBill (1) = the coders bill per CodingType into avr_slice_result.bill
hipError_t launch_slices(int mode, bool sequential, const EngineTables* T, const avr_slice_desc* descs, int n,
                         int max_mb_width, const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                         uint8_t* frames, int* frame_meta, int* order, hipStream_t stream,
                         const SeqFiles& files = SeqFiles(), uint32_t flags = 0, void* qscratch = nullptr,
                         const FieldLane* lane = nullptr);
// Parallel compress / decompress batches larger than the chip holds at once (more than
// resident_slices) run as one persistent launch over a largest-first queue when launch_slices gets
// a queue scratch of queue_scratch_bytes(n) (device); est then needs est_slots(n, max_mb_width)
// estimator scratches of kEstGlobal u16 (one per resident workgroup), else n; with a FieldLane,
// est_slots(n, max_mb_width, true) (the field kernel's workgroups too).
size_t queue_scratch_bytes(int n);
int slots_per_cu(size_t lds);
int resident_slices(size_t lds);
int est_slots(int n, int max_mb_width, bool field_lane = false);
int parallel_kernel_kind(int mode, int n, int max_mb_width);
// one per kernel translation unit (avr_k_*.hip); lds = shared_bytes(max_mb_width)
hipError_t launch_parallel_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                    const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                    const int* order, uint32_t flags, hipStream_t stream,
                                    uint32_t* qhead = nullptr, int qgrid = 0, int qgrid_fld = 0,
                                    size_t lds_fld = 0, const FieldLane* lane = nullptr);
// the persistent queue launches of launch_parallel_compress (qhead != nullptr), a unit of their own
// (avr_k_compress_queue.hip): built without the layout hints, which cost these kernels a VGPR spill
hipError_t launch_queue_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                 const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                 const int* order, uint32_t flags, hipStream_t stream, uint32_t* qhead, int qgrid,
                                 int qgrid_fld, size_t lds_fld, const FieldLane* lane);
hipError_t launch_parallel_decompress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                      const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                      const int* order, uint32_t flags, hipStream_t stream,
                                    uint32_t* qhead = nullptr, int qgrid = 0, int qgrid_fld = 0,
                                    size_t lds_fld = 0, const FieldLane* lane = nullptr);
hipError_t launch_parallel_compress32(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                      const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                      const int* order, uint32_t flags, hipStream_t stream,
                                    uint32_t* qhead = nullptr, int qgrid = 0, int qgrid_fld = 0,
                                    size_t lds_fld = 0, const FieldLane* lane = nullptr);
hipError_t launch_parallel_decompress32(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                        const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                        const int* order, uint32_t flags, hipStream_t stream,
                                    uint32_t* qhead = nullptr, int qgrid = 0, int qgrid_fld = 0,
                                    size_t lds_fld = 0, const FieldLane* lane = nullptr);
hipError_t launch_parallel_generate(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                    const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                    const int* order, uint32_t flags, hipStream_t stream);
hipError_t launch_parallel_trace(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                 const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                 const int* order, uint32_t flags, hipStream_t stream);
hipError_t launch_sequential_compress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                      const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                      uint8_t* frames, int* frame_meta, const int* file_first, int n_files,
                                      uint64_t frame_stride, uint32_t flags, hipStream_t stream);
hipError_t launch_sequential_decompress(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                        const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                        uint8_t* frames, int* frame_meta, const int* file_first, int n_files,
                                      uint64_t frame_stride, uint32_t flags, hipStream_t stream);
// reference-model compress in parallel (avr_k_rmode.hip): scan (count: ops == nullptr; write),
// estimator chains over the op stream, per-slice coder
hipError_t launch_rscan(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds, const uint8_t* in,
                        uint8_t* frames, const int64_t* goff, uint32_t* counts, uint32_t* ops,
                        const uint64_t* op_off, avr_slice_result* res, int32_t* stop_ok, bool fields, hipStream_t stream);
// Several files in one pass (a corpus): file f's ops are [file_op_off[f], file_op_off[f + 1]) (device,
// n_files + 1 entries; ignored for one file), each file with estimators of its own.
size_t rmode_sort_temp_bytes(uint64_t N, int n_files);
int rmode_max_files_per_pass();
hipError_t launch_rmode_estimators(const uint32_t* ops, uint64_t N, const uint64_t* file_op_off, int n_files,
                                   uint32_t* keys, uint64_t* vals, uint32_t* skeys, uint64_t* svals, void* temp,
                                   size_t temp_bytes, uint32_t* rops, hipStream_t stream);
hipError_t launch_rcode(const EngineTables* T, const avr_slice_desc* descs, int n, const uint32_t* rops,
                        const uint64_t* op_off, const uint32_t* counts, uint8_t* out, avr_slice_result* res,
                        const int32_t* stop_ok, uint32_t flags, hipStream_t stream);
// section cycle counters of AVR_PROFILE builds (avr_prof.h); zeros otherwise
hipError_t profile_parallel_compress(unsigned long long* out16);
hipError_t placement_parallel_compress(uint32_t* out8n, int n);
hipError_t placement_parallel_decompress(uint32_t* out8n, int n);
hipError_t profile_parallel_decompress(unsigned long long* out16);
hipError_t profile_parallel_generate(unsigned long long* out16);
hipError_t profile_parallel_trace(unsigned long long* out16);
hipError_t profile_sequential_compress(unsigned long long* out16);
hipError_t profile_sequential_decompress(unsigned long long* out16);
hipError_t launch_derive_decompress(const avr_slice_desc* descs, const avr_slice_result* rc, int n,
                                    avr_slice_desc* dd, hipStream_t stream);
hipError_t launch_verify(const avr_slice_desc* descs, const avr_slice_result* rc, const avr_slice_result* rd, int n,
                         const uint8_t* in, const uint8_t* regen, int32_t* verdict, hipStream_t stream);
hipError_t launch_pack(const avr_slice_desc* descs, const avr_slice_result* res, int n, const uint8_t* out,
                       uint8_t* packed, uint64_t* offsets, hipStream_t stream);
// avr_pack_pieces (avr_k_pieces.hip): launch_pack for units, each keeping what its avr_piece says
hipError_t launch_pack_pieces(const avr_slice_desc* descs, const avr_piece* pieces, const avr_slice_result* res, int n,
                              const uint8_t* out, uint8_t* packed, uint64_t* offsets, uint32_t* kept, int32_t* status,
                              hipStream_t stream);
// avr_stage_pieces (avr_k_pieces.hip): units' streams from anywhere in `out` (src[k], desc[k].payload_size
// bytes) into an arena of cap bytes, each 16-byte aligned and followed by >= 16 zero bytes; the scan
// writes offsets (n + 1), desc[k].payload_offset / read_limit and status (AVR_SLICE_OVERFLOW for a
// unit whose source or place lies outside its buffer: not copied)
hipError_t launch_stage_pieces(avr_slice_desc* descs, const uint64_t* src, int n, const uint8_t* out, uint64_t out_len,
                               uint8_t* arena, uint64_t cap, uint64_t* offsets, int32_t* status, hipStream_t stream);
// avr_verify_units (avr_k_pieces.hip): launch_verify for slices whose regenerated bytes are the packed
// kept bytes of their units [first[k], first[k + 1]) (launch_pack_pieces' outputs)
hipError_t launch_verify_units(const avr_slice_desc* descs, const avr_slice_result* rc, int n, const uint32_t* first,
                               int n_units, const uint8_t* in, const uint8_t* packed, const uint64_t* offsets, const uint32_t* kept,
                               const int32_t* ustatus, int32_t* verdict, hipStream_t stream);
// avr_crc_spans (avr_k_crc.hip): crc[k] = the CRC-32 (zlib's) of buf[off[k], off[k] + len[k]), one
// workgroup per span, any alignment; status[k] = 0, or AVR_SLICE_OVERFLOW (crc 0, nothing read) for a
// span that does not lie inside buf_len
hipError_t launch_crc_spans(const uint8_t* buf, uint64_t buf_len, const uint64_t* off, const uint32_t* len, int n,
                            uint32_t* crc, int32_t* status, hipStream_t stream);
// the same over a slice batch's own spans: its payloads (payload_offset, payload_size), or with regen
// what its decompress left (out_offset, res.out_len; a failed slice: its status, crc 0)
hipError_t launch_crc_slices(const avr_slice_desc* descs, const avr_slice_result* res, int n, bool regen,
                             const uint8_t* buf, uint64_t buf_len, uint32_t* crc, int32_t* status, hipStream_t stream);
// avr_gather_spans / avr_range_tails (avr_k_gather.hip): a window of a file laid out from copy spans
// over one source buffer (one workgroup per span, any alignment; status[k] = 0, or AVR_SLICE_OVERFLOW
// for a span outside src_len or dst_len: nothing of it read or written), then -- after it on the same
// stream -- one thread per selected unit checks its result against its tail record and applies the
// last-byte rule where the slice's final byte lies inside dst_len
hipError_t launch_gather_spans(const avr_span* spans, int n, const uint8_t* src, uint64_t src_len, uint8_t* dst,
                               uint64_t dst_len, int32_t* status, hipStream_t stream);
hipError_t launch_range_tails(const avr_range_tail* tails, const avr_slice_result* res, int n, uint8_t* dst,
                              uint64_t dst_len, int32_t* status, hipStream_t stream);
// avr_check_units (avr_k_check.hip): after the tails on the same stream, one workgroup per selected
// unit whose status is still 0 and whose check has a value: the CRC-32 of its share of the slice in
// src, the last-byte rule applied to the value, against checks[k].crc -- AVR_SLICE_CHECKSUM on a
// mismatch, AVR_SLICE_OVERFLOW (nothing read) for a span outside src_len
hipError_t launch_check_units(const avr_range_tail* tails, const avr_unit_check* checks, const avr_slice_result* res,
                              int n, const uint8_t* src, uint64_t src_len, int32_t* status, hipStream_t stream);

}  // namespace avr
