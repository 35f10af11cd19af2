// Plain records and constants shared by the host code and the kernels.  No HIP here: the host-only
// translation units (avr_host, avr_seams, avr_plan, avr_assemble) compile without ROCm.
#pragma once
#include <cstddef>
#include <cstdint>

namespace avr {

// macroblock columns of the upper row's model bytes in global scratch (avr_kernels.h, kEstMring):
// also the widest picture a seam record holds
constexpr int kMringCols = 288;

constexpr uint32_t kFlagBill = 1;   // launch flag: the coders bill per CodingType (avr_slice_result.bill)
// launch flags bits 16-31: EdgeRec slots of the LDS ring (max_mb_width of shared_bytes), set by
// launch_slices; an MBAFF slice needs 3 mb_width + 7 (Walker::pair_edge)
constexpr int kFlagRingShift = 16;
// launch flag: the batch may hold field pictures / MBAFF frames -- the parallel launches add a
// launch of the field-capable kernel for them, the sequential ones use it for every file
constexpr uint32_t kFlagFields = 2;
// launch flag: parallel model with the P32 container coder (avr_k_*32.hip) instead of the reference's
// arithmetic_code<uint64_t, uint8_t>
constexpr uint32_t kFlagP32 = 4;
// launch flag (set by launch_slices): the progressive parallel kernels keep the upper row's model
// bytes in global scratch instead of LDS, so that four workgroups of a wide picture fit a CU
constexpr uint32_t kFlagMringGlobal = 8;
// ------------------------------------------------------------------ the long-slice split
// The parallel model may cut a long progressive slice at macroblock-row starts into pieces re-coded
// with fresh models (the oracle's restatement in oracle/oracle_seams.c), so its
// decompress runs on one workgroup per piece.  One record per cut ("seam") in device memory:
struct SeamRec {
  uint32_t first_mb, last_dqp_nz;
  uint32_t cd_low, cd_range, cd_k, cd_next;   // compress: the CABAC decoder at the cut (CabacDecoder)
  uint32_t ce_low, ce_range, ce_outstanding, ce_cache;   // decompress: the re-encoder (CabacEncoder,
  int32_t ce_queue;                                     //   a cache byte always present)
  uint32_t q;                                 // the piece's first byte in the slice's CABAC bytes
  uint32_t pad[4];
  uint8_t state[1024];                        // CABAC context bytes
  // then the upper row's EdgeCore records (kEdgeBytes per macroblock column)
};
constexpr int kEdgeBytes = 40;
static_assert(sizeof(SeamRec) == 64 + 1024, "SeamRec layout");
inline size_t seam_rec_bytes(int max_mb_width) {
  return (sizeof(SeamRec) + (size_t)kEdgeBytes * max_mb_width + 15) & ~(size_t)15;
}
// per descriptor of a split launch
struct PieceCtl {
  int32_t seam;        // its start: record index in SplitArgs::recs, -1 = the slice's own start
  uint32_t n_mbs;      // macroblocks in the piece, 0 = to end_of_slice (the slice's last piece)
  int32_t snap;        // compress: the first record index for the cuts this slice may take (-1: none)
  uint32_t snap_cap;   // records from there
};

}  // namespace avr
