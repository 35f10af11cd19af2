/*
 * avrecode-amd: MI355X-native implementation of avrecode's CABAC decode -> predict ->
 * arithmetic re-encode path (ddkang/avrecode, reference mounted at /root/reference).
 *
 * C ABI: extern "C", plain pointers and sizes, integer status codes, no exceptions across the
 * boundary, caller-owned buffers unless stated, one avr_ctx per host thread (not thread-safe).
 *
 * Reference interfaces each group replaces (file:line in /root/reference):
 *   avr_compress_file    compressor(...).run()           recode.cpp:1102-1125, 1275-1297
 *   avr_decompress_file  decompressor(...).run()         recode.cpp:1312-1357, 1359-1409, 1527-1573
 *   avr_roundtrip_file   roundtrip(input, out)           recode.cpp:1594-1624
 *   avr_compress_files / avr_decompress_files  the two runs above over a corpus of files at once
 *   avr_roundtrip_files  roundtrip() over a corpus of files at once
 *   avr_compress_slices  compressor::cabac_decoder x N    recode.cpp:1134-1268 (+ h264_model 615-1059,
 *                        (one CABAC slice per wavefront)  h264_symbol::execute 1061-1100,
 *                                                         arithmetic_code.h encoder 89-203)
 *   avr_decompress_slices decompressor::cabac_decoder x N recode.cpp:1411-1520 (+ cabac_code.h 27-80,
 *                                                         arithmetic_code.h decoder 211-298)
 *   avr_hook_*           the libavcodec-hooks callback surface, AVCodecHooks    recode.cpp:137-228
 *                        (cabac.init_decoder/get/get_bypass/get_terminate/skip_bytes, model.frame_spec/
 *                        mb_xy/begin_sub_mb/end_sub_mb/begin_coding_type/end_coding_type)
 * The device kernels own the CABAC parse; the hooks layer serves the bins the device decoded to a
 * libavcodec-hooks caller, call by call, and checks the caller's parse against the device's.
 */
#ifndef AVRECODE_AMD_H
#define AVRECODE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVRECODE_ABI_VERSION 13 /* 13: unit checksums, opt-in (avr_set_unit_checksums, Block field 18, AVR_SLICE_CHECKSUM,
                                 *    avr_check_units, avr_unit_checks_apply, avr_dec_plan_unit_crcs, AVR_ASSEMBLE_UNIT_CRC,
                                 *    avr_reader_info_t.unit_checked);
                                 * 12: range reads (avr_reader_*, avr_dec_plan_file_size, avr_dec_plan_range(_apply),
                                 *    avr_gather_spans, avr_range_tails);
                                 * 11: checked containers, opt-in (avr_set_checksums, Metadata field 16, AVR_ERR_CHECKSUM,
                                 *    avr_crc_spans, avr_crc32(_combine), avr_assemble_container_args, avr_dec_plan_splice_crc);
                                 * 10: the long-slice split on the P32 coder, opt-in (avr_set_split_p32, the "P32S" / "P32SE"
                                 *    tags, avr_compress_split_slices_m, avr_decompress_pieces_m, AVR_ASSEMBLE_SPLIT32);
                                 * 9: escaped slices re-coded (avr_set_recode_escaped, Block field 17, the "E" tags,
                                 *    avr_assemble_container_opts, avr_escape_payload);
                                 * 8: split compress of slice batches (avr_split_plan, avr_compress_split_slices,
                                 *    avr_seams_build, avr_stage_pieces, avr_verify_units, avr_assemble_container_seams);
                                 * 7: piece plans (avr_dec_plan_load_pieces, avr_decompress_pieces, avr_pack_pieces);
                                 * 6: the parallel model's long-slice split (avr_set_split_bytes, Block field 16);
                                 * 5: avr_slice_desc.file_offset (96 B), dec-plan handle, ranged parse */

typedef enum {
  AVR_OK = 0,
  AVR_ERR_INVALID_ARGUMENT = -1,
  AVR_ERR_DEVICE = -2,          /* HIP error; see avr_last_error */
  AVR_ERR_FORMAT = -3,          /* malformed input file / container */
  AVR_ERR_OUT_OF_MEMORY = -4,
  AVR_ERR_ROUNDTRIP = -5,       /* decompress(compress(x)) != x */
  AVR_ERR_UNSUPPORTED = -6,
  AVR_ERR_CHECKSUM = -7,        /* the container decoded, and the file it gives is not the file it was made from */
} avr_status;

/* Model modes.  REFERENCE = recode.cpp's h264_model exactly (estimators persist across slices,
 * previous-frame and cross-slice contexts); output bytes equal the reference compressor's.
 * Sequential over slices (one wavefront for the whole file).
 * PARALLEL = the same model applied to every slice from a fresh state; slices are
 * independent, one wavefront per slice, shardable across GPUs.  Its decisions go through the
 * reference's own coder, arithmetic_code<uint64_t, uint8_t> with p1 = (range / (pos + neg)) * pos
 * (arithmetic_code.h:106-126, 232-248; recode.cpp:315-316, 816-820).  Tagged in
 * Recoded.Metadata.version as "avrecode-amd:P64".
 * PARALLEL32 = the parallel model with this library's optional 32-bit range coder (byte digits,
 * r1 = floor(range * floor(2^32 / tot) / 2^32) * pos; avr_engine.h PEncoder): fewer instructions per
 * decision, not the reference's arithmetic.  Tagged "avrecode-amd:P32".  Containers of every mode
 * decompress with avr_decompress_file, which reads the tag. */
/* AVR_MODEL_CHAINED: the reference model in chains -- a fresh model (estimators and frame metadata,
 * as at the start of a file) before every AVR_CHAIN_SLICES-th coded slice of a file, tagged
 * "avrecode-amd:R16".  It compresses like the reference model (the estimators learn across a chain's
 * 16 slices: realshort.mp4 0.998, cockatoo.mp4 0.994 of the input, against 0.990 / 0.991 for the
 * reference model and 1.041 / 1.010 for the parallel one), and a file's chains decode on as many
 * workgroups at once.  Whole-file calls only (avr_compress_file(s), avr_decompress_file(s),
 * avr_roundtrip_file(s), the hooks sessions -- the streaming one makes its container at
 * avr_hooks_end from the complete file, as for the reference model -- and the per-rank chain
 * ranges of one file, avr_compress_chain_range / avr_decompress_chain_range); the device
 * slice-batch calls refuse it with AVR_ERR_INVALID_ARGUMENT. */
typedef enum { AVR_MODEL_REFERENCE = 0, AVR_MODEL_PARALLEL = 1, AVR_MODEL_PARALLEL32 = 2, AVR_MODEL_CHAINED = 3 } avr_model;
#define AVR_CHAIN_SLICES 16

typedef struct avr_ctx avr_ctx;

/* device = HIP device ordinal.  Fails with AVR_ERR_DEVICE when no usable GPU is present: the
 * library has no CPU implementation of the hot path. */
int avr_create(int device, avr_ctx** out);
void avr_destroy(avr_ctx* ctx);
const char* avr_last_error(const avr_ctx* ctx);
/* free a buffer returned by the library */
void avr_free(void* p);

/* The parallel model's long-slice split (this library's own format; not in the reference, which
 * decodes a slice as one chain, recode.cpp:1411-1520).  The whole-file compress of AVR_MODEL_PARALLEL
 * cuts a progressive-frame slice at macroblock-row starts into pieces -- a cut candidate every
 * 8 * split_bytes decoded CABAC bits with half a piece still ahead -- each re-coded with a fresh
 * model, so the slice decompresses one workgroup per piece.  Block.cabac holds the pieces' streams
 * one after the other; Block field 16 ("seams", zlib) what each piece's decompress needs from before
 * it (its first macroblock and output byte, the CABAC re-encoder's state, the context states, the
 * upper row's neighbour fields).  Such containers decompress through the whole-file calls
 * (avr_decompress_file(s), avr_roundtrip_file(s)) and the hooks sessions (which regenerate one
 * whole at begin, as a reference-model container) and, piece by piece on any number of ranks,
 * through the piece plans (avr_dec_plan_load_pieces, avr_decompress_pieces, avr_pack_pieces); the
 * per-slice plans (avr_plan_decompress, avr_dec_plan_load) refuse them with AVR_ERR_UNSUPPORTED.
 * A caller that holds slice batches on the device makes them with avr_split_plan,
 * avr_compress_split_slices, avr_seams_build and avr_assemble_container_seams (ABI 8, below).
 * split_bytes = 0: no split.  Default: the environment's AVR_SPLIT_BYTES, else 98304.  Checked by the oracle's
 * restatement (oracle/oracle_seams.c).
 * AVR_MODEL_PARALLEL32 takes the same split only with avr_set_split_p32 on (below): by default its
 * whole-file compress ignores split_bytes and writes the containers it always wrote. */
int avr_set_split_bytes(avr_ctx* ctx, size_t split_bytes);
size_t avr_get_split_bytes(const avr_ctx* ctx);
/* The long-slice split for AVR_MODEL_PARALLEL32, an option, off by default.  With it on,
 * avr_compress_file(s) and avr_roundtrip_file(s) of AVR_MODEL_PARALLEL32 read split_bytes exactly as
 * AVR_MODEL_PARALLEL does: the same candidate slices, the same cuts (a cut is placed from the CABAC
 * decoder's state and the payload alone, so it does not depend on the coder the pieces are re-coded
 * with), every cut checked by the host's restatement; the pieces are P32 streams.  A container with at
 * least one Block field 16 is tagged "avrecode-amd:P32S", with a field 17 as well "avrecode-amd:P32SE"
 * (a reader from before ABI 10 refuses the tag instead of decoding Block.cabac as one stream); one
 * without field 16 keeps "avrecode-amd:P32" / "P32E" and its bytes, option on or off.  Reading needs
 * no option: every decompress call that takes a split AVR_MODEL_PARALLEL container takes these
 * (whole files, avr_dec_plan_load_pieces, the hooks decompress session for "P32S"); field 16 under
 * "avrecode-amd:P32" / "P32E" stays AVR_ERR_FORMAT, and an S tag without any field 16 is accepted.
 * Default: the environment's AVR_SPLIT_P32 (non-zero: on), else 0. */
int avr_set_split_p32(avr_ctx* ctx, int on);
int avr_get_split_p32(const avr_ctx* ctx);

/* Slices whose NAL unit carries emulation-prevention bytes (00 00 03, H.264 7.4.1) re-coded: an
 * option of the parallel models, off by default.  The segmentation looks for a slice's unescaped
 * payload verbatim in the file, as the reference does (recode.cpp:1275-1297); such a slice's payload
 * stands nowhere, so it is stored skip_coded although the device has re-coded and verified it.  With
 * the option on, a candidate slice of status 0 that the search misses is searched once more as
 * E = escape(payload) (avr_escape_payload), inside its own NAL and after the previous coded block;
 * a hit makes it a coded block that stands for E's size + k file bytes and carries Block field 17
 * ("escapes", varint k >= 1); size, length_parity and last_byte keep their meaning on the unescaped
 * payload, and so do the q values of a field 16 on the same block.  A container with at least one
 * field 17 is tagged "avrecode-amd:P64E" / "avrecode-amd:P32E" (same models; a reader from before
 * ABI 9 refuses the tag instead of skipping the field and writing a wrong file); one without keeps
 * the plain tag and the plain bytes.  The decompress regenerates the slice, applies the last-byte
 * patch, escapes, and checks that exactly k bytes were inserted (AVR_ERR_FORMAT otherwise; also for
 * field 17 on a block without cabac, under a tag without E, k = 0 or k > size / 2 + 1).  Every
 * decompress call takes such containers (whole files, avr_plan_decompress, the dec plans, piece
 * plans) except the hooks decompress session: AVR_ERR_UNSUPPORTED there.  Read by
 * avr_compress_file(s) and avr_roundtrip_file(s) for AVR_MODEL_PARALLEL / AVR_MODEL_PARALLEL32; the
 * reference and chained models ignore it (their bytes are pinned), and hooks compress sessions
 * never write the field.  Default: the environment's AVR_RECODE_ESCAPED (non-zero: on), else 0. */
int avr_set_recode_escaped(avr_ctx* ctx, int on);
int avr_get_recode_escaped(const avr_ctx* ctx);
/* 7.4.1 from a clean state: a 03 inserted before any byte <= 3 that follows two zero bytes since
 * the last insertion, nothing appended after the last byte.  *len = the escaped length (at most
 * n + n / 2); written to dst when it fits cap, else AVR_ERR_INVALID_ARGUMENT with *len still set
 * (dst may be NULL with cap 0 to ask for the length).  Host only. */
int avr_escape_payload(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* len);

/* Checked containers: the file's CRC-32 in the container, an option, off by default (with it off every
 * container is byte for byte what it was).  recode.proto has no check of what a container restores,
 * and the splice keeps the reference's rule -- the regenerated length is never compared with `size` --
 * so a damaged Block.cabac can decompress with status 0 to a wrong file.  With the option on,
 * avr_compress_file(s) and avr_roundtrip_file(s) of every model write Recoded.Metadata field 16, wire
 * type 5 (fixed32; bytes 85 01 + the value, little-endian) after `version`: the CRC-32 of the
 * original file exactly as zlib.crc32 gives it (ISO-HDLC: reflected polynomial 0xEDB88320, init and
 * xorout 0xFFFFFFFF).  6 bytes per container; a reference-model container, which has no Metadata
 * otherwise, gets one holding only this field (8 bytes).  No tag changes: the field is additive, and a
 * reader from before it (the reference's included) skips it and decodes the file.  Hooks compress
 * sessions never write it.
 * Reading needs no option: every call that writes a file from a container that has the field checks
 * it (avr_decompress_file(s), avr_splice_container, avr_dec_plan_splice(_crc), avr_hooks_end of a
 * decompress session) and returns AVR_ERR_CHECKSUM on a mismatch -- the whole-file calls without an
 * output, a call that writes into the caller's buffer before it has written anything.  A second
 * field 16 in the Metadata, or one of another wire type, is AVR_ERR_FORMAT.
 * The value is a fold, never a pass over the file: a CRC is linear, so the file's is the combine
 * (avr_crc32_combine), in block order, of each block's file bytes -- a literal's by a host CRC, a coded
 * block's from the CRC of its slice's bytes, which avr_crc_spans computes on the device where the
 * slice lies (the payload arena at compress, the regenerated buffer at decompress), with the
 * last-byte rule (recode.cpp:1345-1356) applied to the value.  Default: the environment's
 * AVR_CHECKSUMS (non-zero: on), else 0. */
int avr_set_checksums(avr_ctx* ctx, int on);
int avr_get_checksums(const avr_ctx* ctx);
/* zlib's crc32 and crc32_combine: avr_crc32 continues `crc` (0 to start) over p[0, n);
 * avr_crc32_combine(crc(A), crc(B), |B|) = crc(AB), in O(log |B|) multiply-mods.  Host only. */
uint32_t avr_crc32(uint32_t crc, const uint8_t* p, size_t n);
uint32_t avr_crc32_combine(uint32_t a, uint32_t b, uint64_t len_b);
/* The CRC-32 of n spans of one device buffer, one workgroup per span on `stream` (NULL = default):
 * d_crc[k] = crc32(d_buf[d_off[k] .. + d_len[k])), any alignment, overlaps allowed; d_status[k] = 0, or
 * AVR_SLICE_OVERFLOW with d_crc[k] = 0 for a span that does not lie inside buf_len (checked on the
 * device; nothing of it is read).  All pointers are device pointers; nothing is synchronised;
 * n <= 0 launches nothing. */
int avr_crc_spans(avr_ctx* ctx, const uint8_t* d_buf, size_t buf_len, const uint64_t* d_off, const uint32_t* d_len,
                  int n, uint32_t* d_crc, int32_t* d_status, void* stream);

/* Unit checksums: a CRC-32 per unit in the container, an option of the parallel models, off by default
 * (with it off every container is byte for byte what it was).  A unit is what one workgroup
 * regenerates: a whole coded slice, or one piece of a cut slice.  The file CRC above guards whole-file
 * calls only -- a range read (avr_reader_*) regenerates a few units and cannot fold a file's value --
 * and a flipped bit in Block.cabac can regenerate a slice of the right length with wrong bytes, which
 * neither the unit statuses nor the reader's length check see.  With the option on,
 * avr_compress_file(s) and avr_roundtrip_file(s) of AVR_MODEL_PARALLEL / AVR_MODEL_PARALLEL32 write
 * Block field 18 ("unit_crcs", wire type 2) on every coded block: 4 m bytes, one little-endian CRC-32
 * (zlib's) per unit in unit order, m = 1 for an uncut block, the number of pieces for one with field
 * 16.  Unit i covers slice bytes [q[i-1], q[i]) (q[-1] = 0, the last unit to `size`: the range
 * planner's coordinates) of the slice's payload, in the unescaped domain (also on a block with field
 * 17), as the file holds them after the last-byte rule; the values combined in order
 * (avr_crc32_combine with the unit lengths) are the payload's CRC.  7 bytes per uncut block,
 * 4 m + 3 for a cut one (m <= 31; 4 m + 4 beyond).  No tag changes: the field is additive and a reader
 * from before it (the reference's included) skips it.  The reference and chained models ignore the
 * option (their bytes are pinned), and hooks compress sessions never write the field.
 * The values come from the device, where the payloads lie: an uncut slice's from the per-slice payload
 * CRC pass of the checked containers, a cut slice's from one avr_crc_spans launch over the payload
 * arena once the cuts are known; a value the device refused is computed on the host.
 * Reading needs no option.  AVR_ERR_FORMAT for the field on a block without cabac, a second one,
 * another wire type, or a length that is not 4 x the block's unit count.  The field may stand on some
 * coded blocks and not on others: a block without it is unchecked.  Every path that regenerates a
 * unit checks it: a range read the units it touched (avr_check_units: AVR_ERR_CHECKSUM names the
 * unit, reads that avoid it still succeed), every whole-file path (avr_decompress_file(s),
 * avr_splice_container, avr_dec_plan_splice(_crc)) each block -- its values combined against the
 * patched CRC of the slice's regenerated bytes, from device values where the caller has them, with or
 * without Metadata field 16 (both present: both checked) -- AVR_ERR_CHECKSUM naming the block.
 * Not covered: hooks sessions ignore the field (either direction); a sharded decompress checks only
 * through rank 0's splice; the reference and chained models; a non-random-access reader checks through
 * its whole-file call.  Default: the environment's AVR_UNIT_CHECKSUMS (non-zero: on), else 0. */
int avr_set_unit_checksums(avr_ctx* ctx, int on);
int avr_get_unit_checksums(const avr_ctx* ctx);

/* ------------------------------------------------------------------ whole files (host memory) */
/* in: an MP4 (avcC) or Annex-B H.264 file.  *out: serialized Recoded protobuf (recode.proto). */
int avr_compress_file(avr_ctx* ctx, const uint8_t* in, size_t n, int model, uint8_t** out, size_t* out_len);
/* in: a Recoded protobuf.  *out: the original file bytes. */
int avr_decompress_file(avr_ctx* ctx, const uint8_t* in, size_t n, uint8_t** out, size_t* out_len);

/* Several files at once (a corpus): compressor::run / decompressor::run (recode.cpp:1102-1357) for
 * each of in[0 .. n_files), with the device work of all files batched.  A file is the reference
 * model's unit of sequential work (its estimators persist across ITS slices, recode.cpp:662-665, and
 * nothing crosses files), so reference-model files run side by side: the compress side in one
 * parallel pass over every slice of every file with per-file estimators, the decompress side one
 * workgroup (wavefront) per file; parallel-model slices of all files run one wavefront each.
 * out[f] / out_len[f]: file f's result (malloc'd, avr_free; NULL on failure).  status (optional,
 * n_files entries) receives each file's status and the call returns AVR_OK unless the batch as a
 * whole failed; without it the call returns the first file failure -- and out[f] is still set for
 * every file that succeeded, so the caller frees every non-NULL out[f] whatever the call returns.
 * avr_last_error holds one message: the last failing file's.  Output bytes equal
 * avr_compress_file / avr_decompress_file on each file alone. */
int avr_compress_files(avr_ctx* ctx, int n_files, const uint8_t* const* in, const size_t* in_len, int model,
                       uint8_t** out, size_t* out_len, int32_t* status);
int avr_decompress_files(avr_ctx* ctx, int n_files, const uint8_t* const* in, const size_t* in_len, uint8_t** out,
                         size_t* out_len, int32_t* status);

/* Where the wall time of a whole-file call goes (seconds).  Host phases by wall clock, device
 * phases by HIP events on the context's stream (summed over the call's device passes):
 *   demux_s      compress: demux, NAL unescape, parameter-set / slice-header parse, plan building;
 *                decompress: container parse, surrogate stream, header parse, plan building
 *   upload_s     host -> device copies of payloads / re-coded streams and descriptors
 *   kernel_s     the device passes (slice kernels, schedule, R-mode scan / sort / coder, verify)
 *   download_s   device -> host copies of results and outputs
 *   container_s  compress: segmentation + Recoded protobuf (and the reference model's re-plans);
 *                decompress: splicing literals + regenerated slices, last-byte patch
 *   other_s      the rest of the call's wall time (allocation, launch and synchronisation
 *                overhead) */
typedef struct {
  double demux_s, upload_s, kernel_s, download_s, container_s, other_s;
} avr_phase_times;

typedef struct {
  uint64_t file_bytes, slices, coded_slices, skipped_slices, payload_bytes, recoded_bytes, bins;
  double compress_s, decompress_s;  /* wall time of the two halves (host + device), summed over attempts */
  /* h264_model::bill / cabac_bill (recode.cpp:615-661), indexed by avr_pip_coding_type: bytes the
   * re-coded encoder emitted per put during compress (recode.cpp:1074-1078, 1213-1220) and bytes
   * the CABAC encoder emitted per put during decompress (1443-1446, 1455-1457, 1466-1468), summed
   * over the file's coded slices (the parallel model's per-slice models included). */
  uint64_t bill[6], cabac_bill[6];
  /* compress + decompress passes the roundtrip took: 1, or 2 when the parallel model's unverified
   * first pass did not come back and the file was compressed again with the per-slice check */
  uint32_t attempts, reserved;
  avr_phase_times compress_phases, decompress_phases;   /* summed over attempts */
} avr_file_stats;
/* The phase breakdown of the last whole-file call on ctx (avr_compress_file(s),
 * avr_decompress_file(s), avr_roundtrip_file: its last decompress). */
int avr_last_phase_times(const avr_ctx* ctx, avr_phase_times* out);
/* compress, decompress, compare (recode.cpp:1594-1624).  Returns AVR_ERR_ROUNDTRIP on mismatch. */
int avr_roundtrip_file(avr_ctx* ctx, const uint8_t* in, size_t n, int model, uint8_t** compressed,
                       size_t* compressed_len, avr_file_stats* stats);
/* avr_roundtrip_file (roundtrip(), recode.cpp:1594-1624) over a corpus, with the device work of
 * all files batched as in avr_compress_files / avr_decompress_files: every file compressed (the parallel model without its
 * per-slice device check), every container decompressed and compared with its input; the files
 * that do not come back are compressed again with the check, decompressed and compared again.
 * out[f] / out_len[f]: file f's container (malloc'd, avr_free; NULL when it failed), status[f]: its
 * result (AVR_ERR_ROUNDTRIP when even the checked container does not restore it).  times (optional,
 * 2 entries): wall seconds of the compress and the decompress calls, summed over attempts.  Returns
 * AVR_OK unless the batch as a whole failed. */
int avr_roundtrip_files(avr_ctx* ctx, int n_files, const uint8_t* const* in, const size_t* in_len, int model,
                        uint8_t** out, size_t* out_len, int32_t* status, double* times);

/* ------------------------------------------------------- slice batches (device-resident data) */
/* One CABAC slice: the (buf, size) FFmpeg hands to AVCodecHooks.cabac.init_decoder
 * (recode.cpp:143), plus the slice-header fields the slice_data() parse needs. */
typedef struct {
  uint64_t payload_offset;   /* byte offset of the CABAC payload in the input buffer */
  uint32_t payload_size;     /* init_decoder's size */
  uint32_t read_limit;       /* bytes readable from payload_offset (>= payload_size) */
  uint64_t out_offset;       /* where this slice's output goes in the output buffer */
  uint32_t out_capacity;     /* bytes reserved there */
  int32_t slice_type;        /* 0 P, 1 B, 2 I */
  int32_t slice_qp, cabac_init_idc, first_mb, mb_width, mb_height;
  int32_t num_ref_idx_l0, num_ref_idx_l1;
  int32_t chroma_array_type, transform_8x8_mode, direct_8x8_inference, x264_build;
  int32_t picture_id;        /* decode-order picture counter (frame_spec, recode.cpp:824-843) */
  int32_t coded;             /* 0: skip_coded slice (reference mode only calls frame_spec) */
  int32_t structure;         /* AVR_STRUCT_*: frame, top / bottom field picture (PAFF), MBAFF frame;
                              * mb_height is the FRAME height in macroblocks in every case */
  uint64_t file_offset;      /* host only (avr_parse_stream): where the payload's bytes stand verbatim in
                              * the parsed file (its NAL has no emulation-prevention bytes), else
                              * UINT64_MAX; the container assembly's segmentation starts there
                              * (recode.cpp:1275-1297).  The kernels ignore it. */
} avr_slice_desc;
enum { AVR_STRUCT_FRAME = 0, AVR_STRUCT_TOP_FIELD = 1, AVR_STRUCT_BOTTOM_FIELD = 2, AVR_STRUCT_MBAFF = 3 };

/* avr_slice_result.status: 0, or why the slice cannot be coded (the container stores it skip_coded) */
enum {
  AVR_SLICE_OK = 0,
  AVR_SLICE_PCM = -2,             /* I_PCM macroblock (skip_bytes; the reference throws, recode.cpp:161-163) */
  AVR_SLICE_BAD_REF_IDX = -3,     /* ref_idx unary prefix past 32 */
  AVR_SLICE_BAD_MVD = -4,         /* mvd suffix exponent past 24 */
  AVR_SLICE_BAD_LEVEL = -5,       /* coeff_abs_level_minus1 suffix exponent past 30 */
  AVR_SLICE_BAD_QP_DELTA = -6,    /* mb_qp_delta past 102 */
  AVR_SLICE_BAD_MB_ADDR = -7,     /* macroblock address past the picture */
  AVR_SLICE_OVERREAD = -8,        /* the parse ran past the payload */
  AVR_SLICE_NO_END = -9,          /* the walk ended without end_of_slice_flag = 1 */
  AVR_SLICE_CODER = -10,          /* coder invariant violated (carry into an emitted byte: corrupt input) */
  AVR_SLICE_NO_STOP = -11,        /* compress: a CABAC re-encode would not restore the payload (last-byte rule) */
  AVR_SLICE_OVERFLOW = -12,       /* output past out_capacity */
  AVR_SLICE_MBAFF_RING = -20,     /* MBAFF slice launched with max_mb_width < 3 * mb_width + 7 */
  AVR_SLICE_NO_ROUNDTRIP = -21,   /* file calls: the device roundtrip check did not regenerate the payload */
  AVR_SLICE_CHECKSUM = -22        /* avr_check_units: the unit's regenerated bytes are not the ones its CRC was made from */
};

typedef struct {
  uint32_t out_len;          /* bytes written at out_offset */
  int32_t status;            /* AVR_SLICE_*: 0 ok, < 0 the slice must be stored skip_coded */
  uint32_t bins;             /* CABAC bins processed */
  uint32_t mbs;              /* macroblocks parsed */
  /* h264_model billing of this slice by avr_pip_coding_type (recode.cpp:615-661), filled only
   * by the whole-file calls (zero from the batch entry points): compress = re-coded bytes emitted
   * per put (h264_model::bill), decompress = CABAC bytes emitted per put (cabac_bill). */
  uint32_t bill[6];
} avr_slice_result;

/* All pointers are device pointers; stream is a hipStream_t (NULL = default stream).
 * Compress: payload bytes -> re-coded bytes.  For each slice the kernel also checks that a
 * CABAC re-encode plus the decompressor's last-byte rule (recode.cpp:1345-1356, 1503-1505)
 * restores the payload, and reports status < 0 otherwise. */
/* max_mb_width / max_mb_height bound every slice's picture size (LDS ring and frame sizing).
 * max_mb_width is the LDS ring's width in macroblock records: mb_width, or 3 * mb_width + 7 for an
 * AVR_STRUCT_MBAFF slice (its pair records live there too) -- the value avr_parse_stream reports.
 * An MBAFF slice launched with less fails alone (status < 0). */
int avr_compress_slices(avr_ctx* ctx, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                        const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, int model, void* stream);
/* Decompress: re-coded bytes (at payload_offset/payload_size = recoded stream) -> regenerated
 * CABAC bytes at out_offset (before the last-byte patch; trailing 0x80 already dropped). */
int avr_decompress_slices(avr_ctx* ctx, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                          const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, int model, void* stream);
/* Pack variable-length per-slice outputs contiguously: d_packed[k] gets slice k's bytes at
 * d_offsets[k] (exclusive prefix sum of out_len, computed on the device). */
int avr_pack_outputs(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_slice_result* d_res, int n,
                     const uint8_t* d_out, uint8_t* d_packed, uint64_t* d_offsets, void* stream);

/* Device-resident roundtrip of a slice batch: recode.cpp:1594-1624 applied per slice, without the
 * container.  Compress d_in -> d_work (at each desc's out_offset), derive the decompress
 * descriptors on the device (d_dec_desc, n entries of scratch), decompress d_work -> d_regen
 * (slice k at d_desc[k].payload_offset, i.e. d_regen has d_in's layout), then apply the last-byte
 * rule (recode.cpp:1345-1356) and compare with the payload.  d_verdict[k]: 1 bit-exact,
 * 0 mismatch, 2 not coded (compress status != 0: the container stores it skip_coded).
 * Everything is enqueued on `stream`; nothing is synchronised. */
int avr_roundtrip_slices(avr_ctx* ctx, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                         const uint8_t* d_in, uint8_t* d_work, uint8_t* d_regen, avr_slice_desc* d_dec_desc,
                         avr_slice_result* d_res_c, avr_slice_result* d_res_d, int32_t* d_verdict, int model,
                         void* stream);

/* The two device steps avr_roundtrip_slices runs between its compress and decompress launches,
 * for callers that time or overlap the halves themselves (same semantics as above). */
int avr_derive_decompress_descs(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c, int n,
                                avr_slice_desc* d_dec_desc, void* stream);
int avr_verify_slices(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c,
                      const avr_slice_result* d_res_d, int n, const uint8_t* d_in, const uint8_t* d_regen,
                      int32_t* d_verdict, void* stream);

/* The chained model (AVR_MODEL_CHAINED) across GPUs, within one file.  Its chains are independent
 * (a fresh reference model before every AVR_CHAIN_SLICES-th coded slice), so a file's chains are cut
 * into `world` contiguous ranges balanced by payload bytes (the rule of the Python shard.partition)
 * and rank `rank` runs its range on this context's GPU:
 *   avr_compress_chain_range: the file parsed and segmented as avr_compress_file does it, then the
 *     reference-model pass over this rank's chains (compressor::run, recode.cpp:1102-1132, with the
 *     model restarted per chain, 662-665).  Outputs for the file's slices [*lo, *hi): status 0 =
 *     coded (its re-coded bytes at recoded + offsets[k], lens[k]), -1 = not coded, -2 = a coded
 *     slice the pass failed (avr_compress_file would demote it and re-segment, which moves every
 *     later chain: compress the file whole instead).  The ranks' outputs, concatenated in rank order,
 *     are avr_assemble_container's status / recoded / offsets / lens for model AVR_MODEL_CHAINED:
 *     byte-identical to avr_compress_file(file, AVR_MODEL_CHAINED).
 *   avr_decompress_chain_range: the container planned as avr_decompress_file plans it (every slice,
 *     coded or not), this rank's chains regenerated (decompressor::cabac_decoder, recode.cpp:
 *     1411-1520, one chain per workgroup).  Outputs for the plan's slices [*lo, *hi): status 0 =
 *     regenerated (bytes at regen + offsets[k], lens[k]), 1 = not coded, < 0 failed.  Concatenated in
 *     rank order they are avr_dec_plan_splice's inputs on a plan of the same container.  A
 *     reference-model container is one unit (rank 0 takes it whole).
 * Buffers are allocated here (avr_free).  No reference counterpart: the reference is one CPU thread. */
int avr_compress_chain_range(avr_ctx* ctx, const uint8_t* file, size_t n, int world, int rank, int* lo, int* hi,
                             int32_t** status, uint8_t** recoded, size_t* recoded_len, uint64_t** offsets,
                             uint32_t** lens);
int avr_decompress_chain_range(avr_ctx* ctx, const uint8_t* avrc, size_t n, int world, int rank, int* lo, int* hi,
                               int32_t** status, uint8_t** regen, size_t* regen_len, uint64_t** offsets,
                               uint32_t** lens);

/* Which device kernel a parallel-model batch of n slices (widest picture max_mb_width macroblocks)
 * runs on this context's GPU, by the rule avr_compress_slices / avr_decompress_slices apply:
 * *kind = 0 the resident kernel (slices_parallel_kernel: one workgroup per slice, the whole batch
 * resident at once), 1 the persistent queue kernel (slices_queue_kernel: more slices than the chip
 * holds at once, or pictures wide enough that their model row lives in global scratch).  For
 * naming the measured kernel in profiles; no reference counterpart (the reference is one CPU
 * thread). */
int avr_slice_kernel(avr_ctx* ctx, int decompress, int n, int max_mb_width, int* kind);

/* ------------------------------------------------------------ host-side slice extraction */
/* What FFmpeg hands AVCodecHooks.cabac.init_decoder for every CABAC slice of a file
 * (av_decoder::decode_video, recode.cpp:73-135): demux (MP4/avcC or Annex-B), unescape, parse
 * SPS/PPS/SEI/slice headers.  Host only, no device needed.  Returns malloc'd arrays (free with
 * avr_free): *descs (n entries; payload_offset/read_limit index *arena, out_offset/out_capacity
 * index a work buffer of *work_len bytes sized for compress output) and *arena (payloads, each
 * 16-byte aligned, followed by >= 16 zero bytes).  desc.coded = 0 for slices the recoder does not
 * take (unsupported syntax, or shorter than a surrogate marker, recode.cpp:1285). */
int avr_parse_stream(const uint8_t* file, size_t n, avr_slice_desc** descs, int* n_slices, uint8_t** arena,
                     size_t* arena_len, size_t* work_len, int* max_mb_width, int* max_mb_height);
/* avr_parse_stream for the slices [lo, hi) only (hi < 0: to the end), descs and arena rebased to
 * them: a rank of a sharded compress takes its own range of a stream without copying the rest
 * (the whole stream's headers are still parsed: slice indices and picture ids are the file's). */
int avr_parse_stream_range(const uint8_t* file, size_t n, int lo, int hi, avr_slice_desc** descs, int* n_slices,
                           uint8_t** arena, size_t* arena_len, size_t* work_len, int* max_mb_width,
                           int* max_mb_height);
/* The payload_size of every CABAC slice of a file (what avr_parse_stream reports), without copying a
 * payload: the input of a sharded run's partition on every rank.  *sizes malloc'd (avr_free). */
int avr_slice_payload_sizes(const uint8_t* file, size_t n, uint32_t** sizes, int* n_slices);

/* Rank 0 of a sharded PARALLEL-model compress: build the Recoded container from per-slice outputs
 * gathered from every rank (compressor::run + find_next_coded_block_and_emit_literal,
 * recode.cpp:1115-1132, 1275-1297).  Host only.  model = the model the outputs were made with (the
 * container's tag): AVR_MODEL_PARALLEL / _PARALLEL32 (avr_compress_slices on each rank's slice
 * range), or AVR_MODEL_CHAINED (avr_compress_chain_range on each rank's chains).  Slice k (avr_parse_stream order) is
 * coded when it is a candidate and status[k] == 0; its re-coded bytes are recoded[offsets[k] ..
 * + lens[k]), inside recoded_len (AVR_ERR_INVALID_ARGUMENT otherwise).  The result is
 * byte-identical to avr_compress_file(..., model).  avr_assemble_container parses `file` again;
 * avr_assemble_container_parsed takes avr_parse_stream's descs and arena for it instead (the parse
 * a sharded caller already holds: no second pass over a multi-GB stream).  Only that call's output,
 * unmodified, for this file is accepted: a coded desc must be a recodable candidate and a verbatim
 * payload must stand at its file_offset (checked on its first and last bytes; otherwise
 * AVR_ERR_INVALID_ARGUMENT).  The segmentation searches only each slice's literal gap when the parse
 * found its payload verbatim, and the container is written once, its bytes copied by host threads. */
int avr_assemble_container(const uint8_t* file, size_t n, int model, int n_slices, const int32_t* status,
                           const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets, const uint32_t* lens,
                           uint8_t** out, size_t* out_len);
int avr_assemble_container_parsed(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                  const uint8_t* arena, size_t arena_len, const int32_t* status,
                                  const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                  const uint32_t* lens, uint8_t** out, size_t* out_len);
/* avr_assemble_container_parsed into the caller's buffer out (out_cap bytes): a step that assembles
 * every time reuses one buffer, already mapped, instead of a fresh multi-GB allocation.  *out_len =
 * the container's size; when it exceeds out_cap nothing is written and AVR_ERR_INVALID_ARGUMENT is
 * returned with *out_len set.  A bound: n + sum(lens of coded slices) + 64 (n_slices + 2). */
int avr_assemble_container_into(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                const uint8_t* arena, size_t arena_len, const int32_t* status, const uint8_t* recoded,
                                size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, uint8_t* out,
                                size_t out_cap, size_t* out_len);
/* The model mode a Recoded container was written with (its Metadata.version): AVR_MODEL_*.
 * AVR_ERR_FORMAT for bytes that are not a Recoded message or name another avrecode-amd format. */
int avr_container_model(const uint8_t* avrc, size_t n, int* model);

/* Sharded PARALLEL-model decompress (decompressor::run, recode.cpp:1312-1357, split over ranks).
 * avr_plan_decompress: the container's coded slices as a decompress batch, host only -- *descs
 * (n entries, in container order; payload_offset / read_limit / payload_size index *arena = the
 * re-coded streams, out_offset / out_capacity index a work buffer of *work_len bytes for the
 * regenerated CABAC bytes) for avr_decompress_slices on any rank's slice range.  Returns
 * AVR_ERR_UNSUPPORTED for a reference-model container (its slices chain: replicas only).
 * avr_splice_container (rank 0): the original file from the container's literals and slice k's
 * regenerated bytes regen[offsets[k] .. + lens[k]) (avr_decompress_slices output before the
 * last-byte patch, which this applies, recode.cpp:1345-1356); status[k] != 0 fails the file with
 * AVR_ERR_FORMAT; a slice whose bytes lie outside regen_len or exceed its descriptor's out_capacity
 * gives AVR_ERR_INVALID_ARGUMENT.  Byte-identical to avr_decompress_file.  A sharded caller
 * decompresses the batch with the container's model (avr_container_model). */
int avr_plan_decompress(const uint8_t* avrc, size_t n, avr_slice_desc** descs, int* n_slices, uint8_t** arena,
                        size_t* arena_len, size_t* work_len, int* max_mb_width, int* max_mb_height);
int avr_splice_container(const uint8_t* avrc, size_t n, int n_slices, const int32_t* status, const uint8_t* regen,
                         size_t regen_len, const uint64_t* offsets, const uint32_t* lens, uint8_t** out,
                         size_t* out_len);

/* The sharded decompress's host halves on one parse (decompressor::run, recode.cpp:1338-1409):
 * a plan handle loads a container -- read_packet's surrogate stream parsed and
 * matched to the coded blocks, as avr_plan_decompress, but without copying any bytes yet -- then
 * writes the descriptors and the re-coded streams' arena where the caller wants them (the arena
 * with host threads), and splices the regenerated slices with the literals and the last-byte patch
 * (recode.cpp:1345-1356) into the caller's buffer, as avr_splice_container.  The container must stay
 * alive and unchanged from avr_dec_plan_load to the last call on it; a handle keeps its scratch
 * (the surrogate stream's buffer) for the next load.  arena_len / work_len / max_mb_* as
 * avr_plan_decompress.  avr_dec_plan_splice: *out_len = the file's size; AVR_ERR_INVALID_ARGUMENT
 * when out_cap is smaller (nothing written) or a slice's bytes lie outside regen or past its
 * capacity, AVR_ERR_FORMAT when a coded block has no slice or a slice's status is not 0.  A
 * parallel-model plan lists the coded slices (one device batch); a reference- or chained-model plan
 * lists every slice, coded or not (the reference model turns frames over on uncoded ones), which is
 * the indexing avr_decompress_chain_range's outputs use. */
typedef struct avr_dec_plan avr_dec_plan;
int avr_dec_plan_new(avr_dec_plan** out);
void avr_dec_plan_free(avr_dec_plan* plan);
int avr_dec_plan_load(avr_dec_plan* plan, const uint8_t* avrc, size_t n, int* n_slices, size_t* arena_len,
                      size_t* work_len, int* max_mb_width, int* max_mb_height);
int avr_dec_plan_descs(const avr_dec_plan* plan, avr_slice_desc* out);
int avr_dec_plan_arena(const avr_dec_plan* plan, uint8_t* out, size_t cap);
int avr_dec_plan_splice(const avr_dec_plan* plan, const int32_t* status, const uint8_t* regen, size_t regen_len,
                        const uint64_t* offsets, const uint32_t* lens, uint8_t* out, size_t out_cap, size_t* out_len);
/* avr_dec_plan_splice with, for a checked container, crcs[k] = the CRC-32 of slice k's lens[k]
 * regenerated bytes as a device computed it (avr_crc_spans over the regenerated buffer, or over a cut
 * slice's units, combined): the splice then reads no slice's bytes for the check.  crcs NULL, and
 * every other splice entry point, computes them from regen on host threads.  The values are read only
 * when the container has the field; wrong ones fail the file (AVR_ERR_CHECKSUM). */
int avr_dec_plan_splice_crc(const avr_dec_plan* plan, const int32_t* status, const uint8_t* regen, size_t regen_len,
                            const uint64_t* offsets, const uint32_t* lens, const uint32_t* crcs, uint8_t* out,
                            size_t out_cap, size_t* out_len);

/* Piece plans: the sharded decompress of a container whose long slices were cut (avr_set_split_bytes).
 * The unit of work is what one workgroup regenerates: a whole coded slice, or one piece of a split
 * slice.  No reference counterpart (the reference decodes a slice as one chain, recode.cpp:1411-1520).
 * avr_dec_plan_load_pieces loads a parallel-model container, with or without seams, into a plan
 * handle (AVR_ERR_UNSUPPORTED for a reference- or chained-model container; every check the
 * whole-file decompress makes on a seams field, with AVR_ERR_FORMAT).  *n_slices = the coded slices,
 * the indexing of avr_dec_plan_descs and avr_dec_plan_splice, a split slice counting once; *n_units
 * = the units, in container order, a split slice's pieces consecutive; *n_recs seam records of
 * *rec_stride bytes (the device layout of the split kernels, for pictures up to 288 macroblocks wide).
 * avr_dec_plan_units: the units' descriptors -- payload_offset / payload_size index the arena
 * avr_dec_plan_arena writes (*arena_len bytes; each unit's stream 16-byte aligned and followed by at
 * least 16 zero bytes), out_offset / out_capacity a work buffer of *work_len bytes (a piece's capacity
 * = its kept bytes + 4096) -- and what each unit is of its slice.  avr_dec_plan_recs: the records.
 * On a container without seams the units are avr_dec_plan_load's slices, descriptor for descriptor.
 * avr_dec_plan_splice takes one (status, offset, len) per coded slice as ever: for a split slice
 * they describe the concatenation of its pieces' kept bytes. */
typedef struct {
  int32_t seam;    /* record index among the plan's seam records where this unit starts; -1: the slice's own start */
  uint32_t n_mbs;  /* macroblocks in the unit; 0: to end_of_slice (a last piece, or a whole slice) */
  int32_t slice;   /* which of the plan's coded slices (avr_dec_plan_splice's index) the unit belongs to */
  uint32_t keep;   /* bytes of the unit's regenerated output that are the slice's: the next cut's first
                    * byte - this one's; UINT32_MAX: all of them (a last piece, or a whole slice) */
} avr_piece;
int avr_dec_plan_load_pieces(avr_dec_plan* plan, const uint8_t* avrc, size_t n, int* n_slices, int* n_units,
                             size_t* arena_len, size_t* work_len, int* max_mb_width, int* max_mb_height,
                             int* n_recs, size_t* rec_stride);
int avr_dec_plan_units(const avr_dec_plan* plan, avr_slice_desc* descs, avr_piece* pieces);
int avr_dec_plan_recs(const avr_dec_plan* plan, uint8_t* out, size_t cap);

/* A batch of units that are pieces or whole progressive-frame slices of AVR_MODEL_PARALLEL (the u64
 * coder), regenerated one workgroup per unit by the split kernel (the one avr_decompress_file runs)
 * on `stream`: d_desc / d_in / d_out / d_res as avr_decompress_slices, pieces = the units' HOST array
 * (seam indexes d_recs: n_recs records of rec_stride bytes in device memory; slice and keep are not
 * read).  The array is checked on the host before anything is launched: -1 <= seam < n_recs,
 * max_mb_width <= 288 and rec_stride no less than a record of max_mb_width columns, otherwise
 * AVR_ERR_INVALID_ARGUMENT.  Field, MBAFF and wider slices are never cut: they go through
 * avr_decompress_slices.  Nothing is synchronised. */
int avr_decompress_pieces(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_piece* pieces, int n,
                          int max_mb_width, int max_mb_height, const uint8_t* d_recs, int n_recs, size_t rec_stride,
                          const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, void* stream);
/* The same for units of either parallel model: model = AVR_MODEL_PARALLEL (avr_decompress_pieces
 * exactly) or AVR_MODEL_PARALLEL32 (the units of an "avrecode-amd:P32S" container, on the P32 split
 * kernel); any other model: AVR_ERR_INVALID_ARGUMENT.  One call runs one coder. */
int avr_decompress_pieces_m(avr_ctx* ctx, int model, const avr_slice_desc* d_desc, const avr_piece* pieces, int n,
                            int max_mb_width, int max_mb_height, const uint8_t* d_recs, int n_recs, size_t rec_stride,
                            const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res, void* stream);
/* avr_pack_outputs for units: unit k's kept bytes -- all out_len of them when d_pieces[k].keep is
 * UINT32_MAX, else the first keep -- packed at d_packed + d_offsets[k] (d_offsets: n + 1 entries, the
 * exclusive prefix sum of d_kept).  d_status[k] = the unit's status, or AVR_SLICE_NO_END when it
 * regenerated fewer than keep bytes; a unit with d_status != 0 keeps nothing.  Packed this way the
 * consecutive units of a slice are the slice's regenerated bytes without gaps, on one rank and after
 * a rank-order concatenation.  All pointers are device pointers (d_pieces: a device copy of the
 * avr_piece array). */
int avr_pack_pieces(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_piece* d_pieces,
                    const avr_slice_result* d_res, int n, const uint8_t* d_out, uint8_t* d_packed,
                    uint64_t* d_offsets, uint32_t* d_kept, int32_t* d_status, void* stream);

/* Split compress of slice batches (ABI 8): what avr_compress_file does with the parallel model's long
 * slices, for a caller that holds a rank's slices on the device -- so a sharded compress writes the
 * container the whole-file call writes.  No reference counterpart (the reference codes a slice as
 * one chain, recode.cpp:1134-1268).
 *
 * avr_split_plan (host only): which of n descriptors the whole-file compress would take through the
 * split walk at split_bytes -- a progressive frame (AVR_STRUCT_FRAME), mb_width <= 288,
 * 2 * payload_size >= 3 * split_bytes, 0 < split_bytes < 2^28 (desc.coded is not read: the caller
 * plans its recodable slices) -- and what that walk needs.  slots[k] = {first, cap}: the candidate's
 * cut records are [first, first + cap) of the batch's *n_recs, cap = 8 * payload_size /
 * (8 * split_bytes) + 1 (a walk makes fewer cuts than cap); {-1, 0} for the others.
 * out_capacity[k] (optional) = 2 * payload_size + 256 + 64 * cap for a candidate, else 0.
 * *rec_stride = the record size of the widest candidate (of one column without any),
 * *n_candidates (optional) their number. */
typedef struct {
  int32_t first;   /* first cut record of the slice's slot; -1: not a candidate, no cut is made */
  uint32_t cap;    /* records in the slot */
} avr_split_slot;
int avr_split_plan(const avr_slice_desc* descs, int n, size_t split_bytes, avr_split_slot* slots,
                   uint32_t* out_capacity, int* n_recs, size_t* rec_stride, int* n_candidates);
/* The split walk on `stream` over the caller's device buffers (d_desc / d_in / d_out / d_res as
 * avr_compress_slices; every slice a progressive frame of AVR_MODEL_PARALLEL, out_capacity as
 * avr_split_plan gives it): each slice is cut as it is walked -- a cut candidate every
 * 8 * split_bytes decoded bits.  slots = avr_split_plan's HOST array.  Slice k's pieces' streams stand
 * one after the other at its out_offset (d_res[k].out_len bytes in all); d_cuts[k] = its cuts,
 * d_piece_end[slots[k].first + i] = where piece i ends in them, d_recs (n_recs records of rec_stride
 * bytes, the split kernels' device layout) record slots[k].first + i = cut i.  d_cuts (n) and
 * d_piece_end (n_recs) are zeroed on the stream first.  Checked on the host before anything is
 * launched (AVR_ERR_INVALID_ARGUMENT): max_mb_width <= 288, rec_stride no less than a record of
 * max_mb_width columns, 0 < split_bytes < 2^28, every slot {-1, 0} or inside n_recs with cap >= 1.
 * Scratch is the context's split scratch (avr_decompress_pieces' too): the call may run beside an
 * avr_compress_slices launch on another stream, not beside another split launch.  Nothing is
 * synchronised. */
int avr_compress_split_slices(avr_ctx* ctx, const avr_slice_desc* d_desc, int n, int max_mb_width, int max_mb_height,
                              const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res,
                              const avr_split_slot* slots, size_t split_bytes, uint8_t* d_recs, int n_recs,
                              size_t rec_stride, uint32_t* d_cuts, uint32_t* d_piece_end, void* stream);
/* The same walk re-coding with either parallel model's coder: model = AVR_MODEL_PARALLEL
 * (avr_compress_split_slices exactly) or AVR_MODEL_PARALLEL32; any other: AVR_ERR_INVALID_ARGUMENT.
 * The cuts, records and counts are the same for both; the streams and piece ends are the coder's. */
int avr_compress_split_slices_m(avr_ctx* ctx, int model, const avr_slice_desc* d_desc, int n, int max_mb_width,
                                int max_mb_height, const uint8_t* d_in, uint8_t* d_out, avr_slice_result* d_res,
                                const avr_split_slot* slots, size_t split_bytes, uint8_t* d_recs, int n_recs,
                                size_t rec_stride, uint32_t* d_cuts, uint32_t* d_piece_end, void* stream);
/* Host only: the Block-field-16 bytes of every cut slice of such a batch, from what the caller read
 * back -- descs / arena (the host descriptors and payloads, avr_parse_stream's), res, cuts,
 * piece_end (n_recs entries) and recs (n_recs * rec_stride bytes, at least recs_len).  status[k] =
 * res[k].status, or with check_cuts AVR_SLICE_CODER when a cut's re-encoder state is not what the
 * host restates from the record's CABAC decoder state and the payload (what avr_compress_file
 * checks; without it the records' re-encoder fields are taken as they are).  A slice with status 0
 * and at least one cut gets its field at *seams + offsets[k], lens[k] bytes (lens[k] = 0 otherwise);
 * *seams is malloc'd (avr_free).  AVR_ERR_INVALID_ARGUMENT, with nothing read out of range, when a
 * slot is not {-1, 0} or inside n_recs, cuts[k] >= cap (or non-zero without a slot), a status-0
 * slice's piece ends decrease or its last is not out_len, rec_stride is less than a record of the
 * slice's mb_width (1 .. 288), its slice_type or (P / B) cabac_init_idc is not 0 .. 2, a payload lies
 * outside arena_len, or recs_len < n_recs * rec_stride. */
int avr_seams_build(const avr_slice_desc* descs, int n, const uint8_t* arena, size_t arena_len,
                    const avr_slice_result* res, const avr_split_slot* slots, const uint32_t* cuts,
                    const uint32_t* piece_end, int n_recs, const uint8_t* recs, size_t recs_len, size_t rec_stride,
                    int check_cuts, int32_t* status, uint8_t** seams, size_t* seams_len, uint64_t* offsets,
                    uint32_t* lens);
/* avr_assemble_container(_parsed) with one optional seams field per slice: slice k's Block field 16
 * is seams[seam_offsets[k] .. + seam_lens[k]) (length 0: none; seams NULL: none at all), so rank 0
 * of a sharded compress writes avr_compress_file's container.  AVR_ERR_INVALID_ARGUMENT when a field
 * lies outside seams_len, when one is given with a model other than AVR_MODEL_PARALLEL, or for a
 * slice that is not coded (not a candidate, or status[k] != 0). */
int avr_assemble_container_seams(const uint8_t* file, size_t n, int model, int n_slices, const int32_t* status,
                                 const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                 const uint32_t* lens, const uint8_t* seams, size_t seams_len,
                                 const uint64_t* seam_offsets, const uint32_t* seam_lens, uint8_t** out,
                                 size_t* out_len);
int avr_assemble_container_seams_parsed(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs,
                                        int n_slices, const uint8_t* arena, size_t arena_len, const int32_t* status,
                                        const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                        const uint32_t* lens, const uint8_t* seams, size_t seams_len,
                                        const uint64_t* seam_offsets, const uint32_t* seam_lens, uint8_t** out,
                                        size_t* out_len);
/* Every avr_assemble_container* above in one call, with a flags word.  descs / arena NULL: the file is
 * parsed here (avr_assemble_container); else avr_parse_stream's (avr_assemble_container_parsed).
 * seams as in avr_assemble_container_seams (NULL: none).  flags = 0: those calls exactly.
 * AVR_ASSEMBLE_ESCAPED: the second search of avr_set_recode_escaped, so rank 0 of a sharded
 * compress writes what avr_compress_file writes with the option on; with descs it parses the file
 * once more when some coded slice's payload does not stand verbatim (a descriptor does not carry
 * its NAL's place).  AVR_ERR_INVALID_ARGUMENT for the flag with a model that is not one of the two
 * parallel ones, and for unknown flag bits.
 * AVR_ASSEMBLE_SPLIT32: seams fields are allowed for AVR_MODEL_PARALLEL32 (without the flag every
 * assemble call refuses them), and a container that holds one is tagged "avrecode-amd:P32S" /
 * "P32SE": what avr_compress_file writes with avr_set_split_p32 on.  AVR_ERR_INVALID_ARGUMENT for the
 * flag with any other model.
 * AVR_ASSEMBLE_CRC: a checked container (avr_set_checksums), for every assemblable model: the file's
 * CRC-32 is folded from the literals and the coded slices' payload CRCs, which the assembly computes
 * on host threads -- or takes from avr_assemble_container_args' crcs.
 * AVR_ASSEMBLE_UNIT_CRC: unit checksums (avr_set_unit_checksums), the parallel models only
 * (AVR_ERR_INVALID_ARGUMENT otherwise): Block field 18 on every coded block, the values computed here on
 * host threads from the payloads and the seams' q.  (Bit 8 is not a flag.) */
enum { AVR_ASSEMBLE_ESCAPED = 1, AVR_ASSEMBLE_SPLIT32 = 2, AVR_ASSEMBLE_CRC = 4, AVR_ASSEMBLE_UNIT_CRC = 16 };
int avr_assemble_container_opts(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                const uint8_t* arena, size_t arena_len, const int32_t* status, const uint8_t* recoded,
                                size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, const uint8_t* seams,
                                size_t seams_len, const uint64_t* seam_offsets, const uint32_t* seam_lens,
                                uint32_t flags, uint8_t** out, size_t* out_len);
/* avr_assemble_container_opts with its parameters in a struct (size = sizeof(avr_assemble_args), first)
 * and one more: crcs[k] = the CRC-32 of slice k's payload (avr_parse_stream order; read for coded
 * slices only, and only with AVR_ASSEMBLE_CRC), as the ranks' devices computed them over their payload
 * arenas (avr_crc_spans).  NULL: computed here.  Values a caller brings are trusted -- rank 0 cannot
 * check them without doing the work again -- so wrong ones give a container that every checking
 * reader refuses.  AVR_ERR_INVALID_ARGUMENT for a size that is not this struct's. */
typedef struct {
  size_t size;
  const uint8_t* file;
  size_t n;
  int model;
  const avr_slice_desc* descs;
  int n_slices;
  const uint8_t* arena;
  size_t arena_len;
  const int32_t* status;
  const uint8_t* recoded;
  size_t recoded_len;
  const uint64_t* offsets;
  const uint32_t* lens;
  const uint8_t* seams;
  size_t seams_len;
  const uint64_t* seam_offsets;
  const uint32_t* seam_lens;
  uint32_t flags;
  const uint32_t* crcs;
} avr_assemble_args;
int avr_assemble_container_args(const avr_assemble_args* args, uint8_t** out, size_t* out_len);
/* The two device steps that let a rank check its split slices without their bytes leaving the device
 * (all pointers device pointers, nothing synchronised).
 * avr_stage_pieces: the units' streams -- unit k's d_desc[k].payload_size bytes at d_out + d_src[k],
 * at any alignment (a split walk leaves a slice's pieces one after the other) -- copied into d_arena
 * in unit order, each 16-byte aligned and followed by at least 16 zero bytes: avr_decompress_pieces'
 * input layout.  Unit k stands at d_offsets[k] (n + 1 entries; d_offsets[k + 1] - d_offsets[k] =
 * its length + 16 rounded up to 16), and d_desc[k].payload_offset / read_limit are set to it.
 * d_status[k] = 0, or AVR_SLICE_OVERFLOW for a unit whose source reaches past out_len or whose place
 * past arena_cap (checked on the device; it is not copied).  d_arena must be 16-byte aligned.
 * avr_verify_units: avr_verify_slices for split slices after avr_pack_pieces.  Slice k's units are
 * [d_first[k], d_first[k + 1]) (n + 1 entries) of the packed batch's n_units (d_packed, d_offsets, d_kept,
 * d_unit_status: avr_pack_pieces' outputs); their kept bytes, contiguous there, are compared with
 * the payload at d_in + d_desc[k].payload_offset under the last-byte rule (recode.cpp:1345-1356:
 * payload_size or payload_size - 1 bytes, the final byte not compared).  d_verdict[k] = 1 bit-exact,
 * 0 mismatch -- also when a unit failed, the slice has no unit or the lengths do not add up --
 * 2 not coded (desc.coded = 0 or d_res_c[k].status != 0). */
int avr_stage_pieces(avr_ctx* ctx, avr_slice_desc* d_desc, const uint64_t* d_src, int n, const uint8_t* d_out,
                     size_t out_len, uint8_t* d_arena, size_t arena_cap, uint64_t* d_offsets, int32_t* d_status,
                     void* stream);
int avr_verify_units(avr_ctx* ctx, const avr_slice_desc* d_desc, const avr_slice_result* d_res_c, int n,
                     const uint32_t* d_first, int n_units, const uint8_t* d_in, const uint8_t* d_packed, const uint64_t* d_offsets,
                     const uint32_t* d_kept, const int32_t* d_unit_status, int32_t* d_verdict, void* stream);

/* ------------------------------------------------------------------ range reads (ABI 12)
 * An opened container serves byte ranges of its file.  In the parallel models' containers every coded
 * slice -- and every piece of a cut slice -- is independent, so a window of the file needs only the
 * units whose bytes it touches.  No reference counterpart (decompressor::run regenerates the whole
 * file, recode.cpp:1312-1357).
 *
 * File coordinates come from the container alone: a literal block stands for its length, a coded block
 * for `size` bytes, a skip_coded block for none; the prefix sum over the blocks places every block and
 * gives the file's size.  Inside a cut block piece i covers slice bytes [q[i-1], q[i]) (q[-1] = 0, the
 * last piece to `size`).
 *
 * avr_dec_plan_file_size: the size of the file a loaded plan (either load) restores.
 * avr_dec_plan_range (a piece plan, avr_dec_plan_load_pieces; host only): the window [off, off + len)
 * clamped to the file, as
 *   - info: the clamped window, the units [unit_lo, unit_hi) whose bytes it touches (units of blocks
 *     that only border it are not selected; an empty window selects none), the counts;
 *   - *spans (n_spans; malloc'd, avr_free): the copies that lay the window out, in window order and
 *     without gap or overlap.  source = AVR_SPAN_LITERAL: src_off indexes the container's bytes;
 *     source = k >= 0: src_off indexes the regenerated bytes of unit unit_lo + k.  No span is longer
 *     than span_cap bytes (0: the library's 16384; otherwise 16 .. 2^30), so one long slice spreads
 *     over many workgroups of avr_gather_spans;
 *   - *tails (unit_hi - unit_lo; malloc'd): what must hold of each selected unit's result, and for the
 *     unit that ends a slice the last-byte rule (recode.cpp:1345-1356).  A piece that is not its
 *     slice's last (keep != UINT32_MAX) must have regenerated at least keep bytes.  A last piece or a
 *     whole slice must make the slice's regenerated total T = q_last + out_len restore exactly `size`
 *     bytes: with the rule (has_rule) T = size when T's parity is length_parity (the final byte is
 *     replaced by last_byte) or T = size - 1 when it differs (last_byte is appended); without it
 *     T = size.  final_pos = where the slice's final byte stands in the window, AVR_RANGE_NO_POS when
 *     it lies outside.  The unit holding a slice's final byte is always its last unit, also when that
 *     byte is the appended one: the rule is decided by the regenerated length, so that unit is
 *     decoded (its span then copies one byte of slack from the unit's output space, which the tail
 *     overwrites).
 * This length check is stricter than the whole-file splice, which keeps the reference's rule and never
 * compares a regenerated length with `size`: a range read's coordinates are the container's sizes, so
 * a touched slice whose length contradicts its block fails the read (AVR_SLICE_NO_END in its status,
 * AVR_ERR_FORMAT from the call).
 * AVR_ERR_UNSUPPORTED for a container with escaped blocks (Block field 17: such a block's file bytes
 * are not a crop of its regenerated bytes), AVR_ERR_FORMAT for a touched coded block without a unit
 * or cuts that do not ascend inside `size`, AVR_ERR_INVALID_ARGUMENT for a plan that is not a piece
 * plan, off + len overflowing or span_cap out of range.  Every index and length emitted is checked.
 * avr_dec_plan_range_apply (host only): the spans and tails applied to host buffers -- what
 * avr_gather_spans and avr_range_tails do on the device.  Unit unit_lo + k's regenerated bytes stand
 * at regen + unit_off[k], its result in res[k]; avrc = the container (literal spans).  status[k]
 * (n_units) = the unit's own status when non-zero, AVR_SLICE_NO_END for a short piece or a slice of
 * the wrong length, else 0.  AVR_OK when every status is 0, else AVR_ERR_FORMAT;
 * AVR_ERR_INVALID_ARGUMENT, before anything is written, when a span or a final_pos does not lie
 * inside its buffers.  Nothing is written outside out[0, out_len). */
enum { AVR_SPAN_LITERAL = -1 };
#define AVR_RANGE_NO_POS UINT64_MAX
typedef struct {
  uint64_t src_off;   /* in the container's bytes (literal) or the source unit's regenerated bytes;
                       * avr_gather_spans: in d_src */
  uint64_t dst_off;   /* in the window */
  uint32_t len;
  int32_t source;     /* AVR_SPAN_LITERAL, or the unit's index among the selected ones (avr_gather_spans ignores it) */
} avr_span;
typedef struct {
  uint32_t keep;            /* a piece that is not its slice's last: the bytes it must have regenerated; else UINT32_MAX */
  uint32_t q_last;          /* a last piece / whole slice: the slice's bytes before this unit */
  uint32_t size;            /* the block's size */
  uint8_t has_rule, length_parity, last_byte, reserved;
  uint64_t final_pos;       /* window position of the slice's final byte; AVR_RANGE_NO_POS */
} avr_range_tail;
typedef struct {
  uint64_t off, len;        /* the window, clamped to the file */
  uint64_t file_size, literal_bytes;
  int32_t unit_lo, unit_hi, n_spans, reserved;
} avr_range_info;
int avr_dec_plan_file_size(const avr_dec_plan* plan, uint64_t* size);
int avr_dec_plan_range(const avr_dec_plan* plan, uint64_t off, uint64_t len, uint32_t span_cap, avr_range_info* info,
                       avr_span** spans, avr_range_tail** tails);
int avr_dec_plan_range_apply(const avr_span* spans, int n_spans, const avr_range_tail* tails, int n_units,
                             const uint8_t* avrc, size_t avrc_len, const uint8_t* regen, size_t regen_len,
                             const uint64_t* unit_off, const avr_slice_result* res, uint8_t* out, size_t out_len,
                             int32_t* status);
/* The two device steps (all pointers device pointers, `stream` a hipStream_t, nothing synchronised;
 * n <= 0 launches nothing).
 * avr_gather_spans: one workgroup per span copies d_spans[k].len bytes from d_src + src_off to
 * d_dst + dst_off, any alignment on either side.  d_status[k] = 0, or AVR_SLICE_OVERFLOW for a span
 * that does not lie inside src_len or dst_len (checked on the device; nothing of it is read or
 * written).  Spans of one launch must not overlap in the destination (the kernel's memory safety does
 * not rely on it).
 * avr_range_tails: after the gather on the same stream, one thread per selected unit reads d_res[k],
 * applies d_tails[k] (above) and writes d_status[k]; for the unit that ends a slice, when the rule
 * replaces or appends and final_pos is inside dst_len, it stores last_byte at d_dst + final_pos
 * (AVR_SLICE_OVERFLOW for a final_pos outside). */
int avr_gather_spans(avr_ctx* ctx, const avr_span* d_spans, int n, const uint8_t* d_src, size_t src_len, uint8_t* d_dst,
                     size_t dst_len, int32_t* d_status, void* stream);
int avr_range_tails(avr_ctx* ctx, const avr_range_tail* d_tails, const avr_slice_result* d_res, int n, uint8_t* d_dst,
                    size_t dst_len, int32_t* d_status, void* stream);
/* The unit check of a range read (ABI 13, avr_set_unit_checksums): after avr_range_tails on the same
 * stream, one workgroup of 256 threads per selected unit k.  Nothing happens when d_status[k] != 0,
 * d_res[k].status != 0 or d_checks[k].have == 0 (the status stays).  Otherwise the CRC-32 of the unit's
 * share of its slice -- d_tails[k].keep bytes of a piece that is not its slice's last (even when it
 * regenerated more), d_res[k].out_len bytes of a last piece or whole slice, at d_src + src_off -- with
 * the last-byte rule applied to the value, decided as avr_range_tails decides it from
 * T = q_last + out_len (replace: the raw byte table's entry for the difference of the two last bytes;
 * append: last_byte through the register, out_len = 0 included; else nothing), is compared with
 * d_checks[k].crc: d_status[k] = AVR_SLICE_CHECKSUM on a mismatch, AVR_SLICE_OVERFLOW for a span that
 * does not lie inside src_len (nothing of it is read).  All pointers are device pointers; nothing is
 * synchronised; n <= 0 launches nothing.
 * avr_dec_plan_unit_crcs (host only, a piece plan): crc / have of the units [unit_lo, unit_hi) from
 * their blocks' field 18 (have = 0 for a unit of a block without it); src_off is the caller's.
 * avr_unit_checks_apply (host only): avr_check_units on host buffers.  AVR_ERR_CHECKSUM when it set an
 * AVR_SLICE_CHECKSUM, else AVR_ERR_FORMAT when it set an AVR_SLICE_OVERFLOW, else AVR_OK. */
typedef struct {
  uint64_t src_off;   /* where the unit's regenerated bytes start in d_src */
  uint32_t crc;       /* the unit's value of Block field 18 */
  uint32_t have;      /* 0: the unit's block carries no field; nothing is checked */
} avr_unit_check;
int avr_check_units(avr_ctx* ctx, const avr_range_tail* d_tails, const avr_unit_check* d_checks,
                    const avr_slice_result* d_res, int n, const uint8_t* d_src, size_t src_len, int32_t* d_status,
                    void* stream);
int avr_dec_plan_unit_crcs(const avr_dec_plan* plan, int unit_lo, int unit_hi, avr_unit_check* out);
int avr_unit_checks_apply(const avr_range_tail* tails, const avr_unit_check* checks, const avr_slice_result* res, int n,
                          const uint8_t* src, size_t src_len, int32_t* status);

/* The reader: pread on an opened container.  avrc must stay valid and unchanged until avr_reader_close;
 * one reader belongs to one context (and its host thread); it owns its device buffers, reuses them
 * across reads and shares none with the whole-file calls, so other calls on the context may come
 * between two reads.  Both reads synchronise before they return.
 * Random-access containers (info.random_access = 1): "avrecode-amd:P64" with or without seams,
 * "P32" and "P32S".  open loads the piece plan once and uploads the seam records once; nothing
 * proportional to the file is reserved.  A read plans its window (avr_dec_plan_range), writes the
 * selected units' streams -- re-placed compactly, 16-byte aligned, >= 16 zero bytes after each -- and
 * the window's literal bytes into one pinned staging buffer, uploads it, regenerates the units on the
 * context's stream (pieces through avr_decompress_pieces_m's path, whole slices -- field and MBAFF
 * ones included -- through avr_decompress_slices', one launch after the other), gathers the window
 * (avr_gather_spans), runs the tails (avr_range_tails) and -- when a selected unit's block carries
 * unit checksums (Block field 18) -- the unit checks (avr_check_units), downloads the statuses and only
 * then the bytes.  A selected unit with a non-zero status fails the read with AVR_ERR_FORMAT, one whose
 * bytes miss its checksum (AVR_SLICE_CHECKSUM) with AVR_ERR_CHECKSUM (avr_last_error on the context
 * names the unit); `out` is then untouched (d_out: unspecified).  A read that touches no block with the
 * field launches nothing more and its avr_read_stats are what they were.
 * Everything else (info.random_access = 0: reference and chained models, every "E" tag -- an escaped
 * block's bytes are not a crop of its regenerated bytes): the first read regenerates the whole file
 * once through avr_decompress_file (so a checked container is checked: AVR_ERR_CHECKSUM), the reader
 * keeps it in host memory and serves every read from there.
 * Checked containers: a partial read cannot verify a file CRC.  info.checked says that field 16 is
 * present; random-access reads are guarded by the per-unit statuses and the strict length check
 * (above), not by field 16 -- and by the unit checksums where the container has them:
 * info.unit_checked = 1 when every coded block carries Block field 18.
 * pread semantics: the window is clamped to the file; *got = 0 with AVR_OK at or past the end and for
 * len = 0 (nothing is launched); off + len overflowing is AVR_ERR_INVALID_ARGUMENT.
 * avr_reader_span: [*lo, *hi) = the file bytes of the block holding off, *coded = 1 for a coded block
 * (a caller that chunks on these boundaries never regenerates a boundary slice twice);
 * AVR_ERR_INVALID_ARGUMENT at or past the end.
 * avr_reader_last: what the last successful read did. */
typedef struct avr_reader avr_reader;
typedef struct {
  uint64_t file_size;
  int32_t model;           /* AVR_MODEL_* */
  int32_t random_access;
  int32_t n_blocks, n_units;   /* n_units: 0 without random access */
  int32_t checked, unit_checked;
} avr_reader_info_t;
typedef struct {
  uint64_t units, pieces;      /* units regenerated; those among them that are pieces of cut slices */
  uint64_t regenerated_bytes, literal_bytes, spans;
  avr_phase_times phases;      /* of the read: demux_s = planning and staging */
} avr_read_stats;
int avr_reader_open(avr_ctx* ctx, const uint8_t* avrc, size_t n, avr_reader** out);
int avr_reader_info(const avr_reader* r, avr_reader_info_t* info);
int avr_reader_read(avr_reader* r, uint64_t off, size_t len, uint8_t* out, size_t* got);
int avr_reader_read_device(avr_reader* r, uint64_t off, size_t len, uint8_t* d_out, size_t* got);
int avr_reader_span(const avr_reader* r, uint64_t off, uint64_t* lo, uint64_t* hi, int* coded);
int avr_reader_last(const avr_reader* r, avr_read_stats* out);
void avr_reader_close(avr_reader* r);

/* Container codec check (host only): parse a Recoded protobuf (recode.proto:1-19) with the
 * library's own wire codec -- the one avr_decompress_file uses -- and return (a) its fields as JSON,
 * {"version": null | hex, "blocks": [{"size": int, "literal": hex, "skip_coded": bool, "cabac": hex,
 * "length_parity": bool, "last_byte": hex, "seams": hex, "escapes": int, "unit_crcs": [int, ...]}, ...]} with only the
 * fields present (AVR_ERR_FORMAT for a malformed Block field 18, avr_set_unit_checksums) -- and
 * "file_crc": int after "version" when the Metadata holds field 16 -- and (b) the message
 * re-serialised by the library's writer (the one avr_compress_file uses; Metadata.version and field 16 only).
 * Both buffers are malloc'd (avr_free).  AVR_ERR_FORMAT when the bytes are not a Recoded message. */
int avr_container_describe(const uint8_t* in, size_t n, char** json, uint8_t** reserialized, size_t* len);

/* Model neighbour geometry (get_neighbor_sub_mb + reverse_scan_8, recode.cpp:279-312, 419-471) as the
 * kernels use it (HotTables::nb_left / nb_up, loaded into every workgroup's LDS): out[n] (n < 48) =
 * the 4x4 block left of block n, out[48 + n] = the block above it, | 128 when that block lies in
 * the left / upper macroblock.  ctx NULL: the table the library builds on the host (no device
 * needed); a context: read back from that device's copy.  Pinned against the reference compiled
 * here by tests/test_oracle_geometry.py and tests/test_gpu_parity.py. */
int avr_neighbor_tables(avr_ctx* ctx, uint8_t out[96]);

/* ------------------------------------------------ libavcodec-hooks callback surface (AVCodecHooks) */
/* For a caller that drives the recode path from its own H.264 decoder exactly as the reference's
 * libavcodec-hooks fork does (recode.cpp:137-228).  A session runs the whole file on the device up
 * front (compress: recoded container + the decode-order bin trace of every coded slice;
 * decompress: the original file + the same traces), then serves the per-bin callbacks from the
 * traces: get() returns the bin and advances *state the way ff_get_cabac / cabac::encoder::put
 * would (recode.cpp:1176, 1443).  Every callback checks the caller's parse against the device's
 * (state byte before each decision, bin kinds, sub-MB / coding-type pairing, recode.cpp:185-189,
 * 933-947); a mismatch makes avr_hooks_end fail with AVR_ERR_FORMAT.  Not thread-safe.
 * LIMITATION (by design): the caller's parse never drives the model.  In the reference the
 * decoder's own calls decide the model keys bin by bin (recode.cpp:1435-1449); here the device's
 * parse (avr_walker.h) has decided every bin, key and coding-type event before the first callback,
 * and the callbacks only replay and verify it.  A caller whose decoder parses a slice differently
 * (another FFmpeg revision's syntax handling, a damaged stream it conceals) is refused with
 * AVR_ERR_FORMAT instead of being followed. */
typedef struct avr_hooks_session avr_hooks_session;

/* CodingType (EACH_PIP_CODING_TYPE, recode.cpp:616) */
typedef enum {
  AVR_PIP_UNKNOWN = 0, AVR_PIP_UNREACHABLE, AVR_PIP_SIGNIFICANCE_MAP, AVR_PIP_SIGNIFICANCE_EOB,
  AVR_PIP_SIGNIFICANCE_NZ, AVR_PIP_RESIDUALS
} avr_pip_coding_type;

/* compressor(input, out) (recode.cpp:1102-1113): file = the H.264 file the caller decodes. */
int avr_hooks_compress_begin(avr_ctx* ctx, const uint8_t* file, size_t n, int model, avr_hooks_session** out);
/* decompressor(input, out) (recode.cpp:1312-1336): avrc = a Recoded container.  *stream is what
 * read_packet feeds the decoder (literals + surrogate blocks, recode.cpp:1359-1409), valid until
 * avr_hooks_destroy.  A parallel-model container (avrecode-amd:P64 / P32) is decoded on demand, as
 * the reference decodes each slice when the decoder reaches it (recode.cpp:1411-1520): begin only
 * plans it; an avr_hook_init_decoder that reaches a slice not yet regenerated regenerates it on
 * the device together with at most 31 coded slices after it, and avr_hooks_end regenerates the
 * rest for the output file.  A reference-model container is regenerated whole at begin (its
 * estimators chain across slices).  AVR_HOOKS_EAGER=1 in the environment: always whole.
 * A container with re-coded escaped slices (Block field 17; "avrecode-amd:P64E" / "P32E") is
 * refused with AVR_ERR_UNSUPPORTED: *stream has no form for a block that stands for escaped bytes.
 * It decompresses through the whole-file calls and the plans.  Compress sessions never write the
 * field, whatever avr_set_recode_escaped says. */
int avr_hooks_decompress_begin(avr_ctx* ctx, const uint8_t* avrc, size_t n, avr_hooks_session** out,
                               const uint8_t** stream, size_t* stream_len);
/* Streaming compress: the caller's demuxer hands the file's bytes to the session as it reads them
 * (avr_hooks_feed: the fork's read_packet, recode.cpp:1127-1131) instead of the whole file up front.
 * Each init_decoder finds its slice in the bytes fed so far and traces that slice alone on the device
 * (the hooks answer with the CABAC parse, whichever model the container uses); a slice not yet fed
 * completely fails the session.  avr_hooks_end compresses the complete file with `model` -- the
 * container needs every slice's model state, as the reference writes it after the last slice
 * (recode.cpp:1102-1125) -- and returns it as avr_hooks_compress_begin's session would.  The
 * callbacks and their checks are the same. */
int avr_hooks_compress_stream_begin(avr_ctx* ctx, int model, avr_hooks_session** out);
int avr_hooks_feed(avr_hooks_session* s, const uint8_t* bytes, size_t n);
/* AVCodecHooks.cabac: opaque = the session.  init_decoder returns the per-slice opaque, or NULL
 * when the slice is not re-coded (the caller then decodes it natively, recode.cpp:1139-1145). */
void* avr_hook_init_decoder(void* opaque, void* cabac_context, const uint8_t* buf, int size);
int avr_hook_get(void* slice, uint8_t* state);
int avr_hook_get_bypass(void* slice);
int avr_hook_get_terminate(void* slice);
/* I_PCM is unsupported, as in the reference (recode.cpp:161-163): records an error, returns NULL. */
const uint8_t* avr_hook_skip_bytes(void* slice, int n);
/* AVCodecHooks.model: opaque = the session */
void avr_hook_frame_spec(void* opaque, int frame_num, int mb_width, int mb_height);
void avr_hook_mb_xy(void* opaque, int x, int y);
void avr_hook_begin_sub_mb(void* opaque, int cat, int scan8index, int max_coeff, int is_dc, int chroma422);
void avr_hook_end_sub_mb(void* opaque, int cat, int scan8index, int max_coeff, int is_dc, int chroma422);
void avr_hook_begin_coding_type(void* opaque, int coding_type, int zigzag_index, int param0, int param1);
void avr_hook_end_coding_type(void* opaque, int coding_type);
/* compress: *out = the Recoded container; decompress: *out = the original file (avr_free). */
int avr_hooks_end(avr_hooks_session* s, uint8_t** out, size_t* out_len);
void avr_hooks_destroy(avr_hooks_session* s);

/* --------------------------------------------------------------- synthetic H.264 (benchmarks) */
typedef struct {
  int32_t mb_width, mb_height;   /* e.g. 120 x 68 for 1080p */
  int32_t slice_type;            /* 0 P, 1 B, 2 I */
  int32_t slice_qp;
  int32_t chroma_format_idc;     /* 1 (4:2:0) .. 3 */
  int32_t transform_8x8_mode;
  int32_t num_ref_idx_l0, num_ref_idx_l1;
  uint64_t seed;
  int32_t slices_per_picture;    /* 0 or 1: one slice per picture; k: k slices (equal MB runs) */
  int32_t gop_length;            /* 0: every picture has slice_type; g > 0: picture i is an IDR
                                  * I picture when i % g == 0, else slice_type (e.g. I + 31 P);
                                  * with slice_type B: I B B P B B P ... (P when (i % g) % 3 == 0) */
  int32_t repeat;                /* 0 or 1: once; r > 1: the n generated pictures are written r
                                  * times, copy t with frame_num / idr_pic_id advanced by t n (a
                                  * long stream tiled from one GOP; the payloads repeat) */
  int32_t structure;             /* 0 progressive frames; 1 field pictures (PAFF: each picture a
                                  * top then a bottom field, mb_height even); 2 MBAFF frames (every
                                  * macroblock pair field or frame coded at random, mb_height even);
                                  * 3 field pictures, bottom field first */
} avr_synth_params;
/* Generate n pictures on the device (each slices_per_picture slices, in decode order) and return
 * them as one Annex-B stream (SPS/PPS + the slice NAL units) in host memory.  Pictures are
 * consecutive frames (frame_num / idr_pic_id = picture index), so the reference model's
 * previous-frame contexts (recode.cpp:824-843, 884) see each P picture's predecessor. */
int avr_synthesize_stream(avr_ctx* ctx, const avr_synth_params* params, int n, uint8_t** out, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif
