"""avrecode-amd: MI355X-native CABAC recode path (ddkang/avrecode's decode -> predict -> re-encode).

Python view of the C ABI in include/avrecode.h (libavrecode.so, built in-tree by
``make -C avrecode_amd``).  The product is the native library and the ``recode`` CLI next to it;
this module is the binding tests, bench.py and the sharded driver use.  There is no Python or CPU
implementation of the hot path: without the library, or without a GPU, every call raises.

Reference interfaces mirrored here (file:line in ddkang/avrecode):
  compress / decompress / roundtrip   recode.cpp:1102-1125, 1312-1357, 1594-1624 (+ CLI 1626-1660)
  parse_stream                        av_decoder::decode_video -> init_decoder(buf, size), recode.cpp:73-143
  Context.compress_slices / ...       compressor::cabac_decoder / decompressor::cabac_decoder per
                                      slice, recode.cpp:1134-1268, 1411-1520
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

__all__ = [
    "AvrError", "Context", "MODEL_REFERENCE", "MODEL_PARALLEL", "MODEL_PARALLEL32", "MODEL_CHAINED", "MODEL_NAMES",
    "SLICE_DESC", "PIECE", "KEEP_ALL",
    "SLICE_RESULT", "SynthParams", "lib", "parse_stream", "assemble_container", "neighbor_tables",
    "plan_decompress", "splice_container", "container_model", "source_sha", "library_path", "EXPORTED_SYMBOLS",
    "seams_of_container", "SPLIT_SLOT", "SplitPlan", "split_plan", "seams_build", "escape_payload",
    "ASSEMBLE_ESCAPED", "ASSEMBLE_SPLIT32", "ASSEMBLE_CRC", "ERR_CHECKSUM", "crc32", "crc32_combine",
    "file_crc_of_container", "Reader", "SPAN", "RANGE_TAIL", "SPAN_LITERAL", "RANGE_NO_POS", "RANGE_SPAN_BYTES",
    "ASSEMBLE_UNIT_CRC", "UNIT_CHECK", "SLICE_CHECKSUM", "unit_checks_apply",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# AVR_LIBRARY selects an instrumented build (e.g. prof/libavrecode.so, `make -C avrecode_amd prof`)
library_path = os.environ.get("AVR_LIBRARY") or os.path.join(_HERE, "libavrecode.so")

# avr_model (include/avrecode.h): the reference model; the parallel model (fresh model per slice)
# on the reference's arithmetic_code<uint64_t, uint8_t>; the parallel model on the optional P32 coder
MODEL_REFERENCE = 0
MODEL_PARALLEL = 1
MODEL_PARALLEL32 = 2
MODEL_CHAINED = 3   # the reference model in chains of CHAIN_SLICES coded slices ("avrecode-amd:R16")
CHAIN_SLICES = 16
ASSEMBLE_ESCAPED = 1   # avr_assemble_container_opts' flag: the second search of Context.recode_escaped
ASSEMBLE_SPLIT32 = 2   # and: seams fields for MODEL_PARALLEL32, under the "P32S" / "P32SE" tags (Context.split_p32)
ASSEMBLE_CRC = 4       # and: a checked container, the file's CRC-32 in Metadata field 16 (Context.checksums)
ASSEMBLE_UNIT_CRC = 16  # and: unit checksums, a CRC-32 per slice / piece in Block field 18 (Context.unit_checksums)
ERR_CHECKSUM = -7      # AVR_ERR_CHECKSUM: the container decoded, and its file is not the file it was made from
SPLIT_BYTES_DEFAULT = 98304   # the parallel model's long-slice split (Context.split_bytes), unless AVR_SPLIT_BYTES
MODEL_NAMES = {MODEL_REFERENCE: "R", MODEL_PARALLEL: "P", MODEL_PARALLEL32: "P32", MODEL_CHAINED: "C"}

AVR_OK = 0
_STATUS = {
    -1: "invalid argument", -2: "device error", -3: "format error", -4: "out of memory",
    -5: "roundtrip mismatch", -6: "unsupported", -7: "checksum mismatch",
}

# every function include/avrecode.h declares
EXPORTED_SYMBOLS = (
    "avr_create", "avr_destroy", "avr_last_error", "avr_free", "avr_compress_file", "avr_decompress_file",
    "avr_roundtrip_file", "avr_compress_slices", "avr_decompress_slices", "avr_pack_outputs",
    "avr_roundtrip_slices", "avr_derive_decompress_descs", "avr_verify_slices", "avr_parse_stream",
    "avr_assemble_container", "avr_assemble_container_parsed", "avr_assemble_container_into", "avr_parse_stream_range", "avr_slice_payload_sizes", "avr_dec_plan_new", "avr_dec_plan_free", "avr_dec_plan_load", "avr_dec_plan_descs", "avr_dec_plan_arena", "avr_dec_plan_splice", "avr_container_model", "avr_synthesize_stream",
    "avr_container_describe", "avr_compress_files", "avr_decompress_files",
    "avr_hooks_compress_begin", "avr_hooks_compress_stream_begin", "avr_hooks_feed",
    "avr_hooks_decompress_begin", "avr_hook_init_decoder", "avr_hook_get",
    "avr_hook_get_bypass", "avr_hook_get_terminate", "avr_hook_skip_bytes", "avr_hook_frame_spec", "avr_hook_mb_xy",
    "avr_hook_begin_sub_mb", "avr_hook_end_sub_mb", "avr_hook_begin_coding_type", "avr_hook_end_coding_type",
    "avr_hooks_end", "avr_hooks_destroy", "avr_neighbor_tables", "avr_last_phase_times",
    "avr_plan_decompress", "avr_splice_container", "avr_roundtrip_files", "avr_slice_kernel",
    "avr_compress_chain_range", "avr_decompress_chain_range", "avr_set_split_bytes", "avr_get_split_bytes",
    "avr_dec_plan_load_pieces", "avr_dec_plan_units", "avr_dec_plan_recs", "avr_decompress_pieces", "avr_pack_pieces",
    "avr_split_plan", "avr_seams_build", "avr_assemble_container_seams", "avr_assemble_container_seams_parsed",
    "avr_compress_split_slices", "avr_stage_pieces", "avr_verify_units",
    "avr_set_recode_escaped", "avr_get_recode_escaped", "avr_escape_payload", "avr_assemble_container_opts",
    "avr_set_split_p32", "avr_get_split_p32", "avr_compress_split_slices_m", "avr_decompress_pieces_m",
    "avr_set_checksums", "avr_get_checksums", "avr_crc32", "avr_crc32_combine", "avr_crc_spans",
    "avr_assemble_container_args", "avr_dec_plan_splice_crc",
    "avr_dec_plan_file_size", "avr_dec_plan_range", "avr_dec_plan_range_apply", "avr_gather_spans", "avr_range_tails",
    "avr_reader_open", "avr_reader_info", "avr_reader_read", "avr_reader_read_device", "avr_reader_span",
    "avr_reader_last", "avr_reader_close",
    "avr_set_unit_checksums", "avr_get_unit_checksums", "avr_check_units", "avr_unit_checks_apply",
    "avr_dec_plan_unit_crcs",
)

# avr_slice_desc / avr_slice_result (include/avrecode.h), C layout
SLICE_DESC = np.dtype([
    ("payload_offset", "<u8"), ("payload_size", "<u4"), ("read_limit", "<u4"),
    ("out_offset", "<u8"), ("out_capacity", "<u4"),
    ("slice_type", "<i4"), ("slice_qp", "<i4"), ("cabac_init_idc", "<i4"), ("first_mb", "<i4"),
    ("mb_width", "<i4"), ("mb_height", "<i4"), ("num_ref_idx_l0", "<i4"), ("num_ref_idx_l1", "<i4"),
    ("chroma_array_type", "<i4"), ("transform_8x8_mode", "<i4"), ("direct_8x8_inference", "<i4"),
    ("x264_build", "<i4"), ("picture_id", "<i4"), ("coded", "<i4"), ("structure", "<i4"),
    ("file_offset", "<u8"),
], align=True)
SLICE_RESULT = np.dtype([("out_len", "<u4"), ("status", "<i4"), ("bins", "<u4"), ("mbs", "<u4"),
                         ("bill", "<u4", (6,))], align=True)
# avr_pip_coding_type (CodingType, recode.cpp:616): the index of avr_file_stats.bill / cabac_bill
CODING_TYPES = ("PIP_UNKNOWN", "PIP_UNREACHABLE", "PIP_SIGNIFICANCE_MAP", "PIP_SIGNIFICANCE_EOB",
                "PIP_SIGNIFICANCE_NZ", "PIP_RESIDUALS")
# avr_piece (include/avrecode.h): what a unit of a piece plan is of its slice
PIECE = np.dtype([("seam", "<i4"), ("n_mbs", "<u4"), ("slice", "<i4"), ("keep", "<u4")], align=True)
KEEP_ALL = 0xFFFFFFFF    # avr_piece.keep of a last piece or a whole slice
SLICE_NO_END = -9        # AVR_SLICE_NO_END
SLICE_CODER = -10        # AVR_SLICE_CODER
SLICE_OVERFLOW = -12     # AVR_SLICE_OVERFLOW
SLICE_CHECKSUM = -22     # AVR_SLICE_CHECKSUM: a unit's regenerated bytes miss its CRC (Block field 18)
# avr_split_slot (include/avrecode.h): a slice's cut records in a split compress batch; (-1, 0): none
# avr_span / avr_range_tail (range reads, ABI 12)
SPAN = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("len", "<u4"), ("source", "<i4")], align=True)
RANGE_TAIL = np.dtype([("keep", "<u4"), ("q_last", "<u4"), ("size", "<u4"), ("has_rule", "u1"), ("length_parity", "u1"),
                       ("last_byte", "u1"), ("reserved", "u1"), ("final_pos", "<u8")], align=True)
# avr_unit_check (unit checksums, ABI 13): where a unit's regenerated bytes start, its CRC, whether it has one
UNIT_CHECK = np.dtype([("src_off", "<u8"), ("crc", "<u4"), ("have", "<u4")], align=True)
SPAN_LITERAL = -1               # avr_span.source of a literal: src_off indexes the container
RANGE_NO_POS = 0xFFFFFFFFFFFFFFFF   # avr_range_tail.final_pos: the slice's final byte lies outside the window
RANGE_SPAN_BYTES = 16384        # the planner's default span cap
SPLIT_SLOT = np.dtype([("first", "<i4"), ("cap", "<u4")], align=True)
# the head of a seam record in the split kernels' device layout (SeamRec, csrc/avr_records.h); then
# 1024 context bytes and 40 edge bytes per macroblock column
SEAM_HEAD = np.dtype([("first_mb", "<u4"), ("last_dqp_nz", "<u4"), ("cd", "<u4", (4,)), ("ce_low", "<u4"),
                      ("ce_range", "<u4"), ("ce_outstanding", "<u4"), ("ce_cache", "<u4"), ("ce_queue", "<i4"),
                      ("q", "<u4")])
assert SLICE_DESC.itemsize == 96 and SLICE_RESULT.itemsize == 40 and PIECE.itemsize == 16 and SPLIT_SLOT.itemsize == 8


class AvrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"avrecode: {_STATUS.get(code, code)}: {msg}")
        self.code = code


PHASES = ("demux_s", "upload_s", "kernel_s", "download_s", "container_s", "other_s")


class _PhaseTimes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in PHASES]


def _phases(p: _PhaseTimes) -> dict:
    return {n: getattr(p, n) for n in PHASES}


class _FileStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("file_bytes", "slices", "coded_slices", "skipped_slices", "payload_bytes", "recoded_bytes", "bins")] + \
               [("compress_s", ctypes.c_double), ("decompress_s", ctypes.c_double),
                ("bill", ctypes.c_uint64 * 6), ("cabac_bill", ctypes.c_uint64 * 6),
                ("attempts", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("compress_phases", _PhaseTimes), ("decompress_phases", _PhaseTimes)]


class _RangeInfo(ctypes.Structure):   # avr_range_info
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("file_size", ctypes.c_uint64),
                ("literal_bytes", ctypes.c_uint64), ("unit_lo", ctypes.c_int32), ("unit_hi", ctypes.c_int32),
                ("n_spans", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _ReaderInfo(ctypes.Structure):   # avr_reader_info_t
    _fields_ = [("file_size", ctypes.c_uint64), ("model", ctypes.c_int32), ("random_access", ctypes.c_int32),
                ("n_blocks", ctypes.c_int32), ("n_units", ctypes.c_int32), ("checked", ctypes.c_int32),
                ("unit_checked", ctypes.c_int32)]


class _ReadStats(ctypes.Structure):   # avr_read_stats
    _fields_ = [("units", ctypes.c_uint64), ("pieces", ctypes.c_uint64), ("regenerated_bytes", ctypes.c_uint64),
                ("literal_bytes", ctypes.c_uint64), ("spans", ctypes.c_uint64), ("phases", _PhaseTimes)]


class _AssembleArgs(ctypes.Structure):   # avr_assemble_args
    _fields_ = [("size", ctypes.c_size_t), ("file", ctypes.c_void_p), ("n", ctypes.c_size_t), ("model", ctypes.c_int),
                ("descs", ctypes.c_void_p), ("n_slices", ctypes.c_int), ("arena", ctypes.c_void_p),
                ("arena_len", ctypes.c_size_t), ("status", ctypes.c_void_p), ("recoded", ctypes.c_void_p),
                ("recoded_len", ctypes.c_size_t), ("offsets", ctypes.c_void_p), ("lens", ctypes.c_void_p),
                ("seams", ctypes.c_void_p), ("seams_len", ctypes.c_size_t), ("seam_offsets", ctypes.c_void_p),
                ("seam_lens", ctypes.c_void_p), ("flags", ctypes.c_uint32), ("crcs", ctypes.c_void_p)]


class _SynthParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("mb_width", "mb_height", "slice_type", "slice_qp", "chroma_format_idc", "transform_8x8_mode",
                 "num_ref_idx_l0", "num_ref_idx_l1")] + [("seed", ctypes.c_uint64)] + \
               [("slices_per_picture", ctypes.c_int32), ("gop_length", ctypes.c_int32), ("repeat", ctypes.c_int32),
                ("structure", ctypes.c_int32)]


@dataclass
class SynthParams:
    """Synthetic slice parameters (avr_synth_params); defaults = one 1080p 4:2:0 High I picture."""
    mb_width: int = 120
    mb_height: int = 68
    slice_type: int = 2
    slice_qp: int = 26
    chroma_format_idc: int = 1
    transform_8x8_mode: int = 1
    num_ref_idx_l0: int = 1
    num_ref_idx_l1: int = 1
    seed: int = 0
    slices_per_picture: int = 1
    gop_length: int = 0          # > 0: IDR I picture every gop_length pictures, slice_type between
    repeat: int = 1              # > 1: the pictures written this many times (frame numbers advance)
    structure: int = 0           # 0 progressive, 1 field pictures (PAFF), 2 MBAFF frames, 3 PAFF bottom first


_lib = None


def source_sha() -> str:
    """sha256 over the native sources libavrecode.so is built from (avrecode_amd/csrc/*,
    include/avrecode.h, the Makefile): identifies the build a profile was taken on, without git
    (the GPU box has no .git).  scripts/pmc_traffic.py records it; bench.py uses a traffic
    profile only when it matches the tree being measured."""
    import hashlib
    root = os.path.dirname(_HERE)
    files = sorted(os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc")))
    files += [os.path.join(root, "include", "avrecode.h"), os.path.join(_HERE, "Makefile")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def lib() -> ctypes.CDLL:
    """Load libavrecode.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(library_path):
        raise ImportError(f"{library_path} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build())")
    L = ctypes.CDLL(library_path)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    pp = ctypes.POINTER(ctypes.c_void_p)
    psz = ctypes.POINTER(ctypes.c_size_t)
    pi = ctypes.POINTER(ctypes.c_int)
    L.avr_create.argtypes = [i32, pp]
    L.avr_destroy.argtypes = [vp]
    L.avr_destroy.restype = None
    L.avr_last_error.argtypes = [vp]
    L.avr_last_error.restype = ctypes.c_char_p
    L.avr_free.argtypes = [vp]
    L.avr_free.restype = None
    L.avr_compress_file.argtypes = [vp, vp, sz, i32, pp, psz]
    L.avr_decompress_file.argtypes = [vp, vp, sz, pp, psz]
    L.avr_roundtrip_file.argtypes = [vp, vp, sz, i32, pp, psz, ctypes.POINTER(_FileStats)]
    for f in (L.avr_compress_slices, L.avr_decompress_slices):
        f.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, vp]
    L.avr_roundtrip_slices.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.avr_derive_decompress_descs.argtypes = [vp, vp, vp, i32, vp, vp]
    L.avr_verify_slices.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.avr_slice_kernel.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_int)]
    L.avr_compress_chain_range.argtypes = [vp, vp, sz, i32, i32] + [vp] * 7
    L.avr_decompress_chain_range.argtypes = [vp, vp, sz, i32, i32] + [vp] * 7
    L.avr_pack_outputs.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    L.avr_parse_stream.argtypes = [vp, sz, pp, pi, pp, psz, psz, pi, pi]
    L.avr_parse_stream_range.argtypes = [vp, sz, i32, i32, pp, pi, pp, psz, psz, pi, pi]
    L.avr_slice_payload_sizes.argtypes = [vp, sz, pp, pi]
    L.avr_assemble_container.argtypes = [vp, sz, i32, i32, vp, vp, sz, vp, vp, pp, psz]
    L.avr_assemble_container_parsed.argtypes = [vp, sz, i32, vp, i32, vp, sz, vp, vp, sz, vp, vp, pp, psz]
    L.avr_assemble_container_into.argtypes = [vp, sz, i32, vp, i32, vp, sz, vp, vp, sz, vp, vp, vp, sz, psz]
    L.avr_dec_plan_new.argtypes = [pp]
    L.avr_dec_plan_free.argtypes = [vp]
    L.avr_dec_plan_free.restype = None
    L.avr_dec_plan_load.argtypes = [vp, vp, sz, pi, psz, psz, pi, pi]
    L.avr_dec_plan_descs.argtypes = [vp, vp]
    L.avr_dec_plan_arena.argtypes = [vp, vp, sz]
    L.avr_dec_plan_splice.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, psz]
    L.avr_dec_plan_load_pieces.argtypes = [vp, vp, sz, pi, pi, psz, psz, pi, pi, pi, psz]
    L.avr_dec_plan_units.argtypes = [vp, vp, vp]
    L.avr_dec_plan_recs.argtypes = [vp, vp, sz]
    L.avr_decompress_pieces.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, sz, vp, vp, vp, vp]
    L.avr_pack_pieces.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.avr_split_plan.argtypes = [vp, i32, sz, vp, vp, pi, psz, pi]
    L.avr_seams_build.argtypes = [vp, i32, vp, sz, vp, vp, vp, vp, i32, vp, sz, sz, i32, vp, pp, psz, vp, vp]
    L.avr_assemble_container_seams.argtypes = [vp, sz, i32, i32, vp, vp, sz, vp, vp, vp, sz, vp, vp, pp, psz]
    L.avr_assemble_container_seams_parsed.argtypes = [vp, sz, i32, vp, i32, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp,
                                                      pp, psz]
    L.avr_compress_split_slices.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp, i32, sz, vp, vp, vp]
    L.avr_stage_pieces.argtypes = [vp, vp, vp, i32, vp, sz, vp, sz, vp, vp, vp]
    L.avr_verify_units.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.avr_container_model.argtypes = [vp, sz, pi]
    L.avr_synthesize_stream.argtypes = [vp, ctypes.POINTER(_SynthParams), i32, pp, psz]
    L.avr_container_describe.argtypes = [vp, sz, pp, pp, psz]
    L.avr_compress_files.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    L.avr_decompress_files.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.avr_roundtrip_files.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp]
    L.avr_neighbor_tables.argtypes = [vp, vp]
    L.avr_plan_decompress.argtypes = [vp, sz, pp, pi, pp, psz, psz, pi, pi]
    L.avr_splice_container.argtypes = [vp, sz, i32, vp, vp, sz, vp, vp, pp, psz]
    L.avr_last_phase_times.argtypes = [vp, vp]
    L.avr_set_split_bytes.argtypes = [vp, sz]
    L.avr_set_recode_escaped.argtypes = [vp, i32]
    L.avr_set_split_p32.argtypes = [vp, i32]
    L.avr_get_split_p32.argtypes = [vp]
    L.avr_decompress_pieces_m.argtypes = [vp, i32, vp, vp, i32, i32, i32, vp, i32, sz, vp, vp, vp, vp]
    L.avr_compress_split_slices_m.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp, i32, sz, vp, vp, vp]
    L.avr_get_recode_escaped.argtypes = [vp]
    L.avr_escape_payload.argtypes = [vp, sz, vp, sz, psz]
    L.avr_assemble_container_opts.argtypes = [vp, sz, i32, vp, i32, vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp,
                                              ctypes.c_uint32, pp, psz]
    L.avr_get_split_bytes.argtypes = [vp]
    L.avr_set_checksums.argtypes = [vp, i32]
    L.avr_get_checksums.argtypes = [vp]
    L.avr_crc32.argtypes = [ctypes.c_uint32, vp, sz]
    L.avr_crc32.restype = ctypes.c_uint32
    L.avr_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    L.avr_crc32_combine.restype = ctypes.c_uint32
    L.avr_crc_spans.argtypes = [vp, vp, sz, vp, vp, i32, vp, vp, vp]
    L.avr_assemble_container_args.argtypes = [ctypes.POINTER(_AssembleArgs), pp, psz]
    L.avr_dec_plan_splice_crc.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, psz]
    L.avr_get_split_bytes.restype = sz
    u64 = ctypes.c_uint64
    L.avr_dec_plan_file_size.argtypes = [vp, ctypes.POINTER(u64)]
    L.avr_dec_plan_range.argtypes = [vp, u64, u64, ctypes.c_uint32, ctypes.POINTER(_RangeInfo), pp, pp]
    L.avr_dec_plan_range_apply.argtypes = [vp, i32, vp, i32, vp, sz, vp, sz, vp, vp, vp, sz, vp]
    L.avr_gather_spans.argtypes = [vp, vp, i32, vp, sz, vp, sz, vp, vp]
    L.avr_range_tails.argtypes = [vp, vp, vp, i32, vp, sz, vp, vp]
    L.avr_reader_open.argtypes = [vp, vp, sz, pp]
    L.avr_reader_info.argtypes = [vp, ctypes.POINTER(_ReaderInfo)]
    L.avr_reader_read.argtypes = [vp, u64, sz, vp, psz]
    L.avr_reader_read_device.argtypes = [vp, u64, sz, vp, psz]
    L.avr_reader_span.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), pi]
    L.avr_reader_last.argtypes = [vp, ctypes.POINTER(_ReadStats)]
    L.avr_reader_close.argtypes = [vp]
    L.avr_reader_close.restype = None
    L.avr_set_unit_checksums.argtypes = [vp, i32]
    L.avr_get_unit_checksums.argtypes = [vp]
    L.avr_check_units.argtypes = [vp, vp, vp, vp, i32, vp, sz, vp, vp]
    L.avr_unit_checks_apply.argtypes = [vp, vp, vp, i32, vp, sz, vp]
    L.avr_dec_plan_unit_crcs.argtypes = [vp, i32, i32, vp]
    for name in EXPORTED_SYMBOLS:   # fails here, not at first use, when the build is stale
        getattr(L, name)
    _lib = L
    return L


def _buf(data) -> tuple[ctypes.c_void_p, int, object]:
    """(pointer, length, keepalive) for bytes / bytearray / memoryview / numpy uint8, without a copy
    (the library only reads its inputs; a 4.47 GB stream must not be duplicated per call)."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    elif isinstance(data, (bytes, bytearray, memoryview)):
        a = np.frombuffer(data, dtype=np.uint8)
    else:
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    if a.nbytes == 0:   # a valid, non-null pointer for empty inputs
        cb = ctypes.create_string_buffer(1)
        return ctypes.cast(cb, ctypes.c_void_p), 0, cb
    return ctypes.c_void_p(a.ctypes.data), a.nbytes, a


def _take(p: ctypes.c_void_p, n: int) -> bytes:
    L = lib()
    try:
        if not n:
            return b""
        # ctypes.string_at's length is a C int: a buffer of 2 GiB or more (a 10-minute 4K stream,
        # its container) is copied through an array view instead
        return ctypes.string_at(p.value, n) if n < (1 << 31) else bytes((ctypes.c_char * n).from_address(p.value))
    finally:
        L.avr_free(p)


class _LibBuffer:
    """A malloc'd library buffer exposed to numpy without a copy; freed (avr_free) when the last
    array viewing it is gone (numpy keeps this object as every view's base)."""

    def __init__(self, p: int, n: int):
        self._p = p
        self._free = lib().avr_free   # held: at interpreter exit the module's globals may be gone
        self._vp = ctypes.c_void_p
        self.__array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (p, False), "version": 3}

    def __del__(self):
        if self._p:
            self._free(self._vp(self._p))
            self._p = 0


def _take_array(p: ctypes.c_void_p, n: int) -> np.ndarray:
    """A library buffer as a numpy uint8 array, without copying it (a 4 GB parse or container is not
    copied again); the buffer is freed with the array."""
    if not n or not p.value:
        if p.value:
            lib().avr_free(p)
        return np.zeros(0, dtype=np.uint8)
    return np.asarray(_LibBuffer(p.value, n))


@dataclass
class ParsedStream:
    """Per-slice descriptors + payload arena (what init_decoder receives, recode.cpp:143)."""
    descs: np.ndarray        # SLICE_DESC[n]
    arena: np.ndarray        # uint8 payloads (16-byte aligned, zero padded)
    work_len: int            # bytes of compress output space the descs' out_offset/out_capacity index
    max_mb_width: int
    max_mb_height: int
    # the units of a piece plan (DecompressPlan.parsed_units): what each desc is of its slice, and the
    # seam records the pieces start from (rec_stride bytes each, the split kernels' device layout)
    pieces: "np.ndarray | None" = None   # PIECE[n]
    recs: "np.ndarray | None" = None     # uint8
    rec_stride: int = 0

    @property
    def payload_bytes(self) -> int:
        return int(self.descs["payload_size"].sum())


def parse_stream(data, lo: int = 0, hi: "int | None" = None) -> ParsedStream:
    """Host-side slice extraction (avr_parse_stream; with a slice range [lo, hi),
    avr_parse_stream_range: that range only, rebased as shard.subset would).  Needs no GPU."""
    L = lib()
    p, n, keep = _buf(data)
    descs, arena = ctypes.c_void_p(), ctypes.c_void_p()
    ns, mw, mh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    alen, wlen = ctypes.c_size_t(), ctypes.c_size_t()
    if lo == 0 and hi is None:
        r = L.avr_parse_stream(p, n, ctypes.byref(descs), ctypes.byref(ns), ctypes.byref(arena), ctypes.byref(alen),
                               ctypes.byref(wlen), ctypes.byref(mw), ctypes.byref(mh))
    else:
        r = L.avr_parse_stream_range(p, n, int(lo), -1 if hi is None else int(hi), ctypes.byref(descs),
                                     ctypes.byref(ns), ctypes.byref(arena), ctypes.byref(alen), ctypes.byref(wlen),
                                     ctypes.byref(mw), ctypes.byref(mh))
    del keep
    if r != AVR_OK:
        raise AvrError(r, "avr_parse_stream failed")
    d = _take_array(descs, ns.value * SLICE_DESC.itemsize).view(SLICE_DESC)
    a = _take_array(arena, alen.value)
    return ParsedStream(d, a, int(wlen.value), int(mw.value), int(mh.value))


def slice_payload_sizes(data) -> np.ndarray:
    """Every CABAC slice's payload_size (avr_slice_payload_sizes): a sharded run's partition input,
    without copying the payloads.  Host only."""
    p, n, keep = _buf(data)
    out, ns = ctypes.c_void_p(), ctypes.c_int()
    r = lib().avr_slice_payload_sizes(p, n, ctypes.byref(out), ctypes.byref(ns))
    if r != AVR_OK:
        raise AvrError(r, "avr_slice_payload_sizes failed")
    return _take_array(out, 4 * ns.value).view(np.uint32)


def plan_decompress(avrc) -> ParsedStream:
    """A PARALLEL-model container's coded slices as a decompress batch (avr_plan_decompress): the
    descs' payloads are the re-coded streams, their outputs the regenerated CABAC bytes.  Host only."""
    L = lib()
    p, n, keep = _buf(avrc)
    descs, arena = ctypes.c_void_p(), ctypes.c_void_p()
    ns, mw, mh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    alen, wlen = ctypes.c_size_t(), ctypes.c_size_t()
    r = L.avr_plan_decompress(p, n, ctypes.byref(descs), ctypes.byref(ns), ctypes.byref(arena), ctypes.byref(alen),
                              ctypes.byref(wlen), ctypes.byref(mw), ctypes.byref(mh))
    del keep
    if r != AVR_OK:
        raise AvrError(r, "avr_plan_decompress failed")
    d = _take_array(descs, ns.value * SLICE_DESC.itemsize).view(SLICE_DESC)
    a = _take_array(arena, alen.value)
    return ParsedStream(d, a, int(wlen.value), int(mw.value), int(mh.value))


class DecompressPlan:
    """The sharded decompress's host halves on one parse of a PARALLEL-model container
    (avr_dec_plan_*): load(avrc) plans it (no bytes copied), parsed(arena_out) gives the decompress
    batch (descs + the re-coded streams' arena, written into arena_out when given), splice(...) the
    file from the regenerated slices (into out when given: the view holding the file is returned).
    The handle keeps its scratch across loads; the container passed to load must stay alive and
    unchanged until the next load.  Host only.

    load(avrc, pieces=True) makes it a piece plan (avr_dec_plan_load_pieces), which also reads a
    container whose long slices were cut (Context.split_bytes): n_slices / descs stay the coded
    slices, the splice's indexing, and n_units / units / pieces list what one workgroup regenerates,
    a whole slice or one piece of a split slice, with the seam records in recs (rec_stride bytes
    each).  parsed_units(arena_out) gives that batch; shard.collapse_units turns its per-unit results
    into splice()'s per-slice ones."""

    def __init__(self):
        self._h = ctypes.c_void_p()
        r = lib().avr_dec_plan_new(ctypes.byref(self._h))
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_new failed")
        self._keep = None

    def load(self, avrc, pieces: bool = False) -> "DecompressPlan":
        p, n, keep = _buf(avrc)
        ns, mw, mh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        al, wl = ctypes.c_size_t(), ctypes.c_size_t()
        nu, nr, rs = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        self.n_units = self.units = self.pieces = self.recs = None
        self.rec_stride = 0
        if pieces:
            r = lib().avr_dec_plan_load_pieces(self._h, p, n, ctypes.byref(ns), ctypes.byref(nu), ctypes.byref(al),
                                               ctypes.byref(wl), ctypes.byref(mw), ctypes.byref(mh), ctypes.byref(nr),
                                               ctypes.byref(rs))
        else:
            r = lib().avr_dec_plan_load(self._h, p, n, ctypes.byref(ns), ctypes.byref(al), ctypes.byref(wl),
                                        ctypes.byref(mw), ctypes.byref(mh))
        if r != AVR_OK:
            self._keep = None
            raise AvrError(r, "avr_dec_plan_load_pieces failed" if pieces else "avr_dec_plan_load failed")
        self._keep = (avrc, keep)
        self.n_slices, self.arena_len, self.work_len = ns.value, al.value, wl.value
        self.max_mb_width, self.max_mb_height = mw.value, mh.value
        d = np.zeros(self.n_slices, dtype=SLICE_DESC)
        if self.n_slices:
            lib().avr_dec_plan_descs(self._h, d.ctypes.data)
        self.descs = d
        if pieces:
            self.n_units, self.rec_stride = nu.value, rs.value
            self.units = np.zeros(self.n_units, dtype=SLICE_DESC)
            self.pieces = np.zeros(self.n_units, dtype=PIECE)
            self.recs = np.zeros(nr.value * rs.value, dtype=np.uint8)
            r = lib().avr_dec_plan_units(self._h, self.units.ctypes.data, self.pieces.ctypes.data)
            r = r or lib().avr_dec_plan_recs(self._h, self.recs.ctypes.data, self.recs.nbytes)
            if r != AVR_OK:
                raise AvrError(r, "avr_dec_plan_units / avr_dec_plan_recs failed")
        return self

    def parsed(self, arena_out: "np.ndarray | None" = None) -> ParsedStream:
        a = np.empty(self.arena_len, dtype=np.uint8) if arena_out is None else arena_out[:self.arena_len]
        if a.nbytes < self.arena_len:
            raise ValueError("DecompressPlan.parsed: arena_out too small")
        r = lib().avr_dec_plan_arena(self._h, a.ctypes.data, a.nbytes)
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_arena failed")
        if self.units is not None:
            raise ValueError("DecompressPlan.parsed: a piece plan's batch is parsed_units()")
        return ParsedStream(self.descs.copy(), a, self.work_len, self.max_mb_width, self.max_mb_height)

    def parsed_units(self, arena_out: "np.ndarray | None" = None) -> ParsedStream:
        """A piece plan's batch: the units' descs and streams, with pieces / recs / rec_stride."""
        if self.units is None:
            raise ValueError("DecompressPlan.parsed_units: load(avrc, pieces=True) first")
        a = np.empty(self.arena_len, dtype=np.uint8) if arena_out is None else arena_out[:self.arena_len]
        if a.nbytes < self.arena_len:
            raise ValueError("DecompressPlan.parsed_units: arena_out too small")
        r = lib().avr_dec_plan_arena(self._h, a.ctypes.data, a.nbytes)
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_arena failed")
        return ParsedStream(self.units.copy(), a, self.work_len, self.max_mb_width, self.max_mb_height,
                            self.pieces.copy(), self.recs, self.rec_stride)

    def splice(self, status, regen, offsets, lens, out: "np.ndarray | None" = None, crcs=None):
        """The file from the regenerated slices (avr_dec_plan_splice).  A checked container is checked
        (AvrError ERR_CHECKSUM); crcs: the CRC-32 of each slice's regenerated bytes as a device
        computed it (avr_dec_plan_splice_crc), else the splice computes them on host threads."""
        st = np.ascontiguousarray(status, dtype=np.int32)
        of = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        if len(st) != self.n_slices or len(of) != len(st) or len(ln) != len(st):
            raise ValueError("DecompressPlan.splice: one status / offset / length per planned slice")
        rp, rn, keep = _buf(regen)
        olen = ctypes.c_size_t()
        L = lib()
        cr = None if crcs is None else np.ascontiguousarray(crcs, dtype=np.uint32)
        if cr is not None and len(cr) != len(st):
            raise ValueError("DecompressPlan.splice: one crc per planned slice")
        cp = None if cr is None else cr.ctypes.data
        if out is None:
            r = L.avr_dec_plan_splice_crc(self._h, st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data, cp, None, 0,
                                          ctypes.byref(olen))
            if r == ERR_CHECKSUM:
                raise AvrError(r, "avr_dec_plan_splice failed")
            out = np.empty(olen.value, dtype=np.uint8)
        r = L.avr_dec_plan_splice_crc(self._h, st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data, cp,
                                      out.ctypes.data, out.nbytes, ctypes.byref(olen))
        if r != AVR_OK:
            raise AvrError(r, f"avr_dec_plan_splice failed (file {olen.value} B, buffer {out.nbytes} B)")
        return out[:olen.value]

    @property
    def file_size(self) -> int:
        """The size of the file the loaded container restores (avr_dec_plan_file_size): the prefix sum
        of its blocks, from the container alone."""
        v = ctypes.c_uint64()
        r = lib().avr_dec_plan_file_size(self._h, ctypes.byref(v))
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_file_size failed")
        return int(v.value)

    def range(self, off: int, n: int, span_cap: int = 0) -> dict:
        """The window [off, off + n) of the file, clamped to it, planned (avr_dec_plan_range; a piece
        plan): {"off", "len", "file_size", "literal_bytes", "unit_lo", "unit_hi", "spans": SPAN[],
        "tails": RANGE_TAIL[unit_hi - unit_lo]}.  A span's source is SPAN_LITERAL (src_off indexes the
        container) or k >= 0 (the regenerated bytes of unit unit_lo + k); none is longer than span_cap
        (0: RANGE_SPAN_BYTES)."""
        info, sp, tl = _RangeInfo(), ctypes.c_void_p(), ctypes.c_void_p()
        r = lib().avr_dec_plan_range(self._h, int(off), int(n), int(span_cap), ctypes.byref(info), ctypes.byref(sp),
                                     ctypes.byref(tl))
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_range failed")
        nu = info.unit_hi - info.unit_lo
        spans = _take_array(sp, max(1, info.n_spans) * SPAN.itemsize).view(SPAN)[:info.n_spans].copy()
        tails = _take_array(tl, max(1, nu) * RANGE_TAIL.itemsize).view(RANGE_TAIL)[:nu].copy()
        return {"off": int(info.off), "len": int(info.len), "file_size": int(info.file_size),
                "literal_bytes": int(info.literal_bytes), "unit_lo": int(info.unit_lo), "unit_hi": int(info.unit_hi),
                "spans": spans, "tails": tails}

    def range_apply(self, rng: dict, regen, unit_off, res) -> "tuple[bytes, np.ndarray]":
        """A planned window applied on the host (avr_dec_plan_range_apply): unit unit_lo + k's regenerated
        bytes stand at regen[unit_off[k]:], its SLICE_RESULT in res[k].  Returns (the window's bytes,
        the per-unit statuses); raises AvrError (format error) when a status is not 0, with the
        statuses as the exception's `status`."""
        avrc, keep = self._keep
        cp, cn, ckeep = _buf(avrc)
        rp, rn, rkeep = _buf(regen)
        spans = np.ascontiguousarray(rng["spans"], dtype=SPAN)
        tails = np.ascontiguousarray(rng["tails"], dtype=RANGE_TAIL)
        uo = np.ascontiguousarray(unit_off, dtype=np.uint64)
        rs = np.ascontiguousarray(res, dtype=SLICE_RESULT)
        nu = len(tails)
        if len(uo) != nu or len(rs) != nu:
            raise ValueError("DecompressPlan.range_apply: one offset and one result per selected unit")
        out = np.zeros(max(1, rng["len"]), dtype=np.uint8)
        st = np.zeros(max(1, nu), dtype=np.int32)
        r = lib().avr_dec_plan_range_apply(spans.ctypes.data, len(spans), tails.ctypes.data, nu, cp, cn, rp, rn,
                                           uo.ctypes.data, rs.ctypes.data, out.ctypes.data, rng["len"], st.ctypes.data)
        if r != AVR_OK:
            e = AvrError(r, "avr_dec_plan_range_apply failed")
            e.status = st[:nu].copy()
            raise e
        return out[:rng["len"]].tobytes(), st[:nu]

    def unit_crcs(self, unit_lo: int, unit_hi: int) -> np.ndarray:
        """UNIT_CHECK[unit_hi - unit_lo] of a piece plan's units (avr_dec_plan_unit_crcs): crc / have from
        their blocks' unit checksums (Block field 18; have = 0 without the field), src_off left 0 for
        the caller."""
        out = np.zeros(max(1, unit_hi - unit_lo), dtype=UNIT_CHECK)
        r = lib().avr_dec_plan_unit_crcs(self._h, int(unit_lo), int(unit_hi), out.ctypes.data)
        if r != AVR_OK:
            raise AvrError(r, "avr_dec_plan_unit_crcs failed")
        return out[:max(0, unit_hi - unit_lo)]

    def close(self):
        if self._h:
            lib().avr_dec_plan_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unit_checks_apply(tails, checks, res, src, status=None) -> "tuple[int, np.ndarray]":
    """avr_check_units on host buffers (avr_unit_checks_apply): unit k's share of its slice at
    src[checks[k].src_off:], its SLICE_RESULT in res[k], its RANGE_TAIL in tails[k].  status: the units'
    statuses so far (default all 0).  Returns (the call's return code -- 0, ERR_CHECKSUM when it set a
    SLICE_CHECKSUM, format error when it set a SLICE_OVERFLOW -- and the statuses).  Host only."""
    tl = np.ascontiguousarray(tails, dtype=RANGE_TAIL)
    ck = np.ascontiguousarray(checks, dtype=UNIT_CHECK)
    rs = np.ascontiguousarray(res, dtype=SLICE_RESULT)
    n = len(tl)
    if len(ck) != n or len(rs) != n:
        raise ValueError("unit_checks_apply: one check and one result per tail")
    st = np.zeros(max(1, n), dtype=np.int32)
    if status is not None:
        st[:n] = np.asarray(status, dtype=np.int32)
    sp, sn, keep = _buf(src)
    r = lib().avr_unit_checks_apply(tl.ctypes.data, ck.ctypes.data, rs.ctypes.data, n, sp, sn, st.ctypes.data)
    return int(r), st[:n]


def crc32(data, crc: int = 0) -> int:
    """zlib.crc32 through the library (avr_crc32).  Host only."""
    p, n, keep = _buf(data)
    return int(lib().avr_crc32(crc & 0xFFFFFFFF, p, n))


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """crc(A + B) from crc(A), crc(B) and len(B) (avr_crc32_combine).  Host only."""
    return int(lib().avr_crc32_combine(a & 0xFFFFFFFF, b & 0xFFFFFFFF, int(len_b)))


def container_model(avrc) -> int:
    """The model mode a Recoded container was written with (avr_container_model): MODEL_*.  Host only."""
    p, n, keep = _buf(avrc)
    m = ctypes.c_int()
    r = lib().avr_container_model(p, n, ctypes.byref(m))
    if r != AVR_OK:
        raise AvrError(r, "avr_container_model failed")
    return int(m.value)


def splice_container(avrc, status: np.ndarray, regen, offsets: np.ndarray, lens: np.ndarray) -> bytes:
    """The original file from a PARALLEL-model container and its slices' regenerated bytes
    (avr_splice_container; last-byte patch applied here).  regen: bytes or a uint8 array.  Host only."""
    L = lib()
    p, n, keep = _buf(avrc)
    st = np.ascontiguousarray(status, dtype=np.int32)
    of = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    rp, rn, keep2 = _buf(regen)
    out, olen = ctypes.c_void_p(), ctypes.c_size_t()
    r = L.avr_splice_container(p, n, len(st), st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data,
                               ctypes.byref(out), ctypes.byref(olen))
    if r != AVR_OK:
        raise AvrError(r, "avr_splice_container failed")
    return _take(out, olen.value)


def container_bound(n_file: int, n_slices: int, recoded_bytes: int) -> int:
    """An upper bound on the size of a container assembled from n_slices slices of a file of n_file
    bytes with recoded_bytes re-coded bytes in all (avr_assemble_container_into's buffer)."""
    return int(n_file) + int(recoded_bytes) + 64 * (int(n_slices) + 2)


@dataclass
class SplitPlan:
    """avr_split_plan's answer for a batch of descriptors at one split_bytes."""
    slots: np.ndarray          # SPLIT_SLOT[n]: (first, cap) of a candidate's cut records, (-1, 0) otherwise
    out_capacity: np.ndarray   # uint32[n]: the output space a candidate's split walk needs, 0 otherwise
    n_recs: int                # cut records in all
    rec_stride: int            # bytes per record: the widest candidate's
    n_candidates: int

    @property
    def candidate(self) -> np.ndarray:
        return self.slots["first"] >= 0


def split_plan(descs, split_bytes: int) -> SplitPlan:
    """Which descriptors the whole-file MODEL_PARALLEL compress would take through the split walk at
    split_bytes, and the cut-record slots and output space that walk needs (avr_split_plan: a
    progressive frame, at most 288 macroblocks wide, of at least 1.5 split_bytes payload bytes;
    descs' coded field is not read).  Host only."""
    d = np.ascontiguousarray(descs, dtype=SLICE_DESC)
    n = len(d)
    slots = np.zeros(n, dtype=SPLIT_SLOT)
    cap = np.zeros(n, dtype=np.uint32)
    nr, nc, rs = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    if split_bytes < 0:
        raise ValueError("split_plan: split_bytes < 0")
    r = lib().avr_split_plan(d.ctypes.data, n, int(split_bytes), slots.ctypes.data, cap.ctypes.data, ctypes.byref(nr),
                             ctypes.byref(rs), ctypes.byref(nc))
    if r != AVR_OK:
        raise AvrError(r, "avr_split_plan failed")
    return SplitPlan(slots, cap, nr.value, rs.value, nc.value)


def seams_build(descs, arena, res, slots, cuts, piece_end, recs, rec_stride: int, check_cuts: bool = True):
    """The Block-field-16 bytes of the cut slices of a split compress batch from what was read back
    from the device (avr_seams_build): (status int32[n], [bytes per slice, b"" without a cut or with
    status != 0]).  descs / arena: the host descriptors and payloads; res SLICE_RESULT[n]; slots
    SPLIT_SLOT[n]; cuts uint32[n]; piece_end uint32[n_recs]; recs: n_recs records of rec_stride bytes.
    check_cuts: a cut whose re-encoder state is not the host's restatement gives its slice
    SLICE_CODER.  Raises AvrError(-1) for arrays that do not fit each other.  Host only."""
    d = np.ascontiguousarray(descs, dtype=SLICE_DESC)
    n = len(d)
    rs = np.ascontiguousarray(res, dtype=SLICE_RESULT)
    sl = np.ascontiguousarray(slots, dtype=SPLIT_SLOT)
    cu = np.ascontiguousarray(cuts, dtype=np.uint32)
    pe = np.ascontiguousarray(piece_end, dtype=np.uint32)
    rc = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
    ar = np.ascontiguousarray(arena, dtype=np.uint8).reshape(-1)
    if not (len(rs) == len(sl) == len(cu) == n):
        raise ValueError("seams_build: one result / slot / cut count per descriptor")
    status = np.zeros(n, dtype=np.int32)
    offs = np.zeros(n, dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint32)
    blob, blen = ctypes.c_void_p(), ctypes.c_size_t()
    P = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    r = lib().avr_seams_build(P(d), n, ar.ctypes.data, ar.nbytes, P(rs), P(sl), P(cu), P(pe), len(pe), P(rc), rc.nbytes,
                              int(rec_stride), 1 if check_cuts else 0, P(status), ctypes.byref(blob),
                              ctypes.byref(blen), P(offs), P(lens))
    if r != AVR_OK:
        raise AvrError(r, "avr_seams_build failed")
    b = _take(blob, blen.value) if blob.value else b""
    return status, [b[int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)]


def assemble_container(data, status: np.ndarray, recoded, offsets: np.ndarray, lens: np.ndarray,
                       model: int = MODEL_PARALLEL, ps: "ParsedStream | None" = None, as_array: bool = False,
                       out: "np.ndarray | None" = None, seams=None, escaped: bool = False, split32: bool = False,
                       crcs=None, checksums: bool = False, unit_checksums: bool = False):
    """Recoded container from per-slice outputs gathered from the ranks (avr_assemble_container; with ps =
    parse_stream(data) already in hand, avr_assemble_container_parsed: no second parse).  recoded:
    bytes or a uint8 array.  model: the model / coder the outputs were made with (PARALLEL, PARALLEL32,
    or CHAINED for Context.compress_chain_range's outputs).  as_array: the container
    as a uint8 array over the library's buffer (no copy into bytes).  out (with ps): a uint8 array
    the container is written into (avr_assemble_container_into; container_bound() bytes suffice);
    returns the view of it that holds the container.  seams: (blob, offsets, lens) -- slice k's
    Block field 16 is blob[offsets[k] : offsets[k] + lens[k]], length 0 for none -- or a list of one
    bytes object per slice (b"" for none): the container of a split compress
    (avr_assemble_container_seams; MODEL_PARALLEL, or MODEL_PARALLEL32 with split32; not with out).
    escaped: the second search of
    Context.recode_escaped (avr_assemble_container_opts with ASSEMBLE_ESCAPED; the parallel models
    only, not with out), so that the result is what ctx.compress writes with the option on.
    split32 (ASSEMBLE_SPLIT32; MODEL_PARALLEL32 only, not with out): seams are allowed for that model
    and a container that holds one is tagged P32S / P32SE, what ctx.compress writes with
    Context.split_p32 on.
    checksums (ASSEMBLE_CRC; any model, not with out): a checked container, what ctx.compress writes
    with Context.checksums on (avr_assemble_container_args); crcs: the CRC-32 of every slice's payload
    as the ranks' devices computed them (read for coded slices; trusted), else the assembly computes
    them on host threads.
    unit_checksums (ASSEMBLE_UNIT_CRC; the parallel models, not with out): Block field 18 on every coded
    block, what ctx.compress writes with Context.unit_checksums on; the assembly computes the values on
    host threads from the payloads and the seams' cuts.  Host only."""
    L = lib()
    flags = (ASSEMBLE_ESCAPED if escaped else 0) | (ASSEMBLE_SPLIT32 if split32 else 0) | \
        (ASSEMBLE_UNIT_CRC if unit_checksums else 0)
    if (flags or checksums) and out is not None:
        raise ValueError("assemble_container: escaped / split32 / checksums / unit_checksums cannot be combined with out")
    p, n, keep = _buf(data)
    st = np.ascontiguousarray(status, dtype=np.int32)
    of = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    rp, rn, keep2 = _buf(recoded)
    res, olen = ctypes.c_void_p(), ctypes.c_size_t()
    if checksums or unit_checksums:
        a = _AssembleArgs()
        a.size, a.file, a.n, a.model, a.n_slices = ctypes.sizeof(_AssembleArgs), p, n, model, len(st)
        a.status, a.recoded, a.recoded_len, a.offsets, a.lens = st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data
        a.flags = flags | (ASSEMBLE_CRC if checksums else 0)
        if len(of) != len(st) or len(ln) != len(st):
            raise ValueError("assemble_container: status / offsets / lens need one entry per slice")
        if ps is not None:
            dd = np.ascontiguousarray(ps.descs)
            if len(dd) != len(st):
                raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
            a.descs, a.arena, a.arena_len = dd.ctypes.data, ps.arena.ctypes.data, ps.arena.nbytes
        if seams is not None:
            if isinstance(seams, list):
                sl = np.array([len(x) for x in seams], dtype=np.uint32)
                so = (np.cumsum(sl, dtype=np.uint64) - sl).astype(np.uint64)
                sb = b"".join(seams)
            else:
                sb, so, sl = seams
                so = np.ascontiguousarray(so, dtype=np.uint64)
                sl = np.ascontiguousarray(sl, dtype=np.uint32)
            if len(so) != len(st) or len(sl) != len(st):
                raise ValueError("assemble_container: seams need one entry per slice")
            sp, sn, keep3 = _buf(sb)
            a.seams, a.seams_len, a.seam_offsets, a.seam_lens = sp, sn, so.ctypes.data, sl.ctypes.data
        if crcs is not None:
            cr = np.ascontiguousarray(crcs, dtype=np.uint32)
            if len(cr) != len(st):
                raise ValueError("assemble_container: crcs need one entry per slice")
            a.crcs = cr.ctypes.data
        r = L.avr_assemble_container_args(ctypes.byref(a), ctypes.byref(res), ctypes.byref(olen))
        if r != AVR_OK:
            raise AvrError(r, "avr_assemble_container_args failed")
        return _take_array(res, olen.value) if as_array else _take(res, olen.value)
    if seams is not None:
        if out is not None:
            raise ValueError("assemble_container: seams cannot be combined with out")
        if isinstance(seams, list):
            sl = np.array([len(s) for s in seams], dtype=np.uint32)
            so = (np.cumsum(sl, dtype=np.uint64) - sl).astype(np.uint64)
            sb = b"".join(seams)
        else:
            sb, so, sl = seams
            so = np.ascontiguousarray(so, dtype=np.uint64)
            sl = np.ascontiguousarray(sl, dtype=np.uint32)
        if len(so) != len(st) or len(sl) != len(st) or len(of) != len(st) or len(ln) != len(st):
            raise ValueError("assemble_container: status / offsets / lens / seams need one entry per slice")
        sp, sn, keep3 = _buf(sb)
        if flags:
            dd = np.ascontiguousarray(ps.descs) if ps is not None else None
            if dd is not None and len(dd) != len(st):
                raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
            r = L.avr_assemble_container_opts(p, n, model, dd.ctypes.data if dd is not None else None, len(st),
                                              ps.arena.ctypes.data if ps is not None else None,
                                              ps.arena.nbytes if ps is not None else 0, st.ctypes.data, rp, rn,
                                              of.ctypes.data, ln.ctypes.data, sp, sn, so.ctypes.data, sl.ctypes.data,
                                              flags, ctypes.byref(res), ctypes.byref(olen))
        elif ps is not None:
            dd = np.ascontiguousarray(ps.descs)
            if len(dd) != len(st):
                raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
            r = L.avr_assemble_container_seams_parsed(p, n, model, dd.ctypes.data, len(dd), ps.arena.ctypes.data,
                                                      ps.arena.nbytes, st.ctypes.data, rp, rn, of.ctypes.data,
                                                      ln.ctypes.data, sp, sn, so.ctypes.data, sl.ctypes.data,
                                                      ctypes.byref(res), ctypes.byref(olen))
        else:
            r = L.avr_assemble_container_seams(p, n, model, len(st), st.ctypes.data, rp, rn, of.ctypes.data,
                                               ln.ctypes.data, sp, sn, so.ctypes.data, sl.ctypes.data,
                                               ctypes.byref(res), ctypes.byref(olen))
        if r != AVR_OK:
            raise AvrError(r, "avr_assemble_container_seams failed")
        return _take_array(res, olen.value) if as_array else _take(res, olen.value)
    if out is not None:
        if ps is None or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("assemble_container: out needs ps and a contiguous uint8 array")
        dd = np.ascontiguousarray(ps.descs)
        if len(dd) != len(st) or len(of) != len(st) or len(ln) != len(st):
            raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
        r = L.avr_assemble_container_into(p, n, model, dd.ctypes.data, len(dd), ps.arena.ctypes.data, ps.arena.nbytes,
                                          st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data, out.ctypes.data,
                                          out.nbytes, ctypes.byref(olen))
        if r != AVR_OK:
            raise AvrError(r, f"avr_assemble_container_into failed (container {olen.value} B, buffer {out.nbytes} B)")
        return out[:olen.value]
    if flags:
        dd = np.ascontiguousarray(ps.descs) if ps is not None else None
        if len(of) != len(st) or len(ln) != len(st) or (dd is not None and len(dd) != len(st)):
            raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
        r = L.avr_assemble_container_opts(p, n, model, dd.ctypes.data if dd is not None else None, len(st),
                                          ps.arena.ctypes.data if ps is not None else None,
                                          ps.arena.nbytes if ps is not None else 0, st.ctypes.data, rp, rn,
                                          of.ctypes.data, ln.ctypes.data, None, 0, None, None, flags,
                                          ctypes.byref(res), ctypes.byref(olen))
    elif ps is not None:
        dd = np.ascontiguousarray(ps.descs)
        if len(dd) != len(st) or len(of) != len(st) or len(ln) != len(st):
            raise ValueError("assemble_container: status / offsets / lens need one entry per parsed slice")
        r = L.avr_assemble_container_parsed(p, n, model, dd.ctypes.data, len(dd), ps.arena.ctypes.data, ps.arena.nbytes,
                                            st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data, ctypes.byref(res),
                                            ctypes.byref(olen))
    else:
        r = L.avr_assemble_container(p, n, model, len(st), st.ctypes.data, rp, rn, of.ctypes.data, ln.ctypes.data,
                                     ctypes.byref(res), ctypes.byref(olen))
    if r != AVR_OK:
        raise AvrError(r, "avr_assemble_container failed")
    return _take_array(res, olen.value) if as_array else _take(res, olen.value)


def _varint(b, i: int) -> tuple[int, int]:
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def seams_of_container(avrc) -> list:
    """The parallel model's long-slice split in a container: (block index, seams field bytes) of every
    coded block that was cut (Block field 16, include/avrecode.h avr_set_split_bytes).  A plain walk
    of the wire format (host only, no library call)."""
    b = memoryview(bytes(avrc))
    out, i, k = [], 0, 0
    while i < len(b):
        tag, i = _varint(b, i)
        wt = tag & 7
        if wt == 0:
            _, i = _varint(b, i)
            continue
        if wt != 2:
            raise ValueError("not a Recoded message")
        n, i = _varint(b, i)
        if tag >> 3 == 2:   # a Block: look for field 16
            j, e = i, i + n
            while j < e:
                t2, j = _varint(b, j)
                if t2 & 7 == 0:
                    _, j = _varint(b, j)
                    continue
                l2, j = _varint(b, j)
                if t2 >> 3 == 16:
                    out.append((k, l2))
                j += l2
            k += 1
        i += n
    return out


def file_crc_of_container(avrc) -> "int | None":
    """The file's CRC-32 a checked container carries (Recoded.Metadata field 16), or None: a walk over
    the top-level fields that reads the Metadata only (no block's bytes).  Host only."""
    b = memoryview(avrc) if not isinstance(avrc, np.ndarray) else memoryview(np.ascontiguousarray(avrc).view(np.uint8))
    i, n = 0, len(b)
    while i < n:
        tag, i = _varint(b, i)
        if tag & 7 != 2:
            return None   # the writer's containers hold length-delimited fields only
        ln, i = _varint(b, i)
        if tag >> 3 == 1:
            j, e = i, i + ln
            while j < e:
                t2, j = _varint(b, j)
                if t2 == (16 << 3 | 5):
                    return int.from_bytes(bytes(b[j:j + 4]), "little")
                if t2 & 7 == 2:
                    l2, j = _varint(b, j)
                    j += l2
                elif t2 & 7 == 0:
                    _, j = _varint(b, j)
                else:
                    j += 4 if t2 & 7 == 5 else 8
        i += ln
    return None


def describe_container(avrc) -> tuple[dict, bytes]:
    """Parse a Recoded protobuf with the library's wire codec (avr_container_describe): its fields
    (hex strings for bytes) and the message re-serialised by the library's writer.  Host only."""
    import json
    L = lib()
    p, n, keep = _buf(avrc)
    js, out, olen = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    r = L.avr_container_describe(p, n, ctypes.byref(js), ctypes.byref(out), ctypes.byref(olen))
    if r != AVR_OK:
        raise AvrError(r, "avr_container_describe failed")
    text = ctypes.string_at(js.value).decode()
    L.avr_free(js)
    return json.loads(text), _take(out, olen.value)


def escape_payload(payload) -> bytes:
    """escape(payload): H.264 7.4.1 from a clean state, the library's own (avr_escape_payload) -- a
    03 before any byte <= 3 that follows two zero bytes since the last insertion.  Host only."""
    L = lib()
    p, n, keep = _buf(payload)
    out = np.empty(n + n // 2 + 1, dtype=np.uint8)
    olen = ctypes.c_size_t()
    r = L.avr_escape_payload(p, n, out.ctypes.data, out.nbytes, ctypes.byref(olen))
    if r != AVR_OK:
        raise AvrError(r, "avr_escape_payload failed")
    return out[:olen.value].tobytes()


def neighbor_tables(ctx=None) -> tuple[bytes, bytes]:
    """(nb_left[48], nb_up[48]): the model's neighbour geometry as the kernels use it
    (avr_neighbor_tables).  ctx None: the host-built table (no GPU); a Context: its device copy."""
    L = lib()
    out = ctypes.create_string_buffer(96)
    r = L.avr_neighbor_tables(ctx._h if ctx is not None else None, out)
    if r != AVR_OK:
        raise AvrError(r, "avr_neighbor_tables failed")
    return out.raw[:48], out.raw[48:96]


class Context:
    """One device context (avr_ctx).  Raises AvrError(AVR_ERR_DEVICE) when no GPU is usable."""

    def __init__(self, device: int = 0):
        L = lib()
        h = ctypes.c_void_p()
        r = L.avr_create(int(device), ctypes.byref(h))
        if r != AVR_OK:
            raise AvrError(r, f"avr_create(device={device}) failed (no usable GPU? the hot path has no CPU path)")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().avr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, r: int, what: str):
        if r != AVR_OK:
            raise AvrError(r, f"{what}: {lib().avr_last_error(self._h).decode(errors='replace')}")

    @property
    def split_bytes(self) -> int:
        """The parallel model's long-slice split (avr_set_split_bytes; 0: none): the whole-file
        compress cuts a progressive slice into pieces of about this many payload bytes."""
        return int(lib().avr_get_split_bytes(self._h))

    @split_bytes.setter
    def split_bytes(self, v: int):
        self._check(lib().avr_set_split_bytes(self._h, int(v)), "avr_set_split_bytes")

    @property
    def split_p32(self) -> bool:
        """The long-slice split for MODEL_PARALLEL32 (avr_set_split_p32; default off, or the
        environment's AVR_SPLIT_P32): with it the whole-file compress and roundtrip of that model read
        split_bytes as MODEL_PARALLEL's do, and a container that holds a cut slice is tagged
        avrecode-amd:P32S (P32SE with recode_escaped's field as well).  Reading needs no option."""
        return bool(lib().avr_get_split_p32(self._h))

    @split_p32.setter
    def split_p32(self, on: bool):
        self._check(lib().avr_set_split_p32(self._h, 1 if on else 0), "avr_set_split_p32")

    @property
    def recode_escaped(self) -> bool:
        """Re-code slices whose NAL unit carries emulation-prevention bytes (avr_set_recode_escaped;
        default off, or the environment's AVR_RECODE_ESCAPED): read by compress / roundtrip of the
        parallel models, whose containers then carry Block field 17 and an "E" tag."""
        return bool(lib().avr_get_recode_escaped(self._h))

    @recode_escaped.setter
    def recode_escaped(self, on: bool):
        self._check(lib().avr_set_recode_escaped(self._h, 1 if on else 0), "avr_set_recode_escaped")

    # ------------------------------------------------------------------ whole files
    @property
    def checksums(self) -> bool:
        """Checked containers (avr_set_checksums; default: AVR_CHECKSUMS, else off): compress and
        roundtrip of every model write the file's CRC-32 (zlib.crc32) into Recoded.Metadata field 16,
        6 bytes (8 for the reference model), folded from per-slice CRCs the device computes.  Reading
        needs no option: every decompress of a container that has the field checks it and raises
        AvrError with code ERR_CHECKSUM on a mismatch."""
        return bool(lib().avr_get_checksums(self._h))

    @checksums.setter
    def checksums(self, on: bool):
        self._check(lib().avr_set_checksums(self._h, 1 if on else 0), "avr_set_checksums")

    @property
    def unit_checksums(self) -> bool:
        """Unit checksums (avr_set_unit_checksums; default: AVR_UNIT_CHECKSUMS, else off): compress and
        roundtrip of the parallel models write one CRC-32 per unit -- a whole coded slice, or each piece
        of a cut one -- into Block field 18 (7 bytes per uncut block), from CRCs the device computes
        over the payloads.  Reading needs no option: a Reader checks the units a read touches
        (AvrError ERR_CHECKSUM naming the unit; reads that avoid it succeed), every whole-file
        decompress each block."""
        return bool(lib().avr_get_unit_checksums(self._h))

    @unit_checksums.setter
    def unit_checksums(self, on: bool):
        self._check(lib().avr_set_unit_checksums(self._h, 1 if on else 0), "avr_set_unit_checksums")

    def check_units(self, d_tails, d_checks, d_res, n, d_src, src_len, d_status, stream=None):
        """avr_check_units: after range_tails on the same stream, unit k's share of its slice (RANGE_TAIL
        and SLICE_RESULT rows) at d_src + d_checks[k].src_off (UNIT_CHECK rows) CRC'd by one workgroup,
        the last-byte rule applied to the value, and compared with d_checks[k].crc: d_status[k] becomes
        SLICE_CHECKSUM on a mismatch, SLICE_OVERFLOW for a span outside src_len; units with a non-zero
        status or have = 0 are left alone."""
        P = self._ptr
        self._check(lib().avr_check_units(self._h, P(d_tails), P(d_checks), P(d_res), int(n), P(d_src), int(src_len),
                                          P(d_status), self._stream(stream)), "check_units")

    def crc_spans(self, d_buf, buf_len, d_off, d_len, n, d_crc, d_status, stream=None):
        """d_crc[k] = the CRC-32 of d_buf[d_off[k] : d_off[k] + d_len[k]] (avr_crc_spans: one workgroup
        per span, device tensors, nothing synchronised); d_status[k] = SLICE_OVERFLOW for a span outside
        buf_len."""
        self._check(lib().avr_crc_spans(self._h, self._ptr(d_buf), int(buf_len), self._ptr(d_off), self._ptr(d_len),
                                        int(n), self._ptr(d_crc), self._ptr(d_status), self._stream(stream)),
                    "avr_crc_spans")

    def compress(self, data, model: int = MODEL_REFERENCE) -> bytes:
        p, n, keep = _buf(data)
        out, olen = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().avr_compress_file(self._h, p, n, model, ctypes.byref(out), ctypes.byref(olen)),
                    "compress")
        return _take(out, olen.value)

    def decompress(self, data) -> bytes:
        p, n, keep = _buf(data)
        out, olen = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().avr_decompress_file(self._h, p, n, ctypes.byref(out), ctypes.byref(olen)), "decompress")
        return _take(out, olen.value)

    def roundtrip(self, data, model: int = MODEL_REFERENCE) -> tuple[bytes, dict]:
        p, n, keep = _buf(data)
        out, olen = ctypes.c_void_p(), ctypes.c_size_t()
        st = _FileStats()
        self._check(lib().avr_roundtrip_file(self._h, p, n, model, ctypes.byref(out), ctypes.byref(olen),
                                             ctypes.byref(st)), "roundtrip")
        stats = {f: getattr(st, f) for f, _ in _FileStats._fields_ if f != "reserved"}
        for f in ("compress_phases", "decompress_phases"):
            stats[f] = _phases(stats[f])
        for f in ("bill", "cabac_bill"):   # by CodingType name, nonzero entries (~h264_model's print)
            stats[f] = {CODING_TYPES[i]: int(v) for i, v in enumerate(stats[f]) if v}
        return _take(out, olen.value), stats

    def _files(self, fn, datas, *extra, tail=()):
        n = len(datas)
        keep = [_buf(d) for d in datas]
        ptrs = (ctypes.c_void_p * max(1, n))(*[k[0].value for k in keep])
        lens = (ctypes.c_size_t * max(1, n))(*[k[1] for k in keep])
        outs = (ctypes.c_void_p * max(1, n))()
        olens = (ctypes.c_size_t * max(1, n))()
        st = (ctypes.c_int32 * max(1, n))()
        self._check(fn(self._h, n, ptrs, lens, *extra, outs, olens, st, *tail), fn.__name__)
        res = []
        failed = [k for k in range(n) if st[k] != AVR_OK]
        # the context keeps one error message: it belongs to a failed file only when there is one
        detail = lib().avr_last_error(self._h).decode(errors="replace") if len(failed) == 1 else ""
        for k in range(n):
            if st[k] != AVR_OK:
                res.append(AvrError(st[k], f"file {k}" + (f": {detail}" if detail else "")))
            else:
                res.append(_take(ctypes.c_void_p(outs[k]), olens[k]))
        del keep
        return res

    def last_phase_times(self) -> dict:
        """avr_last_phase_times: where the last whole-file call's wall time went (seconds)."""
        p = _PhaseTimes()
        self._check(lib().avr_last_phase_times(self._h, ctypes.byref(p)), "avr_last_phase_times")
        return _phases(p)

    def compress_files(self, datas, model: int = MODEL_REFERENCE) -> list:
        """avr_compress_files: one container (bytes) or AvrError per input file."""
        return self._files(lib().avr_compress_files, datas, model)

    def decompress_files(self, datas) -> list:
        """avr_decompress_files: the original file (bytes) or AvrError per container."""
        return self._files(lib().avr_decompress_files, datas)

    def roundtrip_files(self, datas, model: int = MODEL_REFERENCE) -> tuple[list, dict]:
        """avr_roundtrip_files: (one container (bytes) or AvrError per input file, {"compress_s",
        "decompress_s"}: wall seconds of the batched compress and decompress calls)."""
        times = (ctypes.c_double * 2)()
        res = self._files(lib().avr_roundtrip_files, datas, model, tail=(times,))
        return res, {"compress_s": times[0], "decompress_s": times[1]}

    # ------------------------------------------------------- device-resident slice batches
    # All tensor arguments are torch tensors on this context's device (uint8 buffers, and uint8
    # views of descriptor/result arrays); `stream` is a torch.cuda.Stream or None (= its current).
    @staticmethod
    def _ptr(t) -> ctypes.c_void_p:
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()

    @staticmethod
    def _stream(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def compress_slices(self, d_desc, n, max_w, max_h, d_in, d_out, d_res, model=MODEL_PARALLEL, stream=None):
        self._check(lib().avr_compress_slices(self._h, self._ptr(d_desc), n, max_w, max_h, self._ptr(d_in),
                                              self._ptr(d_out), self._ptr(d_res), model, self._stream(stream)),
                    "compress_slices")

    def decompress_slices(self, d_desc, n, max_w, max_h, d_in, d_out, d_res, model=MODEL_PARALLEL, stream=None):
        self._check(lib().avr_decompress_slices(self._h, self._ptr(d_desc), n, max_w, max_h, self._ptr(d_in),
                                                self._ptr(d_out), self._ptr(d_res), model, self._stream(stream)),
                    "decompress_slices")

    def roundtrip_slices(self, d_desc, n, max_w, max_h, d_in, d_work, d_regen, d_dec_desc, d_res_c, d_res_d,
                         d_verdict, model=MODEL_PARALLEL, stream=None):
        P = self._ptr
        self._check(lib().avr_roundtrip_slices(self._h, P(d_desc), n, max_w, max_h, P(d_in), P(d_work), P(d_regen),
                                               P(d_dec_desc), P(d_res_c), P(d_res_d), P(d_verdict), model,
                                               self._stream(stream)), "roundtrip_slices")

    def derive_decompress_descs(self, d_desc, d_res_c, n, d_dec_desc, stream=None):
        P = self._ptr
        self._check(lib().avr_derive_decompress_descs(self._h, P(d_desc), P(d_res_c), n, P(d_dec_desc),
                                                      self._stream(stream)), "derive_decompress_descs")

    def verify_slices(self, d_desc, d_res_c, d_res_d, n, d_in, d_regen, d_verdict, stream=None):
        P = self._ptr
        self._check(lib().avr_verify_slices(self._h, P(d_desc), P(d_res_c), P(d_res_d), n, P(d_in), P(d_regen),
                                            P(d_verdict), self._stream(stream)), "verify_slices")

    def _chain_range(self, fn, name, data, world: int, rank: int):
        p, n, keep = _buf(data)
        lo, hi = ctypes.c_int(), ctypes.c_int()
        st, blob, offs, lens = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        blen = ctypes.c_size_t()
        r = fn(self._h, p, n, world, rank, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(st), ctypes.byref(blob),
               ctypes.byref(blen), ctypes.byref(offs), ctypes.byref(lens))
        del keep
        self._check(r, name)
        k = hi.value - lo.value
        return (lo.value, hi.value, _take_array(st, 4 * k).view(np.int32), _take_array(blob, blen.value),
                _take_array(offs, 8 * k).view(np.uint64), _take_array(lens, 4 * k).view(np.uint32))

    def compress_chain_range(self, data, world: int, rank: int):
        """This rank's chains of a chained-model compress of one file (avr_compress_chain_range):
        (lo, hi, status int32, recoded uint8, offsets uint64, lens uint32) for the file's slices
        [lo, hi); status 0 coded, -1 not coded, -2 failed (compress the file whole)."""
        return self._chain_range(lib().avr_compress_chain_range, "compress_chain_range", data, world, rank)

    def decompress_chain_range(self, avrc, world: int, rank: int):
        """This rank's chains of a chained- (or reference-) model container
        (avr_decompress_chain_range): (lo, hi, status, regen, offsets, lens) for the plan's slices
        [lo, hi); status 0 regenerated, 1 not coded, < 0 failed."""
        return self._chain_range(lib().avr_decompress_chain_range, "decompress_chain_range", avrc, world, rank)

    def slice_kernel(self, n: int, max_mb_width: int, decompress: bool, p32: bool = False) -> str:
        """The kernel a parallel-model batch of n slices runs (avr_slice_kernel), named as rocprofv3
        reports it: slices_parallel_kernel (resident) or slices_queue_kernel (persistent queue),
        template <MODE, FLD = false, P32>."""
        k = ctypes.c_int(-1)
        self._check(lib().avr_slice_kernel(self._h, 1 if decompress else 0, n, max_mb_width, ctypes.byref(k)),
                    "slice_kernel")
        name = ("slices_parallel_kernel", "slices_queue_kernel")[k.value]
        return f"{name}<{1 if decompress else 0}, false, {'true' if p32 else 'false'}>"

    def decompress_pieces(self, d_desc, pieces, n, max_w, max_h, d_recs, n_recs, rec_stride, d_in, d_out, d_res,
                          stream=None, model: int = MODEL_PARALLEL):
        """avr_decompress_pieces_m: a batch of pieces and whole progressive slices of model
        (MODEL_PARALLEL or MODEL_PARALLEL32: one call runs one coder), one
        workgroup per unit.  pieces: the units' PIECE array on the HOST (checked there before the
        launch); d_recs: the n_recs seam records its seam fields index, on the device."""
        pc = np.ascontiguousarray(pieces, dtype=PIECE)
        if len(pc) != n:
            raise ValueError("decompress_pieces: one PIECE per unit")
        self._check(lib().avr_decompress_pieces_m(self._h, int(model), self._ptr(d_desc), pc.ctypes.data, n, max_w,
                                                  max_h, self._ptr(d_recs), n_recs, rec_stride, self._ptr(d_in),
                                                  self._ptr(d_out), self._ptr(d_res), self._stream(stream)),
                    "decompress_pieces")

    def pack_pieces(self, d_desc, d_pieces, d_res, n, d_out, d_packed, d_offsets, d_kept, d_status, stream=None):
        """avr_pack_pieces: every unit's kept bytes packed at d_offsets[k] (n + 1 entries, the prefix
        sum of d_kept); d_status[k] the unit's status, SLICE_NO_END when it came out short of keep."""
        P = self._ptr
        self._check(lib().avr_pack_pieces(self._h, P(d_desc), P(d_pieces), P(d_res), n, P(d_out), P(d_packed),
                                          P(d_offsets), P(d_kept), P(d_status), self._stream(stream)), "pack_pieces")

    def gather_spans(self, d_spans, n, d_src, src_len, d_dst, dst_len, d_status, stream=None):
        """avr_gather_spans: span k (SPAN rows on the device) copies len bytes from d_src + src_off to
        d_dst + dst_off, one workgroup per span, any alignment; d_status[k] SLICE_OVERFLOW for a span
        outside src_len or dst_len (nothing of it read or written)."""
        P = self._ptr
        self._check(lib().avr_gather_spans(self._h, P(d_spans), int(n), P(d_src), int(src_len), P(d_dst), int(dst_len),
                                           P(d_status), self._stream(stream)), "gather_spans")

    def range_tails(self, d_tails, d_res, n, d_dst, dst_len, d_status, stream=None):
        """avr_range_tails: after gather_spans on the same stream, unit k's SLICE_RESULT checked against
        its RANGE_TAIL row (d_status[k]: the unit's status, SLICE_NO_END for a short piece or a slice
        of the wrong length) and the last-byte rule applied at final_pos."""
        P = self._ptr
        self._check(lib().avr_range_tails(self._h, P(d_tails), P(d_res), int(n), P(d_dst), int(dst_len), P(d_status),
                                          self._stream(stream)), "range_tails")

    # the split compress of slice batches (ABI 8); the two host steps need no context
    split_plan = staticmethod(split_plan)
    seams_build = staticmethod(seams_build)

    def compress_split_slices(self, d_desc, n, max_w, max_h, d_in, d_out, d_res, slots, split_bytes, d_recs, n_recs,
                              rec_stride, d_cuts, d_piece_end, stream=None, model: int = MODEL_PARALLEL):
        """avr_compress_split_slices_m: the split walk over a batch of progressive slices re-coded with
        model's coder (MODEL_PARALLEL or MODEL_PARALLEL32), each cut as it is walked.  slots: split_plan's SPLIT_SLOT array on the HOST (checked there
        before the launch); d_recs / d_cuts (uint32[n]) / d_piece_end (uint32[n_recs]): what the walk
        writes, on the device, the latter two zeroed on the stream first."""
        sl = np.ascontiguousarray(slots, dtype=SPLIT_SLOT)
        if len(sl) != n:
            raise ValueError("compress_split_slices: one SPLIT_SLOT per slice")
        P = self._ptr
        self._check(lib().avr_compress_split_slices_m(self._h, int(model), P(d_desc), n, max_w, max_h, P(d_in),
                                                      P(d_out), P(d_res), sl.ctypes.data, int(split_bytes),
                                                      P(d_recs), n_recs, rec_stride, P(d_cuts), P(d_piece_end),
                                                      self._stream(stream)),
                    "compress_split_slices")

    def stage_pieces(self, d_desc, d_src, n, d_out, out_len, d_arena, arena_cap, d_offsets, d_status, stream=None):
        """avr_stage_pieces: unit k's stream (d_desc[k].payload_size bytes at d_out + d_src[k], any
        alignment) copied to d_arena + d_offsets[k], 16-byte aligned with at least 16 zero bytes
        after it; d_desc[k].payload_offset / read_limit set; d_status[k] SLICE_OVERFLOW when it does
        not fit out_len / arena_cap."""
        P = self._ptr
        self._check(lib().avr_stage_pieces(self._h, P(d_desc), P(d_src), n, P(d_out), int(out_len), P(d_arena),
                                           int(arena_cap), P(d_offsets), P(d_status), self._stream(stream)),
                    "stage_pieces")

    def verify_units(self, d_desc, d_res_c, n, d_first, n_units, d_in, d_packed, d_offsets, d_kept, d_unit_status,
                     d_verdict, stream=None):
        """avr_verify_units: d_verdict[k] (1 bit-exact, 0 mismatch, 2 not coded) of slice k from the
        packed kept bytes of its units [d_first[k], d_first[k + 1]) (pack_pieces' outputs) against its
        payload in d_in, under the last-byte rule."""
        P = self._ptr
        self._check(lib().avr_verify_units(self._h, P(d_desc), P(d_res_c), n, P(d_first), n_units, P(d_in), P(d_packed),
                                           P(d_offsets), P(d_kept), P(d_unit_status), P(d_verdict),
                                           self._stream(stream)), "verify_units")

    def pack_outputs(self, d_desc, d_res, n, d_out, d_packed, d_offsets, stream=None):
        P = self._ptr
        self._check(lib().avr_pack_outputs(self._h, P(d_desc), P(d_res), n, P(d_out), P(d_packed), P(d_offsets),
                                           self._stream(stream)), "pack_outputs")

    # ------------------------------------------------------------------ synthetic input
    def synthesize(self, params: SynthParams, n: int) -> bytes:
        sp = _SynthParams(params.mb_width, params.mb_height, params.slice_type, params.slice_qp,
                          params.chroma_format_idc, params.transform_8x8_mode, params.num_ref_idx_l0,
                          params.num_ref_idx_l1, params.seed, params.slices_per_picture, params.gop_length,
                          params.repeat, params.structure)
        out, olen = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(lib().avr_synthesize_stream(self._h, ctypes.byref(sp), int(n), ctypes.byref(out),
                                                ctypes.byref(olen)), "synthesize")
        return _take(out, olen.value)


class Reader:
    """An opened container that serves byte ranges of its file (avr_reader_*): pread semantics, the
    window clamped to the file.  In the parallel models' containers (info["random_access"]) a read
    regenerates only the slices and pieces its window touches; every other container is regenerated
    whole at the first read and served from host memory.  The container's bytes are kept alive by the
    reader.  A context manager; close() before the context closes."""

    def __init__(self, ctx: Context, avrc):
        self._ctx = ctx
        p, n, self._keep = _buf(avrc)
        self._h = ctypes.c_void_p()
        ctx._check(lib().avr_reader_open(ctx._h, p, n, ctypes.byref(self._h)), "avr_reader_open")
        i = _ReaderInfo()
        ctx._check(lib().avr_reader_info(self._h, ctypes.byref(i)), "avr_reader_info")
        self.info = {f: int(getattr(i, f)) for f, _ in _ReaderInfo._fields_}
        self.size = self.info["file_size"]

    def read(self, off: int, n: int) -> bytes:
        n = max(0, min(int(n), self.size - int(off))) if off < self.size else 0
        out = np.empty(max(1, n), dtype=np.uint8)
        got = ctypes.c_size_t()
        self._ctx._check(lib().avr_reader_read(self._h, int(off), n, out.ctypes.data, ctypes.byref(got)),
                         "avr_reader_read")
        return out[:got.value].tobytes()

    def read_into(self, dst, off: int, n: int) -> int:
        """The window into device memory (avr_reader_read_device): dst a torch uint8 tensor on the
        context's device with room for n bytes, or a device pointer (int).  Returns the bytes read."""
        if isinstance(dst, int):
            ptr = ctypes.c_void_p(dst)
        else:
            if dst.numel() * dst.element_size() < min(int(n), max(0, self.size - int(off))):
                raise ValueError("Reader.read_into: the tensor is smaller than the window")
            ptr = ctypes.c_void_p(dst.data_ptr())
        got = ctypes.c_size_t()
        self._ctx._check(lib().avr_reader_read_device(self._h, int(off), int(n), ptr, ctypes.byref(got)),
                         "avr_reader_read_device")
        return int(got.value)

    def span(self, off: int) -> "tuple[int, int, bool]":
        """(lo, hi, coded): the file bytes [lo, hi) of the block holding off."""
        lo, hi, coded = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        self._ctx._check(lib().avr_reader_span(self._h, int(off), ctypes.byref(lo), ctypes.byref(hi),
                                               ctypes.byref(coded)), "avr_reader_span")
        return int(lo.value), int(hi.value), bool(coded.value)

    @property
    def last(self) -> dict:
        """What the last successful read did (avr_reader_last): units regenerated, the pieces among them,
        regenerated / literal bytes, spans, and the read's phase times."""
        s = _ReadStats()
        self._ctx._check(lib().avr_reader_last(self._h, ctypes.byref(s)), "avr_reader_last")
        d = {f: int(getattr(s, f)) for f, _ in _ReadStats._fields_ if f != "phases"}
        d["phases"] = _phases(s.phases)
        return d

    def close(self):
        if getattr(self, "_h", None):
            lib().avr_reader_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

