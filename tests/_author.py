"""Authored streams (oracle/oracle_author.c, TEST INFRASTRUCTURE ONLY): H.264 streams the oracle writes
for the tests, at the extremes of the CABAC syntax that the x264 fixtures and the device generator never
reach -- cabac_init_idc 1 and 2, slice_qp 0 and 51, long level / mvd escapes, long mb_qp_delta,
ref_idx 31, near-all-skip slices -- and, in the forced specs, exactly at the walkers' accept bounds.

One table of named specs (SPECS, BOUNDS); `stream(name)` authors a spec (cached) and returns
(bytes, census dict).  tests/golden/authored.json pins every spec's sha256, size and census."""
import ctypes
from functools import lru_cache

from _oracle import lib

LEVELS, MOTION, SPARSE, MIXED, FORCED = range(5)
F_LEVEL, F_MVD, F_QPDELTA, F_REF = range(4)
MAX_SLICES, MAX_FORCED = 256, 8
QPS = (0, 51, 26, 13, 39, 5)
IDCS = (0, 1, 2)


class _Force(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("slice", "element", "nth", "length")]


class _Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("mb_width", "mb_height", "chroma_format_idc", "transform_8x8_mode", "structure", "num_ref_idx",
                 "pictures", "slices_per_picture", "with_i", "profile", "kmax_level", "kmax_mvd", "n_qp")] + [
        ("qp", ctypes.c_int32 * 8), ("n_idc", ctypes.c_int32), ("idc", ctypes.c_int32 * 4),
        ("n_forced", ctypes.c_int32),
        ("forced", _Force * MAX_FORCED), ("seed", ctypes.c_uint64)]


class _Slice(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("slice_type", "slice_qp", "cabac_init_idc", "first_mb", "structure", "refused")] + [
        ("payload_bytes", ctypes.c_uint32), ("bins", ctypes.c_uint32)]


class _Census(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in
                ("slices", "refused_slices", "mbs", "skipped_mbs", "payload_bytes", "emulation_bytes")] + [
        ("bins", ctypes.c_uint64), ("level_escapes", ctypes.c_uint32), ("level_len", ctypes.c_uint32 * 32),
        ("mvd_escapes", ctypes.c_uint32), ("mvd_k", ctypes.c_uint32 * 32), ("qp_delta_len", ctypes.c_uint32 * 104),
        ("ref_idx", ctypes.c_uint32 * 33), ("idc_used", (ctypes.c_uint32 * 3) * 2), ("qp_used", ctypes.c_uint32 * 52),
        ("slice", _Slice * MAX_SLICES)]


def _sparse(arr):
    """{index: count} of the nonzero entries (JSON keys are strings)."""
    return {str(i): int(v) for i, v in enumerate(arr) if v}


def author(mb_width, mb_height, profile, seed, *, chroma=1, t8=0, structure=0, refs=1, pictures=6, spp=1, with_i=1,
           kmax_level=15, kmax_mvd=21, qps=QPS, idcs=IDCS, forced=()):
    """Author one stream; returns (bytes, census dict).  forced: (slice, element, nth, length) tuples."""
    p = _Params(mb_width=mb_width, mb_height=mb_height, chroma_format_idc=chroma, transform_8x8_mode=t8,
                structure=structure, num_ref_idx=refs, pictures=pictures, slices_per_picture=spp, with_i=with_i,
                profile=profile, kmax_level=kmax_level, kmax_mvd=kmax_mvd, n_qp=len(qps), n_idc=len(idcs),
                n_forced=len(forced), seed=seed)
    p.qp[:len(qps)] = qps
    p.idc[:len(idcs)] = idcs
    for i, f in enumerate(forced):
        p.forced[i] = _Force(*f)
    L = lib()
    fn = L.avr_author_stream
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_Params), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                   ctypes.POINTER(_Census)]
    out, n, c = ctypes.c_void_p(), ctypes.c_size_t(), _Census()
    r = fn(ctypes.byref(p), ctypes.byref(out), ctypes.byref(n), ctypes.byref(c))
    if r != 0:
        raise RuntimeError(f"avr_author_stream failed ({r})")
    data = ctypes.string_at(out.value, n.value)
    ctypes.CDLL(None).free(ctypes.c_void_p(out.value))
    census = dict(
        slices=c.slices, refused_slices=c.refused_slices, mbs=c.mbs, skipped_mbs=c.skipped_mbs,
        payload_bytes=c.payload_bytes, emulation_bytes=c.emulation_bytes, bins=int(c.bins),
        level_escapes=c.level_escapes, level_len=_sparse(c.level_len), mvd_escapes=c.mvd_escapes,
        mvd_k=_sparse(c.mvd_k), qp_delta_len=_sparse(c.qp_delta_len), ref_idx=_sparse(c.ref_idx),
        idc_used={"P": list(c.idc_used[0]), "B": list(c.idc_used[1])}, qp_used=_sparse(c.qp_used),
        slice=[dict(slice_type=s.slice_type, slice_qp=s.slice_qp, cabac_init_idc=s.cabac_init_idc,
                    first_mb=s.first_mb, structure=s.structure, refused=s.refused, payload_bytes=s.payload_bytes,
                    bins=s.bins) for s in c.slice[:c.slices]])
    return data, census


# name -> (args, kwargs) of author().  The smallest shapes that still reach every coverage condition of
# tests/test_author_host.py; the seeds were chosen so that they hold and no NAL unit needs an
# emulation-prevention byte (except in `escaped`, which is made to need some).
SPECS = {
    # dense residual, level prefixes mostly past 14, suffix prefix lengths uniform in 0..15
    "levels420": ((8, 6, LEVELS, 1), dict(t8=1, spp=2, pictures=6)),
    "levels422": ((5, 4, LEVELS, 2), dict(chroma=2, t8=1, spp=2, pictures=6)),
    "levels444": ((5, 4, LEVELS, 3), dict(chroma=3, t8=1, spp=2, pictures=6)),
    # few skips, mvd prefixes mostly past 9, suffix order up to 24, ref_idx uniform in 0..31, long mb_qp_delta
    "motion": ((9, 5, MOTION, 4), dict(refs=32, with_i=0, pictures=13)),
    "motion_unaligned": ((9, 5, MOTION, 5), dict(refs=32, with_i=0, pictures=13, spp=2)),
    # ~98 % of the P / B macroblocks skipped: many bins per byte, a re-coded form larger than the slice.  192
    # macroblocks per slice, not fewer: a slice under 8 bytes is never coded (the reference's marker rule,
    # recode.cpp:27), and every slice here must be
    "sparse": ((32, 18, SPARSE, 100), dict(with_i=0, pictures=9, spp=3, refs=2)),
    "mixed": ((7, 5, MIXED, 7), dict(t8=1, refs=4, pictures=9, spp=2)),
    "levels_paff": ((6, 6, LEVELS, 8), dict(t8=1, structure=1, pictures=6)),
    "motion_paff": ((7, 6, MOTION, 9), dict(structure=3, refs=32, with_i=0, pictures=9)),
    "levels_mbaff": ((6, 6, LEVELS, 10), dict(t8=1, structure=2, pictures=6, spp=2)),
    "motion_mbaff": ((7, 6, MOTION, 11), dict(structure=2, refs=16, with_i=0, pictures=13)),
    "narrow": ((1, 4, MIXED, 103), dict(refs=3, pictures=12)),
    # as levels420, with a seed whose CABAC bytes hold a 00 00 0x: one slice's NAL unit carries an
    # emulation-prevention byte (about one seed in 250 does at this size)
    "escaped": ((8, 6, LEVELS, 760), dict(t8=1, spp=2, pictures=6)),
}
LEVEL_SPECS = ("levels420", "levels422", "levels444", "levels_paff", "levels_mbaff")
MOTION_SPECS = ("motion", "motion_unaligned", "motion_paff", "motion_mbaff")
FIELD_SPECS = ("levels_paff", "motion_paff", "levels_mbaff", "motion_mbaff")

# The walkers' accept bounds (oracle_walker.c / avr_walker.h): the unary prefix of a level escape's
# suffix up to 30 bins (else AVR_SLICE_BAD_LEVEL), an mvd escape's order up to 24 (BAD_MVD), mb_qp_delta up
# to 102 bins, ref_idx below 32.  One forced slice each, the first slice of a two-slice picture: the
# second slice of the picture is an ordinary one.
BOUNDS = {
    # exactly at the bounds: coded
    "bounds_accepted": ((6, 4, FORCED, 21), dict(
        t8=1, refs=4, pictures=4, spp=2, with_i=0,
        forced=((0, F_LEVEL, 2, 30), (2, F_MVD, 3, 21), (2, F_QPDELTA, 1, 102), (4, F_LEVEL, 5, 30),
                (4, F_MVD, 2, 21), (6, F_QPDELTA, 0, 102)))),
    # one past: the walk stops, the slice is stored as it is
    "bounds_refused": ((6, 4, FORCED, 22), dict(
        t8=1, refs=4, pictures=4, spp=2, with_i=0,
        forced=((0, F_LEVEL, 2, 31), (2, F_MVD, 3, 22), (4, F_QPDELTA, 1, 103), (6, F_LEVEL, 4, 31)))),
    # ref_idx 32 in a field macroblock of an MBAFF frame with 32 references (64 reference fields)
    "bounds_refused_mbaff": ((6, 4, FORCED, 23), dict(
        structure=2, refs=32, pictures=3, spp=2, with_i=0, forced=((2, F_REF, 2, 32), (4, F_MVD, 1, 22)))),
}


@lru_cache(None)
def stream(name):
    args, kw = (SPECS.get(name) or BOUNDS[name])
    return author(*args, **kw)


def pins():
    """{name: {sha256, size, census}} of every spec, as tests/golden/authored.json holds it."""
    import hashlib
    out = {}
    for name in list(SPECS) + list(BOUNDS):
        data, census = stream(name)
        out[name] = dict(sha256=hashlib.sha256(data).hexdigest(), size=len(data), census=census)
    return out


if __name__ == "__main__":   # python tests/_author.py: rewrite the pins after a deliberate change of the table
    import json
    from pathlib import Path
    path = Path(__file__).parent / "golden" / "authored.json"
    path.write_text(json.dumps(pins(), indent=1, sort_keys=True) + "\n")
    print(f"wrote {path}")
