"""Unit checksums (Context.unit_checksums, Block field 18, AVR_SLICE_CHECKSUM): the host side, CPU only.

* avr_assemble_container_args with AVR_ASSEMBLE_UNIT_CRC over the oracle's streams of realshort, plain
  and cut at 1024: every value is zlib.crc32 of the unit's share of the payload -- the shares cut here
  from the seams fields, never by the library -- the values combined per block are the payload's CRC,
  the container minus its field-18 bytes is the flag-0 container (the oracle's own), its growth is the
  documented cost, an older reader (the oracle) restores the file, and the protobuf runtime
  re-serialises it byte for byte;
* a malformed field 18 is AVR_ERR_FORMAT from avr_container_describe and from the plan loads;
* the control: one bit of Block.cabac (block 16, byte 1987 of the plain realshort container) decompresses
  on the oracle with status 0 to a file of the right length with three wrong bytes -- damage neither a
  unit status nor a length check can see;
* the plan path on those damaged bytes: avr_unit_checks_apply gives AVR_SLICE_CHECKSUM for that unit
  and for no other, avr_dec_plan_splice of the field-18 container AVR_ERR_CHECKSUM, with no Metadata
  field 16 anywhere; undamaged bytes pass, also piece by piece on the cut container and on cockatoo,
  where the rule keeps, replaces and appends; a stored value off by one fails."""
import ctypes
import os
import tempfile
import zlib
from functools import lru_cache

import numpy as np
import pytest

import _pb
from _oracle import ROOT, oracle_cli
from test_checksum_host import _flat, _oracle_decompress, _outputs, _regen, _rules, _splice, strip_crc
from test_piece_plan_host import _packed, expected_units

import avrecode_amd as avr
from avrecode_amd import shard

FIX = ROOT / "tests" / "fixtures"
ERR_INVALID, ERR_FORMAT, ERR_CHECKSUM = -1, -3, -7
KEEP_ALL = 0xFFFFFFFF
# the control flip, from a sweep of 216 single-bit flips over the 36 coded blocks of this container
FLIP_BLOCK, FLIP_BYTE, FLIP_CABAC_LEN, FLIP_SPAN, FLIP_WRONG = 16, 1987, 1990, (34109, 35989), (35985, 35986, 35987)


# ------------------------------------------------------------------ a wire codec of the test's own
def _varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def _enc(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _fields(b):
    """[(field, wire type, the field's whole bytes, its content)] of one message."""
    i, out = 0, []
    while i < len(b):
        t, j = _varint(b, i)
        f, w = t >> 3, t & 7
        if w == 0:
            _, e = _varint(b, j)
            c = b[j:e]
        elif w == 2:
            n, k = _varint(b, j)
            e = k + n
            c = b[k:e]
        else:
            assert w in (1, 5), w
            e = j + (8 if w == 1 else 4)
            c = b[j:e]
        out.append((f, w, b[i:e], c))
        i = e
    return out


def _ld(field, content):
    return _enc(field << 3 | 2) + _enc(len(content)) + content


def edit_blocks(avrc, fn):
    """The container with every Block rebuilt from fn(block index, its fields) -> list of field bytes."""
    out, k = b"", 0
    for f, w, raw, c in _fields(avrc):
        if f == 2 and w == 2:
            out += _ld(2, b"".join(fn(k, _fields(c))))
            k += 1
        else:
            out += raw
    return out


def strip_units(avrc):
    return edit_blocks(avrc, lambda k, fs: [raw for f, w, raw, c in fs if f != 18])


def unit_cost(avrc):
    """What field 18 adds to the container: 4 m + 3 bytes per coded block (4 m + 4 past 31 units), and
    a byte of a Block's own length prefix where the field carries it over 127 or 16383."""
    cost = grown = 0
    for f, w, raw, c in _fields(avrc):
        if f != 2:
            continue
        units = [x for x in _fields(c) if x[0] == 18]
        for _, _, uraw, uc in units:
            m = len(uc) // 4
            assert len(uraw) == (4 * m + 3 if m <= 31 else 4 * m + 4)
            cost += len(uraw)
            grown += len(_enc(len(c))) - len(_enc(len(c) - len(uraw)))
    return cost, grown


# ------------------------------------------------------------------ the oracle's streams
@lru_cache(None)
def _streams(name, split_bytes):
    """(file, the oracle's container, per parsed slice: status, re-coded stream, seams field)."""
    data = (FIX / name).read_bytes()
    avrc = oracle_cli("compress", FIX / name, mode="P", split_bytes=split_bytes)
    nl = [b for b in avr.describe_container(avrc)[0]["blocks"] if "literal" not in b]
    st = np.array([0 if "cabac" in b else -1 for b in nl], np.int32)
    blobs = [bytes.fromhex(b.get("cabac", "")) for b in nl]
    seams = [bytes.fromhex(b.get("seams", "")) for b in nl]
    assert len(st) == len(avr.parse_stream(data).descs)
    return data, avrc, st, blobs, seams


def _assemble(name, split_bytes, **kw):
    data, _, st, blobs, seams = _streams(name, split_bytes)
    blob, offs, lens = _flat(blobs)
    return avr.assemble_container(data, st, blob, offs, lens, model=avr.MODEL_PARALLEL,
                                  seams=seams if split_bytes else None, **kw)


@lru_cache(None)
def _unit_checked(name="realshort.mp4", split_bytes=0):
    return _assemble(name, split_bytes, unit_checksums=True)


def _coded(avrc):
    return [b for b in avr.describe_container(avrc)[0]["blocks"] if "cabac" in b]


# ------------------------------------------------------------------ writing
@pytest.mark.parametrize("split_bytes", [0, 1024], ids=["plain", "cut1024"])
def test_assembly_writes_every_units_crc(split_bytes):
    data, oracle_avrc, st, blobs, seams = _streams("realshort.mp4", split_bytes)
    plain = _assemble("realshort.mp4", split_bytes)
    assert plain == oracle_avrc
    avrc = _unit_checked("realshort.mp4", split_bytes)
    info, again = avr.describe_container(avrc)
    assert again == avrc   # the re-serialisation keeps the field
    assert all("unit_crcs" not in b for b in avr.describe_container(plain)[0]["blocks"])
    # the units' shares of the payloads, cut by the test from the seams fields
    n_slices, units, _ = expected_units(data, avrc, _streams("realshort.mp4", 0)[1])
    coded = _coded(avrc)
    assert len(coded) == n_slices == 36 and all("unit_crcs" in b for b in coded)
    assert all("unit_crcs" not in b for b in info["blocks"] if "cabac" not in b)
    values = [v for b in coded for v in b["unit_crcs"]]
    assert len(values) == len(units) == (77 if split_bytes else 36)
    assert values == [zlib.crc32(u["true"]) for u in units]
    for s, b in enumerate(coded):   # the invariant: combined in order they are the payload's CRC
        mine = [u["true"] for u in units if u["slice"] == s]
        assert len(mine) == len(b["unit_crcs"]) == (len(mine) if "seams" in b else 1)
        crc = 0
        for v, t in zip(b["unit_crcs"], mine):
            crc = avr.crc32_combine(crc, v, len(t))
        assert crc == zlib.crc32(b"".join(mine)) and len(b"".join(mine)) == b["size"]
    # additive: minus the field it is the flag-0 container, and it costs what the header says
    assert strip_units(avrc) == plain
    cost, grown = unit_cost(avrc)
    assert cost == sum(4 * len(b["unit_crcs"]) + 3 for b in coded) and len(avrc) - len(plain) == cost + grown
    if not split_bytes:
        assert cost == 7 * 36
    # with the file's CRC too: both fields
    both = _assemble("realshort.mp4", split_bytes, unit_checksums=True, checksums=True)
    ib = avr.describe_container(both)[0]
    assert ib["file_crc"] == zlib.crc32(data) and [b["unit_crcs"] for b in _coded(both)] == [b["unit_crcs"] for b in coded]
    assert strip_crc(strip_units(both)) == plain and strip_crc(both) == avrc
    # a reader from before the field, and the protobuf runtime
    assert _oracle_decompress(avrc) == (0, data)
    assert _pb.parse(avrc).SerializeToString() == avrc
    # the 19-argument entry point with the flag
    blob, offs, lens = _flat(blobs)
    if not split_bytes:
        res, olen = ctypes.c_void_p(), ctypes.c_size_t()
        assert avr.lib().avr_assemble_container_opts(data, len(data), avr.MODEL_PARALLEL, None, len(st), None, 0,
                                                     st.ctypes.data, blob, len(blob), offs.ctypes.data, lens.ctypes.data,
                                                     None, 0, None, None, avr.ASSEMBLE_UNIT_CRC, ctypes.byref(res),
                                                     ctypes.byref(olen)) == 0
        assert avr._take(res, olen.value) == avrc


def test_p32_streams_take_the_field_and_other_models_refuse_the_flag():
    data, st, blobs, _ = _outputs("realshort.mp4", True)
    blob, offs, lens = _flat(blobs)
    plain = avr.assemble_container(data, st, blob, offs, lens, model=avr.MODEL_PARALLEL32)
    avrc = avr.assemble_container(data, st, blob, offs, lens, model=avr.MODEL_PARALLEL32, unit_checksums=True)
    assert strip_units(avrc) == plain and avr.container_model(avrc) == avr.MODEL_PARALLEL32
    assert [b["unit_crcs"] for b in _coded(avrc)] == [b["unit_crcs"] for b in _coded(_unit_checked())]
    for model in (avr.MODEL_CHAINED,):
        with pytest.raises(avr.AvrError) as e:
            avr.assemble_container(data, st, blob, offs, lens, model=model, unit_checksums=True)
        assert e.value.code == ERR_INVALID
    # bit 8 stays no flag
    res, olen = ctypes.c_void_p(), ctypes.c_size_t()
    assert avr.lib().avr_assemble_container_opts(data, len(data), avr.MODEL_PARALLEL32, None, len(st), None, 0,
                                                 st.ctypes.data, blob, len(blob), offs.ctypes.data, lens.ctypes.data,
                                                 None, 0, None, None, avr.ASSEMBLE_UNIT_CRC | 8, ctypes.byref(res),
                                                 ctypes.byref(olen)) == ERR_INVALID


def _gloo_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        data, _, st, blobs, seams = _streams("realshort.mp4", 1024)
        lo, hi = shard.partition(avr.parse_stream(data).descs["payload_size"], world)[rank]

        def run_range(part):   # stands in for this rank's device compress, check and seams
            blob, offs, lens = _flat(blobs[lo:hi])
            flat = torch.from_numpy(np.frombuffer(blob + b"\0" * 16, dtype=np.uint8).copy())
            return flat, st[lo:hi].astype(np.int64), offs.astype(np.int64), lens.astype(np.int64), seams[lo:hi]

        out = shard.sharded_compress(None, data, split_bytes=1024, run_range=run_range, unit_checksums=True)
        if rank == 0:
            with open(os.path.join(outdir, "out.bin"), "wb") as f:
                f.write(out)
    finally:
        dist.destroy_process_group()


def test_sharded_compress_option_reaches_the_assembly():
    """shard.sharded_compress(unit_checksums=True) on a gloo world of 2, the device step replaced by
    the oracle's streams: rank 0 writes the assembly's container."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_gloo_worker, args=(2, port, td), nprocs=2, join=True)
        out = open(os.path.join(td, "out.bin"), "rb").read()
    assert out == _unit_checked("realshort.mp4", 1024)


# ------------------------------------------------------------------ malformed fields
def _with_field(avrc, block, make):
    """Block `block` (index among all blocks) with its field 18 replaced by make(content or None)."""
    def fn(k, fs):
        if k != block:
            return [raw for _, _, raw, _ in fs]
        old = next((c for f, w, raw, c in fs if f == 18), None)
        return [raw for f, w, raw, c in fs if f != 18] + [make(old)]
    return edit_blocks(avrc, fn)


def _block_index(avrc, want):
    """Index among all blocks of the first block for which want(describe's dict) holds."""
    return next(i for i, b in enumerate(avr.describe_container(avrc)[0]["blocks"]) if want(b))


@pytest.mark.parametrize("case", ["long", "short_cut", "ragged", "twice", "varint", "fixed32", "literal", "skip"])
def test_a_malformed_field_18_is_a_format_error(case):
    cut = case == "short_cut"
    avrc = _unit_checked("realshort.mp4", 1024 if cut else 0)
    first_coded = _block_index(avrc, lambda b: "cabac" in b and (not cut or "seams" in b))
    if case == "long":       # two values on an uncut block
        bad = _with_field(avrc, first_coded, lambda c: _ld(18, c + c))
    elif case == "short_cut":   # a cut block with one value too few
        bad = _with_field(avrc, first_coded, lambda c: _ld(18, c[:-4]))
    elif case == "ragged":   # not whole values
        bad = _with_field(avrc, first_coded, lambda c: _ld(18, c + b"\0"))
    elif case == "twice":
        bad = _with_field(avrc, first_coded, lambda c: _ld(18, c) + _ld(18, c))
    elif case == "varint":   # wire type 0
        bad = _with_field(avrc, first_coded, lambda c: _enc(18 << 3 | 0) + _enc(int.from_bytes(c, "little")))
    elif case == "fixed32":  # wire type 5
        bad = _with_field(avrc, first_coded, lambda c: _enc(18 << 3 | 5) + c[:4])
    elif case == "literal":
        bad = _with_field(avrc, _block_index(avrc, lambda b: "literal" in b), lambda c: _ld(18, b"\1\2\3\4"))
    else:
        avrc = _unit_checked("cockatoo.mp4", 0)   # its slices with emulation-prevention bytes are skip_coded
        bad = _with_field(avrc, _block_index(avrc, lambda b: "skip_coded" in b), lambda c: _ld(18, b"\1\2\3\4"))
    assert bad != avrc and _pb.parse(bad).SerializeToString() == bad   # still a Recoded message
    with pytest.raises(avr.AvrError) as e:
        avr.describe_container(bad)
    assert e.value.code == ERR_FORMAT
    for pieces in ((True,) if cut else (False, True)):
        with pytest.raises(avr.AvrError) as e:
            avr.DecompressPlan().load(bad, pieces=pieces)
        assert e.value.code == ERR_FORMAT
    # the undamaged container loads
    assert avr.DecompressPlan().load(avrc, pieces=True).n_slices == len(_coded(avrc))


def test_the_field_may_stand_on_some_blocks_only():
    avrc = _unit_checked()
    coded = [i for i, b in enumerate(avr.describe_container(avrc)[0]["blocks"]) if "cabac" in b]
    some = edit_blocks(avrc, lambda k, fs: [raw for f, w, raw, c in fs if f != 18 or k in coded[::2]])
    info = avr.describe_container(some)[0]
    assert sum("unit_crcs" in b for b in info["blocks"]) == len(coded[::2])
    data, chunks = _streams("realshort.mp4", 0)[0], _regen(some, _outputs("realshort.mp4")[3])
    assert _splice(some, chunks) == data
    plan = avr.DecompressPlan().load(some, pieces=True)
    have = plan.unit_crcs(0, plan.n_units)["have"]
    assert list(have) == [1, 0] * 18


# ------------------------------------------------------------------ the control
@lru_cache(None)
def _flipped():
    """(the plain realshort container with the control flip, the oracle's output of it)."""
    data, plain = _streams("realshort.mp4", 0)[:2]
    cabac = bytes.fromhex(_coded(plain)[FLIP_BLOCK]["cabac"])
    at = plain.find(cabac)
    assert len(cabac) == FLIP_CABAC_LEN and at > 0 and plain.find(cabac, at + 1) < 0
    d = bytearray(plain)
    d[at + FLIP_BYTE] ^= 0x10
    rc, out = _oracle_decompress(bytes(d))
    assert rc == 0
    return bytes(d), out


def test_control_the_flip_passes_an_unchecked_reader_with_wrong_bytes():
    data = _streams("realshort.mp4", 0)[0]
    damaged, out = _flipped()
    assert len(out) == len(data)
    assert tuple(int(i) for i in np.flatnonzero(np.frombuffer(out, np.uint8) != np.frombuffer(data, np.uint8))) == FLIP_WRONG
    # the block stands for the bytes the wrong ones lie in
    plan = avr.DecompressPlan().load(damaged, pieces=True)
    rng = plan.range(FLIP_WRONG[0], 3)
    assert rng["unit_hi"] - rng["unit_lo"] == 1 and rng["unit_lo"] == FLIP_BLOCK and int(rng["tails"][0]["size"]) == 1880
    assert avr.describe_container(damaged)[0]["blocks"] and FLIP_SPAN[1] - FLIP_SPAN[0] == 1880


# ------------------------------------------------------------------ reading: the plan path
def _apply(plan, chunks, lo=0, hi=None, status=None):
    """avr_unit_checks_apply over the units [lo, hi) of a piece plan, unit k's regenerated bytes chunks[k]
    packed one after the other: (return code, statuses)."""
    hi = plan.n_units if hi is None else hi
    pu = plan.parsed_units()
    rng = plan.range(0, plan.file_size)
    assert (rng["unit_lo"], rng["unit_hi"]) == (0, plan.n_units)
    blob, offs, lens = _packed(chunks[lo:hi])
    checks = plan.unit_crcs(lo, hi)
    checks["src_off"] = offs
    res = np.zeros(hi - lo, avr.SLICE_RESULT)
    res["out_len"] = lens
    return avr.unit_checks_apply(rng["tails"][lo:hi], checks, res, blob, status)


def test_the_damaged_unit_fails_its_check_and_the_splice():
    data = _streams("realshort.mp4", 0)[0]
    avrc = _unit_checked()
    assert "file_crc" not in avr.describe_container(avrc)[0]   # no Metadata field 16 anywhere here
    _, out = _flipped()
    chunks = _regen(avrc, _outputs("realshort.mp4")[3])
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    assert plan.n_units == len(chunks) == 36
    rc, st = _apply(plan, chunks)
    assert rc == 0 and not st.any()
    assert _splice(avrc, chunks) == data
    bad = list(chunks)
    bad[FLIP_BLOCK] = out[FLIP_SPAN[0]:FLIP_SPAN[1]]   # what the oracle regenerated from the flipped block
    assert len(bad[FLIP_BLOCK]) == len(chunks[FLIP_BLOCK]) and bad[FLIP_BLOCK] != chunks[FLIP_BLOCK]
    rc, st = _apply(plan, bad)
    assert rc == ERR_CHECKSUM and list(np.flatnonzero(st)) == [FLIP_BLOCK] and st[FLIP_BLOCK] == avr.SLICE_CHECKSUM
    rc, st = _apply(plan, bad, FLIP_BLOCK, FLIP_BLOCK + 1)   # the unit alone, as a range read selects it
    assert rc == ERR_CHECKSUM and list(st) == [avr.SLICE_CHECKSUM]
    rc, st = _apply(plan, bad, 0, FLIP_BLOCK)               # reads that avoid it
    assert rc == 0 and not st.any()
    with pytest.raises(avr.AvrError) as e:
        _splice(avrc, bad)
    assert e.value.code == ERR_CHECKSUM
    assert _splice(strip_units(avrc), bad) == out != data   # unchecked, the same bytes pass
    # device values a caller brings (avr_dec_plan_splice_crc) decide the same way
    with pytest.raises(avr.AvrError) as e:
        _splice(avrc, bad, np.array([zlib.crc32(c) for c in bad], np.uint32))
    assert e.value.code == ERR_CHECKSUM
    assert _splice(avrc, chunks, np.array([zlib.crc32(c) for c in chunks], np.uint32)) == data
    # avr_splice_container, one of the older entry points
    blob, offs, lens = _flat(bad)
    with pytest.raises(avr.AvrError) as e:
        avr.splice_container(avrc, np.zeros(36, np.int32), blob + b"\0", offs, lens)
    assert e.value.code == ERR_CHECKSUM
    # a preset status and a unit without a value are left alone
    pre = np.zeros(36, np.int32)
    pre[FLIP_BLOCK] = -9
    rc, st = _apply(plan, bad, status=pre)
    assert rc == 0 and st[FLIP_BLOCK] == -9 and np.count_nonzero(st) == 1
    # with both fields, both are checked: the file's CRC alone also refuses the damage
    both = _assemble("realshort.mp4", 0, unit_checksums=True, checksums=True)
    with pytest.raises(avr.AvrError) as e:
        _splice(both, bad)
    assert e.value.code == ERR_CHECKSUM
    assert _splice(both, chunks) == data


def test_a_stored_value_off_by_one_fails():
    data = _streams("realshort.mp4", 0)[0]
    avrc = _unit_checked()
    chunks = _regen(avrc, _outputs("realshort.mp4")[3])
    k = 7
    block = [i for i, b in enumerate(avr.describe_container(avrc)[0]["blocks"]) if "cabac" in b][k]
    off = _with_field(avrc, block, lambda c: _ld(18, ((int.from_bytes(c, "little") + 1) & 0xFFFFFFFF).to_bytes(4, "little")))
    assert _coded(off)[k]["unit_crcs"][0] == (_coded(avrc)[k]["unit_crcs"][0] + 1) & 0xFFFFFFFF
    with pytest.raises(avr.AvrError) as e:
        _splice(off, chunks)
    assert e.value.code == ERR_CHECKSUM
    rc, st = _apply(avr.DecompressPlan().load(off, pieces=True), chunks)
    assert rc == ERR_CHECKSUM and list(np.flatnonzero(st)) == [k]
    assert _splice(avrc, chunks) == data


def test_pieces_are_checked_one_by_one():
    """The container cut at 1024: every unit's true share passes, the splice of the collapsed units
    passes, and one byte flipped inside a first piece fails that unit alone -- the later pieces of the
    same slice still pass."""
    data = _streams("realshort.mp4", 1024)[0]
    avrc = _unit_checked("realshort.mp4", 1024)
    _, units, _ = expected_units(data, avrc, _streams("realshort.mp4", 0)[1])
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    chunks = [u["true"] for u in units]
    # a last unit regenerates its bytes before the rule: what replaces or appends is not the unit's yet
    rc, st = _apply(plan, chunks)
    assert rc == 0 and not st.any()
    # a piece that is not the last may regenerate more than it keeps
    first = next(k for k, u in enumerate(units) if u["keep"] != KEEP_ALL)
    more = list(chunks)
    more[first] = chunks[first] + b"\xAA" * 5
    rc, st = _apply(plan, more)
    assert rc == 0 and not st.any()
    bad = list(chunks)
    c = bytearray(bad[first])
    c[len(c) // 2] ^= 0x10
    bad[first] = bytes(c)
    rc, st = _apply(plan, bad)
    assert rc == ERR_CHECKSUM and list(np.flatnonzero(st)) == [first]
    assert units[first + 1]["slice"] == units[first]["slice"]
    rc, st = _apply(plan, bad, first + 1, first + 2)
    assert rc == 0 and not st.any()
    # the whole-file path: the slice's units collapsed
    blob, offs, lens = _packed(chunks)
    s0, so, sl = shard.collapse_units(plan.pieces, np.zeros(len(chunks), np.int64), offs, lens)
    assert plan.splice(s0, blob, so, sl).tobytes() == data
    blob, offs, lens = _packed(bad)
    with pytest.raises(avr.AvrError) as e:
        plan.splice(s0, blob, so, sl)
    assert e.value.code == ERR_CHECKSUM
    # a span outside the source
    checks = plan.unit_crcs(0, 1)
    checks["src_off"] = 5
    res = np.zeros(1, avr.SLICE_RESULT)
    res["out_len"] = len(chunks[0])
    rc, st = avr.unit_checks_apply(plan.range(0, plan.file_size)["tails"][:1], checks, res, chunks[0])
    assert rc == ERR_FORMAT and list(st) == [avr.SLICE_OVERFLOW]


def test_keep_replace_and_append_all_pass_on_cockatoo():
    name = "cockatoo.mp4"
    data = _streams(name, 0)[0]
    avrc = _unit_checked(name, 0)
    assert strip_units(avrc) == _streams(name, 0)[1]
    chunks = _regen(avrc, _outputs(name)[3])
    rules = _rules(avrc, chunks)
    assert "append" in rules and "replace" in rules
    # keep: a block whose last_byte field is gone (its regenerated last byte is the payload's already)
    m = _pb.parse(avrc)
    coded = [b for b in m.block if b.HasField("cabac")]
    k = next(i for i, (b, c) in enumerate(zip(coded, chunks)) if rules[i] == "replace" and c[-1:] == b.last_byte)
    coded[k].ClearField("last_byte")
    edited = m.SerializeToString()
    rules = _rules(edited, chunks)
    assert {"keep", "replace", "append"} <= set(rules) and rules[k] == "keep"
    assert [b["unit_crcs"] for b in _coded(edited)] == [b["unit_crcs"] for b in _coded(avrc)]
    plan = avr.DecompressPlan().load(edited, pieces=True)
    rc, st = _apply(plan, chunks)
    assert rc == 0 and not st.any()
    assert _splice(edited, chunks) == data
    # in each case the last regenerated byte, or the one before it, is checked
    for rule in ("keep", "replace", "append"):
        i = rules.index(rule)
        bad = list(chunks)
        at = -1 if rule != "replace" else -2   # a replaced last byte does not reach the file
        bad[i] = bytes(bad[i][:at]) + bytes([bad[i][at] ^ 0x10]) + (bytes(bad[i][at + 1:]) if at != -1 else b"")
        rc, st = _apply(plan, bad)
        assert rc == ERR_CHECKSUM and list(np.flatnonzero(st)) == [i], rule
        with pytest.raises(avr.AvrError) as e:
            _splice(edited, bad)
        assert e.value.code == ERR_CHECKSUM
    i = rules.index("replace")
    same = list(chunks)
    same[i] = same[i][:-1] + bytes([same[i][-1] ^ 0x10])
    rc, st = _apply(plan, same)
    assert rc == 0 and not st.any() and _splice(edited, same) == data
