"""Slices whose NAL unit carries emulation-prevention bytes, re-coded (Context.recode_escaped, Block
field 17, the "E" tags): the host side, CPU only.

* avr_escape_payload against a Python restatement of H.264 7.4.1, and unescape(escape(x)) == x;
* cockatoo.mp4 assembled from the oracle's per-slice streams (slices_p, which stand in for the
  device's outputs): with the flag every slice is a coded block, 13 of them carry field 17, the tag
  is avrecode-amd:P64E; without it 267 / 13 as before;
* the host round trip with no kernel: the plan of that container, spliced with the parse's own
  payloads as the "regenerated" bytes, is the file -- which it is not if an escaped block's
  surrogate occupies `size` instead of `size + k` bytes of read_packet's stream (every later MP4
  sample then moves under the parse);
* the same on an Annex-B stream built here, whose payloads hold 00 00 00, 00 00 01, 00 00 02,
  00 00 03 and a six-zero run, with a slice whose escaping is not the canonical one left skip_coded;
* nothing changes where there is nothing to escape, nor with the flag off;
* damaged containers are refused with AVR_ERR_FORMAT;
* gloo worlds 2 and 3 restore the file through shard.sharded_decompress from a container in which
  an escaped slice is also cut, its pieces on different ranks.  The oracle segments as the reference
  does and so never cuts such a slice: the seams field of that block is another cut slice's of the
  oracle's split container, its piece lengths rewritten.  Its streams are never decoded here (the
  ranks' outputs are fabricated); tests/test_gpu_escaped.py has the device make a real one."""
import ctypes
import os
import pickle
import struct
import tempfile
import zlib
from functools import lru_cache

import numpy as np
import pytest

from _oracle import ROOT, oracle_cli, slices_p

import avrecode_amd as avr
from avrecode_amd import shard

FIX = ROOT / "tests" / "fixtures"
ERR_FORMAT = -3
TAG, TAG_E = b"avrecode-amd:P64", b"avrecode-amd:P64E"


def py_escape(x: bytes) -> bytes:
    """7.4.1 from a clean state, byte by byte."""
    out, zeros = bytearray(), 0
    for b in x:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def py_unescape(x: bytes) -> bytes:
    out, i = bytearray(), 0
    while i < len(x):
        if i + 2 < len(x) and x[i] == 0 and x[i + 1] == 0 and x[i + 2] == 3:
            out += b"\0\0"
            i += 3
        else:
            out.append(x[i])
            i += 1
    return bytes(out)


# ------------------------------------------------------------------ the escape rule
def test_escape_zero_runs():
    """Every zero run of length 0-9 with a carry of 0-2 zeros in front, followed by each of 00-04 (a
    following 00 makes the run one longer), in the middle and at the very end of the buffer."""
    cases = []
    for carry in range(3):
        for run in range(10):
            for nxt in range(5):
                for tail in (b"", b"\x07\x00"):
                    cases.append(b"\x09" + b"\0" * carry + b"\x05" * (carry > 0) + b"\0" * run + bytes([nxt]) + tail)
                    cases.append(b"\0" * carry + b"\0" * run + bytes([nxt]) + tail)
            cases.append(b"\x21" + b"\0" * carry + b"\0" * run)   # the run ends the buffer: nothing appended
            cases.append(b"\0" * (carry + run))
    for x in cases:
        e = avr.escape_payload(x)
        assert e == py_escape(x), x.hex()
        assert py_unescape(e) == x
        assert not e.endswith(b"\0\0\3") or x.endswith(b"\0\0\3")
    assert avr.escape_payload(b"") == b""
    assert avr.escape_payload(b"\0\0") == b"\0\0" and avr.escape_payload(b"\0\0\0") == b"\0\0\3\0"
    assert avr.escape_payload(b"\0\0\0\0\0\0") == b"\0\0\3\0\0\3\0\0"


def test_escape_seeded_buffers():
    rng = np.random.default_rng(17)
    alphabet = np.array([0, 1, 2, 3, 4, 255], np.uint8)
    for _ in range(10000):
        x = alphabet[rng.integers(0, 6, size=int(rng.integers(1, 65)))].tobytes()
        e = avr.escape_payload(x)
        assert e == py_escape(x), x.hex()
        assert py_unescape(e) == x, x.hex()


def test_escape_payload_buffer_contract():
    L = avr.lib()
    src = ctypes.create_string_buffer(b"\0\0\1\0\0\2", 6)
    n = ctypes.c_size_t()
    assert L.avr_escape_payload(src, 6, None, 0, ctypes.byref(n)) == -1 and n.value == 8   # the length asked for
    dst = ctypes.create_string_buffer(8)
    assert L.avr_escape_payload(src, 6, dst, 8, ctypes.byref(n)) == 0 and dst.raw == b"\0\0\3\1\0\0\3\2"
    assert L.avr_escape_payload(src, 6, dst, 8, None) == -1


# ------------------------------------------------------------------ assembly
@lru_cache(None)
def _outputs(name, p32=False):
    data = (FIX / name).read_bytes()
    _, recs = slices_p(data, p32=p32)
    st = np.array([0 if r["recodable"] else -1 for r in recs], np.int32)
    blobs = [r["recoded"] if r["recodable"] else b"" for r in recs]
    return data, st, blobs


def _flat(blobs):
    lens = np.array([len(b) for b in blobs], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    return b"".join(blobs), offs, lens


def _assemble(data, st, blobs, escaped, ps=None, model=avr.MODEL_PARALLEL, seams=None):
    blob, offs, lens = _flat(blobs)
    return avr.assemble_container(data, st, blob, offs, lens, model=model, ps=ps, escaped=escaped, seams=seams)


def _opts(data, st, blobs, flags, model=avr.MODEL_PARALLEL):
    """avr_assemble_container_opts itself (descs NULL: it parses), as (status, bytes)."""
    L = avr.lib()
    blob, offs, lens = _flat(blobs)
    res, olen = ctypes.c_void_p(), ctypes.c_size_t()
    r = L.avr_assemble_container_opts(data, len(data), model, None, len(st), None, 0, st.ctypes.data, blob, len(blob),
                                      offs.ctypes.data, lens.ctypes.data, None, 0, None, None, flags, ctypes.byref(res),
                                      ctypes.byref(olen))
    return r, (avr._take(res, olen.value) if r == 0 else None)


@lru_cache(None)
def _cockatoo_e():
    data, st, blobs = _outputs("cockatoo.mp4")
    return data, _assemble(data, st, blobs, True)


def _counts(avrc):
    d, again = avr.describe_container(avrc)
    assert again == bytes(avrc)   # describe_container round-trips the bytes
    bl = d["blocks"]
    return (bytes.fromhex(d["version"]), sum("cabac" in b for b in bl), sum("skip_coded" in b for b in bl),
            [b for b in bl if "escapes" in b])


@pytest.mark.parametrize("parsed", [False, True], ids=["reparse", "parsed"])
def test_cockatoo_codes_every_slice_with_the_flag(parsed):
    data, st, blobs = _outputs("cockatoo.mp4")
    ps = avr.parse_stream(data) if parsed else None
    tag, coded, skipped, esc = _counts(_assemble(data, st, blobs, False, ps))
    assert (tag, coded, skipped, len(esc)) == (TAG, 267, 13, 0)
    avrc = _assemble(data, st, blobs, True, ps)
    assert avrc == _cockatoo_e()[1]
    tag, coded, skipped, esc = _counts(avrc)
    assert (tag, coded, skipped, len(esc)) == (TAG_E, 280, 0, 13)
    assert sum(b["size"] for b in esc) == 33399
    assert all(b["escapes"] >= 1 and "cabac" in b for b in esc)
    assert avr.container_model(avrc) == avr.MODEL_PARALLEL
    # the blocks and literals cover the file: an escaped block stands for size + k bytes
    d, _ = avr.describe_container(avrc)
    assert sum(len(b.get("literal", "")) // 2 + (b["size"] + b.get("escapes", 0) if "cabac" in b else 0)
               for b in d["blocks"]) == len(data)


def test_p32_gets_its_own_e_tag():
    data, st, blobs = _outputs("cockatoo.mp4", True)
    avrc = _assemble(data, st, blobs, True, model=avr.MODEL_PARALLEL32)
    tag, coded, skipped, esc = _counts(avrc)
    assert (tag, coded, skipped, len(esc)) == (b"avrecode-amd:P32E", 280, 0, 13)
    assert avr.container_model(avrc) == avr.MODEL_PARALLEL32


def _payloads(data):
    """The parse's own payloads, per slice."""
    ps = avr.parse_stream(data)
    return [ps.arena[int(d["payload_offset"]):int(d["payload_offset"]) + int(d["payload_size"])].tobytes()
            for d in ps.descs]


def _coded_payloads(avrc, pays):
    """The payloads of the container's coded blocks, in block order (slice i is the i-th non-literal block)."""
    d, _ = avr.describe_container(avrc)
    nl = [b for b in d["blocks"] if "literal" not in b]
    assert len(nl) == len(pays)
    return [p for b, p in zip(nl, pays) if "cabac" in b]


def _splice_whole(avrc, chunks):
    blob, offs, lens = _flat(chunks)
    return avr.splice_container(avrc, np.zeros(len(chunks), np.int32), blob, offs, lens)


def test_host_round_trip_of_cockatoo():
    data, avrc = _cockatoo_e()
    pays = _coded_payloads(avrc, _payloads(data))
    plan = avr.plan_decompress(avrc)
    assert len(plan.descs) == len(pays) == 280
    # descriptors are in the unescaped domain
    d, _ = avr.describe_container(avrc)
    sizes = [b["size"] for b in d["blocks"] if "cabac" in b]
    assert [int(x) for x in plan.descs["out_capacity"]] == [s + 64 for s in sizes]
    assert sizes == [len(p) for p in pays]
    assert _splice_whole(avrc, pays) == data
    # patch, then escape: every slice one byte short of its parity still restores the file
    assert _splice_whole(avrc, [p[:-1] for p in pays]) == data
    # a regenerated slice whose escape inserts another count than the block's
    k = next(i for i, b in enumerate(x for x in d["blocks"] if "cabac" in x) if "escapes" in b)
    bad = list(pays)
    bad[k] = bytes(len(pays[k]) - 1) + pays[k][-1:]
    with pytest.raises(avr.AvrError) as e:
        _splice_whole(avrc, bad)
    assert e.value.code == ERR_FORMAT
    # the handle's splice (copy jobs and the side buffer) agrees
    dp = avr.DecompressPlan().load(avrc)
    blob, offs, lens = _flat(pays)
    assert dp.splice(np.zeros(len(pays), np.int32), blob, offs, lens).tobytes() == data


# ------------------------------------------------------------------ an Annex-B stream built here
def _annexb():
    """paff_ipp.264's parameter sets, then slices made from its first slice NAL with bytes appended to
    the payload: per slice one of the patterns, canonically escaped; slice 5's NAL holds 00 00 03 7f
    (not what an encoder writes: unescape drops the 03 the FFmpeg way, escape does not put it back);
    slice 6 has nothing to escape."""
    import bench
    head, slices = bench._split_slices((FIX / "paff_ipp.264").read_bytes())
    tmpl = slices[0]
    sc, body = tmpl[:4], tmpl[4:]
    assert sc == b"\0\0\0\1" and py_escape(body[1:]) == body[1:] and body[-1] != 0
    rng = np.random.default_rng(5)
    pats = [b"\0\0\0", b"\0\0\1", b"\0\0\2", b"\0\0\3", b"\0" * 6]
    out, kinds = [head], []
    for i in range(7):
        fill = [rng.integers(4, 256, size=200, dtype=np.uint8).tobytes() for _ in range(3)]
        if i < 5:
            raw = fill[0] + pats[i] + fill[1] + (pats[(i + 2) % 5] + fill[2] if i % 2 else b"")
            out.append(sc + body[:1] + py_escape(body[1:] + raw + b"\x80"))
            kinds.append("escaped")
        elif i == 5:
            raw = fill[0] + b"\0\0\1" + fill[1]
            out.append(sc + body[:1] + py_escape(body[1:] + raw) + b"\0\0\3\x7f" + fill[2] + b"\x80")
            kinds.append("noncanonical")
        else:
            out.append(sc + body + b"".join(fill) + b"\x80")
            kinds.append("plain")
    return b"".join(out), kinds


def test_annexb_stream_round_trips():
    data, kinds = _annexb()
    ps = avr.parse_stream(data)
    assert len(ps.descs) == len(kinds) and (ps.descs["coded"] == 1).all()
    n = len(kinds)
    st = np.zeros(n, np.int32)
    blobs = [b"RC%03d" % i for i in range(n)]
    off = _assemble(data, st, blobs, False)
    tag, coded, skipped, esc = _counts(off)
    assert (tag, coded, skipped, esc) == (TAG, 1, 6, [])
    for parsed in (None, ps):
        avrc = _assemble(data, st, blobs, True, parsed)
        tag, coded, skipped, esc = _counts(avrc)
        assert (tag, coded, skipped, len(esc)) == (TAG_E, 6, 1, 5)
    d, _ = avr.describe_container(avrc)
    nl = [b for b in d["blocks"] if "literal" not in b]
    assert ["skip_coded" in b for b in nl] == [k == "noncanonical" for k in kinds]
    pays = _payloads(data)
    for b, p in zip(nl, pays):
        if "escapes" in b:
            assert b["escapes"] == len(py_escape(p)) - len(p) >= 1 and py_escape(p) in data
    coded_pays = _coded_payloads(avrc, pays)
    assert _splice_whole(avrc, coded_pays) == data
    assert _splice_whole(avrc, [p[:-1] for p in coded_pays]) == data


# ------------------------------------------------------------------ nothing to escape, flag off
def test_no_change_without_affected_slices():
    data, st, blobs = _outputs("realshort.mp4")
    for ps in (None, avr.parse_stream(data)):
        a, b = _assemble(data, st, blobs, False, ps), _assemble(data, st, blobs, True, ps)
        assert a == b and _counts(b)[0] == TAG


@pytest.mark.parametrize("name", ["realshort.mp4", "cockatoo.mp4"])
def test_opts_with_no_flag_is_assemble_container(name):
    data, st, blobs = _outputs(name)
    r, c = _opts(data, st, blobs, 0)
    assert r == 0 and c == _assemble(data, st, blobs, False)
    r, c = _opts(data, st, blobs, avr.ASSEMBLE_ESCAPED)
    assert r == 0 and c == _assemble(data, st, blobs, True)


def test_flag_is_refused_for_other_models_and_unknown_bits():
    data, st, blobs = _outputs("realshort.mp4")
    assert _opts(data, st, blobs, avr.ASSEMBLE_ESCAPED, avr.MODEL_CHAINED)[0] == -1
    assert _opts(data, st, blobs, avr.ASSEMBLE_ESCAPED, avr.MODEL_REFERENCE)[0] == -1
    assert _opts(data, st, blobs, 2)[0] == -1
    assert _opts(data, st, blobs, 0, avr.MODEL_CHAINED)[0] == 0


# ------------------------------------------------------------------ damaged containers
def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _fields(b):
    """A message's fields as [(number, wire type, value)]: ints for varints, bytes for length-delimited."""
    out, i = [], 0
    while i < len(b):
        t, i = avr._varint(b, i)
        if t & 7 == 0:
            v, i = avr._varint(b, i)
        else:
            assert t & 7 == 2
            n, i = avr._varint(b, i)
            v, i = bytes(b[i:i + n]), i + n
        out.append((t >> 3, t & 7, v))
    return out


def _message(fields):
    return b"".join(_varint(f << 3 | w) + (_varint(v) if w == 0 else _varint(len(v)) + v) for f, w, v in fields)


def _rewritten(avrc, edit):
    """The container with edit(index, block fields) -> block fields applied to every Block, and
    edit(None, version) -> version to the tag."""
    top = []
    k = 0
    for f, w, v in _fields(avrc):
        if f == 1:
            md = _fields(v)
            v = _message([(1, 2, edit(None, md[0][2]))])
        elif f == 2:
            v = _message(edit(k, _fields(v)))
            k += 1
        top.append((f, w, v))
    return _message(top)


def test_rewriting_is_the_identity_without_an_edit():
    _, avrc = _cockatoo_e()
    assert _rewritten(avrc, lambda k, x: x) == avrc


def _first_escaped(avrc):
    for k, (f, w, v) in enumerate(x for x in _fields(avrc) if x[0] == 2):
        bf = _fields(v)
        if any(n == 17 for n, _, _ in bf):
            return k, dict((n, x) for n, _, x in bf)
    raise AssertionError("no field 17")


@pytest.mark.parametrize("damage", ["k+1", "k-1", "k=0", "on-literal", "plain-tag", "k>size/2+1"])
def test_damaged_containers_are_refused(damage):
    data, avrc = _cockatoo_e()
    at, blk = _first_escaped(avrc)
    k, size = blk[17], blk[1]

    def set_k(v):
        return lambda i, x: [(n, w, v if n == 17 else y) for n, w, y in x] if i == at else x

    if damage == "k+1":
        bad = _rewritten(avrc, set_k(k + 1))
    elif damage == "k-1":   # on the block with the largest k (k - 1 = 0 is refused as well)
        blocks = [dict((n, y) for n, _, y in _fields(v)) for f, _, v in _fields(avrc) if f == 2]
        at = max(range(len(blocks)), key=lambda i: blocks[i].get(17, 0))
        bad = _rewritten(avrc, set_k(blocks[at][17] - 1))
    elif damage == "k=0":
        bad = _rewritten(avrc, set_k(0))
    elif damage == "k>size/2+1":
        bad = _rewritten(avrc, set_k(size // 2 + 2))
    elif damage == "on-literal":
        bad = _rewritten(avrc, lambda i, x: x + [(17, 0, 1)] if i == 0 else x)
        assert "literal" in avr.describe_container(bad)[0]["blocks"][0]
    else:
        bad = _rewritten(avrc, lambda i, x: TAG if i is None else x)
    pays = _coded_payloads(avrc, _payloads(data))
    with pytest.raises(avr.AvrError) as e:
        avr.plan_decompress(bad)
        _splice_whole(bad, pays)   # k +- 1 within the bounds is caught at the latest here
    assert e.value.code == ERR_FORMAT
    with pytest.raises(avr.AvrError) as e:
        avr.DecompressPlan().load(bad, pieces=True)
        _splice_whole(bad, pays)
    assert e.value.code == ERR_FORMAT


# ------------------------------------------------------------------ sharded splice on gloo
SPLIT = 512
PIECE_BYTES = 1 << 20   # the fabricated pieces' streams: longer than the rest of the container together


@lru_cache(None)
def _split_escaped():
    """(file, container, units): cockatoo's escaped container in which the first affected slice also
    carries a seams field -- a cut slice's of the oracle's split container at SPLIT bytes, every
    piece_len rewritten to PIECE_BYTES, so that every rank boundary at worlds 2 and 3 falls between
    its pieces.  units: per unit (slice index among the coded ones, true bytes)."""
    data, st, blobs = _outputs("cockatoo.mp4")
    blobs = list(blobs)
    pays = _payloads(data)
    plain = avr.describe_container(_assemble(data, st, blobs, True))[0]
    nl = [b for b in plain["blocks"] if "literal" not in b]
    target = next(i for i, b in enumerate(nl) if "escapes" in b)
    donor = None
    for b in avr.describe_container(oracle_cli("compress", FIX / "cockatoo.mp4", mode="P", split_bytes=SPLIT))[0]["blocks"]:
        if "seams" in b:
            field = bytes.fromhex(b["seams"])
            raw = bytearray(zlib.decompress(field[4:]))
            k, w = struct.unpack_from("<II", raw, 4)
            per = 32 + 1024 + 40 * w
            qs = [struct.unpack_from("<I", raw, 12 + 4 * (k + 1) + per * i + 4)[0] for i in range(k)]
            if k >= 2 and qs[-1] < len(pays[target]) - 8:
                donor = (raw, k, qs)
                break
    assert donor is not None
    raw, k, qs = donor
    struct.pack_into(f"<{k + 1}I", raw, 12, *([PIECE_BYTES] * (k + 1)))
    seams = [b""] * len(blobs)
    seams[target] = struct.pack("<I", len(raw)) + zlib.compress(bytes(raw), 1)
    blobs[target] = b"\x5a" * (PIECE_BYTES * (k + 1))
    avrc = _assemble(data, st, blobs, True, seams=seams)
    d = avr.describe_container(avrc)[0]
    both = [b for b in d["blocks"] if "seams" in b and "escapes" in b]
    assert len(both) == 1 and _counts(avrc)[:3] == (TAG_E, 280, 0)
    units = []
    for s, p in enumerate(pays):
        if s != target:
            units.append((s, p))
        else:
            cuts = [0] + qs + [len(p)]
            units += [(s, p[a:b]) for a, b in zip(cuts, cuts[1:])]
    return data, avrc, units, target


def _unit_lens(avrc):
    return avr.DecompressPlan().load(avrc, pieces=True).parsed_units().descs["payload_size"]


def test_split_and_escaped_block_splices_on_one_host():
    data, avrc, units, target = _split_escaped()
    with pytest.raises(avr.AvrError) as e:
        avr.plan_decompress(avrc)   # a split container goes by units
    assert e.value.code == -6
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    assert plan.n_slices == 280 and plan.n_units == len(units)
    blob, offs, lens = _flat([u for _, u in units])
    st, offs, lens = shard.collapse_units(plan.pieces, np.zeros(len(units), np.int64), offs.astype(np.int64),
                                          lens.astype(np.int64))
    assert plan.splice(st, blob + b"\0" * 16, offs, lens).tobytes() == data


def _gloo_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        with open(os.path.join(outdir, "in.pkl"), "rb") as f:   # the parent's container and units
            avrc, units = pickle.load(f)
        lo, hi = shard.partition(_unit_lens(avrc), world)[rank]

        def run_range(part):   # stands in for this rank's device decompress and pack
            assert len(part.descs) == len(part.pieces) == hi - lo
            blob, offs, lens = _flat([u for _, u in units[lo:hi]])
            return (torch.from_numpy(np.frombuffer(blob + b"\0" * 16, np.uint8).copy()), np.zeros(hi - lo, np.int64),
                    offs.astype(np.int64), lens.astype(np.int64))

        out = shard.sharded_decompress(None, avrc, run_range=run_range)
        if rank == 0:
            with open(os.path.join(outdir, "out.bin"), "wb") as f:
                f.write(out)
        else:
            assert out is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_sharded_decompress_of_a_split_escaped_slice(world):
    import socket

    import torch.multiprocessing as mp
    data, avrc, units, target = _split_escaped()
    owners = set()
    for r, (lo, hi) in enumerate(shard.partition(_unit_lens(avrc), world)):
        owners |= {r for s, _ in units[lo:hi] if s == target}
    assert len(owners) >= 2   # the escaped slice's pieces come from different ranks
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "in.pkl"), "wb") as f:
            pickle.dump((avrc, units), f)
        mp.spawn(_gloo_worker, args=(world, port, td), nprocs=world, join=True)
        out = open(os.path.join(td, "out.bin"), "rb").read()
    assert out == data
