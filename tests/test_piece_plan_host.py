"""Piece plans on the host (avr_dec_plan_load_pieces / _units / _recs; shard.subset_units,
shard.collapse_units, the unit path of shard.sharded_decompress): CPU only.

The containers are the oracle's (recode_oracle compress -p with AVR_SPLIT_BYTES), and the cuts are
read here from the seams fields themselves -- u32 raw length, zlib, the layout written down at
avr_seams.cpp's seams_encode -- never from the plan under test:

* the plan lists the expected coded slices and units, each unit's stream is its span of Block.cabac,
  its avr_piece and its seam record carry the field's values, its output fits the work buffer;
* fed every unit's true payload bytes, packed and collapsed, the splice restores the file -- also
  one byte short at each slice's end (the parity rule) -- and refuses a failed unit and a piece that
  came out short;
* a container without seams plans exactly as avr_dec_plan_load; reference and chained ones are refused;
* gloo worlds 2, 3 and 8 restore the file through shard.sharded_decompress with fabricated rank
  outputs, the pieces of one slice on different ranks at worlds 3 and 8."""
import os
import struct
import tempfile
import zlib
from functools import lru_cache

import numpy as np
import pytest

from _oracle import ROOT, oracle_cli

import avrecode_amd as avr
from avrecode_amd import shard

FIX = ROOT / "tests" / "fixtures"
KEEP_ALL = 0xFFFFFFFF
# SeamRec's head (avr_records.h): the decompress side reads first_mb, last_dqp_nz, ce_*, q
SEAM_HEAD = np.dtype([("first_mb", "<u4"), ("last_dqp_nz", "<u4"), ("cd", "<u4", (4,)), ("ce_low", "<u4"),
                      ("ce_range", "<u4"), ("ce_outstanding", "<u4"), ("ce_cache", "<u4"), ("ce_queue", "<i4"),
                      ("q", "<u4")])
# (fixture, split_bytes): coded slices, cut slices, pieces, units -- measured on the oracle's containers
COUNTS = {("realshort.mp4", 1024): (36, 31, 72, 77), ("realshort.mp4", 2048): (36, 3, 8, 41),
          ("cockatoo.mp4", 2048): (267, 41, 88, 314)}


@lru_cache(None)
def _container(name, split_bytes, mode="P"):
    return oracle_cli("compress", FIX / name, mode=mode, split_bytes=split_bytes)


def _seams(field: bytes):
    """A seams field decoded: (mb_width, piece_len[cuts + 1], cuts as dicts)."""
    raw_len, = struct.unpack_from("<I", field, 0)
    raw = zlib.decompress(field[4:])
    assert len(raw) == raw_len
    two, k, w = struct.unpack_from("<III", raw, 0)
    assert two == 2 and k > 0
    piece_len = list(struct.unpack_from(f"<{k + 1}I", raw, 12))
    p, cuts = 12 + 4 * (k + 1), []
    for _ in range(k):
        f = struct.unpack_from("<IIIIiIII", raw, p)
        cuts.append(dict(zip(("first_mb", "q", "last_dqp_nz", "ce_low", "ce_queue", "ce_outstanding", "ce_cache",
                              "ce_range"), f)))
        p += 32 + 1024 + 40 * w
    assert p == len(raw)
    return w, piece_len, cuts


def expected_units(data, avrc, plain):
    """What a piece plan of the container avrc of the file data must list, from the two alone: the
    coded slices' count, per unit (slice, stream, seam, n_mbs, keep, true bytes, the cut it starts
    from), and the cuts in record order.  The slices' own first_mb comes from the plain plan of
    `plain`, the same file's container without cuts.  (tests/test_gpu_pieces.py uses this too.)"""
    info, _ = avr.describe_container(avrc)
    first_mb = avr.DecompressPlan().load(plain).descs["first_mb"]
    units, recs, pos, s = [], [], 0, 0
    for b in info["blocks"]:
        if "literal" in b:
            pos += len(b["literal"]) // 2
        if "cabac" not in b:
            continue
        cabac, payload = bytes.fromhex(b["cabac"]), data[pos:pos + b["size"]]
        pos += b["size"]
        if "seams" not in b:
            units.append(dict(slice=s, stream=cabac, seam=-1, n_mbs=0, keep=KEEP_ALL, true=payload, cut=None))
        else:
            _, piece_len, cuts = _seams(bytes.fromhex(b["seams"]))
            assert sum(piece_len) == len(cabac)
            off = 0
            for i, pl in enumerate(piece_len):
                last = i == len(cuts)
                start_mb = cuts[i - 1]["first_mb"] if i else int(first_mb[s])
                q0 = cuts[i - 1]["q"] if i else 0
                units.append(dict(slice=s, stream=cabac[off:off + pl], seam=len(recs) + i - 1 if i else -1,
                                  n_mbs=0 if last else cuts[i]["first_mb"] - start_mb,
                                  keep=KEEP_ALL if last else cuts[i]["q"] - q0,
                                  true=payload[q0:] if last else payload[q0:cuts[i]["q"]],
                                  cut=cuts[i - 1] if i else None))
                off += pl
            recs += cuts
        s += 1
    assert s == len(first_mb)
    return s, units, recs


@lru_cache(None)
def _expected(name, split_bytes):
    data, avrc = (FIX / name).read_bytes(), _container(name, split_bytes)
    return (data, avrc) + expected_units(data, avrc, _container(name, 0))


def _packed(chunks):
    lens = np.array([len(c) for c in chunks], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return b"".join(chunks) + b"\0" * 16, offs, lens


def _splice(plan, chunks, status=None):
    blob, offs, lens = _packed(chunks)
    st = np.zeros(len(chunks), np.int64) if status is None else status
    st, offs, lens = shard.collapse_units(plan.pieces, st, offs, lens)
    return plan.splice(st, blob, offs, lens).tobytes()


@pytest.mark.parametrize("name,split_bytes", sorted(COUNTS))
def test_piece_plan_lists_the_containers_units(name, split_bytes):
    data, avrc, n_slices, units, recs = _expected(name, split_bytes)
    want_slices, want_cut, want_pieces, want_units = COUNTS[(name, split_bytes)]
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    cut_slices = {u["slice"] for u in units if u["keep"] != KEEP_ALL}
    assert (n_slices, len(cut_slices), sum(u["slice"] in cut_slices for u in units), len(units)) == \
        (want_slices, want_cut, want_pieces, want_units)
    assert plan.n_slices == want_slices and plan.n_units == want_units and len(plan.descs) == want_slices
    pu = plan.parsed_units()
    assert len(pu.descs) == len(pu.pieces) == want_units
    assert pu.rec_stride >= 64 + 1024 + 40 * plan.max_mb_width and pu.rec_stride % 16 == 0
    assert len(pu.recs) == len(recs) * pu.rec_stride
    for k, (u, d, p) in enumerate(zip(units, pu.descs, pu.pieces)):
        o, n = int(d["payload_offset"]), int(d["payload_size"])
        assert o % 16 == 0 and pu.arena[o:o + n].tobytes() == u["stream"], k
        assert not pu.arena[o + n:o + n + 16].any(), k
        assert (int(p["seam"]), int(p["n_mbs"]), int(p["slice"]), int(p["keep"])) == \
            (u["seam"], u["n_mbs"], u["slice"], u["keep"]), k
        assert int(d["out_offset"]) + int(d["out_capacity"]) <= pu.work_len, k
        if u["keep"] != KEEP_ALL:
            assert int(d["out_capacity"]) == u["keep"] + 4096, k
        if u["cut"] is not None:
            assert int(d["first_mb"]) == u["cut"]["first_mb"], k
    for i, cut in enumerate(recs):
        r = pu.recs[i * pu.rec_stride:i * pu.rec_stride + SEAM_HEAD.itemsize].view(SEAM_HEAD)[0]
        for f in cut:
            assert int(r[f]) == cut[f], (i, f)


@pytest.mark.parametrize("name,split_bytes", sorted(COUNTS))
def test_true_unit_bytes_splice_to_the_file(name, split_bytes):
    data, avrc, n_slices, units, _ = _expected(name, split_bytes)
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    true = [u["true"] for u in units]
    assert _splice(plan, true) == data
    # every slice's last unit one byte short of its parity: the stored last byte is appended
    short = [t[:-1] if u["keep"] == KEEP_ALL else t for t, u in zip(true, units)]
    assert _splice(plan, short) == data
    # a failed unit fails the file
    k = next(i for i, u in enumerate(units) if u["seam"] >= 0)
    st = np.zeros(len(units), np.int64)
    st[k] = -8
    with pytest.raises(avr.AvrError):
        _splice(plan, true, st)
    # so does a piece that is not the slice's last and came out one byte short
    k = next(i for i, u in enumerate(units) if u["keep"] != KEEP_ALL)
    with pytest.raises(avr.AvrError) as e:
        _splice(plan, true[:k] + [true[k][:-1]] + true[k + 1:])
    assert e.value.code == -3


def test_collapse_units_statuses():
    pieces = np.zeros(5, avr.PIECE)
    pieces["slice"] = [0, 1, 1, 1, 2]
    pieces["keep"] = [KEEP_ALL, 10, 20, KEEP_ALL, KEEP_ALL]
    offs, lens = np.array([0, 7, 17, 37, 42]), np.array([7, 10, 20, 5, 3])
    st, o, ln = shard.collapse_units(pieces, np.zeros(5), offs, lens)
    assert st.tolist() == [0, 0, 0] and o.tolist() == [0, 7, 42] and ln.tolist() == [7, 35, 3]
    assert st.dtype == np.int32 and o.dtype == np.uint64 and ln.dtype == np.uint32
    # the first non-zero status of a slice's units
    assert shard.collapse_units(pieces, np.array([0, 0, -5, -7, 0]), offs, lens)[0].tolist() == [0, -5, 0]
    # a gap between a slice's units in the blob; a piece that kept less than its share
    assert shard.collapse_units(pieces, np.zeros(5), np.array([0, 7, 18, 38, 43]), lens)[0].tolist() == [0, -9, 0]
    assert shard.collapse_units(pieces, np.zeros(5), np.array([0, 7, 17, 36, 41]),
                                np.array([7, 10, 19, 5, 3]))[0].tolist() == [0, -9, 0]
    assert [len(x) for x in shard.collapse_units(pieces[:0], [], [], [])] == [0, 0, 0]


@pytest.mark.parametrize("name,split_bytes", [("paff_ipp.264", 256), ("mbaff_ib.264", 256), ("realshort.mp4", 0)])
def test_without_seams_the_units_are_the_slices(name, split_bytes):
    avrc = _container(name, split_bytes)
    assert not avr.seams_of_container(avrc)
    a = avr.DecompressPlan().load(avrc)
    b = avr.DecompressPlan().load(avrc, pieces=True)
    assert a.n_slices == b.n_slices == b.n_units > 0
    assert a.descs.tobytes() == b.descs.tobytes() == b.units.tobytes()
    assert (a.arena_len, a.work_len, a.max_mb_width, a.max_mb_height) == \
        (b.arena_len, b.work_len, b.max_mb_width, b.max_mb_height)
    assert a.parsed().arena.tobytes() == b.parsed_units().arena.tobytes()
    assert len(b.recs) == 0
    p = b.pieces
    assert (p["seam"] == -1).all() and (p["n_mbs"] == 0).all() and (p["keep"] == KEEP_ALL).all()
    assert p["slice"].tolist() == list(range(b.n_units))


@pytest.mark.parametrize("mode", ["R", "C"])
def test_piece_plan_refuses_chaining_models(mode):
    with pytest.raises(avr.AvrError) as e:
        avr.DecompressPlan().load(_container("realshort.mp4", 1024, mode), pieces=True)
    assert e.value.code == -6


def test_subset_units_rebases_seams_and_records():
    _, avrc, _, units, recs = _expected("realshort.mp4", 1024)
    pu = avr.DecompressPlan().load(avrc, pieces=True).parsed_units()
    for lo, hi in ((0, len(units)), (5, 23), (30, 31), (40, 40), (len(units) - 9, len(units))):
        sub = shard.subset_units(pu, lo, hi)
        assert len(sub.descs) == len(sub.pieces) == hi - lo and sub.rec_stride == pu.rec_stride
        assert len(sub.recs) % pu.rec_stride == 0
        for k in range(hi - lo):
            u, d, p = units[lo + k], sub.descs[k], sub.pieces[k]
            o = int(d["payload_offset"])
            assert sub.arena[o:o + int(d["payload_size"])].tobytes() == u["stream"]
            assert int(d["out_offset"]) + int(d["out_capacity"]) <= sub.work_len
            assert (int(p["seam"]) >= 0) == (u["seam"] >= 0)
            if u["seam"] >= 0:
                assert 0 <= int(p["seam"]) < len(sub.recs) // pu.rec_stride
                r = sub.recs[int(p["seam"]) * pu.rec_stride:][:SEAM_HEAD.itemsize].view(SEAM_HEAD)[0]
                assert (int(r["first_mb"]), int(r["q"])) == (u["cut"]["first_mb"], u["cut"]["q"])


def _straddles(world):
    """Rank boundaries of shard.partition that fall between two pieces of one slice."""
    _, avrc, _, units, _ = _expected("realshort.mp4", 1024)
    parts = shard.partition([len(u["stream"]) for u in units], world)
    return sum(0 < lo < len(units) and units[lo - 1]["slice"] == units[lo]["slice"] for lo, _ in parts[1:])


def _gloo_units_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, avrc, _, units, _ = _expected("realshort.mp4", 1024)
        lo, hi = shard.partition([len(u["stream"]) for u in units], world)[rank]

        def run_range(part):   # stands in for this rank's device decompress and pack
            assert len(part.descs) == len(part.pieces) == hi - lo
            blob, offs, lens = _packed([u["true"] for u in units[lo:hi]])
            return torch.from_numpy(np.frombuffer(blob, np.uint8).copy()), np.zeros(hi - lo, np.int64), offs, lens

        out = shard.sharded_decompress(None, avrc, run_range=run_range)
        if rank == 0:
            with open(os.path.join(outdir, "out.bin"), "wb") as f:
                f.write(out)
        else:
            assert out is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_gloo_sharded_decompress_of_a_split_container(world):
    import socket

    import torch.multiprocessing as mp
    n = _straddles(world)
    print(f"world {world}: {n} rank boundaries inside a slice")
    if world in (3, 8):
        assert n >= 1   # a slice's pieces come from different ranks
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_gloo_units_worker, args=(world, port, td), nprocs=world, join=True)
        out = open(os.path.join(td, "out.bin"), "rb").read()
    assert out == (FIX / "realshort.mp4").read_bytes()
