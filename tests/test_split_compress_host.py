"""The host side of the split compress of slice batches (avr_split_plan, avr_seams_build,
avr_assemble_container_seams; shard.select and the split path of shard.sharded_compress): CPU only.

The containers are the oracle's (recode_oracle compress -p with AVR_SPLIT_BYTES); their cuts are read
by test_piece_plan_host's own decoder of the seams field, the cut records come from the piece plan of
the same container (avr_dec_plan_recs), and everything built here must reproduce the container's own
bytes:

* avr_split_plan states the candidate rule and the sizes of the whole-file compress on a table of
  descriptors around every threshold;
* avr_seams_build, given a batch laid out as a split walk leaves it, writes each cut slice's Block
  field 16 byte for byte (the records' re-encoder fields taken as they are), fails every cut slice
  with AVR_SLICE_CODER when asked to restate cuts whose decoder state is zero, and refuses every
  array that does not fit the others;
* assemble_container with the container's own cabac and seams blocks gives the container back, and
  refuses seams where the format has none;
* gloo worlds 2, 3 and 8 of sharded_compress(split_bytes=1024) with fabricated rank outputs give the
  oracle's container on rank 0."""
import os
import tempfile
from functools import lru_cache

import numpy as np
import pytest

from _oracle import ROOT
from test_piece_plan_host import _container, _seams

import avrecode_amd as avr
from avrecode_amd import shard

FIX = ROOT / "tests" / "fixtures"
CASES = [("realshort.mp4", 1024), ("realshort.mp4", 2048), ("cockatoo.mp4", 2048)]
SLICE_CODER = -10


def _rule(d, split_bytes):
    """The candidate rule and sizes as the issue states them, in plain Python."""
    on = 0 < split_bytes < 1 << 28
    slots, caps, nrec, max_w = [], [], 0, 1
    for x in d:
        size, w = int(x["payload_size"]), int(x["mb_width"])
        if on and int(x["structure"]) == 0 and w <= 288 and 2 * size >= 3 * split_bytes:
            cap = 8 * size // (8 * split_bytes) + 1
            slots.append((nrec, cap))
            caps.append(2 * size + 256 + 64 * cap)
            nrec += cap
            max_w = max(max_w, w)
        else:
            slots.append((-1, 0))
            caps.append(0)
    return slots, caps, nrec, (64 + 1024 + 40 * max_w + 15) & ~15


def _table(split_bytes):
    rows = []   # (payload_size, structure, mb_width)
    t = (3 * split_bytes + 1) // 2 if split_bytes < 1 << 28 else 3 << 27
    for size in (0, 7, t - 1, t, t + 1, 2 * t, 10 * t + 3):
        for structure in (0, 1, 2, 3):
            for w in (1, 120, 240, 288, 289, 400):
                rows.append((max(0, size), structure, w))
    d = np.zeros(len(rows), avr.SLICE_DESC)
    d["payload_size"], d["structure"], d["mb_width"] = zip(*rows)
    d["coded"] = 1
    return d


@pytest.mark.parametrize("split_bytes", [0, 1, 700, 1024, 98304, 1 << 28])
def test_split_plan_states_the_rule(split_bytes):
    d = _table(split_bytes)
    slots, caps, nrec, stride = _rule(d, split_bytes)
    p = avr.split_plan(d, split_bytes)
    assert [(int(a), int(b)) for a, b in p.slots] == slots
    assert p.out_capacity.tolist() == caps
    assert (p.n_recs, p.rec_stride) == (nrec, stride)
    assert p.n_candidates == sum(f >= 0 for f, _ in slots) == int(p.candidate.sum())
    if split_bytes in (0, 1 << 28):
        assert p.n_candidates == 0 and p.n_recs == 0
    else:
        # just below 1.5 split_bytes is no candidate, at it is one; 288 wide is, 289 is not; frames only
        t = (3 * split_bytes + 1) // 2
        for x, (f, cap) in zip(d, slots):
            want = x["structure"] == 0 and x["mb_width"] <= 288 and x["payload_size"] >= t
            assert (f >= 0) == bool(want)
        assert p.n_candidates > 0


def test_split_plan_of_an_empty_batch():
    p = avr.split_plan(np.zeros(0, avr.SLICE_DESC), 1024)
    assert (len(p.slots), p.n_recs, p.n_candidates, p.rec_stride) == (0, 0, 0, 64 + 1024 + 48)


def test_no_walk_fills_its_slot_and_some_leave_one_record():
    """Every split block of the oracle's P containers of both fixtures at split_bytes 512, 1024 and
    2048 has cuts <= cap - 1 (cap from avr_split_plan on the parsed descriptors): the split walk is
    offered cap - 1 records of a slot, so that the end of its last piece stays inside it.  Slices with
    cuts == cap - 1, the case that offer decides, are among them at every one of the sizes (realshort:
    3, 16 and 1 slices, e.g. slice 31 of 1002 bytes with one cut at 512; cockatoo: 69, 106 and 37).
    realshort at 512 and 2048 and cockatoo at 512 and 2048 are cases of
    test_gpu_split.py::test_fixture_split_matches_oracle, so the device's walk with cap - 1 records is
    already held to the oracle's container there and no GPU case is added."""
    full = {}
    for name in ("realshort.mp4", "cockatoo.mp4"):
        ps = avr.parse_stream((FIX / name).read_bytes())
        for split_bytes in (512, 1024, 2048):
            info, _ = avr.describe_container(_container(name, split_bytes))
            blocks = [b for b in info["blocks"] if "literal" not in b]
            assert len(blocks) == len(ps.descs)
            slots = avr.split_plan(ps.descs, split_bytes).slots
            cut = [(k, len(_seams(bytes.fromhex(b["seams"]))[2])) for k, b in enumerate(blocks) if "seams" in b]
            assert cut
            for k, cuts in cut:
                assert 1 <= cuts <= int(slots[k]["cap"]) - 1, (name, split_bytes, k)
            full[name, split_bytes] = sum(cuts == int(slots[k]["cap"]) - 1 for k, cuts in cut)
    assert all(full.values()), full   # the GPU test's sizes among them


@lru_cache(None)
def _batch(name, split_bytes):
    """The oracle's split container of a fixture as the batch a split walk would have left: the
    file's parse, per slice its block, results, slots, cut counts, piece ends and the records at
    their slots."""
    data, avrc = (FIX / name).read_bytes(), _container(name, split_bytes)
    ps = avr.parse_stream(data)
    info, _ = avr.describe_container(avrc)
    blocks = [b for b in info["blocks"] if "literal" not in b]
    assert len(blocks) == len(ps.descs)
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    sp = avr.split_plan(ps.descs, split_bytes)
    n = len(blocks)
    res = np.zeros(n, avr.SLICE_RESULT)
    cuts = np.zeros(n, np.uint32)
    piece_end = np.zeros(sp.n_recs, np.uint32)
    stride = plan.rec_stride
    assert stride >= sp.rec_stride
    recs = np.zeros(sp.n_recs * stride, np.uint8)
    fields, cabac, rec = [], [], 0
    for k, b in enumerate(blocks):
        f, cap = int(sp.slots[k]["first"]), int(sp.slots[k]["cap"])
        if "cabac" not in b:
            res[k]["status"] = -1
            fields.append(b"")
            cabac.append(b"")
            continue
        c = bytes.fromhex(b["cabac"])
        cabac.append(c)
        res[k]["out_len"] = len(c)
        fields.append(bytes.fromhex(b.get("seams", "")))
        if f >= 0:
            piece_end[f] = len(c)
        if "seams" in b:
            assert f >= 0   # the oracle cuts candidates only
            w, piece_len, cs = _seams(fields[-1])
            assert len(cs) < cap and w == int(ps.descs[k]["mb_width"])
            cuts[k] = len(cs)
            piece_end[f:f + len(cs) + 1] = np.cumsum(piece_len)
            recs[f * stride:(f + len(cs)) * stride] = plan.recs[rec * stride:(rec + len(cs)) * stride]
            rec += len(cs)
    assert rec * stride == len(plan.recs)
    return dict(data=data, avrc=avrc, ps=ps, sp=sp, res=res, cuts=cuts, piece_end=piece_end, recs=recs, stride=stride,
                fields=fields, cabac=cabac)


def _build(b, check_cuts, **over):
    a = dict(descs=b["ps"].descs, arena=b["ps"].arena, res=b["res"], slots=b["sp"].slots, cuts=b["cuts"],
             piece_end=b["piece_end"], recs=b["recs"], rec_stride=b["stride"])
    a.update(over)
    return avr.seams_build(check_cuts=check_cuts, **a)


@pytest.mark.parametrize("name,split_bytes", CASES)
def test_seams_build_writes_the_containers_fields(name, split_bytes):
    b = _batch(name, split_bytes)
    status, fields = _build(b, False)
    assert status.tolist() == b["res"]["status"].tolist()
    if name == "realshort.mp4":   # test_piece_plan_host.py COUNTS: the cut slices
        assert sum(map(bool, b["fields"])) == {1024: 31, 2048: 3}[split_bytes]
    assert any(b["fields"])
    for k, (got, want) in enumerate(zip(fields, b["fields"])):
        assert got == want, k


@pytest.mark.parametrize("name,split_bytes", CASES)
def test_seams_build_checks_cuts_against_the_restatement(name, split_bytes):
    b = _batch(name, split_bytes)
    status, fields = _build(b, True)   # the plan's records carry no decoder state: cd_* are zero
    for k in range(len(status)):
        if b["cuts"][k]:
            assert status[k] == SLICE_CODER and fields[k] == b"", k
        else:
            assert status[k] == b["res"][k]["status"] and fields[k] == b"", k


def test_seams_build_refuses_arrays_that_do_not_fit():
    b = _batch("realshort.mp4", 1024)
    sp, stride = b["sp"], b["stride"]
    k = int(np.flatnonzero(b["cuts"] >= 2)[0])
    f, cap, nc = int(sp.slots[k]["first"]), int(sp.slots[k]["cap"]), int(b["cuts"][k])
    w = int(b["ps"].descs[k]["mb_width"])

    def refused(**over):
        for check in (False, True):
            with pytest.raises(avr.AvrError) as e:
                _build(b, check, **over)
            assert e.value.code == -1

    def changed(name, at, value):
        a = b[name].copy() if name in b else getattr(sp, name).copy()
        a[at] = value
        return a

    refused(cuts=changed("cuts", k, cap))                                    # cuts < cap
    refused(cuts=changed("cuts", k, 0xFFFFFFFF))
    u = int(np.flatnonzero(sp.slots["first"] < 0)[0])
    refused(cuts=changed("cuts", u, 1))                                      # cuts without a slot
    last = int(np.argmax(sp.slots["first"]))
    refused(piece_end=b["piece_end"][:-1], recs=b["recs"][:-stride])         # the last slot outside n_recs
    s = sp.slots.copy()
    s[last]["first"] += 1
    refused(slots=s)
    s = sp.slots.copy()
    s[k]["first"] = -2
    refused(slots=s)
    s = sp.slots.copy()
    s[k]["cap"] = 0
    refused(slots=s)
    refused(piece_end=changed("piece_end", f + 1, int(b["piece_end"][f]) - 1))   # piece ends decrease
    refused(piece_end=changed("piece_end", f + nc, int(b["piece_end"][f + nc]) + 1))   # last != out_len
    r = b["res"].copy()
    r[k]["out_len"] -= 1
    refused(res=r)
    small = ((64 + 1024 + 40 * w + 15) & ~15) - 16                           # less than a record of this width
    refused(rec_stride=small)
    refused(rec_stride=0)
    refused(recs=b["recs"][:-1])                                             # recs shorter than n_recs records
    d = b["ps"].descs.copy()
    d[k]["mb_width"] = 289
    refused(descs=d)
    d = b["ps"].descs.copy()
    d[k]["payload_offset"] = len(b["ps"].arena)                              # a payload outside the arena
    refused(descs=d)
    refused(arena=b["ps"].arena[:int(b["ps"].descs[k]["payload_offset"]) + 1])
    with pytest.raises(ValueError):
        _build(b, False, cuts=b["cuts"][:-1])
    # and unchanged it still builds
    assert _build(b, False)[1][k] == b["fields"][k]


def _outputs(b, lo=0, hi=None):
    """avr_assemble_container's inputs for the slices [lo, hi) from the container's own blocks."""
    hi = len(b["cabac"]) if hi is None else hi
    lens = np.array([len(c) for c in b["cabac"][lo:hi]], np.int64)
    offs = np.cumsum(lens) - lens
    blob = np.frombuffer(b"".join(b["cabac"][lo:hi]) + b"\0" * 16, np.uint8)
    return b["res"]["status"][lo:hi].astype(np.int64), blob, offs, lens


@pytest.mark.parametrize("name,split_bytes", CASES)
def test_assembly_with_the_containers_own_blocks_gives_the_container(name, split_bytes):
    b = _batch(name, split_bytes)
    st, blob, offs, lens = _outputs(b)
    assert avr.assemble_container(b["data"], st, blob, offs, lens, seams=b["fields"]) == b["avrc"]
    assert avr.assemble_container(b["data"], st, blob, offs, lens, ps=b["ps"], seams=b["fields"]) == b["avrc"]
    sl = np.array([len(f) for f in b["fields"]], np.uint32)
    so = np.cumsum(sl, dtype=np.uint64) - sl
    got = avr.assemble_container(b["data"], st, blob, offs, lens, ps=b["ps"],
                                 seams=(np.frombuffer(b"".join(b["fields"]), np.uint8), so, sl), as_array=True)
    assert got.tobytes() == b["avrc"]
    # without them the container has no field 16 and is another one
    plain = avr.assemble_container(b["data"], st, blob, offs, lens)
    assert not avr.seams_of_container(plain) and plain != b["avrc"]


def test_assembly_without_seams_is_unchanged():
    data, avrc = (FIX / "realshort.mp4").read_bytes(), _container("realshort.mp4", 0)
    ps = avr.parse_stream(data)
    info, _ = avr.describe_container(avrc)
    blocks = [x for x in info["blocks"] if "literal" not in x]
    cabac = [bytes.fromhex(x.get("cabac", "")) for x in blocks]
    st = np.array([0 if "cabac" in x else -1 for x in blocks])
    lens = np.array([len(c) for c in cabac])
    offs = np.cumsum(lens) - lens
    blob = b"".join(cabac) + b"\0"
    assert avr.assemble_container(data, st, blob, offs, lens, seams=None) == avrc
    assert avr.assemble_container(data, st, blob, offs, lens, ps=ps, seams=None) == avrc
    assert avr.assemble_container(data, st, blob, offs, lens, ps=ps, seams=[b""] * len(st)) == avrc
    assert avr.assemble_container(data, st, blob, offs, lens, seams=[b""] * len(st)) == avrc


def test_assembly_refuses_seams_where_the_format_has_none():
    b = _batch("realshort.mp4", 1024)
    st, blob, offs, lens = _outputs(b)
    for kw in (dict(), dict(ps=b["ps"])):
        for model in (avr.MODEL_PARALLEL32, avr.MODEL_CHAINED):
            with pytest.raises(avr.AvrError) as e:
                avr.assemble_container(b["data"], st, blob, offs, lens, model=model, seams=b["fields"], **kw)
            assert e.value.code == -1
            # no field, no objection
            avr.assemble_container(b["data"], st, blob, offs, lens, model=model, seams=[b""] * len(st), **kw)
        k = next(i for i, f in enumerate(b["fields"]) if f)
        off = st.copy()
        off[k] = -1   # a seams field on a slice that is not coded
        with pytest.raises(avr.AvrError) as e:
            avr.assemble_container(b["data"], off, blob, offs, lens, seams=b["fields"], **kw)
        assert e.value.code == -1
        # a field outside the blob
        sl = np.array([len(f) for f in b["fields"]], np.uint32)
        so = np.cumsum(sl, dtype=np.uint64) - sl
        with pytest.raises(avr.AvrError) as e:
            avr.assemble_container(b["data"], st, blob, offs, lens,
                                   seams=(np.frombuffer(b"".join(b["fields"]), np.uint8)[:-1], so, sl), **kw)
        assert e.value.code == -1


def test_select_is_subset_for_a_list_of_indices():
    ps = avr.parse_stream((FIX / "realshort.mp4").read_bytes())
    idx = [5, 2, 17, 30]
    sub = shard.select(ps, idx)
    assert len(sub.descs) == 4 and sub.max_mb_height == ps.max_mb_height
    for d, k in zip(sub.descs, idx):
        o, n = int(d["payload_offset"]), int(d["read_limit"])
        s = int(ps.descs[k]["payload_offset"])
        assert o % 16 == 0 and sub.arena[o:o + n].tobytes() == ps.arena[s:s + n].tobytes()
        assert not sub.arena[o + n:o + n + 16].any()
        assert int(d["out_offset"]) % 16 == 0 and int(d["out_offset"]) + int(d["out_capacity"]) <= sub.work_len
        for f in ("payload_size", "first_mb", "mb_width", "slice_type", "slice_qp", "picture_id", "coded"):
            assert d[f] == ps.descs[k][f]
    ends = sub.descs["out_offset"].astype(np.int64) + sub.descs["out_capacity"]
    assert (sub.descs["out_offset"][1:] >= ends[:-1]).all()
    whole = shard.select(ps, range(len(ps.descs)))
    assert whole.descs["payload_size"].tolist() == ps.descs["payload_size"].tolist()
    assert len(shard.select(ps, []).descs) == 0
    # an MBAFF stream: the ring of the coded slices selected, not the stream's
    mb = avr.parse_stream((FIX / "mbaff_ib.264").read_bytes())
    assert shard.select(mb, range(len(mb.descs))).max_mb_width == mb.max_mb_width


def _gloo_compress_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        b = _batch("realshort.mp4", 1024)
        lo, hi = shard.partition(b["ps"].descs["payload_size"], world)[rank]

        def run_range(part):   # stands in for this rank's device compress, check and seams
            assert len(part.descs) == hi - lo
            st, blob, offs, lens = _outputs(b, lo, hi)
            return torch.from_numpy(blob.copy()), st, offs, lens, b["fields"][lo:hi]

        out = shard.sharded_compress(None, b["data"], split_bytes=1024, run_range=run_range)
        if rank == 0:
            with open(os.path.join(outdir, "out.bin"), "wb") as f:
                f.write(out)
        else:
            assert out is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_gloo_sharded_compress_gives_the_split_container(world):
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_gloo_compress_worker, args=(world, port, td), nprocs=world, join=True)
        out = open(os.path.join(td, "out.bin"), "rb").read()
    assert out == _container("realshort.mp4", 1024)
