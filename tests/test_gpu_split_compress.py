"""The split compress of slice batches on the device (avr_compress_split_slices, avr_stage_pieces,
avr_verify_units; batch.SplitBatch, shard.compress_range, shard.sharded_compress(split_bytes=...)):
a rank's long slices cut as the whole-file MODEL_PARALLEL compress cuts them, checked piece by piece
without their bytes leaving the device, their seams fields built on the host, and the container
assembled from gathered outputs equal to ctx.compress's.

Cases, the smallest where this can go wrong: one slice with several cuts; realshort.mp4 at 1024 (31
of 36 slices cut, mixed with uncut ones) and 2048 (3 cut); the 4K 4:4:4 intra slice 240 columns wide
at the default split; the seven synthetic streams of test_gpu_split.py's corpus at 700 (P / B
slices, several slices per picture starting mid-row, 4:2:2 / 4:4:4, field and MBAFF streams, which
are never cut); and the one slice exactly at the candidate threshold.

* SplitBatch.roundtrip: every verdict 1; recoded() and seams() equal the cabac and seams of the
  matching block of ctx.compress's container (which test_gpu_split.py pins to the oracle's);
* avr_stage_pieces against numpy: aligned, equal to its span of d_out, zeros after; a unit that does
  not fit the arena is refused on the device;
* avr_verify_units against numpy on doctored inputs;
* the halves stepped with a byte flipped in a middle piece's staged stream: that slice alone fails,
  and sharded_compress stores it skip_coded;
* world 1 over RCCL, every case: sharded_compress(split_bytes=s) == ctx.compress at split s (== the
  oracle's for the fixtures), and sharded_decompress of it restores the file.  On the code before
  this feature sharded_compress has no split_bytes and writes a container without seams;
* worlds 2 and 3 over gloo, one process per rank;
* split_bytes None / 0 and MODEL_PARALLEL32 give today's containers."""
import os
import socket
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import pytest

from _oracle import ROOT, oracle_cli

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import batch as avr_batch  # noqa: E402
from avrecode_amd import shard  # noqa: E402
from avrecode_amd.batch import SplitBatch  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
ONE_SLICE = avr.SynthParams(mb_width=40, mb_height=23, slice_type=2, slice_qp=24, chroma_format_idc=1, seed=904,
                            slices_per_picture=1, gop_length=1)
# test_gpu_split.py's wide stream: one 4K 4:4:4 intra slice, 240 macroblocks wide
WIDE = avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                       transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1)
# the seven specs of test_gpu_split.py::test_synthetic_corpus_split_matches_oracle
CORPUS = [(22, 18, 2, 6, 6, 1, 25, 1, 0), (14, 9, 3, 5, 5, 0, 27, 3, 0), (30, 17, 1, 4, 2, 2, 29, 2, 0),
          (11, 7, 1, 7, 4, 1, 23, 1, 0), (40, 23, 3, 4, 4, 1, 24, 1, 0), (20, 12, 1, 4, 4, 0, 26, 1, 1),
          (20, 12, 1, 4, 4, 1, 26, 1, 2)]
CASES = ["one_slice@700", "realshort@1024", "realshort@2048", "4k444@default"] + \
        [f"corpus{k}@700" for k in range(len(CORPUS))] + ["one_slice@threshold"]


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    yield c
    c.close()


_streams = {}


def _stream(ctx, case):
    """(file bytes, split_bytes, ctx.compress's container at that split) of a case, made once."""
    if case in _streams:
        return _streams[case]
    name, at = case.split("@")
    if name == "realshort":
        data = (FIX / "realshort.mp4").read_bytes()
    elif name == "one_slice":
        data = ctx.synthesize(ONE_SLICE, 1)
    elif name == "4k444":
        data = ctx.synthesize(WIDE, 1)
    else:
        k = int(name[len("corpus"):])
        w, h, spf, frames, gop, st, qp, cf, structure = CORPUS[k]
        data = ctx.synthesize(avr.SynthParams(mb_width=w, mb_height=h, slice_type=st, slice_qp=qp, chroma_format_idc=cf,
                                              seed=900 + k, slices_per_picture=spf, gop_length=gop, num_ref_idx_l0=2,
                                              structure=structure), frames)
    if at == "default":
        split = avr.SPLIT_BYTES_DEFAULT
    elif at == "threshold":   # the largest split_bytes at which the one slice is still a candidate
        split = int(avr.parse_stream(data).descs["payload_size"].max()) * 2 // 3
    else:
        split = int(at)
    ctx.split_bytes = split
    try:
        avrc = ctx.compress(data, avr.MODEL_PARALLEL)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT
    _streams[case] = (data, split, avrc)
    return _streams[case]


def _blocks(avrc):
    info, _ = avr.describe_container(avrc)
    return [b for b in info["blocks"] if "literal" not in b]


def _candidates(ps, split):
    return np.flatnonzero(avr.split_plan(ps.descs, split).candidate & (ps.descs["coded"] != 0))


_runs = {}


def _run(ctx, case):
    """A case's candidates through SplitBatch.roundtrip, once: (batch, their slice indices, the blocks
    of ctx.compress's container) -- or None where the stream has no candidate."""
    if case not in _runs:
        data, split, avrc = _stream(ctx, case)
        ps = avr.parse_stream(data)
        idx = _candidates(ps, split)
        if not len(idx):
            _runs[case] = None
        else:
            sb = SplitBatch(ctx, shard.select(ps, idx), split)
            sb.roundtrip()
            torch.cuda.synchronize()
            _runs[case] = (sb, idx, _blocks(avrc))
    return _runs[case]


@pytest.mark.parametrize("case", CASES)
def test_split_batch_roundtrip_matches_the_whole_file_compress(ctx, case):
    data, split, avrc = _stream(ctx, case)
    run = _run(ctx, case)
    if run is None:   # field and MBAFF streams: never cut, never a candidate
        assert case in ("corpus5@700", "corpus6@700") and not avr.seams_of_container(avrc)
        return
    sb, idx, blocks = run
    name = case.split("@")[0]
    if name in ("one_slice", "4k444"):
        assert len(idx) == 1 == len([b for b in blocks if "cabac" in b])
    if case == "one_slice@threshold":
        assert 2 * int(sb.ps.descs["payload_size"][0]) >= 3 * split > 2 * int(sb.ps.descs["payload_size"][0]) - 3
        assert not len(_candidates(avr.parse_stream(data), split + 1))
    v = sb.verdicts()
    assert (v == 1).all(), v
    assert (sb.d_stage_status.cpu().numpy()[:sb.nu] == 0).all()
    status, fields = sb.seams(check_cuts=True)
    assert (status == 0).all()
    assert (sb.seams(check_cuts=False)[0] == 0).all()
    recoded = sb.recoded()
    cut = 0
    for j, k in enumerate(idx):
        b = blocks[k]
        assert recoded[j] == bytes.fromhex(b["cabac"]), (case, k)
        assert fields[j] == bytes.fromhex(b.get("seams", "")), (case, k)
        assert (sb.cuts[j] > 0) == ("seams" in b)
        cut += "seams" in b
    # every cut block of the container belongs to a candidate
    assert cut == len(avr.seams_of_container(avrc))
    want = {"one_slice@700": None, "realshort@1024": 31, "realshort@2048": 3, "4k444@default": 1}.get(case)
    if want is not None:
        assert cut == want
    if case == "one_slice@700":
        assert int(sb.cuts[0]) >= 3
    if case.startswith("corpus") and run is not None:
        assert cut > 0


@pytest.mark.parametrize("case", ["one_slice@700", "realshort@1024", "4k444@default"])
def test_stage_pieces_against_numpy(ctx, case):
    sb, _, _ = _run(ctx, case)
    nu = sb.nu
    out = sb.d_out.cpu().numpy()
    arena = sb.d_arena.cpu().numpy()
    offs = sb.d_stage_off.cpu().numpy()
    src = sb.d_src.cpu().numpy()
    units = sb.d_units.cpu().numpy().view(avr.SLICE_DESC)[:nu]
    lens = sb.units["payload_size"].astype(np.int64)
    assert nu > sb.n or case != "realshort@1024"
    assert offs[0] == 0 and (np.diff(offs) == ((lens + 16 + 15) & ~15)).all() and offs[nu] <= sb.arena_cap
    for u in range(nu):
        o, n, s = int(offs[u]), int(lens[u]), int(src[u])
        assert o % 16 == 0
        assert (arena[o:o + n] == out[s:s + n]).all(), u
        assert not arena[o + n:int(offs[u + 1])].any() and int(offs[u + 1]) - (o + n) >= 16, u
        assert int(units[u]["payload_offset"]) == o and int(units[u]["read_limit"]) == n == int(units[u]["payload_size"])
    if case == "realshort@1024":
        assert len({int(s) % 16 for s in src}) > 4   # sources of many alignments
    # an arena too small for the later units, a source past the work buffer: refused on the device, unit by unit
    half = nu // 2
    cap = int(offs[half])
    d_arena = torch.zeros_like(sb.d_arena)
    d_off = torch.zeros_like(sb.d_stage_off)
    d_st = torch.zeros_like(sb.d_stage_status)
    d_units = sb.d_units.clone()
    d_src = sb.d_src.clone()
    d_src[0] = sb.work_len + 1
    ctx.stage_pieces(d_units, d_src, nu, sb.d_out, sb.work_len, d_arena, cap, d_off, d_st)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()[:nu]
    assert st[0] == -12 and (st[1:half] == 0).all() and (st[half:] == -12).all()
    a2 = d_arena.cpu().numpy()
    assert not a2[cap:].any() and not a2[:int(offs[1])].any()
    assert (a2[int(offs[1]):cap] == arena[int(offs[1]):cap]).all()
    with pytest.raises(avr.AvrError) as e:   # an arena that is not 16-byte aligned
        ctx.stage_pieces(d_units, d_src, nu, sb.d_out, sb.work_len, d_arena[1:], cap, d_off, d_st)
    assert e.value.code == -1


def _verify_reference(sb, arena, packed, offs, kept, ustatus, res_status=None):
    """avr_verify_units in numpy."""
    v = np.zeros(sb.n, np.int32)
    for k, d in enumerate(sb.descs):
        if not d["coded"] or (sb.res["status"][k] if res_status is None else res_status[k]) != 0:
            v[k] = 2
            continue
        u0, u1, size = int(sb.first[k]), int(sb.first[k + 1]), int(d["payload_size"])
        ok = u1 > u0 and all(ustatus[u] == 0 and offs[u] + kept[u] == offs[u + 1] for u in range(u0, u1))
        total = int(sum(int(kept[u]) for u in range(u0, u1)))
        if ok and size and total in (size, size - 1):
            p = int(d["payload_offset"])
            o = int(offs[u0])
            v[k] = (arena[p:p + size - 1] == packed[o:o + size - 1]).all()
    return v


def test_verify_units_against_numpy_on_doctored_inputs(ctx):
    sb, _, _ = _run(ctx, "realshort@1024")
    dev = sb.device
    n, nu = sb.n, sb.nu
    arena = sb.ps.arena
    packed = sb.d_packed.cpu().numpy()
    offs = sb.d_pack_off.cpu().numpy()
    kept = sb.d_kept.cpu().numpy().view(np.uint32)[:nu].astype(np.int64)
    ust = sb.d_unit_status.cpu().numpy()[:nu]
    pieces_of = np.diff(sb.first.astype(np.int64))
    k = int(np.flatnonzero(pieces_of >= 3)[0])   # one multi-piece slice, others after it
    assert k < n - 1
    u0, size = int(sb.first[k]), int(sb.descs[k]["payload_size"])
    o0, p0 = int(offs[u0]), int(sb.descs[k]["payload_offset"])
    total = int(kept[u0:int(sb.first[k + 1])].sum())
    assert total in (size, size - 1)
    others = np.arange(n) != k

    def verdicts(arena_h=arena, packed_h=packed, offs_h=offs, kept_h=kept, ust_h=ust, want=None):
        d_verdict = torch.full((n,), 7, dtype=torch.int32, device=dev)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).astype(t)).to(dev)  # noqa: E731
        ctx.verify_units(sb.d_desc, sb.d_res_c, n, sb.d_first, nu, up(arena_h, np.uint8), up(packed_h, np.uint8),
                         up(offs_h, np.int64), up(np.asarray(kept_h).astype(np.uint32).view(np.int32), np.int32),
                         up(ust_h, np.int32), d_verdict)
        torch.cuda.synchronize()
        v = d_verdict.cpu().numpy()
        assert (v == _verify_reference(sb, arena_h, packed_h, offs_h, kept_h, ust_h)).all()
        assert (v[others] == 1).all()   # every other slice of the batch stays bit-exact
        assert v[k] == want
        return v

    def flipped(a, at):
        b = a.copy()
        b[at] ^= 0x01
        return b

    verdicts(want=1)
    verdicts(packed_h=flipped(packed, o0), want=0)                  # the first byte
    verdicts(packed_h=flipped(packed, o0 + size - 2), want=0)       # the last compared byte
    verdicts(arena_h=flipped(arena, p0 + size - 1), want=1)         # the final byte: the patch's, not compared
    if total == size:
        verdicts(packed_h=flipped(packed, o0 + size - 1), want=1)
    # size - 2 bytes in all: the slice's last unit shortened and everything after it moved up
    ul = int(sb.first[k + 1]) - 1
    drop = total - (size - 2)
    kept2 = kept.copy()
    kept2[ul] -= drop
    offs2 = np.concatenate([[0], np.cumsum(kept2)])
    end = int(offs[ul + 1])
    packed2 = np.concatenate([packed[:end - drop], packed[end:]])
    verdicts(packed_h=packed2, offs_h=offs2, kept_h=kept2, want=0)
    # the same bytes with lengths that do not add up
    verdicts(kept_h=kept2, want=0)
    ust2 = ust.copy()
    ust2[u0 + 1] = -8                                               # one unit failed
    verdicts(ust_h=ust2, want=0)
    # a slice the compress refused: not coded
    res = sb.res.copy()
    res[k]["status"] = -5
    d_verdict = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.verify_units(sb.d_desc, torch.from_numpy(res.view(np.uint8).copy()).to(dev), n, sb.d_first, nu, sb.d_in,
                     sb.d_packed, sb.d_pack_off, sb.d_kept, sb.d_unit_status, d_verdict)
    torch.cuda.synchronize()
    v = d_verdict.cpu().numpy()
    assert v[k] == 2 and (v[others] == 1).all()


def test_compress_split_slices_checks_its_arguments(ctx):
    sb, _, _ = _run(ctx, "realshort@2048")
    p = sb.plan
    d_res = torch.zeros_like(sb.d_res_c)
    d_cuts = torch.full_like(sb.d_cuts, 7)

    def call(slots=p.slots, split=sb.split_bytes, max_w=sb.max_w, n_recs=p.n_recs, stride=p.rec_stride):
        ctx.compress_split_slices(sb.d_desc, sb.n, max_w, sb.ps.max_mb_height, sb.d_in, sb.d_out, d_res, slots, split,
                                  sb.d_recs, n_recs, stride, d_cuts, sb.d_piece_end)

    last = int(np.argmax(p.slots["first"]))
    bad = []
    for first, cap in ((int(p.slots[last]["first"]) + 1, int(p.slots[last]["cap"])), (-2, 1), (0, 0)):
        s = p.slots.copy()
        s[last] = (first, cap)
        bad.append(dict(slots=s))
    bad += [dict(n_recs=p.n_recs - 1), dict(split=0), dict(split=1 << 28), dict(max_w=289),
            dict(stride=p.rec_stride - 16), dict(max_w=0)]
    for kw in bad:
        with pytest.raises(avr.AvrError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    torch.cuda.synchronize()
    assert not d_res.any() and (d_cuts == 7).all()   # nothing ran, nothing was zeroed


def _flip_in_middle_piece(sb, k):
    u = int(sb.first[k]) + 1
    at = int(sb.d_stage_off.cpu()[u]) + int(sb.units["payload_size"][u]) // 2
    sb.d_arena[at] ^= 0x55


def test_stepping_the_halves_with_a_damaged_piece(ctx):
    data, split, _ = _stream(ctx, "realshort@1024")
    ps = avr.parse_stream(data)
    idx = _candidates(ps, split)
    sb = SplitBatch(ctx, shard.select(ps, idx), split)
    sb.compress()
    sb.read_back()
    sb.stage()
    k = int(np.flatnonzero(np.diff(sb.first.astype(np.int64)) >= 3)[0])
    _flip_in_middle_piece(sb, k)
    sb.decompress()
    sb.pack()
    sb.verify()
    torch.cuda.synchronize()
    v = sb.verdicts()
    assert v[k] == 0 and (np.delete(v, k) == 1).all()


@pytest.fixture(scope="module")
def world1():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_a_candidate_that_fails_its_check_is_stored_skip_coded(ctx, world1, monkeypatch):
    data, split, avrc = _stream(ctx, "realshort@1024")
    ps = avr.parse_stream(data)
    idx = _candidates(ps, split)
    hit = {}
    stage = SplitBatch.stage

    def damaged_stage(self, stream=None):
        stage(self, stream)
        with torch.cuda.stream(stream):
            hit["k"] = int(np.flatnonzero(np.diff(self.first.astype(np.int64)) >= 3)[0])
            _flip_in_middle_piece(self, hit["k"])

    monkeypatch.setattr(avr_batch.SplitBatch, "stage", damaged_stage)
    out = shard.sharded_compress(ctx, data, split_bytes=split)
    k = int(idx[hit["k"]])
    got, want = _blocks(out), _blocks(avrc)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if i == k:
            assert g.get("skip_coded") is True and "cabac" not in g and "seams" not in g and "cabac" in w
        else:
            assert g == w, i
    assert ctx.decompress(out) == data


@pytest.mark.parametrize("case", CASES)
def test_sharded_compress_world1_rccl_equals_the_whole_file_compress(ctx, world1, case):
    """Fails on the code before the split compress of slice batches: sharded_compress had no
    split_bytes, and its container of a file with long slices has no seams."""
    data, split, avrc = _stream(ctx, case)
    out = shard.sharded_compress(ctx, data, split_bytes=split)
    assert out == avrc
    name = case.split("@")[0]
    if name == "realshort":
        assert out == oracle_cli("compress", FIX / "realshort.mp4", mode="P", split_bytes=split)
    if name not in ("corpus5", "corpus6"):
        assert avr.seams_of_container(out) or case == "one_slice@threshold"
    ctx.split_bytes = split
    try:   # the call the issue names: the context's own split size
        assert shard.sharded_compress(ctx, data, split_bytes=ctx.split_bytes) == ctx.compress(data, avr.MODEL_PARALLEL)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT
    assert shard.sharded_decompress(ctx, out) == data


def test_unchanged_paths(ctx, world1):
    data = (FIX / "realshort.mp4").read_bytes()
    ctx.split_bytes = 0
    try:
        plain = ctx.compress(data, avr.MODEL_PARALLEL)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT
    assert not avr.seams_of_container(plain)
    assert shard.sharded_compress(ctx, data) == plain
    assert shard.sharded_compress(ctx, data, split_bytes=None) == plain
    assert shard.sharded_compress(ctx, data, split_bytes=0) == plain
    p32 = shard.sharded_compress(ctx, data, model=avr.MODEL_PARALLEL32, split_bytes=1024)
    assert not avr.seams_of_container(p32)
    ctx.split_bytes = 1024
    try:
        assert p32 == ctx.compress(data, avr.MODEL_PARALLEL32)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["realshort@1024", "one_slice@700"])
def test_sharded_compress_multirank_gloo(ctx, case, world):
    """One process per rank, each compressing its slice range on the device (all on cuda:0 here), the
    re-coded bytes and the seams fields gathered to rank 0 over gloo."""
    data, split, avrc = _stream(ctx, case)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        src, dst = Path(td) / "in.bin", Path(td) / "out.bin"
        src.write_bytes(data)
        procs = []
        for r in range(world):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r),
                       WORLD_SIZE=str(world), LOCAL_RANK="0")
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).parent / "_split_compress_worker.py"),
                                           str(src), str(split), str(dst)], env=env))
        try:   # until every rank is done, or one has failed: the others would wait for it in the gather
            deadline = time.monotonic() + 100
            while (any(p.poll() is None for p in procs) and not any(p.poll() for p in procs)
                   and time.monotonic() < deadline):
                time.sleep(0.05)
        finally:
            for p in procs:   # a rank that failed or ran out of time leaves none behind
                if p.poll() is None:
                    p.kill()
                    p.wait()
        assert [p.returncode for p in procs] == [0] * world
        assert dst.read_bytes() == avrc
