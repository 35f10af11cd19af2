"""Piece plans on the device (avr_decompress_pieces, avr_pack_pieces; batch.UnitBatch,
shard.decompress_units_range, the unit path of shard.sharded_decompress): a container whose long
slices the whole-file compress cut into pieces (Context.split_bytes), planned by units, regenerated
unit by unit from device-resident descriptors and seam records, packed and spliced.

* every unit of realshort.mp4's containers at split 1024 and 2048 regenerates its own span of its
  slice's payload (the cuts read from the seams fields by tests/test_piece_plan_host.py's decoder),
  and the splice equals the file and the whole-file decompress;
* avr_pack_pieces against numpy, also with one piece asked for more than it regenerated;
* avr_decompress_pieces refuses a record index outside the batch's and a picture wider than a record;
* shard.sharded_decompress at world 1 over RCCL restores the fixtures' split containers and the
  4K 4:4:4 intra slice's at the default split (AVR_ERR_UNSUPPORTED before piece plans);
* at worlds 2 and 3 over gloo, one process per rank, a slice's pieces come from every rank;
* a P32 container and an uncut one still take the slice path."""
import os
import socket
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import pytest

from _oracle import ROOT
from test_piece_plan_host import KEEP_ALL, _seams, expected_units

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402
from avrecode_amd.batch import UnitBatch  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
DATA = (FIX / "realshort.mp4").read_bytes()
# test_gpu_split.py's wide case: one 4K 4:4:4 intra slice, 240 macroblocks wide
WIDE = avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                       transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1)
# one picture, one intra slice, cut into several pieces at split 700
ONE_SLICE = avr.SynthParams(mb_width=40, mb_height=23, slice_type=2, slice_qp=24, chroma_format_idc=1, seed=904,
                            slices_per_picture=1, gop_length=1)


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    yield c
    c.close()


def _compress(ctx, data, split_bytes, model=avr.MODEL_PARALLEL):
    ctx.split_bytes = split_bytes
    try:
        return ctx.compress(data, model)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT


@pytest.fixture(scope="module", params=[1024, 2048])
def run(ctx, request):
    """realshort.mp4's split container with all its units in one range, decompressed and packed once."""
    avrc = _compress(ctx, DATA, request.param)
    n_slices, units, _ = expected_units(DATA, avrc, _compress(ctx, DATA, 0))
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    assert plan.n_slices == n_slices and plan.n_units == len(units) > n_slices
    b = UnitBatch(ctx, plan.parsed_units())
    b.decompress(avr.MODEL_PARALLEL)
    packed = [t.cpu().numpy() for t in b.pack()]
    torch.cuda.synchronize()
    return dict(avrc=avrc, units=units, plan=plan, batch=b, packed=packed, res=b.results(),
                work=b.d_work.cpu().numpy())


def _pack_reference(descs, pieces, res, work):
    """avr_pack_pieces in numpy: (offsets[n + 1], kept, status, bytes)."""
    kept, status = np.zeros(len(descs), np.int64), np.zeros(len(descs), np.int64)
    for k, (p, r) in enumerate(zip(pieces, res)):
        if r["status"] != 0:
            status[k] = r["status"]
        elif p["keep"] == KEEP_ALL:
            kept[k] = r["out_len"]
        elif r["out_len"] >= p["keep"]:
            kept[k] = p["keep"]
        else:
            status[k] = -9
    chunks = [work[int(d["out_offset"]):int(d["out_offset"]) + int(kept[k])] for k, d in enumerate(descs)]
    return np.concatenate([[0], np.cumsum(kept)]), kept, status, np.concatenate(chunks)


def test_every_unit_regenerates_its_span(ctx, run):
    units, plan = run["units"], run["plan"]
    packed, offs, kept, status = run["packed"]
    n = len(units)
    kept = kept[:n].view(np.uint32)
    assert (status[:n] == 0).all() and (run["res"]["status"] == 0).all()
    for k, u in enumerate(units):
        got = packed[int(offs[k]):int(offs[k]) + int(kept[k])].tobytes()
        if u["keep"] != KEEP_ALL:
            assert got == u["true"], k
        else:   # a slice's end: its final byte is the patch's (recode.cpp:1345-1356)
            assert len(got) in (len(u["true"]) - 1, len(u["true"])) and got[:len(u["true"]) - 1] == u["true"][:-1], k
    st, so, sl = shard.collapse_units(plan.pieces, status[:n], offs[:n], kept)
    out = plan.splice(st, packed, so, sl).tobytes()
    assert out == DATA and out == ctx.decompress(run["avrc"])
    # the same through the rank's entry point
    flat, st2, offs2, lens2 = shard.decompress_units_range(ctx, plan.parsed_units())
    assert (st2 == 0).all() and (offs2 == offs[:n]).all() and (lens2 == kept).all()
    assert (flat.cpu().numpy()[:int(offs[n])] == packed[:int(offs[n])]).all()


def test_pack_pieces_against_numpy(run):
    b, res, work = run["batch"], run["res"], run["work"]
    descs, pieces, n = b.part.descs, b.part.pieces, b.n
    packed, offs, kept, status = run["packed"]
    want = _pack_reference(descs, pieces, res, work)
    assert (offs == want[0]).all() and (kept[:n].view(np.uint32) == want[1]).all() and (status[:n] == want[2]).all()
    assert (packed[:len(want[3])] == want[3]).all()
    assert len({int(o) % 16 for o in offs[:n]}) > 4   # destinations of many alignments
    # one piece asked for more than it regenerated: it alone fails, with nothing kept
    k = int(np.flatnonzero(pieces["keep"] != KEEP_ALL)[1])
    more = pieces.copy()
    more["keep"][k] = res["out_len"][k] + 1
    packed2, offs2, kept2, status2 = (t.cpu().numpy() for t in b.pack(more))
    kept2 = kept2[:n].view(np.uint32)
    assert status2[k] == -9 and kept2[k] == 0
    others = np.arange(n) != k
    assert (status2[:n][others] == 0).all() and (kept2[others] == want[1][others]).all()
    want2 = _pack_reference(descs, more, res, work)
    assert (offs2 == want2[0]).all() and (packed2[:len(want2[3])] == want2[3]).all()


def test_decompress_pieces_checks_its_arguments(ctx, run):
    b = run["batch"]
    part = b.part
    idx = np.flatnonzero(b.is_piece)
    dd = b.d_desc[torch.from_numpy(idx).to(b.device)].contiguous()
    dr = torch.zeros(len(idx), avr.SLICE_RESULT.itemsize, dtype=torch.uint8, device=b.device)
    width = int(part.descs["mb_width"].max())
    args = lambda pc, w: (dd, pc, len(idx), w, part.max_mb_height, b.d_recs, b.n_recs, part.rec_stride,  # noqa: E731
                          b.d_in, b.d_work, dr)
    bad = part.pieces[idx].copy()
    bad["seam"][-1] = b.n_recs
    for a in (args(bad, width), args(part.pieces[idx], 289)):
        with pytest.raises(avr.AvrError) as e:
            ctx.decompress_pieces(*a)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert not dr.any()   # nothing ran


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


@pytest.mark.parametrize("case", ["realshort@1024", "realshort@2048", "4k444@default"])
def test_sharded_decompress_world1_rccl(ctx, world1, case):
    """Fails without piece plans: the per-slice plan refuses these containers (AVR_ERR_UNSUPPORTED)."""
    if case == "4k444@default":
        data, split_bytes = ctx.synthesize(WIDE, 1), avr.SPLIT_BYTES_DEFAULT
    else:
        data, split_bytes = DATA, int(case.split("@")[1])
    avrc = _compress(ctx, data, split_bytes)
    cut = avr.seams_of_container(avrc)
    assert cut and (case != "4k444@default" or len(cut) == 1)
    assert shard.sharded_decompress(ctx, avrc) == data


@pytest.mark.parametrize("case", ["P32", "uncut"])
def test_containers_without_seams_take_the_slice_path(ctx, world1, case, monkeypatch):
    def no_units(*a):
        raise AssertionError("the unit path was taken")
    monkeypatch.setattr(shard, "_sharded_decompress_units", no_units)
    avrc = _compress(ctx, DATA, 1024, avr.MODEL_PARALLEL32) if case == "P32" else _compress(ctx, DATA, 0)
    assert not avr.seams_of_container(avrc)
    assert shard.sharded_decompress(ctx, avrc) == DATA


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["realshort@1024", "one_slice@700"])
def test_sharded_decompress_multirank_gloo(ctx, case, world):
    """One process per rank, each regenerating its range of units on the device (all on cuda:0 here),
    gathered to rank 0 over gloo.  The one-slice stream's pieces land on every rank."""
    split_bytes = int(case.split("@")[1])
    data = DATA if case.startswith("realshort") else ctx.synthesize(ONE_SLICE, 1)
    if case.startswith("one_slice"):
        info, _ = avr.describe_container(_compress(ctx, data, split_bytes))
        cut = [b for b in info["blocks"] if "seams" in b]
        assert len(cut) == 1 and len([b for b in info["blocks"] if "cabac" in b]) == 1
        assert len(_seams(bytes.fromhex(cut[0]["seams"]))[1]) >= 3
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
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).parent / "_pieces_worker.py"),
                                           str(src), str(split_bytes), str(dst)], env=env))
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
        assert dst.read_bytes() == data
