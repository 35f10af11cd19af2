"""Checked containers on the device (Context.checksums; avr_k_crc.hip, avr_crc_spans; Metadata field
16; AVR_ERR_CHECKSUM).  Without the feature every test here fails at ctx.checksums or ctx.crc_spans.

* avr_crc_spans against zlib.crc32 at every length where the chunking, the tables or the fold change
  behaviour, at all 16 start alignments, with overlapping spans, a span past the buffer, no span, and
  more workgroups than are resident;
* whole files of every model: the field is zlib.crc32(file), the container minus the field is the
  option-off container, decompress restores the file;
* damage: the single-bit flips of tests/test_checksum_host.py's control, on the checked container, never
  give a wrong file; a flipped literal byte and a flipped stored CRC byte are refused;
* split containers (P64 and P32S at 1024): a byte flipped inside a piece fails the file -- the u64
  case that passes unnoticed without the field;
* escaped blocks; the sharded paths at world 1 (RCCL) and world 2 (gloo)."""
import os
import socket
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np
import pytest

from _oracle import ROOT
from test_checksum_host import flips, strip_crc
from test_piece_plan_host import _seams

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
ERR_FORMAT, ERR_CHECKSUM = -3, -7
MODELS = {"R": avr.MODEL_REFERENCE, "P": avr.MODEL_PARALLEL, "P32": avr.MODEL_PARALLEL32, "C": avr.MODEL_CHAINED}
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65541, 300007)


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    c.checksums = True
    yield c
    c.close()


@pytest.fixture(scope="module")
def realshort():
    return (FIX / "realshort.mp4").read_bytes()


def _compress(ctx, data, model, split_bytes=0, checksums=True):
    ctx.split_bytes, ctx.checksums = split_bytes, checksums
    try:
        return ctx.compress(data, model)
    finally:
        ctx.split_bytes, ctx.checksums = avr.SPLIT_BYTES_DEFAULT, True


# ------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def buffer():
    host = np.random.default_rng(16).integers(0, 256, 1 << 20, dtype=np.uint8)
    return host, torch.from_numpy(host).cuda()


def _spans(ctx, d_buf, buf_len, off, ln):
    n = len(off)
    d_off = torch.tensor(off, dtype=torch.int64).cuda() if n else torch.zeros(1, dtype=torch.int64).cuda()
    d_len = torch.from_numpy(np.array(ln, dtype=np.uint32).view(np.int32).copy()).cuda() if n else \
        torch.zeros(1, dtype=torch.int32).cuda()
    d_crc = torch.full((max(1, n),), 0x5A5A5A5A, dtype=torch.int32).cuda()
    d_status = torch.full((max(1, n),), 77, dtype=torch.int32).cuda()
    ctx.crc_spans(d_buf, buf_len, d_off, d_len, n, d_crc, d_status)
    torch.cuda.synchronize()
    return d_crc.cpu().numpy().view(np.uint32)[:max(1, n)], d_status.cpu().numpy()[:max(1, n)]


def test_crc_spans_against_zlib(ctx, buffer):
    host, dev = buffer
    off, ln = [], []
    at = 0
    for n in LENGTHS:           # every length at the 16 alignments of its start, one after the other
        for a in range(16):
            o = ((at + 15) & ~15) + a
            off.append(o)
            ln.append(n)
            at = o + min(n, 4099)   # the long ones overlap their neighbours: spans need not be disjoint
    off += [1000, 1100]         # two overlapping spans
    ln += [500, 700]
    off += [0, 5, (1 << 20) - 70000, (1 << 20) - 1]    # the whole buffer, its ends
    ln += [1 << 20, (1 << 20) - 5, 70000, 1]
    over = len(off)
    off += [(1 << 20) - 99, 40]                         # one byte past buf_len; and a good neighbour after it
    ln += [100, 41]
    assert max(o + n for o, n in zip(off[:over], ln[:over])) <= 1 << 20
    crc, status = _spans(ctx, dev, 1 << 20, off, ln)
    for k, (o, n) in enumerate(zip(off, ln)):
        if k == over:
            assert (int(status[k]), int(crc[k])) == (avr.SLICE_OVERFLOW, 0)
        else:
            assert (int(status[k]), int(crc[k])) == (0, zlib.crc32(host[o:o + n])), (k, o, n)


def test_crc_spans_at_the_buffers_ends(ctx, buffer):
    """A buffer that neither starts nor ends on a 16-byte boundary: the bytes of the first and last
    partial blocks are read by bytes, and a span may start at the first and end at the last."""
    host, dev = buffer
    view, n = dev[3:3 + 100001], 100001
    off = [0, 0, 1, 13, n - 1, n - 17, n - 40, 0, n]
    ln = [n, 1, 15, 16, 1, 17, 40, 0, 0]
    crc, status = _spans(ctx, view, n, off, ln)
    for k, (o, m) in enumerate(zip(off, ln)):
        assert (int(status[k]), int(crc[k])) == (0, zlib.crc32(host[3 + o:3 + o + m])), (k, o, m)
    crc, status = _spans(ctx, view, n, [n + 1, n - 3], [0, 4])
    assert list(status) == [avr.SLICE_OVERFLOW] * 2 and list(crc) == [0, 0]


def test_crc_spans_without_spans_and_past_residency(ctx, buffer):
    host, dev = buffer
    crc, status = _spans(ctx, dev, 1 << 20, [], [])
    assert (int(crc[0]), int(status[0])) == (0x5A5A5A5A, 77)   # n = 0 launches nothing
    rng = np.random.default_rng(7)
    ln = [k % 41 for k in range(5000)]
    off = [int(x) for x in rng.integers(0, (1 << 20) - 64, 5000)]
    crc, status = _spans(ctx, dev, 1 << 20, off, ln)
    want = np.array([zlib.crc32(host[o:o + n]) for o, n in zip(off, ln)], np.uint32)
    assert not status.any() and (crc == want).all()


# ------------------------------------------------------------------ whole files
@pytest.mark.parametrize("mode", sorted(MODELS))
def test_whole_files_carry_and_check_the_crc(ctx, realshort, mode):
    data, model = realshort, MODELS[mode]
    avrc = _compress(ctx, data, model)
    plain = _compress(ctx, data, model, checksums=False)
    info, again = avr.describe_container(avrc)
    assert info["file_crc"] == zlib.crc32(data) and again == avrc
    assert "file_crc" not in avr.describe_container(plain)[0]
    assert len(avrc) == len(plain) + (8 if mode == "R" else 6) and strip_crc(avrc) == plain
    assert ctx.decompress(avrc) == data
    assert ctx.compress_files([data, data], model) == [avrc, avrc]
    assert ctx.decompress_files([avrc, plain]) == [data, data]
    back, _ = ctx.roundtrip(data, model)
    assert back == avrc
    # the stored value, one byte of it
    bad = bytearray(avrc)
    bad[2 + avrc[1] - 2] ^= 0x10
    with pytest.raises(avr.AvrError) as e:
        ctx.decompress(bytes(bad))
    assert e.value.code == ERR_CHECKSUM
    # one file of a batch fails alone
    got = ctx.decompress_files([avrc, bytes(bad), avrc])
    assert got[0] == data and got[2] == data and isinstance(got[1], avr.AvrError) and got[1].code == ERR_CHECKSUM


def test_the_default_is_off_and_the_environment_turns_it_on(realshort):
    with avr.Context(0) as c:
        assert c.checksums is False
        assert "file_crc" not in avr.describe_container(c.compress(realshort, avr.MODEL_PARALLEL))[0]
    os.environ["AVR_CHECKSUMS"] = "1"
    try:
        with avr.Context(0) as c:
            assert c.checksums is True
    finally:
        del os.environ["AVR_CHECKSUMS"]


# ------------------------------------------------------------------ damage
def test_flipped_bits_never_give_a_wrong_file(ctx, realshort):
    data = realshort
    avrc = _compress(ctx, data, avr.MODEL_PARALLEL)
    codes = []
    for i, where, damaged in flips(avrc):
        try:
            assert ctx.decompress(damaged) == data, (i, where)
            codes.append(0)
        except avr.AvrError as e:
            codes.append(e.code)
    assert len(codes) == 36
    print("flips:", {c: codes.count(c) for c in sorted(set(codes))})
    assert ERR_CHECKSUM in codes
    # a literal byte (the MP4's major brand: the parse does not read it)
    lit = bytes.fromhex(avr.describe_container(avrc)[0]["blocks"][0]["literal"])
    at = avrc.find(lit)
    assert at > 0 and lit[4:8] == b"ftyp"
    bad = bytearray(avrc)
    bad[at + 9] ^= 0x10
    with pytest.raises(avr.AvrError) as e:
        ctx.decompress(bytes(bad))
    assert e.value.code == ERR_CHECKSUM
    assert ctx.decompress(strip_crc(bytes(bad))) != data   # unchecked, the same damage passes


@pytest.mark.parametrize("mode", ["P", "P32"])
def test_a_damaged_piece_fails_the_file(ctx, realshort, mode):
    data, model = realshort, MODELS[mode]
    ctx.split_p32 = True
    try:
        avrc = _compress(ctx, data, model, split_bytes=1024)
    finally:
        ctx.split_p32 = False
    assert avr.seams_of_container(avrc) and avr.describe_container(avrc)[0]["file_crc"] == zlib.crc32(data)
    assert ctx.decompress(avrc) == data
    cut = next(b for b in avr.describe_container(avrc)[0]["blocks"] if "seams" in b)
    cabac = bytes.fromhex(cut["cabac"])
    piece_len = _seams(bytes.fromhex(cut["seams"]))[1]
    at = avrc.find(cabac)
    assert at > 0 and len(piece_len) >= 2
    for where in (piece_len[0] // 2, len(cabac) - piece_len[-1] // 2 - 1):   # the first piece, the last
        bad = bytearray(avrc)
        bad[at + where] ^= 0x10
        with pytest.raises(avr.AvrError) as e:
            ctx.decompress(bytes(bad))
        assert e.value.code in (ERR_CHECKSUM, ERR_FORMAT), where


def test_escaped_blocks_are_covered(ctx):
    data = (FIX / "cockatoo.mp4").read_bytes()
    ctx.recode_escaped = True
    try:
        avrc = _compress(ctx, data, avr.MODEL_PARALLEL)
    finally:
        ctx.recode_escaped = False
    info = avr.describe_container(avrc)[0]
    assert any("escapes" in b for b in info["blocks"]) and info["file_crc"] == zlib.crc32(data)
    assert ctx.decompress(avrc) == data


def test_hooks_decompress_session_checks_the_file(ctx, realshort):
    from test_hooks import _call
    avrc = _compress(ctx, realshort, avr.MODEL_PARALLEL)
    r, back, walked = _call("hooks_decompress", avrc, len(avrc))
    assert r == 0 and back == realshort
    bad = bytearray(avrc)
    bad[2 + avrc[1] - 1] ^= 1
    assert _call("hooks_decompress", bytes(bad), len(bad))[0] == ERR_CHECKSUM


def test_cli_k_switch(realshort, tmp_path):
    cli = ROOT / "avrecode_amd" / "recode"
    src, out, back = tmp_path / "in.mp4", tmp_path / "out.avrc", tmp_path / "back.mp4"
    src.write_bytes(realshort)
    for flags in (["-p", "-k"], ["-k"], ["-k", "-p32"]):
        r = subprocess.run([str(cli), "compress"] + flags + [str(src), str(out)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        avrc = out.read_bytes()
        assert avr.file_crc_of_container(avrc) == zlib.crc32(realshort)
        r = subprocess.run([str(cli), "decompress", str(out), str(back)], capture_output=True, timeout=120)
        assert r.returncode == 0 and back.read_bytes() == realshort
    r = subprocess.run([str(cli), "roundtrip", "-p", "-k", str(src)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    bad = bytearray(avrc)
    bad[2 + avrc[1] - 1] ^= 1
    out.write_bytes(bytes(bad))
    r = subprocess.run([str(cli), "decompress", str(out), str(back)], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"(-7)" in r.stderr


# ------------------------------------------------------------------ sharded
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


def test_sharded_world1_rccl(ctx, world1, realshort):
    data = realshort
    plain = _compress(ctx, data, avr.MODEL_PARALLEL)
    split = _compress(ctx, data, avr.MODEL_PARALLEL, split_bytes=1024)
    assert shard.sharded_compress(ctx, data, checksums=ctx.checksums) == plain
    assert shard.sharded_compress(ctx, data, split_bytes=1024, checksums=True) == split
    assert shard.sharded_compress(ctx, data) == strip_crc(plain)
    assert shard.sharded_decompress(ctx, plain) == data
    assert shard.sharded_decompress(ctx, split) == data
    for avrc in (plain, split):
        c = bytes.fromhex(next(b for b in avr.describe_container(avrc)[0]["blocks"] if "cabac" in b)["cabac"])
        bad = bytearray(avrc)
        bad[avrc.find(c) + len(c) // 2] ^= 0x10
        with pytest.raises(avr.AvrError) as e:
            shard.sharded_decompress(ctx, bytes(bad))
        assert e.value.code in (ERR_CHECKSUM, ERR_FORMAT)


def test_collapse_unit_crcs_folds_the_pieces(ctx, realshort):
    """The device's per-unit values over the packed outputs, folded: the CRC of each slice's bytes."""
    from avrecode_amd.batch import UnitBatch
    split = _compress(ctx, realshort, avr.MODEL_PARALLEL, split_bytes=1024)
    plan = avr.DecompressPlan().load(split, pieces=True)
    b = UnitBatch(ctx, plan.parsed_units())
    b.decompress(avr.MODEL_PARALLEL)
    d_packed, d_off, d_kept, d_status = b.pack()
    d_crc, d_st = b.crcs(d_packed, d_off, d_kept)
    torch.cuda.synchronize()
    assert not d_status.cpu().numpy().any() and not d_st.cpu().numpy().any()
    offs = d_off.cpu().numpy()[:b.n]
    lens = d_kept.cpu().numpy()[:b.n].view(np.uint32).astype(np.int64)
    packed = d_packed.cpu().numpy()
    crcs = d_crc.cpu().numpy()[:b.n].view(np.uint32)
    assert [int(c) for c in crcs] == [zlib.crc32(packed[o:o + n]) for o, n in zip(offs, lens)]
    st, so, sl = shard.collapse_units(plan.pieces, np.zeros(b.n, np.int64), offs, lens)
    got = shard.collapse_unit_crcs(plan.pieces, crcs, lens)
    assert len(got) == plan.n_slices < b.n
    assert [int(c) for c in got] == [zlib.crc32(packed[int(o):int(o) + int(n)]) for o, n in zip(so, sl)]
    assert plan.splice(st, packed, so, sl, crcs=got).tobytes() == realshort


def test_sharded_world2_gloo(realshort):
    """One process per rank on cuda:0, gloo for the gathers (tests/_checksum_worker.py)."""
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        src, dst = Path(td) / "in.bin", Path(td) / "out.bin"
        src.write_bytes(realshort)
        procs = []
        for r in range(world):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r),
                       WORLD_SIZE=str(world), LOCAL_RANK="0")
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).parent / "_checksum_worker.py"),
                                           str(src), str(dst)], env=env))
        try:   # until every rank is done, or one has failed: the others would wait for it in the gather
            deadline = time.monotonic() + 100
            while (any(p.poll() is None for p in procs) and not any(p.poll() for p in procs)
                   and time.monotonic() < deadline):
                time.sleep(0.05)
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        assert [p.returncode for p in procs] == [0] * world
        assert dst.read_bytes() == realshort
        assert Path(str(dst) + ".split").read_bytes() == realshort
