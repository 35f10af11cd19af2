"""The long-slice split on the P32 coder (Context.split_p32; avr_k_split32.hip; the tags
avrecode-amd:P32S / P32SE), on the device.  Without the feature every test here fails at
ctx.split_p32.

The oracle does not restate a P32 split, so the format is held to what is already pinned:
* the cuts of a P32S container are the P64 container's (which test_gpu_split.py holds to the oracle):
  same cut blocks, same seams fields outside the pieces' lengths;
* the first piece of every cut slice is a prefix of the oracle's whole-slice P32 stream, up to the
  bytes the encoder's finish can still change;
* every unit of the piece plan regenerates its own span of the payload;
and everything roundtrips: whole files, batches, mixed batches, sharded, CLI."""
import os
import socket
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np
import pytest

from _oracle import ROOT, slices_p
from test_piece_plan_host import KEEP_ALL, _seams, expected_units

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402
from avrecode_amd.batch import UnitBatch  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
CLI = ROOT / "avrecode_amd" / "recode"
P32, P64 = avr.MODEL_PARALLEL32, avr.MODEL_PARALLEL
TAG, TAG_S, TAG_SE = b"avrecode-amd:P32", b"avrecode-amd:P32S", b"avrecode-amd:P32SE"
# test_gpu_pieces.py's streams: one 4K 4:4:4 intra slice, 240 macroblocks wide; one small intra slice
WIDE = avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                       transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1)
ONE_SLICE = avr.SynthParams(mb_width=40, mb_height=23, slice_type=2, slice_qp=24, chroma_format_idc=1, seed=904,
                            slices_per_picture=1, gop_length=1)


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    c.split_p32 = True
    yield c
    c.close()


def _compress(ctx, data, split_bytes, model=P32):
    ctx.split_bytes = split_bytes
    try:
        return ctx.compress(data, model)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT


def _tag(avrc):
    return bytes.fromhex(avr.describe_container(avrc)[0]["version"])


def _coded(avrc):
    return [b for b in avr.describe_container(avrc)[0]["blocks"] if "cabac" in b or "skip_coded" in b]


def _raw(field_hex):
    f = bytes.fromhex(field_hex)
    raw = zlib.decompress(f[4:])
    assert len(raw) == struct.unpack_from("<I", f, 0)[0]
    return raw


# The bytes of a piece that the encoder's finish can still change, counted from its end (PEncoder,
# avr_engine.h re_finish / pe_shift).  At a cut the encoder holds: digits already written (final: a
# carry reaches only the cache byte and the 0xFF run behind it), one cache byte, `pending` deferred
# 0xFF digits, and a low of 32 bits + carry.  finish picks a value in [low, low + range) and shifts
# while low != 0: every shift drops the top 8 of the 32 bits, so at most 4 flush digits; then the
# cache byte and the run go out.  A carry out of the flush turns cache into cache + 1 and the run's
# 0xFF into 0x00.  From the end of the stream: <= 4 flush digits, then the run (every byte 0xFF or
# 0x00), then the cache byte.  The whole-slice encoder goes on instead, so it agrees with the piece on
# everything before that: strip 4 bytes, then every trailing 0xFF / 0x00 byte, then 1.  (Stripping a
# byte too many only shortens the compared prefix.)
def _stable_prefix(piece: bytes) -> bytes:
    p = piece[:-4]
    while p and p[-1] in (0xFF, 0x00):
        p = p[:-1]
    return p[:-1]


@pytest.fixture(scope="module", params=[("realshort.mp4", 512), ("realshort.mp4", 2048), ("cockatoo.mp4", 512),
                                        ("cockatoo.mp4", 2048)], ids=lambda p: f"{p[0]}@{p[1]}")
def fix(ctx, request):
    name, split_bytes = request.param
    data = (FIX / name).read_bytes()
    return dict(name=name, data=data, split=split_bytes, avrc=_compress(ctx, data, split_bytes),
                p64=_compress(ctx, data, split_bytes, P64), plain=_compress(ctx, data, 0))


def test_fixture_is_split_tagged_and_restored(ctx, fix):
    data, avrc = fix["data"], fix["avrc"]
    assert avr.seams_of_container(avrc) and _tag(avrc) == TAG_S and avr.container_model(avrc) == P32
    assert ctx.decompress(avrc) == data
    ctx.split_bytes = fix["split"]
    try:
        assert ctx.compress_files([data, data], P32) == [avrc, avrc]
        back, _ = ctx.roundtrip_files([data], P32)   # unchecked first pass
        assert back == [avrc]
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT


def test_cuts_are_the_p64_containers(fix):
    """A cut is placed from the CABAC decoder's state and the payload alone: the same blocks are cut
    and every seams field equals the P64 container's outside piece_len[] (bytes 12 .. 12 + 4 (cuts + 1)
    of the inflated field)."""
    a, b = _coded(fix["avrc"]), _coded(fix["p64"])
    assert len(a) == len(b)
    assert [("seams" in x) for x in a] == [("seams" in y) for y in b]
    n = 0
    for x, y in zip(a, b):
        if "seams" not in x:
            continue
        rx, ry = _raw(x["seams"]), _raw(y["seams"])
        cuts = struct.unpack_from("<I", rx, 4)[0]
        lo, hi = 12, 12 + 4 * (cuts + 1)
        assert len(rx) == len(ry) and rx[:lo] == ry[:lo] and rx[hi:] == ry[hi:]
        assert sum(struct.unpack_from(f"<{cuts + 1}I", rx, 12)) == len(x["cabac"]) // 2
        n += 1
    assert n > 0


def test_first_pieces_are_prefixes_of_the_oracles_p32_streams(fix):
    _, recs = slices_p(fix["data"], p32=True)
    blocks = _coded(fix["avrc"])
    assert len(blocks) == len(recs)
    n = 0
    for b, r in zip(blocks, recs):
        if "seams" not in b:
            continue
        _, piece_len, _ = _seams(bytes.fromhex(b["seams"]))
        first = bytes.fromhex(b["cabac"])[:piece_len[0]]
        stable = _stable_prefix(first)
        assert len(stable) > 0 and r["recodable"]
        assert r["recoded"][:len(stable)] == stable
        n += 1
    assert n > 0


def test_every_unit_regenerates_its_span(ctx, fix):
    data, avrc = fix["data"], fix["avrc"]
    n_slices, units, _ = expected_units(data, avrc, fix["plain"])
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    assert plan.n_slices == n_slices and plan.n_units == len(units) > n_slices
    b = UnitBatch(ctx, plan.parsed_units())
    b.decompress(P32)
    packed, offs, kept, status = (t.cpu().numpy() for t in b.pack())
    torch.cuda.synchronize()
    n = len(units)
    kept = kept[:n].view(np.uint32)
    assert (status[:n] == 0).all() and (b.results()["status"] == 0).all()
    for k, u in enumerate(units):
        got = packed[int(offs[k]):int(offs[k]) + int(kept[k])].tobytes()
        if u["keep"] != KEEP_ALL:
            assert got == u["true"], k
        else:   # a slice's end: its final byte is the patch's
            assert len(got) in (len(u["true"]) - 1, len(u["true"])) and got[:len(u["true"]) - 1] == u["true"][:-1], k
    st, so, sl = shard.collapse_units(plan.pieces, status[:n], offs[:n], kept)
    assert plan.splice(st, packed, so, sl).tobytes() == data


# test_gpu_split.py::test_synthetic_corpus_split_matches_oracle's specs: (w, h, slices per picture,
# frames, gop, slice_type, qp, chroma_format_idc, structure), with their seeds
KINDS = {"420": (0, (22, 18, 2, 6, 6, 1, 25, 1, 0)), "444": (1, (14, 9, 3, 5, 5, 0, 27, 3, 0)),
         "intra": (2, (30, 17, 1, 4, 2, 2, 29, 2, 0)), "b3": (4, (40, 23, 3, 4, 4, 1, 24, 1, 0)),
         "paff": (5, (20, 12, 1, 4, 4, 0, 26, 1, 1))}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_slice_kinds(ctx, kind):
    k, (w, h, spf, frames, gop, st, qp, cf, structure) = KINDS[kind]
    data = ctx.synthesize(avr.SynthParams(mb_width=w, mb_height=h, slice_type=st, slice_qp=qp, chroma_format_idc=cf,
                                          seed=900 + k, slices_per_picture=spf, gop_length=gop, num_ref_idx_l0=2,
                                          structure=structure), frames)
    avrc = _compress(ctx, data, 700)
    assert ctx.decompress(avrc) == data
    if structure == 0:
        assert avr.seams_of_container(avrc) and _tag(avrc) == TAG_S
    else:   # field slices are never cut
        assert not avr.seams_of_container(avrc) and _tag(avrc) == TAG


def test_wide_ring(ctx):
    data = ctx.synthesize(WIDE, 1)
    assert ctx.split_bytes == avr.SPLIT_BYTES_DEFAULT
    avrc = ctx.compress(data, P32)
    assert len(avr.seams_of_container(avrc)) == 1 and _tag(avrc) == TAG_S
    assert ctx.decompress(avrc) == data


def test_option_off_is_todays_container():
    data = (FIX / "realshort.mp4").read_bytes()
    with avr.Context(0) as c:
        assert c.split_p32 is bool(int(os.environ.get("AVR_SPLIT_P32", "0") or 0))
        c.split_p32 = False
        off = _compress(c, data, 512)
        assert not avr.seams_of_container(off) and _tag(off) == TAG
        assert off == _compress(c, data, 0)
        c.split_p32 = True
        assert c.split_p32 is True
        assert _compress(c, data, 0) == off
        assert _compress(c, data, 512) != off


def test_mixed_batch(ctx):
    data, other = (FIX / "realshort.mp4").read_bytes(), (FIX / "cockatoo.mp4").read_bytes()
    p64 = _compress(ctx, data, 1024, P64)
    p32s = _compress(ctx, other, 1024)
    plain = _compress(ctx, data, 0)
    r = ctx.compress(data, avr.MODEL_REFERENCE)
    assert avr.seams_of_container(p64) and avr.seams_of_container(p32s) and not avr.seams_of_container(plain)
    assert ctx.decompress_files([p64, p32s, plain, r]) == [data, other, data, data]
    assert ctx.decompress_files([p32s, p64]) == [other, data]


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


@pytest.mark.parametrize("escaped", [False, True], ids=["plain", "escaped"])
def test_sharded_world1_rccl(ctx, world1, escaped):
    data = (FIX / "cockatoo.mp4").read_bytes()
    ctx.recode_escaped = escaped
    try:
        want = _compress(ctx, data, 1024)
    finally:
        ctx.recode_escaped = False
    assert _tag(want) == (TAG_SE if escaped else TAG_S)
    got = shard.sharded_compress(ctx, data, model=P32, split_bytes=1024, split_p32=True, escaped=escaped)
    assert got == want
    assert shard.sharded_decompress(ctx, got) == data
    # without split_p32 the model ignores split_bytes, as before
    assert shard.sharded_compress(ctx, data, model=P32, split_bytes=1024, escaped=escaped) == \
        shard.sharded_compress(ctx, data, model=P32, escaped=escaped)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_multirank_gloo(ctx, world):
    """One process per rank on cuda:0, gloo for the gathers: the sharded compress equals the whole-file
    one, and the one slice's pieces are regenerated on several ranks."""
    data = ctx.synthesize(ONE_SLICE, 1)
    avrc = _compress(ctx, data, 700)
    cut = [b for b in _coded(avrc) if "seams" in b]
    assert len(cut) == 1 and len(_coded(avrc)) == 1 and len(_seams(bytes.fromhex(cut[0]["seams"]))[1]) >= 3
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
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).parent / "_split_p32_worker.py"),
                                           str(src), "700", str(dst)], env=env))
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
        assert Path(str(dst) + ".avrc").read_bytes() == avrc
        assert dst.read_bytes() == data


def test_escapes_with_seams(ctx):
    from test_hooks import _call
    data = (FIX / "cockatoo.mp4").read_bytes()
    ctx.recode_escaped = True
    try:
        se = _compress(ctx, data, 512)
    finally:
        ctx.recode_escaped = False
    info, _ = avr.describe_container(se)
    assert _tag(se) == TAG_SE and any("escapes" in b for b in info["blocks"]) and avr.seams_of_container(se)
    assert ctx.decompress(se) == data
    r, _, _ = _call("hooks_decompress", se, len(se))
    assert r == -6
    s = _compress(ctx, data, 512)
    assert _tag(s) == TAG_S
    r, back, walked = _call("hooks_decompress", s, len(s))
    assert r == 0 and back == data and walked > 0


def _cut_block(ctx):
    data = (FIX / "realshort.mp4").read_bytes()
    avrc = _compress(ctx, data, 1024)
    blk = next(b for b in avr.describe_container(avrc)[0]["blocks"] if "seams" in b)
    return data, avrc, bytes.fromhex(blk["seams"]), bytes.fromhex(blk["cabac"])


def test_damaged_seams_are_refused(ctx):
    data, avrc, field, _ = _cut_block(ctx)
    bad = bytearray(avrc)
    bad[avrc.index(field) + len(field) // 2] ^= 0x55          # inside the zlib stream
    back = ctx.decompress_files([bytes(bad), avrc])
    assert isinstance(back[0], avr.AvrError) and back[0].code == -3
    assert back[1] == data


@pytest.mark.parametrize("which", ["first", "last"])
def test_damaged_piece_stream_fails_the_file(ctx, which):
    """A byte flipped inside one piece's stream fails the file with a slice status: no fault, no
    success.  From the flipped byte on the piece's decoder runs on other decisions and never finds the
    stream's own again.  The format carries no checksum of a stream, and a piece before a cut ends by
    macroblock count with only its first `keep` bytes taken, so what notices is the P32 pieces' own
    end check (walker_slice): a piece must have used up its stream, its decoder 0 .. 4 bytes past the
    end, which is exact for every stream the encoder made.  A damaged piece stops anywhere in its
    stream or runs off it (AVR_SLICE_OVERREAD), so it passes by chance about 5 times in its length;
    the two places here are fixed, the middle of the first and of the last piece of the first cut
    block.  (Before that check both decompressed to a wrong file.)"""
    data, avrc, field, cabac = _cut_block(ctx)
    _, piece_len, _ = _seams(field)
    at = piece_len[0] // 2 if which == "first" else sum(piece_len[:-1]) + piece_len[-1] // 2
    bad = bytearray(avrc)
    bad[avrc.index(cabac) + at] ^= 0x55
    back = ctx.decompress_files([bytes(bad), avrc])
    assert back[1] == data
    print("damaged piece:", back[0] if isinstance(back[0], avr.AvrError) else
          f"a file of {len(back[0])} bytes, equal to the input: {back[0] == data}")
    assert isinstance(back[0], avr.AvrError), "the damaged container decompressed"
    assert back[0].code == -3 and "failed to decode" in str(back[0])


def test_batch_calls_refuse_other_models(ctx):
    z = torch.zeros(256, dtype=torch.uint8, device="cuda")
    slots = np.zeros(1, avr.SPLIT_SLOT)
    slots["first"] = -1
    for model in (avr.MODEL_REFERENCE, avr.MODEL_CHAINED, 7):
        with pytest.raises(avr.AvrError) as e:
            ctx.compress_split_slices(z, 1, 8, 8, z, z, z, slots, 1024, z, 0, 4096, z, z, model=model)
        assert e.value.code == -1
        with pytest.raises(avr.AvrError) as e:
            ctx.decompress_pieces(z, np.zeros(1, avr.PIECE), 1, 8, 8, z, 0, 4096, z, z, z, model=model)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert not z.any()   # nothing ran


def _run(args, env=None):
    assert CLI.exists(), "recode CLI not built (make -C avrecode_amd)"
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, timeout=120, env=env)


def test_cli():
    src = FIX / "realshort.mp4"
    env = dict(os.environ, AVR_SPLIT_BYTES="512")
    with tempfile.TemporaryDirectory() as td:
        c, d = Path(td) / "c.avrc", Path(td) / "d.mp4"
        r = _run(["compress", "-p32", "-s", src, c], env)
        assert r.returncode == 0, r.stderr.decode()
        assert _tag(c.read_bytes()) == TAG_S and avr.seams_of_container(c.read_bytes())
        r = _run(["decompress", c, d])
        assert r.returncode == 0, r.stderr.decode()
        assert d.read_bytes() == src.read_bytes()
        for flags in (["-p", "-s"], ["-c", "-s"], ["-s"]):
            r = _run(["compress"] + flags + [src, c], env)
            assert r.returncode == 1 and b"-s goes with" in r.stderr
        r = _run(["decompress", "-p32", "-s", c, d])
        assert r.returncode == 1 and b"-s goes with" in r.stderr
