"""Unit checksums on the device (avr_k_check.hip: avr_check_units; Context.unit_checksums, Block field
18, AVR_SLICE_CHECKSUM, ABI 13).

* avr_check_units alone against zlib: the lengths at which crc_span's head / 16-byte body / tail paths
  change, source offsets 0, 3 and 13 in a buffer that is not itself aligned, every tail kind (a piece
  that keeps less than or all it regenerated, no rule, keep, replace, append -- also of nothing), a
  preset status and a unit without a value left alone, a span past src_len refused, and one wrong
  expected value failing alone;
* the device compress with the option, as P64, P32, P64 cut at 1024 and P32S cut at 1024: the option-off
  container plus fields whose values are zlib's over the units' shares of the file; Reader over
  Case.windows() returns the file with the stats it has without the field; shard.sharded_compress at
  world 1 writes the same bytes;
* the 216 single-bit flips of Block.cabac over realshort's P64 container (every coded block at l // 5,
  l // 3, l // 2, 2 l // 3, l - 3, l - 1): with the option every read of the flipped block's span and of
  the whole file raises or returns the file's bytes; at (16, 1987) -- where the unchecked container
  returns three wrong bytes with no error, the control -- it raises ERR_CHECKSUM, reads that avoid the
  block succeed before and after, and ctx.decompress raises ERR_CHECKSUM with no Metadata field 16;
* a cut container with a byte flipped in a first piece: reads inside the piece fail, a read inside a
  later piece of the same slice returns the file's bytes, the whole-file call names the block;
* P64E on cockatoo with the option: the round trip passes and a flipped escaped block fails;
* the CLI: -u, and read on the damaged container."""
import ctypes
import os
import socket
import subprocess
import zlib

import numpy as np
import pytest

from _oracle import ROOT

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402
from test_piece_plan_host import expected_units  # noqa: E402
from test_range_plan_host import Case  # noqa: E402
from test_unit_checksum_host import FLIP_BLOCK, FLIP_BYTE, FLIP_SPAN, FLIP_WRONG, _coded, strip_units  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
CLI = ROOT / "avrecode_amd" / "recode"
DEV = "cuda:0"
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4097, 65536]
ALL, NO = avr.KEEP_ALL, avr.RANGE_NO_POS
FLIP_WHERE = ("l//5", "l//3", "l//2", "2l//3", "l-3", "l-1")


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


# ------------------------------------------------------------------ the kernel
def _units(rng):
    """Hand-made units: (tail row, out_len, the bytes the unit regenerated, the bytes its CRC covers)."""
    out = []
    for ln in LENS:
        b = rng.integers(0, 256, ln + 9, dtype=np.uint8).tobytes()
        q = int(rng.integers(0, 50))
        lb = int(rng.integers(0, 256))
        par = (q + ln) & 1
        out.append(((ln, 0, 500000, 0, 0, lb, NO), ln + 9, b, b[:ln]))            # a piece that keeps less than it made
        out.append(((ln, 0, 500000, 1, 1, lb, NO), ln, b[:ln], b[:ln]))           # ... and all of it (no rule applies)
        out.append(((ALL, q, q + ln, 0, par, lb, NO), ln, b[:ln], b[:ln]))        # a last unit without a rule
        if ln:
            out.append(((ALL, q, q + ln, 1, par, lb, 7), ln, b[:ln], b[:ln - 1] + bytes([lb])))   # replace
        else:
            out.append(((ALL, 0, 0, 1, 0, lb, NO), 0, b"", b""))                  # keep: nothing to replace
        out.append(((ALL, q, q + ln + 1, 1, par ^ 1, lb, NO), ln, b[:ln], b[:ln] + bytes([lb])))   # append
    return out


@pytest.mark.parametrize("base", [0, 3, 13])
def test_check_units_against_zlib(ctx, base):
    rng = np.random.default_rng(base)
    units = _units(rng)
    n = len(units)
    assert n == 5 * len(LENS)
    # the units' bytes one after the other at every alignment, the first at the buffer's first byte, the
    # last flush with its end; the buffer itself starts `base` bytes into an allocation
    tails, res, checks = np.zeros(n, avr.RANGE_TAIL), np.zeros(n, avr.SLICE_RESULT), np.zeros(n, avr.UNIT_CHECK)
    chunks, at = [], 0
    for k, (t, out_len, regen, covered) in enumerate(units):
        tails[k] = t[:6] + (0,) + t[6:]
        res[k]["out_len"] = out_len
        checks[k] = (at, zlib.crc32(covered), 1)
        gap = b"\xEE" * ((k * 7) % 16 + 1) if k + 1 < n else b""
        chunks.append(regen + gap)
        at += len(regen) + len(gap)
    src = b"".join(chunks)
    assert len(src) == at and int(checks[-1]["src_off"]) + len(units[-1][2]) == at
    d_src = _dev(np.frombuffer(b"\xEE" * base + src, np.uint8))[base:]
    d_tails, d_res = _dev(tails), _dev(res)

    def run(ck, status):
        d_st = torch.from_numpy(np.asarray(status, np.int32).copy()).to(DEV)
        ctx.check_units(d_tails, _dev(ck), d_res, n, d_src, len(src), d_st)
        torch.cuda.synchronize()
        return d_st.cpu().numpy()

    st = run(checks, np.zeros(n, np.int32))
    assert not st.any(), [(k, units[k][0], int(s)) for k, s in enumerate(st) if s]
    # the host restatement agrees
    rc, hst = avr.unit_checks_apply(tails, checks, res, src)
    assert rc == 0 and not hst.any()
    # one wrong expected value fails, and only there; every unit in turn over a few launches
    for wrong in (0, 3, 4, n // 2, n - 2, n - 1):
        ck = checks.copy()
        ck[wrong]["crc"] ^= 1 << (wrong % 32)
        st = run(ck, np.zeros(n, np.int32))
        assert list(np.flatnonzero(st)) == [wrong] and st[wrong] == avr.SLICE_CHECKSUM
    # every value wrong: a preset status, a failed unit and a unit without a value are left alone
    ck = checks.copy()
    ck["crc"] += 1
    preset = np.zeros(n, np.int32)
    preset[1::5] = avr.SLICE_NO_END
    res2 = res.copy()
    res2["status"][2::5] = -8
    ck["have"][3::5] = 0
    d_res = _dev(res2)
    st = run(ck, preset)
    want = np.full(n, avr.SLICE_CHECKSUM, np.int32)
    want[1::5], want[2::5], want[3::5] = avr.SLICE_NO_END, 0, 0
    assert st.tolist() == want.tolist()
    d_res = _dev(res)
    # a span past src_len: refused, nothing of it read -- the last unit one byte further, a start past
    # the end, an offset that would wrap
    ck = checks.copy()
    ck[n - 1]["src_off"] += 1
    ck[0]["src_off"] = len(src) + 1
    ck[5]["src_off"] = (1 << 64) - 8
    st = run(ck, np.zeros(n, np.int32))
    assert sorted(np.flatnonzero(st)) == [0, 5, n - 1] and set(st[[0, 5, n - 1]].tolist()) == {avr.SLICE_OVERFLOW}
    # no units: nothing launched
    ctx.check_units(None, None, None, 0, None, 0, None)


# ------------------------------------------------------------------ the device compress
def _compress(ctx, data, model, split_bytes, split_p32=False, units=False, escaped=False, checksums=False):
    ctx.split_bytes, ctx.split_p32, ctx.unit_checksums = split_bytes, split_p32, units
    ctx.recode_escaped, ctx.checksums = escaped, checksums
    try:
        return ctx.compress(data, model)
    finally:
        ctx.split_bytes, ctx.split_p32, ctx.unit_checksums = avr.SPLIT_BYTES_DEFAULT, False, False
        ctx.recode_escaped, ctx.checksums = False, False


KINDS = {"P64": (avr.MODEL_PARALLEL, 0, False), "P32": (avr.MODEL_PARALLEL32, 0, False),
         "P64@1024": (avr.MODEL_PARALLEL, 1024, False), "P32S@1024": (avr.MODEL_PARALLEL32, 1024, True)}
_made = {}


def _pair(ctx, kind):
    """(file, the option-off container, the option-on container, the uncut container) of realshort."""
    if kind not in _made:
        model, split_bytes, p32 = KINDS[kind]
        data = (FIX / "realshort.mp4").read_bytes()
        off = _compress(ctx, data, model, split_bytes, p32)
        on = _compress(ctx, data, model, split_bytes, p32, units=True)
        plain = off if not split_bytes else _compress(ctx, data, model, 0)
        _made[kind] = (data, off, on, plain)
    return _made[kind]


@pytest.fixture
def world1():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", list(KINDS))
def test_compress_writes_zlibs_values_and_reads_as_before(ctx, kind):
    data, off, on, plain = _pair(ctx, kind)
    model, split_bytes, p32 = KINDS[kind]
    assert strip_units(on) == off and on != off
    assert avr.describe_container(on)[1] == on
    _, units, _ = expected_units(data, on, plain)
    coded = _coded(on)
    assert all("unit_crcs" in b for b in coded) and bool(avr.seams_of_container(on)) == bool(split_bytes)
    assert [v for b in coded for v in b["unit_crcs"]] == [zlib.crc32(u["true"]) for u in units]
    assert len(units) > len(coded) if split_bytes else len(units) == len(coded)
    print(f"{kind}: {len(off)} -> {len(on)} bytes, {len(coded)} coded blocks, {len(units)} units")
    assert ctx.decompress(on) == data
    # reads: the file, with the stats a read of the option-off container has
    c = Case(data, on, plain)
    size = len(data)
    with avr.Reader(ctx, on) as rd, avr.Reader(ctx, off) as rd0:
        assert rd.info["unit_checked"] == 1 and rd0.info["unit_checked"] == 0
        assert {k: v for k, v in rd.info.items() if k != "unit_checked"} == \
            {k: v for k, v in rd0.info.items() if k != "unit_checked"}
        for k, (o, n) in enumerate(c.windows()):
            w0, w1 = min(o, size), min(o + n, size)
            assert rd.read(o, n) == data[w0:w1], (o, n)
            if w1 > w0:
                want = c.touched(w0, w1) or (0, 0)
                last = rd.last
                assert last["units"] == want[1] - want[0] and last["pieces"] == sum(c.piece[want[0]:want[1]]), (o, n)
                if k % 4 == 0:   # and all of avr_read_stats but the times, beside a read of the option-off container
                    assert rd0.read(o, n) == data[w0:w1]
                    last0 = rd0.last
                    assert {f: v for f, v in last.items() if f != "phases"} == {f: v for f, v in last0.items() if f != "phases"}


@pytest.mark.parametrize("kind", list(KINDS))
def test_sharded_compress_world1_equals_the_whole_file_compress(ctx, world1, kind):
    data, off, on, _ = _pair(ctx, kind)
    model, split_bytes, p32 = KINDS[kind]
    ctx.unit_checksums = True
    try:
        got = shard.sharded_compress(ctx, data, model=model, split_bytes=split_bytes, split_p32=p32,
                                     unit_checksums=ctx.unit_checksums)
    finally:
        ctx.unit_checksums = False
    assert got == on
    assert shard.sharded_compress(ctx, data, model=model, split_bytes=split_bytes, split_p32=p32) == off
    assert shard.sharded_decompress(ctx, on) == data


def test_the_other_models_and_the_environment(ctx):
    data = (FIX / "realshort.mp4").read_bytes()
    for model in (avr.MODEL_REFERENCE, avr.MODEL_CHAINED):   # their bytes are pinned: the option is ignored
        assert _compress(ctx, data, model, avr.SPLIT_BYTES_DEFAULT, units=True) == \
            _compress(ctx, data, model, avr.SPLIT_BYTES_DEFAULT)
    assert ctx.unit_checksums is False
    os.environ["AVR_UNIT_CHECKSUMS"] = "1"
    try:
        with avr.Context(0) as c2:
            assert c2.unit_checksums is True
            c2.split_bytes = 0
            assert c2.compress(data, avr.MODEL_PARALLEL) == _pair(ctx, "P64")[2]
    finally:
        del os.environ["AVR_UNIT_CHECKSUMS"]
    # with the file's CRC too: both fields, both checked
    both = _compress(ctx, data, avr.MODEL_PARALLEL, 0, units=True, checksums=True)
    info = avr.describe_container(both)[0]
    assert info["file_crc"] == zlib.crc32(data) and all("unit_crcs" in b for b in _coded(both))
    assert ctx.decompress(both) == data


# ------------------------------------------------------------------ the 216 flips
def _flips(avrc, where):
    """(block, byte, damaged container) for every coded block at one of the six positions."""
    out = []
    for i, b in enumerate(_coded(avrc)):
        c = bytes.fromhex(b["cabac"])
        at, n = avrc.find(c), len(c)
        assert at > 0 and avrc.find(c, at + 1) < 0
        byte = {"l//5": n // 5, "l//3": n // 3, "l//2": n // 2, "2l//3": 2 * n // 3, "l-3": n - 3, "l-1": n - 1}[where]
        d = bytearray(avrc)
        d[at + byte] ^= 0x10
        out.append((i, byte, bytes(d)))
    return out


@pytest.mark.parametrize("where", FLIP_WHERE)
def test_no_flip_reads_wrong_bytes_from_a_checked_container(ctx, where):
    data, off, on, _ = _pair(ctx, "P64")
    c = Case(data, off, off)
    coded = [(lo, hi) for lo, hi, is_coded in c.blocks if is_coded]
    flips = _flips(on, where)
    assert len(flips) == 36
    outcome = {"raised": 0, "right": 0}
    for i, byte, damaged in flips:
        lo, hi = coded[i]
        with avr.Reader(ctx, damaged) as rd:
            for o, n in ((lo, hi - lo), (0, rd.size)):
                try:
                    got = rd.read(o, n)
                except avr.AvrError as e:
                    assert e.code in (-3, avr.ERR_CHECKSUM), (i, byte, o, n)
                    outcome["raised"] += 1
                else:   # never wrong bytes with status 0
                    assert got == data[o:o + n], (i, byte, o, n)
                    outcome["right"] += 1
    print(where, outcome)


def test_the_silent_flip_is_caught_and_located(ctx):
    data, off, on, _ = _pair(ctx, "P64")
    c = Case(data, off, off)
    coded = [(lo, hi) for lo, hi, is_coded in c.blocks if is_coded]
    lo, hi = coded[FLIP_BLOCK]
    assert (lo, hi) == FLIP_SPAN
    where = next(w for w in FLIP_WHERE if _flips(off, w)[FLIP_BLOCK][1] == FLIP_BYTE)
    # the control: on the option-off container the read returns wrong bytes with no error
    damaged0 = _flips(off, where)[FLIP_BLOCK][2]
    with avr.Reader(ctx, damaged0) as rd:
        got = rd.read(lo, hi - lo)
    diff = [lo + int(i) for i in np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(data[lo:hi], np.uint8))]
    print("control: wrong bytes at", diff)
    assert len(got) == hi - lo and tuple(diff) == FLIP_WRONG
    whole = ctx.decompress(damaged0)
    assert len(whole) == len(data) and whole != data
    # checked: the same read raises, and names the unit
    damaged = _flips(on, where)[FLIP_BLOCK][2]
    assert "file_crc" not in avr.describe_container(damaged)[0]
    with avr.Reader(ctx, damaged) as rd:
        before = (coded[FLIP_BLOCK - 1], (0, lo))
        for a, b in before:
            assert rd.read(a, b - a) == data[a:b]
        for o, n in ((lo, hi - lo), (FLIP_WRONG[0], 3), (hi - 8, 8), (lo, 16), (lo - 5, 10), (0, rd.size)):
            sentinel = np.full(max(1, n), 0xA5, np.uint8)
            got = ctypes.c_size_t(9)
            r = avr.lib().avr_reader_read(rd._h, o, n, sentinel.ctypes.data, ctypes.byref(got))
            assert r == avr.ERR_CHECKSUM and (sentinel == 0xA5).all(), (o, n)   # `out` is untouched
            with pytest.raises(avr.AvrError) as e:
                rd.read(o, n)
            assert e.value.code == avr.ERR_CHECKSUM and f"unit {FLIP_BLOCK} " in str(e.value)
        for a, b in before + (coded[FLIP_BLOCK + 1], (hi, rd.size)):
            assert rd.read(a, b - a) == data[a:b]
    with pytest.raises(avr.AvrError) as e:
        ctx.decompress(damaged)
    assert e.value.code == avr.ERR_CHECKSUM and "block" in str(e.value)
    # the batch call: that file alone fails
    res = ctx.decompress_files([on, damaged, on])
    assert res[0] == res[2] == data and isinstance(res[1], avr.AvrError) and res[1].code == avr.ERR_CHECKSUM


# ------------------------------------------------------------------ a cut container
@pytest.mark.parametrize("kind", ["P64@1024", "P32S@1024"])
def test_a_damaged_piece_fails_alone(ctx, kind):
    data, off, on, plain = _pair(ctx, kind)
    c = Case(data, on, plain)
    _, units, _ = expected_units(data, on, plain)
    # a first piece with at least two pieces after it
    first = next(k for k, u in enumerate(units) if u["keep"] != ALL and u["seam"] < 0 and
                 units[k + 2]["slice"] == u["slice"])
    stream = units[first]["stream"]
    at = on.find(stream)
    assert at > 0 and on.find(stream, at + 1) < 0
    lo, hi = c.unit_span[first]
    later = c.unit_span[first + 2]
    blocks = avr.describe_container(on)[0]["blocks"]
    block = [i for i, b in enumerate(blocks) if "cabac" in b][units[first]["slice"]]

    def flipped(byte):
        d = bytearray(on)
        d[at + byte] ^= 0x10
        return bytes(d)

    def check(damaged, codes):
        with avr.Reader(ctx, damaged) as rd:
            for o, n in ((lo, hi - lo), (lo + 1, hi - lo - 2), (lo - 3, 8), (hi - 4, 8), (0, rd.size)):
                with pytest.raises(avr.AvrError) as e:
                    rd.read(o, n)
                assert e.value.code in codes and f"unit {first} " in str(e.value), (o, n, str(e.value))
            # wholly inside a later piece of the same slice: the file's bytes
            assert rd.read(later[0], later[1] - later[0]) == data[later[0]:later[1]]
            assert rd.last["units"] == 1 and rd.last["pieces"] == 1
            assert rd.read(later[0] + 3, 5) == data[later[0] + 3:later[0] + 8]
        with pytest.raises(avr.AvrError) as e:
            ctx.decompress(damaged)
        assert e.value.code in codes and f"block {block}:" in str(e.value), str(e.value)

    # the middle of the piece's stream: the piece fails to decode, or decodes to other bytes
    check(flipped(len(stream) // 2), (-3, avr.ERR_CHECKSUM))
    # a flip that still decodes -- the damage only the checksum sees: the first such from the stream's end
    silent = None
    for byte in range(len(stream) - 1, max(len(stream) - 40, 0), -1):
        with avr.Reader(ctx, flipped(byte)) as rd:
            try:
                assert rd.read(lo, hi - lo) == data[lo:hi]   # a flip of the last bits may change nothing the piece keeps
            except avr.AvrError as e:
                if e.code == avr.ERR_CHECKSUM:
                    silent = byte
                    break
    assert silent is not None, "no flip of the piece's stream decoded to other bytes"
    print(f"{kind}: unit {first}, stream byte {silent} of {len(stream)}: checksum only")
    check(flipped(silent), (avr.ERR_CHECKSUM,))
    # unchecked, the same flip passes the whole-file call with a wrong file
    assert ctx.decompress(strip_units(flipped(silent))) != data


# ------------------------------------------------------------------ escaped blocks
def test_escaped_blocks_are_checked_in_the_unescaped_domain(ctx):
    data = (FIX / "cockatoo.mp4").read_bytes()
    on = _compress(ctx, data, avr.MODEL_PARALLEL, 0, units=True, escaped=True)
    off = _compress(ctx, data, avr.MODEL_PARALLEL, 0, escaped=True)
    assert strip_units(on) == off
    blocks = avr.describe_container(on)[0]["blocks"]
    esc = [b for b in blocks if "escapes" in b]
    assert esc and all("unit_crcs" in b for b in blocks if "cabac" in b)
    assert ctx.decompress(on) == data
    with avr.Reader(ctx, on) as rd:   # no random access: the whole-file call, which checks
        assert rd.info["random_access"] == 0 and rd.info["unit_checked"] == 1
        assert rd.read(1000, 5000) == data[1000:6000]
    # an escaped block's value is the CRC of its unescaped payload: the file's bytes, unescaped
    pos = 0
    for b in blocks:
        if "literal" in b:
            pos += len(b["literal"]) // 2
        elif "cabac" in b:
            n = b["size"] + b.get("escapes", 0)
            if "escapes" in b:
                raw = data[pos:pos + n]
                payload = raw.replace(b"\x00\x00\x03", b"\x00\x00")
                assert len(payload) == b["size"] and b["unit_crcs"] == [zlib.crc32(payload)]
            pos += n
    assert pos == len(data)
    cabac = bytes.fromhex(esc[0]["cabac"])
    at = on.find(cabac)
    for byte in (len(cabac) // 2, len(cabac) - 3):
        d = bytearray(on)
        d[at + byte] ^= 0x10
        with pytest.raises(avr.AvrError):
            ctx.decompress(bytes(d))


# ------------------------------------------------------------------ the CLI
def test_cli_writes_and_checks_the_field(ctx, tmp_path):
    data, off, on, _ = _pair(ctx, "P64@1024")
    src = FIX / "realshort.mp4"
    env = dict(os.environ, AVR_SPLIT_BYTES="1024")
    out = tmp_path / "u.avrc"
    r = subprocess.run([str(CLI), "compress", "-p", "-u", str(src), str(out)], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()
    assert out.read_bytes() == on
    r = subprocess.run([str(CLI), "roundtrip", "-p32", "-u", str(src)], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()
    for bad in (["compress", "-u", str(src)], ["decompress", "-p", "-u", str(out)]):
        assert subprocess.run([str(CLI)] + bad, capture_output=True, timeout=120).returncode != 0
    # read on the damaged container of the control flip
    _, off64, on64, _ = _pair(ctx, "P64")
    damaged = tmp_path / "d.avrc"
    damaged.write_bytes(_flips(on64, "l-3")[FLIP_BLOCK][2])
    assert _flips(on64, "l-3")[FLIP_BLOCK][1] == FLIP_BYTE
    r = subprocess.run([str(CLI), "read", str(damaged), str(FLIP_WRONG[0]), "3"], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"checksum" in r.stderr and b"(-7)" in r.stderr and r.stdout == b""
    r = subprocess.run([str(CLI), "read", str(damaged), "0", "1000"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == data[:1000]
    r = subprocess.run([str(CLI), "decompress", str(damaged)], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"(-7)" in r.stderr
