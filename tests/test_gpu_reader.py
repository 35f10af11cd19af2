"""Range reads on the device (avr_k_gather.hip: avr_gather_spans, avr_range_tails; avr_reader_*, ABI 12).

* the two kernels alone: gather_spans over every (source, destination) alignment pair and the lengths
  at which its head / 16-byte body / tail paths change, at the first and the last byte of a source
  buffer that is itself not aligned, and refused spans with the destination's guard bytes intact;
  range_tails on hand-made results;
* Reader.read against the file, over the window list of tests/test_range_plan_host.py, for
  realshort.mp4 compressed by the device as P64, P32, P64 cut at 1024 and P32S cut at 1024, cockatoo.mp4
  as P64 cut at 2048 (its slices that append their last byte) and the committed PAFF / MBAFF streams;
  Reader.last reports exactly the units the window touches;
* the whole file, device output, and another call on the context between two reads;
* the containers without random access (R, R16, P64E) and their checksum;
* a damaged block on the random-access path: the (block, offset) below is one for which the oracle's
  decompress, run on the CPU over the flip list of tests/test_checksum_host.py, returns 0 and a file
  288 bytes too short;
* the CLI's read command."""
import ctypes
import subprocess

import numpy as np
import pytest

from _oracle import ROOT

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from test_checksum_host import flips  # noqa: E402
from test_range_plan_host import Case  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
CLI = ROOT / "avrecode_amd" / "recode"
DEV = "cuda:0"
GUARD = 0xA5
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4097, 65536]
# flips(plain P64 container of realshort.mp4): coded block 1, Block.cabac byte l // 2 = 436 -- the oracle
# decompresses it with status 0 to a file 288 bytes shorter, first wrong byte at file offset 5655 (the
# block stands for file bytes [5272, 6082)).  (Of the ten silent flips of that list the ones that make
# the slice longer than its output space -- block 2's, + 158 bytes -- fail on the device with
# AVR_SLICE_OVERFLOW: not silent there.)
DAMAGE = (1, 436)
# flips(R16 container of realshort.mp4): block 2 at l // 2 = 583 decompresses on the oracle with status 0
# to a wrong file
DAMAGE_CHAINED = (2, 583)


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _gather(ctx, spans, d_src, src_len, d_dst, dst_len):
    sp = np.zeros(len(spans), avr.SPAN)
    for k, (so, do, ln) in enumerate(spans):
        sp[k] = (so, do, ln, 0)
    d_st = torch.full((max(1, len(spans)),), 77, dtype=torch.int32, device=DEV)
    ctx.gather_spans(_dev(sp), len(spans), d_src, src_len, d_dst, dst_len, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy()[:len(spans)]


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("ln", LENS)
def test_gather_spans_every_alignment_pair(ctx, ln):
    room = (ln + 32 + 15) & ~15
    rng = np.random.default_rng(ln)
    src = rng.integers(0, 256, 256 * room + 16, dtype=np.uint8)
    spans = [(i * room + (i >> 4), i * room + (i & 15), ln) for i in range(256)]
    want = np.full(256 * room + 16, GUARD, np.uint8)
    for so, do, n in spans:
        want[do:do + n] = src[so:so + n]
    d_dst = torch.full((len(want),), GUARD, dtype=torch.uint8, device=DEV)
    st = _gather(ctx, spans, _dev(src), len(src), d_dst, len(want))
    assert not st.any()
    assert np.array_equal(d_dst.cpu().numpy(), want)


@pytest.mark.parametrize("base", [0, 3, 13])
def test_gather_spans_at_the_source_buffers_edges(ctx, base):
    """A source that starts at the buffer's first byte and one that ends flush with its last, the
    buffer itself at any alignment: no 16-byte block outside it may be loaded, and the bytes are right."""
    n = 1000 + 5
    rng = np.random.default_rng(base)
    whole = rng.integers(0, 256, base + n, dtype=np.uint8)
    d_src = _dev(whole)[base:]
    src = whole[base:]
    spans, at = [], 1
    for so, ln in ((0, 257), (n - 257, 257), (0, n), (n - 1, 1), (n - 16, 16), (n - 33, 33), (0, 16), (1, 40)):
        for da in (0, 5):
            spans.append((so, at + da, ln))
            at += (ln + 64) & ~15
    want = np.full(at + 64, GUARD, np.uint8)
    for so, do, ln in spans:
        want[do:do + ln] = src[so:so + ln]
    d_dst = torch.full((len(want),), GUARD, dtype=torch.uint8, device=DEV)
    st = _gather(ctx, spans, d_src, n, d_dst, len(want))
    assert not st.any()
    assert np.array_equal(d_dst.cpu().numpy(), want)


def test_gather_spans_refuses_what_lies_outside(ctx):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 4096, dtype=np.uint8)
    src_len, dst_len = 3000, 2000   # the tensors are longer: nothing past these may be touched
    spans = [(0, 0, 100),                    # fine
             (src_len - 99, 200, 100),       # one byte past src_len
             (src_len + 1, 400, 0),          # starts past src_len
             (100, dst_len - 99, 100),       # one byte past dst_len
             (100, dst_len + 1, 0),
             (src_len - 100, dst_len - 100, 100),   # flush with both ends: fine
             (1 << 40, 600, 16), (0, 1 << 40, 16)]
    want = np.full(4096, GUARD, np.uint8)
    want[0:100] = src[0:100]
    want[dst_len - 100:dst_len] = src[src_len - 100:src_len]
    d_dst = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    st = _gather(ctx, spans, _dev(src), src_len, d_dst, dst_len)
    assert st.tolist() == [0, avr.SLICE_OVERFLOW, avr.SLICE_OVERFLOW, avr.SLICE_OVERFLOW, avr.SLICE_OVERFLOW, 0,
                           avr.SLICE_OVERFLOW, avr.SLICE_OVERFLOW]
    assert np.array_equal(d_dst.cpu().numpy(), want)
    # no spans: nothing launched
    ctx.gather_spans(None, 0, None, 0, None, 0, None)


def test_range_tails_on_hand_made_results(ctx):
    NO, ALL = avr.RANGE_NO_POS, avr.KEEP_ALL
    # (keep, q_last, size, has_rule, parity, last_byte, final_pos), (out_len, status) -> status, byte written
    cases = [
        ((ALL, 0, 100, 0, 0, 0x11, 1), (100, 0), 0, None),        # keep: no rule, the length is the size
        ((ALL, 0, 100, 1, 0, 0x22, 2), (100, 0), 0, 0x22),        # replace
        ((ALL, 40, 101, 1, 1, 0x33, 3), (60, 0), 0, 0x33),        # append: 100 bytes regenerated of 101
        ((ALL, 40, 101, 1, 1, 0x34, 4), (61, 0), 0, 0x34),        # the same slice at full length: replace
        ((50, 0, 500, 0, 0, 0x44, NO), (49, 0), avr.SLICE_NO_END, None),   # a short piece
        ((50, 0, 500, 0, 0, 0x44, NO), (50, 0), 0, None),
        ((50, 0, 500, 0, 0, 0x44, NO), (4000, 0), 0, None),       # a piece may run past its share
        ((ALL, 0, 100, 1, 0, 0x55, 5), (98, 0), avr.SLICE_NO_END, None),   # a slice of the wrong length
        ((ALL, 0, 100, 0, 0, 0x55, 6), (99, 0), avr.SLICE_NO_END, None),   # no rule: nothing is appended
        ((ALL, 0, 100, 1, 0, 0x55, 7), (101, 0), avr.SLICE_NO_END, None),
        ((ALL, 10, 100, 1, 0, 0x55, 8), (100, 0), avr.SLICE_NO_END, None),
        ((ALL, 0, 100, 1, 0, 0x66, 9), (100, -8), -8, None),       # a failed unit: its own status
        ((ALL, 0, 100, 1, 0, 0x77, NO), (100, 0), 0, None),        # the final byte outside the window
        ((ALL, 0, 100, 1, 0, 0x88, 64), (100, 0), avr.SLICE_OVERFLOW, None),   # ... or outside the buffer
    ]
    tails = np.zeros(len(cases), avr.RANGE_TAIL)
    res = np.zeros(len(cases), avr.SLICE_RESULT)
    want = np.full(128, GUARD, np.uint8)
    for k, (t, r, _, byte) in enumerate(cases):
        tails[k] = t[:6] + (0,) + t[6:]
        res[k]["out_len"], res[k]["status"] = r
        if byte is not None:
            want[t[6]] = byte
    d_dst = torch.full((128,), GUARD, dtype=torch.uint8, device=DEV)
    d_st = torch.full((len(cases),), 77, dtype=torch.int32, device=DEV)
    ctx.range_tails(_dev(tails), _dev(res), len(cases), d_dst, 64, d_st)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().tolist() == [c[2] for c in cases]
    assert np.array_equal(d_dst.cpu().numpy(), want)


# ------------------------------------------------------------------ reads against the file
def _compress(ctx, data, model, split_bytes, split_p32=False, escaped=False, checksums=False):
    ctx.split_bytes, ctx.split_p32, ctx.recode_escaped, ctx.checksums = split_bytes, split_p32, escaped, checksums
    try:
        return ctx.compress(data, model)
    finally:
        ctx.split_bytes, ctx.split_p32 = avr.SPLIT_BYTES_DEFAULT, False
        ctx.recode_escaped, ctx.checksums = False, False


KINDS = {"P64": (avr.MODEL_PARALLEL, 0, False), "P32": (avr.MODEL_PARALLEL32, 0, False),
         "P64@1024": (avr.MODEL_PARALLEL, 1024, False), "P32S@1024": (avr.MODEL_PARALLEL32, 1024, True),
         "P64@2048": (avr.MODEL_PARALLEL, 2048, False)}
_cases = {}


def _case(ctx, name, kind):
    """The device's container of a fixture against its file (test_range_plan_host.Case), made once."""
    if (name, kind) not in _cases:
        model, split_bytes, p32 = KINDS[kind]
        data = (FIX / name).read_bytes()
        avrc = _compress(ctx, data, model, split_bytes, p32)
        plain = avrc if not split_bytes else _compress(ctx, data, model, 0)
        assert bool(avr.seams_of_container(avrc)) == bool(split_bytes)
        _cases[(name, kind)] = Case(data, avrc, plain)
    return _cases[(name, kind)]


def _read_windows(ctx, c, windows):
    size = len(c.data)
    with avr.Reader(ctx, c.avrc) as rd:
        assert rd.size == size and rd.info["random_access"] == 1 and rd.info["n_units"] == len(c.unit_span)
        for off, n in windows:
            w0, w1 = min(off, size), min(off + n, size)
            assert rd.read(off, n) == c.data[w0:w1], (off, n)
            if w1 > w0:
                want = c.touched(w0, w1) or (0, 0)
                last = rd.last
                assert last["units"] == want[1] - want[0], (off, n)
                assert last["pieces"] == sum(c.piece[want[0]:want[1]]), (off, n)
                lit = sum(min(hi, w1) - max(lo, w0) for lo, hi, coded in c.blocks if not coded and lo < w1 and hi > w0)
                assert last["literal_bytes"] == lit, (off, n)


@pytest.mark.parametrize("kind", ["P64", "P32", "P64@1024", "P32S@1024"])
def test_reads_equal_the_file(ctx, kind):
    c = _case(ctx, "realshort.mp4", kind)
    _read_windows(ctx, c, c.windows())
    with avr.Reader(ctx, c.avrc) as rd:
        # a window inside one slice: one unit; inside one piece of a cut slice: that piece alone
        k = next(i for i, (lo, hi) in enumerate(c.unit_span) if hi - lo >= 5 and (c.piece[i] or "@" not in kind))
        lo, hi = c.unit_span[k]
        assert rd.read(lo + 1, hi - lo - 2) == c.data[lo + 1:hi - 1]
        assert (rd.last["units"], rd.last["pieces"]) == (1, int(c.piece[k]))
        assert rd.last["regenerated_bytes"] >= hi - lo - 1 and rd.last["spans"] == 1
        assert rd.span(lo + 1)[:2] == next((a, b) for a, b, _ in c.blocks if a <= lo < b)
        assert rd.span(lo + 1)[2] is True and rd.span(0)[2] is False
        with pytest.raises(avr.AvrError):
            rd.span(rd.size)


@pytest.mark.parametrize("part", ["even boundaries", "odd boundaries", "random"])
def test_reads_of_appending_slices(ctx, part):
    """cockatoo.mp4 has slices whose last byte the rule appends: a window across every block boundary
    (the host test runs all three kinds of each) and 50 random windows, in three parts, a read of one of
    these slices being some 14 ms of kernel time."""
    c = _case(ctx, "cockatoo.mp4", "P64@2048")
    assert c.appending > 0
    size = len(c.data)
    if part == "random":
        rng = np.random.default_rng(7)
        w = [(int(rng.integers(0, size)), int(rng.integers(1, 60000))) for _ in range(50)]
    else:
        w = [(lo - 1, 2) for lo, _, _ in c.blocks if 0 < lo < size][part == "odd boundaries"::2]
    _read_windows(ctx, c, w)


@pytest.mark.parametrize("name", ["paff_ipp.264", "mbaff_ib.264"])
def test_reads_of_field_and_mbaff_streams(ctx, name):
    c = _case(ctx, name, "P64")
    _read_windows(ctx, c, c.windows(n_random=60))


def test_whole_file_device_output_and_calls_in_between(ctx):
    c = _case(ctx, "realshort.mp4", "P64@1024")
    size = len(c.data)
    with avr.Reader(ctx, c.avrc) as rd:
        whole = rd.read(0, size)
        assert whole == ctx.decompress(c.avrc) == c.data
        assert rd.last["units"] == len(c.unit_span)
        t = torch.full((5000 + 16,), GUARD, dtype=torch.uint8, device=DEV)
        for off, n in ((0, 5000), (size // 3 + 1, 4097), (size - 100, 5000)):
            t.fill_(GUARD)
            got = rd.read_into(t[3:], off, n)   # the destination at any alignment
            host = t.cpu().numpy()
            assert got == len(c.data[off:off + n]) and host[3:3 + got].tobytes() == rd.read(off, n) == c.data[off:off + n]
            assert (host[:3] == GUARD).all() and (host[3 + got:] == GUARD).all()
        a = rd.read(size // 2, 3000)
        ctx.compress((FIX / "paff_ipp.264").read_bytes(), avr.MODEL_PARALLEL)   # the context's own buffers move
        assert rd.read(size // 2, 3000) == a == c.data[size // 2:size // 2 + 3000]
        # pread at and past the end, and an empty window: nothing, and nothing launched
        before = rd.last
        assert rd.read(size, 10) == rd.read(size + 5, 10) == rd.read(7, 0) == b""
        assert rd.last == before
        got = ctypes.c_size_t(9)
        r = avr.lib().avr_reader_read(rd._h, (1 << 64) - 4, 8, None, ctypes.byref(got))
        assert r == -1 and got.value == 0


# ------------------------------------------------------------------ without random access
@pytest.mark.parametrize("kind", ["R", "R16", "P64E"])
def test_fallback_serves_the_whole_file(ctx, kind):
    name = "cockatoo.mp4" if kind == "P64E" else "realshort.mp4"
    data = (FIX / name).read_bytes()
    model = {"R": avr.MODEL_REFERENCE, "R16": avr.MODEL_CHAINED, "P64E": avr.MODEL_PARALLEL}[kind]
    avrc = _compress(ctx, data, model, avr.SPLIT_BYTES_DEFAULT, escaped=kind == "P64E", checksums=True)
    if kind == "P64E":
        assert any("escapes" in b for b in avr.describe_container(avrc)[0]["blocks"])
    size = len(data)
    rng = np.random.default_rng(11)
    with avr.Reader(ctx, avrc) as rd:
        assert rd.info["random_access"] == 0 and rd.info["checked"] == 1 and rd.size == size
        assert rd.info["model"] == model and rd.info["n_units"] == 0
        for off, n in [(0, 1), (size - 1, 1), (0, size), (size - 3, 100), (size, 4), (5, 0)] + \
                [(int(rng.integers(0, size)), int(rng.integers(1, 50000))) for _ in range(20)]:
            assert rd.read(off, n) == data[off:off + n], (off, n)
        t = torch.zeros(4096, dtype=torch.uint8, device=DEV)
        assert rd.read_into(t, 1000, 4096) == 4096 and t.cpu().numpy().tobytes() == data[1000:5096]


def test_fallback_checks_the_files_crc(ctx):
    data = (FIX / "realshort.mp4").read_bytes()
    avrc = _compress(ctx, data, avr.MODEL_CHAINED, avr.SPLIT_BYTES_DEFAULT, checksums=True)
    damaged = next(d for i, where, d in flips(avrc) if (i, where) == DAMAGE_CHAINED)
    with avr.Reader(ctx, damaged) as rd:
        assert rd.info["random_access"] == 0 and rd.info["checked"] == 1
        with pytest.raises(avr.AvrError) as e:
            rd.read(0, 16)
        assert e.value.code == avr.ERR_CHECKSUM


# ------------------------------------------------------------------ damage on the random-access path
def test_a_damaged_block_fails_the_reads_that_touch_it(ctx):
    c = _case(ctx, "realshort.mp4", "P64")
    data = c.data
    damaged = next(d for i, where, d in flips(c.avrc) if (i, where) == DAMAGE)
    wrong = ctx.decompress(damaged)          # the whole-file call: status 0, and not the file
    assert wrong != data and len(wrong) != len(data)
    coded = [(lo, hi) for lo, hi, is_coded in c.blocks if is_coded]
    lo, hi = coded[DAMAGE[0]]
    with avr.Reader(ctx, damaged) as rd:
        assert rd.size == len(data)          # the coordinates are the container's sizes
        for off, n in ((lo, 16), (lo + 5, hi - lo - 10), (hi - 4, 4), (lo - 3, 8), (hi - 2, 6), (0, rd.size)):
            try:
                got = rd.read(off, n)
            except avr.AvrError as e:
                assert e.code == -3, (off, n)
            else:   # never wrong bytes with status 0
                assert got == data[off:off + n], (off, n)
        # the slice regenerates to another length than its block's size: every read inside it is refused
        with pytest.raises(avr.AvrError) as e:
            rd.read(lo, 16)
        assert e.value.code == -3 and "failed to decode (-9)" in str(e.value)
        # reads that avoid the block succeed, before and after a failed one
        for a, b in (coded[DAMAGE[0] - 1], coded[DAMAGE[0] + 1], (0, lo), (hi, rd.size)):
            assert rd.read(a, b - a) == data[a:b]


# ------------------------------------------------------------------ the CLI
def test_cli_read(ctx, tmp_path):
    c = _case(ctx, "realshort.mp4", "P64@1024")
    f = tmp_path / "x.avrc"
    f.write_bytes(c.avrc)
    size = len(c.data)
    lo, hi = next(s for s, p in zip(c.unit_span, c.piece) if p)
    for k, (off, n) in enumerate(((0, 100), (lo + 1, 3000), (size - 50, 1000))):
        out = tmp_path / f"w{k}.bin"
        r = subprocess.run([str(CLI), "read", str(f), str(off), str(n), str(out)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        assert out.read_bytes() == c.data[off:off + n]
    r = subprocess.run([str(CLI), "read", str(f), "10", "20"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == c.data[10:30]
    for bad in (["12x", "4"], ["-1", "4"], ["0"], ["0", "4k"]):
        r = subprocess.run([str(CLI), "read", str(f)] + bad, capture_output=True, timeout=120)
        assert r.returncode != 0, bad
