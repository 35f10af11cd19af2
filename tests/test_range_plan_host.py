"""The range planner on the host (avr_dec_plan_file_size / _range / _range_apply, avr_plan.cpp): CPU only.

The containers are the oracle's -- realshort.mp4 at split_bytes 0, 1024 and 2048, cockatoo.mp4 at 2048,
the COUNTS cases of test_piece_plan_host.py -- and what a window must select is derived here from
expected_units' per-unit true byte spans (the container's fields and the file), never from the plan
under test:

* file_size is the file's length; the selected unit range is exactly the units whose true bytes the
  window touches; no span exceeds the cap and the spans tile the window without gap or overlap;
* range_apply, fed each selected unit's true payload bytes (the final byte withheld where the
  container's rule appends it: cockatoo has such slices, realshort none), restores file[off:off+n];
* a piece one byte short of its share, a slice two bytes short of its size and a failed unit fail the
  window with the documented statuses;
* reference and chained containers are refused as load_pieces refuses them."""
from functools import lru_cache

import numpy as np
import pytest

import avrecode_amd as avr
from _oracle import patch_restores, slices_p
from test_piece_plan_host import COUNTS, FIX, KEEP_ALL, _container, expected_units

CASES = [("realshort.mp4", 0)] + sorted(COUNTS)
PAD = 16   # junk after every unit's bytes in the regen buffer: what a span must not copy
SLICE_NO_END, SLICE_OVERREAD = -9, -8


class Case:
    """A container against its file: the blocks' file spans, and per unit (expected_units' order) its
    true file span, its bytes as a device would regenerate them, whether it ends a slice and whether
    it is a piece of a cut slice.  plain: the same file's container without cuts (expected_units).
    (tests/test_gpu_reader.py builds these from the device's containers.)"""

    def __init__(self, data, avrc, plain):
        self.data, self.avrc = data, avrc
        _, units, _ = expected_units(data, avrc, plain)
        info, _ = avr.describe_container(avrc)
        self.blocks, self.unit_span, self.regen, self.ends, self.cuts = [], [], [], [], []
        self.piece = [u["keep"] != KEEP_ALL or u["seam"] >= 0 for u in units]
        self.appending = 0
        pos, u = 0, 0
        # what each coded slice regenerates to, before the last-byte rule: the oracle's decode of it
        regens = iter(r["regen"] for r in slices_p(data)[1] if r["recodable"])
        for b in info["blocks"]:
            if "literal" in b:
                n = len(b["literal"]) // 2
                self.blocks.append((pos, pos + n, False))
                pos += n
            elif "cabac" in b:
                size, s, at = b["size"], units[u]["slice"], pos
                # the rule appends when the slice regenerates one byte less than its size (the container
                # does not say: length_parity is the size's); a re-codable slice stored skip_coded is passed over
                regen = next(g for g in regens if patch_restores(g, data[pos:pos + size]))
                assert len(regen) in (size, size - 1)
                append = len(regen) == size - 1
                self.appending += append
                while u < len(units) and units[u]["slice"] == s:
                    true = units[u]["true"]
                    last = units[u]["keep"] == KEEP_ALL
                    if at > pos:
                        self.cuts.append(at)
                    self.unit_span.append((at, at + len(true)))
                    self.regen.append(true[:-1] if last and append else true)
                    self.ends.append(last)
                    at += len(true)
                    u += 1
                assert at == pos + size
                self.blocks.append((pos, pos + size, True))
                pos += size
        assert u == len(units) and pos == len(data)
        self.plan = avr.DecompressPlan().load(avrc, pieces=True)

    def touched(self, w0, w1):
        k = [i for i, (lo, hi) in enumerate(self.unit_span) if lo < w1 and hi > w0]
        return (k[0], k[-1] + 1) if k else None

    def windows(self, n_random=200):
        size = len(self.data)
        w = [(0, 1), (size - 1, 1), (0, size), (10, 0), (size, 7), (size + 5, 3), (size - 3, 100)]

        def around(b):
            return [(b - 1, 2), (b, 1), (b - 1, 1)] if 0 < b < size else []

        for lo, _, _ in self.blocks:
            w += around(lo)
        # every cut of one split slice (the one with the most pieces)
        if self.cuts:
            per_block = {}
            for q in self.cuts:
                blk = next(b for b in self.blocks if b[0] < q < b[1])
                per_block.setdefault(blk, []).append(q)
            for q in max(per_block.values(), key=len):
                w += around(q)
        lit = next((lo, hi) for lo, hi, coded in self.blocks if not coded and hi - lo >= 5)
        w.append((lit[0] + 1, lit[1] - lit[0] - 2))
        one = next((lo, hi) for lo, hi in self.unit_span if hi - lo >= 5)
        w.append((one[0] + 1, one[1] - one[0] - 2))
        rng = np.random.default_rng(20251)
        for _ in range(n_random):
            off = int(rng.integers(0, size))
            n = int(rng.integers(1, 200000)) if rng.integers(0, 4) == 0 else int(rng.integers(1, 3000))
            w.append((off, n))
        return w

    def feed(self, rng, short=None, status=None):
        """The selected units' bytes packed with PAD junk bytes after each: (regen, unit_off, res)."""
        lo, hi = rng["unit_lo"], rng["unit_hi"]
        res = np.zeros(hi - lo, avr.SLICE_RESULT)
        chunks, offs, at = [], [], 0
        for k in range(lo, hi):
            b = self.regen[k]
            if short and k in short:
                b = b[:len(b) - short[k]]
            res[k - lo]["out_len"] = len(b)
            res[k - lo]["status"] = (status or {}).get(k, 0)
            offs.append(at)
            # a span may take one byte of slack behind an appending slice's bytes: it is junk, as on the device
            chunks.append(b + b"\xEE" * PAD)
            at += len(b) + PAD
        return b"".join(chunks) + b"\xEE", np.array(offs, np.uint64), res


@lru_cache(None)
def _case(name, split_bytes):
    return Case((FIX / name).read_bytes(), _container(name, split_bytes), _container(name, 0))


def _check_window(c, off, n, span_cap=0):
    size = len(c.data)
    r = c.plan.range(off, n, span_cap)
    w0 = min(off, size)
    w1 = min(off + n, size)
    assert (r["off"], r["len"], r["file_size"]) == (w0, w1 - w0, size), (off, n)
    want = c.touched(w0, w1) if w1 > w0 else None
    if want is None:
        assert r["unit_lo"] == r["unit_hi"] and len(r["tails"]) == 0, (off, n)
    else:
        assert (r["unit_lo"], r["unit_hi"]) == want, (off, n)
    cap = span_cap or avr.RANGE_SPAN_BYTES
    sp = r["spans"]
    at = 0
    for s in sp:
        assert 0 < int(s["len"]) <= cap and int(s["dst_off"]) == at, (off, n)
        assert int(s["source"]) == avr.SPAN_LITERAL or 0 <= int(s["source"]) < r["unit_hi"] - r["unit_lo"]
        at += int(s["len"])
    assert at == w1 - w0, (off, n)
    assert r["literal_bytes"] == sum(int(s["len"]) for s in sp if s["source"] == avr.SPAN_LITERAL)
    out, st = c.plan.range_apply(r, *c.feed(r))
    assert out == c.data[w0:w1], (off, n)
    assert not st.any()
    return r


@pytest.mark.parametrize("name,split_bytes", CASES)
def test_file_size_and_appending_slices(name, split_bytes):
    c = _case(name, split_bytes)
    assert c.plan.file_size == len(c.data)
    assert (c.appending > 0) == (name == "cockatoo.mp4")
    # a slice plan knows the file's size too, and is no range plan
    p = avr.DecompressPlan().load(_container(name, 0))
    assert p.file_size == len(c.data)
    with pytest.raises(avr.AvrError) as e:
        p.range(0, 16)
    assert e.value.code == -1


@pytest.mark.parametrize("name,split_bytes", CASES)
def test_windows_select_the_touched_units_and_restore_the_bytes(name, split_bytes):
    c = _case(name, split_bytes)
    ws = c.windows()
    assert len(ws) > 200
    for off, n in ws:
        _check_window(c, off, n)
    # the whole file is every unit, a window inside one unit that unit alone
    assert _check_window(c, 0, len(c.data))["unit_hi"] == len(c.unit_span)
    lo, hi = next(s for s in c.unit_span if s[1] - s[0] >= 5)
    r = _check_window(c, lo + 1, hi - lo - 2)
    assert r["unit_hi"] - r["unit_lo"] == 1 and r["literal_bytes"] == 0


@pytest.mark.parametrize("span_cap", [16, 4096, 1 << 20])
def test_span_caps(span_cap):
    c = _case("realshort.mp4", 1024)
    size = len(c.data)
    for off, n in ((0, size), (size // 3, 70000), (c.blocks[3][0] - 1, 40)):
        r = _check_window(c, off, n, span_cap)
        assert max(int(s["len"]) for s in r["spans"]) <= span_cap
    for bad in (1, 15, (1 << 30) + 1):
        with pytest.raises(avr.AvrError) as e:
            c.plan.range(0, 10, bad)
        assert e.value.code == -1
    with pytest.raises(avr.AvrError) as e:
        c.plan.range((1 << 64) - 4, 8)   # off + len overflows
    assert e.value.code == -1


@pytest.mark.parametrize("name,split_bytes", [("realshort.mp4", 1024), ("cockatoo.mp4", 2048)])
def test_short_units_fail_the_window(name, split_bytes):
    c = _case(name, split_bytes)
    # a piece that is not its slice's last, one byte short of keep
    k = next(i for i, last in enumerate(c.ends) if not last)
    lo, hi = c.unit_span[k]
    r = c.plan.range(lo, hi - lo)
    assert (r["unit_lo"], r["unit_hi"]) == (k, k + 1)
    with pytest.raises(avr.AvrError) as e:
        c.plan.range_apply(r, *c.feed(r, short={k: 1}))
    assert e.value.code == -3 and e.value.status.tolist() == [SLICE_NO_END]
    # a slice two bytes short of its size (one byte short could be the parity rule's append): its last
    # unit fails, the units before it do not
    k = next(i for i, last in enumerate(c.ends) if last and i and not c.ends[i - 1])
    r = c.plan.range(c.unit_span[k - 1][0], c.unit_span[k][1] - c.unit_span[k - 1][0])
    assert (r["unit_lo"], r["unit_hi"]) == (k - 1, k + 1)
    with pytest.raises(avr.AvrError) as e:
        c.plan.range_apply(r, *c.feed(r, short={k: 2}))
    assert e.value.code == -3 and e.value.status.tolist() == [0, SLICE_NO_END]
    # so does a whole slice, also one byte too long; a failed unit reports its own status
    k = next(i for i, last in enumerate(c.ends) if last and (i == 0 or c.ends[i - 1]))
    lo, hi = c.unit_span[k]
    r = c.plan.range(lo + 2, 3)
    assert (r["unit_lo"], r["unit_hi"]) == (k, k + 1)
    for short in (2, -1):
        regen, offs, res = c.feed(r)
        res[0]["out_len"] = int(res[0]["out_len"]) - short
        with pytest.raises(avr.AvrError) as e:
            c.plan.range_apply(r, regen, offs, res)
        assert e.value.status.tolist() == [SLICE_NO_END]
    with pytest.raises(avr.AvrError) as e:
        c.plan.range_apply(r, *c.feed(r, status={k: SLICE_OVERREAD}))
    assert e.value.code == -3 and e.value.status.tolist() == [SLICE_OVERREAD]
    # a span outside the buffers it is given is refused, nothing written
    regen, offs, res = c.feed(r)
    with pytest.raises(avr.AvrError) as e:
        c.plan.range_apply(r, regen[:2], offs, res)
    assert e.value.code == -1


@pytest.mark.parametrize("mode", ["R", "C"])
def test_range_plans_refuse_chaining_models(mode):
    with pytest.raises(avr.AvrError) as e:
        avr.DecompressPlan().load(_container("realshort.mp4", 1024, mode), pieces=True)
    assert e.value.code == -6
    # the slice plan such a container loads as gives the size, and no ranges
    p = avr.DecompressPlan().load(_container("realshort.mp4", 1024, mode))
    assert p.file_size == (FIX / "realshort.mp4").stat().st_size
    with pytest.raises(avr.AvrError) as e:
        p.range(0, 16)
    assert e.value.code == -1
