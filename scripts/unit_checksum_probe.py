"""What unit checksums (Context.unit_checksums, Block field 18) cost: bytes in the container, and time in
a range read.
* growth: realshort.mp4, cockatoo.mp4 and the configs[4] corpus (workloads.corpus) compressed with the
  option off and on (P64, the default split): the difference against the format's formula -- 4 m + 3
  bytes per coded block of m units (4 m + 4 past 31), plus a byte of a Block's own length prefix where
  the field carries it over 127 / 16383 bytes.  It must match exactly.
* read cost, the cases (a), (b) and (d) of scripts/reader_probe.py: Reader.read of the same window from
  the option-off and the option-on container, alternating in one process, median of 9 after 2 warm-ups,
  wall clock around the synchronising call; and the check launch alone (avr_check_units) by HIP events,
  over units of the window's sizes in a device buffer.
Run on a GPU:
  python3 scripts/unit_checksum_probe.py > profiles/unit_checksum_probe.json"""
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import avrecode_amd as avr  # noqa: E402
from avrecode_amd import workloads  # noqa: E402

WARMUPS, CALLS = 2, 9
SECONDS = int(os.environ.get("READER_PROBE_SECONDS", "40"))   # of 4K at 30 fps: about 7.5 MB each
DEV = torch.device("cuda", 0)


def stats(ts):
    return {"ms": 1e3 * statistics.median(ts), "ms_range": [1e3 * min(ts), 1e3 * max(ts)]}


def varint_len(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def pair(ctx, data):
    ctx.unit_checksums = False
    off = ctx.compress(data, avr.MODEL_PARALLEL)
    ctx.unit_checksums = True
    try:
        on = ctx.compress(data, avr.MODEL_PARALLEL)
    finally:
        ctx.unit_checksums = False
    return off, on


def _varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def _fields(b, lo, hi):
    """(field, wire type, start, content start, end) of a message's fields in b[lo:hi]; contents are not copied."""
    i = lo
    while i < hi:
        t, j = _varint(b, i)
        f, w = t >> 3, t & 7
        if w == 0:
            _, e = _varint(b, j)
            c = j
        elif w == 2:
            n, c = _varint(b, j)
            e = c + n
        else:
            c, e = j, j + (8 if w == 1 else 4)
        yield f, w, i, c, e
        i = e


def growth(off, on):
    """The container's growth against the formula, from the option-on container's own blocks."""
    fields = prefix = units = coded = 0
    for f, w, _, c, e in _fields(on, 0, len(on)):
        if f != 2 or w != 2:
            continue
        for f2, w2, s2, c2, e2 in _fields(on, c, e):
            if f2 != 18:
                continue
            m = (e2 - c2) // 4
            cost = 4 * m + (3 if m <= 31 else 4)
            assert w2 == 2 and e2 - s2 == cost and (e2 - c2) % 4 == 0
            fields += cost
            prefix += varint_len(e - c) - varint_len(e - c - cost)
            units += m
            coded += 1
    out = {"bytes_off": len(off), "bytes_on": len(on), "growth": len(on) - len(off), "coded_blocks": coded,
           "units": units, "formula_fields": fields, "formula_length_prefixes": prefix,
           "growth_over_container": (len(on) - len(off)) / len(off)}
    assert out["growth"] == fields + prefix, out
    return out


def beside(ctx, off, on, o, n, want):
    """Reader.read(o, n) of the option-off and the option-on container, alternating."""
    t_off, t_on = [], []
    with avr.Reader(ctx, off) as r0, avr.Reader(ctx, on) as r1:
        assert r0.info["unit_checked"] == 0 and r1.info["unit_checked"] == 1
        for i in range(WARMUPS + CALLS):
            t0 = time.perf_counter()
            a = r0.read(o, n)
            t1 = time.perf_counter()
            b = r1.read(o, n)
            t2 = time.perf_counter()
            assert a == b == want
            if i >= WARMUPS:
                t_off.append(t1 - t0)
                t_on.append(t2 - t1)
        last0, last1 = r0.last, r1.last
    assert {k: v for k, v in last0.items() if k != "phases"} == {k: v for k, v in last1.items() if k != "phases"}
    a, b = stats(t_off), stats(t_on)
    return {"offset": o, "length": n, "read_off": a, "read_on": b, "on_minus_off_ms": b["ms"] - a["ms"],
            "kernel_ms_off": 1e3 * last0["phases"]["kernel_s"], "kernel_ms_on": 1e3 * last1["phases"]["kernel_s"],
            "units": last1["units"], "pieces": last1["pieces"], "regenerated_bytes": last1["regenerated_bytes"]}


def check_alone(ctx, on, o, n):
    """avr_check_units alone over units of the window's sizes (random bytes, zlib's values)."""
    plan = avr.DecompressPlan().load(on, pieces=True)
    r = plan.range(o, n)
    tails = r["tails"].copy()
    tails["has_rule"] = 0
    nu = len(tails)
    share = [int(t["keep"]) if int(t["keep"]) != avr.KEEP_ALL else int(t["size"]) - int(t["q_last"]) for t in tails]
    rng = np.random.default_rng(1)
    checks, res = np.zeros(nu, avr.UNIT_CHECK), np.zeros(nu, avr.SLICE_RESULT)
    chunks, at = [], 0
    for k, s in enumerate(share):
        b = rng.integers(0, 256, s, dtype=np.uint8).tobytes()
        checks[k] = (at, zlib.crc32(b), 1)
        res[k]["out_len"] = s
        chunks.append(b + b"\0" * (-s % 16))
        at += s + (-s % 16)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)  # noqa: E731
    d_src, d_tails, d_checks, d_res = to(np.frombuffer(b"".join(chunks) + b"\0", np.uint8)), to(tails), to(checks), to(res)
    d_st = torch.zeros(max(1, nu), dtype=torch.int32, device=DEV)
    ts = []
    for i in range(WARMUPS + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.check_units(d_tails, d_checks, d_res, nu, d_src, at, d_st)
        e1.record()
        e1.synchronize()
        if i >= WARMUPS:
            ts.append(e0.elapsed_time(e1))
    assert not d_st.cpu().numpy().any()
    return {"units": nu, "bytes": sum(share), "ms": statistics.median(ts), "ms_range": [min(ts), max(ts)]}


def main():
    ctx = avr.Context(0)
    out = {"method": f"median of {CALLS} calls after {WARMUPS} warm-ups, option off and on alternating in one process; "
                     "wall clock around the synchronising call, the check launch alone by HIP events"}
    fix = os.path.join(ROOT, "tests", "fixtures")
    # growth
    out["growth"] = {}
    for name in ("realshort.mp4", "cockatoo.mp4"):
        data = open(os.path.join(fix, name), "rb").read()
        out["growth"][name] = growth(*pair(ctx, data))
    tot = {}
    for name, data in workloads.corpus(ctx):
        g = growth(*pair(ctx, data))
        for k, v in g.items():
            if k != "growth_over_container":
                tot[k] = tot.get(k, 0) + v
    tot["growth_over_container"] = tot["growth"] / tot["bytes_off"]
    out["growth"]["corpus_configs4"] = tot
    print("growth", json.dumps(out["growth"]), file=sys.stderr, flush=True)
    # (d) a 4 KiB read inside one slice of realshort.mp4
    data = open(os.path.join(fix, "realshort.mp4"), "rb").read()
    off, on = pair(ctx, data)
    with avr.Reader(ctx, on) as rd:
        lo = next(o for o in range(len(data) // 2, len(data)) if rd.span(o)[2] and rd.span(o)[1] - o > 600)
        n = min(4096, rd.span(lo)[1] - lo)
    out["small_read_realshort"] = beside(ctx, off, on, lo, n, data[lo:lo + n])
    out["small_read_realshort"]["check_alone"] = check_alone(ctx, on, lo, n)
    print("d", json.dumps(out["small_read_realshort"]), file=sys.stderr, flush=True)
    # (b) 64 KiB in the middle of one 4K 4:4:4 intra slice cut into pieces
    data = ctx.synthesize(avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                                          transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1), 1)
    off, on = pair(ctx, data)
    o = len(data) // 2
    out["intra_444_slice_64KiB"] = beside(ctx, off, on, o, 65536, data[o:o + 65536])
    out["intra_444_slice_64KiB"]["check_alone"] = check_alone(ctx, on, o, 65536)
    print("b", json.dumps(out["intra_444_slice_64KiB"]), file=sys.stderr, flush=True)
    # (a) 1 MiB in the middle of a tiled 4K stream
    data = workloads.stream_4k(ctx, seconds=SECONDS)
    off, on = pair(ctx, data)
    o = len(data) // 2
    out["stream_4k_1MiB"] = beside(ctx, off, on, o, 1 << 20, data[o:o + (1 << 20)])
    out["stream_4k_1MiB"]["check_alone"] = check_alone(ctx, on, o, 1 << 20)
    out["stream_4k_1MiB"]["seconds_of_4k"] = SECONDS
    out["stream_4k_1MiB"]["growth"] = growth(off, on)
    print("a", json.dumps(out["stream_4k_1MiB"]), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
