"""What a range read costs (avrecode_amd.Reader; avr_gather_spans) next to the whole-file decompress.
* (a) Reader.read of 1 MiB at the middle of a tiled 4K stream of a few hundred MB (workloads.stream_4k,
  the configs[3] stream shortened; compressed with the default split), beside ctx.decompress of the same
  container in the same process, alternating.
* (b) 64 KiB at the middle of the 4K 4:4:4 intra slice of tests/test_gpu_split.py (one slice cut into
  pieces at the default split), beside ctx.decompress of its container; Reader.last says how few
  pieces the read touched.
* (c) the gather launch alone, by HIP events, over the spans of a whole-file window of (a) at span caps
  of 16 / 64 / 256 KiB, in bytes per second (the sources' contents do not matter to it: the literals
  are the container's, the units' outputs a buffer laid out as the plan's work buffer).
* (d) a 4 KiB read inside one slice of realshort.mp4: the fixed cost of a read, by phase.
Median of 9 calls after 2 warm-ups, wall clock around the synchronising call.  Run on a GPU:
  python3 scripts/reader_probe.py > profiles/reader_probe.json"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import avrecode_amd as avr  # noqa: E402
from avrecode_amd import workloads  # noqa: E402

WARMUPS, CALLS = 2, 9
SECONDS = int(os.environ.get("READER_PROBE_SECONDS", "40"))   # of 4K at 30 fps: about 7.5 MB each


def stats(ts):
    return {"ms": 1e3 * statistics.median(ts), "ms_range": [1e3 * min(ts), 1e3 * max(ts)]}


def beside(ctx, rd, avrc, off, n, want):
    """Reader.read(off, n) and ctx.decompress(avrc), alternating."""
    tr, td = [], []
    for i in range(WARMUPS + CALLS):
        t0 = time.perf_counter()
        got = rd.read(off, n)
        t1 = time.perf_counter()
        whole = ctx.decompress(avrc)
        t2 = time.perf_counter()
        assert got == want and len(whole) == rd.size
        if i >= WARMUPS:
            tr.append(t1 - t0)
            td.append(t2 - t1)
    last = rd.last
    r, d = stats(tr), stats(td)
    return {"file_bytes": rd.size, "container_bytes": len(avrc), "offset": off, "length": n, "units_in_container":
            rd.info["n_units"], "read": r, "decompress": d, "decompress_over_read": d["ms"] / r["ms"], "last": last}


def gather_alone(ctx, avrc, size):
    plan = avr.DecompressPlan().load(avrc, pieces=True)
    dev = torch.device("cuda", 0)
    base = (len(avrc) + 255) & ~255
    d_src = torch.zeros(base + plan.work_len + 64, dtype=torch.uint8, device=dev)
    d_src[:len(avrc)] = torch.from_numpy(np.frombuffer(avrc, np.uint8).copy()).to(dev)
    d_dst = torch.zeros(size, dtype=torch.uint8, device=dev)
    out = {}
    for cap in (16384, 65536, 262144):
        r = plan.range(0, size, cap)
        sp = r["spans"].copy()
        unit = sp["source"] >= 0
        sp["src_off"][unit] += base + plan.units["out_offset"][r["unit_lo"] + sp["source"][unit]]
        d_sp = torch.from_numpy(sp.view(np.uint8).reshape(-1).copy()).to(dev)
        d_st = torch.zeros(len(sp), dtype=torch.int32, device=dev)
        ts = []
        for i in range(WARMUPS + CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.gather_spans(d_sp, len(sp), d_src, d_src.numel(), d_dst, size, d_st)
            e1.record()
            e1.synchronize()
            if i >= WARMUPS:
                ts.append(e0.elapsed_time(e1))
        assert not d_st.cpu().numpy().any()
        ms = statistics.median(ts)
        out[str(cap)] = {"spans": len(sp), "ms": ms, "ms_range": [min(ts), max(ts)], "GBps": size / ms / 1e6}
    s0 = r["spans"][0]   # the file starts with a literal: the copy is a copy
    if s0["source"] == avr.SPAN_LITERAL:
        o, n = int(s0["src_off"]), int(s0["len"])
        assert d_dst[:n].cpu().numpy().tobytes() == avrc[o:o + n]
    return out


def main():
    ctx = avr.Context(0)
    out = {"method": f"median of {CALLS} calls after {WARMUPS} warm-ups; wall clock around the synchronising call, "
                     "the gather alone by HIP events", "span_cap_default": avr.RANGE_SPAN_BYTES}
    # (d) first: the fixed cost
    data = open(os.path.join(ROOT, "tests", "fixtures", "realshort.mp4"), "rb").read()
    avrc = ctx.compress(data, avr.MODEL_PARALLEL)
    with avr.Reader(ctx, avrc) as rd:
        lo = next(o for o in range(len(data) // 2, len(data)) if rd.span(o)[2] and rd.span(o)[1] - o > 600)
        n = min(4096, rd.span(lo)[1] - lo)
        out["small_read_realshort"] = beside(ctx, rd, avrc, lo, n, data[lo:lo + n])
    print("small", json.dumps(out["small_read_realshort"]), file=sys.stderr, flush=True)
    # (b)
    data = ctx.synthesize(avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                                          transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1), 1)
    avrc = ctx.compress(data, avr.MODEL_PARALLEL)
    with avr.Reader(ctx, avrc) as rd:
        off = len(data) // 2
        out["intra_444_slice_64KiB"] = beside(ctx, rd, avrc, off, 65536, data[off:off + 65536])
    print("b", json.dumps(out["intra_444_slice_64KiB"]), file=sys.stderr, flush=True)
    # (a)
    data = workloads.stream_4k(ctx, seconds=SECONDS)
    avrc = ctx.compress(data, avr.MODEL_PARALLEL)
    with avr.Reader(ctx, avrc) as rd:
        off = len(data) // 2
        out["stream_4k_1MiB"] = beside(ctx, rd, avrc, off, 1 << 20, data[off:off + (1 << 20)])
        out["stream_4k_1MiB"]["seconds_of_4k"] = SECONDS
    print("a", json.dumps(out["stream_4k_1MiB"]), file=sys.stderr, flush=True)
    # (c)
    out["gather_whole_file_window"] = gather_alone(ctx, avrc, len(data))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
