"""What a checked container costs (Context.checksums, avr_crc_spans).
* On the bench's headline batch (1024 synthetic 1080p slices, built as bench.py builds it): the CRC
  launch over all payload spans, and avr_verify_slices over the same buffers as the yardstick (it reads
  the payloads and their regenerated copies: twice the bytes, one compare per 16), by HIP events.
* Whole-file roundtrip wall time with the option off and on, alternating, on cockatoo.mp4 and the
  corpus's 4K 4:4:4 file.
Median of 9 calls after 2 warm-ups (the method of scripts/split_p32_probe.py).  Run on a GPU:
  python3 scripts/checksum_probe.py > profiles/checksum_probe.json"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import avrecode_amd as avr  # noqa: E402
import bench  # noqa: E402
from avrecode_amd import workloads  # noqa: E402
from avrecode_amd.batch import DeviceBatch  # noqa: E402

WARMUPS, CALLS = 2, 9


def event_ms(f):
    """Median, min and max of CALLS launches of f by HIP events on the current stream, after WARMUPS."""
    for _ in range(WARMUPS):
        f()
    ts = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def headline(ctx):
    args = argparse.Namespace(slices=1024, mb_width=120, mb_height=68, seed=0)
    data = bench.make_input(ctx, args.slices, 0, args)
    ps = avr.parse_stream(data)
    b = DeviceBatch(ctx, ps)
    b.roundtrip(avr.MODEL_PARALLEL)
    torch.cuda.synchronize()
    assert (b.verdicts() == 1).all()
    payload = int(ps.descs["payload_size"].sum())
    d_crc, d_status = b.crcs("in")
    torch.cuda.synchronize()
    pays = b.payloads()
    assert not d_status.cpu().numpy().any()
    assert [int(c) for c in d_crc.cpu().numpy().view("uint32")[:b.n]] == [zlib.crc32(p) for p in pays]
    from avrecode_amd.batch import _payload_spans
    d_off, d_len = _payload_spans(ps.descs, b.device)
    crc = event_ms(lambda: ctx.crc_spans(b.d_in, b.d_in.numel(), d_off, d_len, b.n, d_crc, d_status))
    ver = event_ms(lambda: ctx.verify_slices(b.d_desc, b.d_res_c, b.d_res_d, b.n, b.d_in, b.d_regen, b.d_verdict))
    t0 = time.perf_counter()
    for p in pays:
        zlib.crc32(p)
    host = time.perf_counter() - t0
    return {"slices": b.n, "payload_bytes": payload, "largest_payload": int(ps.descs["payload_size"].max()),
            "crc_spans_ms": crc[0], "crc_spans_ms_range": [crc[1], crc[2]], "crc_spans_GBps": payload / crc[0] / 1e6,
            "verify_slices_ms": ver[0], "verify_slices_ms_range": [ver[1], ver[2]],
            "verify_slices_GBps_of_payload": payload / ver[0] / 1e6,
            "crc_over_verify": crc[0] / ver[0], "host_zlib_one_thread_ms": 1e3 * host}


def roundtrips(ctx, data, model):
    """Whole-file roundtrip wall time, option off and on alternating: medians of CALLS each."""
    ts = {False: [], True: []}
    sizes = {}
    for i in range(WARMUPS + CALLS):
        for on in (False, True):
            ctx.checksums = on
            t0 = time.perf_counter()
            avrc, _ = ctx.roundtrip(data, model)
            t = time.perf_counter() - t0
            sizes[on] = len(avrc)
            if i >= WARMUPS:
                ts[on].append(t)
    ctx.checksums = False
    assert avr.file_crc_of_container(avrc) == zlib.crc32(data)
    off, on = statistics.median(ts[False]), statistics.median(ts[True])
    return {"bytes": len(data), "off_ms": 1e3 * off, "off_ms_range": [1e3 * min(ts[False]), 1e3 * max(ts[False])],
            "on_ms": 1e3 * on, "on_ms_range": [1e3 * min(ts[True]), 1e3 * max(ts[True])], "on_over_off": on / off,
            "container_bytes_off": sizes[False], "container_bytes_on": sizes[True]}


def main():
    ctx = avr.Context(0)
    out = {"method": f"median of {CALLS} calls after {WARMUPS} warm-ups; kernels by HIP events, files by wall clock",
           "headline_batch": headline(ctx), "files": {}}
    print("headline", json.dumps(out["headline_batch"]), file=sys.stderr, flush=True)
    corpus = dict(workloads.corpus(ctx, fixtures=False))
    files = {"cockatoo.mp4": open(os.path.join(ROOT, "tests", "fixtures", "cockatoo.mp4"), "rb").read(),
             "4K_IBBP_1spf_444": corpus["4K_IBBP_1spf_444"]}
    for name, data in files.items():
        out["files"][name] = {}
        for label, model in (("P", avr.MODEL_PARALLEL), ("P32", avr.MODEL_PARALLEL32)):
            out["files"][name][label] = roundtrips(ctx, data, model)
            print(name, label, json.dumps(out["files"][name][label]), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
