"""What the long-slice split does for MODEL_PARALLEL32 (Context.split_p32): the corpus's 4K 4:4:4 IBBP
file and the lone 4K 4:4:4 intra slice, checked compress and decompress, split off against split on
at the default 96 KiB, with MODEL_PARALLEL's split figures from the same run next to them.  Median
of 9 calls after 2 warm-ups (the method of DESIGN §8.2's piece-plan figures); container bytes with
the seams' share.  Run on a GPU:
  python3 scripts/split_p32_probe.py > profiles/split_p32_probe.json"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import workloads  # noqa: E402

WIDE = avr.SynthParams(mb_width=240, mb_height=135, slice_type=2, slice_qp=30, chroma_format_idc=3,
                       transform_8x8_mode=1, seed=4006, slices_per_picture=1, gop_length=1)
WARMUPS, CALLS = 2, 9


def timed(f):
    for _ in range(WARMUPS):
        r = f()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return r, statistics.median(ts), min(ts), max(ts)


def measure(ctx, data, model, split_bytes):
    ctx.split_bytes = split_bytes
    avrc, c_med, c_min, c_max = timed(lambda: ctx.compress(data, model))
    back, d_med, d_min, d_max = timed(lambda: ctx.decompress(avrc))
    assert back == data
    info, _ = avr.describe_container(avrc)
    seams = [len(b["seams"]) // 2 for b in info["blocks"] if "seams" in b]
    pieces = 0
    if seams:
        plan = avr.DecompressPlan().load(avrc, pieces=True)
        pieces = int(plan.n_units - plan.n_slices + len(seams))
    return {"tag": bytes.fromhex(info["version"]).decode(), "compress_ms": 1e3 * c_med,
            "compress_ms_range": [1e3 * c_min, 1e3 * c_max], "decompress_ms": 1e3 * d_med,
            "decompress_ms_range": [1e3 * d_min, 1e3 * d_max], "container_bytes": len(avrc),
            "cut_blocks": len(seams), "pieces_of_cut_blocks": pieces, "seams_bytes": sum(seams),
            "seams_share": sum(seams) / len(avrc)}


def main():
    ctx = avr.Context(0)
    ctx.split_p32 = True
    corpus = dict(workloads.corpus(ctx, fixtures=False))
    cases = {"4K_IBBP_1spf_444": corpus["4K_IBBP_1spf_444"], "4K_444_intra_slice": ctx.synthesize(WIDE, 1)}
    out = {"method": f"median of {CALLS} calls after {WARMUPS} warm-ups; checked ctx.compress, ctx.decompress",
           "split_bytes": avr.SPLIT_BYTES_DEFAULT, "cases": {}}
    for name, data in cases.items():
        rec = {"bytes": len(data), "largest_payloads": sorted(avr.slice_payload_sizes(data).tolist(), reverse=True)[:4]}
        for label, model, split in (("P32_split_off", avr.MODEL_PARALLEL32, 0),
                                    ("P32_split_on", avr.MODEL_PARALLEL32, avr.SPLIT_BYTES_DEFAULT),
                                    ("P64_split_off", avr.MODEL_PARALLEL, 0),
                                    ("P64_split_on", avr.MODEL_PARALLEL, avr.SPLIT_BYTES_DEFAULT)):
            rec[label] = measure(ctx, data, model, split)
            print(name, label, json.dumps(rec[label]), file=sys.stderr, flush=True)
        for m in ("P32", "P64"):
            rec[f"{m}_decompress_gain"] = rec[f"{m}_split_off"]["decompress_ms"] / rec[f"{m}_split_on"]["decompress_ms"]
        out["cases"][name] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
