"""The walkers' hot loops after their rare sides moved out of line: small synthetic streams through the
resident and the split kernels, slice by slice against the oracle.

The layout hints (AVR_LIKELY / AVR_UNLIKELY, avr_engine.h) move every rare path of a per-bin branch --
a refill, a ring flush, an escape, an estimator fallback, an error exit -- to another place in the
kernel.  That may not change a byte.  Each stream below is 6 x 4 macroblocks, two slices per picture
(12 macroblocks, two rows: one possible cut for the split kernels), eight pictures = 16 slices.  The
comment beside a stream says which rare paths its content is meant to exercise; what the results can
show of that is asserted (RARE: escapes, window refills, sparse maps), the rest is the stream's
intent, checked only through the bytes.

* resident kernels (DeviceBatch.roundtrip): every slice's bin count, re-coded bytes and regenerated
  payload equal the oracle's fresh-model path (`_oracle.slices_p`), every slice bit-exact;
* split kernels (SplitBatch.roundtrip over the stream's split candidates, and the whole-file compress /
  decompress, which runs them too): every candidate bit-exact on the device, its bin count equal to
  `slices_p`'s, its re-coded bytes equal to `slices_p`'s where the walk did not cut it and to the
  oracle's container at that split where it did; the container equals the oracle's and decompresses to
  the stream (a slice is a candidate from 1.5 split_bytes of payload on; each stream's split_bytes is
  chosen so that at least three of its slices are);
* the rare paths were reached, read off the results: see RARE below.

Coefficient positions: a macroblock holds 384 (4:2:0) or 768 (4:4:4) coefficients at the most, so
`macroblocks * that` bounds the stream's coefficient count from above.  A stream whose bins exceed it
spends more than one bin per possible coefficient: dense maps and long level prefixes, the escape
path (coeff_abs_level_minus1 >= 14) among them."""
import tempfile
from pathlib import Path

import numpy as np
import pytest

from _oracle import oracle_cli, patch_restores, slices_p

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402
from avrecode_amd.batch import DeviceBatch, SplitBatch  # noqa: E402

pytestmark = pytest.mark.gpu
K_STAGE = 1024   # avr_engine.h kStage: bytes per LDS input window
W, H, SPP, PICS = 6, 4, 2, 8

# id: (slice_type, qp, chroma_format_idc, transform_8x8_mode, split_bytes)
STREAMS = {
    # the lowest QP the generator takes (slice_qp_delta = -26): dense 8x8 blocks and long level prefixes.
    # Asserted: more than one bin per coefficient position (escapes), payloads and re-coded streams
    # longer than the input window (in_fill_call from cd_refill and from the recoded decoder's digits).
    # Meant as well, not asserted: more than 64 staged level ops inside one block, full rings
    "i420_t8_qp0": (2, 0, 1, 1, 512),
    # the same without the 8x8 transform: 4x4-class maps only (the maps with deferred estimator stores),
    # blocks of 16 coefficients with long prefixes; the same two assertions
    "i420_t4_qp0": (2, 0, 1, 0, 512),
    # QP 22, the benchmark's neighbourhood: level-1 coefficients and zero map bins as the common path
    "i420_t8_qp22": (2, 22, 1, 1, 256),
    # P slices after an I picture (gop 4): mvd and ref_idx bins, skip runs, the P contexts' init tables
    "p420_t8_qp22": (0, 22, 1, 1, 128),
    "p420_t4_qp22": (0, 22, 1, 0, 128),
    # 4:4:4: the Cb / Cr planes coded like luma (ctxBlockCat 6-13: other context lanes and estimator bases)
    "i444_t8_qp22": (2, 22, 3, 1, 256),
    # a high QP: sparse maps (most blocks uncoded, maps that end at their first coefficient), P skips
    "p420_t8_qp40": (0, 40, 1, 1, 48),
}
# what each stream has to show in its results (test_rare_paths_were_reached)
RARE = {
    "i420_t8_qp0": ("escapes", "window"),
    "i420_t4_qp0": ("escapes", "window"),
    "p420_t8_qp40": ("sparse",),
}


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    yield c
    c.close()


_cache = {}


def _case(ctx, name):
    """Everything of one stream, made once: the stream, the oracle's answer, the resident run."""
    if name in _cache:
        return _cache[name]
    st, qp, cf, t8, split = STREAMS[name]
    p = avr.SynthParams(mb_width=W, mb_height=H, slice_type=st, slice_qp=qp, chroma_format_idc=cf,
                        transform_8x8_mode=t8, num_ref_idx_l0=2, seed=8100 + 7 * qp + 3 * cf + t8 + st,
                        slices_per_picture=SPP, gop_length=4 if st != 2 else 0)
    data = ctx.synthesize(p, PICS)
    ps = avr.parse_stream(data)
    total, ref = slices_p(data)
    assert total == len(ps.descs) == SPP * PICS
    b = DeviceBatch(ctx, ps)
    b.roundtrip(avr.MODEL_PARALLEL)
    torch.cuda.synchronize()
    c = dict(data=data, ps=ps, ref=ref, split=split, verdict=b.verdicts(), rc=b.results("c").copy(),
             recoded=b.recoded(), regen=b.regenerated(), payloads=b.payloads())
    print(f"{name}: payload bytes {[int(x) for x in ps.descs['payload_size']]} re-coded bytes "
          f"{[int(x) for x in c['rc']['out_len']]} bins {[int(x) for x in c['rc']['bins']]}")
    _cache[name] = c
    return c


@pytest.mark.parametrize("name", list(STREAMS))
def test_resident_kernels_match_oracle(ctx, name):
    c = _case(ctx, name)
    # (a P slice of nothing but skips, two payload bytes, is not recodable for the oracle either)
    assert sum(bool(r["recodable"]) for r in c["ref"]) >= len(c["ref"]) // 2
    for k, r in enumerate(c["ref"]):
        assert (c["verdict"][k] == 1) == bool(r["recodable"]), (k, int(c["verdict"][k]), r["recodable"])
        if not r["recodable"]:
            continue
        assert r["status_c"] == 0 and r["status_d"] == 0 and c["rc"][k]["status"] == 0, (k, r["status_c"], r["status_d"])
        assert c["rc"][k]["bins"] == r["bins"], k
        assert c["recoded"][k] == r["recoded"], f"slice {k}: re-coded bytes differ"
        assert c["regen"][k] == r["regen"], f"slice {k}: regenerated bytes differ"
        assert patch_restores(c["regen"][k], c["payloads"][k]), k


@pytest.mark.parametrize("name", list(STREAMS))
def test_split_kernels_match_oracle(ctx, name):
    c = _case(ctx, name)
    data, ps, ref, split = c["data"], c["ps"], c["ref"], c["split"]
    idx = np.flatnonzero(avr.split_plan(ps.descs, split).candidate & (ps.descs["coded"] != 0))
    print(f"{name}: split {split}, candidates {len(idx)} of {len(ps.descs)}")
    assert len(idx) >= 3, "the stream's split leaves the split kernels too few slices"
    ctx.split_bytes = split
    try:
        avrc = ctx.compress(data, avr.MODEL_PARALLEL)
        with tempfile.TemporaryDirectory() as td:
            f = Path(td) / "s.264"
            f.write_bytes(data)
            assert avrc == oracle_cli("compress", f, mode="P", split_bytes=split)
        assert ctx.decompress(avrc) == data
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT
    blocks = [b for b in avr.describe_container(avrc)[0]["blocks"] if "literal" not in b]
    assert len(blocks) == len(ps.descs)
    sb = SplitBatch(ctx, shard.select(ps, idx), split)
    sb.roundtrip()
    torch.cuda.synchronize()
    assert (sb.verdicts() == 1).all(), sb.verdicts()   # the payloads regenerated, compared on the device
    recoded = sb.recoded()
    print(f"{name}: cuts {[int(x) for x in sb.cuts]}")
    for j, k in enumerate(idx):
        assert sb.res[j]["status"] == 0 and sb.res[j]["bins"] == ref[k]["bins"], (k, int(sb.res[j]["bins"]), ref[k]["bins"])
        assert recoded[j] == bytes.fromhex(blocks[k]["cabac"]), f"slice {k}: re-coded bytes differ from the container's"
        assert (sb.cuts[j] > 0) == ("seams" in blocks[k]), k
        if not sb.cuts[j]:   # an uncut walk is the fresh-model path itself
            assert recoded[j] == ref[k]["recoded"], f"slice {k}: re-coded bytes differ"


@pytest.mark.parametrize("name", list(RARE))
def test_rare_paths_were_reached(ctx, name):
    c = _case(ctx, name)
    ps, rc = c["ps"], c["rc"]
    cf = STREAMS[name][2]
    positions = W * H * PICS * (768 if cf == 3 else 384)   # the stream's coefficient count at the most
    bins = int(rc["bins"].sum())
    print(f"{name}: bins {bins}, coefficient positions {positions}, longest payload "
          f"{int(ps.descs['payload_size'].max())}, longest re-coded stream {int(rc['out_len'].max())}")
    if "escapes" in RARE[name]:
        assert bins > positions
    if "window" in RARE[name]:
        # both walkers' inputs outgrow the LDS window: the compress walker reads the payload, the
        # decompress walker the re-coded stream
        assert int(ps.descs["payload_size"].min()) > K_STAGE and int(rc["out_len"].min()) > K_STAGE
    if "sparse" in RARE[name]:
        assert bins < positions   # the other side of the same line: under one bin per possible coefficient
