"""bench.py host logic (no GPU): the all-cores CPU baseline cuts one synthesized Annex-B stream into
standalone single-slice files (the stream's parameter sets + one slice NAL unit each).  A slice of
the parallel model is independent of its neighbours, so the oracle must give each standalone file
exactly what it gives that slice inside the whole stream -- otherwise the baseline would time
different work than the batch it stands for."""
import sys

from _oracle import ROOT, build_oracle, slices_p

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_split_slices_layout():
    s = (b"\x00\x00\x00\x01\x67SPS" + b"\x00\x00\x00\x01\x68PPS" + b"\x00\x00\x01\x65IDR\x01"
         + b"\x00\x00\x00\x00\x01\x41P\x80" + b"\x00\x00\x01\x06SEI")
    head, nals = bench._split_slices(s)
    assert head == b"\x00\x00\x00\x01\x67SPS\x00\x00\x00\x01\x68PPS"
    # trailing zero bytes before a start code are not part of the NAL unit; an SEI after the
    # first slice is neither a slice nor part of the parameter-set head
    assert nals == [b"\x00\x00\x00\x01\x65IDR\x01", b"\x00\x00\x00\x01\x41P\x80"]


def test_standalone_slices_match_the_stream():
    build_oracle()
    data = (ROOT / "tests" / "fixtures" / "paff_ipp.264").read_bytes()
    head, nals = bench._split_slices(data)
    total, whole = slices_p(data, 0, 4)
    assert total == len(nals) and len(whole) == 4
    for i in range(4):
        n, one = slices_p(head + nals[i], 0, 1)
        assert n == 1
        assert one[0]["status_c"] == whole[i]["status_c"] == 0
        assert one[0]["bins"] == whole[i]["bins"]
        assert one[0]["recoded"] == whole[i]["recoded"]
        assert one[0]["regen"] == whole[i]["regen"]


def test_bench_golden_is_consistent():
    """tests/golden/bench_batch.json (the oracle's answer for the headline batch, made by
    tests/golden/make_bench_golden.py): one record per slice, totals equal to the sums, every slice
    coded by the oracle; bench.golden_check applies it only to the batch it was made for."""
    import json

    import bench
    g = json.loads(bench.GOLDEN_BATCH.read_text())
    assert g["config"]["slices"] == len(g["slices"]) == 1024 and g["config"]["seed"] == 0
    assert g["bins_total"] == sum(s["bins"] for s in g["slices"])
    assert g["recoded_total"] == sum(s["recoded_len"] for s in g["slices"])
    assert all(s["status"] == 0 and len(s["recoded_sha256"]) == 64 for s in g["slices"])

    class A:
        slices, mb_width, mb_height, seed = 1024, 120, 68, 1
    assert bench.golden_check(None, b"", A) is None   # another seed: not this golden's batch


def test_dump_outputs_arrays(tmp_path):
    """bench.dump_outputs on a stand-in batch of host tensors: the arrays' names, dtypes and shapes,
    the per-slice sums over exactly each slice's valid bytes (a failed or uncoded slice counts as
    empty), a sample drawn from the slices' bytes laid end to end at the same positions every run."""
    import numpy as np
    import pytest
    torch = pytest.importorskip("torch")
    import avrecode_amd as avr

    n = 3
    descs = np.zeros(n, dtype=avr.SLICE_DESC)
    descs["out_offset"] = [0, 16, 48]
    descs["payload_offset"] = [0, 32, 64]
    descs["coded"] = [1, 1, 0]
    work = np.arange(1, 81, dtype=np.uint8)
    regen = np.arange(101, 181, dtype=np.uint8)
    res_c = np.zeros(n, dtype=avr.SLICE_RESULT)
    res_c["out_len"], res_c["status"], res_c["bins"] = [5, 7, 9], [0, 0, 0], [50, 70, 90]
    res_c["bill"][1] = [1, 2, 3, 4, 5, 6]
    res_d = np.zeros(n, dtype=avr.SLICE_RESULT)
    res_d["out_len"], res_d["status"] = [4, 6, 8], [0, -3, 0]

    class PS:
        pass

    class Batch:
        ps = PS()
        d_work, d_regen = torch.from_numpy(work), torch.from_numpy(regen)
        results = staticmethod(lambda which="c": res_c if which == "c" else res_d)
        verdicts = staticmethod(lambda: np.array([1, 0, 1], dtype=np.int32))

    Batch.ps.descs = descs
    bench.dump_outputs(Batch, tmp_path / "a")
    bench.dump_outputs(Batch, tmp_path / "b")
    names = {"verdict", "compress_results", "decompress_results", "recoded_sums", "recoded_sample",
             "regenerated_sums", "regenerated_sample"}
    assert {p.stem for p in (tmp_path / "a").iterdir()} == names
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    for k in names:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy"))
    assert a["verdict"].tolist() == [1, 0, 1]
    assert a["compress_results"].shape == a["decompress_results"].shape == (n, 10)
    assert a["compress_results"][1].tolist() == [7, 0, 70, 0, 1, 2, 3, 4, 5, 6]
    assert a["decompress_results"][1, :2].tolist() == [6, -3]
    w = lambda seg: [float(sum(seg)), float(sum(b * (i % 251 + 1) for i, b in enumerate(seg)))]  # noqa: E731
    # slice 2 is not coded, slice 1's decompress failed: no bytes of theirs count
    assert a["recoded_sums"].tolist() == [w(range(1, 6)), w(range(17, 24)), [0.0, 0.0]]
    assert a["regenerated_sums"].tolist() == [w(range(101, 105)), [0.0, 0.0], w(range(165, 173))]
    # 12 valid bytes each: every sample is one of them, in end-to-end order
    assert len(a["recoded_sample"]) == len(a["regenerated_sample"]) == 12
    assert set(a["recoded_sample"]) <= set(range(1, 6)) | set(range(17, 24))
    assert list(a["recoded_sample"]) == sorted(a["recoded_sample"])
