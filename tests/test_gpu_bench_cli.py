"""bench.py on one GPU as the driver runs it: a plain run and a --full run, at tiny sizes.

* A plain run (`--gpus 1 --steps K --warmup W`) times K steps and prints one JSON line with the
  headline keys; none of the other legs' keys (they run only with --full).
* --dump-outputs DIR writes the last step's outputs as float .npy files, at most 64 MB, identical
  from run to run with the same arguments, and every slice of the batch regenerated bit-exactly.
* --full reports the other legs in the same line.
"""
import json
import subprocess
import sys

import numpy as np
import pytest

from _oracle import ROOT

pytestmark = pytest.mark.gpu

TINY = ["--gpus", "1", "--slices", "8", "--mb-width", "40", "--mb-height", "24"]
FULL_ONLY = ("oracle_parity", "p32", "file_roundtrip", "corpus", "rmode_files", "rmode_clips", "stream_shard")


def _bench(extra):
    r = subprocess.run([sys.executable, "bench.py"] + TINY + extra, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return d, [_bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(d / tag)]) for tag in "ab"]


def test_plain_run_is_the_headline_alone(plain):
    _, (line, _) = plain
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["bit_exact"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    # value is the batch's bytes over the time of the steps: the two figures say the same
    assert line["value"] == pytest.approx(line["config"]["input_bytes_per_gpu"] / line["ms_per_step"] / 1e3, rel=1e-9)
    assert line["cpu_baseline"] is None and not [k for k in FULL_ONLY if k in line]


def test_dumped_outputs_repeat(plain):
    d, _ = plain
    files = sorted(p.name for p in (d / "a").iterdir())
    assert files == sorted(p.name for p in (d / "b").iterdir()) and "verdict.npy" in files
    assert sum(p.stat().st_size for p in (d / "a").iterdir()) <= 64 << 20
    for f in files:
        a, b = np.load(d / "a" / f), np.load(d / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0
        assert np.array_equal(a, b), f
    a = {f[:-4]: np.load(d / "a" / f) for f in files}
    assert a["verdict"].shape == (8,) and (a["verdict"] == 1).all()
    assert (a["compress_results"][:, 1] == 0).all() and (a["decompress_results"][:, 1] == 0).all()
    # the regenerated payloads are the input's: their lengths and byte sums are those of the batch
    assert (a["regenerated_sums"][:, 0] > 0).all() and (a["recoded_sums"][:, 0] > 0).all()


def test_full_run_reports_the_other_legs():
    # the quick legs only (the file, corpus and stream legs have tests of their own calls)
    line = _bench(["--full", "--steps", "1", "--warmup", "1", "--cpu-seconds", "1", "--no-files", "--no-corpus"])
    assert line["bit_exact"] is True and line["steps"] == 1
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] == 1
    assert line["p32"]["bit_exact"] is True and line["p32"]["value"] > 0
