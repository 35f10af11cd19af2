"""The range planner (avrecode_amd/csrc/avr_plan.cpp: avr_dec_plan_file_size / _range / _range_apply,
over avr_seams.cpp, avr_host.cpp and avr_front.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/range_check.cpp is a stand-alone program linked from those four HIP-free files with
g++ -fsanitize=address,undefined and -lz, exactly as tests/native/plan_fuzz.cpp is
(tests/test_plan_sanitizers.py): no ROCm include path, no HIP library, no device, nothing loaded into
Python.  It plans and applies the window list of tests/test_range_plan_host.py over the oracle's
containers of realshort.mp4 (unsplit, split at 1024 and at 2048) and cockatoo.mp4 (split at 2048) into
buffers of exactly the planned sizes -- a call that returns 0 wrote exactly the file's bytes -- and then
seeded mutations of those containers, whose accepted plans are applied blind: every call returns a
documented status and no byte outside a window or a unit's share is touched."""
import shutil
import subprocess

import pytest

from _oracle import ROOT, oracle_cli

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "range_check.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CASES = [("realshort.mp4", 0), ("realshort.mp4", 1024), ("realshort.mp4", 2048), ("cockatoo.mp4", 2048)]


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "range_check"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    td = tmp_path_factory.mktemp("range_check")
    out = []
    for name, split_bytes in CASES:
        p = td / f"{name}_{split_bytes}.avrc"
        p.write_bytes(oracle_cli("compress", FIX / name, mode="P", split_bytes=split_bytes))
        out += [str(p), str(FIX / name)]
    return out


def _run(harness, iters, seed, pairs):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed)] + pairs, capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_true_windows_restore_the_files_bytes(harness, pairs):
    print(_run(harness, 0, 0, pairs))


@pytest.mark.parametrize("seed", [1, 2])
def test_mutated_containers_under_sanitizers(harness, pairs, seed):
    # the mutations draw on the realshort containers only: cockatoo's would mostly time its parse
    print(_run(harness, 1500, seed, pairs[:6]))
