"""The decompress planner and the seams codec (avrecode_amd/csrc/avr_plan.cpp, avr_seams.cpp, over
avr_host.cpp and avr_front.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/plan_fuzz.cpp links those four files with g++ -fsanitize=address,undefined and -lz: no
ROCm include path, no HIP library, no device.  That the build succeeds is the standing proof that
the host-only translation units are HIP-free; avr_assemble.cpp, which links against the kernels'
shared_bytes, is compiled the same way without linking.  The program then drives the plan ABI of
include/avrecode.h (avr_dec_plan_*) over the oracle's containers -- realshort.mp4 in mode P unsplit
and split at 1024 and 2048 bytes, in mode R, and paff_ipp.264 in mode P -- first unmutated (the
counts are test_piece_plan_host.py's COUNTS), then over seeded mutations: front_fuzz's byte
mutations of the whole container, and seams fields inflated, mutated and deflated again, which is
what reaches seams_decode and the piece plan's layout.  Any sanitizer report, an undocumented
status, or an accepted plan that describes bytes outside its buffers fails the test.

Two seeds of 3,000 mutated containers each, half of them rewritten seams fields (about a third of
those load, and their plans are exercised): about 46 s for the whole file on a CPU-only machine --
22 s of it the sanitized builds and the oracle's containers, 11-12 s per seed."""
import shutil
import subprocess

import pytest

from _oracle import ROOT, oracle_cli

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "plan_fuzz.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# (slices, units) of realshort.mp4's piece plans: test_piece_plan_host.py COUNTS
COUNTS = {1024: (36, 77), 2048: (36, 41)}


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "plan_fuzz"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-o", str(exe)], check=True)
    # the container writer is HIP-free source too (compile only: it links against shared_bytes)
    subprocess.run(["g++"] + SAN + ["-c", str(CSRC / "avr_assemble.cpp"), "-o", str(BUILD / "avr_assemble.o")], check=True)
    return exe


@pytest.fixture(scope="module")
def specs(tmp_path_factory):
    td = tmp_path_factory.mktemp("plan_fuzz")
    out = []

    def add(kind, name, mode, split_bytes=None):
        p = td / f"{name}_{mode}_{split_bytes}.avrc"
        p.write_bytes(oracle_cli("compress", FIX / name, mode=mode, split_bytes=split_bytes))
        out.append(f"{kind}:{p}")

    add("plain", "realshort.mp4", "P", 0)
    for sb, (ns, nu) in sorted(COUNTS.items()):
        add(f"split:{ns}:{nu}", "realshort.mp4", "P", sb)
    add("ref", "realshort.mp4", "R")
    add("plain", "paff_ipp.264", "P")
    return out


def _run(harness, iters, seed, specs):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed)] + specs, capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_unmutated_containers_through_the_plan_abi(harness, specs):
    _run(harness, 0, 0, specs)


@pytest.mark.parametrize("seed", [1, 2])
def test_plan_and_seams_mutations_under_sanitizers(harness, specs, seed):
    print(_run(harness, 3000, seed, specs))
