"""The host steps of the split compress of slice batches (avr_split_plan and avr_seams_build in
avrecode_amd/csrc/avr_seams.cpp, avr_assemble_container_seams(_parsed) in avr_assemble.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/seams_build_fuzz.cpp is a stand-alone program with its own main: it links the host-only
sources with g++ -fsanitize=address,undefined and -lz -- no ROCm include path, no HIP library, no
device, nothing preloaded, not through Python -- which is also the standing proof that the new entry
points need no device (avr::shared_bytes, the one kernel-side symbol avr_assemble.cpp uses, is a stub
in the program).  It lays the oracle's split container of realshort.mp4 out as the batch a split walk
leaves (the parse, avr_split_plan's slots, the piece plan's records), requires avr_seams_build and
the assembly to reproduce the container byte for byte, then mutates counts, slots, piece ends,
strides, record counts, buffer lengths, descriptors, results, the records' coder fields and the
seams offsets / lengths of the assembly.  Every buffer is a heap allocation of exactly the length
passed.  Any sanitizer report, a positive status or an accepted call that describes bytes outside
its blob fails the test.

Two seeds of 1,500 mutated batches (about 8 s each here), after the sanitized build (about 15 s)."""
import shutil
import subprocess

import pytest

from _oracle import ROOT, oracle_cli

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "seams_build_fuzz.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp", "avr_assemble.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SPLIT_BYTES = 1024


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "seams_build_fuzz"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    p = tmp_path_factory.mktemp("seams_build_fuzz") / "realshort_P_1024.avrc"
    p.write_bytes(oracle_cli("compress", FIX / "realshort.mp4", mode="P", split_bytes=SPLIT_BYTES))
    return p


def _run(harness, iters, seed, container):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed), str(SPLIT_BYTES), str(FIX / "realshort.mp4"),
                        str(container)], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_the_valid_batch_builds_the_oracles_container(harness, container):
    _run(harness, 0, 0, container)


@pytest.mark.parametrize("seed", [1, 2])
def test_seams_build_and_assembly_mutations_under_sanitizers(harness, container, seed):
    out = _run(harness, 1500, seed, container)
    print(out)
    built, refused = (int(out.split(w)[0].split()[-1]) for w in (" built", " refused;"))
    assert built > 50 and refused > 50   # the mutations reach both sides of the checks
