"""The piece plans of the P32 coder's split containers (tags avrecode-amd:P32S / P32SE;
avr_dec_plan_load_pieces, avrecode_amd/csrc/avr_plan.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer.

tests/native/split32_plan_fuzz.cpp is a stand-alone program with its own main: it links the host-only
sources with g++ -fsanitize=address,undefined and -lz -- no ROCm include path, no HIP library, no
device, nothing preloaded, not through Python.  It retags the oracle's P64 split container of
realshort.mp4 (the plan layer decodes no stream), requires the S-tagged plans to list what the P64
plan lists and the plain P32 tags to refuse the seams, then feeds seeded mutations of the retagged
container through avr_dec_plan_load_pieces and reads every accepted plan out into buffers of exactly
the reported sizes.  Any sanitizer report, an undocumented status or a unit outside its buffers
fails the test.

Two seeds of 1,500 mutated containers (a few seconds each), after the sanitized build."""
import shutil
import subprocess

import pytest

from _oracle import ROOT, oracle_cli

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "split32_plan_fuzz.cpp"
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
    exe = BUILD / "split32_plan_fuzz"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    p = tmp_path_factory.mktemp("split32_plan_fuzz") / "realshort_P_1024.avrc"
    p.write_bytes(oracle_cli("compress", FIX / "realshort.mp4", mode="P", split_bytes=SPLIT_BYTES))
    return p


def _run(harness, iters, seed, container):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed), str(container)], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_the_retagged_containers_plan_like_the_p64_one(harness, container):
    _run(harness, 0, 0, container)


@pytest.mark.parametrize("seed", [1, 2])
def test_piece_plan_mutations_under_sanitizers(harness, container, seed):
    out = _run(harness, 1500, seed, container)
    print(out)
    accepted, refused = (int(out.split(w)[0].split()[-1]) for w in (" accepted", " refused;"))
    assert accepted > 50 and refused > 50   # the mutations reach both sides of the checks
