"""The CRC, the fold and the splice check of checked containers (Recoded.Metadata field 16) under
AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/crc_check.cpp is a stand-alone program with its own main: g++ -fsanitize=address,undefined
links it with the host translation units (avr_front.cpp, avr_host.cpp, avr_seams.cpp, avr_plan.cpp,
avr_assemble.cpp; no ROCm include path, no HIP library, no device), the way
tests/test_escaped_sanitizers.py builds escaped_fuzz.  It checks avr_crc32 / avr_crc32_combine against
a bit-by-bit CRC, the fold against the CRC of its items' bytes written out, restores cockatoo.mp4 from
its checked container, and puts seeded mutations of that container through the plan and the splice: a
splice that returns AVR_OK has written a file with the container's CRC.  The container comes from the
oracle's per-slice streams (the ordinary library assembles it here; the program under the sanitizers
is never loaded into Python)."""
import shutil
import subprocess

import pytest

from _oracle import ROOT

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "crc_check.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp", "avr_assemble.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "crc_check"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-lpthread", "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    from test_checksum_host import _checked
    p = tmp_path_factory.mktemp("crc_check") / "cockatoo_k.avrc"
    p.write_bytes(_checked("cockatoo.mp4")[1])
    return p


def _run(harness, container, iters, seed):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed), str(FIX / "cockatoo.mp4"), str(container)],
                       capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_crc_fold_and_the_unmutated_container(harness, container):
    _run(harness, container, 0, 0)


@pytest.mark.parametrize("seed", [1, 2])
def test_mutated_checked_containers_under_sanitizers(harness, container, seed):
    print(_run(harness, container, 600, seed))
