"""escape(), decompress_setup and the splice on containers with Block field 17 under
AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/escaped_fuzz.cpp is a stand-alone program: g++ -fsanitize=address,undefined links it
with the host translation units (avr_front.cpp, avr_host.cpp, avr_seams.cpp, avr_plan.cpp,
avr_assemble.cpp; no ROCm include path, no HIP library, no device), the way
tests/test_plan_sanitizers.py builds plan_fuzz.  It checks escape() on the edge cases of
tests/test_escaped_host.py, restores cockatoo.mp4 from its escaped container with the file's own
payloads, and puts seeded mutations of that container -- byte mutations, and field 17 rewritten to
every value the format refuses -- through the plan and the splice.  The container comes from the
oracle's per-slice streams (the ordinary library assembles it here; the program under the
sanitizers is never loaded into Python)."""
import shutil
import subprocess

import pytest

from _oracle import ROOT

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "escaped_fuzz.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp", "avr_assemble.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "escaped_fuzz"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-lpthread", "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    from test_escaped_host import _cockatoo_e
    p = tmp_path_factory.mktemp("escaped_fuzz") / "cockatoo_e.avrc"
    p.write_bytes(_cockatoo_e()[1])
    return p


def _run(harness, container, iters, seed):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
           "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness), str(iters), str(seed), str(FIX / "cockatoo.mp4"), str(container)],
                       capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_escape_rule_and_the_unmutated_container(harness, container):
    _run(harness, container, 0, 0)


@pytest.mark.parametrize("seed", [1, 2])
def test_mutated_escaped_containers_under_sanitizers(harness, container, seed):
    print(_run(harness, container, 1500, seed))
