"""The compress planner (avrecode_amd/csrc/avr_cplan.cpp) and the one-line rules of avr_host.h, on
the CPU under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/cplan_check.cpp is a stand-alone program with its own main: it links the HIP-free
sources with g++ -fsanitize=address,undefined and -lz -- no ROCm include path, no HIP library, no
device, nothing preloaded, not through Python (avr::shared_bytes, the one kernel-side symbol
avr_assemble.cpp uses, is a stub in the program).  What it checks is what compress and decompress
must apply alike, and what only GPU tests reached before: the chained model's chain rule, the
chain cuts of both directions on a chained container of the oracle, partition_range against
shard.partition, the frame generations of the parallel reference-model pass, the last-byte rule.

The sanitized build takes about 20 s, each check well under a second."""
import random
import shutil
import subprocess

import pytest

from _oracle import ROOT, oracle_cli

CSRC = ROOT / "avrecode_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "cplan_check.cpp"
LINKED = [CSRC / n for n in ("avr_front.cpp", "avr_host.cpp", "avr_seams.cpp", "avr_plan.cpp", "avr_cplan.cpp",
                             "avr_assemble.cpp")]
BUILD = ROOT / "tests" / "native" / "_build"
FIX = ROOT / "tests" / "fixtures"
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "cplan_check"
    subprocess.run(["g++"] + SAN + [str(SRC)] + [str(f) for f in LINKED] + ["-lz", "-o", str(exe)], check=True)
    return exe


def _run(harness, *args):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(harness)] + [str(a) for a in args], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    assert b"no finding" in r.stdout
    return r.stdout.decode()


def test_cplan_compiles_without_rocm(tmp_path):
    """avr_cplan.cpp is a HIP-free unit: g++ -std=c++17 compiles it with no ROCm include path."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", str(CSRC / "avr_cplan.cpp"), "-o",
                    str(tmp_path / "avr_cplan.o")], check=True)


def test_chain_rule(harness):
    """chain_starts and the file_first appender against a brute-force statement of the rule: 0, 1,
    15, 16, 17, 32 and 33 coded slices, with no, one and three uncoded slices before, after and
    around every multiple-of-16 coded slice."""
    assert "63 flag vectors" in _run(harness, "chain")


def _tiled(copies=5, lead=0):
    """tests/test_gpu_chained.py::_tiled: the PAFF fixture's 8 slices tiled, `lead` slices of the
    first GOP before the tiles."""
    import bench
    head, sl = bench._split_slices((FIX / "paff_ipp.264").read_bytes())
    return head + b"".join(sl[:lead] + sl * copies)


@pytest.mark.parametrize("lead", [0, 3], ids=["idr_aligned", "mid_gop"])
def test_compress_and_decompress_cut_alike(harness, tmp_path, lead):
    """paff_ipp.264 tiled to 40 (43) slices, three chains: the reference plan built from the file and
    the decompress plan built from the oracle's chained container have the same file_first and the
    same number of descriptors.  (The oracle codes every candidate of this fixture, which the
    program checks: the premise of comparing the two.)"""
    f = tmp_path / "x.264"
    f.write_bytes(_tiled(lead=lead))
    c = tmp_path / "x.avrc"
    c.write_bytes(oracle_cli("compress", f, mode="C"))
    out = _run(harness, "cut", f, c)
    assert f"{40 + lead} slices, {40 + lead} coded, 3 chains" in out


def test_partition_range_equals_shard_partition(harness, tmp_path):
    """Seeded cases, world 1 to 8 and 0 to 40 units of integer byte counts (all zero, one unit
    heavier than the rest together, fewer units than ranks among them): every rank's [lo, hi) equals
    shard.partition's.  The totals are far below 2^53, so every sum is exact in both languages and
    the comparison is exact."""
    from avrecode_amd import shard
    rng = random.Random(20240611)
    cases = []
    for world in range(1, 9):
        for n in list(range(0, 9)) + [rng.randrange(9, 41) for _ in range(6)] + [40]:
            kinds = [[rng.randrange(0, 1 << 20) for _ in range(n)],
                     [rng.choice([0, 0, 1, 4096, 1 << 30]) for _ in range(n)],
                     [0] * n,
                     [7] * n]
            if n:
                heavy = [rng.randrange(1, 1000) for _ in range(n)]
                heavy[rng.randrange(n)] = sum(heavy) + 1
                kinds.append(heavy)
            cases += [(world, w) for w in kinds]
    assert any(len(w) < world for world, w in cases) and any(w and not sum(w) for _, w in cases)
    lines = []
    for world, w in cases:
        cuts = shard.partition(w, world)
        assert len(cuts) == world
        lines.append(" ".join(map(str, [world, len(w)] + w + [int(x) for lohi in cuts for x in lohi])))
    p = tmp_path / "partition_cases.txt"
    p.write_text("\n".join(lines) + "\n")
    assert f"{len(cases)} cases" in _run(harness, "partition", p)


def test_rmode_generations(harness):
    """Hand-built descriptor sequences: a generation per picture with the previous one as the other
    frame, slices of one picture sharing theirs, a new file resetting both frames, the fallback on
    more than 4 GiB of metadata, the first-field bit.

    The issue's fourth case (a size change while the other frame holds a generation of the old
    size returns the fallback) describes a state the rule cannot reach: update_frame_spec
    (recode.cpp:829-835) re-initialises the other frame together with the current one, so both
    frames always have one size and the stale-frame guard never fires.  The program asserts what the
    rule gives there instead: the pass goes on, goff[2k + 1] == -1 at the change, and the next
    picture sees the new generation."""
    _run(harness, "rmode")


def test_last_byte_rule(harness):
    """The three outcomes over has_parity x has_last_byte x empty / non-empty last_byte x parity
    equal / different x length 0 / 1."""
    assert "32 cases" in _run(harness, "lastbyte")
