"""Authored streams on the host (tests/_author.py, oracle/oracle_author.c): the streams the oracle writes
at the extremes of the CABAC syntax are what the table says they are, reach what they are meant to reach,
and pass through the oracle itself and the product's host front end.

* every spec regenerates to the sha256, size and census pinned in tests/golden/authored.json;
* the committed census meets the coverage conditions (long level / mvd escapes, ref_idx 31, mb_qp_delta of
  52 bins, cabac_init_idc 0..2 in P and in B slices, slice_qp 0 and 51, bins per byte of `sparse`);
* nothing is left out: every slice of every spec is recodable by the oracle on both coders and no NAL unit
  carries an emulation-prevention byte (`escaped` is the one spec made to carry some);
* recode_oracle roundtrip succeeds in R, P, P32 and C;
* avr.parse_stream sees every slice as the author recorded it;
* the product's context initialisation tables (h264_tables.h) give the oracle's state bytes for every
  cabac_init_idc, slice_qp and context (tests/native/init_tables_check.cpp).  The two tables are separate
  transcriptions of ITU-T H.264 Tables 9-12..9-33 and pin each other only: nothing in this repository
  holds a third, so an error both share would pass.
* the bounds streams (section "bounds" of the table): at the bounds every slice is recodable, one past
  them exactly the forced slices are refused, with the walker's status for that bound."""
import hashlib
import json
import shutil
import subprocess

import pytest

import _author
from _oracle import ROOT, oracle_cli, slices_p

import avrecode_amd as avr

PINS = json.loads((ROOT / "tests" / "golden" / "authored.json").read_text())
ALL = list(_author.SPECS) + list(_author.BOUNDS)
PB_SPECS = [n for n in _author.SPECS]   # every spec holds P and B slices


def _count(census, key, lo, hi=10 ** 9):
    return sum(v for k, v in census[key].items() if lo <= int(k) <= hi)


def test_table_and_pins_name_the_same_specs():
    assert sorted(PINS) == sorted(ALL)


@pytest.mark.parametrize("name", ALL)
def test_stream_matches_pin(name):
    args, kw = _author.SPECS.get(name) or _author.BOUNDS[name]
    data, census = _author.author(*args, **kw)          # not the cached one: authored again
    pin = PINS[name]
    assert len(data) == pin["size"]
    assert hashlib.sha256(data).hexdigest() == pin["sha256"]
    assert json.loads(json.dumps(census)) == pin["census"]
    assert data == _author.stream(name)[0]              # same parameters, same bytes


@pytest.mark.parametrize("name", _author.LEVEL_SPECS)
def test_level_specs_reach_long_escapes(name):
    c = PINS[name]["census"]
    assert c["level_escapes"] >= 1000
    assert c["level_escapes"] == _count(c, "level_len", 0)
    assert _count(c, "level_len", 6) >= 100
    for k in range(6, 16):
        assert c["level_len"].get(str(k), 0) >= 1, k


@pytest.mark.parametrize("name", _author.MOTION_SPECS)
def test_motion_specs_reach_long_escapes(name):
    c = PINS[name]["census"]
    assert c["mvd_escapes"] >= 100
    assert c["mvd_k"].get("24", 0) >= 1
    assert c["ref_idx"].get("31", 0) >= 1
    assert c["qp_delta_len"].get("52", 0) >= 1


@pytest.mark.parametrize("name", PB_SPECS)
def test_every_init_table_and_both_qp_ends(name):
    c = PINS[name]["census"]
    for st in ("P", "B"):
        assert all(n >= 1 for n in c["idc_used"][st]), (st, c["idc_used"])
    assert c["qp_used"].get("0", 0) >= 1 and c["qp_used"].get("51", 0) >= 1
    # and the slices say so themselves
    seen = {(s["slice_type"], s["cabac_init_idc"]) for s in c["slice"]}
    assert {(t, i) for t in (0, 1) for i in (0, 1, 2)} <= seen


def test_sparse_bins_per_byte():
    c = PINS["sparse"]["census"]
    assert c["bins"] >= 8 * c["payload_bytes"]
    pb = [s for s in c["slice"] if s["slice_type"] != 2]
    assert sum(s["bins"] for s in pb) >= 8 * sum(s["payload_bytes"] for s in pb)


def _emulation_bytes(data):
    """00 00 03 inside the NAL units of an Annex-B stream with 4-byte start codes (7.4.1)."""
    return sum(nal.count(b"\x00\x00\x03") for nal in data.split(b"\x00\x00\x00\x01")[1:])


@pytest.mark.parametrize("name", list(_author.SPECS))
def test_nothing_left_out(name):
    data, census = _author.stream(name)
    assert census["refused_slices"] == 0
    if name == "escaped":
        assert census["emulation_bytes"] >= 1
    else:
        assert census["emulation_bytes"] == 0
    assert _emulation_bytes(data) == census["emulation_bytes"]
    for p32 in (False, True):
        total, recs = slices_p(data, p32=p32)
        assert total == census["slices"] == len(recs)
        for k, r in enumerate(recs):
            assert r["recodable"] == 1 and r["status_c"] == 0 and r["status_d"] == 0, (k, p32, r["status_c"])
            assert r["bins"] == census["slice"][k]["bins"], k
    if name == "sparse":   # near-all-skip slices whose re-coded form is larger than the slice
        assert sum(len(r["recoded"]) > s["payload_bytes"] for r, s in zip(recs, census["slice"])) >= 3


@pytest.mark.parametrize("name", ALL)
def test_oracle_roundtrip_every_model(name, tmp_path):
    data, census = _author.stream(name)
    f = tmp_path / "a.264"
    f.write_bytes(data)
    # not coded: the refused slices, and those whose NAL unit carries emulation-prevention bytes
    skipped = census["refused_slices"] + sum(b"\x00\x00\x03" in nal for nal in data.split(b"\x00\x00\x00\x01")[1:])
    coded = census["slices"] - skipped
    for mode in ("R", "P", "P32", "C"):
        out = oracle_cli("roundtrip", f, mode).decode()
        assert "roundtrip succeeded" in out, (mode, out)
        assert f" slices {census['slices']} coded {coded} skipped {skipped} " in out, (mode, out)


@pytest.mark.parametrize("name", ALL)
def test_host_front_end_sees_the_authors_slices(name):
    data, census = _author.stream(name)
    args, kw = _author.SPECS.get(name) or _author.BOUNDS[name]
    w, h = args[:2]
    d = avr.parse_stream(data).descs
    assert len(d) == census["slices"]
    for k, s in enumerate(census["slice"]):
        for f in ("slice_type", "slice_qp", "cabac_init_idc", "first_mb", "structure"):
            assert int(d[k][f]) == s[f], (k, f)
        assert (int(d[k]["mb_width"]), int(d[k]["mb_height"])) == (w, h)
        # FFmpeg's payload size leaves out a last byte that holds the stop bit alone
        assert s["payload_bytes"] - 1 <= int(d[k]["payload_size"]) <= s["payload_bytes"], k
        assert int(d[k]["num_ref_idx_l0"]) == (0 if s["slice_type"] == 2 else kw.get("refs", 1))
    assert d["coded"].all()   # every slice is a device candidate (the file search decides on escaped ones)


# ------------------------------------------------------------------------------ the init tables
@pytest.fixture(scope="module")
def init_tables_check():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    build = ROOT / "tests" / "native" / "_build"
    build.mkdir(parents=True, exist_ok=True)
    exe = build / "init_tables_check"
    _author.lib()   # liboracle.so is built
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", str(ROOT / "oracle"),
                    "-I", str(ROOT / "avrecode_amd" / "csrc"), str(ROOT / "tests" / "native" / "init_tables_check.cpp"),
                    "-L", str(ROOT / "oracle"), "-loracle", f"-Wl,-rpath,{ROOT / 'oracle'}", "-o", str(exe)], check=True)
    return exe


def test_init_tables_agree_with_the_oracle(init_tables_check):
    """4 x 52 x 1,024 state bytes of the product's tables against the oracle's.  Two separate
    transcriptions of the standard's tables that pin each other: there is no third on this side."""
    r = subprocess.run([str(init_tables_check)], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"no finding" in r.stdout, r.stdout.decode()[-2000:]
    assert b"212992 states compared, 0 differ" in r.stdout


@pytest.mark.parametrize("idc,ctx", [(1, 11), (1, 227), (1, 459), (2, 40), (2, 54), (2, 402), (0, 60), (-1, 5)])
def test_init_tables_check_sees_one_wrong_pair(init_tables_check, idc, ctx):
    """The check is sharp: one (m, n) pair off by one in m is a finding, whichever table it is in."""
    r = subprocess.run([str(init_tables_check), str(idc), str(ctx)], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"differ" in r.stdout and b"no finding" not in r.stdout


# ------------------------------------------------------------------------------ the bounds
def test_bounds_accepted_on_the_oracle():
    data, census = _author.stream("bounds_accepted")
    assert census["level_len"].get("30", 0) >= 2 and census["mvd_k"].get("24", 0) >= 2
    assert census["qp_delta_len"].get("102", 0) == 2 and census["refused_slices"] == 0
    assert not any(int(k) > 30 for k in census["level_len"]) and not any(int(k) > 24 for k in census["mvd_k"])
    for p32 in (False, True):
        _, recs = slices_p(data, p32=p32)
        assert all(r["recodable"] == 1 and r["status_c"] == 0 and r["status_d"] == 0 for r in recs)


@pytest.mark.parametrize("name,status", [("bounds_refused", [-5, -4, -6, -5]), ("bounds_refused_mbaff", [-3, -4])])
def test_bounds_refused_on_the_oracle(name, status):
    """One bin past each bound: the oracle's walker ends the slice with that bound's status (-5 level, -4
    mvd, -6 mb_qp_delta, -3 ref_idx) and the slice is not coded; its neighbour in the picture is."""
    data, census = _author.stream(name)
    refused = [k for k, s in enumerate(census["slice"]) if s["refused"]]
    assert len(refused) == len(status) == census["refused_slices"]
    if name == "bounds_refused":
        assert census["level_len"]["31"] == 2 and census["mvd_k"]["25"] == 1 and census["qp_delta_len"]["103"] == 1
    else:
        assert census["ref_idx"]["32"] == 1 and census["mvd_k"]["25"] == 1
    for p32 in (False, True):
        _, recs = slices_p(data, p32=p32)
        assert [k for k, r in enumerate(recs) if not r["recodable"]] == refused
        assert [recs[k]["status_c"] for k in refused] == status
        assert all(k + 1 not in refused for k in refused)   # each next to an ordinary slice
