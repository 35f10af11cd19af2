"""Slices whose NAL unit carries emulation-prevention bytes, re-coded on the device
(Context.recode_escaped; Block field 17, the "E" tags).  No kernel changes with the option: the
compress, verify and decompress walkers already handle these slices, and the option keeps what they
make.  cockatoo.mp4 has 13 such slices of 280.

* P64 and P32 with the option: the roundtrip succeeds with 280 coded and 0 skipped slices, the
  container is the host assembly of the oracle's per-slice streams with the flag (which
  tests/test_escaped_host.py holds to the format), ctx.decompress returns the file, and a context
  with the default still writes the golden container;
* split and escape together at split_bytes 512: at least one block carries both field 16 and
  field 17, ctx.decompress returns the file, and so does shard.sharded_decompress at world 1 over
  RCCL (the unit route);
* shard.sharded_compress(escaped=True) at world 1 equals ctx.compress byte for byte, unsplit and split;
* the reference and chained models ignore the option: their golden containers;
* hooks: a decompress session refuses an E container (AVR_ERR_UNSUPPORTED), a compress session on a
  context with the option on writes today's container."""
import hashlib
import json
import os
import socket

import pytest

from _oracle import ROOT
from test_escaped_host import _assemble, _counts, _outputs

torch = pytest.importorskip("torch")
import avrecode_amd as avr  # noqa: E402
from avrecode_amd import shard  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = ROOT / "tests" / "fixtures"
DATA = (FIX / "cockatoo.mp4").read_bytes()
GOLD = {(g["file"], g["mode"]): g for g in json.loads((ROOT / "tests/golden/fixtures.json").read_text())}
MODELS = {"P": avr.MODEL_PARALLEL, "P32": avr.MODEL_PARALLEL32, "R": avr.MODEL_REFERENCE, "C": avr.MODEL_CHAINED}
SPLIT = 512


@pytest.fixture(scope="module")
def ctx():
    c = avr.Context(0)
    c.recode_escaped = True
    yield c
    c.close()


@pytest.fixture(scope="module")
def world1():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def _golden(avrc, mode):
    g = GOLD[("cockatoo.mp4", mode)]
    return len(avrc) == g["avrc_len"] and hashlib.sha256(avrc).hexdigest() == g["avrc_sha256"]


def test_option_defaults_off_and_is_settable():
    with avr.Context(0) as c:
        assert c.recode_escaped is bool(int(os.environ.get("AVR_RECODE_ESCAPED", "0") or 0))
        c.recode_escaped = True
        assert c.recode_escaped is True
        c.recode_escaped = False
        assert c.recode_escaped is False


@pytest.mark.parametrize("mode", ["P", "P32"])
def test_cockatoo_codes_every_slice(ctx, mode):
    model = MODELS[mode]
    avrc, stats = ctx.roundtrip(DATA, model)
    assert (stats["slices"], stats["coded_slices"], stats["skipped_slices"]) == (280, 280, 0)
    data, st, blobs = _outputs("cockatoo.mp4", mode == "P32")
    want = _assemble(data, st, blobs, True, model=model)
    assert avrc == want
    assert ctx.compress(DATA, model) == want   # with the per-slice device check
    tag, coded, skipped, esc = _counts(avrc)
    assert (tag, coded, skipped, len(esc)) == (b"avrecode-amd:" + (b"P64E" if mode == "P" else b"P32E"), 280, 0, 13)
    assert ctx.decompress(avrc) == DATA
    with avr.Context(0) as plain:   # the default: today's container
        assert not plain.recode_escaped
        assert _golden(plain.compress(DATA, model), mode)
        assert plain.decompress(avrc) == DATA   # reading needs no option


@pytest.fixture(scope="module")
def split_container(ctx):
    ctx.split_bytes = SPLIT
    try:
        return ctx.compress(DATA, avr.MODEL_PARALLEL)
    finally:
        ctx.split_bytes = avr.SPLIT_BYTES_DEFAULT


def test_split_and_escape_together(ctx, world1, split_container):
    avrc = split_container
    d, again = avr.describe_container(avrc)
    assert again == avrc
    both = [b for b in d["blocks"] if "seams" in b and "escapes" in b]
    assert len(both) >= 1
    assert _counts(avrc)[:3] == (b"avrecode-amd:P64E", 280, 0)
    assert ctx.decompress(avrc) == DATA
    assert avr.seams_of_container(avrc)
    assert shard.sharded_decompress(ctx, avrc) == DATA   # by units


def test_sharded_compress_equals_the_whole_file_compress(ctx, world1, split_container):
    for model in (avr.MODEL_PARALLEL, avr.MODEL_PARALLEL32):
        out = shard.sharded_compress(ctx, DATA, model=model, escaped=ctx.recode_escaped)
        assert out == ctx.compress(DATA, model) and len(_counts(out)[3]) == 13
        assert shard.sharded_decompress(ctx, out) == DATA   # per slice
    assert shard.sharded_compress(ctx, DATA, split_bytes=SPLIT, escaped=True) == split_container
    # without the argument: today's container
    assert _golden(shard.sharded_compress(ctx, DATA), "P")


@pytest.mark.parametrize("mode", ["R", "C"])
def test_reference_and_chained_models_ignore_the_option(ctx, mode):
    assert ctx.recode_escaped
    avrc = ctx.compress(DATA, MODELS[mode])
    assert _golden(avrc, mode)
    rt, stats = ctx.roundtrip(DATA, MODELS[mode])
    assert rt == avrc and stats["skipped_slices"] == 13


def test_hooks_sessions(ctx, monkeypatch):
    from test_hooks import _call
    avrc = ctx.compress(DATA, avr.MODEL_PARALLEL)
    assert _counts(avrc)[0] == b"avrecode-amd:P64E"
    r, _, _ = _call("hooks_decompress", avrc, len(avrc))
    assert r == -6
    # the driver makes its own context: the option on from the environment
    monkeypatch.setenv("AVR_RECODE_ESCAPED", "1")
    with avr.Context(0) as c:
        assert c.recode_escaped
    r, out, walked = _call("hooks_compress", DATA, len(DATA), avr.MODEL_PARALLEL)
    assert r == 0 and walked > 0 and _golden(out, "P")


def test_cli_flag(tmp_path):
    """`recode roundtrip|compress -p -e` (either order of the flags); -e without a parallel model is refused."""
    import subprocess
    cli = ROOT / "avrecode_amd" / "recode"
    assert cli.exists(), "recode CLI not built (make -C avrecode_amd)"
    src = FIX / "cockatoo.mp4"
    r = subprocess.run([str(cli), "roundtrip", "-p", "-e", str(src)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b" slices 280 coded 280 skipped 0 " in r.stdout, (r.stdout, r.stderr)
    out = tmp_path / "e.avrc"
    r = subprocess.run([str(cli), "compress", "-e", "-p32", str(src), str(out)], capture_output=True, timeout=120)
    assert r.returncode == 0 and _counts(out.read_bytes())[0] == b"avrecode-amd:P32E", r.stderr
    r = subprocess.run([str(cli), "roundtrip", "-p", str(src)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b" slices 280 coded 267 skipped 13 " in r.stdout, (r.stdout, r.stderr)
    for args in (["compress", "-e"], ["compress", "-c", "-e"], ["decompress", "-p", "-e"]):
        r = subprocess.run([str(cli)] + args + [str(src), str(out)], capture_output=True, timeout=120)
        assert r.returncode == 1 and b"-e goes with" in r.stderr, (args, r.stderr)
