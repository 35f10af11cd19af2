"""The P32 coder's split containers on the host (tags avrecode-amd:P32S / P32SE; AVR_ASSEMBLE_SPLIT32):
CPU only.  The plan layer never decodes a stream, so the container is the oracle's P64 split
container of realshort.mp4 at split 1024 with only its Metadata.version rewritten.

* tagged P32S, avr_dec_plan_load_pieces lists the same units, descriptors, arena and records as
  under P64, container_model says MODEL_PARALLEL32, and the per-slice plans answer AVR_ERR_UNSUPPORTED;
* tagged P32 or P32E, the seams are refused with AVR_ERR_FORMAT, as before the S tags;
* an S tag without any field 16 is accepted;
* assemble_container(model=P32, seams=..., split32=True) writes the S tag (SE with escaped) and the
  library's codec parses and re-serialises it byte for byte; without split32 it raises as before."""
import ctypes

import numpy as np
import pytest

import avrecode_amd as avr
from test_piece_plan_host import _container
from test_split_compress_host import _batch, _outputs

P64_TAG = b"avrecode-amd:P64"


def _retag(avrc: bytes, tag: bytes) -> bytes:
    """The container with another Metadata.version: Recoded field 1 (Metadata) holding field 1 (version),
    the first bytes of every avrecode-amd container."""
    assert avrc[0] == 0x0A and avrc[2] == 0x0A and avrc[1] == avrc[3] + 2 and avrc[4:4 + avrc[3]] == P64_TAG
    return bytes([0x0A, len(tag) + 2, 0x0A, len(tag)]) + tag + avrc[4 + avrc[3]:]


def _plan_load(avrc):
    """avr_plan_decompress's return code alone."""
    L = avr.lib()
    descs, arena = ctypes.c_void_p(), ctypes.c_void_p()
    ns, mw, mh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    al, wl = ctypes.c_size_t(), ctypes.c_size_t()
    r = L.avr_plan_decompress(avrc, len(avrc), ctypes.byref(descs), ctypes.byref(ns), ctypes.byref(arena),
                              ctypes.byref(al), ctypes.byref(wl), ctypes.byref(mw), ctypes.byref(mh))
    assert r != 0
    return r


def test_retagged_p32s_plans_like_p64():
    p64 = _container("realshort.mp4", 1024)
    s = _retag(p64, b"avrecode-amd:P32S")
    assert _retag(p64, P64_TAG) == p64 and len(s) == len(p64) + 1
    assert avr.container_model(s) == avr.MODEL_PARALLEL32 and avr.container_model(p64) == avr.MODEL_PARALLEL
    a = avr.DecompressPlan().load(p64, pieces=True)
    b = avr.DecompressPlan().load(s, pieces=True)
    assert a.n_units == b.n_units > a.n_slices == b.n_slices
    assert a.descs.tobytes() == b.descs.tobytes() and a.units.tobytes() == b.units.tobytes()
    assert a.pieces.tobytes() == b.pieces.tobytes() and (b.pieces["seam"] >= 0).any()
    assert a.rec_stride == b.rec_stride and bytes(a.recs) == bytes(b.recs) and len(b.recs) > 0
    assert (a.arena_len, a.work_len, a.max_mb_width, a.max_mb_height) == \
        (b.arena_len, b.work_len, b.max_mb_width, b.max_mb_height)
    assert a.parsed_units().arena.tobytes() == b.parsed_units().arena.tobytes()
    # the per-slice plans keep refusing split blocks
    with pytest.raises(avr.AvrError) as e:
        avr.DecompressPlan().load(s)
    assert e.value.code == -6
    assert _plan_load(s) == -6


@pytest.mark.parametrize("tag", [b"avrecode-amd:P32", b"avrecode-amd:P32E"])
def test_seams_under_the_plain_p32_tags_stay_a_format_error(tag):
    bad = _retag(_container("realshort.mp4", 1024), tag)
    assert avr.container_model(bad) == avr.MODEL_PARALLEL32
    with pytest.raises(avr.AvrError) as e:
        avr.DecompressPlan().load(bad, pieces=True)
    assert e.value.code == -3


@pytest.mark.parametrize("tag", [b"avrecode-amd:P32S", b"avrecode-amd:P32SE"])
def test_an_s_tag_without_seams_is_accepted(tag):
    plain = _container("realshort.mp4", 0)
    s = _retag(plain, tag)
    a, b = avr.DecompressPlan().load(plain), avr.DecompressPlan().load(s)
    assert a.descs.tobytes() == b.descs.tobytes() and b.n_slices > 0
    assert avr.DecompressPlan().load(s, pieces=True).n_units == b.n_slices
    assert avr.container_model(s) == avr.MODEL_PARALLEL32


def test_unknown_tags_are_still_refused():
    for tag in (b"avrecode-amd:P64S", b"avrecode-amd:P32ES", b"avrecode-amd:P32SS"):
        with pytest.raises(avr.AvrError) as e:
            avr.container_model(_retag(_container("realshort.mp4", 1024), tag))
        assert e.value.code == -3


def test_assembly_writes_the_s_tags_only_when_asked():
    b = _batch("realshort.mp4", 1024)
    st, blob, offs, lens = _outputs(b)
    P32 = avr.MODEL_PARALLEL32
    for kw in (dict(), dict(ps=b["ps"])):
        got = avr.assemble_container(b["data"], st, blob, offs, lens, model=P32, seams=b["fields"], split32=True, **kw)
        # the P64 container's blocks under the new tag
        assert got == _retag(b["avrc"], b"avrecode-amd:P32S")
        info, again = avr.describe_container(got)
        assert again == got and bytes.fromhex(info["version"]) == b"avrecode-amd:P32S"
        assert sum("seams" in x for x in info["blocks"]) == sum(bool(f) for f in b["fields"]) > 0
        # no field 16, no S: the plain tag and the plain bytes, flag or not
        none = [b""] * len(st)
        plain = avr.assemble_container(b["data"], st, blob, offs, lens, model=P32, **kw)
        assert avr.assemble_container(b["data"], st, blob, offs, lens, model=P32, seams=none, split32=True, **kw) == plain
        assert avr.assemble_container(b["data"], st, blob, offs, lens, model=P32, split32=True, **kw) == plain
        assert bytes.fromhex(avr.describe_container(plain)[0]["version"]) == b"avrecode-amd:P32"
        # without the flag seams are refused for the model, as before; the flag is P32's alone
        with pytest.raises(avr.AvrError) as e:
            avr.assemble_container(b["data"], st, blob, offs, lens, model=P32, seams=b["fields"], **kw)
        assert e.value.code == -1
        for model in (avr.MODEL_PARALLEL, avr.MODEL_CHAINED):
            with pytest.raises(avr.AvrError) as e:
                avr.assemble_container(b["data"], st, blob, offs, lens, model=model, seams=b["fields"], split32=True,
                                       **kw)
            assert e.value.code == -1
    # P64's tags do not change
    assert avr.assemble_container(b["data"], st, blob, offs, lens, seams=b["fields"]) == b["avrc"]


def test_assembly_with_seams_and_escapes_writes_se():
    """cockatoo.mp4 has slices that only the escaped search finds; with seams on other blocks of the same
    container the tag is P32SE, and the container plans (the plan layer decodes no stream)."""
    b = _batch("cockatoo.mp4", 2048)
    st, blob, offs, lens = _outputs(b)
    # every candidate slice offered as coded: the escaped search finds the ones stored skip_coded
    ps = b["ps"]
    st = np.where(ps.descs["coded"] != 0, 0, -1).astype(np.int64)
    cab = [c if c else b"\0" * 8 for c in b["cabac"]]
    lens = np.array([len(c) for c in cab], np.int64)
    offs = np.cumsum(lens) - lens
    blob = np.frombuffer(b"".join(cab) + b"\0" * 16, np.uint8)
    got = avr.assemble_container(b["data"], st, blob, offs, lens, model=avr.MODEL_PARALLEL32, seams=b["fields"],
                                 split32=True, escaped=True)
    info, again = avr.describe_container(got)
    assert again == got and bytes.fromhex(info["version"]) == b"avrecode-amd:P32SE"
    assert any("escapes" in x for x in info["blocks"]) and any("seams" in x for x in info["blocks"])
    assert avr.container_model(got) == avr.MODEL_PARALLEL32
    plan = avr.DecompressPlan().load(got, pieces=True)
    assert plan.n_units > plan.n_slices
