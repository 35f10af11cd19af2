"""Multi-GPU sharding: one process per GPU.

PARALLEL model, one file over the ranks, both directions.  Every slice is an independent unit
(fresh CABAC contexts per H.264 9.3.1, fresh re-coded coder per slice, recode.cpp:1263/1422, model
reset per slice), so a file's slices are cut into contiguous ranges balanced by bytes, one range
per rank.  The only collective is the final gather of the variable-length per-slice outputs to
rank 0 (point-to-point send/recv over xGMI with backend "nccl" = RCCL; CPU tensors with "gloo"):
  sharded_compress    re-coded blocks -> rank 0 builds the Recoded container (avr_assemble_container)
  sharded_decompress  regenerated CABAC payloads -> rank 0 splices them with the container's
                      literals and applies the last-byte patch (avr_splice_container)
Both are byte-identical to the single-GPU calls.  The whole-file compress cuts the parallel model's
long slices into pieces (Context.split_bytes); sharded_compress(split_bytes=...) does the same on
each rank for its range's long slices -- the split walk, a check of the pieces on the device and the
seams fields (batch.SplitBatch), beside the batch of the rest -- and a second gather brings the
fields to rank 0, which writes them into the container (avr_assemble_container_seams).  Its default,
split_bytes=None, codes every slice whole: the whole-file container at ctx.split_bytes = 0.

A container whose long slices were cut into pieces (Context.split_bytes; Block field 16) is
decompressed by units instead of slices: a unit is what one workgroup regenerates, a whole slice or
one piece of a split slice (DecompressPlan.load(avrc, pieces=True)).  The units are partitioned by
their re-coded bytes, so the pieces of one long slice land on several ranks; each rank regenerates
its units from their streams and seam records (decompress_units_range: avr_decompress_pieces for the
pieces, avr_decompress_slices for the rest, one avr_pack_pieces that keeps of every piece only its
share of the slice), the gather concatenates them in rank order, and rank 0 folds the units back
into slices (collapse_units) for the same splice.

CHAINED model (the reference model restarted every AVR_CHAIN_SLICES coded slices), one file over
the ranks, both directions: its chains are independent, so a file's chains are cut into contiguous
ranges balanced by bytes (the library applies partition()'s rule), each rank runs its chains on its
GPU (avr_compress_chain_range / avr_decompress_chain_range), and the same gather brings the
re-coded (regenerated) slices to rank 0, which assembles (splices) them:
  sharded_compress_chained / sharded_decompress_chained: byte-identical to ctx.compress(data,
  MODEL_CHAINED) / ctx.decompress(avrc).

A corpus of files (BASELINE configs[4]): files are dealt to ranks whole (deal_files, LPT by
bytes) and each rank runs its files through the batched corpus calls; the reference model's
unit of sequential work is a file (its estimators carry across slices, recode.cpp:662-665), so
this is also the reference model's only split -- replicas over files.
"""
from __future__ import annotations

import numpy as np

from . import (MODEL_CHAINED, MODEL_PARALLEL, MODEL_PARALLEL32, PIECE, SLICE_NO_END, DecompressPlan, ParsedStream, assemble_container,
               container_model, crc32, crc32_combine, file_crc_of_container, parse_stream, plan_decompress,
               seams_of_container, splice_container)


def partition(sizes, world: int) -> list[tuple[int, int]]:
    """Contiguous [lo, hi) slice ranges, one per rank, balanced by cumulative bytes.

    Rank r takes the slices whose byte-prefix midpoint falls in [r, r+1) * total / world, so
    every slice is owned exactly once and ranges are ordered by rank."""
    sizes = np.asarray(sizes, dtype=np.float64)
    n = len(sizes)
    if world <= 1 or n == 0:
        return [(0, n)] + [(n, n)] * max(0, world - 1)
    total = sizes.sum()
    if total <= 0:
        cuts = [round(r * n / world) for r in range(world + 1)]
    else:
        mid = np.cumsum(sizes) - sizes / 2
        owner = np.minimum((mid * world / total).astype(np.int64), world - 1)
        cuts = [int(np.searchsorted(owner, r, side="left")) for r in range(world)] + [n]
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def pinned(nbytes: int):
    """A page-locked host buffer (uint8 numpy view of a pinned torch tensor): device copies into and
    out of it run as DMA at the link's rate, and one allocation is reused from step to step (a
    fresh multi-GB numpy array costs its page faults on every step)."""
    import torch
    t = torch.empty(max(1, nbytes), dtype=torch.uint8, pin_memory=True)
    return t.numpy()


def gather_flat(flat, status, offsets, lens, dst: int = 0, device=None, out=None):
    """Gather every rank's per-slice (status, bytes) to `dst`, in rank order.

    flat: this rank's outputs packed in one uint8 tensor (device tensor with RCCL), slice k's bytes
    at flat[offsets[k] : offsets[k] + lens[k]].  Returns (status int32[n_total], blob uint8 array,
    offsets uint64, lens uint32) on dst, None elsewhere.  The blob is one host array written in
    place (out: a caller's buffer of at least the total size, ideally pinned(): reused across steps,
    copied into by DMA); a multi-GB gather is copied once, device to host.  Counts first (a
    fixed-size all_gather), then one send/recv of the per-slice metadata and one of the flat bytes
    per rank: RCCL has no gatherv, and the payload moves device to device over xGMI.
    On dst the receives are posted for all ranks at once (each peer's xGMI link carries its own)
    and each rank's bytes go to the host on a copy stream as soon as they have arrived, while the
    later ranks' are still in flight."""
    import torch
    import torch.distributed as dist

    rank, world = dist.get_rank(), dist.get_world_size()
    dev = device if device is not None else flat.device
    status = np.asarray(status, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(status)
    nbytes = int((offsets + lens).max()) if n else 0
    hdr = torch.tensor([n, nbytes], dtype=torch.int64, device=dev)
    allh = [torch.zeros_like(hdr) for _ in range(world)]
    dist.all_gather(allh, hdr)
    counts = [int(h[0]) for h in allh]
    sizes = [int(h[1]) for h in allh]
    meta = torch.from_numpy(np.concatenate([status, offsets, lens])).to(dev)
    body = flat[:nbytes].to(dev)
    if rank != dst:
        if counts[rank]:
            dist.send(meta, dst)
        if sizes[rank]:
            dist.send(body, dst)
        return None
    total = sum(sizes)
    if out is not None and out.nbytes >= total:
        blob = out[:total]
    else:
        blob = np.empty(total, dtype=np.uint8)
    # post every receive, then drain them in rank order
    bufs, works = [], []
    for r in range(world):
        if r == rank:
            bufs.append((meta, body))
            continue
        m = torch.empty(3 * counts[r], dtype=torch.int64, device=dev)
        f = torch.empty(sizes[r], dtype=torch.uint8, device=dev)
        if counts[r]:
            works.append(dist.irecv(m, r))
        if sizes[r]:
            works.append(dist.irecv(f, r))
        bufs.append((m, f))
    on_gpu = dev.type == "cuda"
    copy_stream = torch.cuda.Stream(dev) if on_gpu else None
    st, offs, ln, base, wi = [], [], [], 0, 0
    for r in range(world):
        m, f = bufs[r]
        if r != rank:
            for _ in range(int(counts[r] > 0) + int(sizes[r] > 0)):
                works[wi].wait()
                wi += 1
        c = counts[r]
        if sizes[r]:
            dst_t = torch.from_numpy(blob[base:base + sizes[r]])
            if on_gpu:
                # after the receive (waited on the current stream), on the copy stream: this rank's
                # D2H overlaps the next ranks' receives
                copy_stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(copy_stream):
                    dst_t.copy_(f, non_blocking=dst_t.is_pinned())
                    f.record_stream(copy_stream)
            else:
                dst_t.copy_(f)
        mh = m.cpu().numpy()
        st.append(mh[:c])
        offs.append(mh[c:2 * c] + base)
        ln.append(mh[2 * c:])
        base += sizes[r]
    if on_gpu:
        copy_stream.synchronize()
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    return cat(st, np.int32), blob, cat(offs, np.uint64), cat(ln, np.uint32)


def gather_blocks(local: list[bytes], status: list[int], dst: int = 0, device=None, out=None):
    """gather_flat for host byte strings (one per slice)."""
    import torch
    lens = np.array([len(b) for b in local], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else lens
    flat = torch.from_numpy(np.frombuffer(b"".join(local), dtype=np.uint8).copy())
    dev = device if device is not None else torch.device("cpu")
    return gather_flat(flat, status, offs, lens, dst=dst, device=dev, out=out)


def subset(ps: ParsedStream, lo: int, hi: int, copy_arena: bool = True) -> ParsedStream:
    """The slices [lo, hi) of a parsed stream as a self-contained batch (offsets rebased).
    copy_arena False: the arena is a view of ps.arena's range (valid while ps.arena is)."""
    d = ps.descs[lo:hi].copy()
    if len(d) == 0:
        return ParsedStream(d, np.zeros(16, np.uint8), 0, ps.max_mb_width, ps.max_mb_height)
    a0 = int(d[0]["payload_offset"])
    a1 = int(ps.descs[hi]["payload_offset"]) if hi < len(ps.descs) else len(ps.arena)
    w0 = int(d[0]["out_offset"])
    w1 = int(d[-1]["out_offset"]) + ((int(d[-1]["out_capacity"]) + 15) & ~15)
    d["payload_offset"] -= a0
    d["out_offset"] -= w0
    arena = ps.arena[a0:a1]
    return ParsedStream(d, arena.copy() if copy_arena else arena, w1 - w0, ps.max_mb_width, ps.max_mb_height)


def select(ps: ParsedStream, idx) -> ParsedStream:
    """subset() for a list of slice indices (ascending or not): those slices as a self-contained
    batch in the order given -- the payloads copied into an arena of their own (each 16-byte aligned
    and followed by at least 16 zero bytes), the outputs placed one after the other.  max_mb_width is
    the widest LDS ring among the selected coded slices (3 W + 7 for an MBAFF slice), so a selection
    of progressive slices is not widened by the MBAFF ones it leaves out."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    d = ps.descs[idx].copy()
    if len(d) == 0:
        return ParsedStream(d, np.zeros(16, np.uint8), 0, 1, ps.max_mb_height)
    span = d["read_limit"].astype(np.int64)
    room = (span + 16 + 15) & ~15
    off = np.cumsum(room) - room
    arena = np.zeros(int(room.sum()) + 16, np.uint8)
    for o, s, n in zip(off, ps.descs["payload_offset"][idx].astype(np.int64), span):
        arena[o:o + n] = ps.arena[s:s + n]
    d["payload_offset"] = off
    wroom = (d["out_capacity"].astype(np.int64) + 15) & ~15
    d["out_offset"] = np.cumsum(wroom) - wroom
    cols = np.where(d["structure"] == 3, 3 * d["mb_width"] + 7, d["mb_width"])[d["coded"] != 0]
    return ParsedStream(d, arena, int(wroom.sum()), int(cols.max()) if len(cols) else 1, ps.max_mb_height)


def subset_units(pu: ParsedStream, lo: int, hi: int, copy_arena: bool = True) -> ParsedStream:
    """The units [lo, hi) of a piece plan's batch (DecompressPlan.parsed_units) as a self-contained
    batch: subset(), plus the seam records the range's pieces start from, seam rebased to the first
    of them."""
    sub = subset(pu, lo, hi, copy_arena)
    p = pu.pieces[lo:hi].copy()
    cut = p["seam"] >= 0
    recs = np.zeros(0, np.uint8)
    if cut.any():
        r0, r1 = int(p["seam"][cut].min()), int(p["seam"][cut].max()) + 1
        p["seam"][cut] -= r0
        recs = pu.recs[r0 * pu.rec_stride:r1 * pu.rec_stride]
    sub.pieces, sub.recs, sub.rec_stride = p, recs, pu.rec_stride
    return sub


def collapse_units(pieces, status, offsets, lens):
    """Per-unit results of a piece plan (all its units, in order: pieces = DecompressPlan.pieces; unit
    k's kept bytes at offsets[k], lens[k] of the gathered blob) as DecompressPlan.splice's per-slice
    (status int32, offsets uint64, lens uint32).  A slice's status is the first non-zero status of
    its units, or SLICE_NO_END when a piece but the last did not keep exactly its share or the
    slice's units do not follow each other in the blob without a gap; its bytes start at its first
    unit's and are as long as its units' together."""
    pieces = np.asarray(pieces, dtype=PIECE)
    status = np.asarray(status, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(pieces)
    if not (len(status) == len(offsets) == len(lens) == n):
        raise ValueError("collapse_units: one status / offset / length per unit")
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    sl = pieces["slice"]
    first = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]]))
    count = np.diff(np.concatenate([first, [n]]))
    st = status[first].copy()
    off = offsets[first].copy()
    ln = np.add.reduceat(lens, first)
    for s in np.flatnonzero(count > 1):
        a, b = int(first[s]), int(first[s] + count[s])
        bad = status[a:b][status[a:b] != 0]
        if len(bad):
            st[s] = bad[0]
        elif ((lens[a:b - 1] != pieces["keep"][a:b - 1]).any()
              or (offsets[a:b - 1] + lens[a:b - 1] != offsets[a + 1:b]).any()):
            st[s] = SLICE_NO_END
    return st.astype(np.int32), off.astype(np.uint64), ln.astype(np.uint32)


def collapse_unit_crcs(pieces, crcs, lens):
    """collapse_units for the units' CRCs (batch.UnitBatch.crcs over the packed outputs, gathered in
    unit order): per slice the CRC-32 of its units' kept bytes one after the other, uint32 --
    DecompressPlan.splice's crcs.  A whole slice's is its unit's; a cut slice's is folded from its
    pieces' with crc32_combine (a CRC is linear: no byte is read again)."""
    pieces = np.asarray(pieces, dtype=PIECE)
    crcs = np.asarray(crcs).astype(np.uint32)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(pieces)
    if not (len(crcs) == len(lens) == n):
        raise ValueError("collapse_unit_crcs: one crc / length per unit")
    if n == 0:
        return np.zeros(0, np.uint32)
    sl = pieces["slice"]
    first = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]]))
    count = np.diff(np.concatenate([first, [n]]))
    out = crcs[first].copy()
    for s in np.flatnonzero(count > 1):
        c = int(out[s])
        for u in range(int(first[s]) + 1, int(first[s] + count[s])):
            c = crc32_combine(c, int(crcs[u]), int(lens[u]))
        out[s] = c
    return out


def _host_crcs(part: ParsedStream) -> np.ndarray:
    """The payload CRCs of a batch on the host (a device step that brought none)."""
    return np.array([crc32(part.arena[int(d["payload_offset"]):int(d["payload_offset"]) + int(d["payload_size"])])
                     for d in part.descs], dtype=np.uint32)


def _gather_u32(values, status, dev):
    """One uint32 per slice (unit) through gather_flat, as 4-byte items: rank 0 gets them in rank order."""
    import torch
    v = np.ascontiguousarray(values, dtype=np.uint32)
    n = len(v)
    flat = torch.from_numpy(np.concatenate([v.view(np.uint8), np.zeros(16, np.uint8)]))
    g = gather_flat(flat.to(dev) if dev.type == "cuda" else flat, np.asarray(status, np.int64)[:n] * 0,
                    4 * np.arange(n, dtype=np.int64), np.full(n, 4, np.int64), dst=0, device=dev)
    if g is None:
        return None
    _, blob, offs, _ = g
    return np.ascontiguousarray(blob[:4 * len(offs)]).view(np.uint32).copy()


def compress_range(ctx, part: ParsedStream, device=None, model: int = MODEL_PARALLEL, split_bytes: int = 0,
                   split_p32: bool = False, checksums: bool = False):
    """This rank's slice range of a sharded compress on its GPU: (flat uint8 tensor, status, offsets,
    lens, seams) with slice k's re-coded bytes at flat[offsets[k] : offsets[k] + lens[k]] and status 0
    where it is to be coded (-1: stored skip_coded).  split_bytes 0 (or a model other than
    MODEL_PARALLEL, or MODEL_PARALLEL32 with split_p32): every slice whole through batch.DeviceBatch,
    seams None.  Otherwise the range's
    split candidates (split_plan at split_bytes, coded slices only) go through batch.SplitBatch on a
    side stream beside the DeviceBatch of the rest; the two are joined before the packs; seams is one
    bytes per slice (b"" without a cut).  A candidate whose walk, cut check or verify fails is
    stored skip_coded, as the whole-file compress stores it: no unsplit retry.
    checksums: a sixth value, the CRC-32 of every slice's payload (uint32), computed over the batches'
    input arenas on the device (DeviceBatch.crcs / SplitBatch.crcs) for a checked container."""
    import torch

    from . import split_plan
    from .batch import DeviceBatch, SplitBatch

    n = len(part.descs)
    dev = torch.device("cuda", ctx.device) if device is None else device
    cand = np.zeros(n, bool)
    split_bytes = split_bytes if model == MODEL_PARALLEL or (model == MODEL_PARALLEL32 and split_p32) else 0
    if split_bytes:
        cand = split_plan(part.descs, split_bytes).candidate & (part.descs["coded"] != 0)
    if not cand.any():
        b = DeviceBatch(ctx, part, device=dev)
        b.roundtrip(model)
        flat, d_off = b.pack()
        d_crc = b.crcs("in")[0] if checksums else None
        torch.cuda.synchronize()
        v = b.verdicts()
        res = b.results("c")
        offs = d_off.cpu().numpy()[:n].astype(np.int64)
        lens = np.where(res["status"] == 0, res["out_len"], 0).astype(np.int64)
        status = np.where(v == 1, 0, -1).astype(np.int64)
        out = (flat, status, offs, lens, ([b""] * n if split_bytes else None))
        return out + (d_crc.cpu().numpy()[:n].view(np.uint32).copy(),) if checksums else out
    idx_c, idx_r = np.flatnonzero(cand), np.flatnonzero(~cand)
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    sb = SplitBatch(ctx, select(part, idx_c), split_bytes, device=dev, model=model)
    side.wait_stream(cur)                   # after the batch's uploads and zero fills on the current stream
    sb.compress(side)                       # the long walks first, beside everything below
    b = None
    if len(idx_r):
        b = DeviceBatch(ctx, select(part, idx_r), device=dev)
        b.roundtrip(model)
    with torch.cuda.stream(side):
        sb.read_back(side)
        sb.stage(side)
        sb.decompress(side)
        sb.pack(side)
        sb.verify(side)
    cur.wait_stream(side)                   # joined before the packs
    flat_c, off_c = sb.pack_recoded()
    if b is not None:
        flat_r, off_r = b.pack()
    crcs = np.zeros(n, np.uint32)
    if checksums:
        crc_c = sb.crcs()[0]
        crc_r = b.crcs("in")[0] if b is not None else None
    torch.cuda.synchronize()
    if checksums:
        crcs[idx_c] = crc_c.cpu().numpy()[:len(idx_c)].view(np.uint32)
        if b is not None:
            crcs[idx_r] = crc_r.cpu().numpy()[:len(idx_r)].view(np.uint32)
    status = np.full(n, -1, np.int64)
    offs, lens = np.zeros(n, np.int64), np.zeros(n, np.int64)
    seams = [b""] * n
    st_c, fields = sb.seams(check_cuts=True)
    ok = (sb.verdicts() == 1) & (st_c == 0)
    total_c = int(off_c.cpu().numpy()[len(idx_c)])
    status[idx_c] = np.where(ok, 0, -1)
    offs[idx_c] = off_c.cpu().numpy()[:len(idx_c)]
    lens[idx_c] = np.where(ok, sb.res["out_len"], 0)
    for j, k in enumerate(idx_c):
        if ok[j]:
            seams[k] = fields[j]
    flat = flat_c[:max(16, total_c)]
    if b is not None:
        res = b.results("c")
        status[idx_r] = np.where(b.verdicts() == 1, 0, -1)
        offs[idx_r] = off_r.cpu().numpy()[:len(idx_r)] + total_c
        lens[idx_r] = np.where(res["status"] == 0, res["out_len"], 0)
        total_r = int(off_r.cpu().numpy()[len(idx_r)])
        flat = torch.cat([flat_c[:total_c], flat_r[:max(16, total_r)]])
    return (flat, status, offs, lens, seams, crcs) if checksums else (flat, status, offs, lens, seams)


def sharded_compress(ctx, data: bytes, device=None, ps: ParsedStream | None = None,
                     model: int = MODEL_PARALLEL, split_bytes: int | None = None, run_range=None,
                     escaped: bool = False, split_p32: bool = False, checksums: bool = False,
                     unit_checksums: bool = False) -> bytes | None:
    """PARALLEL-model compress of one file across all ranks; the container is returned on rank 0.

    Every rank parses the file (host), takes its contiguous slice range (partition), runs it on its
    GPU (compress_range: compress + device roundtrip check -- a slice is coded only if it regenerates
    its payload -- and the re-coded bytes packed on the device) and sends them to rank 0 (gather_flat
    over RCCL), which assembles the Recoded container from its own parse
    (avr_assemble_container_parsed).  model = MODEL_PARALLEL or MODEL_PARALLEL32.
    split_bytes None or 0 (the default): every slice is coded whole -- byte-identical to
    ctx.compress(data, model) at ctx.split_bytes = 0, or where no slice is a split candidate.
    split_bytes = s with MODEL_PARALLEL, or with MODEL_PARALLEL32 and split_p32 (pass ctx.split_p32;
    without it MODEL_PARALLEL32 ignores split_bytes, as the whole-file call does by default):
    each rank takes its range's split candidates (a progressive slice of at least 1.5 s payload
    bytes) through the split walk, checks them piece by piece on the device and builds their seams
    fields (batch.SplitBatch); a second gather_flat brings the fields to rank 0, which assembles with
    them (avr_assemble_container_seams_parsed; for MODEL_PARALLEL32 avr_assemble_container_opts with
    ASSEMBLE_SPLIT32, which writes the P32S / P32SE tag).  Byte-identical to ctx.compress(data, model)
    at ctx.split_bytes = s (and ctx.split_p32 on for MODEL_PARALLEL32); sharded_compress(ctx, x, split_bytes=ctx.split_bytes) is the whole-file
    container.  A slice is one rank's: the cut pieces help the decompress, a single slice's compress
    walk stays one chain.
    escaped (pass ctx.recode_escaped): rank 0 assembles with the second search of
    Context.recode_escaped (avr_assemble_container_opts, ASSEMBLE_ESCAPED) -- the ranks' work does not
    change, since every candidate slice is compressed and checked anyway -- and the container is
    byte-identical to ctx.compress(data, model) with that option on.
    checksums (pass ctx.checksums): a checked container.  Each rank computes its slices' payload
    CRCs on its device, over the arenas its batches uploaded (compress_range's sixth value), and one
    more gather_flat of 4-byte items brings them to rank 0, whose assembly folds them with the
    literals' into the file's CRC (avr_assemble_container_args, ASSEMBLE_CRC): byte-identical to
    ctx.compress(data, model) with ctx.checksums on.  A device step that returns no sixth value has
    them computed from the payloads on the host.
    unit_checksums (pass ctx.unit_checksums): rank 0 assembles with ASSEMBLE_UNIT_CRC -- Block field 18
    on every coded block, the unit values computed there on host threads from the payloads and the
    seams' cuts (the ranks' work does not change; values brought from their devices are not taken
    yet) -- byte-identical to ctx.compress(data, model) with ctx.unit_checksums on.
    run_range(part) -> compress_range's tuple replaces the device step (CPU tests)."""
    import torch
    import torch.distributed as dist

    rank, world = dist.get_rank(), dist.get_world_size()
    ps = ps if ps is not None else parse_stream(data)
    split32 = model == MODEL_PARALLEL32 and bool(split_p32)
    split = int(split_bytes or 0) if model == MODEL_PARALLEL or split32 else 0
    lo, hi = partition(ps.descs["payload_size"], world)[rank]
    part = subset(ps, lo, hi)
    dev = _gather_device(ctx, device)
    seams = crcs = None
    if hi > lo:
        out = (run_range or (lambda p: compress_range(ctx, p, None, model, split, split_p32=split32,
                                                      checksums=checksums)))(part)
        flat, status, offs, lens, seams = out[:5]
        crcs = out[5] if len(out) > 5 else None
    else:
        flat = torch.zeros(16, dtype=torch.uint8, device=dev)
        offs = lens = status = np.zeros(0, np.int64)
    g = gather_flat(flat, status, offs, lens, dst=0, device=dev)
    gs = None
    if split:
        # the seams fields, by the same gather: one (possibly empty) field per slice
        fields = seams if seams is not None else [b""] * (hi - lo)
        sl = np.array([len(f) for f in fields], dtype=np.int64)
        so = np.cumsum(sl) - sl
        sflat = torch.from_numpy(np.frombuffer(b"".join(fields) + b"\0" * 16, dtype=np.uint8).copy())
        gs = gather_flat(sflat.to(dev) if dev.type == "cuda" else sflat, np.asarray(status, np.int64), so, sl, dst=0,
                         device=dev)
    gc = None
    if checksums:
        gc = _gather_u32(crcs if crcs is not None else _host_crcs(part), status, dev)
    if g is None:
        return None
    st, blob, offs, lens = g
    if gs is not None:
        _, sblob, soffs, slens = gs
        return assemble_container(data, st, blob, offs, lens, model=model, ps=ps, seams=(sblob, soffs, slens),
                                  escaped=escaped, split32=split32, checksums=checksums, crcs=gc,
                                  unit_checksums=unit_checksums)
    return assemble_container(data, st, blob, offs, lens, model=model, ps=ps, escaped=escaped, checksums=checksums,
                              crcs=gc, unit_checksums=unit_checksums)


def _gather_device(ctx, device):
    import torch
    import torch.distributed as dist
    # RCCL ("nccl") moves device tensors only; gloo moves host tensors
    if dist.get_backend() == "nccl":
        return device if device is not None else torch.device("cuda", ctx.device)
    return torch.device("cpu")


def decompress_range(ctx, part: ParsedStream, device=None, model: int = MODEL_PARALLEL, crcs: bool = False):
    """This rank's slice range of a sharded decompress on its GPU: (flat uint8 tensor, status,
    offsets, lens) with slice k's regenerated bytes at flat[offsets[k] : offsets[k] + lens[k]]
    (packed on the device, avr_pack_outputs).  model: the container's (container_model).
    crcs (a checked container): a fifth value, the CRC-32 of each slice's packed bytes (uint32),
    computed on the device (DeviceBatch.crcs over the packed outputs)."""
    import torch

    from .batch import DeviceBatch

    b = DeviceBatch(ctx, part, device=device)
    b.decompress(model)
    flat, d_off = b.pack(which="d")
    d_crc = b.crcs("packed")[0] if crcs else None
    torch.cuda.synchronize()
    res = b.results("d")
    n = len(part.descs)
    offs = d_off.cpu().numpy()[:n].astype(np.int64)
    status = res["status"].astype(np.int64)
    lens = np.where(status == 0, res["out_len"], 0).astype(np.int64)
    out = (flat, status, offs, lens)
    return out + (d_crc.cpu().numpy()[:n].view(np.uint32).copy(),) if crcs else out


def decompress_units_range(ctx, part: ParsedStream, device=None, model: int = MODEL_PARALLEL, crcs: bool = False):
    """This rank's unit range of a sharded decompress of a split container on its GPU
    (batch.UnitBatch): (flat uint8 tensor, status, offsets, lens) per unit, unit k's kept bytes at
    flat[offsets[k] : offsets[k] + lens[k]].  The pieces go through avr_decompress_pieces_m on the
    container's coder (model: MODEL_PARALLEL, or MODEL_PARALLEL32 for a P32S container), the whole
    slices through avr_decompress_slices, one launch after the other on the current stream, and one
    avr_pack_pieces packs all units in unit order, each piece cut down to its share of its slice.
    crcs (a checked container): a fifth value, the CRC-32 of each unit's kept bytes (UnitBatch.crcs)."""
    import torch

    from .batch import UnitBatch

    b = UnitBatch(ctx, part, device=device)
    b.decompress(model)
    flat, d_off, d_kept, d_status = b.pack()
    d_crc = b.crcs(flat, d_off, d_kept)[0] if crcs else None
    torch.cuda.synchronize()
    n = len(part.descs)
    offs = d_off.cpu().numpy()[:n].astype(np.int64)
    lens = d_kept.cpu().numpy()[:n].view(np.uint32).astype(np.int64)
    out = (flat, d_status.cpu().numpy()[:n].astype(np.int64), offs, lens)
    return out + (d_crc.cpu().numpy()[:n].view(np.uint32).copy(),) if crcs else out


def _sharded_decompress_units(ctx, avrc, device, run_range):
    """sharded_decompress of a container with seams: units instead of slices."""
    import torch
    import torch.distributed as dist

    rank, world = dist.get_rank(), dist.get_world_size()
    plan = DecompressPlan().load(avrc, pieces=True)
    pu = plan.parsed_units()
    model = container_model(avrc)
    lo, hi = partition(pu.descs["payload_size"], world)[rank]
    part = subset_units(pu, lo, hi)
    dev = _gather_device(ctx, device)
    checked = file_crc_of_container(avrc) is not None
    crcs = None
    if hi > lo:
        out = (run_range or (lambda p: decompress_units_range(ctx, p, device, model, crcs=checked)))(part)
        flat, status, offs, lens = out[:4]
        crcs = out[4] if len(out) > 4 else None
    else:
        flat = torch.zeros(16, dtype=torch.uint8, device=dev)
        offs = lens = status = np.zeros(0, np.int64)
    g = gather_flat(flat, status, offs, lens, dst=0, device=dev)
    gc = _gather_regen_crcs(checked, crcs, flat, status, offs, lens, dev)
    if g is None:
        return None
    st, blob, offs, lens = g
    if gc is not None:
        gc = collapse_unit_crcs(plan.pieces, gc, lens)
    st, offs, lens = collapse_units(plan.pieces, st, offs, lens)
    return plan.splice(st, blob, offs, lens, crcs=gc).tobytes()


def _gather_regen_crcs(checked, crcs, flat, status, offs, lens, dev):
    """A checked container's per-slice (per-unit) CRCs gathered to rank 0, one more gather_flat of
    4-byte items; None for a container without the field.  A device step that brought no values has
    them computed from its packed bytes on the host."""
    if not checked:
        return None
    if crcs is None:
        h = flat.cpu().numpy()
        crcs = np.array([crc32(h[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)], dtype=np.uint32)
    return _gather_u32(crcs, status, dev)


def sharded_decompress(ctx, avrc: bytes, device=None, run_range=None) -> bytes | None:
    """PARALLEL-model decompress of one container across all ranks; the file is returned on rank 0.

    Every rank plans the container (host: avr_plan_decompress), takes its contiguous range of
    coded slices balanced by re-coded bytes (partition), regenerates them on its GPU
    (decompress_range: avr_decompress_slices + avr_pack_outputs), and sends the packed payloads to
    rank 0 (gather_flat over RCCL), which splices them with the literals and applies the last-byte
    patch (avr_splice_container, recode.cpp:1338-1357).  Byte-identical to ctx.decompress(avrc).
    run_range(part) -> (flat, status, offsets, lens) replaces the device step (CPU tests).
    A container whose long slices were cut (Block field 16) goes by units instead: planned with
    pieces, partitioned by the units' re-coded bytes, each rank's units through
    decompress_units_range (run_range then gets the unit batch of subset_units and returns per-unit
    outputs), and on rank 0 collapse_units before DecompressPlan.splice.
    A block that stands for escaped bytes (Block field 17, Context.recode_escaped) changes neither
    route: descriptors and units are in the unescaped domain, and rank 0's splice escapes.
    A checked container (Context.checksums, Metadata field 16) is checked on rank 0 (AvrError
    ERR_CHECKSUM): each rank computes the CRC-32 of its slices' (units') regenerated bytes on its
    device, over the packed outputs, one more gather_flat brings the values, and rank 0 folds them
    (collapse_unit_crcs for the pieces of a cut slice, then the splice's fold with the literals)."""
    import torch
    import torch.distributed as dist

    if seams_of_container(avrc):
        return _sharded_decompress_units(ctx, avrc, device, run_range)
    rank, world = dist.get_rank(), dist.get_world_size()
    plan = plan_decompress(avrc)
    model = container_model(avrc)
    lo, hi = partition(plan.descs["payload_size"], world)[rank]
    part = subset(plan, lo, hi)
    dev = _gather_device(ctx, device)
    checked = file_crc_of_container(avrc) is not None
    crcs = None
    if hi > lo:
        out = (run_range or (lambda p: decompress_range(ctx, p, device, model, crcs=checked)))(part)
        flat, status, offs, lens = out[:4]
        crcs = out[4] if len(out) > 4 else None
    else:
        flat = torch.zeros(16, dtype=torch.uint8, device=dev)
        offs = lens = status = np.zeros(0, np.int64)
    g = gather_flat(flat, status, offs, lens, dst=0, device=dev)
    gc = _gather_regen_crcs(checked, crcs, flat, status, offs, lens, dev)
    if g is None:
        return None
    st, blob, offs, lens = g
    if gc is not None:   # the device's values: the splice reads no slice's bytes for the check
        return DecompressPlan().load(avrc).splice(st, blob, offs, lens, crcs=gc).tobytes()
    return splice_container(avrc, st, blob, offs, lens)


def _host_to_gather(blob, dev):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(blob) if len(blob) else np.zeros(16, np.uint8))
    return t.to(dev) if dev.type == "cuda" else t


def sharded_compress_chained(ctx, data, device=None, run_range=None) -> bytes | None:
    """CHAINED-model compress of one file across all ranks; the container is returned on rank 0.

    Every rank runs its contiguous range of the file's chains on its GPU
    (Context.compress_chain_range: parse and segmentation of the whole file, the reference-model
    pass over its chains), the re-coded slices go to rank 0 (gather_flat over RCCL), which assembles
    the Recoded container (avr_assemble_container, model CHAINED).  Byte-identical to
    ctx.compress(data, MODEL_CHAINED).  A coded slice that failed on its rank (status -2: the
    whole-file call would demote it and re-segment, moving every later chain) makes rank 0 compress
    the file whole.  run_range() -> compress_chain_range's tuple replaces the device step (tests)."""
    import torch.distributed as dist

    rank, world = dist.get_rank(), dist.get_world_size()
    dev = _gather_device(ctx, device)
    lo, hi, st, blob, offs, lens = (run_range or (lambda: ctx.compress_chain_range(data, world, rank)))()
    g = gather_flat(_host_to_gather(blob, dev), st.astype(np.int64), offs.astype(np.int64), lens.astype(np.int64),
                    dst=0, device=dev)
    if g is None:
        return None
    st, blob, offs, lens = g
    if (st < -1).any():
        return ctx.compress(data, MODEL_CHAINED)
    return assemble_container(data, st, blob, offs, lens, model=MODEL_CHAINED)


def sharded_decompress_chained(ctx, avrc, device=None, run_range=None) -> bytes | None:
    """CHAINED-model decompress of one container across all ranks; the file is returned on rank 0.

    Every rank plans the container and regenerates its contiguous range of chains on its GPU
    (Context.decompress_chain_range); the regenerated slices go to rank 0 (gather_flat), which
    splices them with the literals and the last-byte patch on its plan of the same container
    (DecompressPlan.splice, recode.cpp:1338-1357).  Byte-identical to ctx.decompress(avrc).
    A reference-model container is one unit: rank 0 decodes it whole."""
    import torch.distributed as dist

    rank, world = dist.get_rank(), dist.get_world_size()
    dev = _gather_device(ctx, device)
    lo, hi, st, regen, offs, lens = (run_range or (lambda: ctx.decompress_chain_range(avrc, world, rank)))()
    g = gather_flat(_host_to_gather(regen, dev), st.astype(np.int64), offs.astype(np.int64), lens.astype(np.int64),
                    dst=0, device=dev)
    if g is None:
        return None
    st, blob, offs, lens = g
    out = DecompressPlan().load(avrc).splice(st, blob, offs, lens)
    return out.tobytes()


def scatter_parsed(ps: "ParsedStream | None", ranges, device, src: int = 0):
    """Rank src's decompress batch (ps, e.g. DecompressPlan.parsed of the container it assembled) cut
    into the contiguous slice ranges `ranges` (one [lo, hi) per rank): each rank receives its own as
    (descs, arena, n, work_len, max_mb_width, max_mb_height) -- host arrays on src, the arena as a
    device tensor elsewhere (point-to-point over RCCL / xGMI: one header, the descriptors and the
    re-coded streams per rank; gloo moves host tensors).  Offsets are rebased as in subset()."""
    import torch
    import torch.distributed as dist

    from . import SLICE_DESC

    rank, world = dist.get_rank(), dist.get_world_size()
    if rank == src:
        mine = None
        pending = []   # every rank's messages in flight at once (each peer has its own xGMI link)
        for r in range(world):
            lo, hi = ranges[r]
            sub = ps if (lo, hi) == (0, len(ps.descs)) else subset(ps, lo, hi, copy_arena=r == rank)
            if r == rank:
                mine = sub
                continue
            hdr = torch.tensor([hi - lo, sub.arena.nbytes, sub.work_len, sub.max_mb_width, sub.max_mb_height],
                               dtype=torch.int64, device=device)
            msgs = [hdr]
            if hi > lo:
                # the arena range is a view of rank src's (pinned) arena: one DMA to the device
                msgs.append(torch.from_numpy(np.ascontiguousarray(sub.descs).view(np.uint8).reshape(-1)).to(device))
                msgs.append(torch.from_numpy(sub.arena).to(device, non_blocking=True))
            for t in msgs:
                pending.append((dist.isend(t, r), t))
        for w, _ in pending:
            w.wait()
        return (mine.descs, mine.arena, len(mine.descs), mine.work_len, mine.max_mb_width, mine.max_mb_height)
    hdr = torch.zeros(5, dtype=torch.int64, device=device)
    dist.recv(hdr, src)
    n, alen, wlen, mw, mh = (int(x) for x in hdr.cpu())
    descs = np.zeros(0, dtype=SLICE_DESC)
    arena = torch.zeros(16, dtype=torch.uint8, device=device)
    if n:
        d = torch.empty(n * SLICE_DESC.itemsize, dtype=torch.uint8, device=device)
        dist.recv(d, src)
        descs = d.cpu().numpy().view(SLICE_DESC)
        arena = torch.empty(alen, dtype=torch.uint8, device=device)
        dist.recv(arena, src)
    return descs, arena, n, wlen, mw, mh


def deal_files(sizes, world: int) -> list[list[int]]:
    """Files to ranks, whole: longest-processing-time-first by bytes (the largest file goes to the
    least-loaded rank).  Returns each rank's file indices in ascending order."""
    sizes = [int(x) for x in sizes]
    load = [0] * max(1, world)
    owned = [[] for _ in range(max(1, world))]
    for f in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)):
        r = min(range(len(load)), key=lambda q: (load[q], q))
        load[r] += sizes[f]
        owned[r].append(f)
    return [sorted(o) for o in owned]


def corpus_roundtrip(ctx, files: list[bytes], model: int, dst: int = 0):
    """A corpus over the ranks (BASELINE configs[4]): this rank's files (deal_files) compressed
    and decompressed as one batch each (avr_compress_files / avr_decompress_files) and checked
    byte for byte.  Returns (files done here, bytes in, container bytes, all files bit-exact here);
    the callers reduce these over ranks."""
    rank, world = _rank_world()
    mine = deal_files([len(f) for f in files], world)[rank]
    if not mine:
        return 0, 0, 0, True
    sub = [files[i] for i in mine]
    comp = ctx.compress_files(sub, model)
    ok = not any(isinstance(c, Exception) for c in comp)
    dec = ctx.decompress_files([c for c in comp if not isinstance(c, Exception)]) if ok else []
    ok = ok and all(not isinstance(d, Exception) and d == f for d, f in zip(dec, sub))
    return len(sub), sum(map(len, sub)), sum(len(c) for c in comp if not isinstance(c, Exception)), ok


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1
