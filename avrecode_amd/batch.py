"""Device-resident slice batches: HBM layout + one call per roundtrip (avr_roundtrip_slices).

HBM layout of a batch (DESIGN.md "Data layout"):
  d_in      payload arena: slice k's unescaped CABAC payload at desc[k].payload_offset (16-B aligned,
            >= 16 zero bytes after it) -- exactly what init_decoder receives (recode.cpp:143)
  d_work    re-coded output: slice k at desc[k].out_offset, desc[k].out_capacity bytes reserved
  d_regen   regenerated CABAC bytes, laid out like d_in
  d_desc / d_dec_desc   avr_slice_desc[n] (96 B each) for compress / derived decompress
  d_res_c / d_res_d     avr_slice_result[n] (40 B each); d_verdict int32[n]
torch only allocates and owns these buffers and supplies the stream; all compute is in
libavrecode.so.
"""
from __future__ import annotations

import numpy as np
import torch

from . import KEEP_ALL, PIECE, SLICE_DESC, SLICE_RESULT, MODEL_PARALLEL, MODEL_PARALLEL32, Context, ParsedStream


def _dev_bytes(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)


def _payload_spans(descs, device):
    """(d_off int64[n], d_len int32[n]) of a batch's payloads in its input arena."""
    off = torch.from_numpy(descs["payload_offset"].astype(np.int64)).to(device)
    ln = torch.from_numpy(descs["payload_size"].astype(np.uint32).view(np.int32).copy()).to(device)
    return off, ln


def _packed_spans(d_offsets, n: int, d_kept=None):
    """(d_off, d_len) of n packed outputs: where a pack left them, as long as it made them."""
    off = d_offsets[:n].contiguous()
    ln = d_kept[:n].contiguous() if d_kept is not None else (d_offsets[1:n + 1] - d_offsets[:n]).to(torch.int32)
    return off, ln


def _crc_spans(b, d_off, d_len, d_buf, stream=None):
    n = int(d_off.numel())
    d_crc = torch.zeros(max(1, n), dtype=torch.int32, device=b.device)
    d_status = torch.zeros(max(1, n), dtype=torch.int32, device=b.device)
    with torch.cuda.stream(stream) if stream is not None else _null():
        b.ctx.crc_spans(d_buf, d_buf.numel(), d_off, d_len, n, d_crc, d_status, stream)
    return d_crc, d_status


class DeviceBatch:
    def __init__(self, ctx: Context, ps: ParsedStream, device=None):
        self.ctx = ctx
        self.ps = ps
        self.device = torch.device("cuda", ctx.device) if device is None else device
        self.n = len(ps.descs)
        n = max(1, self.n)
        self.d_desc = _dev_bytes(ps.descs, self.device)
        self.d_in = _dev_bytes(ps.arena, self.device)
        self.d_work = torch.zeros(max(16, ps.work_len + 16), dtype=torch.uint8, device=self.device)
        self.d_regen = torch.zeros_like(self.d_in)
        self.d_dec_desc = torch.zeros(n * SLICE_DESC.itemsize, dtype=torch.uint8, device=self.device)
        self.d_res_c = torch.zeros(n * SLICE_RESULT.itemsize, dtype=torch.uint8, device=self.device)
        self.d_res_d = torch.zeros_like(self.d_res_c)
        self.d_verdict = torch.zeros(n, dtype=torch.int32, device=self.device)

    def roundtrip(self, model: int = MODEL_PARALLEL, stream=None):
        self.ctx.roundtrip_slices(self.d_desc, self.n, self.ps.max_mb_width, self.ps.max_mb_height, self.d_in,
                                  self.d_work, self.d_regen, self.d_dec_desc, self.d_res_c, self.d_res_d,
                                  self.d_verdict, model, stream)

    def roundtrip_timed(self, ev, model: int = MODEL_PARALLEL, stream=None):
        """roundtrip() as its four launches; ev = 4 events recorded on `stream`:
        ev[0] compress ev[1] derive ev[2] decompress ev[3] verify."""
        c, n, w, h = self.ctx, self.n, self.ps.max_mb_width, self.ps.max_mb_height
        ev[0].record(stream)
        c.compress_slices(self.d_desc, n, w, h, self.d_in, self.d_work, self.d_res_c, model, stream)
        ev[1].record(stream)
        c.derive_decompress_descs(self.d_desc, self.d_res_c, n, self.d_dec_desc, stream)
        ev[2].record(stream)
        c.decompress_slices(self.d_dec_desc, n, w, h, self.d_work, self.d_regen, self.d_res_d, model, stream)
        ev[3].record(stream)
        c.verify_slices(self.d_desc, self.d_res_c, self.d_res_d, n, self.d_in, self.d_regen, self.d_verdict, stream)

    def compress(self, model: int = MODEL_PARALLEL, stream=None):
        self.ctx.compress_slices(self.d_desc, self.n, self.ps.max_mb_width, self.ps.max_mb_height, self.d_in,
                                 self.d_work, self.d_res_c, model, stream)

    def decompress(self, model: int = MODEL_PARALLEL, stream=None):
        """A decompress batch (ps from plan_decompress: payloads = re-coded streams): d_in -> d_work,
        results in d_res_d (avr_decompress_slices)."""
        self.ctx.decompress_slices(self.d_desc, self.n, self.ps.max_mb_width, self.ps.max_mb_height, self.d_in,
                                   self.d_work, self.d_res_d, model, stream)

    def pack(self, stream=None, which: str = "c"):
        """d_work's per-slice outputs packed contiguously on the device (avr_pack_outputs) by the
        compress ("c") or decompress ("d") results: (d_packed uint8, d_offsets uint64[n + 1]); slice
        k's bytes (status 0) start at offsets[k]."""
        if not hasattr(self, "d_packed"):
            self.d_packed = torch.zeros(max(16, self.ps.work_len + 16), dtype=torch.uint8, device=self.device)
            self.d_offsets = torch.zeros(max(1, self.n) + 1, dtype=torch.int64, device=self.device)
        res = self.d_res_c if which == "c" else self.d_res_d
        self.ctx.pack_outputs(self.d_desc, res, self.n, self.d_work, self.d_packed, self.d_offsets, stream)
        return self.d_packed, self.d_offsets

    def crcs(self, which: str = "in", stream=None):
        """The CRC-32 of every slice's bytes where they lie on the device (avr_crc_spans), for a checked
        container: "in" = the payloads in the input arena (a compress batch: what the file's CRC is
        folded from), "packed" = the outputs pack() left in d_packed (a decompress batch: the
        regenerated slices).  (d_crc int32[n] holding uint32, d_status int32[n]); nothing is synchronised."""
        return _crc_spans(self, *(_payload_spans(self.ps.descs, self.device) if which == "in" else
                                  _packed_spans(self.d_offsets, self.n)),
                          self.d_in if which == "in" else self.d_packed, stream)

    # ----------------------------------------------------------------- results (host copies)
    def results(self, which: str = "c") -> np.ndarray:
        t = self.d_res_c if which == "c" else self.d_res_d
        return t.cpu().numpy().view(SLICE_RESULT)[: self.n]

    def verdicts(self) -> np.ndarray:
        return self.d_verdict.cpu().numpy()[: self.n]

    def recoded(self) -> list[bytes]:
        """Per-slice re-coded bytes (b'' where compress failed)."""
        res = self.results("c")
        work = self.d_work.cpu().numpy()
        out = []
        for k, d in enumerate(self.ps.descs):
            o, ln = int(d["out_offset"]), int(res[k]["out_len"])
            out.append(work[o:o + ln].tobytes() if res[k]["status"] == 0 and d["coded"] else b"")
        return out

    def regenerated(self) -> list[bytes]:
        res = self.results("d")
        regen = self.d_regen.cpu().numpy()
        out = []
        for k, d in enumerate(self.ps.descs):
            o, ln = int(d["payload_offset"]), int(res[k]["out_len"])
            out.append(regen[o:o + ln].tobytes() if res[k]["status"] == 0 else b"")
        return out

    def payloads(self) -> list[bytes]:
        return [self.ps.arena[int(d["payload_offset"]):int(d["payload_offset"]) + int(d["payload_size"])].tobytes()
                for d in self.ps.descs]


class DecompressRange:
    """One rank's decompress batch of a sharded container decompress, in device buffers that grow
    as needed and are reused from step to step: the planned slices' descriptors and re-coded
    streams (d_desc, d_in), the regenerated bytes (d_work), the results (d_res), and their packed
    copy (d_packed, d_offsets) for the gather to rank 0.  upload() takes a host ParsedStream
    (DecompressPlan.parsed / shard.subset) or device tensors received from rank 0."""

    def __init__(self, ctx: Context, device=None):
        self.ctx = ctx
        self.device = torch.device("cuda", ctx.device) if device is None else device
        self.n = 0
        self._cap = {}

    def _buf(self, name: str, nbytes: int, dtype=torch.uint8) -> torch.Tensor:
        itemsize = torch.empty(0, dtype=dtype).element_size()
        count = max(1, (nbytes + itemsize - 1) // itemsize)
        t = self._cap.get(name)
        if t is None or t.numel() < count:
            t = torch.empty(count + count // 16, dtype=dtype, device=self.device)
            self._cap[name] = t
        return t

    def upload(self, descs, arena, n: int, work_len: int, max_mb_width: int, max_mb_height: int, stream=None):
        """descs / arena: numpy (host) or uint8 torch tensors (device)."""
        self.n, self.work_len = n, work_len
        self.max_mb_width, self.max_mb_height = max_mb_width, max_mb_height
        nd = n * SLICE_DESC.itemsize
        self.d_desc = self._buf("desc", nd)
        self.d_in = self._buf("in", (arena.nbytes if isinstance(arena, np.ndarray) else arena.numel()) + 16)
        with torch.cuda.stream(stream) if stream is not None else _null():
            for dst, src, k in ((self.d_desc, descs, nd), (self.d_in, arena, None)):
                if isinstance(src, np.ndarray):
                    src = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1))
                k = src.numel() if k is None else k
                if k:
                    dst[:k].copy_(src[:k], non_blocking=False)
        self.d_work = self._buf("work", work_len + 16)
        self.d_res = self._buf("res", max(1, n) * SLICE_RESULT.itemsize)

    def run(self, model: int = MODEL_PARALLEL, stream=None):
        self.ctx.decompress_slices(self.d_desc, self.n, self.max_mb_width, self.max_mb_height, self.d_in, self.d_work,
                                   self.d_res, model, stream)

    def pack(self, stream=None):
        d_packed = self._buf("packed", self.work_len + 16)
        d_offsets = self._buf("offsets", 8 * (self.n + 1), torch.int64)
        self.ctx.pack_outputs(self.d_desc, self.d_res, self.n, self.d_work, d_packed, d_offsets, stream)
        return d_packed, d_offsets

    def results(self) -> np.ndarray:
        return self.d_res[:max(1, self.n) * SLICE_RESULT.itemsize].cpu().numpy().view(SLICE_RESULT)[: self.n]


class UnitBatch:
    """The units of a piece plan (DecompressPlan.parsed_units / shard.subset_units: whole slices and
    the pieces of split slices) on the device.  Buffers in unit order: d_desc, d_in (the streams),
    d_recs (the seam records), d_work (the regenerated bytes), d_res.
    decompress(): the units that are pieces -- they start at a seam, stop after n_mbs macroblocks or
    keep only their share -- through avr_decompress_pieces_m on the model's coder, the whole slices (field, MBAFF and
    over-wide ones among them, which are never cut) through avr_decompress_slices, one launch after
    the other on the stream; the descriptor rows of each launch are gathered, and its result rows
    scattered back, by index with torch.  pack(): one avr_pack_pieces over all units."""

    def __init__(self, ctx: Context, part: ParsedStream, device=None):
        self.ctx, self.part = ctx, part
        self.device = torch.device("cuda", ctx.device) if device is None else device
        self.n = n = len(part.descs)
        self.d_desc = _dev_bytes(part.descs, self.device).view(n, SLICE_DESC.itemsize)
        self.d_in = _dev_bytes(part.arena, self.device)
        self.d_work = torch.zeros(max(16, part.work_len + 16), dtype=torch.uint8, device=self.device)
        self.d_res = torch.zeros(n, SLICE_RESULT.itemsize, dtype=torch.uint8, device=self.device)
        self.n_recs = len(part.recs) // part.rec_stride if part.rec_stride else 0
        self.d_recs = (_dev_bytes(part.recs, self.device) if self.n_recs
                       else torch.zeros(16, dtype=torch.uint8, device=self.device))
        pc = part.pieces
        self.is_piece = (pc["seam"] >= 0) | (pc["n_mbs"] > 0) | (pc["keep"] != KEEP_ALL)

    def decompress(self, model: int = MODEL_PARALLEL, stream=None):
        part, n = self.part, self.n
        idx_p, idx_r = np.flatnonzero(self.is_piece), np.flatnonzero(~self.is_piece)
        if len(idx_p) and model not in (MODEL_PARALLEL, MODEL_PARALLEL32):
            raise ValueError("UnitBatch: pieces exist in the parallel models' containers only")
        with torch.cuda.stream(stream) if stream is not None else _null():
            for idx, pieces in ((idx_p, True), (idx_r, False)):
                if not len(idx):
                    continue
                whole = len(idx) == n
                rows = None if whole else torch.from_numpy(idx).to(self.device)
                dd = self.d_desc if whole else self.d_desc[rows].contiguous()
                dr = self.d_res if whole else torch.zeros(len(idx), SLICE_RESULT.itemsize, dtype=torch.uint8,
                                                          device=self.device)
                if pieces:
                    self.ctx.decompress_pieces(dd, part.pieces[idx], len(idx), int(part.descs["mb_width"][idx].max()),
                                               part.max_mb_height, self.d_recs, self.n_recs, part.rec_stride,
                                               self.d_in, self.d_work, dr, stream, model=model)
                else:
                    self.ctx.decompress_slices(dd, len(idx), part.max_mb_width, part.max_mb_height, self.d_in,
                                               self.d_work, dr, model, stream)
                if not whole:
                    self.d_res[rows] = dr

    def pack(self, pieces: "np.ndarray | None" = None, stream=None):
        """(d_packed uint8, d_offsets int64[n + 1], d_kept int32[n] holding uint32, d_status int32[n]):
        unit k's kept bytes at d_offsets[k].  pieces: another PIECE array than the batch's (tests)."""
        n = self.n
        d_pieces = _dev_bytes(np.ascontiguousarray(self.part.pieces if pieces is None else pieces, dtype=PIECE),
                              self.device)
        d_packed = torch.zeros(max(16, self.part.work_len + 16), dtype=torch.uint8, device=self.device)
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        d_kept = torch.zeros(max(1, n), dtype=torch.int32, device=self.device)
        d_status = torch.zeros(max(1, n), dtype=torch.int32, device=self.device)
        self.ctx.pack_pieces(self.d_desc, d_pieces, self.d_res, n, self.d_work, d_packed, d_offsets, d_kept,
                             d_status, stream)
        return d_packed, d_offsets, d_kept, d_status

    def crcs(self, d_packed, d_offsets, d_kept, stream=None):
        """The CRC-32 of every unit's kept bytes in pack()'s outputs (avr_crc_spans): (d_crc, d_status) per
        unit; shard.collapse_unit_crcs folds a cut slice's into the slice's."""
        return _crc_spans(self, *_packed_spans(d_offsets, self.n, d_kept), d_packed, stream)

    def results(self) -> np.ndarray:
        return self.d_res.cpu().numpy().reshape(-1).view(SLICE_RESULT)[: self.n]


class SplitBatch:
    """A rank's split candidates (split_plan of ps.descs at split_bytes: every slice of ps must be one)
    on the device, compressed as the whole-file compress of model (MODEL_PARALLEL, or MODEL_PARALLEL32
    with Context.split_p32) compresses them: each slice cut as it is walked, its pieces' streams one after the other in d_out.  roundtrip() runs, on one
    stream,
      compress()    avr_compress_split_slices
      read_back()   waits for it; cuts, piece ends, records and results to the host, where the unit
                    descriptors and the PIECE array of every piece are built (the streams stay on the
                    device); a slice whose cut count or piece ends are not a walk's gets SLICE_CODER
      stage()       avr_stage_pieces: the pieces' streams into the aligned layout the decompress reads
      decompress()  avr_decompress_pieces over all units
      pack()        avr_pack_pieces: every piece cut down to its share of its slice
      verify()      avr_verify_units: d_verdict per slice
    and the halves are callable one by one in that order.  recoded() / verdicts() / seams() give the
    host what a container needs."""

    def __init__(self, ctx: Context, ps: ParsedStream, split_bytes: int, device=None, model: int = MODEL_PARALLEL):
        from . import split_plan
        if model not in (MODEL_PARALLEL, MODEL_PARALLEL32):
            raise ValueError("SplitBatch: the parallel models only")
        self.ctx, self.ps, self.split_bytes, self.model = ctx, ps, int(split_bytes), int(model)
        self.device = dev = torch.device("cuda", ctx.device) if device is None else device
        self.n = n = len(ps.descs)
        self.plan = plan = split_plan(ps.descs, split_bytes)
        if plan.n_candidates != n:
            raise ValueError("SplitBatch: every slice of the batch must be a split candidate (split_plan)")
        d = ps.descs.copy()
        d["out_capacity"] = plan.out_capacity
        room = (d["out_capacity"].astype(np.int64) + 15) & ~15
        d["out_offset"] = np.cumsum(room) - room
        self.descs = d
        self.work_len = int(room.sum())
        self.max_w = int(d["mb_width"].max()) if n else 1
        self.d_desc = _dev_bytes(d, dev)
        self.d_in = _dev_bytes(ps.arena, dev)
        self.d_out = torch.zeros(self.work_len + 16, dtype=torch.uint8, device=dev)
        self.d_res_c = torch.zeros(max(1, n) * SLICE_RESULT.itemsize, dtype=torch.uint8, device=dev)
        self.d_recs = torch.zeros(plan.n_recs * plan.rec_stride + 64, dtype=torch.uint8, device=dev)
        self.d_cuts = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        self.d_piece_end = torch.zeros(max(1, plan.n_recs), dtype=torch.int32, device=dev)
        self.d_verdict = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        self.nu = 0

    def compress(self, stream=None):
        p = self.plan
        self.ctx.compress_split_slices(self.d_desc, self.n, self.max_w, self.ps.max_mb_height, self.d_in, self.d_out,
                                       self.d_res_c, p.slots, self.split_bytes, self.d_recs, p.n_recs, p.rec_stride,
                                       self.d_cuts, self.d_piece_end, stream, model=self.model)

    def read_back(self, stream=None):
        from . import SEAM_HEAD, SLICE_CODER
        (stream if stream is not None else torch.cuda.current_stream(self.device)).synchronize()
        p, n = self.plan, self.n
        self.res = self.d_res_c.cpu().numpy().view(SLICE_RESULT)[:n].copy()
        self.cuts = self.d_cuts.cpu().numpy().view(np.uint32)[:n].copy()
        self.piece_end = self.d_piece_end.cpu().numpy().view(np.uint32)[:p.n_recs].copy()
        self.recs = self.d_recs.cpu().numpy()[:p.n_recs * p.rec_stride].copy()
        # what the walk itself can fail (seams_build's index checks): too many cuts, piece ends that
        # are not the stream's
        self.status = self.res["status"].astype(np.int32)
        rows, pc, src, first = [], [], [], [0]   # per unit: (slice, first_mb, stream length), PIECE, source
        for k in range(n):
            f, cap, nc = int(p.slots[k]["first"]), int(p.slots[k]["cap"]), int(self.cuts[k])
            size, mb0 = int(self.descs[k]["payload_size"]), int(self.descs[k]["first_mb"])
            if self.status[k] == 0:
                ends = [int(e) for e in self.piece_end[f:f + nc + 1]] if nc < cap else None
                head = self.recs.reshape(-1, p.rec_stride)[f:f + nc, :SEAM_HEAD.itemsize].copy().view(SEAM_HEAD).reshape(-1)
                mbs = [mb0] + [int(x) for x in head["first_mb"]]
                qs = [0] + [int(x) for x in head["q"]]
                # cuts move forward in macroblocks and in bytes of the payload
                if (ends is None or ends != sorted(ends) or ends[-1] != int(self.res[k]["out_len"])
                        or any(y <= x for x, y in zip(mbs, mbs[1:])) or any(y <= x for x, y in zip(qs, qs[1:]))
                        or qs[-1] >= size):
                    self.status[k] = SLICE_CODER
            if self.status[k] == 0:
                for i in range(nc + 1):
                    last = i == nc
                    begin = ends[i - 1] if i else 0
                    rows.append((k, mbs[i], ends[i] - begin))
                    pc.append((f + i - 1 if i else -1, 0 if last else mbs[i + 1] - mbs[i], k,
                               KEEP_ALL if last else qs[i + 1] - qs[i]))
                    src.append(int(self.descs[k]["out_offset"]) + begin)
            first.append(len(rows))
        self.nu = nu = len(rows)
        self.units = self.descs[[r[0] for r in rows]].copy() if nu else np.zeros(0, SLICE_DESC)
        self.pieces = np.array(pc, dtype=PIECE) if nu else np.zeros(0, PIECE)
        if nu:
            self.units["first_mb"] = [r[1] for r in rows]
            self.units["payload_size"] = self.units["read_limit"] = [r[2] for r in rows]
            self.units["out_capacity"] = self.descs["payload_size"][[r[0] for r in rows]] + 4096
        self.first = np.array(first, dtype=np.uint32)
        room = (self.units["out_capacity"].astype(np.int64) + 15) & ~15
        self.units["out_offset"] = np.cumsum(room) - room
        self.unit_work_len = int(room.sum())
        self.arena_cap = int((((self.units["payload_size"].astype(np.int64) + 16 + 15) & ~15).sum())) + 16
        dev = self.device
        self.d_units = _dev_bytes(self.units, dev) if nu else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_src = torch.from_numpy(np.array(src, dtype=np.int64)).to(dev) if nu else torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_first = torch.from_numpy(self.first.view(np.int32).copy()).to(dev)
        self.d_arena = torch.zeros(self.arena_cap, dtype=torch.uint8, device=dev)
        self.d_stage_off = torch.zeros(nu + 1, dtype=torch.int64, device=dev)
        self.d_stage_status = torch.zeros(max(1, nu), dtype=torch.int32, device=dev)
        self.d_unit_work = torch.zeros(self.unit_work_len + 16, dtype=torch.uint8, device=dev)
        self.d_unit_res = torch.zeros(max(1, nu) * SLICE_RESULT.itemsize, dtype=torch.uint8, device=dev)

    def stage(self, stream=None):
        self.ctx.stage_pieces(self.d_units, self.d_src, self.nu, self.d_out, self.work_len, self.d_arena, self.arena_cap,
                              self.d_stage_off, self.d_stage_status, stream)

    def decompress(self, stream=None):
        if self.nu:
            self.ctx.decompress_pieces(self.d_units, self.pieces, self.nu, self.max_w, self.ps.max_mb_height,
                                       self.d_recs, self.plan.n_recs, self.plan.rec_stride, self.d_arena,
                                       self.d_unit_work, self.d_unit_res, stream, model=self.model)

    def pack(self, stream=None):
        nu, dev = self.nu, self.device
        self.d_pieces = _dev_bytes(self.pieces, dev) if nu else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_packed = torch.zeros(self.unit_work_len + 16, dtype=torch.uint8, device=dev)
        self.d_pack_off = torch.zeros(nu + 1, dtype=torch.int64, device=dev)
        self.d_kept = torch.zeros(max(1, nu), dtype=torch.int32, device=dev)
        self.d_unit_status = torch.zeros(max(1, nu), dtype=torch.int32, device=dev)
        self.ctx.pack_pieces(self.d_units, self.d_pieces, self.d_unit_res, nu, self.d_unit_work, self.d_packed,
                             self.d_pack_off, self.d_kept, self.d_unit_status, stream)

    def verify(self, stream=None):
        self.ctx.verify_units(self.d_desc, self.d_res_c, self.n, self.d_first, self.nu, self.d_in, self.d_packed,
                              self.d_pack_off, self.d_kept, self.d_unit_status, self.d_verdict, stream)

    def roundtrip(self, stream=None):
        if stream is not None:   # the constructor's uploads and zero fills ran on the current stream
            stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream) if stream is not None else _null():
            self.compress(stream)
            self.read_back(stream)
            self.stage(stream)
            self.decompress(stream)
            self.pack(stream)
            self.verify(stream)

    def crcs(self, stream=None):
        """The CRC-32 of every slice's payload in the input arena (avr_crc_spans): (d_crc, d_status)."""
        return _crc_spans(self, *_payload_spans(self.ps.descs, self.device), self.d_in, stream)

    def pack_recoded(self, stream=None):
        """The slices' re-coded bytes packed contiguously on the device (avr_pack_outputs):
        (d_packed uint8, d_offsets int64[n + 1])."""
        d_packed = torch.zeros(self.work_len + 16, dtype=torch.uint8, device=self.device)
        d_offsets = torch.zeros(max(1, self.n) + 1, dtype=torch.int64, device=self.device)
        self.ctx.pack_outputs(self.d_desc, self.d_res_c, self.n, self.d_out, d_packed, d_offsets, stream)
        return d_packed, d_offsets

    # ----------------------------------------------------------------- results (host copies)
    def verdicts(self) -> np.ndarray:
        """1 bit-exact, 0 mismatch (or refused at read_back), 2 not coded, per slice."""
        return self.d_verdict.cpu().numpy()[: self.n]

    def recoded(self) -> list[bytes]:
        """Per-slice re-coded bytes, the pieces' streams one after the other (b'' where the walk failed)."""
        work = self.d_out.cpu().numpy()
        return [work[int(d["out_offset"]):int(d["out_offset"]) + int(r["out_len"])].tobytes() if st == 0 else b""
                for d, r, st in zip(self.descs, self.res, self.status)]

    def seams(self, check_cuts: bool = True):
        """(status int32[n], [Block field 16 per slice, b'' without a cut]) through avr_seams_build; a
        slice refused at read_back keeps SLICE_CODER and gets no field."""
        from . import seams_build
        res = self.res.copy()
        res["status"] = self.status
        p = self.plan
        return seams_build(self.ps.descs, self.ps.arena, res, p.slots, self.cuts, self.piece_end, self.recs,
                           p.rec_stride, check_cuts)


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
