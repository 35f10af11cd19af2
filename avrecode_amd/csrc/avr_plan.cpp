// The decompress planner: a container read into the slice (or piece) batch the device regenerates,
// and the splice of the regenerated slices back into the file -- the whole-file decompress
// (avr_api.cpp) and the sharded decompress plans of the C ABI (avr_dec_plan_*).  No HIP: every
// entry point here works without a device, on bytes the caller does not control
// (tests/native/plan_fuzz.cpp runs them under sanitizers).
#include <cstdio>
#include <cstdlib>

#include "avr_host.h"

using namespace avr_host;

namespace avr_host {

namespace {
// Block field 18 of block i taken into the job: one value per unit -- the cuts' q say where the units
// end, the last at `size` -- combined in order into the CRC-32 of the slice's payload.  False: not one
// value per unit.
bool take_unit_crcs(DecJob* j, size_t i, const std::vector<uint32_t>& q) {
  const avr::PbBlock& b = j->blocks[i];
  if (b.unit_crcs.size() != 4 * (q.size() + 1)) return false;
  if (j->block_checked.empty()) {
    j->block_checked.assign(j->blocks.size(), 0);
    j->block_crc.assign(j->blocks.size(), 0);
  }
  uint32_t crc = 0;
  for (size_t u = 0; u <= q.size(); u++) {
    const uint64_t lo = u ? q[u - 1] : 0, hi = u < q.size() ? q[u] : (uint64_t)b.size;
    crc = avr_crc32_combine(crc, b.unit_crc(u), hi - lo);
  }
  j->block_checked[i] = 1;
  j->block_crc[i] = crc;
  return true;
}
}  // namespace

int decompress_setup(ErrSink* c, const uint8_t* in, size_t n, DecJob* j, Plan* plan, SplitPlan* sp) {
  const bool tm = getenv("AVR_ASM_TIMING") != nullptr;
  double t0 = now_s();
  std::string version;
  avr::PbFileCrc fc;
  if (!avr::pb_parse(in, n, &j->blocks, &version, nullptr, &fc)) return fail(c, AVR_ERR_FORMAT, "not a Recoded protobuf");
  j->has_crc = fc.present;
  j->file_crc = fc.value;
  j->block_checked.clear();
  j->block_crc.clear();
  j->model = avr::model_of_version(version);
  // another avrecode-amd container format (the round-2 "avrecode-amd:P", ...) would be read as a
  // reference-model container and fail late: refuse it here
  if (j->model < 0)
    return fail(c, AVR_ERR_FORMAT, "unsupported container version " + version + " (expected " + avr::kParallelModelTag +
                                       " or " + avr::kParallel32ModelTag + ")");
  j->parallel = parallel_model(j->model);
  const bool esc_tag = avr::escaped_version(version);
  // seams (field 16) belong to the u64 coder's containers and, of the P32 coder's, to those tagged S
  const bool seams_ok = j->model == AVR_MODEL_PARALLEL || avr::split32_version(version);
  // read_packet (recode.cpp:1359-1409): literals and surrogate blocks form the stream -- its layout
  // first, then one allocation, the markers, and the literal copies and 'X' fills on host threads
  uint64_t seq = 1;
  size_t total = 0;
  // An escaped block (field 17) stands for size + escapes file bytes, and its surrogate occupies as
  // many: the literals around it hold what places every later byte of the file -- an MP4's NAL
  // length prefixes and its moov sample tables -- so a surrogate of `size` bytes would shift every
  // later sample under the parse.
  for (auto& b : j->blocks) {
    if ((int)b.has_literal + (int)b.has_cabac + (int)b.has_skip != 1)
      return fail(c, AVR_ERR_FORMAT, "Invalid input block: must have exactly one type");
    if (b.has_escapes && (!b.has_cabac || !esc_tag))
      return fail(c, AVR_ERR_FORMAT, "escapes field on a block that is not coded, or under a tag without E");
    if (b.has_literal) {
      total += b.literal_len;
    } else if (b.has_cabac) {
      if (!b.has_size) return fail(c, AVR_ERR_FORMAT, "CABAC block requires size field.");
      if (b.size < avr::kSurrogateMarkerBytes || b.size > ((int64_t)1 << 31))
        return fail(c, AVR_ERR_FORMAT, "Invalid coded block size for surrogate: " + std::to_string(b.size));
      if (b.has_escapes && (b.escapes == 0 || b.escapes > (uint64_t)b.size / 2 + 1))
        return fail(c, AVR_ERR_FORMAT, "Invalid escapes count in coded block: " + std::to_string(b.escapes));
      total += (size_t)b.size + (size_t)b.escapes;
      // an uncut block's one unit is the slice (a cut block's values wait for its seams, below)
      if (b.has_unit_crcs && !b.has_seams) take_unit_crcs(j, (size_t)(&b - j->blocks.data()), {});
    } else if (!b.skip_coded) {
      return fail(c, AVR_ERR_FORMAT, "Unknown input block type");
    }
  }
  j->stream.resize(total);
  // the surrogate fills: no 0x00 / 0x03 byte in them ('X'), so the parse steps over them
  avr::SkipRanges skips;
  {
    std::vector<avr::PbCopy> fills;
    fills.reserve(j->blocks.size());
    size_t at = 0;
    for (auto& b : j->blocks) {
      if (b.has_literal) {
        if (b.literal_len) fills.push_back({at, b.literal, b.literal_len});
        at += b.literal_len;
      } else if (b.has_cabac) {
        avr::surrogate_marker(seq++, j->stream.data() + at);
        const size_t sur = (size_t)b.size + (size_t)b.escapes;   // the marker, then 'X' fill
        fills.push_back({at + 8, nullptr, sur - 8});
        if (sur > 8) skips.push_back({at + 8, at + sur});
        at += sur;
      }
    }
    parallel_copies(fills, j->stream.data(), (uint8_t)'X');
  }
  static_assert('X' != 0 && 'X' != 3, "surrogate fill: no start-code or emulation-prevention byte");
  if (tm) fprintf(stderr, "setup: pb+stream %.3f s\n", now_s() - t0), t0 = now_s();
  ParsedFile pf;
  if (int r = parse_file(c, j->stream.data(), j->stream.size(), &pf, /*views=*/true, &skips)) return r;
  if (tm) fprintf(stderr, "setup: parse %.3f s\n", now_s() - t0), t0 = now_s();
  // recognize_coded_block (recode.cpp:1546-1573): slices claim coded blocks in order
  j->desc_of_block.assign(j->blocks.size(), -1);
  size_t next_coded = 0;
  uint64_t seq_check = 1;
  std::vector<avr_slice_desc> descs;
  std::vector<int> block_of;
  for (auto& s : pf.slices) {
    while (next_coded < j->blocks.size() && !j->blocks[next_coded].has_cabac && !j->blocks[next_coded].has_skip)
      next_coded++;
    if (next_coded >= j->blocks.size())
      return fail(c, AVR_ERR_FORMAT, "Coded block expected, but not recorded in the compressed data.");
    const avr::PbBlock& b = j->blocks[next_coded];
    if ((size_t)b.size + (size_t)b.escapes != s.size) return fail(c, AVR_ERR_FORMAT, "Invalid surrogate block size.");
    avr_slice_desc d = desc_from_header(s);
    if (b.has_cabac) {
      uint8_t mk[8];
      avr::surrogate_marker(seq_check++, mk);
      if (memcmp(s.payload(), mk, 8) != 0) return fail(c, AVR_ERR_FORMAT, "Invalid surrogate marker in coded block.");
      d.payload_size = (uint32_t)b.cabac_len;
      d.read_limit = (uint32_t)b.cabac_len;
      d.out_capacity = (uint32_t)(b.size + 64);
    } else {
      d.coded = 0;
    }
    if (b.has_cabac && b.has_seams) {   // a split block: its pieces go to the split plan
      if (!sp) return fail(c, AVR_ERR_UNSUPPORTED, "split slices (block field 16) decompress through the whole-file calls only");
      if (!seams_ok || d.structure != AVR_STRUCT_FRAME || d.mb_width > SplitPlan::kMringCols)
        return fail(c, AVR_ERR_FORMAT, "seams on a block that cannot be split");
      SeamsDecoded sd;
      if (!seams_decode(b.seams, b.seams_len, d, sp->stride, &sd))
        return fail(c, AVR_ERR_FORMAT, "Invalid seams field in coded block.");
      uint64_t tot = 0;
      for (uint32_t l : sd.piece_len) tot += l;
      if (tot != b.cabac_len || sd.q.back() >= (uint64_t)b.size || sd.first_mb[0] <= (uint32_t)d.first_mb)
        return fail(c, AVR_ERR_FORMAT, "Invalid seams field in coded block.");
      if (b.has_unit_crcs && !take_unit_crcs(j, next_coded, sd.q))
        return fail(c, AVR_ERR_FORMAT, "unit checksums (block field 18): not one value per piece");
      SplitBlock x;
      x.block = (int)next_coded;
      x.first = (int)sp->plan.descs.size();
      x.pieces = sd.cuts + 1;
      x.q = sd.q;
      const uint32_t rec0 = (uint32_t)(sp->recs.size() / sp->stride);
      sp->recs.insert(sp->recs.end(), sd.recs.begin(), sd.recs.end());
      append_pieces(&sp->plan, &sp->ctl, d, b.cabac, sd.piece_len, sd.first_mb, rec0, [&](size_t i) {   // its share of q
        return (uint32_t)((i < (size_t)sd.cuts ? sd.q[i] : (uint32_t)b.size) - (i ? sd.q[i - 1] : 0u) + 4096);
      });
      j->desc_of_block[next_coded] = -2 - (int)j->splits.size();
      j->splits.push_back(std::move(x));
      next_coded++;
      continue;
    }
    if (j->parallel && !d.coded) {   // the parallel model has no cross-slice state: skip it
      next_coded++;
      continue;
    }
    block_of.push_back((int)next_coded);
    descs.push_back(d);
    next_coded++;
  }
  // all checks passed: append to the shared plan (append_aligned's layout: 16-byte aligned streams,
  // each followed by >= 16 zero bytes), the re-coded streams copied on host threads
  if (!plan) {
    for (size_t k = 0; k < descs.size(); k++) j->desc_of_block[block_of[k]] = (int)k;
    return AVR_OK;
  }
  std::vector<avr::PbCopy> copies;
  copies.reserve(descs.size());
  uint64_t at = plan->layout_only ? plan->arena_end : plan->arena.size();
  for (size_t k = 0; k < descs.size(); k++) {
    avr_slice_desc& d = descs[k];
    const avr::PbBlock& b = j->blocks[block_of[k]];
    if (d.coded) {
      d.payload_offset = (at + 15) & ~(uint64_t)15;
      copies.push_back({(size_t)d.payload_offset, b.cabac, b.cabac_len});
      at = d.payload_offset + b.cabac_len + 16;
      plan->max_w = std::max(plan->max_w, ring_cols(d));
    }
  }
  if (plan->layout_only) {
    plan->arena_copies.insert(plan->arena_copies.end(), copies.begin(), copies.end());
    plan->arena_end = at;
  } else {
    const size_t a0 = plan->arena.size();
    plan->arena.resize(at);
    zero_gaps(copies, plan->arena.data(), a0, at);
    parallel_copies(copies, plan->arena.data());
  }
  for (size_t k = 0; k < descs.size(); k++) {
    j->desc_of_block[block_of[k]] = (int)plan->descs.size();
    plan->descs.push_back(descs[k]);
  }
  if (tm) fprintf(stderr, "setup: match+arena %.3f s\n", now_s() - t0);
  return AVR_OK;
}

}  // namespace avr_host

// ------------------------------------------------------------------ sharded decompress plans
// (struct avr_dec_plan: avr_host.h -- the reader of avr_api.cpp works on one too)

namespace {

// File coordinates from the container alone: block i stands for file bytes [block_off[i],
// block_off[i + 1]) -- a literal for its length, a coded block for size (+ escapes) bytes, a
// skip_coded block for none (decompress_setup has checked every size).
void map_blocks(avr_dec_plan* h) {
  const std::vector<avr::PbBlock>& bl = h->job.blocks;
  h->block_off.assign(bl.size() + 1, 0);
  uint64_t at = 0;
  for (size_t i = 0; i < bl.size(); i++) {
    h->block_off[i] = at;
    if (bl[i].has_literal) at += bl[i].literal_len;
    else if (bl[i].has_cabac) at += (uint64_t)bl[i].size + bl[i].escapes;
    h->escapes |= bl[i].has_escapes;
  }
  h->block_off[bl.size()] = at;
}

// splice_job's output laid out: the literal and regenerated-slice copies, the last-byte patches
// (position, byte) and the total length.  An escaped block (field 17) is one more copy job: its
// bytes -- regenerated, patched, then escaped -- stand in `side`, which the layout's caller keeps
// until the copies are done.
// A checked container (job.has_crc) is checked here, before anything is written: the fold of the
// blocks' CRCs (fold_file_crc) -- the slices' from crcs, or without them from regen on host threads --
// against the container's value, AVR_ERR_CHECKSUM when they differ.  So is every block with unit
// checksums (field 18): its values combined (job.block_crc) against the patched CRC of its slice's
// regenerated bytes, from the same crcs or bytes, with or without the file's field.
int splice_layout(const avr_dec_plan* h, const int32_t* status, const uint8_t* regen, size_t regen_len,
                  const uint64_t* offsets, const uint32_t* lens, std::vector<avr::PbCopy>* copies,
                  std::vector<std::pair<size_t, uint8_t>>* patches, std::vector<std::vector<uint8_t>>* side,
                  size_t* total, const uint32_t* crcs = nullptr) {
  const DecJob& j = h->job;
  const int ns = (int)h->plan.descs.size();
  // every slice's regenerated bytes inside regen and within its own output capacity
  for (int k = 0; k < ns; k++)
    if (status[k] == 0 && (offsets[k] > regen_len || lens[k] > regen_len - offsets[k] ||
                           lens[k] > h->plan.descs[k].out_capacity))
      return AVR_ERR_INVALID_ARGUMENT;
  copies->reserve(j.blocks.size());
  std::vector<CrcItem> items;
  std::vector<std::pair<size_t, size_t>> unit_checks;   // (item, block): blocks with field 18
  if (j.has_crc || !j.block_checked.empty()) items.reserve(j.blocks.size());
  // the patched CRC of a coded block's regenerated (unescaped) bytes: the file's item, a unit check's, or both
  auto slice_item = [&](size_t i, int k, bool in_file) {
    if (j.unit_checked(i)) unit_checks.push_back({items.size(), i});
    items.push_back(crc_item_of_slice(j.blocks[i], regen + offsets[k], lens[k], crcs ? &crcs[k] : nullptr));
    items.back().in_file = in_file;
  };
  size_t at = 0;
  for (size_t i = 0; i < j.blocks.size(); i++) {
    const avr::PbBlock& b = j.blocks[i];
    if (b.has_literal) {
      if (b.literal_len) copies->push_back({at, b.literal, b.literal_len});
      if (j.has_crc) items.push_back(CrcItem{b.literal, b.literal_len});
      at += b.literal_len;
      continue;
    }
    if (!b.has_cabac) continue;
    const int k = j.desc_of_block[i];
    if (k < 0) return AVR_ERR_FORMAT;          // "Not all blocks were decoded." (recode.cpp:1354)
    if (status[k]) return AVR_ERR_FORMAT;      // the slice failed to decode
    const size_t len = lens[k];
    if (b.has_escapes) {
      std::vector<uint8_t> p(regen + offsets[k], regen + offsets[k] + len);
      patch_last_byte(b, len, &p);
      std::vector<uint8_t> e = avr::escape(p.data(), p.size());
      if (e.size() - p.size() != b.escapes) return AVR_ERR_FORMAT;   // not the count the block recorded
      side->push_back(std::move(e));
      copies->push_back({at, side->back().data(), side->back().size()});
      if (j.has_crc) items.push_back(CrcItem{side->back().data(), side->back().size()});
      if (j.unit_checked(i)) slice_item(i, k, false);
      at += side->back().size();
      continue;
    }
    if (len) copies->push_back({at, regen + offsets[k], len});
    if (j.has_crc || j.unit_checked(i)) slice_item(i, k, j.has_crc);
    const LastByte rule = last_byte_rule(b, len);
    const size_t m = len + (rule == LastByte::kAppend);
    if (rule != LastByte::kKeep) patches->push_back({at + m - 1, (uint8_t)b.last_byte[0]});
    at += m;
  }
  *total = at;
  resolve_crc_items(&items);
  for (const auto& uc : unit_checks)
    if (items[uc.first].crc != j.block_crc[uc.second]) return AVR_ERR_CHECKSUM;
  if (j.has_crc && combine_crc_items(items) != j.file_crc) return AVR_ERR_CHECKSUM;
  return AVR_OK;
}

// a splice written out: the copies on host threads, then the last-byte patches
void write_splice(const std::vector<avr::PbCopy>& copies, const std::vector<std::pair<size_t, uint8_t>>& patches,
                  uint8_t* out) {
  parallel_copies(copies, out);
  for (const auto& pt : patches) out[pt.first] = pt.second;
}

}  // namespace

// ------------------------------------------------------------------ range reads: the planner
namespace avr_host {

size_t block_of_offset(const avr_dec_plan* h, uint64_t off) {
  // the last block that starts at or before off and stands for at least one byte
  const auto it = std::upper_bound(h->block_off.begin(), h->block_off.end(), off);
  return (size_t)(it - h->block_off.begin()) - 1;
}

// One window [off, off + len) of the file (include/avrecode.h, avr_dec_plan_range).  The blocks it
// touches in file order: a literal gives spans out of the container, a coded block the units whose
// share [q0, q1) of its slice the window reaches, spans out of their regenerated bytes and -- for
// every unit from the first selected to the last -- a tail.  Runs on bytes the caller does not
// control: everything read from the plan is checked against the block it belongs to before it is
// emitted.
int plan_range(const avr_dec_plan* h, uint64_t off, uint64_t len, uint32_t span_cap, RangePlan* rp) {
  if (!h || !h->avrc || !h->pieces || !rp || off + len < off) return AVR_ERR_INVALID_ARGUMENT;
  if (!span_cap) span_cap = kRangeSpanBytes;
  if (span_cap < 16 || span_cap > (1u << 30)) return AVR_ERR_INVALID_ARGUMENT;
  if (h->escapes) return AVR_ERR_UNSUPPORTED;   // an escaped block's bytes are not a crop of its regenerated bytes
  const std::vector<avr::PbBlock>& bl = h->job.blocks;
  const size_t nb = bl.size(), nu = h->units.size();
  if (h->block_off.size() != nb + 1 || h->unit_first.size() != nb + 1 || h->unit_q0.size() != nu ||
      h->unit_pieces.size() != nu)
    return AVR_ERR_INVALID_ARGUMENT;
  const uint64_t file_size = h->block_off[nb];
  rp->spans.clear();
  rp->tails.clear();
  rp->info = avr_range_info{};
  rp->info.file_size = file_size;
  const uint64_t w0 = std::min(off, file_size), w1 = w0 + std::min(len, file_size - w0);
  rp->info.off = w0;
  rp->info.len = w1 - w0;
  if (w0 == w1) return AVR_OK;
  int ulo = -1, uhi = -1;
  // (source, src_off) + [a, b) of the file -> spans of at most span_cap bytes
  auto emit = [&](int32_t source, uint64_t src_off, uint64_t a, uint64_t b) {
    while (a < b) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(span_cap, b - a);
      rp->spans.push_back(avr_span{src_off, a - w0, n, source});
      src_off += n;
      a += n;
    }
  };
  // unit sources are written as plan indices first and rebased to unit_lo at the end
  for (size_t i = block_of_offset(h, w0); i < nb && h->block_off[i] < w1; i++) {
    const avr::PbBlock& b = bl[i];
    const uint64_t b0 = h->block_off[i], b1 = h->block_off[i + 1];
    const uint64_t a0 = std::max(b0, w0), a1 = std::min(b1, w1);
    if (a0 >= a1) continue;   // a block of no bytes (skip_coded, an empty literal)
    if (b.has_literal) {
      if (b1 - b0 != b.literal_len || b.literal < h->avrc || (size_t)(b.literal - h->avrc) > h->n ||
          b.literal_len > h->n - (size_t)(b.literal - h->avrc))
        return AVR_ERR_FORMAT;
      emit(AVR_SPAN_LITERAL, (uint64_t)(b.literal - h->avrc) + (a0 - b0), a0, a1);
      rp->info.literal_bytes += a1 - a0;
      continue;
    }
    const int u0 = h->unit_first[i], u1 = h->unit_first[i + 1];
    // a coded block that no slice claimed ("Not all blocks were decoded.", recode.cpp:1354)
    if (!b.has_cabac || u0 < 0 || u1 <= u0 || (size_t)u1 > nu || b.size <= 0 || (uint64_t)b.size != b1 - b0)
      return AVR_ERR_FORMAT;
    const uint32_t size = (uint32_t)b.size;
    for (int u = u0; u < u1; u++) {
      const bool last = u + 1 == u1;
      const uint32_t q0 = h->unit_q0[u], q1 = last ? size : h->unit_q0[u + 1];
      const avr_piece& pc = h->unit_pieces[u];
      // the cuts ascend inside the slice, and keep is this unit's share of it
      if (q0 > q1 || q1 > size || (u == u0 && q0 != 0) || (last ? pc.keep != UINT32_MAX : pc.keep != q1 - q0))
        return AVR_ERR_FORMAT;
      const uint64_t s0 = std::max(b0 + q0, a0), s1 = std::min(b0 + q1, a1);
      if (s0 >= s1) continue;
      if (ulo < 0) ulo = u;
      uhi = u + 1;
      emit(u, s0 - (b0 + q0), s0, s1);
    }
  }
  if (ulo >= 0) {
    rp->tails.reserve((size_t)(uhi - ulo));
    // the tails of [ulo, uhi): the blocks these units belong to, walked once more
    size_t i = block_of_offset(h, w0);
    for (int u = ulo; u < uhi; u++) {
      while (i < nb && h->unit_first[i + 1] <= u) i++;
      if (i >= nb) return AVR_ERR_FORMAT;
      const avr::PbBlock& b = bl[i];
      const bool last = u + 1 == h->unit_first[i + 1];
      avr_range_tail t{};
      t.size = (uint32_t)b.size;
      t.final_pos = AVR_RANGE_NO_POS;
      if (!last) {
        t.keep = h->unit_pieces[u].keep;
      } else {
        t.keep = UINT32_MAX;
        t.q_last = h->unit_q0[u];
        t.has_rule = b.has_parity && b.has_last_byte && !b.last_byte.empty();
        t.length_parity = b.length_parity ? 1 : 0;
        t.last_byte = t.has_rule ? (uint8_t)b.last_byte[0] : 0;
        const uint64_t fin = h->block_off[i] + (uint64_t)b.size - 1;
        if (fin >= w0 && fin < w1) t.final_pos = fin - w0;
      }
      rp->tails.push_back(t);
    }
    for (avr_span& s : rp->spans)
      if (s.source >= 0) s.source -= ulo;
  }
  // what was emitted tiles the window: in order, without gap or overlap
  uint64_t at = 0;
  for (const avr_span& s : rp->spans) {
    if (s.dst_off != at || !s.len || s.len > span_cap) return AVR_ERR_FORMAT;
    at += s.len;
  }
  if (at != w1 - w0 || rp->spans.size() > (size_t)INT32_MAX) return AVR_ERR_FORMAT;
  rp->info.unit_lo = std::max(ulo, 0);
  rp->info.unit_hi = std::max(uhi, 0);
  rp->info.n_spans = (int32_t)rp->spans.size();
  return AVR_OK;
}

}  // namespace avr_host

extern "C" {

int avr_dec_plan_file_size(const avr_dec_plan* h, uint64_t* size) {
  if (!h || !h->avrc || !size || h->block_off.empty()) return AVR_ERR_INVALID_ARGUMENT;
  *size = h->block_off.back();
  return AVR_OK;
}

int avr_dec_plan_range(const avr_dec_plan* h, uint64_t off, uint64_t len, uint32_t span_cap, avr_range_info* info,
                       avr_span** spans, avr_range_tail** tails) {
  if (!h || !info || !spans || !tails) return AVR_ERR_INVALID_ARGUMENT;
  *spans = nullptr;
  *tails = nullptr;
  return guarded(nullptr, [&]() -> int {
    RangePlan rp;
    if (int r = plan_range(h, off, len, span_cap, &rp)) return r;
    avr_span* s = (avr_span*)malloc(sizeof(avr_span) * std::max<size_t>(1, rp.spans.size()));
    avr_range_tail* t = (avr_range_tail*)malloc(sizeof(avr_range_tail) * std::max<size_t>(1, rp.tails.size()));
    if (!s || !t) {
      free(s);
      free(t);
      return AVR_ERR_OUT_OF_MEMORY;
    }
    if (!rp.spans.empty()) memcpy(s, rp.spans.data(), sizeof(avr_span) * rp.spans.size());
    if (!rp.tails.empty()) memcpy(t, rp.tails.data(), sizeof(avr_range_tail) * rp.tails.size());
    *spans = s;
    *tails = t;
    *info = rp.info;
    return AVR_OK;
  });
}

// What gather_spans_kernel and range_tails_kernel (avr_k_gather.hip) do, on host buffers: the CPU
// tests' reference for the two, and what tests/native/range_check.cpp drives under sanitizers.
int avr_dec_plan_range_apply(const avr_span* spans, int n_spans, const avr_range_tail* tails, int n_units,
                             const uint8_t* avrc, size_t avrc_len, const uint8_t* regen, size_t regen_len,
                             const uint64_t* unit_off, const avr_slice_result* res, uint8_t* out, size_t out_len,
                             int32_t* status) {
  if (n_spans < 0 || n_units < 0 || (n_spans && (!spans || !out)) || (n_units && (!tails || !unit_off || !res || !status)))
    return AVR_ERR_INVALID_ARGUMENT;
  // every span inside its source and the window, every final byte inside the window: before any write
  for (int k = 0; k < n_spans; k++) {
    const avr_span& s = spans[k];
    if (s.dst_off > out_len || s.len > out_len - s.dst_off) return AVR_ERR_INVALID_ARGUMENT;
    if (s.source == AVR_SPAN_LITERAL) {
      if (!avrc || s.src_off > avrc_len || s.len > avrc_len - s.src_off) return AVR_ERR_INVALID_ARGUMENT;
    } else {
      if (s.source < 0 || s.source >= n_units || !regen) return AVR_ERR_INVALID_ARGUMENT;
      const uint64_t base = unit_off[s.source];
      if (base > regen_len || s.src_off > regen_len - base || s.len > regen_len - base - s.src_off)
        return AVR_ERR_INVALID_ARGUMENT;
    }
  }
  for (int k = 0; k < n_units; k++)
    if (tails[k].final_pos != AVR_RANGE_NO_POS && tails[k].final_pos >= out_len) return AVR_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n_spans; k++) {
    const avr_span& s = spans[k];
    const uint8_t* src = s.source == AVR_SPAN_LITERAL ? avrc + s.src_off : regen + unit_off[s.source] + s.src_off;
    if (s.len) memcpy(out + s.dst_off, src, s.len);
  }
  bool failed = false;
  for (int k = 0; k < n_units; k++) {
    const avr_range_tail& t = tails[k];
    const avr_slice_result& r = res[k];
    int32_t st = r.status;
    if (!st) {
      if (t.keep != UINT32_MAX) {
        if (r.out_len < t.keep) st = AVR_SLICE_NO_END;
      } else {
        const uint64_t T = (uint64_t)t.q_last + r.out_len;
        const bool append = t.has_rule && (uint32_t)(T & 1) != (uint32_t)(t.length_parity & 1);
        if (T + (append ? 1 : 0) != t.size) st = AVR_SLICE_NO_END;
        else if (t.has_rule && t.final_pos != AVR_RANGE_NO_POS) out[t.final_pos] = t.last_byte;
      }
    }
    status[k] = st;
    failed |= st != 0;
  }
  return failed ? AVR_ERR_FORMAT : AVR_OK;
}

// What check_units_kernel (avr_k_check.hip) does, on host buffers: the CPU tests' reference for it, and
// what tests/native/unit_check.cpp drives under sanitizers.  The last-byte rule goes onto the value
// with fold_file_crc's arithmetic (avr_host.cpp).
int avr_unit_checks_apply(const avr_range_tail* tails, const avr_unit_check* checks, const avr_slice_result* res, int n,
                          const uint8_t* src, size_t src_len, int32_t* status) {
  if (n < 0 || (n && (!tails || !checks || !res || !status))) return AVR_ERR_INVALID_ARGUMENT;
  bool mismatch = false, outside = false;
  for (int k = 0; k < n; k++) {
    const avr_range_tail& t = tails[k];
    const avr_unit_check& ck = checks[k];
    if (status[k] != 0 || res[k].status != 0 || !ck.have) continue;
    const uint32_t out_len = res[k].out_len;
    uint32_t len = out_len;
    LastByte rule = LastByte::kKeep;
    if (t.keep != UINT32_MAX) {
      len = t.keep;   // a piece that is not its slice's last: its share, even when it regenerated more
    } else if (t.has_rule) {
      const uint64_t T = (uint64_t)t.q_last + out_len;
      rule = (uint32_t)(T & 1) != (uint32_t)(t.length_parity & 1) ? LastByte::kAppend
             : len                                                ? LastByte::kReplace
                                                                  : LastByte::kKeep;
    }
    if (ck.src_off > src_len || len > src_len - ck.src_off || (len && !src)) {
      status[k] = AVR_SLICE_OVERFLOW;
      outside = true;
      continue;
    }
    uint32_t crc = len ? avr_crc32(0, src + ck.src_off, len) : 0;
    if (rule == LastByte::kAppend) {
      crc = avr_crc32(crc, &t.last_byte, 1);
    } else if (rule == LastByte::kReplace) {
      uint32_t e = (uint32_t)(src[ck.src_off + len - 1] ^ t.last_byte);   // the raw byte table's entry
      for (int i = 0; i < 8; i++) e = (e >> 1) ^ (0xEDB88320u & (0u - (e & 1)));
      crc ^= e;
    }
    if (crc != ck.crc) {
      status[k] = AVR_SLICE_CHECKSUM;
      mismatch = true;
    }
  }
  return mismatch ? AVR_ERR_CHECKSUM : outside ? AVR_ERR_FORMAT : AVR_OK;
}

int avr_dec_plan_unit_crcs(const avr_dec_plan* h, int unit_lo, int unit_hi, avr_unit_check* out) {
  if (!h || !h->avrc || !h->pieces || unit_lo < 0 || unit_hi < unit_lo || (size_t)unit_hi > h->units.size() ||
      (unit_hi > unit_lo && !out) || h->unit_first.size() != h->job.blocks.size() + 1)
    return AVR_ERR_INVALID_ARGUMENT;
  const std::vector<avr::PbBlock>& bl = h->job.blocks;
  size_t i = 0;
  for (int u = unit_lo; u < unit_hi; u++) {
    while (i < bl.size() && h->unit_first[i + 1] <= u) i++;
    if (i >= bl.size()) return AVR_ERR_FORMAT;
    const size_t at = (size_t)(u - h->unit_first[i]);
    const bool have = h->job.unit_checked(i) && 4 * (at + 1) <= bl[i].unit_crcs.size();
    out[u - unit_lo].crc = have ? bl[i].unit_crc(at) : 0u;
    out[u - unit_lo].have = have ? 1u : 0u;
  }
  return AVR_OK;
}

int avr_dec_plan_new(avr_dec_plan** out) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    *out = new avr_dec_plan();
    return AVR_OK;
  });
}

void avr_dec_plan_free(avr_dec_plan* h) { delete h; }

int avr_dec_plan_load(avr_dec_plan* h, const uint8_t* avrc, size_t n, int* n_slices, size_t* arena_len,
                      size_t* work_len, int* max_mb_width, int* max_mb_height) {
  if (!h || !avrc || !n_slices || !arena_len || !work_len || !max_mb_width || !max_mb_height)
    return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    h->reset();
    if (int r = decompress_setup(nullptr, avrc, n, &h->job, &h->plan)) return r;
    uint64_t w = 0;
    int mh = 1;
    for (auto& d : h->plan.descs) {
      place_output(&d, &w);
      mh = std::max(mh, d.mb_height);
    }
    map_blocks(h);
    h->avrc = avrc;
    h->n = n;
    h->work = w;
    h->max_h = mh;
    *n_slices = (int)h->plan.descs.size();
    *arena_len = h->plan.arena_end + 16;
    *work_len = w;
    *max_mb_width = h->plan.max_w;
    *max_mb_height = mh;
    return AVR_OK;
  });
}

// A piece plan: decompress_setup with a split plan (every check of the whole-file decompress on a
// seams field), then the units laid out in container order -- a whole slice as avr_dec_plan_load
// lays it out, a split slice's pieces one after the other, each stream copied straight from its
// span of Block.cabac -- and plan.descs rebuilt as the coded slices, split ones included, for the
// splice.
int avr_dec_plan_load_pieces(avr_dec_plan* h, const uint8_t* avrc, size_t n, int* n_slices, int* n_units,
                             size_t* arena_len, size_t* work_len, int* max_mb_width, int* max_mb_height, int* n_recs,
                             size_t* rec_stride) {
  if (!h || !avrc || !n_slices || !n_units || !arena_len || !work_len || !max_mb_width || !max_mb_height || !n_recs ||
      !rec_stride)
    return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    h->reset();
    SplitPlan sp;
    if (int r = decompress_setup(nullptr, avrc, n, &h->job, &h->plan, &sp)) return r;
    // units for slice- and piece-range sharding: the parallel models only, as avr_plan_decompress
    if (!h->job.parallel) return AVR_ERR_UNSUPPORTED;
    DecJob& j = h->job;
    std::vector<avr_slice_desc> slices;
    std::vector<avr::PbCopy> copies;
    uint64_t at = 0, work = 0, swork = 0;
    int mw = std::max(h->plan.max_w, sp.plan.max_w), mh = 1;
    auto unit = [&](avr_slice_desc d, const uint8_t* src, size_t len, const avr_piece& p) {
      d.payload_offset = (at + 15) & ~(uint64_t)15;
      copies.push_back({(size_t)d.payload_offset, src, len});
      at = d.payload_offset + len + 16;
      place_output(&d, &work);
      mh = std::max(mh, d.mb_height);
      h->units.push_back(d);
      h->unit_pieces.push_back(p);
    };
    h->unit_first.assign(j.blocks.size() + 1, 0);
    for (size_t i = 0; i < j.blocks.size(); i++) {
      const avr::PbBlock& b = j.blocks[i];
      const int k = j.desc_of_block[i];
      h->unit_first[i] = (int)h->units.size();
      if (!b.has_cabac || k == -1) continue;
      const int s = (int)slices.size();
      const size_t u0 = h->units.size();
      avr_slice_desc sd;
      if (k >= 0) {
        sd = h->plan.descs[k];
        unit(sd, b.cabac, b.cabac_len, avr_piece{-1, 0, s, UINT32_MAX});
        h->unit_q0.push_back(0);
      } else {
        const SplitBlock& x = j.splits[-2 - k];
        sd = sp.plan.descs[x.first];
        sd.payload_size = sd.read_limit = (uint32_t)b.cabac_len;
        sd.out_capacity = (uint32_t)(b.size + 64);
        size_t off = 0;
        for (int p = 0; p < x.pieces; p++) {
          const avr_slice_desc& pd = sp.plan.descs[x.first + p];
          const avr::PieceCtl& pc = sp.ctl[x.first + p];
          const uint32_t keep = p + 1 < x.pieces ? x.q[p] - (p ? x.q[p - 1] : 0u) : UINT32_MAX;
          // the plan's records say where their piece's bytes start in the slice (the kernels do not read it)
          if (pc.seam >= 0) ((avr::SeamRec*)(sp.recs.data() + (size_t)pc.seam * sp.stride))->q = x.q[p - 1];
          unit(pd, b.cabac + off, pd.payload_size, avr_piece{pc.seam, pc.n_mbs, s, keep});
          h->unit_q0.push_back(p ? x.q[p - 1] : 0u);
          off += pd.payload_size;
        }
      }
      sd.payload_offset = h->units[u0].payload_offset;
      place_output(&sd, &swork);
      j.desc_of_block[i] = s;
      slices.push_back(sd);
    }
    h->unit_first[j.blocks.size()] = (int)h->units.size();
    map_blocks(h);
    j.splits.clear();
    h->plan.descs = std::move(slices);
    h->plan.arena_copies = std::move(copies);
    h->plan.arena_end = at;
    h->plan.max_w = mw;
    h->recs = std::move(sp.recs);
    h->rec_stride = sp.stride;
    h->pieces = true;
    h->avrc = avrc;
    h->n = n;
    h->work = work;
    h->max_h = mh;
    *n_slices = (int)h->plan.descs.size();
    *n_units = (int)h->units.size();
    *arena_len = h->plan.arena_end + 16;
    *work_len = work;
    *max_mb_width = mw;
    *max_mb_height = mh;
    *n_recs = (int)(h->recs.size() / h->rec_stride);
    *rec_stride = h->rec_stride;
    return AVR_OK;
  });
}

int avr_dec_plan_units(const avr_dec_plan* h, avr_slice_desc* descs, avr_piece* pieces) {
  if (!h || !h->avrc || !h->pieces || ((!descs || !pieces) && !h->units.empty())) return AVR_ERR_INVALID_ARGUMENT;
  if (!h->units.empty()) {
    memcpy(descs, h->units.data(), sizeof(avr_slice_desc) * h->units.size());
    memcpy(pieces, h->unit_pieces.data(), sizeof(avr_piece) * h->unit_pieces.size());
  }
  return AVR_OK;
}

int avr_dec_plan_recs(const avr_dec_plan* h, uint8_t* out, size_t cap) {
  if (!h || !h->avrc || !h->pieces || cap < h->recs.size() || (!out && !h->recs.empty())) return AVR_ERR_INVALID_ARGUMENT;
  if (!h->recs.empty()) memcpy(out, h->recs.data(), h->recs.size());
  return AVR_OK;
}

int avr_dec_plan_descs(const avr_dec_plan* h, avr_slice_desc* out) {
  if (!h || !h->avrc || (!out && !h->plan.descs.empty())) return AVR_ERR_INVALID_ARGUMENT;
  if (!h->plan.descs.empty()) memcpy(out, h->plan.descs.data(), sizeof(avr_slice_desc) * h->plan.descs.size());
  return AVR_OK;
}

int avr_dec_plan_arena(const avr_dec_plan* h, uint8_t* out, size_t cap) {
  if (!h || !h->avrc || !out || cap < h->plan.arena_end + 16) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    zero_gaps(h->plan.arena_copies, out, 0, h->plan.arena_end + 16);
    parallel_copies(h->plan.arena_copies, out);
    return AVR_OK;
  });
}

int avr_dec_plan_splice(const avr_dec_plan* h, const int32_t* status, const uint8_t* regen, size_t regen_len,
                        const uint64_t* offsets, const uint32_t* lens, uint8_t* out, size_t out_cap, size_t* out_len) {
  return avr_dec_plan_splice_crc(h, status, regen, regen_len, offsets, lens, nullptr, out, out_cap, out_len);
}

int avr_dec_plan_splice_crc(const avr_dec_plan* h, const int32_t* status, const uint8_t* regen, size_t regen_len,
                            const uint64_t* offsets, const uint32_t* lens, const uint32_t* crcs, uint8_t* out,
                            size_t out_cap, size_t* out_len) {
  const int ns = h ? (int)h->plan.descs.size() : 0;
  if (!h || !h->avrc || !out_len || (ns && (!status || !regen || !offsets || !lens))) return AVR_ERR_INVALID_ARGUMENT;
  *out_len = 0;
  return guarded(nullptr, [&]() -> int {
    std::vector<avr::PbCopy> copies;
    std::vector<std::pair<size_t, uint8_t>> patches;
    std::vector<std::vector<uint8_t>> side;
    size_t total = 0;
    if (int r = splice_layout(h, status, regen, regen_len, offsets, lens, &copies, &patches, &side, &total, crcs)) return r;
    *out_len = total;
    if (total > out_cap || (total && !out)) return AVR_ERR_INVALID_ARGUMENT;
    write_splice(copies, patches, out);
    return AVR_OK;
  });
}

int avr_plan_decompress(const uint8_t* avrc, size_t n, avr_slice_desc** descs, int* n_slices, uint8_t** arena,
                        size_t* arena_len, size_t* work_len, int* max_mb_width, int* max_mb_height) {
  if (!avrc || !descs || !n_slices || !arena || !arena_len || !work_len || !max_mb_width || !max_mb_height)
    return AVR_ERR_INVALID_ARGUMENT;
  *descs = nullptr;
  *arena = nullptr;
  return guarded(nullptr, [&]() -> int {
    avr_dec_plan h;
    int ns = 0;
    size_t al = 0;
    if (int r = avr_dec_plan_load(&h, avrc, n, &ns, &al, work_len, max_mb_width, max_mb_height)) return r;
    // a slice batch for slice-range sharding: the parallel models only (the reference model's
    // slices chain; the chained model shards by chains, avr_decompress_chain_range)
    if (!h.job.parallel) return AVR_ERR_UNSUPPORTED;
    *descs = (avr_slice_desc*)malloc(sizeof(avr_slice_desc) * std::max(1, ns));
    *arena = host_alloc(al);
    if (!*descs || !*arena) {
      free(*descs);
      free(*arena);
      *descs = nullptr;
      *arena = nullptr;
      return AVR_ERR_OUT_OF_MEMORY;
    }
    avr_dec_plan_descs(&h, *descs);
    if (int r = avr_dec_plan_arena(&h, *arena, al)) return r;
    *n_slices = ns;
    *arena_len = al;
    return AVR_OK;
  });
}

int avr_splice_container(const uint8_t* avrc, size_t n, int n_slices, const int32_t* status, const uint8_t* regen,
                         size_t regen_len, const uint64_t* offsets, const uint32_t* lens, uint8_t** out,
                         size_t* out_len) {
  if (!avrc || n_slices < 0 || (n_slices && (!status || !regen || !offsets || !lens)) || !out || !out_len)
    return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(nullptr, [&]() -> int {
    avr_dec_plan h;
    int ns = 0, mw = 0, mh = 0;
    size_t al = 0, wl = 0;
    if (int r = avr_dec_plan_load(&h, avrc, n, &ns, &al, &wl, &mw, &mh)) return r;
    if (ns != n_slices) return AVR_ERR_INVALID_ARGUMENT;
    std::vector<avr::PbCopy> copies;
    std::vector<std::pair<size_t, uint8_t>> patches;
    std::vector<std::vector<uint8_t>> side;
    size_t total = 0;
    if (int r = splice_layout(&h, status, regen, regen_len, offsets, lens, &copies, &patches, &side, &total)) return r;
    uint8_t* o = host_alloc(total);
    if (!o) return AVR_ERR_OUT_OF_MEMORY;
    write_splice(copies, patches, o);
    *out = o;
    *out_len = total;
    return AVR_OK;
  });
}

int avr_container_model(const uint8_t* avrc, size_t n, int* model) {
  if (!avrc || !model) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    std::vector<avr::PbBlock> blocks;
    std::string version;
    if (!avr::pb_parse(avrc, n, &blocks, &version)) return AVR_ERR_FORMAT;
    const int m = avr::model_of_version(version);
    if (m < 0) return AVR_ERR_FORMAT;
    *model = m;
    return AVR_OK;
  });
}

}  // extern "C"
