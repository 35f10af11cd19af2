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

int decompress_setup(ErrSink* c, const uint8_t* in, size_t n, DecJob* j, Plan* plan, SplitPlan* sp) {
  const bool tm = getenv("AVR_ASM_TIMING") != nullptr;
  double t0 = now_s();
  std::string version;
  avr::PbFileCrc fc;
  if (!avr::pb_parse(in, n, &j->blocks, &version, nullptr, &fc)) return fail(c, AVR_ERR_FORMAT, "not a Recoded protobuf");
  j->has_crc = fc.present;
  j->file_crc = fc.value;
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
// decompressor::run (recode.cpp:1338-1409) cut in two around the device work: load = read_packet's
// surrogate stream parsed and matched to the container's coded blocks (decompress_setup in layout
// mode: descs and the arena layout, no bytes copied), then the arena written where the caller wants
// it, and the splice of the regenerated slices with the literals and the last-byte patch
// (recode.cpp:1345-1356).  A handle keeps its scratch (the surrogate stream) for the next load.
struct avr_dec_plan {
  DecJob job;
  Plan plan;
  uint64_t work = 0;
  int max_h = 1;
  const uint8_t* avrc = nullptr;   // the caller's container (the blocks point into it)
  size_t n = 0;
  // a piece plan (avr_dec_plan_load_pieces): plan.descs = the coded slices (a split slice once, the
  // splice's indexing), units = what one workgroup regenerates, in container order; plan's arena
  // layout is the units'
  bool pieces = false;
  std::vector<avr_slice_desc> units;
  std::vector<avr_piece> unit_pieces;
  Bytes recs;                      // the seam records, rec_stride apart
  size_t rec_stride = 0;
  void reset() {
    avrc = nullptr;
    pieces = false;
    job.blocks.clear();
    job.desc_of_block.clear();
    job.splits.clear();
    job.stream.clear();   // keeps its capacity: the next stream is written over mapped pages
    plan.descs.clear();
    plan.arena_copies.clear();
    plan.arena_end = 0;
    plan.max_w = 1;
    plan.layout_only = true;
    units.clear();
    unit_pieces.clear();
    recs.clear();
  }
};

namespace {

// splice_job's output laid out: the literal and regenerated-slice copies, the last-byte patches
// (position, byte) and the total length.  An escaped block (field 17) is one more copy job: its
// bytes -- regenerated, patched, then escaped -- stand in `side`, which the layout's caller keeps
// until the copies are done.
// A checked container (job.has_crc) is checked here, before anything is written: the fold of the
// blocks' CRCs (fold_file_crc) -- the slices' from crcs, or without them from regen on host threads --
// against the container's value, AVR_ERR_CHECKSUM when they differ.
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
  if (j.has_crc) items.reserve(j.blocks.size());
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
      at += side->back().size();
      continue;
    }
    if (len) copies->push_back({at, regen + offsets[k], len});
    if (j.has_crc) items.push_back(crc_item_of_slice(b, regen + offsets[k], len, crcs ? &crcs[k] : nullptr));
    const LastByte rule = last_byte_rule(b, len);
    const size_t m = len + (rule == LastByte::kAppend);
    if (rule != LastByte::kKeep) patches->push_back({at + m - 1, (uint8_t)b.last_byte[0]});
    at += m;
  }
  *total = at;
  if (j.has_crc && fold_file_crc(&items) != j.file_crc) return AVR_ERR_CHECKSUM;
  return AVR_OK;
}

// a splice written out: the copies on host threads, then the last-byte patches
void write_splice(const std::vector<avr::PbCopy>& copies, const std::vector<std::pair<size_t, uint8_t>>& patches,
                  uint8_t* out) {
  parallel_copies(copies, out);
  for (const auto& pt : patches) out[pt.first] = pt.second;
}

}  // namespace

extern "C" {

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
    for (size_t i = 0; i < j.blocks.size(); i++) {
      const avr::PbBlock& b = j.blocks[i];
      const int k = j.desc_of_block[i];
      if (!b.has_cabac || k == -1) continue;
      const int s = (int)slices.size();
      const size_t u0 = h->units.size();
      avr_slice_desc sd;
      if (k >= 0) {
        sd = h->plan.descs[k];
        unit(sd, b.cabac, b.cabac_len, avr_piece{-1, 0, s, UINT32_MAX});
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
          off += pd.payload_size;
        }
      }
      sd.payload_offset = h->units[u0].payload_offset;
      place_output(&sd, &swork);
      j.desc_of_block[i] = s;
      slices.push_back(sd);
    }
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
