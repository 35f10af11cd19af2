// Host-only mutation harness for the decompress planner and the seams codec (avr_plan.cpp,
// avr_seams.cpp over avr_host.cpp and avr_front.cpp), built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_plan_sanitizers.py: g++ alone, no ROCm include path, no
// HIP library.  That it links is the proof that these translation units need no device; every
// sharded decompress runs them first, on container bytes it does not control.
//
//   plan_fuzz <iterations> <seed> <spec>...
//     plain:<path>                   a parallel-model container without seams
//     split:<slices>:<units>:<path>  one whose long slices are cut (coded slices, units expected)
//     ref:<path>                     a reference-model container
//
// Through the public ABI (include/avrecode.h) only.  The unmutated containers first: the plain ones
// load as slice plans and as piece plans, the split ones are refused as slice plans
// (AVR_ERR_UNSUPPORTED) and load as piece plans with the expected counts, the reference one is refused
// as a piece plan; every accessor fills a buffer of exactly the reported size, and a splice whose
// statuses all say "failed" returns AVR_ERR_FORMAT.  Then two kinds of mutation:
//   - bytes: front_fuzz's mutations of the whole container (most die in the protobuf reader or zlib);
//   - seams: one block's seams field inflated, its raw bytes mutated -- the counts, a cut's
//     first_mb, q, last_dqp_nz or ce_*, a piece length, a context state set to 0x80 or above, a
//     truncation -- deflated again and the container rewritten with pb_put_block: this is what
//     reaches seams_decode's checks and the piece plan's layout.
// Every call must return AVR_OK or a documented error, and an accepted plan must describe bytes
// inside the buffers it reports.  Exit status 0 = no sanitizer report and no broken invariant.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../../avrecode_amd/csrc/avr_front.h"
#include "../../include/avrecode.h"

namespace {

typedef std::vector<uint8_t> Buf;

Buf read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return Buf(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// front_fuzz's byte mutations (tests/native/front_fuzz.cpp)
void mutate_bytes(Buf* d, std::mt19937_64& rng) {
  const int n = 1 + (int)(rng() % 8);
  for (int k = 0; k < n && !d->empty(); k++) {
    const size_t at = rng() % d->size();
    switch (rng() % 6) {
      case 0: (*d)[at] ^= (uint8_t)(1u << (rng() % 8)); break;
      case 1: {
        static const uint8_t v[] = {0x00, 0x01, 0x7f, 0x80, 0xff};
        (*d)[at] = v[rng() % 5];
        break;
      }
      case 2: d->resize(at); break;
      case 3: {
        static const uint32_t v[] = {0u, 1u, 7u, 8u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
        const uint32_t x = v[rng() % 7];
        for (int b = 0; b < 4 && at + b < d->size(); b++) (*d)[at + b] = (uint8_t)(x >> (24 - 8 * b));
        break;
      }
      case 4: {
        const size_t len = std::min<size_t>(1 + rng() % 64, d->size() - at);
        Buf span(d->begin() + at, d->begin() + at + len);
        d->insert(d->begin() + at, span.begin(), span.end());
        break;
      }
      default: {
        static const uint8_t sc[] = {0, 0, 1};
        d->insert(d->begin() + at, sc, sc + 3);
        break;
      }
    }
  }
}

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void put32(uint8_t* p, uint32_t v) {
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// The raw bytes of a seams field (the layout at avr_seams.cpp's seams_encode): { u32 2, cuts, mb_width,
// u32 piece_len[cuts + 1], per cut 8 u32 + 1024 state bytes + 40 mb_width edge bytes }.  1-3 mutations.
void mutate_seams_raw(Buf* raw, std::mt19937_64& rng) {
  if (raw->size() < 12) return;
  const uint32_t k = le32(raw->data() + 4), w = le32(raw->data() + 8);
  const size_t per = 32 + 1024 + (size_t)40 * w, cuts0 = 12 + 4 * ((size_t)k + 1);
  const bool whole = k > 0 && k < 65536 && cuts0 + per * k == raw->size();
  auto u32_value = [&](uint32_t old) -> uint32_t {
    static const uint32_t v[] = {0u, 1u, 0xffu, 0x100u, 510u, 511u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    switch (rng() % 5) {
      case 0: return old + 1;
      case 1: return old - 1;
      case 2: return old + w;
      case 3: return (uint32_t)rng();
      default: return v[rng() % 9];
    }
  };
  const int n = 1 + (int)(rng() % 3);
  for (int m = 0; m < n && raw->size() >= 12; m++) {
    const unsigned what = (unsigned)(rng() % 8);
    if (what == 0) {   // the tag, the cut count or the width
      uint8_t* p = raw->data() + 4 * (rng() % 3);
      put32(p, u32_value(le32(p)));
    } else if (what == 1) {   // a truncation (or a few bytes more)
      if (rng() % 4) raw->resize(rng() % raw->size());
      else raw->insert(raw->end(), 1 + rng() % 64, (uint8_t)rng());
    } else if (!whole) {
      (*raw)[rng() % raw->size()] = (uint8_t)rng();
    } else if (what == 2) {   // a piece length
      uint8_t* p = raw->data() + 12 + 4 * (rng() % (k + 1));
      put32(p, u32_value(le32(p)));
    } else if (what == 3) {   // a context state of 0x80 or above (stored XOR the initial state, itself < 0x80)
      (*raw)[cuts0 + per * (rng() % k) + 32 + rng() % 1024] = (uint8_t)(0x80 | rng());
    } else if (what == 4) {   // an edge byte
      if (w) (*raw)[cuts0 + per * (rng() % k) + 32 + 1024 + rng() % ((size_t)40 * w)] = (uint8_t)rng();
    } else {   // first_mb, q, last_dqp_nz, ce_low, ce_queue, ce_outstanding, ce_cache, ce_range
      uint8_t* p = raw->data() + cuts0 + per * (rng() % k) + 4 * (rng() % 8);
      put32(p, u32_value(le32(p)));
    }
  }
}

// The container with block `which`'s seams field (u32 raw length, zlib) replaced by `raw` deflated;
// lie: the length written differs from raw's.
bool with_seams(const Buf& avrc, size_t which, const Buf& raw, int lie, Buf* out) {
  std::vector<avr::PbBlock> blocks;
  std::string version;
  bool has_md = false;
  if (!avr::pb_parse(avrc.data(), avrc.size(), &blocks, &version, &has_md) || which >= blocks.size()) return false;
  uLongf zl = compressBound(raw.size());
  Buf field(4 + zl);
  if (compress2(field.data() + 4, &zl, raw.data(), raw.size(), 1) != Z_OK) return false;
  field.resize(4 + zl);
  put32(field.data(), (uint32_t)raw.size() + (uint32_t)lie);
  blocks[which].seams = field.data();
  blocks[which].seams_len = field.size();
  out->clear();
  if (has_md) avr::pb_put_metadata_version(out, version);
  for (const avr::PbBlock& b : blocks) avr::pb_put_block(out, b);
  return true;
}

// the blocks of a container that carry a seams field, each with the field's raw bytes
struct SeamsField {
  size_t block;
  Buf raw;
};
std::vector<SeamsField> seams_fields(const Buf& avrc) {
  std::vector<SeamsField> f;
  std::vector<avr::PbBlock> blocks;
  std::string version;
  if (!avr::pb_parse(avrc.data(), avrc.size(), &blocks, &version)) return f;
  for (size_t i = 0; i < blocks.size(); i++) {
    const avr::PbBlock& b = blocks[i];
    if (!b.has_seams || b.seams_len < 4) continue;
    Buf raw(le32(b.seams));
    uLongf got = raw.size();
    if (uncompress(raw.data(), &got, b.seams + 4, b.seams_len - 4) == Z_OK && got == raw.size()) f.push_back({i, raw});
  }
  return f;
}

// a container whose blocks claim more than this many stream bytes would only time the surrogate fill
constexpr int64_t kMaxStreamBytes = (int64_t)64 << 20;
bool too_large(const Buf& d) {
  std::vector<avr::PbBlock> blocks;
  std::string version;
  if (!avr::pb_parse(d.data(), d.size(), &blocks, &version)) return false;
  int64_t total = 0;
  for (const avr::PbBlock& b : blocks) total += b.has_cabac && b.size > 0 ? b.size : 0;
  return total > kMaxStreamBytes;
}

bool documented(int r) {
  return r == AVR_OK || r == AVR_ERR_INVALID_ARGUMENT || r == AVR_ERR_FORMAT || r == AVR_ERR_OUT_OF_MEMORY ||
         r == AVR_ERR_UNSUPPORTED;
}
#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

struct Sizes {
  int n_slices = 0, n_units = 0, max_w = 0, max_h = 0, n_recs = 0;
  size_t arena_len = 0, work_len = 0, rec_stride = 0;
};

// An accepted plan: every accessor into a buffer of exactly the reported size (the sanitizer sees a
// byte written past it), the descriptors inside the arena and the work buffer, and the two splices.
// pristine: the container is an unmutated one, so it has coded slices and the failed splice must say so.
int exercise(const avr_dec_plan* h, bool pieces, const Sizes& z, bool pristine) {
  REQUIRE(z.n_slices >= 0 && z.n_units >= 0 && z.n_recs >= 0 && z.arena_len >= 16, "plan: negative counts");
  std::vector<avr_slice_desc> descs((size_t)z.n_slices);
  int r = avr_dec_plan_descs(h, descs.data());
  REQUIRE(r == AVR_OK, "avr_dec_plan_descs: %d", r);
  Buf arena(z.arena_len);
  r = avr_dec_plan_arena(h, arena.data(), arena.size());
  REQUIRE(r == AVR_OK, "avr_dec_plan_arena: %d", r);
  std::vector<avr_slice_desc> units;
  if (pieces) {
    units.resize((size_t)z.n_units);
    std::vector<avr_piece> pc((size_t)z.n_units);
    r = avr_dec_plan_units(h, units.data(), pc.data());
    REQUIRE(r == AVR_OK, "avr_dec_plan_units: %d", r);
    // n_recs * rec_stride is what avr_dec_plan_recs writes: it fits exactly, and one byte less is refused
    const size_t rb = (size_t)z.n_recs * z.rec_stride;
    Buf recs(rb);
    r = avr_dec_plan_recs(h, recs.data(), rb);
    REQUIRE(r == AVR_OK, "avr_dec_plan_recs(%zu): %d", rb, r);
    if (rb) {
      r = avr_dec_plan_recs(h, recs.data(), rb - 1);
      REQUIRE(r == AVR_ERR_INVALID_ARGUMENT, "avr_dec_plan_recs(%zu) with %zu bytes of records: %d", rb - 1, rb, r);
    }
    for (int k = 0; k < z.n_units; k++)
      REQUIRE(pc[k].seam >= -1 && pc[k].seam < z.n_recs && pc[k].slice >= 0 && pc[k].slice < z.n_slices,
              "unit %d: seam %d of %d records, slice %d of %d", k, pc[k].seam, z.n_recs, pc[k].slice, z.n_slices);
  } else {
    units = descs;
  }
  for (size_t k = 0; k < units.size(); k++) {
    const avr_slice_desc& d = units[k];
    if (!d.coded) continue;   // a reference-model plan lists uncoded slices too: no stream, no output
    REQUIRE(d.payload_offset <= z.arena_len && d.payload_size <= z.arena_len - d.payload_offset,
            "unit %zu: stream [%llu, +%u) outside an arena of %zu", k, (unsigned long long)d.payload_offset,
            d.payload_size, z.arena_len);
    REQUIRE(d.out_offset <= z.work_len && d.out_capacity <= z.work_len - d.out_offset,
            "unit %zu: output [%llu, +%u) outside a work buffer of %zu", k, (unsigned long long)d.out_offset,
            d.out_capacity, z.work_len);
  }
  // the splice: every slice failed, then every slice regenerated as zero bytes
  const size_t ns = (size_t)z.n_slices;
  std::vector<int32_t> status(ns, AVR_SLICE_OVERREAD);
  std::vector<uint64_t> offsets(ns, 0);
  std::vector<uint32_t> lens(ns, 0);
  const Buf regen(16, 0);
  size_t out_len = 0;
  r = avr_dec_plan_splice(h, status.data(), regen.data(), regen.size(), offsets.data(), lens.data(), nullptr, 0, &out_len);
  REQUIRE(documented(r) && (!pristine || r == AVR_ERR_FORMAT), "avr_dec_plan_splice of failed slices: %d", r);
  std::fill(status.begin(), status.end(), 0);
  r = avr_dec_plan_splice(h, status.data(), regen.data(), regen.size(), offsets.data(), lens.data(), nullptr, 0, &out_len);
  REQUIRE(documented(r), "avr_dec_plan_splice sizing: %d", r);
  if (r == AVR_ERR_INVALID_ARGUMENT && out_len) {
    Buf out(out_len);
    size_t len2 = 0;
    r = avr_dec_plan_splice(h, status.data(), regen.data(), regen.size(), offsets.data(), lens.data(), out.data(),
                            out.size(), &len2);
    REQUIRE(r == AVR_OK && len2 == out_len, "avr_dec_plan_splice into %zu bytes: %d, %zu", out_len, r, len2);
  }
  return 0;
}

long g_slice_plans = 0, g_piece_plans = 0;   // loads accepted so far

struct Expect {
  int slice_plan, piece_plan;   // the two loads' results
  int n_slices, n_units;        // of the piece plan (-1: not pinned)
};

// Both loads of one container and, for what they accept, exercise(); e: an unmutated container.
int check(const Buf& d, const Expect* e) {
  avr_dec_plan* h = nullptr;
  REQUIRE(avr_dec_plan_new(&h) == AVR_OK && h, "avr_dec_plan_new");
  int rc = 0, model = -1;
  const int rm = avr_container_model(d.data(), d.size(), &model);
  Sizes z;
  const int r1 = avr_dec_plan_load(h, d.data(), d.size(), &z.n_slices, &z.arena_len, &z.work_len, &z.max_w, &z.max_h);
  if (!documented(rm) || !documented(r1) || (e && r1 != e->slice_plan)) {
    fprintf(stderr, "avr_container_model: %d, avr_dec_plan_load: %d\n", rm, r1);
    rc = 1;
  }
  g_slice_plans += r1 == AVR_OK;
  if (!rc && r1 == AVR_OK) rc = exercise(h, false, z, e != nullptr);
  if (!rc) {
    z = Sizes();
    const int r2 = avr_dec_plan_load_pieces(h, d.data(), d.size(), &z.n_slices, &z.n_units, &z.arena_len, &z.work_len,
                                            &z.max_w, &z.max_h, &z.n_recs, &z.rec_stride);
    if (!documented(r2) || (e && r2 != e->piece_plan)) {
      fprintf(stderr, "avr_dec_plan_load_pieces: %d\n", r2);
      rc = 1;
    } else if (r2 == AVR_OK) {
      g_piece_plans++;
      if (e && e->n_slices >= 0 && (z.n_slices != e->n_slices || z.n_units != e->n_units)) {
        fprintf(stderr, "piece plan: %d slices, %d units; expected %d, %d\n", z.n_slices, z.n_units, e->n_slices,
                e->n_units);
        rc = 1;
      } else {
        rc = exercise(h, true, z, e != nullptr);
      }
    }
  }
  avr_dec_plan_free(h);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <iterations> <seed> plain:<path> | split:<slices>:<units>:<path> | ref:<path> ...\n", argv[0]);
    return 2;
  }
  const long iters = strtol(argv[1], nullptr, 10);
  std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
  std::vector<Buf> inputs;
  std::vector<std::pair<size_t, SeamsField>> fields;   // (input, one of its seams fields)
  for (int i = 3; i < argc; i++) {
    const std::string spec = argv[i];
    Expect e{AVR_OK, AVR_OK, -1, -1};
    size_t path = spec.find(':') + 1;
    if (spec.compare(0, 6, "split:") == 0) {
      char* end = nullptr;
      e.slice_plan = AVR_ERR_UNSUPPORTED;
      e.n_slices = (int)strtol(spec.c_str() + 6, &end, 10);
      e.n_units = (int)strtol(end + 1, &end, 10);
      path = (size_t)(end + 1 - spec.c_str());
    } else if (spec.compare(0, 4, "ref:") == 0) {
      e.piece_plan = AVR_ERR_UNSUPPORTED;
    } else if (spec.compare(0, 6, "plain:") != 0) {
      fprintf(stderr, "bad spec %s\n", argv[i]);
      return 2;
    }
    inputs.push_back(read_file(spec.c_str() + path));
    const Buf& in = inputs.back();
    if (in.empty()) {
      fprintf(stderr, "cannot read %s\n", spec.c_str() + path);
      return 2;
    }
    if (check(in, &e)) {
      fprintf(stderr, "unmutated %s\n", argv[i]);
      return 1;
    }
    const std::vector<SeamsField> sf = seams_fields(in);
    if ((e.slice_plan == AVR_ERR_UNSUPPORTED) != !sf.empty()) {
      fprintf(stderr, "%s: %zu seams fields\n", argv[i], sf.size());
      return 1;
    }
    for (const SeamsField& f : sf) fields.push_back({inputs.size() - 1, f});
    // the rewrite itself changes nothing: a field put back as it was loads as before
    if (!sf.empty()) {
      Buf same;
      if (!with_seams(in, sf[0].block, sf[0].raw, 0, &same) || check(same, &e)) {
        fprintf(stderr, "rewritten %s\n", argv[i]);
        return 1;
      }
    }
  }
  long seams_runs = 0, skipped = 0;
  g_slice_plans = g_piece_plans = 0;
  for (long it = 0; it < iters; it++) {
    Buf d;
    if (!fields.empty() && it % 2 == 0) {
      const auto& f = fields[rng() % fields.size()];
      Buf raw = f.second.raw;
      mutate_seams_raw(&raw, rng);
      const int lie = rng() % 16 ? 0 : (int)(rng() % 3) - 1;
      if (!with_seams(inputs[f.first], f.second.block, raw, lie, &d)) {
        fprintf(stderr, "iteration %ld: cannot rewrite the container\n", it);
        return 1;
      }
      seams_runs++;
    } else {
      d = inputs[rng() % inputs.size()];
      mutate_bytes(&d, rng);
    }
    if (too_large(d)) {
      skipped++;
      continue;
    }
    if (check(d, nullptr)) {
      fprintf(stderr, "iteration %ld\n", it);
      return 1;
    }
  }
  printf("plan_fuzz: %ld mutated containers (%ld seams fields rewritten, %ld skipped as too large), %ld slice plans and "
         "%ld piece plans accepted, no finding\n", iters, seams_runs, skipped, g_slice_plans, g_piece_plans);
  return 0;
}
