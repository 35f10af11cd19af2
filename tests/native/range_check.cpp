// Host-only harness for the range planner (avr_plan.cpp: avr_dec_plan_file_size, avr_dec_plan_range,
// avr_dec_plan_range_apply), built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_range_sanitizers.py from the HIP-free sources, as plan_fuzz.cpp is: g++ alone, no device.
//
//   range_check <iterations> <seed> <container> <file> [<container> <file> ...]
//
// Through the public ABI (include/avrecode.h) only.  Every window is planned and then applied with
// buffers of exactly the sizes the plan describes -- the window, and each selected unit's share of its
// slice -- so a byte read or written outside them is a sanitizer report.
//   - The unmutated containers (parallel-model ones, with or without seams, and the files they were
//     made from): the first and the last byte, every block boundary as [b-1, b+1), [b, b+1), [b-1, b),
//     every cut likewise, the whole file, len = 0, off = size, off = size + 5, a window past the end
//     and seeded random windows.  Each is applied twice -- every unit at its full share, and every
//     slice's last unit one byte short, which the last-byte rule appends -- and must give the file's
//     bytes both times.
//   - Seeded mutations: plan_fuzz's byte mutations of the whole container, and a cut slice's seams
//     field inflated, one of its u32 fields (a q, a first_mb, a piece length, the counts) changed, and
//     deflated again.  Whatever loads is planned over random windows and applied with results of
//     random lengths: every call returns AVR_OK or a documented error.
// Exit status 0 = no sanitizer report and no broken invariant.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
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

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

bool documented(int r) {
  return r == AVR_OK || r == AVR_ERR_INVALID_ARGUMENT || r == AVR_ERR_FORMAT || r == AVR_ERR_OUT_OF_MEMORY ||
         r == AVR_ERR_UNSUPPORTED;
}

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void put32(uint8_t* p, uint32_t v) {
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// plan_fuzz's byte mutations (tests/native/plan_fuzz.cpp)
void mutate_bytes(Buf* d, std::mt19937_64& rng) {
  const int n = 1 + (int)(rng() % 8);
  for (int k = 0; k < n && !d->empty(); k++) {
    const size_t at = rng() % d->size();
    switch (rng() % 5) {
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
      default: {
        const size_t len = std::min<size_t>(1 + rng() % 64, d->size() - at);
        Buf span(d->begin() + at, d->begin() + at + len);
        d->insert(d->begin() + at, span.begin(), span.end());
        break;
      }
    }
  }
}

// The blocks that carry a seams field, each with the field's raw bytes: { u32 2, cuts, mb_width,
// u32 piece_len[cuts + 1], per cut 8 u32 (first_mb, q, ...) + 1024 state bytes + 40 mb_width edge bytes }.
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
// one u32 of the field changed: a count, a piece length, or one of a cut's first two words (first_mb, q)
void mutate_seams_raw(Buf* raw, std::mt19937_64& rng) {
  if (raw->size() < 16) return;
  const uint32_t k = le32(raw->data() + 4), w = le32(raw->data() + 8);
  const size_t per = 32 + 1024 + (size_t)40 * w, cuts0 = 12 + 4 * ((size_t)k + 1);
  uint8_t* p = raw->data() + 4 * (rng() % 3);
  if (k > 0 && k < 65536 && cuts0 + per * k == raw->size() && rng() % 8) {
    if (rng() % 3 == 0) p = raw->data() + 12 + 4 * (rng() % (k + 1));
    else p = raw->data() + cuts0 + per * (rng() % k) + 4 * (rng() % 2);
  }
  static const uint32_t v[] = {0u, 1u, 0xffu, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  const uint32_t old = le32(p);
  switch (rng() % 5) {
    case 0: put32(p, old + 1); break;
    case 1: put32(p, old - 1); break;
    case 2: put32(p, old + (uint32_t)(rng() % 4096)); break;
    case 3: put32(p, old - (uint32_t)(rng() % 4096)); break;
    default: put32(p, v[rng() % 6]); break;
  }
}
bool with_seams(const Buf& avrc, size_t which, const Buf& raw, Buf* out) {
  std::vector<avr::PbBlock> blocks;
  std::string version;
  bool has_md = false;
  if (!avr::pb_parse(avrc.data(), avrc.size(), &blocks, &version, &has_md) || which >= blocks.size()) return false;
  uLongf zl = compressBound(raw.size());
  Buf field(4 + zl);
  if (compress2(field.data() + 4, &zl, raw.data(), raw.size(), 1) != Z_OK) return false;
  field.resize(4 + zl);
  put32(field.data(), (uint32_t)raw.size());
  blocks[which].seams = field.data();
  blocks[which].seams_len = field.size();
  out->clear();
  if (has_md) avr::pb_put_metadata_version(out, version);
  for (const avr::PbBlock& b : blocks) avr::pb_put_block(out, b);
  return true;
}

constexpr int64_t kMaxStreamBytes = (int64_t)64 << 20;
bool too_large(const Buf& d) {
  std::vector<avr::PbBlock> blocks;
  std::string version;
  if (!avr::pb_parse(d.data(), d.size(), &blocks, &version)) return false;
  int64_t total = 0;
  for (const avr::PbBlock& b : blocks) total += b.has_cabac && b.size > 0 ? b.size : 0;
  return total > kMaxStreamBytes;
}

struct Plan {
  avr_dec_plan* h = nullptr;
  int n_units = 0;
  uint64_t file_size = 0;
  std::vector<avr_piece> pieces;
  ~Plan() { avr_dec_plan_free(h); }
};
// AVR_OK: a piece plan with its units' avr_piece array and the file's size
int load(const Buf& d, Plan* p) {
  if (avr_dec_plan_new(&p->h) != AVR_OK || !p->h) return AVR_ERR_OUT_OF_MEMORY;
  int ns = 0, mw = 0, mh = 0, nr = 0;
  size_t al = 0, wl = 0, rs = 0;
  if (int r = avr_dec_plan_load_pieces(p->h, d.data(), d.size(), &ns, &p->n_units, &al, &wl, &mw, &mh, &nr, &rs)) return r;
  std::vector<avr_slice_desc> descs((size_t)p->n_units);
  p->pieces.resize((size_t)p->n_units);
  if (int r = avr_dec_plan_units(p->h, descs.data(), p->pieces.data())) return r;
  return avr_dec_plan_file_size(p->h, &p->file_size);
}

struct Ranged {
  avr_range_info info{};
  avr_span* spans = nullptr;
  avr_range_tail* tails = nullptr;
  ~Ranged() {   // avr_free is free(); it lives with the device units, which this program does not link
    free(spans);
    free(tails);
  }
};

// One window of a mutated container: planned, then applied to buffers of exactly the planned sizes
// with results of random lengths.  Nothing is known about the file: only that no call misbehaves.
int blind_window(const Buf& d, const Plan& p, uint64_t off, uint64_t len, std::mt19937_64& rng) {
  Ranged g;
  const int r = avr_dec_plan_range(p.h, off, len, rng() % 4 ? 0 : 16 + (uint32_t)(rng() % 5000), &g.info, &g.spans, &g.tails);
  REQUIRE(documented(r), "avr_dec_plan_range: %d", r);
  if (r != AVR_OK) return 0;
  const int nu = g.info.unit_hi - g.info.unit_lo;
  REQUIRE(g.info.off <= p.file_size && g.info.len <= p.file_size - g.info.off && nu >= 0 && g.info.unit_lo >= 0 &&
              g.info.unit_hi <= p.n_units && g.info.n_spans >= 0,
          "range: window or units outside the plan");
  // each unit's room: what its spans reach, to the byte
  std::vector<uint64_t> room((size_t)nu, 0), unit_off((size_t)nu, 0);
  uint64_t at = 0;
  for (int k = 0; k < g.info.n_spans; k++) {
    const avr_span& s = g.spans[k];
    REQUIRE(s.dst_off == at && s.len > 0, "range: spans do not tile the window");
    at += s.len;
    if (s.source == AVR_SPAN_LITERAL) {
      REQUIRE(s.src_off <= d.size() && s.len <= d.size() - s.src_off, "range: a literal span outside the container");
    } else {
      REQUIRE(s.source >= 0 && s.source < nu, "range: a span of a unit that is not selected");
      room[(size_t)s.source] = std::max(room[(size_t)s.source], s.src_off + s.len);
    }
  }
  REQUIRE(at == g.info.len, "range: spans cover %llu of %llu bytes", (unsigned long long)at, (unsigned long long)g.info.len);
  uint64_t total = 0;
  for (int k = 0; k < nu; k++) unit_off[(size_t)k] = total, total += room[(size_t)k];
  REQUIRE(total <= ((uint64_t)1 << 32), "range: units of %llu bytes", (unsigned long long)total);
  std::unique_ptr<uint8_t[]> regen(new uint8_t[(size_t)total + 1]), out(new uint8_t[(size_t)g.info.len]);
  memset(regen.get(), 0x5a, (size_t)total);
  std::vector<avr_slice_result> res((size_t)nu);
  std::vector<int32_t> status((size_t)nu, 77);
  for (int k = 0; k < nu; k++) {
    memset(&res[(size_t)k], 0, sizeof(avr_slice_result));
    const avr_range_tail& t = g.tails[k];
    const uint32_t full = t.keep != UINT32_MAX ? t.keep : t.size - std::min(t.size, t.q_last);
    res[(size_t)k].out_len = rng() % 3 ? full : rng() % 2 ? full - 1 : (uint32_t)rng();
    res[(size_t)k].status = rng() % 16 ? 0 : AVR_SLICE_OVERREAD;
    REQUIRE(t.final_pos == AVR_RANGE_NO_POS || t.final_pos < g.info.len, "range: a final byte outside the window");
  }
  const int ra = avr_dec_plan_range_apply(g.spans, g.info.n_spans, g.tails, nu, d.data(), d.size(), regen.get(), (size_t)total,
                                          unit_off.data(), res.data(), out.get(), (size_t)g.info.len, status.data());
  REQUIRE(ra == AVR_OK || ra == AVR_ERR_FORMAT, "avr_dec_plan_range_apply: %d", ra);
  return 0;
}

// The windows of an unmutated container against the file it was made from.
int true_windows(const Buf& avrc, const Buf& file, std::mt19937_64& rng, long* n_windows) {
  Plan p;
  int r = load(avrc, &p);
  REQUIRE(r == AVR_OK, "unmutated container: load %d", r);
  REQUIRE(p.file_size == file.size(), "file_size %llu, the file has %zu bytes", (unsigned long long)p.file_size, file.size());
  std::vector<avr::PbBlock> blocks;
  std::string version;
  REQUIRE(avr::pb_parse(avrc.data(), avrc.size(), &blocks, &version), "pb_parse");
  // every unit's true span of the file: a coded block's units one after the other, each its share
  std::vector<std::pair<uint64_t, uint64_t>> span((size_t)p.n_units);
  std::vector<char> ends((size_t)p.n_units, 0);
  std::vector<uint64_t> edges;
  uint64_t pos = 0;
  int u = 0;
  for (const avr::PbBlock& b : blocks) {
    edges.push_back(pos);
    if (b.has_literal) pos += b.literal_len;
    if (!b.has_cabac) continue;
    REQUIRE(u < p.n_units, "more coded blocks than slices");
    const int s = p.pieces[(size_t)u].slice;
    uint64_t at = pos;
    for (; u < p.n_units && p.pieces[(size_t)u].slice == s; u++) {
      const bool last = p.pieces[(size_t)u].keep == UINT32_MAX;
      const uint64_t end = last ? pos + (uint64_t)b.size : at + p.pieces[(size_t)u].keep;
      if (at > pos) edges.push_back(at);
      span[(size_t)u] = {at, end};
      ends[(size_t)u] = last;
      at = end;
    }
    REQUIRE(at == pos + (uint64_t)b.size, "a slice's units do not add up to its size");
    pos += (uint64_t)b.size;
  }
  REQUIRE(u == p.n_units && pos == file.size(), "units or blocks left over");
  const uint64_t size = file.size();
  std::vector<std::pair<uint64_t, uint64_t>> w = {{0, 1}, {size - 1, 1}, {0, size}, {10, 0}, {size, 7}, {size + 5, 3}, {size - 3, 100}};
  for (uint64_t b : edges)
    if (b > 0 && b < size) w.push_back({b - 1, 2}), w.push_back({b, 1}), w.push_back({b - 1, 1});
  for (int k = 0; k < 200; k++) w.push_back({rng() % size, rng() % 4 ? 1 + rng() % 3000 : 1 + rng() % 200000});
  for (const auto& win : w) {
    const uint64_t w0 = std::min(win.first, size), w1 = std::min(win.first + win.second, size);
    Ranged g;
    r = avr_dec_plan_range(p.h, win.first, win.second, 0, &g.info, &g.spans, &g.tails);
    REQUIRE(r == AVR_OK && g.info.off == w0 && g.info.len == w1 - w0, "window %llu + %llu: %d", (unsigned long long)win.first,
            (unsigned long long)win.second, r);
    int lo = -1, hi = -1;
    for (int k = 0; k < p.n_units; k++)
      if (span[(size_t)k].first < w1 && span[(size_t)k].second > w0) lo = lo < 0 ? k : lo, hi = k + 1;
    if (w1 == w0 || lo < 0) REQUIRE(g.info.unit_lo == g.info.unit_hi, "units selected by a window that touches none");
    else REQUIRE(g.info.unit_lo == lo && g.info.unit_hi == hi, "window %llu + %llu: units [%d, %d), expected [%d, %d)",
                 (unsigned long long)win.first, (unsigned long long)win.second, g.info.unit_lo, g.info.unit_hi, lo, hi);
    const int nu = g.info.unit_hi - g.info.unit_lo;
    for (int shorten = 0; shorten < 2; shorten++) {
      // the units' true bytes, each in a buffer of its own share exactly (one less for a shortened last unit)
      std::vector<uint64_t> unit_off((size_t)nu);
      std::vector<avr_slice_result> res((size_t)nu);
      uint64_t total = 0;
      for (int k = 0; k < nu; k++) {
        const auto& sp = span[(size_t)(g.info.unit_lo + k)];
        unit_off[(size_t)k] = total;
        total += sp.second - sp.first;
      }
      std::unique_ptr<uint8_t[]> regen(new uint8_t[(size_t)total + 1]), out(new uint8_t[(size_t)(w1 - w0) + 1]);
      for (int k = 0; k < nu; k++) {
        const auto& sp = span[(size_t)(g.info.unit_lo + k)];
        memset(&res[(size_t)k], 0, sizeof(avr_slice_result));
        memcpy(regen.get() + unit_off[(size_t)k], file.data() + sp.first, (size_t)(sp.second - sp.first));
        res[(size_t)k].out_len = (uint32_t)(sp.second - sp.first);
        if (shorten && ends[(size_t)(g.info.unit_lo + k)]) {   // the rule appends the slice's last byte: withhold it
          res[(size_t)k].out_len--;
          regen[(size_t)(unit_off[(size_t)k] + res[(size_t)k].out_len)] = 0xEE;
        }
      }
      std::vector<int32_t> status((size_t)nu, 77);
      out[(size_t)(w1 - w0)] = 0xC3;
      r = avr_dec_plan_range_apply(g.spans, g.info.n_spans, g.tails, nu, avrc.data(), avrc.size(), regen.get(), (size_t)total,
                                   unit_off.data(), res.data(), out.get(), (size_t)(w1 - w0), status.data());
      REQUIRE(r == AVR_OK, "window %llu + %llu (%d): apply %d", (unsigned long long)win.first, (unsigned long long)win.second,
              shorten, r);
      REQUIRE(memcmp(out.get(), file.data() + w0, (size_t)(w1 - w0)) == 0 && out[(size_t)(w1 - w0)] == 0xC3,
              "window %llu + %llu (%d): not the file's bytes", (unsigned long long)win.first, (unsigned long long)win.second,
              shorten);
    }
    ++*n_windows;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 3) % 2) {
    fprintf(stderr, "usage: %s <iterations> <seed> <container> <file> [<container> <file> ...]\n", argv[0]);
    return 2;
  }
  const long iters = strtol(argv[1], nullptr, 10);
  std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
  std::vector<Buf> inputs;
  std::vector<std::pair<size_t, SeamsField>> fields;
  long n_windows = 0;
  for (int i = 3; i + 1 < argc; i += 2) {
    inputs.push_back(read_file(argv[i]));
    const Buf file = read_file(argv[i + 1]);
    if (inputs.back().empty() || file.empty()) {
      fprintf(stderr, "cannot read %s or %s\n", argv[i], argv[i + 1]);
      return 2;
    }
    if (true_windows(inputs.back(), file, rng, &n_windows)) {
      fprintf(stderr, "unmutated %s\n", argv[i]);
      return 1;
    }
    for (const SeamsField& f : seams_fields(inputs.back())) fields.push_back({inputs.size() - 1, f});
  }
  long planned = 0, skipped = 0;
  for (long it = 0; it < iters; it++) {
    Buf d;
    if (!fields.empty() && it % 2 == 0) {
      const auto& f = fields[rng() % fields.size()];
      Buf raw = f.second.raw;
      mutate_seams_raw(&raw, rng);
      if (!with_seams(inputs[f.first], f.second.block, raw, &d)) {
        fprintf(stderr, "iteration %ld: cannot rewrite the container\n", it);
        return 1;
      }
    } else {
      d = inputs[rng() % inputs.size()];
      mutate_bytes(&d, rng);
    }
    if (too_large(d)) {
      skipped++;
      continue;
    }
    Plan p;
    const int r = load(d, &p);
    if (!documented(r)) {
      fprintf(stderr, "iteration %ld: load %d\n", it, r);
      return 1;
    }
    if (r != AVR_OK) continue;
    planned++;
    for (int k = 0; k < 12; k++) {
      const uint64_t size = p.file_size ? p.file_size : 1;
      const uint64_t off = k == 0 ? 0 : rng() % (size + 8), len = k == 0 ? size : k == 1 ? UINT64_MAX - off : 1 + rng() % 100000;
      if (blind_window(d, p, off, len, rng)) {
        fprintf(stderr, "iteration %ld, window %llu + %llu\n", it, (unsigned long long)off, (unsigned long long)len);
        return 1;
      }
    }
  }
  printf("range_check: %ld windows of unmutated containers restored their bytes; %ld mutated containers (%ld skipped as "
         "too large), %ld planned, no finding\n", n_windows, iters, skipped, planned);
  return 0;
}
