// Host-only mutation harness for the piece plans of the P32 coder's split containers (tags
// avrecode-amd:P32S / P32SE; avr_dec_plan_load_pieces in avr_plan.cpp), built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_split_p32_sanitizers.py: g++ alone, no ROCm include path,
// no HIP library (avr::shared_bytes, the one device symbol the host units link against, is a stub).
//
//   split32_plan_fuzz <iterations> <seed> <container>
//
// <container> is the oracle's P64 split container of a fixture; the plan layer decodes no stream, so
// it is retagged here (only Metadata.version rewritten).  Through the public ABI only.  First the
// unmutated ones: under P32S the piece plan lists what it lists under P64, under P32SE too, under
// P32 / P32E the seams are AVR_ERR_FORMAT, and the per-slice plan answers AVR_ERR_UNSUPPORTED.  Then
// seeded mutations of the retagged container -- bit flips, extreme values, truncations, repeated
// spans, half of them inside the first 64 bytes (the tag) -- through avr_dec_plan_load_pieces.  An
// accepted plan is read out through every accessor into heap buffers of exactly the reported sizes
// (a byte past one is a sanitizer report) and must keep its units inside the arena, the work buffer
// and the records.  Exit status 0 = no report and no broken invariant.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../../include/avrecode.h"

namespace avr {
size_t shared_bytes(int) { return 0; }   // the kernels' LDS need (avr_kernels.hip): not linked here
}  // namespace avr

namespace {

typedef std::vector<uint8_t> Buf;

Buf read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return Buf(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, "FINDING: "); \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

// Recoded field 1 (Metadata) holding field 1 (version): the first bytes of an avrecode-amd container
bool retag(const Buf& avrc, const std::string& tag, Buf* out) {
  if (avrc.size() < 4 || avrc[0] != 0x0a || avrc[2] != 0x0a || avrc[1] != avrc[3] + 2 || avrc.size() < 4u + avrc[3] ||
      tag.size() > 100)
    return false;
  out->assign({0x0a, (uint8_t)(tag.size() + 2), 0x0a, (uint8_t)tag.size()});
  out->insert(out->end(), tag.begin(), tag.end());
  out->insert(out->end(), avrc.begin() + 4 + avrc[3], avrc.end());
  return true;
}

struct Sizes {
  int n_slices = 0, n_units = 0, max_w = 0, max_h = 0, n_recs = 0;
  size_t arena_len = 0, work_len = 0, rec_stride = 0;
};
int load_pieces(avr_dec_plan* h, const Buf& d, Sizes* z) {
  return avr_dec_plan_load_pieces(h, d.data(), d.size(), &z->n_slices, &z->n_units, &z->arena_len, &z->work_len,
                                  &z->max_w, &z->max_h, &z->n_recs, &z->rec_stride);
}

struct Listing {
  std::vector<avr_slice_desc> descs, units;
  std::vector<avr_piece> pieces;
  Buf arena, recs;
};

// An accepted piece plan, read out into buffers of exactly the reported sizes and checked
int exercise(const avr_dec_plan* h, const Sizes& z, Listing* l) {
  REQUIRE(z.n_slices >= 0 && z.n_units >= z.n_slices && z.n_recs >= 0 && z.arena_len >= 16, "plan: counts");
  REQUIRE(z.max_w >= 1 && z.rec_stride > 0,"plan: width %d, stride %zu", z.max_w, z.rec_stride);
  l->descs.assign((size_t)z.n_slices, avr_slice_desc{});
  int r = avr_dec_plan_descs(h, l->descs.data());
  REQUIRE(r == AVR_OK, "avr_dec_plan_descs: %d", r);
  l->arena.assign(z.arena_len, 0xa5);
  r = avr_dec_plan_arena(h, l->arena.data(), l->arena.size());
  REQUIRE(r == AVR_OK, "avr_dec_plan_arena: %d", r);
  REQUIRE(avr_dec_plan_arena(h, l->arena.data(), l->arena.size() - 1) == AVR_ERR_INVALID_ARGUMENT, "arena one byte short");
  l->units.assign((size_t)z.n_units, avr_slice_desc{});
  l->pieces.assign((size_t)z.n_units, avr_piece{});
  r = avr_dec_plan_units(h, l->units.data(), l->pieces.data());
  REQUIRE(r == AVR_OK, "avr_dec_plan_units: %d", r);
  const size_t rb = (size_t)z.n_recs * z.rec_stride;
  l->recs.assign(rb, 0);
  r = avr_dec_plan_recs(h, l->recs.data(), rb);
  REQUIRE(r == AVR_OK, "avr_dec_plan_recs: %d", r);
  if (rb) REQUIRE(avr_dec_plan_recs(h, l->recs.data(), rb - 1) == AVR_ERR_INVALID_ARGUMENT, "records one byte short");
  int32_t next_seam = 0;
  for (int k = 0; k < z.n_units; k++) {
    const avr_slice_desc& d = l->units[k];
    const avr_piece& p = l->pieces[k];
    REQUIRE(p.seam >= -1 && p.seam < z.n_recs && p.slice >= 0 && p.slice < z.n_slices, "unit %d: seam %d, slice %d", k,
            p.seam, p.slice);
    if (p.seam >= 0) {   // the records are used once each, in unit order
      REQUIRE(p.seam == next_seam, "unit %d: seam %d, expected %d", k, p.seam, next_seam);
      next_seam++;
    }
    REQUIRE(d.payload_offset % 16 == 0 && d.payload_offset <= z.arena_len &&
                (uint64_t)d.payload_size + 16 <= z.arena_len - d.payload_offset,
            "unit %d: stream outside the arena", k);
    REQUIRE(d.read_limit == d.payload_size, "unit %d: read_limit %u of %u", k, d.read_limit, d.payload_size);
    for (int i = 0; i < 16; i++)   // what the P32 decoder reads past a piece: zeros
      REQUIRE(l->arena[d.payload_offset + d.payload_size + i] == 0, "unit %d: byte %d after its stream is not zero", k, i);
    REQUIRE(d.out_offset <= z.work_len && d.out_capacity <= z.work_len - d.out_offset, "unit %d: output outside the work buffer", k);
    REQUIRE(d.mb_width >= 1 && d.mb_width <= z.max_w, "unit %d: width %d of %d", k, d.mb_width, z.max_w);
    if (p.seam >= 0 || p.n_mbs || p.keep != UINT32_MAX)
      REQUIRE(d.mb_width <= 288 && z.rec_stride >= 64 + 1024 + (size_t)40 * d.mb_width, "unit %d: a piece wider than a record", k);
  }
  REQUIRE(next_seam == z.n_recs, "%d records, %d used", z.n_recs, next_seam);
  return 0;
}

void mutate(Buf* d, std::mt19937_64& rng) {
  const int n = 1 + (int)(rng() % 6);
  for (int k = 0; k < n && !d->empty(); k++) {
    const size_t span = rng() % 2 ? std::min<size_t>(64, d->size()) : d->size();
    const size_t at = rng() % span;
    switch (rng() % 5) {
      case 0: (*d)[at] ^= (uint8_t)(1u << (rng() % 8)); break;
      case 1: {
        static const uint8_t v[] = {0x00, 0x01, 0x7f, 0x80, 0xff, 'S', 'E', '2', '4'};
        (*d)[at] = v[rng() % 9];
        break;
      }
      case 2: d->resize(at + (rng() % 2 ? 0 : std::min<size_t>(d->size() - at, 1 + rng() % 4096))); break;
      case 3: {
        static const uint32_t v[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
        const uint32_t x = v[rng() % 5];
        for (int b = 0; b < 4 && at + b < d->size(); b++) (*d)[at + b] = (uint8_t)(x >> (8 * b));
        break;
      }
      default: {
        const size_t len = std::min<size_t>(1 + rng() % 64, d->size() - at);
        Buf s(d->begin() + at, d->begin() + at + len);
        d->insert(d->begin() + at, s.begin(), s.end());
        break;
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <iterations> <seed> <container>\n", argv[0]);
    return 2;
  }
  const long iters = atol(argv[1]);
  const uint64_t seed = strtoull(argv[2], nullptr, 10);
  const Buf p64 = read_file(argv[3]);
  Buf s, se, plain, plain_e;
  REQUIRE(retag(p64, "avrecode-amd:P32S", &s) && retag(p64, "avrecode-amd:P32SE", &se) &&
              retag(p64, "avrecode-amd:P32", &plain) && retag(p64, "avrecode-amd:P32E", &plain_e),
          "the container does not start with a Metadata.version");
  avr_dec_plan* h = nullptr;
  REQUIRE(avr_dec_plan_new(&h) == AVR_OK && h, "avr_dec_plan_new");

  // the unmutated containers
  Sizes z64, z;
  Listing l64, l;
  int r = load_pieces(h, p64, &z64);
  REQUIRE(r == AVR_OK && z64.n_units > z64.n_slices && z64.n_recs > 0, "the P64 container: %d", r);
  if (exercise(h, z64, &l64)) return 1;
  for (const Buf* c : {&s, &se}) {
    r = load_pieces(h, *c, &z);
    REQUIRE(r == AVR_OK, "a retagged S container: %d", r);
    if (exercise(h, z, &l)) return 1;
    REQUIRE(z.n_slices == z64.n_slices && z.n_units == z64.n_units && z.n_recs == z64.n_recs &&
                z.arena_len == z64.arena_len && z.work_len == z64.work_len && z.rec_stride == z64.rec_stride,
            "the S container's plan has other sizes than the P64 one's");
    REQUIRE(l.arena == l64.arena && l.recs == l64.recs &&
                memcmp(l.units.data(), l64.units.data(), sizeof(avr_slice_desc) * l.units.size()) == 0 &&
                memcmp(l.pieces.data(), l64.pieces.data(), sizeof(avr_piece) * l.pieces.size()) == 0,
            "the S container's plan lists other units than the P64 one's");
    int model = -1;
    REQUIRE(avr_container_model(c->data(), c->size(), &model) == AVR_OK && model == AVR_MODEL_PARALLEL32, "model %d", model);
    int ns, mw, mh;
    size_t al, wl;
    r = avr_dec_plan_load(h, c->data(), c->size(), &ns, &al, &wl, &mw, &mh);
    REQUIRE(r == AVR_ERR_UNSUPPORTED, "avr_dec_plan_load of an S container: %d", r);
  }
  for (const Buf* c : {&plain, &plain_e}) {
    r = load_pieces(h, *c, &z);
    REQUIRE(r == AVR_ERR_FORMAT, "seams under a tag without S: %d", r);
  }

  // mutations
  std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 12345);
  long accepted = 0, refused = 0, with_pieces = 0;
  for (long it = 0; it < iters; it++) {
    Buf d = rng() % 4 ? s : se;
    mutate(&d, rng);
    // exactly sized: a read past the container is a report
    Buf exact(d.begin(), d.end());
    exact.shrink_to_fit();
    if (exact.empty()) continue;
    r = load_pieces(h, exact, &z);
    REQUIRE(r == AVR_OK || r == AVR_ERR_FORMAT || r == AVR_ERR_UNSUPPORTED || r == AVR_ERR_OUT_OF_MEMORY ||
                r == AVR_ERR_INVALID_ARGUMENT,
            "iteration %ld: status %d", it, r);
    if (r != AVR_OK) {
      refused++;
      continue;
    }
    accepted++;
    with_pieces += z.n_recs > 0;
    if (exercise(h, z, &l)) {
      fprintf(stderr, "  (iteration %ld, seed %llu)\n", it, (unsigned long long)seed);
      return 1;
    }
  }
  avr_dec_plan_free(h);
  printf("%ld accepted (%ld with pieces), %ld refused; no finding\n", accepted, with_pieces, refused);
  return 0;
}
