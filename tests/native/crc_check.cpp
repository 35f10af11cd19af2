// Host-only harness for checked containers (Recoded.Metadata field 16, the file's CRC-32): the CRC and
// its combine, the fold (fold_file_crc, avr_host.cpp) and the splice check (avr_plan.cpp) on a checked
// container and on seeded mutations of it.  Built with AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_checksum_sanitizers.py: g++ alone, no ROCm, no device, its own main -- nothing here is
// loaded into Python.
//
//   crc_check <iterations> <seed> <file> <container>
//     file       the original file (tests/fixtures/cockatoo.mp4)
//     container  its parallel-model container assembled with AVR_ASSEMBLE_CRC
//
// 1. avr_crc32 and avr_crc32_combine against a bit-by-bit CRC, over seeded buffers and the lengths
//    where a table or a chunked CRC goes wrong.
// 2. fold_file_crc against the bit-by-bit CRC of the items' bytes written out: known and unknown
//    values, the three cases of the last-byte rule, empty items, an item longer than a host
//    thread's chunk, and enough bytes in all for the fold to take its threads.
// 3. The unmutated container: its plan, spliced with the file's own payloads as the regenerated
//    bytes, is the file -- also with every slice one byte short of its parity and with the payloads'
//    CRCs brought; one byte off in a slice, or one CRC off, is AVR_ERR_CHECKSUM with nothing written.
// 4. Mutations: seeded byte mutations of the whole container.  Every call returns AVR_OK or a
//    documented error, and a splice that returns AVR_OK on a container that still has the field has
//    written a file with that CRC.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../../avrecode_amd/csrc/avr_host.h"

// avr_assemble.cpp asks the device library for a slice's LDS size; nothing here assembles a container
namespace avr {
size_t shared_bytes(int) { return 0; }
}  // namespace avr

namespace {

typedef std::vector<uint8_t> Buf;
int g_bad = 0;

#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      printf("FINDING %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                 \
      printf("\n");                        \
      g_bad++;                             \
    }                                      \
  } while (0)

Buf read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return Buf(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// CRC-32 / ISO-HDLC one bit at a time
uint32_t crc_by_bits(uint32_t crc, const uint8_t* p, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; i++) {
    crc ^= p[i];
    for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1)));
  }
  return ~crc;
}

Buf seeded(std::mt19937_64& rng, size_t n) {
  Buf b(n);
  for (auto& x : b) x = (uint8_t)rng();
  return b;
}

// ------------------------------------------------------------------ 1. the CRC and its combine
void crc_cases() {
  std::mt19937_64 rng(3);
  CHECK(avr_crc32(0, nullptr, 0) == 0, "the empty buffer's CRC");
  const uint8_t check[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
  CHECK(avr_crc32(0, check, 9) == 0xCBF43926u, "the check value of CRC-32/ISO-HDLC");
  const size_t lens[] = {0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65541};
  for (size_t la : lens)
    for (size_t lb : lens) {
      if (la > 300 && lb > 300) continue;
      const Buf a = seeded(rng, la), b = seeded(rng, lb);
      // copies of exactly the size on the heap: a read past either end is a sanitizer report
      uint8_t* pa = (uint8_t*)malloc(la ? la : 1);
      if (la) memcpy(pa, a.data(), la);
      const uint32_t ca = avr_crc32(0, pa, la), cb = avr_crc32(0, b.data(), lb);
      free(pa);
      CHECK(ca == crc_by_bits(0, a.data(), la), "avr_crc32 on %zu bytes", la);
      CHECK(avr_crc32(ca, b.data(), lb) == crc_by_bits(ca, b.data(), lb), "avr_crc32 carried over %zu + %zu", la, lb);
      CHECK(avr_crc32_combine(ca, cb, lb) == crc_by_bits(ca, b.data(), lb), "avr_crc32_combine %zu + %zu", la, lb);
    }
  // a long second part: zeros, whose CRC the carried form gives without a second buffer
  const size_t n = (size_t)40 << 20;
  const Buf z(n, 0);
  const uint32_t ca = avr_crc32(0, check, 9);
  CHECK(avr_crc32_combine(ca, avr_crc32(0, z.data(), n), n) == avr_crc32(ca, z.data(), n), "combine over 40 MiB");
  // lengths past 32 bits (8 len past 64): the combine is associative, whatever the values
  const uint64_t lb = ((uint64_t)1 << 33) + 1, lc = ((uint64_t)1 << 61) + 7;
  CHECK(avr_crc32_combine(avr_crc32_combine(ca, 0x12345678u, lb), 0x9abcdef0u, lc) ==
            avr_crc32_combine(ca, avr_crc32_combine(0x12345678u, 0x9abcdef0u, lc), lb + lc),
        "combine at lengths past 2^32");
}

// ------------------------------------------------------------------ 2. the fold
void fold_cases(int rounds, uint64_t seed) {
  using avr_host::CrcItem;
  using avr_host::LastByte;
  std::mt19937_64 rng(seed * 1000003 + 11);
  for (int it = 0; it < rounds; it++) {
    const int n = 1 + (int)(rng() % 12);
    std::vector<Buf> bytes(n);
    std::vector<CrcItem> items(n);
    Buf whole;
    for (int i = 0; i < n; i++) {
      // round 0: one item past a host thread's chunk, and enough bytes for the fold's threads
      const size_t len = it == 0 && i == 0 ? ((size_t)66 << 20) + 5 : rng() % 5 == 0 ? 0 : 1 + rng() % 3000;
      bytes[i] = seeded(rng, len);
      CrcItem& c = items[i];
      c.p = bytes[i].data();
      c.len = len;
      c.known = rng() % 2;
      if (c.known) c.crc = crc_by_bits(0, bytes[i].data(), len), c.p = len && rng() % 2 ? c.p : nullptr;
      whole.insert(whole.end(), bytes[i].begin(), bytes[i].end());
      const int rule = (int)(rng() % 3);
      const uint8_t lb = (uint8_t)rng();
      if (rule == 1) {
        c.rule = LastByte::kAppend, c.last_byte = lb;
        whole.push_back(lb);
      } else if (rule == 2 && len) {
        c.rule = LastByte::kReplace, c.last_byte = lb, c.regen_last = bytes[i][len - 1];
        whole.back() = lb;
      }
    }
    const uint32_t got = avr_host::fold_file_crc(&items);
    CHECK(got == avr_crc32(0, whole.data(), whole.size()), "fold of %d items (round %d)", n, it);
  }
}

// ------------------------------------------------------------------ 3. and 4. plans and splices
bool documented(int r) {
  return r == AVR_OK || r == AVR_ERR_FORMAT || r == AVR_ERR_INVALID_ARGUMENT || r == AVR_ERR_UNSUPPORTED ||
         r == AVR_ERR_OUT_OF_MEMORY || r == AVR_ERR_CHECKSUM;
}

struct PlanHandle {
  avr_dec_plan* h = nullptr;
  PlanHandle() { avr_dec_plan_new(&h); }
  ~PlanHandle() { avr_dec_plan_free(h); }
};

// the regenerated bytes of a plan's slices, one after the other
struct Regen {
  Buf bytes;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<int32_t> status;
  std::vector<uint32_t> crc;
  void add(const uint8_t* p, size_t n) {
    off.push_back(bytes.size());
    len.push_back((uint32_t)n);
    status.push_back(0);
    crc.push_back(avr_crc32(0, p, n));
    bytes.insert(bytes.end(), p, p + n);
  }
};

// avr_dec_plan_splice(_crc) into a buffer of exactly the reported size
int splice(const avr_dec_plan* h, const Regen& g, bool crcs, Buf* out) {
  size_t need = 0;
  // a NULL regen with slices is refused: a plan without slices has no bytes
  const uint8_t* rp = g.bytes.empty() ? (const uint8_t*)"" : g.bytes.data();
  int r = avr_dec_plan_splice_crc(h, g.status.data(), rp, g.bytes.size(), g.off.data(), g.len.data(),
                                  crcs ? g.crc.data() : nullptr, nullptr, 0, &need);
  if (r != AVR_ERR_INVALID_ARGUMENT && r != AVR_OK) return r;
  uint8_t* o = (uint8_t*)malloc(need ? need : 1);
  memset(o, 0xEE, need ? need : 1);
  r = avr_dec_plan_splice_crc(h, g.status.data(), rp, g.bytes.size(), g.off.data(), g.len.data(),
                              crcs ? g.crc.data() : nullptr, o, need, &need);
  out->assign(o, o + (r == AVR_OK ? need : 0));
  if (r == AVR_ERR_CHECKSUM)   // refused before anything was written
    for (size_t i = 0; i < need; i++)
      if (o[i] != 0xEE) {
        CHECK(false, "a refused splice wrote byte %zu", i);
        break;
      }
  free(o);
  return r;
}

void unmutated(const Buf& file, const Buf& avrc) {
  std::vector<avr::PbBlock> blocks;
  std::string version;
  avr::PbFileCrc fc;
  CHECK(avr::pb_parse(avrc.data(), avrc.size(), &blocks, &version, nullptr, &fc) && fc.present, "the container has the field");
  CHECK(fc.value == crc_by_bits(0, file.data(), file.size()), "the field is the file's CRC");
  PlanHandle ph;
  int ns = 0, mw = 0, mh = 0;
  size_t al = 0, wl = 0;
  CHECK(avr_dec_plan_load(ph.h, avrc.data(), avrc.size(), &ns, &al, &wl, &mw, &mh) == AVR_OK, "plan load");
  // the file's own payloads: a coded block stands for `size` bytes of the file after the literals and coded blocks before it
  Regen whole, shorter;
  size_t at = 0;
  int appends = 0;
  for (const avr::PbBlock& b : blocks) {
    if (b.has_literal) at += b.literal_len;
    if (b.has_cabac) {
      whole.add(file.data() + at, (size_t)b.size);
      shorter.add(file.data() + at, (size_t)b.size - 1);   // the parity rule appends the last byte
      appends++;
      at += (size_t)b.size;   // a skip_coded slice's bytes lie in the literals
    }
  }
  CHECK((int)whole.len.size() == ns && appends > 0, "the plan lists the coded blocks");
  Buf out;
  for (int crcs = 0; crcs < 2; crcs++) {
    CHECK(splice(ph.h, whole, crcs, &out) == AVR_OK && out == file, "the splice restores the file (crcs %d)", crcs);
    CHECK(splice(ph.h, shorter, crcs, &out) == AVR_OK && out == file, "one byte short at every slice's end (crcs %d)", crcs);
  }
  for (size_t k : {(size_t)0, whole.len.size() / 2, whole.len.size() - 1}) {
    Regen bad = whole;
    bad.bytes[bad.off[k] + bad.len[k] / 2] ^= 0x10;
    CHECK(splice(ph.h, bad, false, &out) == AVR_ERR_CHECKSUM, "a damaged slice %zu passes the check", k);
    bad = whole;
    bad.crc[k] += 1;
    CHECK(splice(ph.h, bad, true, &out) == AVR_ERR_CHECKSUM, "a wrong CRC for slice %zu passes the check", k);
  }
  // the older entry point
  uint8_t* o = nullptr;
  size_t on = 0;
  CHECK(avr_splice_container(avrc.data(), avrc.size(), ns, whole.status.data(), whole.bytes.data(), whole.bytes.size(),
                             whole.off.data(), whole.len.data(), &o, &on) == AVR_OK && on == file.size() &&
            memcmp(o, file.data(), on) == 0, "avr_splice_container restores the file");
  free(o);   // avr_free is free (avr_api.cpp, not linked here)
  Regen bad = whole;
  bad.bytes[bad.off[1]] ^= 1;
  o = nullptr;
  CHECK(avr_splice_container(avrc.data(), avrc.size(), ns, bad.status.data(), bad.bytes.data(), bad.bytes.size(),
                             bad.off.data(), bad.len.data(), &o, &on) == AVR_ERR_CHECKSUM && !o,
        "avr_splice_container checks the file");
  free(o);   // avr_free is free (avr_api.cpp, not linked here)
}

void mutate(Buf* b, std::mt19937_64& rng) {
  const int k = 1 + (int)(rng() % 3);
  for (int i = 0; i < k && !b->empty(); i++) {
    const size_t at = rng() % b->size();
    switch (rng() % 5) {
      case 0: (*b)[at] ^= (uint8_t)(1u << (rng() % 8)); break;
      case 1: (*b)[at] = (uint8_t)rng(); break;
      case 2: b->erase(b->begin() + (long)at); break;
      case 3: b->insert(b->begin() + (long)at, (uint8_t)rng()); break;
      default: b->resize(at + 1); break;
    }
  }
}

void mutations(const Buf& avrc, int iters, uint64_t seed) {
  std::mt19937_64 rng(seed);
  int accepted = 0, refused = 0, wrote = 0;
  for (int it = 0; it < iters; it++) {
    Buf m = avrc;
    // half of the mutations in the first 4 KiB, where the Metadata and the first blocks' headers are
    if (it % 2) {
      Buf head(m.begin(), m.begin() + (long)std::min<size_t>(4096, m.size()));
      mutate(&head, rng);
      m.erase(m.begin(), m.begin() + (long)std::min<size_t>(4096, m.size()));
      m.insert(m.begin(), head.begin(), head.end());
    } else {
      mutate(&m, rng);
    }
    // a copy of exactly the size on the heap: a read past its end is a sanitizer report
    uint8_t* p = (uint8_t*)malloc(m.size() ? m.size() : 1);
    if (!m.empty()) memcpy(p, m.data(), m.size());
    PlanHandle ph;
    int ns = 0, mw = 0, mh = 0;
    size_t al = 0, wl = 0;
    int r = avr_dec_plan_load(ph.h, p, m.size(), &ns, &al, &wl, &mw, &mh);
    CHECK(documented(r), "avr_dec_plan_load returned %d", r);
    if (r == AVR_OK) {
      std::vector<avr::PbBlock> blocks;
      std::string version;
      avr::PbFileCrc fc;
      CHECK(avr::pb_parse(p, m.size(), &blocks, &version, nullptr, &fc), "a loaded container parses");
      std::vector<avr_slice_desc> d((size_t)ns);
      avr_dec_plan_descs(ph.h, d.data());
      Regen g;
      for (int k = 0; k < ns; k++) {   // zero-rich bytes of each slice's size
        Buf x(d[k].out_capacity >= 64 ? d[k].out_capacity - 64 : 0);
        for (auto& y : x) y = rng() % 3 ? 0 : (uint8_t)rng();
        g.add(x.data(), x.size());
      }
      Buf out;
      const bool crcs = rng() % 2;
      r = splice(ph.h, g, crcs, &out);
      CHECK(documented(r), "avr_dec_plan_splice_crc returned %d", r);
      accepted++;
      if (r == AVR_OK) {
        wrote++;
        CHECK(!fc.present || avr_crc32(0, out.data(), out.size()) == fc.value, "a checked splice wrote a file of another CRC");
      } else if (r == AVR_ERR_CHECKSUM) {
        refused++;
        CHECK(fc.present, "AVR_ERR_CHECKSUM on a container without the field");
      }
    }
    free(p);
  }
  printf("mutations: %d, plans accepted %d, splices refused by the CRC %d, files written %d\n", iters, accepted, refused, wrote);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: crc_check <iterations> <seed> <file> <container>\n");
    return 2;
  }
  const int iters = atoi(argv[1]);
  const uint64_t seed = strtoull(argv[2], nullptr, 10);
  const Buf file = read_file(argv[3]), avrc = read_file(argv[4]);
  if (file.empty() || avrc.empty()) {
    fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  if (iters == 0) {
    crc_cases();
    fold_cases(200, seed);
    unmutated(file, avrc);
  } else {
    fold_cases(20, seed);
    mutations(avrc, iters, seed);
  }
  if (g_bad) {
    printf("%d finding(s)\n", g_bad);
    return 1;
  }
  printf("no finding\n");
  return 0;
}
