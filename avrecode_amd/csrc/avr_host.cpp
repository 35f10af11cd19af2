// Host helpers shared by the translation units of libavrecode (avr_host.h): errors, the parse of a
// whole file, descriptors, and the bulk byte work on host threads.  No HIP.
#include <sys/mman.h>
#include <zlib.h>

#include <chrono>
#include <cstdlib>

#include "avr_host.h"

namespace avr_host {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int fail(ErrSink* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

avr_slice_desc desc_from_header(const avr::SliceInfo& s) {
  avr_slice_desc d;
  memset(&d, 0, sizeof(d));
  d.slice_type = s.h.slice_type == 3 ? 0 : s.h.slice_type == 4 ? 2 : s.h.slice_type;
  d.slice_qp = s.h.slice_qp;
  d.cabac_init_idc = s.h.cabac_init_idc;
  d.first_mb = s.h.first_mb;
  d.mb_width = s.h.mb_width;
  d.mb_height = s.h.mb_height;
  d.num_ref_idx_l0 = s.h.num_ref_idx[0];
  d.num_ref_idx_l1 = s.h.num_ref_idx[1];
  d.chroma_array_type = s.h.chroma_array_type;
  d.transform_8x8_mode = s.h.transform_8x8_mode;
  d.direct_8x8_inference = s.h.direct_8x8_inference;
  d.x264_build = s.h.x264_build;
  d.picture_id = s.picture_id;
  d.coded = 1;
  d.file_offset = ~(uint64_t)0;
  d.structure = s.h.field_pic ? (s.h.bottom_field ? AVR_STRUCT_BOTTOM_FIELD : AVR_STRUCT_TOP_FIELD)
              : s.h.mbaff ? AVR_STRUCT_MBAFF : AVR_STRUCT_FRAME;
  return d;
}

int parse_file(ErrSink* c, const uint8_t* in, size_t n, ParsedFile* pf, bool views, const avr::SkipRanges* skips) {
  std::vector<avr::NalRef> nals;
  if (!avr::demux(in, n, &nals, skips)) return fail(c, AVR_ERR_FORMAT, "not an MP4/avcC or Annex-B H.264 stream");
  avr::StreamParser sp;
  sp.set_skips(in, skips);
  for (auto& nr : nals) {
    avr::SliceInfo s;
    if (sp.next(in + nr.offset, nr.size, &s, views)) {
      s.nal_offset = nr.offset;
      s.nal_size = nr.size;
      pf->slices.push_back(std::move(s));
    }
  }
  return AVR_OK;
}

thread_local bool tl_in_file_pool = false;   // see avr_host.h
unsigned bulk_threads() {
  return tl_in_file_pool ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
}

// A large host output buffer handed to the caller (freed by avr_free = free): 2 MiB aligned and
// advised to transparent huge pages, so its first touch costs one fault per 2 MiB instead of per
// 4 KiB page (a 4.4 GB container or payload arena: ~1 s of page faults otherwise).
uint8_t* host_alloc(size_t n) {
  constexpr size_t kHuge = (size_t)2 << 20;
  if (n < 16 * kHuge) return (uint8_t*)malloc(n ? n : 1);
  void* p = nullptr;
  if (posix_memalign(&p, kHuge, n)) return nullptr;
  (void)madvise(p, n & ~(kHuge - 1), MADV_HUGEPAGE);
  return (uint8_t*)p;
}

// Byte copies of a container's literals and re-coded blocks, spread over host threads when they are
// large (a 10-minute 4K stream's container is 4.4 GB).  A job without a source fills its bytes
// with `fill` (the decompressor's surrogate blocks).
static void copy_part(uint8_t* dst, const uint8_t* src, size_t len, uint8_t fill) {
  if (src) memcpy(dst, src, len);
  else memset(dst, fill, len);
}
void parallel_copies(const std::vector<avr::PbCopy>& jobs, uint8_t* base, uint8_t fill) {
  uint64_t total = 0;
  for (const auto& j : jobs) total += j.len;
  const unsigned T = total < ((uint64_t)64 << 20) ? 1u : bulk_threads();
  if (T == 1) {
    for (const auto& j : jobs) copy_part(base + j.dst, j.src, j.len, fill);
    return;
  }
  // thread t copies the bytes [t total / T, (t + 1) total / T) of the concatenated jobs
  auto work = [&](unsigned t) {
    const uint64_t lo = total * t / T, hi = total * (t + 1) / T;
    uint64_t at = 0;
    for (const auto& j : jobs) {
      const uint64_t a = std::max(at, lo), b = std::min(at + j.len, hi);
      if (a < b) copy_part(base + j.dst + (a - at), j.src ? j.src + (a - at) : nullptr, (size_t)(b - a), fill);
      at += j.len;
      if (at >= hi) break;
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
}

void zero_gaps(const std::vector<avr::PbCopy>& jobs, uint8_t* base, uint64_t from, uint64_t end) {
  uint64_t z = from;
  for (const auto& j : jobs) {
    memset(base + z, 0, j.dst - z);
    z = j.dst + j.len;
  }
  memset(base + z, 0, end - z);
}

// ------------------------------------------------------------------ checked containers
namespace {

// a b mod P in the reflected representation (bit 31 - k is the coefficient of x^k), as the kernel's
// crc_mulmod (avr_k_crc.hip)
uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1));
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1)));
  }
  return p;
}

// x^(2^k) mod P, k < 67: x^(8 len) for any 64-bit len is a product of at most 64 of them
struct CrcPowers {
  uint32_t p[67];
  CrcPowers() {
    p[0] = 0x40000000u;
    for (int k = 1; k < 67; k++) p[k] = crc_mulmod(p[k - 1], p[k - 1]);
  }
};

constexpr size_t kCrcChunk = (size_t)4 << 20;   // a long item's share of one host thread's turn

}  // namespace

void resolve_crc_items(std::vector<CrcItem>* items) {
  // the bytes nobody has CRC'd yet, in chunks, on host threads when they are many
  struct Job {
    size_t item;
    const uint8_t* p;
    size_t len;
    uint32_t crc;
  };
  std::vector<Job> jobs;
  uint64_t bytes = 0;
  for (size_t i = 0; i < items->size(); i++) {
    const CrcItem& it = (*items)[i];
    if (it.known) continue;
    for (uint64_t at = 0; at < it.len; at += kCrcChunk)
      jobs.push_back({i, it.p + at, (size_t)std::min<uint64_t>(kCrcChunk, it.len - at), 0});
    bytes += it.len;
  }
  const unsigned T = bytes < ((uint64_t)64 << 20) ? 1u : bulk_threads();
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t k; (k = next.fetch_add(1)) < jobs.size();) jobs[k].crc = avr_crc32(0, jobs[k].p, jobs[k].len);
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  for (CrcItem& it : *items)
    if (!it.known) it.crc = 0;
  for (const Job& j : jobs) (*items)[j.item].crc = avr_crc32_combine((*items)[j.item].crc, j.crc, j.len);
  // the last-byte rule on each value
  const z_crc_t* byte_table = get_crc_table();
  for (CrcItem& it : *items) {
    if (it.rule == LastByte::kAppend) it.crc = avr_crc32(it.crc, &it.last_byte, 1), it.len++;
    else if (it.rule == LastByte::kReplace) it.crc ^= (uint32_t)byte_table[it.regen_last ^ it.last_byte];
    it.known = true;
    it.rule = LastByte::kKeep;
  }
}

// the blocks in file order
uint32_t combine_crc_items(const std::vector<CrcItem>& items) {
  uint32_t crc = 0;
  for (const CrcItem& it : items)
    if (it.in_file) crc = avr_crc32_combine(crc, it.crc, it.len);
  return crc;
}

uint32_t fold_file_crc(std::vector<CrcItem>* items) {
  resolve_crc_items(items);
  return combine_crc_items(*items);
}

}  // namespace avr_host

extern "C" {

uint32_t avr_crc32(uint32_t crc, const uint8_t* p, size_t n) {
  while (n) {   // zlib takes 32-bit lengths
    const size_t k = std::min<size_t>(n, (size_t)1 << 30);
    crc = (uint32_t)crc32(crc, p, (uInt)k);
    p += k;
    n -= k;
  }
  return crc;
}

uint32_t avr_crc32_combine(uint32_t a, uint32_t b, uint64_t len_b) {
  static const avr_host::CrcPowers pw;
  uint32_t m = 0x80000000u;   // x^(8 len_b)
  for (int k = 0; len_b; len_b >>= 1, k++)
    if (len_b & 1) m = avr_host::crc_mulmod(m, pw.p[k + 3]);
  return avr_host::crc_mulmod(a, m) ^ b;
}

}  // extern "C"
