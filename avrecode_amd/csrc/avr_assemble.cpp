// The container writer: which slices the device may re-code, the segmentation of a file into
// literals and coded blocks (find_next_coded_block_and_emit_literal, recode.cpp:1275-1297), the
// Recoded protobuf written once, rank 0's assembly of gathered slice outputs, and the stream-parse
// entry points of the C ABI.  No HIP in this source; it links against avr::shared_bytes
// (avr_kernels.hip) for the LDS a slice's ring needs.
#include <cstdio>
#include <cstdlib>

#include "avr_host.h"

using namespace avr_host;

namespace {

constexpr size_t kLdsBudget = 160 * 1024;   // LDS per workgroup (one slice) on gfx950

// Every 00 00 0y trigram (y <= 3) of a file, keyed by y and the four bytes after it, then by
// position.  In an escaped H.264 stream these occur only at start codes, emulation-prevention bytes
// (00 00 03) and container bytes (MP4 lengths and boxes), so the index is small.
struct TrigramIndex {
  bool built = false;
  struct Entry {
    uint64_t key;   // y << 32 | the next four bytes (big-endian, zeros past the end)
    uint64_t pos;
    bool operator<(const Entry& o) const { return key != o.key ? key < o.key : pos < o.pos; }
  };
  std::vector<Entry> e;
  // per y, every trigram position in ascending order: the lookups whose payload holds no four bytes
  // after its trigram (built at the first such lookup)
  bool pos_built = false;
  std::vector<uint64_t> pos[4];
  void build_pos() {
    pos_built = true;
    for (const Entry& x : e) pos[x.key >> 32].push_back(x.pos);
    for (auto& v : pos) std::sort(v.begin(), v.end());
  }
  static uint64_t key_at(const uint8_t* f, size_t n, size_t p) {   // trigram at p (p + 2 < n)
    uint32_t nx = 0;
    for (int k = 0; k < 4; k++) nx = nx << 8 | (p + 3 + k < n ? f[p + 3 + k] : 0u);
    return (uint64_t)f[p + 2] << 32 | nx;
  }
  // the trigrams starting in [lo, hi)
  static void scan(const uint8_t* f, size_t n, size_t lo, size_t hi, std::vector<Entry>* out) {
    const uint8_t* end = f + std::min(hi, n >= 2 ? n - 2 : 0);
    for (const uint8_t* p = f + lo; p < end;) {
      p = (const uint8_t*)memchr(p, 0, (size_t)(end - p));
      if (!p) break;
      if (p[1] == 0 && p[2] <= 3) out->push_back({key_at(f, n, (size_t)(p - f)), (uint64_t)(p - f)});
      p++;
    }
  }
  void build(const uint8_t* f, size_t n) {
    built = true;
    // a multi-GB file is scanned in chunks on host threads
    const unsigned T = n < ((size_t)256 << 20) ? 1u : bulk_threads();
    std::vector<std::vector<Entry>> part(T);
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(scan, f, n, n * t / T, n * (t + 1) / T, &part[t]);
    scan(f, n, 0, n / T, &part[0]);
    for (auto& x : th) x.join();
    for (auto& v : part) e.insert(e.end(), v.begin(), v.end());
    std::sort(e.begin(), e.end());
  }
};

// memmem(in + from, n - from, P, m) (the reference's search, recode.cpp:1285) without its cost on a
// miss.  A payload P holding a 00 00 0y trigram (y <= 3) at offset j -- an unescaped payload whose
// NAL had emulation-prevention bytes -- can only occur at q with a trigram of the file at q + j
// followed by the same four bytes as in P (when P has them), so the index's entries with that key
// from position from + j on, in ascending order, are the only candidates and the first that matches
// is memmem's answer.  Such payloads are exactly the ones that usually occur nowhere, where memmem
// would scan to the end of the file for each of them (O(misses x file): minutes for a 10-minute 4K
// stream); with the key a miss costs a binary search.  A payload without one is found in its own
// NAL (its bytes are verbatim there), so memmem stops at most one NAL past `from`.
// `end` (<= n): the occurrence must lie within in[from, end) -- the escaped search of segment(), which
// stops inside the slice's own NAL.
const uint8_t* find_payload(const uint8_t* in, size_t n, size_t from, const uint8_t* P, size_t m, TrigramIndex* ix,
                            size_t end = ~(size_t)0) {
  end = std::min(end, n);
  if (from > end || m > end - from) return nullptr;
  size_t j = 0;
  bool anchor = false;
  for (const uint8_t* q = P; m >= 3 && q + 2 < P + m;) {
    q = (const uint8_t*)memchr(q, 0, (size_t)(P + m - 2 - q));
    if (!q) break;
    if (q[1] == 0 && q[2] <= 3) {
      j = (size_t)(q - P);
      anchor = true;
      break;
    }
    q++;
  }
  if (!anchor) return (const uint8_t*)memmem(in + from, end - from, P, m);
  if (!ix->built) {
    const double tb = now_s();
    ix->build(in, n);
    if (getenv("AVR_ASM_TIMING")) fprintf(stderr, "index build %.3f s, %zu entries\n", now_s() - tb, ix->e.size());
  }
  using E = TrigramIndex::Entry;
  if (j + 7 > m) {
    // the trigram lies in P's last six bytes: no key beyond y; y's positions from from + j on, in
    // ascending order -- the first that matches is memmem's answer
    if (!ix->pos_built) ix->build_pos();
    const std::vector<uint64_t>& ps = ix->pos[P[j + 2]];
    for (auto it = std::lower_bound(ps.begin(), ps.end(), (uint64_t)(from + j)); it != ps.end(); ++it) {
      const size_t q = (size_t)*it - j;
      if (q + m > end) break;
      if (memcmp(in + q, P, m) == 0) return in + q;
    }
    return nullptr;
  }
  const uint64_t key = TrigramIndex::key_at(P, m, j);   // P holds the four bytes after its trigram
  for (auto it = std::lower_bound(ix->e.begin(), ix->e.end(), E{key, (uint64_t)(from + j)}); it != ix->e.end(); ++it) {
    if (it->key != key) break;
    const size_t q = (size_t)it->pos - j;
    if (q + m > end) break;
    if (memcmp(in + q, P, m) == 0) return in + q;
  }
  return nullptr;
}

// memmem(in + from, n - from, P, m) for a payload that stands verbatim at `own` >= from (segment
// checks it): memmem's
// answer is the first occurrence at or after `from` and `own` is one, so only [from, own) -- the
// literal gap before the slice: start code or length, NAL and slice header, skipped NAL units --
// needs a search.  Candidates are the gap's bytes equal to P[0] (memchr), each checked on its first
// 64 bytes and, if those agree, in full; a gap with more than a few such deep candidates (only a
// degenerate payload has them) goes to memmem over [from, own + m - 1).  O(gap) per slice instead
// of memmem's O(m) needle preparation plus its scan: the segmentation of a 4 GB stream no longer
// reads the stream once more.
const uint8_t* find_before(const uint8_t* in, size_t from, size_t own, const uint8_t* P, size_t m) {
  const size_t head = std::min<size_t>(m, 64);
  int deep = 0;
  for (size_t q = from; q < own;) {
    const uint8_t* h = (const uint8_t*)memchr(in + q, P[0], own - q);
    if (!h) break;
    if (memcmp(h, P, head) == 0) {
      if (++deep > 4) {
        const uint8_t* r = (const uint8_t*)memmem(in + from, own - from + m - 1, P, m);
        return r ? r : in + own;
      }
      if (memcmp(h + head, P + head, m - head) == 0) return h;
    }
    q = (size_t)(h - in) + 1;
  }
  return in + own;
}

// Rank 0's container from gathered per-slice outputs (both avr_assemble_container entry points).
// The optional seams fields of avr_assemble_container_seams: slice i's Block field 16 is
// p[offsets[i] .. + lens[i]) (length 0: none; p null: none at all).
struct SeamsArg {
  const uint8_t* p = nullptr;
  size_t len = 0;
  const uint64_t* offsets = nullptr;
  const uint32_t* lens = nullptr;
};

int assemble(const uint8_t* file, size_t n, int model, const std::vector<SliceView>& sv, const int32_t* status,
             const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, uint8_t** out,
             size_t* out_len, uint8_t* dst = nullptr, size_t cap = 0, const SeamsArg& sa = SeamsArg(),
             uint32_t flags = 0, const uint32_t* crcs = nullptr) {
  // the escaped second chance and the unit checksums are the parallel models' own format, the opt-in
  // split the P32 coder's; the file's CRC is any model's
  if ((flags & ~(uint32_t)(AVR_ASSEMBLE_ESCAPED | AVR_ASSEMBLE_SPLIT32 | AVR_ASSEMBLE_CRC | AVR_ASSEMBLE_UNIT_CRC)) ||
      ((flags & (AVR_ASSEMBLE_ESCAPED | AVR_ASSEMBLE_UNIT_CRC)) && !parallel_model(model)) ||
      ((flags & AVR_ASSEMBLE_SPLIT32) && model != AVR_MODEL_PARALLEL32))
    return AVR_ERR_INVALID_ARGUMENT;
  const bool seams_ok = model == AVR_MODEL_PARALLEL || (flags & AVR_ASSEMBLE_SPLIT32);
  std::vector<char> ok(sv.size(), 0);
  std::vector<std::pair<const uint8_t*, size_t>> blobs(sv.size(), {nullptr, 0}), fields;
  if (sa.p) fields.assign(sv.size(), {nullptr, 0});
  for (size_t i = 0; i < sv.size(); i++) {
    ok[i] = sv[i].candidate && status[i] == 0;
    if (ok[i]) {
      if (!recoded || offsets[i] > recoded_len || lens[i] > recoded_len - offsets[i]) return AVR_ERR_INVALID_ARGUMENT;
      blobs[i] = {recoded + offsets[i], lens[i]};
    }
    if (sa.p && sa.lens[i]) {
      // a seams field belongs to a coded slice of the parallel model -- on the u64 coder, or on the P32
      // coder with AVR_ASSEMBLE_SPLIT32 -- and lies in the blob
      if (!seams_ok || !ok[i] || sa.offsets[i] > sa.len || sa.lens[i] > sa.len - sa.offsets[i])
        return AVR_ERR_INVALID_ARGUMENT;
      fields[i] = {sa.p + sa.offsets[i], sa.lens[i]};
    }
  }
  const double t0 = now_s();
  std::vector<uint32_t> escapes;
  const bool esc = (flags & AVR_ASSEMBLE_ESCAPED) != 0;
  const std::vector<const uint8_t*> found = segment(file, n, sv, ok, esc ? &escapes : nullptr);
  const double t1 = now_s();
  const int r = emit_container(file, n, sv, found, blobs, model, out, out_len, dst, cap, sa.p ? &fields : nullptr,
                               esc ? &escapes : nullptr, FileCrcArg{(flags & AVR_ASSEMBLE_CRC) != 0, crcs},
                               UnitCrcArg{(flags & AVR_ASSEMBLE_UNIT_CRC) != 0, nullptr});
  if (getenv("AVR_ASM_TIMING")) fprintf(stderr, "assemble: segment %.3f s, emit %.3f s\n", t1 - t0, now_s() - t1);
  return r;
}

int assemble_parsed(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                    const uint8_t* arena, size_t arena_len, const int32_t* status, const uint8_t* recoded,
                    size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, uint8_t** out, size_t* out_len,
                    uint8_t* dst, size_t cap, const SeamsArg& sa = SeamsArg(), uint32_t flags = 0,
                    const uint32_t* crcs = nullptr) {
  if (!file || !out_len || n_slices < 0 || (n_slices && (!descs || !arena || !status || !offsets || !lens)) ||
      !assemblable(model) || (sa.p && n_slices && (!sa.offsets || !sa.lens)))
    return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    std::vector<SliceView> sv((size_t)n_slices);
    for (int i = 0; i < n_slices; i++) {
      const avr_slice_desc& d = descs[i];
      if (d.payload_offset > arena_len || d.payload_size > arena_len - d.payload_offset) return AVR_ERR_INVALID_ARGUMENT;
      // only avr_parse_stream's own descriptors of this file: a coded slice is one recodable_candidate
      // accepted (a surrogate marker long, its LDS ring within a workgroup), and a payload the parse
      // found verbatim stands at file_offset (its first and last bytes checked: O(1) per slice)
      if (d.coded && (d.payload_size < (uint32_t)avr::kSurrogateMarkerBytes ||
                      avr::shared_bytes(ring_cols(d)) > kLdsBudget))
        return AVR_ERR_INVALID_ARGUMENT;
      const uint8_t* P = arena + d.payload_offset;
      const size_t m = d.payload_size;
      if (d.file_offset != ~(uint64_t)0) {
        const size_t k = std::min<size_t>(m, 16);
        if (d.file_offset > n || m > n - d.file_offset || memcmp(file + d.file_offset, P, k) != 0 ||
            memcmp(file + d.file_offset + m - k, P + m - k, k) != 0)
          return AVR_ERR_INVALID_ARGUMENT;
      }
      sv[i] = {P, m, d.coded != 0, d.file_offset};
    }
    // the escaped search needs each affected slice's NAL, which a descriptor does not carry: the
    // file is parsed here once when a coded slice's payload does not stand verbatim in it
    bool affected = false;
    for (int i = 0; i < n_slices && (flags & AVR_ASSEMBLE_ESCAPED); i++)
      affected = affected || (descs[i].coded && status[i] == 0 && descs[i].file_offset == ~(uint64_t)0);
    if (affected) {
      ParsedFile pf;
      if (int r = parse_file(nullptr, file, n, &pf, /*views=*/true)) return r;
      if ((size_t)n_slices != pf.slices.size()) return AVR_ERR_INVALID_ARGUMENT;
      for (int i = 0; i < n_slices; i++)
        sv[i].nal_lo = pf.slices[i].nal_offset, sv[i].nal_hi = pf.slices[i].nal_offset + pf.slices[i].nal_size;
    }
    return assemble(file, n, model, sv, status, recoded, recoded_len, offsets, lens, out, out_len, dst, cap, sa, flags,
                    crcs);
  });
}

}  // namespace

namespace avr_host {

// A slice the device can take: supported syntax, at least a surrogate marker long, and an LDS ring
// (ring_cols: 3 W + 7 records for an MBAFF slice) that fits a workgroup's LDS -- a very wide MBAFF
// picture is stored skip_coded instead of failing the whole file's launch.
bool recodable_candidate(const avr::SliceInfo& s) {
  const int cols = s.h.mbaff && !s.h.field_pic ? 3 * s.h.mb_width + 7 : s.h.mb_width;
  return s.h.supported && s.size >= (size_t)avr::kSurrogateMarkerBytes && avr::shared_bytes(cols) <= kLdsBudget;
}

std::vector<SliceView> views_of(const ParsedFile& pf) {
  std::vector<SliceView> v(pf.slices.size());
  for (size_t i = 0; i < v.size(); i++)
    v[i] = {pf.slices[i].payload(), pf.slices[i].size, recodable_candidate(pf.slices[i]),
            pf.slices[i].file_payload_offset(), pf.slices[i].nal_offset, pf.slices[i].nal_offset + pf.slices[i].nal_size};
  return v;
}

// find_next_coded_block_and_emit_literal (recode.cpp:1275-1297): slice i becomes a cabac block when
// it is recodable (ok[i]), at least a surrogate marker long, and its payload occurs verbatim after
// the previous coded block.  Returns the payload's position in the file per slice (null = skip).
// With `escapes`, a slice the search misses gets a second chance (the parallel models' opt-in
// format, Block field 17): E = escape(payload) -- 7.4.1 from a clean state -- is searched from the
// end of the previous coded block, inside the slice's own NAL only: E holds a 00 00 03 trigram, so a
// miss costs find_payload a binary search, and a hit anywhere else would put the surrogate where
// the decompressor's parse does not meet this slice.  A hit makes the block stand for E: size + k
// bytes of the file.  A NAL whose escaping is not the canonical one, or whose slice header leaves zero bytes in
// front of the payload (the file's 03 is then not where the clean-state escape puts it), has no E in
// it and stays skip_coded.
std::vector<const uint8_t*> segment(const uint8_t* in, size_t n, const std::vector<SliceView>& sv,
                                    const std::vector<char>& ok, std::vector<uint32_t>* escapes) {
  std::vector<const uint8_t*> found(sv.size(), nullptr);
  if (escapes) escapes->assign(sv.size(), 0);
  TrigramIndex ix;
  // a recorded position is trusted only where the payload's bytes stand there (a payload that is a
  // view of the file at that position trivially; a copy -- rank 0's parse arena, another revision
  // of the file -- compared in full, on host threads); else the plain search
  std::vector<char> own_ok(sv.size(), 0);
  {
    std::vector<size_t> chk;
    for (size_t i = 0; i < sv.size(); i++) {
      const uint64_t own = sv[i].file_pos;
      if (!ok[i] || sv[i].size < (size_t)avr::kSurrogateMarkerBytes || own == ~(uint64_t)0 || own + sv[i].size > n) continue;
      if (sv[i].payload == in + own) own_ok[i] = 1;
      else chk.push_back(i);
    }
    uint64_t bytes = 0;
    for (size_t i : chk) bytes += sv[i].size;
    const unsigned T = bytes < ((uint64_t)64 << 20) ? 1u : bulk_threads();
    auto work = [&](unsigned t) {
      for (size_t k = t; k < chk.size(); k += T) {
        const size_t i = chk[k];
        own_ok[i] = memcmp(in + sv[i].file_pos, sv[i].payload, sv[i].size) == 0;
      }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
  }
  size_t prev_end = 0;
  for (size_t i = 0; i < sv.size(); i++) {
    if (!ok[i] || sv[i].size < (size_t)avr::kSurrogateMarkerBytes) continue;
    const uint64_t own = sv[i].file_pos;
    const uint8_t* f = own_ok[i] && own >= prev_end
                           ? find_before(in, prev_end, (size_t)own, sv[i].payload, sv[i].size)
                           : find_payload(in, n, prev_end, sv[i].payload, sv[i].size, &ix);
    if (f) {
      found[i] = f;
      prev_end = (size_t)(f - in) + sv[i].size;
    } else if (escapes && sv[i].nal_hi > sv[i].nal_lo && sv[i].nal_hi <= n) {
      const std::vector<uint8_t> e = avr::escape(sv[i].payload, sv[i].size);
      if (e.size() == sv[i].size) continue;
      f = find_payload(in, n, std::max(prev_end, sv[i].nal_lo), e.data(), e.size(), &ix, sv[i].nal_hi);
      if (f) {
        found[i] = f;
        (*escapes)[i] = (uint32_t)(e.size() - sv[i].size);
        prev_end = (size_t)(f - in) + e.size();
      }
    }
  }
  return found;
}
std::vector<const uint8_t*> segment(const uint8_t* in, size_t n, const ParsedFile& pf, const std::vector<char>& ok,
                                    std::vector<uint32_t>* escapes) {
  return segment(in, n, views_of(pf), ok, escapes);
}

namespace {
// The unit values of every coded slice from its payload, on host threads: unit u of slice i covers
// payload bytes [q[u - 1], q[u]) -- q from the slice's seams field, none for an uncut slice -- the last
// to the payload's size.  AVR_ERR_INVALID_ARGUMENT for a seams field whose cuts cannot be read or do
// not ascend inside the payload.
int host_unit_crcs(const std::vector<SliceView>& sv, const std::vector<const uint8_t*>& found,
                   const std::vector<std::pair<const uint8_t*, size_t>>* seams, std::vector<std::vector<uint32_t>>* out) {
  struct Job {
    size_t slice, unit;
    const uint8_t* p;
    size_t len;
  };
  std::vector<Job> jobs;
  uint64_t bytes = 0;
  out->assign(sv.size(), {});
  std::vector<uint32_t> q;
  for (size_t i = 0; i < sv.size(); i++) {
    if (!found[i]) continue;
    q.clear();
    if (seams && (*seams)[i].second && !seams_cut_q((*seams)[i].first, (*seams)[i].second, &q)) return AVR_ERR_INVALID_ARGUMENT;
    (*out)[i].assign(q.size() + 1, 0);
    for (size_t u = 0; u <= q.size(); u++) {
      const size_t lo = u ? q[u - 1] : 0, hi = u < q.size() ? q[u] : sv[i].size;
      if (lo > hi || hi > sv[i].size) return AVR_ERR_INVALID_ARGUMENT;
      jobs.push_back({i, u, sv[i].payload + lo, hi - lo});
    }
    bytes += sv[i].size;
  }
  const unsigned T = bytes < ((uint64_t)64 << 20) ? 1u : bulk_threads();
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t k; (k = next.fetch_add(1)) < jobs.size();)
      (*out)[jobs[k].slice][jobs[k].unit] = avr_crc32(0, jobs[k].p, jobs[k].len);
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  return AVR_OK;
}
}  // namespace

// compressor::run's block stream (recode.cpp:1115-1125, 1275-1297) as a Recoded protobuf, written
// once: the blocks' headers in order, their bytes by parallel_copies, into the caller's buffer dst
// (cap bytes; too small: AVR_ERR_INVALID_ARGUMENT with *out_len = the size needed) or, without one,
// into one exactly sized buffer allocated here (*out).
int emit_container(const uint8_t* in, size_t n, const std::vector<SliceView>& sv, const std::vector<const uint8_t*>& found,
                   const std::vector<std::pair<const uint8_t*, size_t>>& recoded, int model, uint8_t** out,
                   size_t* out_len, uint8_t* dst, size_t cap,
                   const std::vector<std::pair<const uint8_t*, size_t>>* seams, const std::vector<uint32_t>* escapes,
                   const FileCrcArg& crc, const UnitCrcArg& units) {
  // unit checksums (Block field 18): per coded slice one value per unit, brought or computed here
  std::vector<std::vector<uint32_t>> own_units;
  if (units.on && !units.values) {
    if (int r = host_unit_crcs(sv, found, seams, &own_units)) return r;
  }
  const std::vector<std::vector<uint32_t>>* unit_values = units.on ? (units.values ? units.values : &own_units) : nullptr;
  bool any_escapes = false, any_seams = false;
  std::vector<avr::PbBlock> blocks;
  blocks.reserve(2 * sv.size() + 1);
  // a checked container: what each block contributes to the file's CRC (fold_file_crc) -- a literal
  // its bytes, a coded block its payload's CRC, an escaped one the size + k file bytes it stands for
  std::vector<CrcItem> items;
  if (crc.on) items.reserve(2 * sv.size() + 1);
  size_t prev_end = 0;
  for (size_t i = 0; i < sv.size(); i++) {
    const SliceView& s = sv[i];
    avr::PbBlock b;
    if (found[i]) {
      avr::PbBlock lit;
      lit.has_literal = true;
      lit.literal = in + prev_end;
      lit.literal_len = (size_t)(found[i] - (in + prev_end));
      blocks.push_back(lit);
      const uint32_t k = escapes ? (*escapes)[i] : 0u;   // the block stands for size + k file bytes
      if (crc.on) {
        items.push_back(CrcItem{lit.literal, lit.literal_len});
        if (k || !crc.crcs) items.push_back(CrcItem{found[i], s.size + k});
        else items.push_back(CrcItem{nullptr, s.size, crc.crcs[i], true});
      }
      prev_end = (size_t)(found[i] - in) + s.size + k;
      if (k) b.has_escapes = any_escapes = true, b.escapes = k;
      b.has_size = true;
      b.size = (int64_t)s.size;
      b.has_parity = true;
      b.length_parity = s.size & 1;
      if (s.size > 1) b.has_last_byte = true, b.last_byte.assign(1, (char)s.payload[s.size - 1]);
      b.has_cabac = true;
      b.cabac = recoded[i].first;
      b.cabac_len = recoded[i].second;
      if (seams && (*seams)[i].second)
        b.has_seams = any_seams = true, b.seams = (*seams)[i].first, b.seams_len = (*seams)[i].second;
      if (unit_values && i < unit_values->size() && !(*unit_values)[i].empty()) {
        b.has_unit_crcs = true;
        for (uint32_t v : (*unit_values)[i])
          for (int k = 0; k < 4; k++) b.unit_crcs.push_back((char)(uint8_t)(v >> (8 * k)));
      }
    } else {
      b.has_skip = true;
      b.skip_coded = true;
      b.has_size = true;
      b.size = (int64_t)s.size;
    }
    blocks.push_back(std::move(b));
  }
  avr::PbBlock lit;
  lit.has_literal = true;
  lit.literal = in + prev_end;
  lit.literal_len = n - prev_end;
  blocks.push_back(lit);
  if (crc.on) items.push_back(CrcItem{lit.literal, lit.literal_len});
  std::vector<uint8_t> md;
  // a container without field 17 keeps the plain tag and the plain bytes; so does a P32 one without
  // field 16, and one with it says so in its tag (P32S / P32SE; P64's seams need none)
  const char* tag = any_seams && model == AVR_MODEL_PARALLEL32 ? avr::split32_version_of(any_escapes)
                    : any_escapes                              ? avr::escaped_version_of_model(model)
                                                               : avr::version_of_model(model);
  if (any_escapes && !tag) return fail(nullptr, AVR_ERR_INVALID_ARGUMENT, "escapes on a model without the field");
  if (crc.on) {
    const std::string version = tag ? tag : "";
    avr::pb_put_metadata(&md, tag ? &version : nullptr, fold_file_crc(&items));
  } else if (tag) {
    avr::pb_put_metadata_version(&md, tag);
  }
  size_t total = md.size();
  for (const auto& b : blocks) total += avr::pb_block_size(b);
  if (dst && total > cap) {
    *out_len = total;
    return AVR_ERR_INVALID_ARGUMENT;
  }
  uint8_t* o = dst ? dst : host_alloc(total);
  if (!o) return AVR_ERR_OUT_OF_MEMORY;
  if (!md.empty()) memcpy(o, md.data(), md.size());
  size_t at = md.size();
  std::vector<avr::PbCopy> copies;
  copies.reserve(2 * blocks.size());
  for (const auto& b : blocks) at = avr::pb_write_block(o, at, b, &copies);
  if (at != total) {
    if (!dst) free(o);
    return fail(nullptr, AVR_ERR_DEVICE, "internal error: container size");
  }
  parallel_copies(copies, o);
  if (out) *out = dst ? nullptr : o;
  *out_len = total;
  return AVR_OK;
}

}  // namespace avr_host

extern "C" {

int avr_assemble_container_args(const avr_assemble_args* a, uint8_t** out, size_t* out_len) {
  if (!a || a->size != sizeof(avr_assemble_args) || !out) return AVR_ERR_INVALID_ARGUMENT;
  const SeamsArg sa{a->seams, a->seams_len, a->seam_offsets, a->seam_lens};
  if (a->descs || a->arena)
    return assemble_parsed(a->file, a->n, a->model, a->descs, a->n_slices, a->arena, a->arena_len, a->status, a->recoded,
                           a->recoded_len, a->offsets, a->lens, out, out_len, nullptr, 0, sa, a->flags, a->crcs);
  if (!a->file || !out_len || a->n_slices < 0 || (a->n_slices && (!a->status || !a->offsets || !a->lens)) ||
      !assemblable(a->model) || (a->seams && a->n_slices && (!a->seam_offsets || !a->seam_lens)))
    return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    ParsedFile pf;
    if (int r = parse_file(nullptr, a->file, a->n, &pf, /*views=*/true)) return r;
    if ((size_t)a->n_slices != pf.slices.size()) return AVR_ERR_INVALID_ARGUMENT;
    return assemble(a->file, a->n, a->model, views_of(pf), a->status, a->recoded, a->recoded_len, a->offsets, a->lens, out,
                    out_len, nullptr, 0, sa, a->flags, a->crcs);
  });
}

int avr_assemble_container_opts(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                const uint8_t* arena, size_t arena_len, const int32_t* status, const uint8_t* recoded,
                                size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, const uint8_t* seams,
                                size_t seams_len, const uint64_t* seam_offsets, const uint32_t* seam_lens,
                                uint32_t flags, uint8_t** out, size_t* out_len) {
  const avr_assemble_args a{sizeof(avr_assemble_args), file, n, model, descs, n_slices, arena, arena_len, status, recoded,
                            recoded_len, offsets, lens, seams, seams_len, seam_offsets, seam_lens, flags, nullptr};
  return avr_assemble_container_args(&a, out, out_len);
}

int avr_assemble_container_seams(const uint8_t* file, size_t n, int model, int n_slices, const int32_t* status,
                                 const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                 const uint32_t* lens, const uint8_t* seams, size_t seams_len,
                                 const uint64_t* seam_offsets, const uint32_t* seam_lens, uint8_t** out,
                                 size_t* out_len) {
  return avr_assemble_container_opts(file, n, model, nullptr, n_slices, nullptr, 0, status, recoded, recoded_len, offsets,
                                     lens, seams, seams_len, seam_offsets, seam_lens, 0, out, out_len);
}

int avr_assemble_container(const uint8_t* file, size_t n, int model, int n_slices, const int32_t* status,
                           const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets, const uint32_t* lens,
                           uint8_t** out, size_t* out_len) {
  return avr_assemble_container_opts(file, n, model, nullptr, n_slices, nullptr, 0, status, recoded, recoded_len, offsets,
                                     lens, nullptr, 0, nullptr, nullptr, 0, out, out_len);
}

int avr_assemble_container_seams_parsed(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs,
                                        int n_slices, const uint8_t* arena, size_t arena_len, const int32_t* status,
                                        const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                        const uint32_t* lens, const uint8_t* seams, size_t seams_len,
                                        const uint64_t* seam_offsets, const uint32_t* seam_lens, uint8_t** out,
                                        size_t* out_len) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  return assemble_parsed(file, n, model, descs, n_slices, arena, arena_len, status, recoded, recoded_len, offsets, lens,
                         out, out_len, nullptr, 0, SeamsArg{seams, seams_len, seam_offsets, seam_lens});
}

int avr_assemble_container_parsed(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                  const uint8_t* arena, size_t arena_len, const int32_t* status,
                                  const uint8_t* recoded, size_t recoded_len, const uint64_t* offsets,
                                  const uint32_t* lens, uint8_t** out, size_t* out_len) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  return assemble_parsed(file, n, model, descs, n_slices, arena, arena_len, status, recoded, recoded_len, offsets, lens,
                         out, out_len, nullptr, 0);
}

int avr_assemble_container_into(const uint8_t* file, size_t n, int model, const avr_slice_desc* descs, int n_slices,
                                const uint8_t* arena, size_t arena_len, const int32_t* status, const uint8_t* recoded,
                                size_t recoded_len, const uint64_t* offsets, const uint32_t* lens, uint8_t* out,
                                size_t out_cap, size_t* out_len) {
  if (!out) return AVR_ERR_INVALID_ARGUMENT;
  return assemble_parsed(file, n, model, descs, n_slices, arena, arena_len, status, recoded, recoded_len, offsets, lens,
                         nullptr, out_len, out, out_cap);
}

int avr_parse_stream_range(const uint8_t* file, size_t n, int lo, int hi, avr_slice_desc** descs, int* n_slices,
                           uint8_t** arena, size_t* arena_len, size_t* work_len, int* max_w, int* max_h) {
  if (!file || !descs || !n_slices || !arena || !arena_len || !work_len || !max_w || !max_h || lo < 0)
    return AVR_ERR_INVALID_ARGUMENT;
  *descs = nullptr;
  *arena = nullptr;
  return guarded(nullptr, [&]() -> int {
    ParsedFile pf;
    if (int r = parse_file(nullptr, file, n, &pf, /*views=*/true)) return r;
    const int total = (int)pf.slices.size();
    const int b = std::min(lo, total), e = hi < 0 ? total : std::max(b, std::min(hi, total));
    // the arena's layout first (append_aligned's: 16-byte aligned payloads, each followed by >= 16
    // zero bytes), then one allocation and the payload copies on host threads
    const size_t ns = (size_t)(e - b);
    std::vector<avr_slice_desc> dv(ns);
    std::vector<avr::PbCopy> copies(ns);
    uint64_t work = 0, at = 0;
    int mw = 1, mh = 1;
    for (size_t i = 0; i < ns; i++) {
      const avr::SliceInfo& s = pf.slices[b + i];
      avr_slice_desc& d = dv[i];
      d = desc_from_header(s);
      d.payload_offset = (at + 15) & ~(uint64_t)15;
      at = d.payload_offset + s.read_limit + 16;
      copies[i] = {(size_t)d.payload_offset, s.payload(), s.read_limit};
      d.payload_size = (uint32_t)s.size;
      d.read_limit = (uint32_t)s.read_limit;
      d.coded = recodable_candidate(s);
      d.file_offset = s.file_payload_offset();
      d.out_capacity = parallel_out_capacity(s.size);
      place_output(&d, &work);
      if (d.coded) mw = std::max(mw, ring_cols(d));   // uncoded slices are never walked
      mh = std::max(mh, d.mb_height);
    }
    const size_t alen = at + 16;
    const size_t dn = sizeof(avr_slice_desc) * ns;
    *descs = (avr_slice_desc*)malloc(dn ? dn : 1);
    *arena = host_alloc(alen);
    if (!*descs || !*arena) {
      free(*descs);
      free(*arena);
      *descs = nullptr;
      *arena = nullptr;
      return AVR_ERR_OUT_OF_MEMORY;
    }
    if (dn) memcpy(*descs, dv.data(), dn);
    parallel_copies(copies, *arena);
    zero_gaps(copies, *arena, 0, alen);
    *n_slices = (int)ns;
    *arena_len = alen;
    *work_len = work;
    *max_w = mw;
    *max_h = mh;
    return AVR_OK;
  });
}

int avr_parse_stream(const uint8_t* file, size_t n, avr_slice_desc** descs, int* n_slices, uint8_t** arena,
                     size_t* arena_len, size_t* work_len, int* max_w, int* max_h) {
  return avr_parse_stream_range(file, n, 0, -1, descs, n_slices, arena, arena_len, work_len, max_w, max_h);
}

int avr_slice_payload_sizes(const uint8_t* file, size_t n, uint32_t** sizes, int* n_slices) {
  if (!file || !sizes || !n_slices) return AVR_ERR_INVALID_ARGUMENT;
  *sizes = nullptr;
  return guarded(nullptr, [&]() -> int {
    ParsedFile pf;
    if (int r = parse_file(nullptr, file, n, &pf, /*views=*/true)) return r;
    *sizes = (uint32_t*)malloc(sizeof(uint32_t) * std::max<size_t>(1, pf.slices.size()));
    if (!*sizes) return AVR_ERR_OUT_OF_MEMORY;
    for (size_t i = 0; i < pf.slices.size(); i++) (*sizes)[i] = (uint32_t)pf.slices[i].size;
    *n_slices = (int)pf.slices.size();
    return AVR_OK;
  });
}

int avr_escape_payload(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* len) {
  if ((!src && n) || !len || (!dst && cap)) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    const std::vector<uint8_t> e = avr::escape(src, n);
    *len = e.size();
    if (e.size() > cap) return AVR_ERR_INVALID_ARGUMENT;
    if (!e.empty()) memcpy(dst, e.data(), e.size());
    return AVR_OK;
  });
}

int avr_container_describe(const uint8_t* in, size_t n, char** json, uint8_t** reserialized, size_t* len) {
  if (!in || !json || !reserialized || !len) return AVR_ERR_INVALID_ARGUMENT;
  *json = nullptr;
  *reserialized = nullptr;
  std::vector<avr::PbBlock> blocks;
  std::string version;
  bool has_md = false;
  avr::PbFileCrc fc;
  if (!avr::pb_parse(in, n, &blocks, &version, &has_md, &fc)) return AVR_ERR_FORMAT;
  static const char* hexd = "0123456789abcdef";
  auto hex = [&](const uint8_t* p, size_t k) {
    std::string h;
    h.reserve(2 * k);
    for (size_t i = 0; i < k; i++) h += hexd[p[i] >> 4], h += hexd[p[i] & 15];
    return h;
  };
  std::string j = "{\"version\": ";
  j += has_md ? "\"" + hex((const uint8_t*)version.data(), version.size()) + "\"" : std::string("null");
  if (fc.present) j += ", \"file_crc\": " + std::to_string(fc.value);
  j += ", \"blocks\": [";
  std::vector<uint8_t> o;
  if (fc.present) avr::pb_put_metadata(&o, fc.has_version ? &version : nullptr, fc.value);
  else if (has_md) avr::pb_put_metadata_version(&o, version);
  for (size_t i = 0; i < blocks.size(); i++) {
    const avr::PbBlock& b = blocks[i];
    std::string e;
    auto add = [&](const std::string& kv) { e += (e.empty() ? "" : ", ") + kv; };
    if (b.has_size) add("\"size\": " + std::to_string(b.size));
    if (b.has_literal) add("\"literal\": \"" + hex(b.literal, b.literal_len) + "\"");
    if (b.has_skip) add(std::string("\"skip_coded\": ") + (b.skip_coded ? "true" : "false"));
    if (b.has_cabac) add("\"cabac\": \"" + hex(b.cabac, b.cabac_len) + "\"");
    if (b.has_parity) add(std::string("\"length_parity\": ") + (b.length_parity ? "true" : "false"));
    if (b.has_last_byte) add("\"last_byte\": \"" + hex((const uint8_t*)b.last_byte.data(), b.last_byte.size()) + "\"");
    if (b.has_seams) add("\"seams\": \"" + hex(b.seams, b.seams_len) + "\"");
    if (b.has_escapes) add("\"escapes\": " + std::to_string(b.escapes));
    if (b.has_unit_crcs) {   // one value per unit: the cut block's count from its seams
      std::vector<uint32_t> q;
      if (b.has_seams && !seams_cut_q(b.seams, b.seams_len, &q)) return AVR_ERR_FORMAT;
      if (b.unit_crcs.size() != 4 * (q.size() + 1)) return AVR_ERR_FORMAT;
      std::string v;
      for (size_t u = 0; u <= q.size(); u++) v += (u ? ", " : "") + std::to_string(b.unit_crc(u));
      add("\"unit_crcs\": [" + v + "]");
    }
    j += (i ? ", {" : "{") + e + "}";
    avr::pb_put_block(&o, b);
  }
  j += "]}";
  *json = (char*)malloc(j.size() + 1);
  *reserialized = (uint8_t*)malloc(o.size() ? o.size() : 1);
  if (!*json || !*reserialized) {
    free(*json);
    free(*reserialized);
    *json = nullptr;
    *reserialized = nullptr;
    return AVR_ERR_OUT_OF_MEMORY;
  }
  memcpy(*json, j.c_str(), j.size() + 1);
  if (!o.empty()) memcpy(*reserialized, o.data(), o.size());
  *len = o.size();
  return AVR_OK;
}

}  // extern "C"
