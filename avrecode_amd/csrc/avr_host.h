// Host-side types and helpers shared by the translation units of libavrecode (internal).  No HIP
// here: avr_host.cpp, avr_seams.cpp, avr_plan.cpp and avr_assemble.cpp compile without ROCm, and the
// first three link without the device library (tests/native/plan_fuzz.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/avrecode.h"
#include "avr_front.h"
#include "avr_records.h"

namespace avr {
// LDS of one slice workgroup: defined in avr_kernels.hip from the walker's struct sizes
size_t shared_bytes(int max_mb_width);
}  // namespace avr

namespace avr_host {

// Where a call leaves its error text (avr_last_error): the base of avr_ctx, so that host code needs
// no complete avr_ctx; null for the entry points that take no context.
struct ErrSink {
  std::string err;
};
int fail(ErrSink* c, int code, const std::string& msg);
// No C++ exception crosses the C ABI: the entry points that build host containers run their body
// through guarded(), which turns an allocation failure into AVR_ERR_OUT_OF_MEMORY.
template <class F>
int guarded(ErrSink* c, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(c, AVR_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(c, AVR_ERR_DEVICE, std::string("internal error: ") + e.what());
  }
}

double now_s();

// Model modes (include/avrecode.h): the reference model, and the parallel model on the reference's
// arithmetic_code<uint64_t, uint8_t> (PARALLEL) or on the optional 32-bit P32 coder (PARALLEL32).
inline bool valid_model(int m) {
  return m == AVR_MODEL_REFERENCE || m == AVR_MODEL_PARALLEL || m == AVR_MODEL_PARALLEL32 || m == AVR_MODEL_CHAINED;
}
inline bool parallel_model(int m) { return m == AVR_MODEL_PARALLEL || m == AVR_MODEL_PARALLEL32; }
// the reference model over a whole file, or in chains of AVR_CHAIN_SLICES coded slices
inline bool reference_model(int m) { return m == AVR_MODEL_REFERENCE || m == AVR_MODEL_CHAINED; }
// models whose per-slice outputs come from several ranks and are assembled on one: the parallel
// models (slice ranges) and the chained model (chain ranges); the reference model is one unit
inline bool assemblable(int m) { return parallel_model(m) || m == AVR_MODEL_CHAINED; }
inline uint32_t coder_flag(int m) { return m == AVR_MODEL_PARALLEL32 ? avr::kFlagP32 : 0u; }

// A byte vector whose resize() leaves new bytes uninitialised (multi-GB buffers that are written
// right after: no memset pass first).
template <class T>
struct DefaultInit : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = DefaultInit<U>;
  };
  DefaultInit() = default;
  template <class U>
  DefaultInit(const DefaultInit<U>&) {}
  template <class U>
  void construct(U* p) {
    ::new ((void*)p) U;
  }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    ::new ((void*)p) U(std::forward<A>(a)...);
  }
};
typedef std::vector<uint8_t, DefaultInit<uint8_t>> Bytes;

struct Plan {
  std::vector<avr_slice_desc> descs;
  Bytes arena;   // payloads (compress) or recoded streams (decompress)
  // decompress_setup with layout_only: the arena is not built; its byte copies are listed in
  // arena_copies (dst in the arena, source in the container) and its length in arena_end
  bool layout_only = false;
  std::vector<avr::PbCopy> arena_copies;
  uint64_t arena_end = 0;
  int max_w = 1;
  // sequential (reference-model) plans over several files: file f is descs[file_first[f] ..
  // file_first[f + 1]); empty = one file
  std::vector<int> file_first;
  int n_files() const { return file_first.empty() ? 1 : (int)file_first.size() - 1; }
  int file_begin(int f) const { return file_first.empty() ? 0 : file_first[f]; }
  int file_end(int f) const { return file_first.empty() ? (int)descs.size() : file_first[f + 1]; }
  // field pictures / MBAFF frames present: launches add the field-capable kernels (kFlagFields)
  bool fields() const {
    for (const auto& d : descs)
      if (d.structure != AVR_STRUCT_FRAME) return true;
    return false;
  }
  // both kinds of slice: the field kernel has work beside the progressive one (avr::FieldLane)
  bool mixed() const {
    bool f = false, p = false;
    for (const auto& d : descs) (d.structure != AVR_STRUCT_FRAME ? f : p) = true;
    return f && p;
  }
};

template <class V>
void append_aligned(V* arena, const uint8_t* p, size_t n, size_t extra, uint64_t* off) {
  size_t o = (arena->size() + 15) & ~(size_t)15;
  arena->resize(o + n + extra, 0);
  if (n) memcpy(arena->data() + o, p, n);
  *off = o;
}

// EdgeRec slots of the LDS ring a slice needs (launch max_mb_width): an MBAFF slice keeps its pair
// edges and records there too (Walker::pair_edge)
inline int ring_cols(const avr_slice_desc& d) { return d.structure == AVR_STRUCT_MBAFF ? 3 * d.mb_width + 7 : d.mb_width; }

avr_slice_desc desc_from_header(const avr::SliceInfo& s);

// A slice's place in a batch's output buffer: out_capacity bytes at the next 16-byte boundary
// (*total: the buffer's length so far).
inline void place_output(avr_slice_desc* d, uint64_t* total) {
  d->out_offset = *total;
  *total += ((uint64_t)d->out_capacity + 15) & ~15ull;
}

struct ParsedFile {
  std::vector<avr::SliceInfo> slices;
};

// views: slices without emulation-prevention bytes point into `in` instead of holding a copy (the
// caller keeps `in` alive while it uses pf)
int parse_file(ErrSink* c, const uint8_t* in, size_t n, ParsedFile* pf, bool views = false,
               const avr::SkipRanges* skips = nullptr);

// ------------------------------------------------------------------ avr_host.cpp: bulk host work
// Host threads for one file's bulk steps (trigram index, container copies): up to 16, or 1 inside a
// parallel_files worker, which already spreads the files over the thread budget (a corpus of large
// files would otherwise start ~16 x 16 threads at once).
extern thread_local bool tl_in_file_pool;
unsigned bulk_threads();
uint8_t* host_alloc(size_t n);
void parallel_copies(const std::vector<avr::PbCopy>& jobs, uint8_t* base, uint8_t fill = 0);
// the zero bytes between and after copy jobs laid out in ascending order within base[from, end)
void zero_gaps(const std::vector<avr::PbCopy>& jobs, uint8_t* base, uint64_t from, uint64_t end);

// fn(f) for f in [0, nf) on up to 16 host threads (independent files: segmentation, containers).
// An exception in a worker (allocation failure) is rethrown here, on the caller's thread, so that
// guarded() still turns it into a status.
template <class F>
void parallel_files(int nf, F&& fn) {
  const unsigned T = (unsigned)std::min<int>(nf, (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (T <= 1) {
    for (int f = 0; f < nf; f++) fn(f);
    return;
  }
  std::atomic<int> next{0};
  std::exception_ptr err;
  std::mutex mu;
  auto work = [&]() {
    const bool was = tl_in_file_pool;
    tl_in_file_pool = true;   // each file's own bulk steps stay on this thread
    try {
      for (int f; (f = next.fetch_add(1)) < nf;) fn(f);
    } catch (...) {
      std::lock_guard<std::mutex> g(mu);
      if (!err) err = std::current_exception();
      next = nf;
    }
    tl_in_file_pool = was;
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  if (err) std::rethrow_exception(err);
}

// ------------------------------------------------------------------ avr_assemble.cpp: the container writer
// A slice as the container writer sees it: its payload (init_decoder's buf, size) and whether the
// device may re-code it (recodable_candidate).
struct SliceView {
  const uint8_t* payload;
  size_t size;
  bool candidate;
  uint64_t file_pos;   // where the payload stands verbatim in the file (the parse knows), or ~0
  size_t nal_lo = 0, nal_hi = 0;   // the slice's own NAL in the file, [lo, hi) (0, 0: not known)
};
bool recodable_candidate(const avr::SliceInfo& s);
std::vector<SliceView> views_of(const ParsedFile& pf);
// escapes (the parallel models' opt-in second chance, AVR_ASSEMBLE_ESCAPED): a slice the search
// does not find verbatim is searched as escape(payload) inside its own NAL; (*escapes)[i] = the
// bytes that escape inserted when found[i] is such a hit (the block stands for size + that many
// file bytes), else 0.  Null: today's segmentation.
std::vector<const uint8_t*> segment(const uint8_t* in, size_t n, const std::vector<SliceView>& sv,
                                    const std::vector<char>& ok, std::vector<uint32_t>* escapes = nullptr);
std::vector<const uint8_t*> segment(const uint8_t* in, size_t n, const ParsedFile& pf, const std::vector<char>& ok,
                                    std::vector<uint32_t>* escapes = nullptr);
int emit_container(const uint8_t* in, size_t n, const std::vector<SliceView>& sv, const std::vector<const uint8_t*>& found,
                   const std::vector<std::pair<const uint8_t*, size_t>>& recoded, int model, uint8_t** out,
                   size_t* out_len, uint8_t* dst = nullptr, size_t cap = 0,
                   const std::vector<std::pair<const uint8_t*, size_t>>* seams = nullptr,
                   const std::vector<uint32_t>* escapes = nullptr);

// ------------------------------------------------------------------ avr_seams.cpp: the seams codec
struct SeamCe {
  uint32_t q, low, outstanding, cache, range;
  int32_t queue;
};
// the pieces of a split block: per cut a device record (decompress fields), the pieces' streams
struct SeamsDecoded {
  int cuts = 0;
  std::vector<uint32_t> piece_len, first_mb, q;
  std::vector<uint8_t> recs;   // cuts records of rec_stride bytes
};
bool seam_encoder(const uint8_t* pay, size_t n, uint64_t bitpos, uint32_t offset, uint32_t range, SeamCe* s);
bool seams_encode(const std::vector<const avr::SeamRec*>& recs, const std::vector<SeamCe>& ce, const avr_slice_desc& d,
                  const std::vector<uint32_t>& piece_len, std::vector<uint8_t>* out);
bool seams_decode(const uint8_t* p, size_t n, const avr_slice_desc& d, size_t rec_stride, SeamsDecoded* sd);
bool splice_pieces(const avr_slice_desc* d, const avr_slice_result* r, const uint8_t* out, const std::vector<uint32_t>& q,
                   std::vector<uint8_t>* o);
void last_byte_patch(std::vector<uint8_t>* o, const uint8_t* payload, size_t size);
// The long-slice split's rule and sizes: whether the parallel model's compress takes d (payload_size
// set) through the split walk at split_bytes, the cut records of its slot and its output space.
bool split_slot(const avr_slice_desc& d, size_t split_bytes, uint64_t* cap, uint64_t* out_capacity);
// The seams step over what a split walk has left (the arrays of avr_seams_build, include/avrecode.h,
// with rec_stride > 0 and n_recs records in recs): every index checked before anything is read
// through it, every cut checked against seam_encoder (check_cuts), the pieces' lengths, Block field 16.
// A slice whose indices do not fit the arrays gets status `misfit`, or with misfit 0 (the caller
// brought the arrays) fails the call: AVR_ERR_INVALID_ARGUMENT.  AVR_ERR_OUT_OF_MEMORY: zlib failed.
struct SliceSeams {
  int32_t status = 0;           // res[k].status, misfit, or AVR_SLICE_CODER: a cut the host does not restate
  std::vector<uint8_t> field;   // status 0 and at least one cut
  std::vector<uint32_t> piece_len, first_mb, q;   // status 0, in a slot: per piece; per cut
};
int seams_build(const avr_slice_desc* descs, int n, const uint8_t* arena, size_t arena_len, const avr_slice_result* res,
                const avr_split_slot* slots, const uint32_t* cuts, const uint32_t* piece_end, int n_recs,
                const uint8_t* recs, size_t rec_stride, bool check_cuts, int32_t misfit, std::vector<SliceSeams>* out);

// ------------------------------------------------------------------ avr_plan.cpp: the decompress planner
// A split block (the parallel model's long-slice split): its pieces in the split plan, the cuts' q
// (piece i's bytes end at q[i]), the spliced regenerated bytes after the run
struct SplitBlock {
  int block = -1, first = 0, pieces = 0;
  std::vector<uint32_t> q;
  std::vector<uint8_t> regen;
  int32_t status = 0;
  avr_slice_result bill{};
};
struct SplitPlan {
  Plan plan;                        // the pieces (descs, their re-coded streams in the arena)
  std::vector<avr::PieceCtl> ctl;
  Bytes recs;                       // the cut records, rec_stride apart
  size_t stride = avr::seam_rec_bytes(kMringCols);
  static constexpr int kMringCols = avr::kMringCols;   // widest picture a record holds
};
// The pieces of a cut slice appended to a plan: copies of its descriptor d, piece i's stream
// (piece_len[i] bytes of `streams`, one after the other) in the arena, starting at cut i - 1's
// first_mb and record rec0 + i - 1 (the slice's own start for piece 0), out_capacity(i) bytes of output.
template <class Cap>
void append_pieces(Plan* plan, std::vector<avr::PieceCtl>* ctl, const avr_slice_desc& d, const uint8_t* streams,
                   const std::vector<uint32_t>& piece_len, const std::vector<uint32_t>& first_mb, uint32_t rec0,
                   Cap&& out_capacity) {
  const size_t cuts = first_mb.size();
  uint64_t off = 0;
  for (size_t i = 0; i <= cuts; i++) {
    avr_slice_desc pd = d;
    if (i) pd.first_mb = (int32_t)first_mb[i - 1];
    append_aligned(&plan->arena, streams + off, piece_len[i], 16, &pd.payload_offset);
    off += piece_len[i];
    pd.payload_size = pd.read_limit = piece_len[i];
    pd.out_capacity = out_capacity(i);
    plan->max_w = std::max(plan->max_w, pd.mb_width);
    plan->descs.push_back(pd);
    ctl->push_back(avr::PieceCtl{i ? (int32_t)(rec0 + i - 1) : -1, i < cuts ? first_mb[i] - (uint32_t)pd.first_mb : 0u, -1, 0});
  }
}
struct DecJob {
  std::vector<avr::PbBlock> blocks;
  Bytes stream;                      // read_packet's stream: literals + surrogate blocks
  bool parallel = false;
  int model = AVR_MODEL_REFERENCE;   // from Recoded.Metadata.version
  std::vector<int> desc_of_block;    // plan index per coded block (-1: none; <= -2: split block -2 - k)
  std::vector<SplitBlock> splits;
};

// sp: where the pieces of split blocks go (nullptr: such a container is refused -- the sharded and
// hooks paths decompress slices, not pieces)
int decompress_setup(ErrSink* c, const uint8_t* in, size_t n, DecJob* j, Plan* plan, SplitPlan* sp = nullptr);

// decompressor::run's output (recode.cpp:1338-1357): the literals and the regenerated slices in
// block order, each slice patched by the last-byte rule (x264 padding correction, 1345-1356), then
// -- a block with field 17 -- escaped: the patch decides the slice's last byte and length, and both
// can change what is inserted before that byte.
// slice(k, &p, &len) gives plan slice k's regenerated bytes and returns its status.
template <class Slice>
int splice_job(ErrSink* c, const DecJob& j, Slice&& slice, std::vector<uint8_t>* o) {
  o->reserve(j.stream.size());
  for (size_t i = 0; i < j.blocks.size(); i++) {
    const avr::PbBlock& b = j.blocks[i];
    if (b.has_literal) {
      o->insert(o->end(), b.literal, b.literal + b.literal_len);
      continue;
    }
    if (!b.has_cabac) continue;
    const int k = j.desc_of_block[i];
    if (k == -1) return fail(c, AVR_ERR_FORMAT, "Not all blocks were decoded.");
    const uint8_t* p = nullptr;
    size_t len = 0;
    if (int stt = slice(k, &p, &len))
      return fail(c, AVR_ERR_FORMAT, "slice " + std::to_string(k) + " failed to decode (" + std::to_string(stt) + ")");
    const size_t o0 = o->size();
    o->insert(o->end(), p, p + len);
    if (b.has_parity && b.has_last_byte && !b.last_byte.empty()) {
      const size_t n = o->size() - o0;
      if ((int)b.length_parity != (int)(n & 1)) o->push_back((uint8_t)b.last_byte[0]);
      else if (n) o->back() = (uint8_t)b.last_byte[0];
    }
    if (b.has_escapes) {
      const std::vector<uint8_t> e = avr::escape(o->data() + o0, o->size() - o0);
      if (e.size() - (o->size() - o0) != b.escapes)
        return fail(c, AVR_ERR_FORMAT, "slice " + std::to_string(k) + ": escape count differs from the block's");
      o->resize(o0);
      o->insert(o->end(), e.begin(), e.end());
    }
  }
  return AVR_OK;
}

}  // namespace avr_host
