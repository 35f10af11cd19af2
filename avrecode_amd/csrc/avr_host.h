// Host-side types and helpers shared by the translation units of libavrecode (internal).  No HIP
// here: avr_host.cpp, avr_seams.cpp, avr_plan.cpp (the decompress planner), avr_cplan.cpp (the
// compress planner) and avr_assemble.cpp compile without ROCm, and all but the last link without
// the device library (tests/native/plan_fuzz.cpp, cplan_check.cpp).  The one-line rules several
// units share (the output capacities, the last-byte rule) are inline here, so using one adds no
// link dependency.
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

// Output space of a slice of `size` payload bytes: the parallel models' compress, the reference
// model's compress.
inline uint32_t parallel_out_capacity(size_t size) { return (uint32_t)(size * 2 + 256); }
inline uint32_t reference_out_capacity(size_t size) { return (uint32_t)(size * 4 + 4096); }
// The bin trace of the hooks surface: 2 bytes per bin (H.264 bounds a slice's bins by ~32/3 per
// payload byte plus a per-macroblock allowance, 7.4.2.2) and 12 bytes of map events per residual
// block (<= 51 per macroblock).
inline uint32_t trace_out_capacity(size_t size, int mb_width, int mb_height) {
  return (uint32_t)std::min<uint64_t>(0xfffffff0ull, 32ull * size + 1280ull * mb_width * mb_height + 8192);
}

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

// ------------------------------------------------------------------ avr_cplan.cpp: the compress planner
// A parsed slice taken into a plan (returns its index): the header's descriptor, and -- coded -- its
// payload in the arena, its sizes, out_capacity bytes of output and its columns of the LDS ring.
// An uncoded slice of a reference-model plan is never walked: it only turns the frames over.
int plan_slice(Plan* plan, const avr::SliceInfo& s, uint32_t out_capacity, bool coded = true);

// The chained model's rule: a fresh model before every AVR_CHAIN_SLICES-th coded slice of a file.
// Chain c starts at slice first[c], the slice holding the (AVR_CHAIN_SLICES c)-th coded slice
// (uncoded slices before it stay in chain c - 1, where they only turn the old chain's frames
// over); first.back() = the slice count.  Compress and decompress cut by this one function.
std::vector<int> chain_starts(const std::vector<char>& coded);
// The file whose slices are plan->descs[n0 ..] joins file_first: its start, and (chained) the
// starts of its later chains -- each a "file" of the sequential launch (estimators, frames).
void append_file_chains(Plan* plan, size_t n0, bool chained);

// One range of a parsed file appended to a reference-model plan: every slice of [lo, hi), the
// coded ones (coded[i], per slice of the file) with their payloads, then the range's chains in
// file_first (the caller closes file_first after the last range).  idx (optional): (file, slice)
// per descriptor.
void reference_plan(Plan* rp, const ParsedFile& pf, int lo, int hi, const std::vector<char>& coded, bool chained,
                    int file = 0, std::vector<std::pair<int, int>>* idx = nullptr);

// Where a slice's re-coded bytes come from (the parallel models' compress), or a container block's
// regenerated bytes (decompress): nowhere, entry `index` of the batch plan, or split slice `index`.
struct Route {
  enum Kind : uint8_t { kNone, kBatch, kSplit } kind = kNone;
  int index = 0;
};
// DecJob::desc_of_block's encoding
inline Route route_of_block(int k) {
  return k >= 0 ? Route{Route::kBatch, k} : k <= -2 ? Route{Route::kSplit, -2 - k} : Route{};
}
// The parallel models' candidate pass over parsed files (st[f] != 0: the parse failed): every
// recodable candidate goes to the batch plan, or -- a long slice, split_slot at split_bytes -- to
// the split job (its slice, and a descriptor holding the header's fields and payload_size).
void plan_candidates(const std::vector<ParsedFile>& pf, const std::vector<int32_t>& st, size_t split_bytes, Plan* batch,
                     std::vector<const avr::SliceInfo*>* split_sl, std::vector<avr_slice_desc>* split_d,
                     std::vector<std::vector<Route>>* route);

// [lo, hi) of rank's contiguous range of units weighted w: shard.partition's rule (the owner of a
// unit is the rank its byte-prefix midpoint falls in), so both sides cut identically.
std::pair<int, int> partition_range(const std::vector<double>& w, int world, int rank);

// One rank's outputs over its slice range [lo, hi) of the file (compress) or of the container's
// plan (decompress): per slice a status and its bytes (blob + offsets[k], lens[k]).
struct ChainRangeOut {
  int lo = 0, hi = 0;
  std::vector<int32_t> status;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lens;
  std::vector<uint8_t> blob;
};
// descs / res / out: a range's plan after its run (slice lo first).  Status 0 with its bytes for
// a coded slice that came out, failed(its status) for one that did not, `uncoded` for the rest.
void pack_range(int lo, const std::vector<avr_slice_desc>& descs, const std::vector<avr_slice_result>& res,
                const uint8_t* out, int32_t uncoded, int32_t (*failed)(int32_t), ChainRangeOut* o);

// Does the parallel reference-model compress beat one workgroup per file on this plan?
bool rmode_parallel_pays(const Plan& plan);
// Frame metadata generations of a reference-model plan for the parallel pass: per slice k the
// buffer offsets of its frame's generation (goff[2k]; bit 0: the first field of its frame) and of
// the other frame's (goff[2k + 1], -1: none), and the bytes of all generations.  False: the plan
// is left to the sequential kernel.
bool rmode_generations(const Plan& plan, std::vector<int64_t>* goff, int64_t* frame_bytes);

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
// A checked container (Recoded.Metadata field 16, the file's CRC-32): write the field, with the
// payload CRC of slice i from crcs[i] where the caller brings them (a device computed them; read for
// coded blocks only, and trusted) or from the payloads on host threads.
struct FileCrcArg {
  bool on = false;
  const uint32_t* crcs = nullptr;
};
// Unit checksums (Block field 18, include/avrecode.h, avr_set_unit_checksums): write the field on
// every coded block -- slice i's values from (*values)[i] where the caller brings them (a device
// computed them over the payload arena; empty: none for that slice) or from the payload on host
// threads, a cut block's units read from its seams field.
struct UnitCrcArg {
  bool on = false;
  const std::vector<std::vector<uint32_t>>* values = nullptr;
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
                   const std::vector<uint32_t>* escapes = nullptr, const FileCrcArg& crc = FileCrcArg(),
                   const UnitCrcArg& units = UnitCrcArg());

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
bool seams_cut_q(const uint8_t* p, size_t n, std::vector<uint32_t>* q);   // the cuts' q only, no descriptor needed
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
  bool has_crc = false;              // Recoded.Metadata field 16: the file's CRC-32 (a checked container)
  uint32_t file_crc = 0;
  // Block field 18 (unit checksums): per block, whether it carries the field and its unit values
  // combined in order -- the CRC-32 of the slice's payload, which every splice compares with the
  // patched CRC of the slice's regenerated bytes.  Empty: no block has the field.
  std::vector<char> block_checked;
  std::vector<uint32_t> block_crc;
  bool unit_checked(size_t i) const { return i < block_checked.size() && block_checked[i]; }
};

// sp: where the pieces of split blocks go (nullptr: such a container is refused -- the sharded and
// hooks paths decompress slices, not pieces)
int decompress_setup(ErrSink* c, const uint8_t* in, size_t n, DecJob* j, Plan* plan, SplitPlan* sp = nullptr);

// The last-byte rule (x264 padding correction, recode.cpp:1345-1356) on a slice regenerated as `len`
// bytes: the block's last_byte replaces its last byte, or -- the length's parity differs from the
// block's -- is appended.  (The compress side's form, from the payload: last_byte_patch.)
enum class LastByte { kKeep, kReplace, kAppend };
inline LastByte last_byte_rule(const avr::PbBlock& b, size_t len) {
  if (!b.has_parity || !b.has_last_byte || b.last_byte.empty()) return LastByte::kKeep;
  if ((int)b.length_parity != (int)(len & 1)) return LastByte::kAppend;
  return len ? LastByte::kReplace : LastByte::kKeep;
}
// the rule applied to the len regenerated bytes at the end of *v
template <class V>
void patch_last_byte(const avr::PbBlock& b, size_t len, V* v) {
  const LastByte r = last_byte_rule(b, len);
  if (r == LastByte::kAppend) v->push_back((uint8_t)b.last_byte[0]);
  else if (r == LastByte::kReplace) v->back() = (uint8_t)b.last_byte[0];
}

// ------------------------------------------------------------------ avr_host.cpp: checked containers
// The file's CRC-32 (Recoded.Metadata field 16; avr_crc32 / avr_crc32_combine, include/avrecode.h)
// folded from its blocks in file order -- stated once, for the writer (emit_container) and every
// splice.  An item is what one block contributes to the file: len bytes whose CRC the caller brings
// (known: a device computed it over a slice's payload or regenerated bytes) or that stand at p and
// are CRC'd here on host threads, a long one cut into chunks (literals: parameter sets, headers,
// uncoded slices; an escaped block's bytes; every slice of a caller without device values).  rule:
// the last-byte rule then applied to the CRC of a regenerated slice instead of to its bytes --
// kAppend one more byte, kReplace the byte table's entry for the difference of the two last bytes
// (two messages of one length that differ in the last byte differ by the raw CRC of that
// difference), kKeep nothing.
struct CrcItem {
  const uint8_t* p = nullptr;
  uint64_t len = 0;
  uint32_t crc = 0;
  bool known = false;
  LastByte rule = LastByte::kKeep;
  uint8_t last_byte = 0, regen_last = 0;   // the block's last_byte; kReplace: the regenerated last byte
  bool in_file = true;   // false: a value of its own beside the file's fold (an escaped block's unescaped bytes)
};
// The two steps of the fold.  resolve: every item's crc and len made final -- the bytes nobody has
// CRC'd yet on host threads, then the last-byte rule on the value (rule becomes kKeep).  combine: the
// in_file items of a resolved list, in order.  fold_file_crc = both.
void resolve_crc_items(std::vector<CrcItem>* items);
uint32_t combine_crc_items(const std::vector<CrcItem>& items);
uint32_t fold_file_crc(std::vector<CrcItem>* items);
// a coded block's item: its len regenerated bytes at p (read for kReplace's one byte, and for the CRC
// unless the caller brings it)
inline CrcItem crc_item_of_slice(const avr::PbBlock& b, const uint8_t* p, size_t len, const uint32_t* crc) {
  CrcItem it;
  it.p = p;
  it.len = len;
  it.known = crc != nullptr;
  if (crc) it.crc = *crc;
  it.rule = last_byte_rule(b, len);
  if (it.rule != LastByte::kKeep) it.last_byte = (uint8_t)b.last_byte[0];
  if (it.rule == LastByte::kReplace) it.regen_last = p[len - 1];
  return it;
}

// decompressor::run's output (recode.cpp:1338-1357): the literals and the regenerated slices in
// block order, each slice patched by the last-byte rule, then -- a block with field 17 -- escaped:
// the patch decides the slice's last byte and length, and both can change what is inserted before
// that byte.
// slice(route, &p, &len) gives a coded block's regenerated bytes and returns its status.
// A checked container (j.has_crc) is checked here: crc_of(route, &crc) gives the CRC of those len
// bytes where a device computed it (false: from the bytes, on host threads), and a file whose fold
// is not the container's value is AVR_ERR_CHECKSUM.
// So is every block with unit checksums (Block field 18, j.block_crc): its values combined against the
// patched CRC of the slice's regenerated, unescaped bytes -- the same crc_of values or bytes -- with or
// without the file's field; AVR_ERR_CHECKSUM names the block.
template <class Slice, class Crc>
int splice_job(ErrSink* c, const DecJob& j, Slice&& slice, std::vector<uint8_t>* o, Crc&& crc_of) {
  o->reserve(j.stream.size());
  std::vector<CrcItem> items;
  std::vector<std::pair<size_t, size_t>> unit_checks;   // (item, block): blocks with field 18
  if (j.has_crc || !j.block_checked.empty()) items.reserve(j.blocks.size());
  for (size_t i = 0; i < j.blocks.size(); i++) {
    const avr::PbBlock& b = j.blocks[i];
    if (b.has_literal) {
      o->insert(o->end(), b.literal, b.literal + b.literal_len);
      if (j.has_crc) items.push_back(CrcItem{b.literal, b.literal_len});
      continue;
    }
    if (!b.has_cabac) continue;
    const int k = j.desc_of_block[i];
    if (k == -1) return fail(c, AVR_ERR_FORMAT, "Not all blocks were decoded.");
    const uint8_t* p = nullptr;
    size_t len = 0;
    if (int stt = slice(route_of_block(k), &p, &len))
      return fail(c, AVR_ERR_FORMAT, "block " + std::to_string(i) + ": slice " + std::to_string(k) + " failed to decode (" +
                                         std::to_string(stt) + ")");
    const size_t o0 = o->size();
    o->insert(o->end(), p, p + len);
    patch_last_byte(b, len, o);
    if (b.has_escapes) {
      const std::vector<uint8_t> e = avr::escape(o->data() + o0, o->size() - o0);
      if (e.size() - (o->size() - o0) != b.escapes)
        return fail(c, AVR_ERR_FORMAT, "slice " + std::to_string(k) + ": escape count differs from the block's");
      o->resize(o0);
      o->insert(o->end(), e.begin(), e.end());
      if (j.has_crc) items.push_back(CrcItem{nullptr, e.size(), avr_crc32(0, e.data(), e.size()), true});
    }
    if ((j.has_crc && !b.has_escapes) || j.unit_checked(i)) {   // the unescaped bytes' patched CRC
      uint32_t crc = 0;
      const bool have = crc_of(route_of_block(k), &crc);
      if (j.unit_checked(i)) unit_checks.push_back({items.size(), i});
      items.push_back(crc_item_of_slice(b, p, len, have ? &crc : nullptr));
      items.back().in_file = j.has_crc && !b.has_escapes;
    }
  }
  resolve_crc_items(&items);
  for (const auto& uc : unit_checks)
    if (items[uc.first].crc != j.block_crc[uc.second])
      return fail(c, AVR_ERR_CHECKSUM, "block " + std::to_string(uc.second) +
                                           ": the regenerated slice is not the one its unit checksums were made from (CRC-32)");
  if (j.has_crc && combine_crc_items(items) != j.file_crc)
    return fail(c, AVR_ERR_CHECKSUM, "the container decoded to a file that is not the file it was made from (CRC-32)");
  return AVR_OK;
}

}  // namespace avr_host

// ------------------------------------------------------------------ avr_plan.cpp: the plan handle
// decompressor::run (recode.cpp:1338-1409) cut in two around the device work: load = read_packet's
// surrogate stream parsed and matched to the container's coded blocks (decompress_setup in layout
// mode: descs and the arena layout, no bytes copied), then the arena written where the caller wants
// it, and the splice of the regenerated slices with the literals and the last-byte patch
// (recode.cpp:1345-1356).  A handle keeps its scratch (the surrogate stream) for the next load.
struct avr_dec_plan {
  avr_host::DecJob job;
  avr_host::Plan plan;
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
  avr_host::Bytes recs;            // the seam records, rec_stride apart
  size_t rec_stride = 0;
  // file coordinates, from the container alone (range reads): block i stands for file bytes
  // [block_off[i], block_off[i + 1]); a piece plan also knows block i's units, [unit_first[i],
  // unit_first[i + 1]), and where in its slice each unit's bytes start (unit_q0)
  std::vector<uint64_t> block_off;
  std::vector<int> unit_first;
  std::vector<uint32_t> unit_q0;
  bool escapes = false;            // some block carries field 17
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
    block_off.clear();
    unit_first.clear();
    unit_q0.clear();
    escapes = false;
  }
};

namespace avr_host {

// The range planner (include/avrecode.h, avr_dec_plan_range): a window of the file as the units to
// regenerate, the copies that lay it out and the per-unit checks.  No device.
// the best of 16 / 64 / 256 KiB for the gather launch alone over a whole-file window of a 298 MB 4K
// stream (scripts/reader_probe.py, profiles/reader_probe.json; DESIGN §2, "Range reads")
constexpr uint32_t kRangeSpanBytes = 16384;
struct RangePlan {
  avr_range_info info{};
  std::vector<avr_span> spans;
  std::vector<avr_range_tail> tails;
};
int plan_range(const avr_dec_plan* h, uint64_t off, uint64_t len, uint32_t span_cap, RangePlan* rp);
// the block holding file byte off (off < the file's size)
size_t block_of_offset(const avr_dec_plan* h, uint64_t off);

}  // namespace avr_host
