// The libavcodec-hooks surface of the C ABI (include/avrecode.h, avr_hooks_* / avr_hook_*).
// The reference's hook objects (compressor::cabac_decoder recode.cpp:1134-1268,
// decompressor::cabac_decoder 1411-1520) answer each bin request by running the model inline.
// Here the device has already done the whole file; the session replays the device's decode-order
// bin trace (MODE_TRACE kernel) to the caller and cross-checks the caller's parse against it.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "avr_ctx.h"
#include "h264_tables.h"

using namespace avr_host;

struct avr_hooks_session;

// A significance map of the device's parse (MODE_TRACE event records): the bins [begin, end) it
// spans and the model state it starts under -- mb_xy and begin_sub_mb's arguments.
struct HookMap {
  uint32_t begin = 0, end = 0;
  int x = 0, y = 0;
  int sub[5] = {0, 0, 0, 0, 0};   // cat, scan8 index, max_coeff, is_dc, chroma422
};

struct avr_hooks_slice {
  avr_hooks_session* sess = nullptr;
  int index = 0;                 // slice index (decode order)
  const uint8_t* trace = nullptr;   // 2 bytes per bin: bin | kind << 1, state byte before it
  size_t nbins = 0, cur = 0;
  const HookMap* maps = nullptr;
  size_t nmaps = 0, map_cur = 0;
  bool sub_open = false;
  int sub_args[5] = {0, 0, 0, 0, 0};
  int coding_type = 0;
};

// Streaming compress session: incremental demux + parse of the bytes fed so far.  Only what is new
// is parsed: an Annex-B NAL unit once the next start code (00 00 00 / 00 00 01, demux_annexb's rule)
// has been fed -- the unit in progress provisionally when a decoder already asks for its slice (a
// later feed that extends it fails the session) -- and an MP4 sample once the moov box and the
// whole sample are in.  Slices come out in decode order exactly as parse_file gives them.
struct StreamIngest {
  avr::StreamParser sp;
  int kind = 0;                 // 0 undecided (< 8 bytes), 1 Annex-B, 2 MP4
  // Annex-B
  size_t scan = 0;              // where the search for the next boundary / start code resumes
  bool in_nal = false;          // a NAL unit started at nal_begin (after its start code)
  size_t nal_begin = 0;
  size_t prov_end = 0;          // the unit in progress was parsed provisionally through here (0: not)
  // MP4
  bool have_layout = false;
  avr::Mp4Layout layout;
  size_t next_sample = 0;
};

struct avr_hooks_session {
  avr_ctx* c = nullptr;
  bool decompress = false;
  std::vector<uint8_t> original;   // the H.264 file
  std::vector<uint8_t> result;     // compress: the container; decompress: the original file
  std::vector<uint8_t> stream;     // decompress: read_packet's stream
  ParsedFile pf;
  std::vector<char> coded;
  std::vector<std::vector<uint8_t>> bins;   // per slice: the device's bins (2 bytes each)
  std::vector<std::vector<HookMap>> maps;    // per slice: its significance maps
  std::vector<avr_hooks_slice> slices;
  size_t next_slice = 0;
  uint64_t next_marker = 1;
  avr_hooks_slice* live = nullptr;  // the slice model hooks refer to (one live CABAC context, recode.cpp:199)
  uint64_t mb_calls = 0;
  int mb_x = -1, mb_y = -1;         // the caller's last mb_xy (h264_model::mb_coord)
  // frame_spec (update_frame_spec, recode.cpp:824-843): the caller's last call and the slice it
  // belonged to; a call made between slices waits for the next init_decoder
  bool fs_have = false, fs_pending = false;
  int fs_num = 0, fs_w = 0, fs_h = 0, fs_slice = -1;
  int pend_num = 0, pend_w = 0, pend_h = 0;
  // streaming compress (avr_hooks_compress_stream_begin): `original` grows by avr_hooks_feed; pf holds
  // the slices parsed from it so far (ing: incremental), traced[i] = slice i's device work is done --
  // its bin trace and, for the parallel model, its final re-coded block (blocks / block_status: the
  // container is assembled from them at avr_hooks_end without another device pass)
  bool streaming = false;
  StreamIngest ing;
  std::vector<char> traced;
  std::vector<std::vector<uint8_t>> blocks;
  std::vector<int32_t> block_status;
  int model = 0;
  // decompress of a parallel-model container, on demand: the container's plan (every coded slice's
  // re-coded block) is made at begin, and a slice is regenerated on the device -- with the coded
  // slices after it that are not yet, up to kLazyBatch -- when init_decoder reaches it; its bins
  // are traced from the regenerated payload (recode.cpp:1435-1449 decodes each bin as FFmpeg asks)
  bool lazy = false;
  DecJob job;
  Plan dplan;
  std::vector<int> plan_of;          // per slice: its dplan index (-1: not coded)
  std::vector<int> block_of;         // per slice: its container block
  std::vector<char> regen_done;
  std::vector<std::vector<uint8_t>> regen;   // per slice: its regenerated payload (last-byte patched)
  std::string err;
  void fail_once(const std::string& m) {
    if (err.empty()) err = m;
  }
};

namespace {

// FFmpeg's state transition for one decoded bin (ff_h264_mlps_state, cabac_code.h:46-48)
uint8_t next_state(uint8_t s, int bin) {
  const int p = s >> 1, mps = s & 1;
  if (bin == mps) return (uint8_t)(2 * (p < 62 ? p + 1 : p) + mps);
  return (uint8_t)(p == 0 ? (s ^ 1) : 2 * avr::kTransIdxLPS[p] + mps);
}

// Device trace (MODE_TRACE kernel) of the slices `which` of hs->pf into hs->bins / hs->maps.
int trace_slices(avr_hooks_session* hs, const std::vector<int>& which) {
  avr_ctx* c = hs->c;
  Plan plan;
  for (const int i : which) {
    const avr::SliceInfo& s = hs->pf.slices[i];
    plan_slice(&plan, s, trace_out_capacity(s.size, s.h.mb_width, s.h.mb_height));
  }
  if (plan.descs.empty()) return AVR_OK;
  std::vector<avr_slice_result> res;
  std::vector<uint8_t> traces;
  if (int r = run_plan(c, 3, false, plan, &res, &traces)) return r;
  for (size_t k = 0; k < plan.descs.size(); k++) {
    const int i = which[k];
    if (res[k].status != 0)
      return fail(c, AVR_ERR_FORMAT, "hooks: device trace of slice " + std::to_string(i) + " failed (" +
                                         std::to_string(res[k].status) + ")");
    // split the records: bins (kinds 0-2) and map events (kind 3, avr_slice_lds.h TRACE_EV_*)
    const uint8_t* t = traces.data() + plan.descs[k].out_offset;
    const size_t len = res[k].out_len;
    std::vector<uint8_t>& b = hs->bins[i];
    std::vector<HookMap>& m = hs->maps[i];
    b.clear();
    m.clear();
    b.reserve(len);
    bool open = false;
    for (size_t at = 0; at + 2 <= len;) {
      if (((t[at] >> 1) & 3) != 3) {
        b.push_back(t[at]);
        b.push_back(t[at + 1]);
        at += 2;
        continue;
      }
      const uint32_t bin_index = (uint32_t)(b.size() / 2);
      if (t[at + 1] == 1 && at + 10 <= len && !open) {
        HookMap h;
        h.begin = bin_index;
        h.x = t[at + 2] | t[at + 3] << 8;
        h.y = t[at + 4] | t[at + 5] << 8;
        h.sub[0] = t[at + 6], h.sub[1] = t[at + 7], h.sub[2] = t[at + 8];
        h.sub[3] = t[at + 9] & 1, h.sub[4] = t[at + 9] >> 1;
        m.push_back(h);
        open = true;
        at += 10;
      } else if (t[at + 1] == 2 && open) {
        m.back().end = bin_index;
        open = false;
        at += 2;
      } else {
        return fail(c, AVR_ERR_DEVICE, "hooks: malformed device trace of slice " + std::to_string(i));
      }
    }
    if (open) return fail(c, AVR_ERR_DEVICE, "hooks: device trace of slice " + std::to_string(i) + " ends in a map");
  }
  return AVR_OK;
}

// Device trace of every coded slice of hs->pf (decode order).
int run_traces(avr_hooks_session* hs) {
  std::vector<int> which;
  for (size_t i = 0; i < hs->pf.slices.size(); i++)
    if (hs->coded[i]) which.push_back((int)i);
  hs->bins.assign(hs->pf.slices.size(), {});
  hs->maps.assign(hs->pf.slices.size(), {});
  return trace_slices(hs, which);
}

// Streaming session: one NAL unit of the fed bytes through the stream parser (a slice joins pf).
void ingest_nal(avr_hooks_session* hs, size_t off, size_t size) {
  avr::SliceInfo si;
  if (!hs->ing.sp.next(hs->original.data() + off, size, &si)) return;
  si.nal_offset = off;
  si.nal_size = size;
  hs->pf.slices.push_back(std::move(si));
}

// Parse what the fed bytes newly complete.  final: the stream has ended (avr_hooks_end: the unit in
// progress ends with it).  want: the number of slices a decoder needs now -- when the complete units
// do not reach it, the Annex-B unit in progress is taken provisionally.
int ingest(avr_hooks_session* hs, bool final, size_t want) {
  StreamIngest& g = hs->ing;
  const uint8_t* f = hs->original.data();
  const size_t n = hs->original.size();
  if (!g.kind) {
    if (n < 8 && !final) return AVR_OK;
    g.kind = avr::is_mp4(f, n) ? 2 : 1;
  }
  if (g.kind == 2) {
    if (!g.have_layout) {
      const int r = avr::mp4_layout(f, n, &g.layout);
      if (r < 0 || (r == 0 && final)) return fail(hs->c, AVR_ERR_FORMAT, "hooks: not an MP4/avcC H.264 stream");
      if (r == 0) return AVR_OK;   // the moov box is not in yet (a moov-last file: not before the end)
      g.have_layout = true;
      for (const avr::NalRef& nr : g.layout.param_sets) ingest_nal(hs, nr.offset, nr.size);
    }
    std::vector<avr::NalRef> nals;
    for (; g.next_sample < g.layout.samples.size(); g.next_sample++) {
      const avr::NalRef& smp = g.layout.samples[g.next_sample];
      if (smp.offset > n || smp.size > n - smp.offset) {
        if (final) return fail(hs->c, AVR_ERR_FORMAT, "hooks: an MP4 sample lies past the end of the stream");
        break;   // not complete yet
      }
      nals.clear();
      avr::mp4_sample_nals(f, smp, g.layout.len_size, &nals);
      for (const avr::NalRef& nr : nals) ingest_nal(hs, nr.offset, nr.size);
    }
    return AVR_OK;
  }
  // Annex-B (demux_annexb's rules, resumed where the last call stopped)
  auto is_sc = [&](size_t j) { return j + 3 <= n && f[j] == 0 && f[j + 1] == 0 && f[j + 2] == 1; };
  auto unit_end = [&](size_t begin, size_t end) {   // trailing zero bytes belong to the next start code
    while (end > begin && f[end - 1] == 0) end--;
    return end;
  };
  for (;;) {
    if (!g.in_nal) {
      size_t i = g.scan;
      while (i + 3 <= n && !is_sc(i)) i++;
      if (i + 3 > n) {
        g.scan = i;
        break;
      }
      g.in_nal = true;
      g.nal_begin = g.scan = i + 3;
    }
    size_t j = g.scan;
    while (j + 3 <= n && !(f[j] == 0 && f[j + 1] == 0 && (f[j + 2] == 1 || f[j + 2] == 0))) j++;
    if (j + 3 > n) {
      g.scan = j;
      break;
    }
    // the unit in progress is complete: [nal_begin, j) without trailing zeros
    const size_t end = unit_end(g.nal_begin, j);
    if (g.prov_end) {
      if (end != g.prov_end)
        return fail(hs->c, AVR_ERR_FORMAT, "hooks: a slice was decoded before its NAL unit was complete");
      g.prov_end = 0;
    } else if (end > g.nal_begin) {
      ingest_nal(hs, g.nal_begin, end - g.nal_begin);
    }
    g.in_nal = false;
    g.scan = j;
  }
  // the unit in progress: at the end of the stream it is complete; before it, it is parsed
  // provisionally when the decoder needs a slice the complete units do not hold
  if (g.in_nal && (final || hs->pf.slices.size() < want)) {
    const size_t end = unit_end(g.nal_begin, n);
    if (g.prov_end && end != g.prov_end)
      return fail(hs->c, AVR_ERR_FORMAT, "hooks: a slice was decoded before its NAL unit was complete");
    if (!g.prov_end && end > g.nal_begin) {
      ingest_nal(hs, g.nal_begin, end - g.nal_begin);
      g.prov_end = end;
    }
    if (final) g.in_nal = false, g.prov_end = 0;
  }
  return AVR_OK;
}

// Per-slice state for the slices parsed so far.
void grow_session(avr_hooks_session* hs) {
  const size_t n = hs->pf.slices.size();
  hs->coded.resize(n, 0);
  hs->bins.resize(n);
  hs->maps.resize(n);
  hs->slices.resize(n);   // no slice object is live here (init_decoder closed it first)
  hs->traced.resize(n, 0);
  hs->blocks.resize(n);
  hs->block_status.resize(n, AVR_SLICE_NO_ROUNDTRIP);
}

// Streaming session: the device work of slice i and of every parsed slice after it not done yet
// (trace-ahead: the slices a feed completed go to the device together) -- their decode-order bin
// traces, and for the parallel model their final re-coded blocks (compress + the per-slice device
// roundtrip check, as avr_compress_file runs it).
int stream_device_work(avr_hooks_session* hs, size_t i) {
  std::vector<int> which;
  for (size_t k = i; k < hs->pf.slices.size(); k++)
    if (!hs->traced[k]) {
      hs->traced[k] = 1;
      if (recodable_candidate(hs->pf.slices[k])) which.push_back((int)k);
    }
  if (which.empty()) return AVR_OK;
  if (int r = trace_slices(hs, which)) return r;
  if (!parallel_model(hs->model)) return AVR_OK;
  Plan plan;
  for (const int k : which) {
    const avr::SliceInfo& s = hs->pf.slices[k];
    plan_slice(&plan, s, parallel_out_capacity(s.size));
  }
  std::vector<avr_slice_result> res;
  std::vector<uint8_t> outb;
  if (int r = run_plan(hs->c, 0, false, plan, &res, &outb, /*verify=*/true, coder_flag(hs->model))) return r;
  for (size_t q = 0; q < which.size(); q++) {
    const int k = which[q];
    hs->block_status[k] = res[q].status;
    if (res[q].status == 0)
      hs->blocks[k].assign(outb.begin() + plan.descs[q].out_offset, outb.begin() + plan.descs[q].out_offset + res[q].out_len);
  }
  return AVR_OK;
}

// Lazy decompress session: regenerate the coded slices from i on that are not yet (at most
// kLazyBatch, one device launch), patch each by the last-byte rule (recode.cpp:1345-1356) and put
// the regenerated payload in place of the surrogate one; trace = also trace them (init_decoder).
constexpr size_t kLazyBatch = 32;
int lazy_device_work(avr_hooks_session* hs, size_t i, bool trace, size_t batch = kLazyBatch) {
  std::vector<int> which;
  for (size_t k = i; k < hs->pf.slices.size() && which.size() < batch; k++)
    if (hs->coded[k] && !hs->regen_done[k]) which.push_back((int)k);
  if (which.empty()) return AVR_OK;
  Plan sub;
  for (const int k : which) {
    avr_slice_desc d = hs->dplan.descs[hs->plan_of[k]];
    append_aligned(&sub.arena, hs->dplan.arena.data() + d.payload_offset, d.payload_size, 16, &d.payload_offset);
    sub.max_w = std::max(sub.max_w, ring_cols(d));
    sub.descs.push_back(d);
  }
  std::vector<avr_slice_result> res;
  std::vector<uint8_t> outb;
  if (int r = run_plan(hs->c, 1, false, sub, &res, &outb, false, coder_flag(hs->model))) return r;
  for (size_t q = 0; q < which.size(); q++) {
    const int k = which[q];
    if (res[q].status != 0)
      return fail(hs->c, AVR_ERR_FORMAT, "slice " + std::to_string(k) + " failed to decode (" +
                                             std::to_string(res[q].status) + ")");
    std::vector<uint8_t>& g = hs->regen[k];
    g.assign(outb.begin() + sub.descs[q].out_offset, outb.begin() + sub.descs[q].out_offset + res[q].out_len);
    patch_last_byte(hs->job.blocks[hs->block_of[k]], g.size(), &g);
    // the regenerated payload in place of the surrogate one; the NAL's bytes after the payload
    // (from the literal that follows the block) stay, as does the parse's read limit
    avr::SliceInfo& s = hs->pf.slices[k];
    s.own();
    if (g.size() != s.size || s.rbsp.size() < s.h.cabac_start + s.size)
      return fail(hs->c, AVR_ERR_FORMAT, "slice " + std::to_string(k) + " regenerated " + std::to_string(g.size()) +
                                             " bytes for a " + std::to_string(s.size) + "-byte payload");
    std::copy(g.begin(), g.end(), s.rbsp.begin() + s.h.cabac_start);
    hs->regen_done[k] = 1;
  }
  return trace ? trace_slices(hs, which) : AVR_OK;
}

// which slices of the file a container re-codes: the i-th non-literal block is slice i's
bool coded_from_container(const std::vector<avr::PbBlock>& blocks, size_t n_slices, std::vector<char>* coded) {
  coded->assign(n_slices, 0);
  size_t i = 0;
  for (auto& b : blocks) {
    if (b.has_literal) continue;
    if (i >= n_slices) return false;
    (*coded)[i++] = b.has_cabac ? 1 : 0;
  }
  return i == n_slices;
}

// the live slice is done (the next init_decoder or avr_hooks_end): every bin and every map consumed
void close_live(avr_hooks_session* hs) {
  avr_hooks_slice* h = hs->live;
  hs->live = nullptr;
  if (!h) return;
  if (h->cur != h->nbins)
    hs->fail_once("hooks: slice " + std::to_string(h->index) + " ended after " + std::to_string(h->cur) + " of " +
                  std::to_string(h->nbins) + " bins");
  else if (h->map_cur != h->nmaps)
    hs->fail_once("hooks: slice " + std::to_string(h->index) + " reported " + std::to_string(h->map_cur) + " of its " +
                  std::to_string(h->nmaps) + " significance maps");
  else if (!hs->fs_have || hs->pf.slices[hs->fs_slice].picture_id != hs->pf.slices[h->index].picture_id)
    hs->fail_once("hooks: slice " + std::to_string(h->index) + " was decoded without a frame_spec for its picture");
}

// frame_spec of slice i: the model's frames (update_frame_spec, recode.cpp:824-843) turn over where
// the device's pictures do (its decode-order picture counter, which the two fields of a frame
// share, as they share frame_num), and the size must be the picture's.  A caller that starts a new
// frame inside one of the device's pictures is refused.  A caller whose frame_num stays the same
// while the device starts a new picture is accepted only where the two pictures' slice headers
// carry the same frame_num: the fork passes that syntax element, and consecutive pictures share it
// after a non-reference picture (e.g. B(frame_num 4, nal_ref_idc 0) then P(4)) -- the model keeps
// its per-picture frames there (frame_spec takes a picture counter).  Any other
// repeat is a caller whose frames differ from the pictures it decodes.
void check_frame_spec(avr_hooks_session* hs, int i, int frame_num, int w, int h) {
  const avr::SliceInfo& s = hs->pf.slices[i];
  const std::string where = "hooks: slice " + std::to_string(i) + ": frame_spec(" + std::to_string(frame_num) + ", " +
                            std::to_string(w) + ", " + std::to_string(h) + ")";
  if (w != s.h.mb_width || h != s.h.mb_height) {
    hs->fail_once(where + " size differs from the picture's " + std::to_string(s.h.mb_width) + " x " +
                  std::to_string(s.h.mb_height));
    return;
  }
  if (hs->fs_have) {
    const avr::SliceInfo& p = hs->pf.slices[hs->fs_slice];
    const bool caller_new = frame_num != hs->fs_num || w != hs->fs_w || h != hs->fs_h;
    const bool device_new = s.picture_id != p.picture_id || w != hs->fs_w || h != hs->fs_h;
    const bool syntax_repeat = !caller_new && device_new && s.h.frame_num == p.h.frame_num;
    if (caller_new != device_new && !syntax_repeat)
      hs->fail_once(where + (device_new ? " keeps the frame of slice " : " starts a new frame after slice ") +
                    std::to_string(hs->fs_slice) + ", the device's parse " +
                    (device_new ? "starts a new picture" : "stays in the same picture"));
  }
  hs->fs_have = true;
  hs->fs_num = frame_num, hs->fs_w = w, hs->fs_h = h, hs->fs_slice = i;
}

int hooks_finish_setup(avr_hooks_session* hs, const std::vector<avr::PbBlock>& blocks) {
  if (int r = parse_file(hs->c, hs->original.data(), hs->original.size(), &hs->pf)) return r;
  if (!coded_from_container(blocks, hs->pf.slices.size(), &hs->coded))
    return fail(hs->c, AVR_ERR_FORMAT, "hooks: container blocks do not match the file's slices");
  if (int r = run_traces(hs)) return r;
  hs->slices.resize(hs->pf.slices.size());
  return AVR_OK;
}

}  // namespace

int avr_hooks_compress_begin(avr_ctx* c, const uint8_t* file, size_t n, int model, avr_hooks_session** out) {
  if (!c || !file || !out) return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  std::unique_ptr<avr_hooks_session> hs(new avr_hooks_session);
  hs->c = c;
  hs->original.assign(file, file + n);
  uint8_t* avrc = nullptr;
  size_t avrc_len = 0;
  // a session's container never carries Block field 17: the callbacks serve the slices the plain
  // segmentation codes; nor the file's CRC (Metadata field 16), nor unit checksums (Block field 18)
  const int esc = avr_get_recode_escaped(c), chk = avr_get_checksums(c), uck = avr_get_unit_checksums(c);
  avr_set_recode_escaped(c, 0);
  avr_set_checksums(c, 0);
  avr_set_unit_checksums(c, 0);
  const int cr = avr_compress_file(c, file, n, model, &avrc, &avrc_len);
  avr_set_recode_escaped(c, esc);
  avr_set_checksums(c, chk);
  avr_set_unit_checksums(c, uck);
  if (cr) return cr;
  hs->result.assign(avrc, avrc + avrc_len);
  free(avrc);
  std::vector<avr::PbBlock> blocks;
  std::string version;
  if (!avr::pb_parse(hs->result.data(), hs->result.size(), &blocks, &version))
    return fail(c, AVR_ERR_FORMAT, "hooks: container does not parse");
  if (int r = hooks_finish_setup(hs.get(), blocks)) return r;
  *out = hs.release();
  return AVR_OK;
}

int avr_hooks_decompress_begin(avr_ctx* c, const uint8_t* avrc, size_t n, avr_hooks_session** out,
                               const uint8_t** stream, size_t* stream_len) {
  if (!c || !avrc || !out) return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  std::unique_ptr<avr_hooks_session> hs(new (std::nothrow) avr_hooks_session);
  if (!hs) return fail(c, AVR_ERR_OUT_OF_MEMORY, "host allocation failed");
  hs->c = c;
  hs->decompress = true;
  {
    // the container's model from its Metadata.version alone (no block list), inside guarded(): no
    // exception crosses the C ABI
    int m = 0;
    bool split = false;   // a long-slice split container: regenerated whole at begin (its pieces are
                          // a whole-file launch), as a reference-model one is
    if (int r = guarded(c, [&]() -> int {
          std::string version;
          m = avr::pb_read_version(avrc, n, &version) ? avr::model_of_version(version) : 0;
          // the surrogate stream a session hands its caller has no form for a block that stands for
          // escaped bytes
          if (avr::escaped_version(version))
            return fail(c, AVR_ERR_UNSUPPORTED, "hooks: a container with re-coded escaped slices (" + version +
                                                    ") decompresses through the whole-file calls and the plans only");
          if (parallel_model(m)) {   // either coder's split (P32's: the "P32S" tag)
            std::vector<avr::PbBlock> blocks;
            if (avr::pb_parse(avrc, n, &blocks, &version))
              for (const auto& b : blocks) split = split || b.has_seams;
          }
          return AVR_OK;
        }))
      return r;
    if (parallel_model(m) && !split && !getenv("AVR_HOOKS_EAGER")) {
      // the parallel model's slices are independent: plan the container now, regenerate on demand
      if (int r = guarded(c, [&]() -> int {
            hs->lazy = true;
            hs->model = m;
            hs->original.assign(avrc, avrc + n);   // the container (the job's blocks point into it)
            if (int e = decompress_setup(c, hs->original.data(), hs->original.size(), &hs->job, &hs->dplan)) return e;
            hs->stream.assign(hs->job.stream.begin(), hs->job.stream.end());
            if (int e = parse_file(c, hs->stream.data(), hs->stream.size(), &hs->pf)) return e;
            if (!coded_from_container(hs->job.blocks, hs->pf.slices.size(), &hs->coded))
              return fail(c, AVR_ERR_FORMAT, "hooks: container blocks do not match the file's slices");
            const size_t ns = hs->pf.slices.size();
            hs->plan_of.assign(ns, -1);
            hs->block_of.assign(ns, -1);
            size_t i = 0;
            for (size_t bi = 0; bi < hs->job.blocks.size(); bi++) {
              if (hs->job.blocks[bi].has_literal) continue;
              hs->block_of[i] = (int)bi;
              if (hs->job.blocks[bi].has_cabac) hs->plan_of[i] = hs->job.desc_of_block[bi];
              i++;
            }
            for (size_t k = 0; k < ns; k++)
              if (hs->coded[k] && hs->plan_of[k] < 0) return fail(c, AVR_ERR_FORMAT, "hooks: a coded block has no plan slice");
            hs->regen_done.assign(ns, 0);
            hs->regen.assign(ns, {});
            hs->bins.assign(ns, {});
            hs->maps.assign(ns, {});
            hs->slices.resize(ns);
            return AVR_OK;
          }))
        return r;
      if (stream) *stream = hs->stream.data();
      if (stream_len) *stream_len = hs->stream.size();
      *out = hs.release();
      return AVR_OK;
    }
  }
  uint8_t* orig = nullptr;
  size_t orig_len = 0;
  if (int r = avr_decompress_file(c, avrc, n, &orig, &orig_len)) return r;
  hs->original.assign(orig, orig + orig_len);
  hs->result = hs->original;
  free(orig);
  std::vector<avr::PbBlock> blocks;
  std::string version;
  if (!avr::pb_parse(avrc, n, &blocks, &version)) return fail(c, AVR_ERR_FORMAT, "hooks: container does not parse");
  // read_packet (recode.cpp:1359-1409)
  uint64_t seq = 1;
  for (auto& b : blocks) {
    if (b.has_literal) {
      hs->stream.insert(hs->stream.end(), b.literal, b.literal + b.literal_len);
    } else if (b.has_cabac) {
      uint8_t mk[8];
      avr::surrogate_marker(seq++, mk);
      hs->stream.insert(hs->stream.end(), mk, mk + 8);
      hs->stream.insert(hs->stream.end(), (size_t)b.size - 8, (uint8_t)'X');
    }
  }
  if (int r = hooks_finish_setup(hs.get(), blocks)) return r;
  if (stream) *stream = hs->stream.data();
  if (stream_len) *stream_len = hs->stream.size();
  *out = hs.release();
  return AVR_OK;
}

int avr_hooks_compress_stream_begin(avr_ctx* c, int model, avr_hooks_session** out) {
  if (!c || !out) return AVR_ERR_INVALID_ARGUMENT;
  if (!valid_model(model)) return AVR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  avr_hooks_session* hs = new (std::nothrow) avr_hooks_session;
  if (!hs) return AVR_ERR_OUT_OF_MEMORY;
  hs->c = c;
  hs->streaming = true;
  hs->model = model;
  *out = hs;
  return AVR_OK;
}

int avr_hooks_feed(avr_hooks_session* hs, const uint8_t* bytes, size_t n) {
  if (!hs || (!bytes && n) || !hs->streaming) return AVR_ERR_INVALID_ARGUMENT;
  try {
    hs->original.insert(hs->original.end(), bytes, bytes + n);
  } catch (const std::bad_alloc&) {
    return AVR_ERR_OUT_OF_MEMORY;
  }
  return AVR_OK;
}

void* avr_hook_init_decoder(void* opaque, void* /*cabac_context*/, const uint8_t* buf, int size) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs) return nullptr;
  close_live(hs);
  if (hs->streaming) {
    // the slice the decoder starts is in the bytes its demuxer has read (read_packet feeds them
    // before the packet is decoded): parse what is new
    int r = guarded(hs->c, [&] {
      const int e = ingest(hs, false, hs->next_slice + 1);
      grow_session(hs);
      return e;
    });
    if (r) {
      hs->fail_once("hooks: the bytes fed so far do not parse (" + std::to_string(r) + "): " + hs->c->err);
      hs->next_slice++;
      return nullptr;
    }
  }
  if (hs->next_slice >= hs->pf.slices.size()) {
    hs->fail_once(hs->streaming ? "hooks: init_decoder for a slice not yet fed" : "hooks: more slices than the file holds");
    return nullptr;
  }
  const size_t i = hs->next_slice++;
  if (hs->fs_pending) {   // the frame_spec made before this slice's decode
    hs->fs_pending = false;
    check_frame_spec(hs, (int)i, hs->pend_num, hs->pend_w, hs->pend_h);
  }
  const avr::SliceInfo& s = hs->pf.slices[i];
  if (!buf || size < 0 || (size_t)size != s.size) {
    hs->fail_once("hooks: slice " + std::to_string(i) + " size differs from the device's parse");
    return nullptr;
  }
  if (hs->streaming) {
    // find_next_coded_block (recode.cpp:1139-1145, 1275-1297) on the slice's own bytes: a slice the
    // device can re-code gets hooks; the container (avr_hooks_end) may still store it skip_coded
    hs->coded[i] = memcmp(buf, s.payload(), s.size) == 0 && recodable_candidate(s) ? 1 : 0;
    if (hs->coded[i] && guarded(hs->c, [&] { return stream_device_work(hs, i); }) != AVR_OK) {
      hs->fail_once("hooks: device trace of slice " + std::to_string(i) + " failed: " + hs->c->err);
      return nullptr;
    }
  }
  if (!hs->coded[i]) return nullptr;  // not re-coded: decode natively (recode.cpp:1139-1145)
  if (hs->lazy && !hs->regen_done[i] && guarded(hs->c, [&] { return lazy_device_work(hs, i, true); }) != AVR_OK) {
    hs->fail_once("hooks: device decode of slice " + std::to_string(i) + " failed: " + hs->c->err);
    return nullptr;
  }
  if (hs->decompress) {
    // recognize_coded_block (recode.cpp:1546-1573)
    uint8_t mk[8];
    avr::surrogate_marker(hs->next_marker++, mk);
    if (size < 8 || memcmp(buf, mk, 8) != 0) {
      hs->fail_once("hooks: invalid surrogate marker in slice " + std::to_string(i));
      return nullptr;
    }
  } else if (memcmp(buf, s.payload(), s.size) != 0) {
    hs->fail_once("hooks: slice " + std::to_string(i) + " payload differs from the file's");
    return nullptr;
  }
  avr_hooks_slice& h = hs->slices[i];
  h.sess = hs;
  h.index = (int)i;
  h.trace = hs->bins[i].data();
  h.nbins = hs->bins[i].size() / 2;
  h.cur = 0;
  h.maps = hs->maps[i].data();
  h.nmaps = hs->maps[i].size();
  h.map_cur = 0;
  hs->live = &h;
  return &h;
}

static int hook_bin(void* slice, int kind, uint8_t* state) {
  avr_hooks_slice* h = (avr_hooks_slice*)slice;
  if (!h || !h->sess) return 0;
  if (h->cur >= h->nbins) {
    h->sess->fail_once("hooks: slice " + std::to_string(h->index) + " asked for more bins than it holds");
    return 0;
  }
  const uint8_t t = h->trace[2 * h->cur], pre = h->trace[2 * h->cur + 1];
  h->cur++;
  const int bin = t & 1;
  if (((t >> 1) & 3) != kind) {
    h->sess->fail_once("hooks: slice " + std::to_string(h->index) + " bin " + std::to_string(h->cur - 1) +
                       ": bin kind differs from the device's parse");
    return bin;
  }
  if (state) {
    if (*state != pre)
      h->sess->fail_once("hooks: slice " + std::to_string(h->index) + " bin " + std::to_string(h->cur - 1) +
                         ": context state differs from the device's parse");
    *state = next_state(*state, bin);
  }
  return bin;
}

int avr_hook_get(void* slice, uint8_t* state) {
  if (!state) {
    if (slice && ((avr_hooks_slice*)slice)->sess) ((avr_hooks_slice*)slice)->sess->fail_once("hooks: get without a state");
    return 0;
  }
  return hook_bin(slice, 0, state);
}
int avr_hook_get_bypass(void* slice) { return hook_bin(slice, 1, nullptr); }
int avr_hook_get_terminate(void* slice) { return hook_bin(slice, 2, nullptr); }

const uint8_t* avr_hook_skip_bytes(void* slice, int /*n*/) {
  avr_hooks_slice* h = (avr_hooks_slice*)slice;
  if (h && h->sess) h->sess->fail_once("hooks: skip_bytes (I_PCM) is not supported");
  return nullptr;
}

void avr_hook_frame_spec(void* opaque, int frame_num, int mb_width, int mb_height) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs) return;
  avr_hooks_slice* h = hs->live;
  if (h && h->cur < h->nbins) {   // inside a slice's decode: that slice's picture
    check_frame_spec(hs, h->index, frame_num, mb_width, mb_height);
    return;
  }
  if (hs->fs_pending && (hs->pend_num != frame_num || hs->pend_w != mb_width || hs->pend_h != mb_height))
    hs->fail_once("hooks: two different frame_spec calls before one slice");
  hs->fs_pending = true;
  hs->pend_num = frame_num, hs->pend_w = mb_width, hs->pend_h = mb_height;
}

void avr_hook_mb_xy(void* opaque, int x, int y) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs) return;
  hs->mb_calls++;
  hs->mb_x = x;
  hs->mb_y = y;
}

void avr_hook_begin_sub_mb(void* opaque, int cat, int scan8index, int max_coeff, int is_dc, int chroma422) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs || !hs->live) return;
  avr_hooks_slice* h = hs->live;
  if (h->sub_open) hs->fail_once("hooks: begin_sub_mb inside an open sub-macroblock");
  h->sub_open = true;
  const int a[5] = {cat, scan8index, max_coeff, is_dc, chroma422};
  memcpy(h->sub_args, a, sizeof(a));
}

void avr_hook_end_sub_mb(void* opaque, int cat, int scan8index, int max_coeff, int is_dc, int chroma422) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs || !hs->live) return;
  avr_hooks_slice* h = hs->live;
  const int a[5] = {cat, scan8index, max_coeff, is_dc, chroma422};
  if (!h->sub_open || memcmp(h->sub_args, a, sizeof(a)) != 0)  // recode.cpp:185-189
    hs->fail_once("hooks: end_sub_mb does not match begin_sub_mb");
  h->sub_open = false;
}

// begin_coding_type(SIG_MAP) (recode.cpp:951-974) starts the model's significance-map keys: it
// must come exactly before the device's map's first bin, under the device's macroblock (mb_xy)
// and sub-macroblock (begin_sub_mb), with zigzag_index 0 (recode.cpp:961); end_coding_type right
// after its last bin (recode.cpp:931-950).  Other coding types carry no device event.
void avr_hook_begin_coding_type(void* opaque, int coding_type, int zigzag_index, int /*param0*/, int /*param1*/) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs || !hs->live) return;
  avr_hooks_slice* h = hs->live;
  if (h->coding_type != AVR_PIP_UNKNOWN) hs->fail_once("hooks: nested begin_coding_type");
  h->coding_type = coding_type;
  if (coding_type != AVR_PIP_SIGNIFICANCE_MAP) return;
  const std::string where = "hooks: slice " + std::to_string(h->index) + " bin " + std::to_string(h->cur) + ": ";
  if (h->map_cur >= h->nmaps) {
    hs->fail_once(where + "begin_coding_type(SIG_MAP) where the device's parse has no significance map");
    return;
  }
  const HookMap& m = h->maps[h->map_cur];
  if (h->cur != m.begin)
    hs->fail_once(where + "begin_coding_type(SIG_MAP) where the device's map begins at bin " + std::to_string(m.begin));
  else if (zigzag_index != 0)
    hs->fail_once(where + "begin_coding_type(SIG_MAP) with zigzag_index != 0");
  else if (hs->mb_x != m.x || hs->mb_y != m.y)
    hs->fail_once(where + "significance map under mb_xy(" + std::to_string(hs->mb_x) + ", " + std::to_string(hs->mb_y) +
                  "), the device's is (" + std::to_string(m.x) + ", " + std::to_string(m.y) + ")");
  else if (!h->sub_open || memcmp(h->sub_args, m.sub, sizeof(m.sub)) != 0)
    hs->fail_once(where + "significance map outside the device's sub-macroblock (cat " + std::to_string(m.sub[0]) +
                  ", scan8 " + std::to_string(m.sub[1]) + ", max " + std::to_string(m.sub[2]) + ")");
}

void avr_hook_end_coding_type(void* opaque, int coding_type) {
  avr_hooks_session* hs = (avr_hooks_session*)opaque;
  if (!hs || !hs->live) return;
  avr_hooks_slice* h = hs->live;
  if (h->coding_type != coding_type) hs->fail_once("hooks: end_coding_type does not match begin_coding_type");
  h->coding_type = AVR_PIP_UNKNOWN;
  if (coding_type != AVR_PIP_SIGNIFICANCE_MAP || h->map_cur >= h->nmaps) return;
  const HookMap& m = h->maps[h->map_cur++];
  if (h->cur != m.end)
    hs->fail_once("hooks: slice " + std::to_string(h->index) + " bin " + std::to_string(h->cur) +
                  ": end_coding_type(SIG_MAP) where the device's map ends at bin " + std::to_string(m.end));
}

int avr_hooks_end(avr_hooks_session* hs, uint8_t** out, size_t* out_len) {
  if (!hs || !out || !out_len) return AVR_ERR_INVALID_ARGUMENT;
  close_live(hs);
  if (hs->streaming) {
    // the whole file is in: its last slices, and the container (recode.cpp:1102-1125).  The
    // parallel model's blocks are final as each slice was traced (slices independent): the container
    // is assembled from them.  The reference model's estimators chain across slices, so its
    // container comes from one compress of the whole file.
    if (int r = guarded(hs->c, [&] {
          const int e = ingest(hs, true, 0);
          grow_session(hs);
          if (!e && hs->err.empty() && parallel_model(hs->model)) return stream_device_work(hs, 0);
          return e;
        }))
      return r;
    if (hs->err.empty()) {
      uint8_t* avrc = nullptr;
      size_t avrc_len = 0;
      if (parallel_model(hs->model)) {
        if (int r = guarded(hs->c, [&] {
              std::vector<char> ok(hs->pf.slices.size(), 0);
              std::vector<std::pair<const uint8_t*, size_t>> blobs(hs->pf.slices.size(), {nullptr, 0});
              for (size_t i = 0; i < ok.size(); i++) {
                ok[i] = recodable_candidate(hs->pf.slices[i]) && hs->block_status[i] == 0;
                blobs[i] = {hs->blocks[i].data(), hs->blocks[i].size()};
              }
              const std::vector<SliceView> sv = views_of(hs->pf);
              return emit_container(hs->original.data(), hs->original.size(), sv,
                                    segment(hs->original.data(), hs->original.size(), sv, ok), blobs, hs->model,
                                    &avrc, &avrc_len);
            }))
          return r;
      } else {   // as at avr_hooks_compress_begin: a session's container carries no file CRC and no unit checksums
        const int chk = avr_get_checksums(hs->c), uck = avr_get_unit_checksums(hs->c);
        avr_set_checksums(hs->c, 0);
        avr_set_unit_checksums(hs->c, 0);
        const int r = avr_compress_file(hs->c, hs->original.data(), hs->original.size(), hs->model, &avrc, &avrc_len);
        avr_set_checksums(hs->c, chk);
        avr_set_unit_checksums(hs->c, uck);
        if (r) return r;
      }
      hs->result.assign(avrc, avrc + avrc_len);
      free(avrc);
    }
  }
  if (hs->lazy && hs->err.empty()) {
    // the original file: literals and regenerated slices in block order (decompressor::run's output,
    // recode.cpp:1338-1357), slices no init_decoder reached regenerated now
    if (int r = guarded(hs->c, [&]() -> int {
          if (int e = lazy_device_work(hs, 0, false, hs->pf.slices.size())) return e;
          std::vector<uint8_t> o;
          o.reserve(hs->stream.size());
          size_t i = 0;
          for (const avr::PbBlock& b : hs->job.blocks) {
            if (b.has_literal) {
              o.insert(o.end(), b.literal, b.literal + b.literal_len);
              continue;
            }
            if (b.has_cabac) o.insert(o.end(), hs->regen[i].begin(), hs->regen[i].end());
            i++;
          }
          // a checked container: the file as the session regenerated it, slice by slice, against its CRC
          if (hs->job.has_crc && avr_crc32(0, o.data(), o.size()) != hs->job.file_crc)
            return fail(hs->c, AVR_ERR_CHECKSUM, "the container decoded to a file that is not the file it was made from (CRC-32)");
          hs->result.swap(o);
          return AVR_OK;
        }))
      return r;
  }
  if (hs->next_slice != hs->pf.slices.size())
    hs->fail_once("hooks: " + std::to_string(hs->next_slice) + " of " + std::to_string(hs->pf.slices.size()) +
                  " slices were decoded");
  if (!hs->err.empty()) return fail(hs->c, AVR_ERR_FORMAT, hs->err);
  *out = (uint8_t*)malloc(hs->result.size() ? hs->result.size() : 1);
  if (!*out) return AVR_ERR_OUT_OF_MEMORY;
  memcpy(*out, hs->result.data(), hs->result.size());
  *out_len = hs->result.size();
  return AVR_OK;
}

void avr_hooks_destroy(avr_hooks_session* hs) { delete hs; }

// Debug (tests, host only; not part of include/avrecode.h): how many slices a decompress session
// has regenerated on the device so far (a lazy parallel-model session: those init_decoder reached,
// in batches; -1: an eager session, which regenerated the whole file at begin).
extern "C" int avr_debug_hooks_regenerated(const avr_hooks_session* hs) {
  if (!hs || !hs->decompress) return AVR_ERR_INVALID_ARGUMENT;
  if (!hs->lazy) return -1;
  int k = 0;
  for (const char d : hs->regen_done) k += d ? 1 : 0;
  return k;
}

// Debug (tests, host only; not part of include/avrecode.h): the slices a streaming session's
// incremental parser finds when `file` is fed in pieces ending at cuts[0] < ... < cuts[ncuts - 1] = n
// (incremental = 1; after each piece the parser is asked for one slice more than it holds when
// provisional = 1, as a decoder's next init_decoder would), or that parse_file finds in the whole
// file (incremental = 0).  out: 4 u64 per slice (NAL offset, NAL size, payload size, picture id).
// Returns the slice count (at most cap written), or < 0.
extern "C" int avr_debug_stream_slices(const uint8_t* file, size_t n, const uint64_t* cuts, int ncuts, int incremental,
                                       int provisional, uint64_t* out, int cap) {
  if (!file || (incremental && (!cuts || ncuts <= 0)) || (!out && cap)) return AVR_ERR_INVALID_ARGUMENT;
  return guarded(nullptr, [&]() -> int {
    avr_hooks_session hs;
    hs.streaming = true;
    if (incremental) {
      size_t fed = 0;
      for (int k = 0; k < ncuts; k++) {
        const size_t end = std::min<size_t>(n, cuts[k]);
        if (end > fed) hs.original.insert(hs.original.end(), file + fed, file + end);
        fed = std::max(fed, end);
        if (int r = ingest(&hs, false, 0)) return r;
        if (provisional)
          if (int r = ingest(&hs, false, hs.pf.slices.size() + 1)) return r;
      }
      if (fed < n) hs.original.insert(hs.original.end(), file + fed, file + n);
      if (int r = ingest(&hs, true, 0)) return r;
    } else if (int r = parse_file(nullptr, file, n, &hs.pf)) {
      return r;
    }
    const int cnt = (int)hs.pf.slices.size();
    for (int i = 0; i < cnt && i < cap; i++) {
      const avr::SliceInfo& si = hs.pf.slices[i];
      out[4 * i] = si.nal_offset, out[4 * i + 1] = si.nal_size, out[4 * i + 2] = si.size;
      out[4 * i + 3] = (uint64_t)si.picture_id;
    }
    return cnt;
  });
}
