// The seams codec of the parallel model's long-slice split (avr_api.cpp, "the long-slice split"):
// the re-encoder state at a cut restated on the host, Block field 16 written and read, and the
// splice of a split slice's pieces; at the end, the host steps of the split's compress side (split_slot,
// seams_build), which the whole-file compress and the ABI's avr_split_plan / avr_seams_build share.
// No HIP: seams_decode reads untrusted bytes and is reached by the stand-alone sanitizer program
// tests/native/plan_fuzz.cpp, seams_build reads what came back from a device and is reached through
// avr_seams_build by tests/native/seams_build_fuzz.cpp.
#include <zlib.h>

#include "avr_host.h"
#include "h264_tables.h"

namespace avr_host {

namespace {

void put_le32(std::vector<uint8_t>* o, uint32_t v) {
  for (int k = 0; k < 4; k++) o->push_back((uint8_t)(v >> (8 * k)));
}
uint32_t get_le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The slice's initial context states (9.3.1.1), as init_slice_state sets them on the device.
void cabac_init_states(const avr_slice_desc& d, uint8_t out[1024]) {
  const int qp = d.slice_qp < 0 ? 0 : d.slice_qp > 51 ? 51 : d.slice_qp;
  for (int c = 0; c < 1024; c++) {
    int m, n;
    avr::mn_for_ctx(d.slice_type == 2 ? -1 : d.cabac_init_idc, c, &m, &n);
    int pre = ((m * qp) >> 4) + n;
    pre = pre < 1 ? 1 : pre > 126 ? 126 : pre;
    out[c] = pre <= 63 ? (uint8_t)((63 - pre) << 1) : (uint8_t)(((pre - 64) << 1) | 1);
  }
}
// an upper-row edge byte as the seams field keeps it: what the parse of the row below reads of it --
// nnz only as nonzero (coded_block_flag's context), |mvd| only up to 33 (absMvdComp's sum against
// 3 and 32)
uint8_t edge_norm(int j, uint8_t b) {
  if (j >= 4 && j < 16) return b != 0;
  if (j >= 16 && j < 32) return b > 33 ? 33 : b;
  return b;
}

}  // namespace

// The re-encoder where the decoder stands after bitpos bits with codIOffset `offset` (the oracle's
// avr_seam_encoder): m = (bitpos - 10) / 8 whole bytes have left the window; the last byte of L
// below m that is not 0xFF (q) is the cache, the 0xFF bytes after it outstanding, the rest in low.
bool seam_encoder(const uint8_t* pay, size_t n, uint64_t bitpos, uint32_t offset, uint32_t range, SeamCe* s) {
  if (bitpos < 26) return false;
  const uint64_t m = (bitpos - 10) / 8, sb = m > 12 ? m - 12 : 0, e = (bitpos + 7) / 8;
  unsigned __int128 x = 0;
  for (uint64_t j = sb; j < e; j++) x = x << 8 | (j < n ? pay[j] : 0);
  x >>= 8 * e - bitpos;
  if (x < offset) return false;
  const unsigned __int128 y = x - offset;
  for (uint64_t j = m; j-- > sb;) {
    const uint32_t b = (uint32_t)(y >> (bitpos - 8 * j - 8)) & 0xff;
    if (b == 0xff) continue;
    const unsigned lowbits = (unsigned)(bitpos - 8 * m);
    s->q = (uint32_t)j;
    s->cache = b;
    s->outstanding = (uint32_t)(m - 1 - j);
    s->low = (uint32_t)(y & (((unsigned __int128)1 << lowbits) - 1));
    s->queue = (int32_t)lowbits - 18;
    s->range = range;
    return true;
  }
  return false;
}

// Block field 16: u32 raw length, then zlib (level 9) of { u32 2, u32 cuts, u32 mb_width,
// u32 piece_len[cuts + 1], per cut { u32 first_mb, q, last_dqp_nz, ce_low, ce_queue,
// ce_outstanding, ce_cache, ce_range, u8 state[1024] XOR the slice's initial states, u8 edges
// byte-major (byte j of every column, j = 0..39; edge_norm) } } (little-endian)
bool seams_encode(const std::vector<const avr::SeamRec*>& recs, const std::vector<SeamCe>& ce, const avr_slice_desc& d,
                  const std::vector<uint32_t>& piece_len, std::vector<uint8_t>* out) {
  const int mb_width = d.mb_width;
  uint8_t init[1024];
  cabac_init_states(d, init);
  std::vector<uint8_t> raw;
  put_le32(&raw, 2);
  put_le32(&raw, (uint32_t)recs.size());
  put_le32(&raw, (uint32_t)mb_width);
  for (uint32_t l : piece_len) put_le32(&raw, l);
  for (size_t i = 0; i < recs.size(); i++) {
    put_le32(&raw, recs[i]->first_mb);
    put_le32(&raw, ce[i].q);
    put_le32(&raw, recs[i]->last_dqp_nz);
    put_le32(&raw, ce[i].low);
    put_le32(&raw, (uint32_t)ce[i].queue);
    put_le32(&raw, ce[i].outstanding);
    put_le32(&raw, ce[i].cache);
    put_le32(&raw, ce[i].range);
    for (int c = 0; c < 1024; c++) raw.push_back((uint8_t)(recs[i]->state[c] ^ init[c]));
    const uint8_t* e = (const uint8_t*)(recs[i] + 1);
    for (int j = 0; j < avr::kEdgeBytes; j++)
      for (int c = 0; c < mb_width; c++) raw.push_back(edge_norm(j, e[(size_t)avr::kEdgeBytes * c + j]));
  }
  uLongf zl = compressBound(raw.size());
  out->assign(4 + zl, 0);
  if (compress2(out->data() + 4, &zl, raw.data(), raw.size(), 9) != Z_OK) return false;
  out->resize(4 + zl);
  for (int k = 0; k < 4; k++) (*out)[k] = (uint8_t)(raw.size() >> (8 * k));
  return true;
}

bool seams_decode(const uint8_t* p, size_t n, const avr_slice_desc& d, size_t rec_stride, SeamsDecoded* sd) {
  const int mb_width = d.mb_width;
  uint8_t init[1024];
  cabac_init_states(d, init);
  if (n < 4) return false;
  const uint32_t rl = get_le32(p);
  if (rl < 12 || rl > (1u << 30)) return false;
  std::vector<uint8_t> raw(rl);
  uLongf got = rl;
  if (uncompress(raw.data(), &got, p + 4, n - 4) != Z_OK || got != rl || get_le32(raw.data()) != 2) return false;
  const uint32_t k = get_le32(raw.data() + 4), w = get_le32(raw.data() + 8);
  const size_t per = 32 + 1024 + (size_t)avr::kEdgeBytes * w;
  if ((int)w != mb_width || k == 0 || k > 65536 || 12 + 4 * ((size_t)k + 1) + per * k != rl) return false;
  sd->cuts = (int)k;
  const uint8_t* q = raw.data() + 12;
  sd->piece_len.resize(k + 1);
  for (uint32_t i = 0; i <= k; i++, q += 4) sd->piece_len[i] = get_le32(q);
  sd->recs.assign((size_t)k * rec_stride, 0);
  sd->first_mb.resize(k);
  sd->q.resize(k);
  for (uint32_t i = 0; i < k; i++, q += per) {
    avr::SeamRec* r = (avr::SeamRec*)(sd->recs.data() + (size_t)i * rec_stride);
    r->first_mb = sd->first_mb[i] = get_le32(q);
    sd->q[i] = get_le32(q + 4);
    r->last_dqp_nz = get_le32(q + 8);
    r->ce_low = get_le32(q + 12);
    r->ce_queue = (int32_t)get_le32(q + 16);
    r->ce_outstanding = get_le32(q + 20);
    r->ce_cache = get_le32(q + 24);
    r->ce_range = get_le32(q + 28);
    // a cut's state is what seam_encoder can produce: the window 12 bytes deep at most
    if (r->ce_queue < -8 || r->ce_queue > -1 || r->ce_cache > 0xff || r->ce_range < 256 || r->ce_range > 510 ||
        r->ce_low >= (1u << (r->ce_queue + 18)) || r->ce_outstanding > 12 || (i && sd->q[i] <= sd->q[i - 1]) ||
        (i && sd->first_mb[i] <= sd->first_mb[i - 1]) || sd->first_mb[i] % w ||
        sd->first_mb[i] >= (uint32_t)w * (uint32_t)std::max(1, d.mb_height))
      return false;
    for (int c = 0; c < 1024; c++) r->state[c] = (uint8_t)(q[32 + c] ^ init[c]);
    uint8_t* e = (uint8_t*)(r + 1);
    for (int j = 0; j < avr::kEdgeBytes; j++)
      for (uint32_t c = 0; c < w; c++) e[(size_t)avr::kEdgeBytes * c + j] = q[32 + 1024 + (size_t)j * w + c];
  }
  return true;
}

// The cuts' q alone (piece i covers slice bytes [q[i - 1], q[i])), for the callers that need a cut
// block's units and hold no descriptor: the container writer's unit CRCs and avr_container_describe.
// The layout's own checks only; the states are seams_decode's business.
bool seams_cut_q(const uint8_t* p, size_t n, std::vector<uint32_t>* q) {
  q->clear();
  if (n < 4) return false;
  const uint32_t rl = get_le32(p);
  if (rl < 12 || rl > (1u << 30)) return false;
  std::vector<uint8_t> raw(rl);
  uLongf got = rl;
  if (uncompress(raw.data(), &got, p + 4, n - 4) != Z_OK || got != rl || get_le32(raw.data()) != 2) return false;
  const uint32_t k = get_le32(raw.data() + 4), w = get_le32(raw.data() + 8);
  const size_t per = 32 + 1024 + (size_t)avr::kEdgeBytes * w;
  if (k == 0 || k > 65536 || w > (uint32_t)avr::kMringCols || 12 + 4 * ((size_t)k + 1) + per * k != rl) return false;
  const uint8_t* r = raw.data() + 12 + 4 * ((size_t)k + 1);
  for (uint32_t i = 0; i < k; i++, r += per) {
    q->push_back(get_le32(r + 4));
    if (i && (*q)[i] <= (*q)[i - 1]) return false;
  }
  return true;
}

// the regenerated bytes of a split slice from its q.size() + 1 pieces, units d[i] / r[i] of a pieces
// launch that wrote `out`: piece i's bytes up to cut i's q (the cut's first byte), the last piece
// whole; false if a piece failed or came out short
bool splice_pieces(const avr_slice_desc* d, const avr_slice_result* r, const uint8_t* out, const std::vector<uint32_t>& q,
                   std::vector<uint8_t>* o) {
  o->clear();
  for (size_t i = 0; i <= q.size(); i++) {
    if (r[i].status) return false;
    const size_t start = i ? q[i - 1] : 0;
    if (o->size() != start) return false;
    size_t keep = r[i].out_len;
    if (i < q.size()) {
      if (q[i] < start || q[i] - start > keep) return false;
      keep = q[i] - start;
    }
    o->insert(o->end(), out + d[i].out_offset, out + d[i].out_offset + keep);
  }
  return true;
}
// recode.cpp:1345-1356 on a regenerated slice (before it: the trailing 0x80 already dropped): the
// compress side's form of last_byte_rule (avr_host.h), from the payload whose block, size > 1, will
// carry the payload's parity and last byte
void last_byte_patch(std::vector<uint8_t>* o, const uint8_t* payload, size_t size) {
  if (size <= 1) return;
  if ((int)(size & 1) != (int)(o->size() & 1)) o->push_back(payload[size - 1]);
  else if (!o->empty()) o->back() = payload[size - 1];
}

// ------------------------------------------------------------ the compress side of the split
bool split_slot(const avr_slice_desc& d, size_t split_bytes, uint64_t* cap, uint64_t* out_capacity) {
  if (!split_bytes || split_bytes >= ((size_t)1 << 28) || d.structure != AVR_STRUCT_FRAME || d.mb_width < 1 ||
      d.mb_width > avr::kMringCols || 2 * (uint64_t)d.payload_size < 3 * (uint64_t)split_bytes)
    return false;
  *cap = 8ull * d.payload_size / (8ull * split_bytes) + 1;
  *out_capacity = 2ull * d.payload_size + 256 + 64 * *cap;
  return true;
}

int seams_build(const avr_slice_desc* descs, int n, const uint8_t* arena, size_t arena_len, const avr_slice_result* res,
                const avr_split_slot* slots, const uint32_t* cuts, const uint32_t* piece_end, int n_recs,
                const uint8_t* recs, size_t rec_stride, bool check_cuts, int32_t misfit, std::vector<SliceSeams>* out) {
  out->assign(n, SliceSeams());
  // every index first: nothing below reads out of range
  for (int k = 0; k < n; k++) {
    const avr_split_slot& s = slots[k];
    const avr_slice_desc& d = descs[k];
    SliceSeams& o = (*out)[k];
    o.status = res[k].status;
    bool fits = true;
    if (s.first == -1 && s.cap == 0) {
      fits = cuts[k] == 0;
    } else if (s.first < 0 || s.cap == 0 || (uint64_t)s.first + s.cap > (uint64_t)n_recs || cuts[k] >= s.cap) {
      fits = false;
    } else if (!o.status) {
      // (slice_type / cabac_init_idc index the context init tables of the field's state XOR)
      fits = d.mb_width >= 1 && d.mb_width <= avr::kMringCols && rec_stride >= avr::seam_rec_bytes(d.mb_width) &&
             d.payload_offset <= arena_len && d.payload_size <= arena_len - d.payload_offset && d.slice_type >= 0 &&
             d.slice_type <= 2 && (d.slice_type == 2 || (d.cabac_init_idc >= 0 && d.cabac_init_idc <= 2));
      uint32_t prev = 0;
      for (uint32_t i = 0; fits && i <= cuts[k]; i++) {
        const uint32_t e = piece_end[s.first + i];
        fits = e >= prev;
        o.piece_len.push_back(e - prev);
        prev = e;
      }
      fits = fits && prev == res[k].out_len;
    }
    if (fits) continue;
    if (!misfit) return AVR_ERR_INVALID_ARGUMENT;
    o.status = misfit;
  }
  for (int k = 0; k < n; k++) {
    SliceSeams& o = (*out)[k];
    const uint32_t nc = cuts[k];
    if (o.status || !nc) continue;
    const avr_slice_desc& d = descs[k];
    std::vector<const avr::SeamRec*> rp;
    std::vector<SeamCe> ce(nc);
    // copies of the records: the caller's buffer and stride need not be aligned for a SeamRec
    const size_t rb = avr::seam_rec_bytes(d.mb_width);
    std::vector<uint64_t> copy((rb / 8 + 1) * nc);
    for (uint32_t i = 0; i < nc; i++) {
      uint64_t* raw = copy.data() + (rb / 8 + 1) * i;
      memcpy(raw, recs + (size_t)((uint32_t)slots[k].first + i) * rec_stride, rb);
      const avr::SeamRec& r = *(const avr::SeamRec*)raw;
      SeamCe& c = ce[i];
      if (check_cuts) {
        const uint64_t bitpos = 8ull * r.cd_next - r.cd_k;
        if (r.cd_k >= 32 || 8ull * r.cd_next < r.cd_k ||
            !seam_encoder(arena + d.payload_offset, d.payload_size, bitpos, r.cd_low >> r.cd_k, r.cd_range, &c) ||
            c.q != r.q || c.low != r.ce_low || c.range != r.ce_range || c.outstanding != r.ce_outstanding ||
            c.cache != r.ce_cache || c.queue != r.ce_queue) {
          o.status = AVR_SLICE_CODER;
          break;
        }
      } else {
        c = SeamCe{r.q, r.ce_low, r.ce_outstanding, r.ce_cache, r.ce_range, r.ce_queue};
      }
      rp.push_back(&r);
      o.first_mb.push_back(r.first_mb);
      o.q.push_back(c.q);
    }
    if (!o.status && !seams_encode(rp, ce, d, o.piece_len, &o.field)) return AVR_ERR_OUT_OF_MEMORY;
  }
  return AVR_OK;
}

}  // namespace avr_host

// ------------------------------------------------------------ the split compress of slice batches
// (include/avrecode.h, ABI 8): the rule and sizes, and the seams step, for a caller that ran the split
// walk over its own device buffers.  Everything read here is the caller's.
extern "C" {

int avr_split_plan(const avr_slice_desc* descs, int n, size_t split_bytes, avr_split_slot* slots,
                   uint32_t* out_capacity, int* n_recs, size_t* rec_stride, int* n_candidates) {
  if (n < 0 || (n && (!descs || !slots)) || !n_recs || !rec_stride) return AVR_ERR_INVALID_ARGUMENT;
  uint64_t nrec = 0, cap, oc;
  int max_w = 1, cand = 0;
  for (int k = 0; k < n; k++) {
    slots[k] = avr_split_slot{-1, 0};
    if (out_capacity) out_capacity[k] = 0;
    if (!avr_host::split_slot(descs[k], split_bytes, &cap, &oc)) continue;
    if (nrec + cap > INT32_MAX || oc > UINT32_MAX) return AVR_ERR_INVALID_ARGUMENT;
    slots[k] = avr_split_slot{(int32_t)nrec, (uint32_t)cap};
    if (out_capacity) out_capacity[k] = (uint32_t)oc;
    nrec += cap;
    max_w = std::max(max_w, (int)descs[k].mb_width);
    cand++;
  }
  *n_recs = (int)nrec;
  *rec_stride = avr::seam_rec_bytes(max_w);
  if (n_candidates) *n_candidates = cand;
  return AVR_OK;
}

int avr_seams_build(const avr_slice_desc* descs, int n, const uint8_t* arena, size_t arena_len,
                    const avr_slice_result* res, const avr_split_slot* slots, const uint32_t* cuts,
                    const uint32_t* piece_end, int n_recs, const uint8_t* recs, size_t recs_len, size_t rec_stride,
                    int check_cuts, int32_t* status, uint8_t** seams, size_t* seams_len, uint64_t* offsets,
                    uint32_t* lens) {
  using namespace avr_host;
  if (n < 0 || n_recs < 0 || !seams || !seams_len ||
      (n && (!descs || !arena || !res || !slots || !cuts || !status || !offsets || !lens)) ||
      (n_recs && (!piece_end || !recs)) || (n_recs && (rec_stride == 0 || recs_len / rec_stride < (size_t)n_recs)))
    return AVR_ERR_INVALID_ARGUMENT;
  *seams = nullptr;
  *seams_len = 0;
  return guarded(nullptr, [&]() -> int {
    std::vector<SliceSeams> ss;
    if (int r = seams_build(descs, n, arena, arena_len, res, slots, cuts, piece_end, n_recs, recs, rec_stride,
                            check_cuts != 0, 0, &ss))
      return r;
    size_t total = 0;
    for (const SliceSeams& s : ss) {
      if (s.field.size() > UINT32_MAX) return AVR_ERR_INVALID_ARGUMENT;
      total += s.field.size();
    }
    uint8_t* o = (uint8_t*)malloc(total ? total : 1);
    if (!o) return AVR_ERR_OUT_OF_MEMORY;
    size_t at = 0;
    for (int k = 0; k < n; k++) {
      status[k] = ss[k].status;
      offsets[k] = at;
      lens[k] = (uint32_t)ss[k].field.size();
      if (lens[k]) memcpy(o + at, ss[k].field.data(), lens[k]);
      at += lens[k];
    }
    *seams = o;
    *seams_len = total;
    return AVR_OK;
  });
}

}  // extern "C"

