// The compress planner: parsed files taken into the slice batches the device compresses -- the
// parallel models' candidate pass, the reference-model plan with the chained model's boundaries,
// the chain ranges of the chained model across GPUs, and the frame generations of the parallel
// reference-model pass.  No HIP: the whole-file calls (avr_api.cpp) and the hooks surface
// (avr_hooks.cpp) launch what is planned here, and tests/native/cplan_check.cpp runs it without a
// device.  Every rule that compress and decompress must apply alike is stated here once.
#include <cmath>
#include <cstdlib>

#include "avr_host.h"

namespace avr_host {

int plan_slice(Plan* plan, const avr::SliceInfo& s, uint32_t out_capacity, bool coded) {
  avr_slice_desc d = desc_from_header(s);
  d.coded = coded;
  if (coded) {
    append_aligned(&plan->arena, s.payload(), s.read_limit, 16, &d.payload_offset);
    d.payload_size = (uint32_t)s.size;
    d.read_limit = (uint32_t)s.read_limit;
    d.out_capacity = out_capacity;
    plan->max_w = std::max(plan->max_w, ring_cols(d));
  }
  plan->descs.push_back(d);
  return (int)plan->descs.size() - 1;
}

std::vector<int> chain_starts(const std::vector<char>& coded) {
  std::vector<int> first{0};
  int coded_n = 0;
  for (size_t i = 0; i < coded.size(); i++) {
    if (!coded[i]) continue;
    if (coded_n > 0 && coded_n % AVR_CHAIN_SLICES == 0) first.push_back((int)i);
    coded_n++;
  }
  first.push_back((int)coded.size());
  return first;
}

void append_file_chains(Plan* plan, size_t n0, bool chained) {
  std::vector<char> coded(chained ? plan->descs.size() - n0 : 0);   // not chained: the file is one chain
  for (size_t k = 0; k < coded.size(); k++) coded[k] = plan->descs[n0 + k].coded != 0;
  const std::vector<int> first = chain_starts(coded);
  for (size_t ch = 0; ch + 1 < first.size(); ch++) plan->file_first.push_back((int)n0 + first[ch]);
}

void reference_plan(Plan* rp, const ParsedFile& pf, int lo, int hi, const std::vector<char>& coded, bool chained, int file,
                    std::vector<std::pair<int, int>>* idx) {
  const size_t n0 = rp->descs.size();
  for (int i = lo; i < hi; i++) {
    plan_slice(rp, pf.slices[i], reference_out_capacity(pf.slices[i].size), coded[i] != 0);
    if (idx) idx->push_back({file, i});
  }
  append_file_chains(rp, n0, chained);
}

void plan_candidates(const std::vector<ParsedFile>& pf, const std::vector<int32_t>& st, size_t split_bytes, Plan* batch,
                     std::vector<const avr::SliceInfo*>* split_sl, std::vector<avr_slice_desc>* split_d,
                     std::vector<std::vector<Route>>* route) {
  route->assign(pf.size(), {});
  for (size_t f = 0; f < pf.size(); f++) {
    (*route)[f].assign(pf[f].slices.size(), Route{});
    if (st[f]) continue;
    for (size_t i = 0; i < pf[f].slices.size(); i++) {
      const avr::SliceInfo& s = pf[f].slices[i];
      if (!recodable_candidate(s)) continue;
      avr_slice_desc d = desc_from_header(s);
      d.payload_size = (uint32_t)s.size;
      uint64_t cap, oc;
      if (split_slot(d, split_bytes, &cap, &oc)) {
        (*route)[f][i] = Route{Route::kSplit, (int)split_sl->size()};
        split_sl->push_back(&s);
        split_d->push_back(d);
      } else {
        (*route)[f][i] = Route{Route::kBatch, plan_slice(batch, s, parallel_out_capacity(s.size))};
      }
    }
  }
}

std::pair<int, int> partition_range(const std::vector<double>& w, int world, int rank) {
  const int n = (int)w.size();
  if (world <= 1) return rank == 0 ? std::make_pair(0, n) : std::make_pair(n, n);
  double total = 0;
  for (double x : w) total += x;
  std::vector<int> cuts(world + 1, n);
  if (total <= 0) {
    for (int r = 0; r < world; r++) cuts[r] = (int)std::nearbyint((double)r * n / world);
  } else {
    std::vector<int> owner(n);
    double acc = 0;
    for (int i = 0; i < n; i++) {
      acc += w[i];
      const double mid = acc - w[i] / 2;
      owner[i] = std::min((int)(mid * world / total), world - 1);
    }
    for (int r = 0; r < world; r++) cuts[r] = (int)(std::lower_bound(owner.begin(), owner.end(), r) - owner.begin());
  }
  return {cuts[rank], cuts[rank + 1]};
}

void pack_range(int lo, const std::vector<avr_slice_desc>& descs, const std::vector<avr_slice_result>& res,
                const uint8_t* out, int32_t uncoded, int32_t (*failed)(int32_t), ChainRangeOut* o) {
  const int nr = (int)descs.size();
  o->lo = lo;
  o->hi = lo + nr;
  o->status.assign(nr, uncoded);
  o->offsets.assign(nr, 0);
  o->lens.assign(nr, 0);
  uint64_t total = 0;
  for (int k = 0; k < nr; k++)
    if (descs[k].coded && res[k].status == 0) total += res[k].out_len;
  o->blob.resize(total);
  uint64_t at = 0;
  for (int k = 0; k < nr; k++) {
    if (!descs[k].coded) continue;
    if (res[k].status != 0) {
      o->status[k] = failed(res[k].status);
      continue;
    }
    o->status[k] = 0;
    o->offsets[k] = at;
    o->lens[k] = res[k].out_len;
    if (res[k].out_len) memcpy(o->blob.data() + at, out + descs[k].out_offset, res[k].out_len);
    at += res[k].out_len;
  }
}

// The parallel pass's time is its largest slice's: the scan twice (count, write) and the recoded
// coder, one after the other; the sequential kernel's is its largest file's, with walker, modeler
// and coder overlapped on three waves.  Measured per payload byte of the chain
// (profiles/r05_rcode_ab.txt and r05m_rmode_files_before.log: a 4K 4:4:4 slice of 1.38 MB, scan
// 1.3-1.8 s per pass, coder ~1.5 s per MB; the per-file kernel's compress of a 2-slice such file
// 1.4 s per MB): the parallel pass pays when the largest file's payload exceeds ~3.7 times the
// largest slice's (cockatoo.mp4: 280 slices; a 1-2-slice-per-picture 4K file does not).
// AVR_RMODE_PARALLEL=1 forces the parallel pass (tests), AVR_RMODE_SEQUENTIAL=1 the sequential kernel.
bool rmode_parallel_pays(const Plan& plan) {
  if (getenv("AVR_RMODE_PARALLEL")) return true;
  const int nf = plan.n_files(), n = (int)plan.descs.size();
  uint64_t max_slice = 0, max_file = 0;
  for (int f = 0; f < nf; f++) {
    const int e = f + 1 < nf ? plan.file_begin(f + 1) : n;
    uint64_t fs = 0;
    for (int k = plan.file_begin(f); k < e; k++) {
      const uint64_t s = plan.descs[k].coded ? plan.descs[k].payload_size : 0;
      fs += s;
      max_slice = std::max(max_slice, s);
    }
    max_file = std::max(max_file, fs);
  }
  return max_file * 10 > max_slice * 37;
}

// The generations mirror update_frame_spec (recode.cpp:824-843) as slices_sequential_kernel
// implements it: a slice of another picture, or of another size, takes the other frame and opens a
// generation there; a new size re-initialises the other frame with it (its generation is dropped).
// A plan with more than 4 GiB of frame metadata is left to the sequential kernel.
bool rmode_generations(const Plan& plan, std::vector<int64_t>* goff, int64_t* frame_bytes) {
  const int n = (int)plan.descs.size();
  struct Fb { int gen = -1, w = 0, h = 0, fid = 0; } fb[2];
  std::vector<uint8_t> gen_parity;   // field parities (1 top, 2 bottom) seen per frame generation
  int cur = 0;
  std::vector<int64_t> gen_off;
  goff->assign(2 * (size_t)n, 0);
  int64_t fbytes = 0;
  std::vector<char> file_start(n + 1, 0);
  for (int f = 0; f < plan.n_files(); f++) file_start[plan.file_begin(f)] = 1;
  for (int k = 0; k < n; k++) {
    if (file_start[k]) {   // a new file: a fresh model, frames of its own
      fb[0] = Fb();
      fb[1] = Fb();
      cur = 0;
    }
    const avr_slice_desc& d = plan.descs[k];
    const int W = d.mb_width, H = d.mb_height;
    if (fb[cur].w != W || fb[cur].h != H || !(fb[cur].fid == d.picture_id && fb[cur].w && fb[cur].h)) {
      cur = 1 - cur;
      Fb& nw = fb[cur];
      Fb& ot = fb[1 - cur];
      const bool reinit_other = (nw.w != W || nw.h != H) && (ot.w != W || ot.h != H);
      nw.gen = (int)gen_off.size();
      gen_off.push_back(fbytes);
      gen_parity.push_back(0);
      fbytes += (int64_t)W * H * 52;
      if (reinit_other) {
        ot.gen = -1;
        ot.w = W;
        ot.h = H;
      }
      nw.w = W;
      nw.h = H;
      nw.fid = d.picture_id;
    }
    const Fb& ot = fb[1 - cur];
    // a stale other frame: cannot arise while both frames are re-initialised together, as above
    if (ot.gen >= 0 && (ot.w != W || ot.h != H)) return false;
    (*goff)[2 * k] = gen_off[fb[cur].gen];
    (*goff)[2 * k + 1] = ot.gen < 0 ? -1 : gen_off[ot.gen];
    // a field whose frame has no slice of the other parity yet (its rows are still zero in the
    // sequential model, but filled in the buffer the parallel scan reads): offsets are 4-aligned
    if (d.structure == AVR_STRUCT_TOP_FIELD || d.structure == AVR_STRUCT_BOTTOM_FIELD) {
      uint8_t& seen = gen_parity[fb[cur].gen];
      if (!(seen & (d.structure == AVR_STRUCT_TOP_FIELD ? 2 : 1))) (*goff)[2 * k] |= 1;
      seen |= (uint8_t)(d.structure == AVR_STRUCT_TOP_FIELD ? 1 : 2);
    }
  }
  *frame_bytes = fbytes;
  return fbytes <= ((int64_t)4 << 30);
}

}  // namespace avr_host
