// The slice kernels and their host launchers: one slice on a workgroup (single-wave or walker +
// modeler + coder), the resident, persistent-queue and split launches of the parallel model, and
// the reference model's sequential kernel.  Each avr_k_*.hip instantiates what it launches.
#pragma once
#include "avr_walker.h"
#include "avr_coder.h"

namespace avr {

// Single-wave slice (the generator: CABAC encode inline, no coder wave).
template <int MODE, bool RM, bool FLD, bool P32, bool SPL, bool SRD>
AVR_FI void run_slice_inline(Walker<MODE, RM, FLD, P32, SPL, SRD>& w, const avr_slice_desc* d, const uint8_t* in, uint8_t* out,
                             avr_slice_result* res) {
  begin_slice(w, d, in, out);
  profile_slice(w);
  w.rc_writeback();
  w.mc_store();
  int status = w.err;
  if (!status && !w.finished) status = AVR_SLICE_NO_END;
  if (MODE == MODE_GENERATE && w.ce.err) status = AVR_SLICE_CODER;
  if (out_overflow(w.out)) status = AVR_SLICE_OVERFLOW;
  if (__lane_id() == 0) {
    res->out_len = out_total(w.out);
    res->status = status;
    res->bins = w.bins;
    res->mbs = (uint32_t)w.mbs_done;
    for (int i = 0; i < 6; i++) res->bill[i] = 0;
  }
}

// Copy the per-bin lookup tables into this workgroup's LDS (16 B per thread per step).
AVR_FI void load_hot_tables(Shared* sh, const EngineTables* G) {
  const uint4* src = (const uint4*)&G->hot;
  uint4* dst = (uint4*)&sh->tab;
  for (int i = threadIdx.x; i < (int)(sizeof(HotTables) / 16); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// Threads per workgroup: two waves (walker + coder) for compress / decompress, one for generate.
template <int MODE>
constexpr int slice_threads() {
  return MODE == MODE_GENERATE || MODE == MODE_TRACE ? 64 : MODE == MODE_COMPRESS ? 192 : 128;
}

// One slice of a parallel launch on this workgroup (every thread): the hot tables are in LDS
// already; est_g is the slice's estimator scratch; cell = the walker's CU-board cell (kNoCell:
// register one).
// MG: the launch may keep the model row in global scratch (the persistent kernel, which every wide
// launch uses); the resident kernel's row is always in LDS (a constant: no branch at its accesses).
template <int MODE, bool FLD, bool P32, bool MG, bool SPL = false>
AVR_FI void parallel_slice(uint8_t* smem, const EngineTables* G, const avr_slice_desc* descs, int s, const uint8_t* in,
                           uint8_t* out, avr_slice_result* res, uint16_t* est_g, uint32_t flags, uint32_t cell,
                           const SplitArgs* sp = nullptr) {
  const avr_slice_desc* d = &descs[s];
  // MG is the persistent queue kernel: its walker keeps the scalar recoded decoder (Walker SRD)
  typedef Walker<MODE, false, FLD, P32, SPL, MG> WalkerT;
  WalkerT w;
  w.sh = (Shared*)smem;
  w.ring = (typename WalkerT::ERec*)(smem + sizeof(Shared));
  bool seam_end = false;
  uint32_t* piece_end = nullptr;
  if constexpr (SPL) {
    const PieceCtl c = sp->ctl[s];
    w.seam = c.seam >= 0 ? (const SeamRec*)(sp->recs + (size_t)c.seam * sp->rec_stride) : nullptr;
    w.piece_mbs = c.n_mbs;
    w.cut = 0;
    seam_end = c.n_mbs != 0;
    piece_end = MODE == MODE_COMPRESS && c.snap >= 0 && sp->piece_end ? sp->piece_end + c.snap : nullptr;
    w.snap = MODE == MODE_COMPRESS && c.snap >= 0 ? sp->recs + (size_t)c.snap * sp->rec_stride : nullptr;
    w.snap_cap = c.snap_cap;
    w.snap_n = 0;
    w.snap_last = 0;
    w.snap_q = 0;
    w.split_bits = sp->split_bits;
    w.rec_stride = sp->rec_stride;
    w.snap_count = sp->snap_n ? sp->snap_n + s : nullptr;
  }
  w.mring_global = MG && !FLD && (flags & kFlagMringGlobal);
  w.mring = w.mring_global ? (uint32_t*)(est_g + kEstMring)
                           : (uint32_t*)(smem + sizeof(Shared) + (size_t)(flags >> kFlagRingShift) * sizeof(EdgeCore));
  w.prio_cell = cell;
  w.T = &w.sh->tab;
  w.G = G;
  w.frames = nullptr;
  w.cur_off = 0;
  w.prev_off = -1;
  w.gmode = false;
  w.gsink = nullptr;
  w.gcount = 0;
  w.est_g = est_g;
  w.ring_cols = flags >> kFlagRingShift;
  if (!d->coded) {
    if (threadIdx.x == 0) {
      res[s].out_len = 0;
      res[s].status = 1;
      res[s].bins = 0;
      res[s].mbs = 0;
      for (int i = 0; i < 6; i++) res[s].bill[i] = 0;
    }
    return;
  }
  // fresh model for this slice: undo the last model's stores to the HBM estimator table
  if (MODE == MODE_COMPRESS || MODE == MODE_DECOMPRESS) est_table_reset(w.est_g, w.sh);
  w.d = d;
  w.W = d->mb_width;
  if ((MODE == MODE_COMPRESS || MODE == MODE_DECOMPRESS) && threadIdx.x == 0) w.sh->prio = 0;   // before init_slice_state's barrier
  init_slice_state(w, G);
  if (MODE == MODE_GENERATE || MODE == MODE_TRACE) {
    run_slice_inline(w, d, in, out, &res[s]);
    return;
  }
  const int wave = threadIdx.x >> 6;
  AVR_PLACE(s, wave);
  if (wave == 0) {
    AVR_PLACE_T(s, 0);
    walker_slice(w, d, in, &res[s]);
    AVR_PLACE_T(s, 1);
  }
  else if (MODE == MODE_COMPRESS && wave == 1) model_slice<SPL>(w.sh, w.est_g);
  else if constexpr (SPL) coder_slice<MODE, P32, false, true>(w.sh, w.T, d, out, flags, w.seam, seam_end, piece_end);
  else coder_slice<MODE, P32>(w.sh, w.T, d, out, flags);
  __syncthreads();
  if (threadIdx.x == 0) finish_slice<MODE>(w.sh, d, &res[s], seam_end);
}

// The long-slice split's launches (avr_kernels.h SplitArgs): progressive frame slices and pieces of
// the parallel model on either of its coders, the model row in LDS; each workgroup
// takes descriptors blockIdx.x, blockIdx.x + gridDim.x, ... (a grid of at most the resident slots:
// one estimator scratch per workgroup).  Compress: whole long slices in a single walk, each cut as
// it is walked -- the cut records taken (PieceCtl::snap) and the model started afresh at every cut;
// or pieces (seam >= 0: started from a record, n_mbs > 0: stopped at the next cut).  Decompress: the
// pieces, from records the host wrote (the container's seams).
// P32: the same launches on the P32 coder (avr_k_split32.hip; the cuts do not depend on the coder).
template <int MODE, bool P32 = false>
__global__ __launch_bounds__(192, 4) void slices_split_kernel(const EngineTables* G, const avr_slice_desc* descs, int n,
                                                             const uint8_t* in, uint8_t* out, avr_slice_result* res,
                                                             uint16_t* est_scratch, SplitArgs sp, uint32_t flags) {
  extern __shared__ __align__(16) uint8_t smem[];
  uint32_t cell = kNoCell;
  bool loaded = false;
  for (int s = blockIdx.x; s < n; s += gridDim.x) {
    __syncthreads();   // the previous descriptor's finish_slice has read the workgroup's LDS
    if (!loaded) {
      load_hot_tables((Shared*)smem, G);
      loaded = true;
      if (threadIdx.x < 64) cell = cu_cell();
    }
    parallel_slice<MODE, false, P32, false, true>(smem, G, descs, s, in, out, res,
                                                  est_scratch + (size_t)blockIdx.x * kEstGlobal, flags, cell, &sp);
  }
}

// FLD = false: the progressive frames of the batch; FLD = true: its field pictures and MBAFF frames
// (a second launch over the same batch: each kernel leaves the other's slices alone).
//
// Two ways to run a batch:
//  - qhead == nullptr: workgroup b runs slice order[b] (the CU grouping of schedule_kernel) or b,
//    with the estimator scratch of that slice -- a batch that is resident all at once;
//  - qhead != nullptr (a batch larger than the chip holds at once): a persistent grid of about one
//    workgroup per resident slot; each workgroup takes the next entry of the queue `order` (the
//    slices sorted largest first, queue_order_kernel) by an atomic on *qhead until the queue is
//    empty, with one estimator scratch per workgroup (est_table_reset undoes the previous slice's
//    stores).  Every workgroup leaves when it draws past the end, so the grid always drains.
//    Largest first is LPT: the batch ends on small slices instead of on a large one started late,
//    and there are no launch boundaries inside the batch to wait at.
template <int MODE, bool FLD, bool P32 = false>
__global__ __launch_bounds__(192, 4) void slices_parallel_kernel(const EngineTables* G, const avr_slice_desc* descs, int n,
                                                                const uint8_t* in, uint8_t* out, avr_slice_result* res,
                                                                uint16_t* est_scratch, const int* order,
                                                                uint32_t flags) {
  extern __shared__ __align__(16) uint8_t smem[];
  if ((int)blockIdx.x >= n) return;
  const int s = order ? order[blockIdx.x] : (int)blockIdx.x;   // CU grouping (schedule_kernel)
  if ((descs[s].structure != AVR_STRUCT_FRAME) != FLD) return;
  load_hot_tables((Shared*)smem, G);
  parallel_slice<MODE, FLD, P32, false>(smem, G, descs, s, in, out, res, est_scratch + (size_t)s * kEstGlobal, flags,
                                        kNoCell);
}

// The persistent variant (a kernel of its own: the loop's state would change the resident
// kernel's register allocation): about one workgroup per resident slot, each taking the next entry
// of the largest-first queue by an atomic on *qhead until the queue is empty.
template <int MODE, bool FLD, bool P32 = false>
__global__ __launch_bounds__(192, 4) void slices_queue_kernel(const EngineTables* G, const avr_slice_desc* descs, int n,
                                                             const uint8_t* in, uint8_t* out, avr_slice_result* res,
                                                             uint16_t* est_scratch, const int* queue, uint32_t* qhead,
                                                             uint32_t flags) {
  extern __shared__ __align__(16) uint8_t smem[];
  Shared* sh = (Shared*)smem;
  // the hot tables and the walker wave's CU-board cell are set up at the first slice this
  // workgroup takes (a field-kernel workgroup that finds no field slice does neither).  The other
  // order (both set up before the first draw) hangs the first queue launch of a
  // process in its uninstrumented build only: every instrumented build of it (bounded waits with
  // invariant checks, host-mapped progress records) runs clean and sees no invariant violated, so the
  // hang follows that build's code generation, not an ordering rule of the protocol below.  The
  // build switches for that order and for the instrumented builds were removed in this commit; the
  // parent commit and profiles/r06_queue_hang.md hold them.
  uint32_t cell = kNoCell;
  bool loaded = false;
  for (;;) {
    if (threadIdx.x == 0) *(volatile __attribute__((address_space(3))) uint32_t*)&sh->qnext = atomicAdd(qhead, 1u);
    __syncthreads();
    const uint32_t k = __builtin_amdgcn_readfirstlane(*(volatile __attribute__((address_space(3))) uint32_t*)&sh->qnext);
    __syncthreads();   // every thread has its entry before thread 0 draws again
    if (k >= (uint32_t)n) break;
    const int s = queue[k];
    if ((descs[s].structure != AVR_STRUCT_FRAME) != FLD) continue;
    if (!loaded) {
      load_hot_tables(sh, G);
      loaded = true;
      if ((MODE == MODE_COMPRESS || MODE == MODE_DECOMPRESS) && threadIdx.x < 64) cell = cu_cell();
    }
    parallel_slice<MODE, FLD, P32, true>(smem, G, descs, s, in, out, res, est_scratch + (size_t)blockIdx.x * kEstGlobal,
                                         flags, cell);
  }
}

// Host side of the parallel launches (instantiated in each kernel TU, avr_k_*.hip, with that TU's
// own CU board): the progressive kernel over the batch, then -- when the batch may hold field
// pictures / MBAFF frames -- the field-capable kernel over the same batch (its workgroups for
// progressive slices return at once).  The board starts empty on every launch (cu_cell's slot
// counter must not carry a previous launch's residue).  q.head: the persistent queue launch
// (slices_parallel_kernel) over q.grid workgroups, q.head[0] for the progressive kernel and
// q.head[1] for the field one (both zero on entry).  q.lane (FieldLane): the field kernel runs on a
// stream of its own beside the progressive one, so a mixed batch takes the longer of the two
// kernels instead of their sum.  The two kernels share the board (it ranks the slices of a CU
// whichever kernel walks them; one reset before both) and touch disjoint slices; their persistent
// workgroups take disjoint estimator scratches (the field kernel's after the q.grid progressive ones).
struct QueueLaunch {
  uint32_t* head = nullptr;
  int grid = 0, grid_fld = 0;   // persistent grids of the progressive and the field kernel
  size_t lds_fld = 0;           // LDS of the field kernel (0: the progressive kernel's)
  const FieldLane* lane = nullptr;
};
// KINDS: the kernels a unit instantiates -- both, or the resident ones only with the persistent ones
// in a unit of their own (a unit is what the layout hints' switch covers, avr_engine.h); a launch of
// the kind the unit does not hold is refused.
enum { kLaunchBoth = 0, kLaunchResident = 1, kLaunchQueue = 2 };
template <int MODE, bool P32, int KINDS = kLaunchBoth>
inline hipError_t launch_parallel(const EngineTables* T, const avr_slice_desc* descs, int n, size_t lds,
                                  const uint8_t* in, uint8_t* out, avr_slice_result* res, uint16_t* est,
                                  const int* order, uint32_t flags, hipStream_t stream, QueueLaunch q = QueueLaunch()) {
  const size_t lds_fld = q.lds_fld ? q.lds_fld : lds;
  const bool fields = (flags & kFlagFields) != 0;
  const bool side = fields && q.lane && q.lane->stream;
  if ((KINDS == kLaunchResident && q.head) || (KINDS == kLaunchQueue && !q.head)) return hipErrorInvalidValue;
  if (hipError_t e = reset_cu_board(stream); e != hipSuccess) return e;
  hipStream_t fs = stream;
  if (side) {
    fs = q.lane->stream;
    if (hipError_t e = hipEventRecord(q.lane->fork, stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamWaitEvent(fs, q.lane->fork, 0); e != hipSuccess) return e;
  }
  if (q.head) {
    if constexpr (KINDS != kLaunchResident)
      hipLaunchKernelGGL((slices_queue_kernel<MODE, false, P32>), dim3(q.grid), dim3(slice_threads<MODE>()), lds, stream,
                         T, descs, n, in, out, res, est, order, q.head, flags);
  } else {
    if constexpr (KINDS != kLaunchQueue)
      hipLaunchKernelGGL((slices_parallel_kernel<MODE, false, P32>), dim3(n), dim3(slice_threads<MODE>()), lds, stream,
                         T, descs, n, in, out, res, est, order, flags);
  }
  if (fields) {
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (!side)
      if (hipError_t e = reset_cu_board(stream); e != hipSuccess) return e;
    // beside the progressive kernel, the persistent field workgroups take the scratches after its grid
    uint16_t* est_f = side && q.head ? est + (size_t)q.grid * kEstGlobal : est;
    if (q.head) {
      if constexpr (KINDS != kLaunchResident)
        hipLaunchKernelGGL((slices_queue_kernel<MODE, true, P32>), dim3(q.grid_fld), dim3(slice_threads<MODE>()), lds_fld,
                           fs, T, descs, n, in, out, res, est_f, order, q.head + 1, flags & ~kFlagMringGlobal);
    } else {
      if constexpr (KINDS != kLaunchQueue)
        hipLaunchKernelGGL((slices_parallel_kernel<MODE, true, P32>), dim3(n), dim3(slice_threads<MODE>()), lds_fld,
                           fs, T, descs, n, in, out, res, est_f, order, flags & ~kFlagMringGlobal);
    }
    if (side) {
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
      if (hipError_t e = hipEventRecord(q.lane->join, fs); e != hipSuccess) return e;
      if (hipError_t e = hipStreamWaitEvent(stream, q.lane->join, 0); e != hipSuccess) return e;
    }
  }
  return hipGetLastError();
}

// Reference model: one workgroup (walker + coder wave) walks every slice of a file in file order
// with persistent estimators and frame metadata.  Several files at once: workgroup f walks file f,
// the slices [file_first[f], file_first[f + 1]) (file_first == nullptr: one file, all n slices),
// with its own estimator table (est_g + f kEstGlobal), frames (frames + f frame_stride) and
// frame_meta[f] -- files share nothing, as separate runs of the reference would not.
// FLD = true when the files may hold field pictures or MBAFF frames (the field-capable walker
// also walks progressive slices); FLD = false refuses such a slice (status -21)
template <int MODE, bool FLD>
__global__ __launch_bounds__(192) void slices_sequential_kernel(const EngineTables* G, const avr_slice_desc* descs, int n,
                                                                  const uint8_t* in, uint8_t* out,
                                                                  avr_slice_result* res, uint16_t* est_g,
                                                                  uint8_t* frames, int* frame_meta,
                                                                  const int* file_first, uint64_t frame_stride,
                                                                  uint32_t flags) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int file = (int)blockIdx.x;
  const int s_begin = file_first ? file_first[file] : 0;
  const int s_end = file_first ? file_first[file + 1] : n;
  est_g += (size_t)file * kEstGlobal;
  frames += (size_t)file * frame_stride;
  frame_meta += file;
  Walker<MODE, true, FLD> w;
  w.sh = (Shared*)smem;
  w.ring = (typename Walker<MODE, true, FLD>::ERec*)(smem + sizeof(Shared));
  w.mring = nullptr;   // the reference model reads its neighbours' model bytes from the frame
  w.mring_global = false;
  load_hot_tables(w.sh, G);
  w.T = &w.sh->tab;
  w.G = G;
  w.est_g = est_g;
  w.frames = frames;
  w.ring_cols = flags >> kFlagRingShift;
  // fresh global model
  {
    uint4* e4 = (uint4*)est_g;
    for (int i = tid; i < kEstGlobal / 8; i += nt) e4[i] = make_uint4(0, 0, 0, 0);
    if (tid == 0) {
      w.sh->elog_n = 0;
      w.sh->prio = 0;
    }
    for (int i = tid; i < kEstDefault + 2; i += nt) w.sh->est[i] = 0;
    for (int i = tid; i < kEtabSize + 64; i += nt) w.sh->etab[i] = 0;
  }
  // frame_meta: [0] cur_frame.  Frame ids / sizes of the two frames, as scalars (no private arrays).
  int cur = 0, fid0 = 0, fid1 = 0, fw0 = 0, fw1 = 0, fh0 = 0, fh1 = 0;
  __syncthreads();
  for (int s = s_begin; s < s_end; s++) {
    const avr_slice_desc* d = &descs[s];
    const int W = d->mb_width, H = d->mb_height;
    // update_frame_spec (recode.cpp:824-843)
    const int fwc = cur ? fw1 : fw0, fhc = cur ? fh1 : fh0, fidc = cur ? fid1 : fid0;
    if (fwc != W || fhc != H || !(fidc == d->picture_id && fwc && fhc)) {
      cur = 1 - cur;
      const int fwn = cur ? fw1 : fw0, fhn = cur ? fh1 : fh0;   // the new current frame
      const int fwo = cur ? fw0 : fw1, fho = cur ? fh0 : fh1;   // the other one
      const bool reinit_other = (fwn != W || fhn != H) && (fwo != W || fho != H);
      // fresh/cleared current frame; a dimension change also clears the other one
      uint32_t* f32 = (uint32_t*)(frames + (size_t)cur * W * H * 52);
      for (int i = tid; i < W * H * 13; i += nt) f32[i] = 0;
      if (reinit_other) {
        uint32_t* o32 = (uint32_t*)(frames + (size_t)(1 - cur) * W * H * 52);
        for (int i = tid; i < W * H * 13; i += nt) o32[i] = 0;
        if (cur) { fw0 = W; fh0 = H; } else { fw1 = W; fh1 = H; }
      }
      if (cur) { fw1 = W; fh1 = H; fid1 = d->picture_id; } else { fw0 = W; fh0 = H; fid0 = d->picture_id; }
      __threadfence_block();
      __syncthreads();
    }
    if (!d->coded || (!FLD && d->structure != AVR_STRUCT_FRAME)) {
      if (tid == 0) {
        res[s].out_len = 0;
        res[s].status = d->coded ? -21 : 1;
        res[s].bins = 0;
        res[s].mbs = 0;
      for (int i = 0; i < 6; i++) res[s].bill[i] = 0;
      }
      continue;
    }
    w.cur_off = (int64_t)cur * W * H * 52;
    w.prev_off = (int64_t)(1 - cur) * W * H * 52;
    w.gmode = false;
    w.gsink = nullptr;
    w.gcount = 0;
    w.d = d;
    w.W = W;
    init_slice_state(w, G);
    const int wave = tid >> 6;
    if (wave == 0) walker_slice(w, d, in, &res[s]);
    else if (MODE == MODE_COMPRESS && wave == 1) model_slice(w.sh, w.est_g);
    else coder_slice<MODE, false, true>(w.sh, w.T, d, out, flags);
    __syncthreads();
    if (tid == 0) finish_slice<MODE>(w.sh, d, &res[s]);
    __syncthreads();
  }
  if (tid == 0) frame_meta[0] = cur;
}

}  // namespace avr
