// Host-only mutation harness for the split compress's host steps (avr_split_plan, avr_seams_build in
// avr_seams.cpp; avr_assemble_container_seams(_parsed) in avr_assemble.cpp), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_split_compress_sanitizers.py: g++ alone,
// no ROCm include path, no HIP library (the one device symbol avr_assemble.cpp links against,
// avr::shared_bytes, is a stub below).  A rank runs these on what it read back from its device and on
// what other ranks sent it.
//
//   seams_build_fuzz <iterations> <seed> <split_bytes> <file> <container>
//
// <container> is the oracle's split container of <file>.  Through the public ABI only.  First the
// valid batch -- the file's parse, avr_split_plan's slots, and per slot the cut counts, piece ends
// and records of the container's piece plan, laid out as a split walk leaves them: avr_seams_build
// must give fields with which avr_assemble_container_seams(_parsed) writes the container byte for
// byte.  Then seeded mutations of counts, slots, piece ends, strides, record counts, buffer lengths,
// descriptors, results and the records' coder fields, and of the seams offsets and lengths given to
// the assembly.  Every buffer is a heap allocation of exactly the length passed, so a read past it
// is a sanitizer report; every call must return AVR_OK or a negative status, and an AVR_OK must
// describe fields inside its blob.  Exit status 0 = no report and no broken invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
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

// avr_free is free() and lives with the device side (avr_api.cpp), which is not linked here
void lib_free(void* p) { free(p); }

int fail(const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "FINDING: %s (%ld, %ld)\n", what, a, b);
  return 1;
}

// what avr_seams_build reads, each array a vector of exactly the length the call is told
struct Batch {
  std::vector<avr_slice_desc> descs;
  Buf arena;
  std::vector<avr_slice_result> res;
  std::vector<avr_split_slot> slots;
  std::vector<uint32_t> cuts, piece_end;
  Buf recs;
  int n_recs = 0;
  size_t stride = 0;
};

struct Fields {
  std::vector<int32_t> status;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lens;
  Buf blob;
};

// returns the status; on AVR_OK checks what came back
int build(const Batch& b, int check_cuts, Fields* f, int* finding) {
  const int n = (int)b.descs.size();
  f->status.assign(n, 77);
  f->offsets.assign(n, 0);
  f->lens.assign(n, 0);
  f->blob.clear();
  uint8_t* blob = nullptr;
  size_t blen = 0;
  const int r = avr_seams_build(b.descs.data(), n, b.arena.data(), b.arena.size(), b.res.data(), b.slots.data(),
                                b.cuts.data(), b.piece_end.data(), b.n_recs, b.recs.data(), b.recs.size(), b.stride,
                                check_cuts, f->status.data(), &blob, &blen, f->offsets.data(), f->lens.data());
  if (r > 0) *finding |= fail("positive status", r);
  if (r != AVR_OK) {
    if (blob) *finding |= fail("a blob with an error");
    return r;
  }
  if (!blob) {
    *finding |= fail("AVR_OK without a blob");
    return r;
  }
  for (int k = 0; k < n; k++) {
    if (f->offsets[k] > blen || f->lens[k] > blen - f->offsets[k]) *finding |= fail("field outside the blob", k);
    if (f->lens[k] && f->status[k]) *finding |= fail("a field on a failed slice", k);
    if (f->status[k] != b.res[k].status && f->status[k] != AVR_SLICE_CODER) *finding |= fail("status", k, f->status[k]);
  }
  f->blob.assign(blob, blob + blen);
  lib_free(blob);
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const long iters = atol(argv[1]);
  std::mt19937_64 rng((uint64_t)atoll(argv[2]));
  const size_t split_bytes = (size_t)atoll(argv[3]);
  const Buf file = read_file(argv[4]), avrc = read_file(argv[5]);
  if (file.empty() || avrc.empty()) return 2;
  int finding = 0;

  // ---- the valid batch
  avr_slice_desc* pd = nullptr;
  uint8_t* pa = nullptr;
  int n = 0, mw = 0, mh = 0;
  size_t alen = 0, wlen = 0;
  if (avr_parse_stream(file.data(), file.size(), &pd, &n, &pa, &alen, &wlen, &mw, &mh) != AVR_OK || n <= 0) return 2;
  Batch v;
  v.descs.assign(pd, pd + n);
  v.arena.assign(pa, pa + alen);
  lib_free(pd);
  lib_free(pa);
  v.slots.resize(n);
  std::vector<uint32_t> cap(n);
  int ncand = 0;
  size_t plan_stride = 0;
  if (avr_split_plan(v.descs.data(), n, split_bytes, v.slots.data(), cap.data(), &v.n_recs, &plan_stride, &ncand) != AVR_OK ||
      ncand <= 0)
    return fail("avr_split_plan on the parse");

  avr_dec_plan* plan = nullptr;
  int ns = 0, nu = 0, pw = 0, ph = 0, nr = 0;
  size_t parena = 0, pwork = 0, stride = 0;
  if (avr_dec_plan_new(&plan) != AVR_OK ||
      avr_dec_plan_load_pieces(plan, avrc.data(), avrc.size(), &ns, &nu, &parena, &pwork, &pw, &ph, &nr, &stride) != AVR_OK)
    return 2;
  std::vector<avr_slice_desc> sd(ns), ud(nu);
  std::vector<avr_piece> pc(nu);
  Buf prec((size_t)nr * stride), streams(parena);
  if (avr_dec_plan_descs(plan, sd.data()) != AVR_OK || avr_dec_plan_units(plan, ud.data(), pc.data()) != AVR_OK ||
      avr_dec_plan_recs(plan, prec.data(), prec.size()) != AVR_OK ||
      avr_dec_plan_arena(plan, streams.data(), streams.size()) != AVR_OK || stride < plan_stride)
    return 2;
  v.stride = stride;
  v.res.assign(n, avr_slice_result{});
  v.cuts.assign(n, 0);
  v.piece_end.assign(v.n_recs, 0);
  v.recs.assign((size_t)v.n_recs * stride, 0);
  // the plan's coded slices are the parse's coded slices the container holds, in order
  std::vector<int32_t> status(n, -1);
  std::vector<uint64_t> offsets(n, 0);
  std::vector<uint32_t> lens(n, 0);
  Buf recoded;
  int u = 0, i = 0;
  for (int j = 0; j < ns; j++) {
    while (i < n && !(v.descs[i].coded && v.descs[i].picture_id == sd[j].picture_id && v.descs[i].first_mb == sd[j].first_mb))
      v.res[i++].status = -1;
    if (i >= n) return fail("a coded slice of the container is not in the parse", j);
    offsets[i] = recoded.size();
    uint32_t total = 0, pieces = 0;
    const int32_t first = v.slots[i].first;
    for (; u < nu && pc[u].slice == j; u++, pieces++) {
      recoded.insert(recoded.end(), streams.begin() + ud[u].payload_offset,
                     streams.begin() + ud[u].payload_offset + ud[u].payload_size);
      total += ud[u].payload_size;
      if (first >= 0) v.piece_end[first + pieces] = total;
      if (pieces) {
        if (first < 0 || pieces >= v.slots[i].cap || pc[u].seam < 0) return fail("a cut outside its slot", j);
        memcpy(v.recs.data() + (size_t)(first + pieces - 1) * stride, prec.data() + (size_t)pc[u].seam * stride, stride);
      }
    }
    if (!pieces) return fail("a coded slice without a unit", j);
    v.cuts[i] = pieces - 1;
    v.res[i].out_len = lens[i] = total;
    status[i] = 0;
    i++;
  }
  for (; i < n; i++) v.res[i].status = -1;
  avr_dec_plan_free(plan);
  recoded.resize(recoded.size() + 16, 0);

  Fields f;
  if (build(v, 0, &f, &finding) != AVR_OK) return fail("the valid batch is refused");
  int cut = 0;
  for (int k = 0; k < n; k++) cut += f.lens[k] != 0;
  if (!cut) return fail("no field built");
  for (int parsed = 0; parsed < 2; parsed++) {
    uint8_t* out = nullptr;
    size_t olen = 0;
    const int r = parsed ? avr_assemble_container_seams_parsed(file.data(), file.size(), AVR_MODEL_PARALLEL, v.descs.data(), n,
                                                               v.arena.data(), v.arena.size(), status.data(), recoded.data(),
                                                               recoded.size(), offsets.data(), lens.data(), f.blob.data(),
                                                               f.blob.size(), f.offsets.data(), f.lens.data(), &out, &olen)
                         : avr_assemble_container_seams(file.data(), file.size(), AVR_MODEL_PARALLEL, n, status.data(),
                                                        recoded.data(), recoded.size(), offsets.data(), lens.data(),
                                                        f.blob.data(), f.blob.size(), f.offsets.data(), f.lens.data(), &out,
                                                        &olen);
    if (r != AVR_OK || olen != avrc.size() || memcmp(out, avrc.data(), olen) != 0)
      finding |= fail("the assembled container is not the oracle's", r, (long)olen);
    lib_free(out);
  }
  Fields g;
  if (build(v, 1, &g, &finding) != AVR_OK) finding |= fail("the valid batch is refused with check_cuts");
  for (int k = 0; k < n; k++)   // the plan's records carry no decoder state
    if ((v.cuts[k] != 0) != (g.status[k] == AVR_SLICE_CODER) || g.lens[k]) finding |= fail("check_cuts on zero cd_*", k);

  // ---- mutations
  static const uint32_t kVals[] = {0u, 1u, 2u, 15u, 16u, 0xffu, 1087u, 1088u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  auto val = [&](uint32_t old) -> uint32_t {
    switch (rng() % 5) {
      case 0: return old + 1;
      case 1: return old - 1;
      case 2: return (uint32_t)rng();
      case 3: return (uint32_t)(rng() % 4096);
      default: return kVals[rng() % (sizeof(kVals) / sizeof(kVals[0]))];
    }
  };
  long ok = 0, refused = 0, asm_ok = 0, asm_refused = 0;
  for (long it = 0; it < iters && !finding; it++) {
    Batch b = v;
    const int m = 1 + (int)(rng() % 3);
    for (int q = 0; q < m; q++) {
      const int k = (int)(rng() % n);
      switch (rng() % 12) {
        case 0: b.cuts[k] = val(b.cuts[k]); break;
        case 1: b.slots[k].first = (int32_t)val((uint32_t)b.slots[k].first); break;
        case 2: b.slots[k].cap = val(b.slots[k].cap); break;
        case 3:
          if (!b.piece_end.empty()) {
            uint32_t& e = b.piece_end[rng() % b.piece_end.size()];
            e = val(e);
          }
          break;
        case 4: b.stride = rng() % 3 ? val((uint32_t)b.stride) : (size_t)rng(); break;
        case 5: {   // another record count: the piece ends follow it, the records may or may not
          b.n_recs = (int)(val((uint32_t)b.n_recs) % 600);
          b.piece_end.resize(b.n_recs, 0);
          if (rng() % 2 && b.stride < (1u << 13)) b.recs.resize((size_t)b.n_recs * b.stride, 0);
          break;
        }
        case 6: b.recs.resize(rng() % (b.recs.size() + 1)); break;
        case 7: b.arena.resize(rng() % (b.arena.size() + 1)); break;
        case 8: {
          avr_slice_desc& d = b.descs[k];
          switch (rng() % 4) {
            case 0: d.mb_width = (int32_t)val((uint32_t)d.mb_width); break;
            case 1: d.payload_offset = rng() % 2 ? val((uint32_t)d.payload_offset) : rng(); break;
            case 2: d.payload_size = val(d.payload_size); break;
            default: d.slice_qp = (int32_t)val((uint32_t)d.slice_qp), d.slice_type = (int32_t)(rng() % 5), d.cabac_init_idc = (int32_t)val(0); break;
          }
          break;
        }
        case 9:
          if (rng() % 2) b.res[k].out_len = val(b.res[k].out_len);
          else b.res[k].status = (int32_t)(rng() % 3) - 1;
          break;
        default: {   // a record's coder fields: the decoder state the cut check restates from, the re-encoder's
          if (b.recs.size() < 64) break;
          const size_t nrec = b.stride ? b.recs.size() / b.stride : 0;
          if (!nrec) break;
          uint8_t* r = b.recs.data() + (rng() % nrec) * b.stride;
          if (r + 64 > b.recs.data() + b.recs.size()) break;
          const int field = (int)(rng() % 12);
          uint32_t x;
          memcpy(&x, r + 4 * field, 4);
          x = val(x);
          if (field == 5 && rng() % 2) x = (uint32_t)(rng() % 4096);   // cd_next inside the payload
          if (field == 4 && rng() % 2) x = (uint32_t)(rng() % 40);     // cd_k
          memcpy(r + 4 * field, &x, 4);
          break;
        }
      }
    }
    // exact-size heap copies (vectors shrink their capacity on copy-assign only by luck: force it)
    Batch e;
    e.descs.assign(b.descs.begin(), b.descs.end());
    e.arena = Buf(b.arena.begin(), b.arena.end());
    e.res = b.res;
    e.slots = b.slots;
    e.cuts = b.cuts;
    e.piece_end = std::vector<uint32_t>(b.piece_end.begin(), b.piece_end.end());
    e.recs = Buf(b.recs.begin(), b.recs.end());
    e.arena.shrink_to_fit();
    e.piece_end.shrink_to_fit();
    e.recs.shrink_to_fit();
    e.n_recs = b.n_recs;
    e.stride = b.stride;
    Fields h;
    const int r = build(e, (int)(rng() % 2), &h, &finding);
    if (r == AVR_OK) ok++;
    else refused++;
    if (r != AVR_OK && r != AVR_ERR_INVALID_ARGUMENT && r != AVR_ERR_OUT_OF_MEMORY) finding |= fail("undocumented status", r);
    if (it % 4) continue;
    // the assembly with mutated seams offsets / lengths / statuses / model, on the valid fields
    std::vector<uint64_t> so = f.offsets;
    std::vector<uint32_t> sl = f.lens;
    std::vector<int32_t> st = status;
    Buf blob = f.blob;
    int model = AVR_MODEL_PARALLEL;
    const int k = (int)(rng() % n);
    switch (rng() % 6) {
      case 0: so[k] = rng() % 2 ? val((uint32_t)so[k]) : rng(); break;
      case 1: sl[k] = val(sl[k]); break;
      case 2: st[k] = (int32_t)(rng() % 3) - 1; break;
      case 3: blob.resize(rng() % (blob.size() + 1)); blob.shrink_to_fit(); break;
      case 4: model = (int)(rng() % 6) - 1; break;
      default: break;
    }
    uint8_t* out = nullptr;
    size_t olen = 0;
    const int ra = rng() % 8 ? avr_assemble_container_seams_parsed(file.data(), file.size(), model, v.descs.data(), n,
                                                                   v.arena.data(), v.arena.size(), st.data(), recoded.data(),
                                                                   recoded.size(), offsets.data(), lens.data(), blob.data(),
                                                                   blob.size(), so.data(), sl.data(), &out, &olen)
                               : avr_assemble_container_seams(file.data(), file.size(), model, n, st.data(), recoded.data(),
                                                              recoded.size(), offsets.data(), lens.data(), blob.data(),
                                                              blob.size(), so.data(), sl.data(), &out, &olen);
    if (ra > 0) finding |= fail("assembly: positive status", ra);
    if (ra == AVR_OK) {
      asm_ok++;
      if (!out || !olen) finding |= fail("assembly: AVR_OK without a container");
    } else {
      asm_refused++;
      if (out) finding |= fail("assembly: a container with an error");
    }
    lib_free(out);
  }
  printf("%ld batches: %ld built, %ld refused; %ld assemblies: %ld written, %ld refused\n", iters, ok, refused,
         asm_ok + asm_refused, asm_ok, asm_refused);
  if (finding) return 1;
  printf("no finding\n");
  return 0;
}
