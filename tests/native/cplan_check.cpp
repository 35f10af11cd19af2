// Host-only checks of the compress planner (avrecode_amd/csrc/avr_cplan.cpp) and of the one-line
// rules in avr_host.h, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_cplan_host.py: g++ alone, no ROCm include path, no HIP library (avr::shared_bytes, the
// one device symbol avr_assemble.cpp links against, is a stub below).
//
//   cplan_check chain                       the chain rule against a brute-force statement of it
//   cplan_check cut <file> <container>      compress and decompress cut a chained file alike
//   cplan_check partition <cases>           partition_range against recorded shard.partition answers
//   cplan_check rmode                       the frame generations of the parallel reference-model pass
//   cplan_check lastbyte                    the last-byte rule's three outcomes
//
// Exit status 0 and "no finding" = every expectation held.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>

#include "../../avrecode_amd/csrc/avr_host.h"

namespace avr {
size_t shared_bytes(int) { return 0; }   // the kernels' LDS need (avr_kernels.hip): not linked here
}  // namespace avr

using namespace avr_host;

namespace {

int findings = 0;
void finding(const char* what, long a = 0, long b = 0, long c = 0) {
  fprintf(stderr, "FINDING: %s (%ld, %ld, %ld)\n", what, a, b, c);
  findings++;
}

std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// ---- 1) the chain rule.  Stated by brute force: slice i starts a chain when it is the file's first
// slice, or when it is coded and the coded slices before it number a positive multiple of
// AVR_CHAIN_SLICES; the slice count closes the list.
std::vector<int> brute_chain_starts(const std::vector<char>& coded) {
  std::vector<int> first;
  for (size_t i = 0; i < coded.size(); i++) {
    int before = 0;
    for (size_t j = 0; j < i; j++) before += coded[j] != 0;
    if (i == 0 || (coded[i] && before > 0 && before % AVR_CHAIN_SLICES == 0)) first.push_back((int)i);
  }
  if (coded.empty()) first.push_back(0);
  first.push_back((int)coded.size());
  return first;
}

void check_chain() {
  static const int kCoded[] = {0, 1, 15, 16, 17, 32, 33};
  static const int kUncoded[] = {0, 1, 3};
  int cases = 0;
  for (int n_coded : kCoded)
    for (int u : kUncoded)
      for (int where = 0; where < 3; where++) {   // uncoded slices before / after / around each multiple of 16
        std::vector<char> coded;
        for (int j = 0; j < n_coded; j++) {
          if (j % AVR_CHAIN_SLICES == 0 && where != 1) coded.insert(coded.end(), u, 0);
          coded.push_back(1);
          if (j % AVR_CHAIN_SLICES == 0 && where != 0) coded.insert(coded.end(), u, 0);
        }
        if (!n_coded) coded.assign(u, 0);
        const std::vector<int> want = brute_chain_starts(coded);
        if (chain_starts(coded) != want) finding("chain_starts differs from the rule", n_coded, u, where);
        const int chains = (n_coded + AVR_CHAIN_SLICES - 1) / AVR_CHAIN_SLICES;
        if ((int)want.size() - 1 != std::max(1, chains)) finding("the rule's own chain count", n_coded, u, where);
        // the appender: the file's slices after those of an earlier file
        for (int chained = 0; chained < 2; chained++) {
          Plan plan;
          plan.descs.resize(5 + coded.size());
          for (auto& d : plan.descs) memset(&d, 0, sizeof(d)), d.coded = 1;
          for (size_t k = 0; k < coded.size(); k++) plan.descs[5 + k].coded = coded[k];
          plan.file_first.push_back(0);
          append_file_chains(&plan, 5, chained != 0);
          std::vector<int> cuts{0};
          for (size_t ch = 0; ch + 1 < want.size() && (chained || ch == 0); ch++) cuts.push_back(5 + want[ch]);
          if (plan.file_first != cuts) finding("append_file_chains differs from the rule", n_coded, u, where);
        }
        cases++;
      }
  printf("chain: %d flag vectors\n", cases);
}

// ---- 2) both directions cut alike: the reference plan of the file (parse, segmentation with every
// recodable candidate, the plan builder with the chained model) against the decompress plan of its
// chained container (decompress_setup, then the appender).
int check_cut(const char* file_path, const char* container_path) {
  const std::vector<uint8_t> file = read_file(file_path), avrc = read_file(container_path);
  if (file.empty() || avrc.empty()) return 2;
  ParsedFile pf;
  if (parse_file(nullptr, file.data(), file.size(), &pf, /*views=*/true) != AVR_OK) return 2;
  const size_t ns = pf.slices.size();
  std::vector<char> ok(ns), coded(ns);
  for (size_t i = 0; i < ns; i++) ok[i] = recodable_candidate(pf.slices[i]);
  const std::vector<const uint8_t*> found = segment(file.data(), file.size(), pf, ok);
  size_t n_coded = 0;
  for (size_t i = 0; i < ns; i++) n_coded += coded[i] = found[i] != nullptr;
  Plan cp;
  std::vector<std::pair<int, int>> idx;
  reference_plan(&cp, pf, 0, (int)ns, coded, /*chained=*/true, 0, &idx);
  cp.file_first.push_back((int)cp.descs.size());

  DecJob job;
  Plan dp;
  if (decompress_setup(nullptr, avrc.data(), avrc.size(), &job, &dp) != AVR_OK) return 2;
  if (job.model != AVR_MODEL_CHAINED) finding("not a chained-model container", job.model);
  append_file_chains(&dp, 0, /*chained=*/true);
  dp.file_first.push_back((int)dp.descs.size());

  size_t d_coded = 0;
  for (const auto& d : dp.descs) d_coded += d.coded != 0;
  // the premise: the oracle coded every candidate the segmentation found
  if (d_coded != n_coded) finding("the container's coded slices are not the file's candidates", (long)d_coded, (long)n_coded);
  if (cp.descs.size() != dp.descs.size()) finding("descriptor counts differ", (long)cp.descs.size(), (long)dp.descs.size());
  if (idx.size() != cp.descs.size()) finding("one (file, slice) index per descriptor", (long)idx.size());
  if (cp.file_first != dp.file_first) finding("compress and decompress cut differently", (long)cp.file_first.size(), (long)dp.file_first.size());
  printf("cut: %zu slices, %zu coded, %zu chains\n", cp.descs.size(), n_coded, cp.file_first.size() - 1);
  return 0;
}

// ---- 3) partition_range against shard.partition.  A case per line: world, n, the n weights, then
// shard.partition's lo hi per rank.
int check_partition(const char* path) {
  std::ifstream f(path);
  std::string line;
  int cases = 0;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    int world = 0, n = -1;
    if (!(ls >> world >> n) || world < 1 || n < 0) return 2;
    std::vector<double> w(n);
    for (double& x : w) {
      long long v;
      if (!(ls >> v)) return 2;
      x = (double)v;
    }
    for (int r = 0; r < world; r++) {
      int lo, hi;
      if (!(ls >> lo >> hi)) return 2;
      const std::pair<int, int> got = partition_range(w, world, r);
      if (got.first != lo || got.second != hi) finding("partition_range differs from shard.partition", cases, r, got.first);
    }
    cases++;
  }
  printf("partition: %d cases\n", cases);
  return cases ? 0 : 2;
}

// ---- 4) the frame generations, expectations written from the rule (update_frame_spec,
// recode.cpp:824-843: a slice of another picture, or of another size, takes the other frame and
// opens a generation there; both frames start anew with a file)
avr_slice_desc pic(int id, int w, int h, int structure = AVR_STRUCT_FRAME) {
  avr_slice_desc d;
  memset(&d, 0, sizeof(d));
  d.mb_width = w, d.mb_height = h, d.picture_id = id, d.structure = structure, d.coded = 1;
  return d;
}
void check_rmode() {
  const int64_t S = 20 * 15 * 52;   // one generation of a 20 x 15 picture
  std::vector<int64_t> goff;
  int64_t fbytes = 0;
  {   // picture ids 0, 1, 2, ...: a generation each, the other frame's is the previous one
    Plan p;
    for (int k = 0; k < 6; k++) p.descs.push_back(pic(k, 20, 15));
    if (!rmode_generations(p, &goff, &fbytes)) finding("pictures in turn: fallback");
    for (int k = 0; k < 6; k++)
      if (goff[2 * k] != k * S || goff[2 * k + 1] != (k ? (k - 1) * S : -1)) finding("pictures in turn", k, (long)goff[2 * k], (long)goff[2 * k + 1]);
    if (fbytes != 6 * S) finding("pictures in turn: frame bytes", (long)fbytes);
  }
  {   // two slices of one picture share a generation
    Plan p;
    for (int k = 0; k < 6; k++) p.descs.push_back(pic(k / 2, 20, 15));
    if (!rmode_generations(p, &goff, &fbytes)) finding("two slices a picture: fallback");
    for (int k = 0; k < 6; k++)
      if (goff[2 * k] != (k / 2) * S || goff[2 * k + 1] != (k / 2 ? (k / 2 - 1) * S : -1)) finding("two slices a picture", k, (long)goff[2 * k]);
    if (fbytes != 3 * S) finding("two slices a picture: frame bytes", (long)fbytes);
  }
  {   // a new file resets both frames: no other frame, and a generation even for the same picture id
    Plan p;
    for (int id : {0, 1, 1, 2}) p.descs.push_back(pic(id, 20, 15));
    p.file_first = {0, 2, 4};
    if (!rmode_generations(p, &goff, &fbytes)) finding("two files: fallback");
    const int64_t want[8] = {0, -1, S, 0, 2 * S, -1, 3 * S, 2 * S};
    for (int q = 0; q < 8; q++)
      if (goff[q] != want[q]) finding("two files", q, (long)goff[q], (long)want[q]);
  }
  {   // a size change.  The issue's case -- the other frame still holding a generation of the old
      // size, hence the fallback verdict -- is a state the rule cannot reach: update_frame_spec
      // re-initialises the other frame together with the current one (recode.cpp:829-835), so both
      // always have one size.  What the rule gives: the pass goes on, the other frame's generation
      // is dropped, and the next picture sees the new size's generation.
    Plan p;
    p.descs = {pic(0, 20, 15), pic(1, 20, 15), pic(2, 22, 18), pic(3, 22, 18)};
    const int64_t T = 22 * 18 * 52;
    if (!rmode_generations(p, &goff, &fbytes)) finding("size change: fallback");
    const int64_t want[8] = {0, -1, S, 0, 2 * S, -1, 2 * S + T, 2 * S};
    for (int q = 0; q < 8; q++)
      if (goff[q] != want[q]) finding("size change", q, (long)goff[q], (long)want[q]);
    if (fbytes != 2 * S + 2 * T) finding("size change: frame bytes", (long)fbytes);
  }
  {   // more than 4 GiB of frame metadata: the sequential kernel's
    Plan p;
    p.descs = {pic(0, 8192, 8192), pic(1, 8192, 8192)};
    if (rmode_generations(p, &goff, &fbytes)) finding("more than 4 GiB of frame metadata: no fallback");
  }
  {   // fields: the first field of a frame has bit 0 of its offset set, the second has not
    Plan p;
    p.descs = {pic(0, 20, 16, AVR_STRUCT_TOP_FIELD), pic(0, 20, 16, AVR_STRUCT_TOP_FIELD), pic(0, 20, 16, AVR_STRUCT_BOTTOM_FIELD),
               pic(1, 20, 16, AVR_STRUCT_BOTTOM_FIELD), pic(1, 20, 16, AVR_STRUCT_TOP_FIELD)};
    const int64_t F = 20 * 16 * 52;
    if (!rmode_generations(p, &goff, &fbytes)) finding("fields: fallback");
    const int64_t want[5] = {0 | 1, 0 | 1, 0, F | 1, F};
    for (int k = 0; k < 5; k++)
      if (goff[2 * k] != want[k]) finding("fields", k, (long)goff[2 * k], (long)want[k]);
  }
  printf("rmode: 6 sequences\n");
}

// ---- 5) the last-byte rule (recode.cpp:1345-1356): only a block with a parity, a last_byte field
// and a byte in it patches; a length of the other parity gets the byte appended, one of the
// block's parity has its last byte replaced -- when it has one.
void check_lastbyte() {
  int cases = 0;
  for (int has_parity = 0; has_parity < 2; has_parity++)
    for (int has_last = 0; has_last < 2; has_last++)
      for (int filled = 0; filled < 2; filled++)
        for (int equal = 0; equal < 2; equal++)
          for (size_t len = 0; len < 2; len++, cases++) {
            avr::PbBlock b;
            b.has_parity = has_parity, b.has_last_byte = has_last;
            if (filled) b.last_byte = "\x5a";
            b.length_parity = ((len & 1) != 0) == (equal != 0);
            LastByte want = LastByte::kKeep;
            if (has_parity && has_last && filled) want = !equal ? LastByte::kAppend : len ? LastByte::kReplace : LastByte::kKeep;
            if (last_byte_rule(b, len) != want) finding("last_byte_rule", has_parity * 4 + has_last * 2 + filled, equal, (long)len);
            std::vector<uint8_t> v(len, 0x11), w = v;
            patch_last_byte(b, len, &v);
            if (want == LastByte::kAppend) w.push_back(0x5a);
            if (want == LastByte::kReplace) w.back() = 0x5a;
            if (v != w) finding("patch_last_byte", has_parity * 4 + has_last * 2 + filled, equal, (long)len);
          }
  printf("lastbyte: %d cases\n", cases);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  int r = 0;
  if (cmd == "chain" && argc == 2) check_chain();
  else if (cmd == "cut" && argc == 4) r = check_cut(argv[2], argv[3]);
  else if (cmd == "partition" && argc == 3) r = check_partition(argv[2]);
  else if (cmd == "rmode" && argc == 2) check_rmode();
  else if (cmd == "lastbyte" && argc == 2) check_lastbyte();
  else return 2;
  if (r) return r;
  if (findings) return 1;
  printf("no finding\n");
  return 0;
}
