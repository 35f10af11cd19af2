// recode CLI (recode.cpp:1627-1659): recode [compress|decompress|roundtrip] [-p|-p32|-c] [-e] [-s] [-k] [-u] <input> [output]
//                                    recode read <in.avrc> <offset> <length> [output]
//   read  a byte range of the file a container restores (avr_reader_*): only the slices and pieces the
//         range touches are regenerated where the container allows it; the range is clamped to the file.
//         A unit whose bytes miss its checksum (-u) fails the read: the error names it, the exit status is 1.
//   -p    parallel model (fresh model per slice; slices independent) on the reference's
//         arithmetic_code<uint64_t, uint8_t>; default = reference model.
//   -p32  parallel model on the optional 32-bit P32 coder (avrecode-amd:P32 containers).
//   -c    the reference model in chains of 16 coded slices (avrecode-amd:R16 containers).
//   -e    with -p / -p32, compress and roundtrip: slices whose NAL unit carries emulation-prevention
//         bytes are re-coded too (avr_set_recode_escaped; avrecode-amd:P64E / P32E containers).
//   -s    with -p32, compress and roundtrip: long slices are split as -p splits them
//         (avr_set_split_p32; avrecode-amd:P32S / P32SE containers).
//   -k    compress and roundtrip, any model: a checked container -- the file's CRC-32 in its Metadata
//         (avr_set_checksums); decompress checks the field wherever it finds it.
//   -u    with -p / -p32, compress and roundtrip: unit checksums -- a CRC-32 per slice and per piece of a
//         cut slice in the container (avr_set_unit_checksums); decompress and read check them wherever
//         they find them.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/avrecode.h"

static bool read_file(const char* p, std::vector<uint8_t>* v) {
  std::ifstream f(p, std::ios::binary);
  if (!f) return false;
  v->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

// ~h264_model (recode.cpp:634-655): the bills to stderr, nonzero entries by CodingType name -- the
// compressor's (re-coded bytes) and the decompressor's (CABAC bytes), summed over the file.
static const char* const kBillingNames[6] = {"PIP_UNKNOWN", "PIP_UNREACHABLE", "PIP_SIGNIFICANCE_MAP",
                                             "PIP_SIGNIFICANCE_EOB", "PIP_SIGNIFICANCE_NZ", "PIP_RESIDUALS"};
static void print_bill(const char* title, const uint64_t* b) {
  bool first = true;
  for (int i = 0; i < 6; i++) {
    if (!b[i]) continue;
    if (first) std::cerr << title << "\n=============\n";
    first = false;
    std::cerr << kBillingNames[i] << " : " << b[i] << "\n";
  }
}

// a non-negative decimal number and nothing else
static bool parse_u64(const char* s, uint64_t* v) {
  if (!*s || *s < '0' || *s > '9') return false;
  char* end = nullptr;
  errno = 0;
  *v = strtoull(s, &end, 10);
  return errno == 0 && *end == 0;
}

// recode read <in.avrc> <offset> <length> [output]
static int read_range(int argc, char** argv) {
  uint64_t off = 0, len = 0;
  if (argc < 5 || argc > 6 || !parse_u64(argv[3], &off) || !parse_u64(argv[4], &len) || off + len < off) {
    std::cerr << "Usage: " << argv[0] << " read <in.avrc> <offset> <length> [output]" << std::endl;
    return 1;
  }
  std::vector<uint8_t> in;
  if (!read_file(argv[2], &in)) {
    std::cerr << "Failed to open file: " << argv[2] << std::endl;
    return 1;
  }
  avr_ctx* ctx = nullptr;
  if (avr_create(0, &ctx) != AVR_OK) {
    std::cerr << "No usable MI355X / HIP device" << std::endl;
    return 1;
  }
  avr_reader* rd = nullptr;
  avr_reader_info_t info;
  int r = avr_reader_open(ctx, in.data(), in.size(), &rd);
  if (r == AVR_OK) r = avr_reader_info(rd, &info);
  std::vector<uint8_t> out;
  size_t got = 0;
  if (r == AVR_OK) {
    const uint64_t o = off < info.file_size ? off : info.file_size;
    out.resize((size_t)(len < info.file_size - o ? len : info.file_size - o));
    r = avr_reader_read(rd, off, out.size(), out.data(), &got);
  }
  if (r != AVR_OK) {
    std::cerr << "Exception: " << avr_last_error(ctx) << " (" << r << ")" << std::endl;
    avr_reader_close(rd);
    avr_destroy(ctx);
    return 1;
  }
  if (argc == 6) {
    std::ofstream f(argv[5], std::ios::binary);
    f.write((const char*)out.data(), (std::streamsize)got);
  } else {
    fwrite(out.data(), 1, got, stdout);
  }
  avr_reader_close(rd);
  avr_destroy(ctx);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "Usage: " << argv[0] << " [compress|decompress|roundtrip] [-p|-p32|-c] [-e] [-s] [-k] [-u] <input> [output]\n"
              << "       " << argv[0] << " read <in.avrc> <offset> <length> [output]" << std::endl;
    return 1;
  }
  std::string cmd = argv[1];
  if (cmd == "read") return read_range(argc, argv);
  int a = 2, model = AVR_MODEL_REFERENCE;
  bool escaped = false, split32 = false, checks = false, units = false;
  for (; a < argc; a++) {   // the model, -e, -s, -k and -u, in any order
    if (!strcmp(argv[a], "-p")) model = AVR_MODEL_PARALLEL;
    else if (!strcmp(argv[a], "-p32")) model = AVR_MODEL_PARALLEL32;
    else if (!strcmp(argv[a], "-c")) model = AVR_MODEL_CHAINED;
    else if (!strcmp(argv[a], "-e")) escaped = true;
    else if (!strcmp(argv[a], "-s")) split32 = true;
    else if (!strcmp(argv[a], "-k")) checks = true;
    else if (!strcmp(argv[a], "-u")) units = true;
    else break;
  }
  if (escaped && ((model != AVR_MODEL_PARALLEL && model != AVR_MODEL_PARALLEL32) || cmd == "decompress")) {
    std::cerr << "-e goes with compress or roundtrip and -p or -p32" << std::endl;
    return 1;
  }
  if (split32 && (model != AVR_MODEL_PARALLEL32 || cmd == "decompress")) {
    std::cerr << "-s goes with compress or roundtrip and -p32" << std::endl;
    return 1;
  }
  if (units && ((model != AVR_MODEL_PARALLEL && model != AVR_MODEL_PARALLEL32) || cmd == "decompress")) {
    std::cerr << "-u goes with compress or roundtrip and -p or -p32" << std::endl;
    return 1;
  }
  if (a >= argc) return 1;
  const char* input = argv[a++];
  const char* output = a < argc ? argv[a] : nullptr;
  std::vector<uint8_t> in;
  if (!read_file(input, &in)) {
    std::cerr << "Failed to open file: " << input << std::endl;
    return 1;
  }
  avr_ctx* ctx = nullptr;
  if (avr_create(0, &ctx) != AVR_OK) {
    std::cerr << "No usable MI355X / HIP device" << std::endl;
    return 1;
  }
  if (escaped) avr_set_recode_escaped(ctx, 1);
  if (split32) avr_set_split_p32(ctx, 1);
  if (checks) avr_set_checksums(ctx, 1);
  if (units) avr_set_unit_checksums(ctx, 1);
  uint8_t* out = nullptr;
  size_t out_len = 0;
  int r;
  if (cmd == "compress") {
    r = avr_compress_file(ctx, in.data(), in.size(), model, &out, &out_len);
  } else if (cmd == "decompress") {
    r = avr_decompress_file(ctx, in.data(), in.size(), &out, &out_len);
  } else if (cmd == "roundtrip") {
    avr_file_stats st;
    r = avr_roundtrip_file(ctx, in.data(), in.size(), model, &out, &out_len, &st);
    if (r == AVR_OK) {
      std::cout << "Compress-decompress roundtrip succeeded:" << std::endl;
      std::cout << " compression ratio: " << out_len * 100.0 / in.size() << "%" << std::endl;
      std::cout << " slices " << st.slices << " coded " << st.coded_slices << " skipped " << st.skipped_slices
                << " payload " << st.payload_bytes << " recoded " << st.recoded_bytes << std::endl;
      std::cout << " compress " << st.compress_s << "s decompress " << st.decompress_s << "s" << std::endl;
      print_bill("Avrecode Bill", st.bill);
      print_bill("CABAC Bill", st.cabac_bill);
    } else {
      std::cerr << "Compress-decompress roundtrip failed: " << avr_last_error(ctx) << std::endl;
      avr_destroy(ctx);
      return 1;
    }
    if (!output) {
      avr_free(out);
      avr_destroy(ctx);
      return 0;
    }
  } else {
    std::cerr << "Unknown command: " << cmd << std::endl;
    return 1;
  }
  if (r != AVR_OK) {
    std::cerr << "Exception: " << avr_last_error(ctx) << " (" << r << ")" << std::endl;
    avr_destroy(ctx);
    return 1;
  }
  if (output) {
    std::ofstream f(output, std::ios::binary);
    f.write((const char*)out, (std::streamsize)out_len);
  } else {
    fwrite(out, 1, out_len, stdout);
  }
  avr_free(out);
  avr_destroy(ctx);
  return 0;
}
