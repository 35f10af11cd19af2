// The product's CABAC context initialisation tables (avrecode_amd/csrc/h264_tables.h: kInitI,
// kInitPB[0..2], kMap444 through avr::mn_for_ctx) against the oracle's (oracle_tables.c through
// avr_cabac_init_states): the state byte of every context 0..1023 for every cabac_init_idc in
// {-1 (I slices), 0, 1, 2} and every slice_qp 0..51.  The loop below is the one avr_seams.cpp
// cabac_init_states and the device's init_slice_state run (9.3.1.1: preCtxState = Clip3(1, 126,
// ((m * Clip3(0, 51, SliceQPY)) >> 4) + n), FFmpeg's state byte (pStateIdx << 1) | valMPS).
//
// Stand-alone, host only: g++, h264_tables.h and liboracle; no HIP, no device.  The two tables are
// separate transcriptions of ITU-T H.264 Tables 9-12..9-33; they pin each other, nothing else here does.
//
//   init_tables_check            compare everything; "no finding", exit 0
//   init_tables_check IDC CTX    the same with m of kInitPB[IDC][CTX] (or kInitI for IDC -1) off by
//                                one, to show that the comparison sees a single wrong pair: exit 1
#include <cstdio>
#include <cstdlib>

#include "avr_oracle.h"
#include "h264_tables.h"

int main(int argc, char** argv) {
  const int bad_idc = argc > 2 ? atoi(argv[1]) : -2, bad_ctx = argc > 2 ? atoi(argv[2]) : -1;
  long findings = 0, compared = 0;
  for (int idc = -1; idc <= 2; idc++) {
    for (int qp = 0; qp <= 51; qp++) {
      uint8_t want[1024];
      avr_cabac_init_states(want, idc, qp);
      for (int c = 0; c < 1024; c++) {
        int m, n;
        avr::mn_for_ctx(idc, c, &m, &n);
        // the pair a context of 460..1023 borrows is the damaged one too: find it as mn_for_ctx does
        int src = c;
        if (c >= 460)
          for (const auto& r : avr::kMap444)
            if (c >= r[0] && c < r[0] + r[2]) { src = r[1] + (c - r[0]); break; }
        if (idc == bad_idc && src == bad_ctx) m += 1;
        int pre = ((m * qp) >> 4) + n;
        pre = pre < 1 ? 1 : pre > 126 ? 126 : pre;
        const uint8_t got = pre <= 63 ? (uint8_t)((63 - pre) << 1) : (uint8_t)(((pre - 64) << 1) | 1);
        compared++;
        if (got != want[c]) {
          if (findings < 8) printf("idc %d qp %d ctx %d: product %d, oracle %d (m %d n %d)\n", idc, qp, c, got, want[c], m, n);
          findings++;
        }
      }
    }
  }
  printf("%ld states compared, %ld differ\n", compared, findings);
  if (findings) return 1;
  printf("no finding\n");
  return 0;
}
