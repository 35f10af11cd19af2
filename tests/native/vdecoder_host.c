/* Host restatement of the decompress walker's VGPR-resident recoded decoder (avr_engine.h,
 * VDecoder), put in the place of the oracle's ac_dec_get for arithmetic_code<uint64_t, uint8_t>:
 * the interval as range and d = low - range, the decision as the sign of d + r1, one or two
 * digits of renormalisation chosen by the high word of range.  Built with the oracle's other
 * sources into one library (tests/test_gpu_vdecoder.py), so the oracle's whole decompress path runs
 * on it, and counts per decision:
 *   vd_digits[k]   decisions that renormalised by k digits (k = 0, 1, 2)
 *   vd_mismatch    decisions whose bin or state differ from the oracle's own ac_dec_get
 */
#define ac_dec_get ac_dec_get_oracle
#include "../../oracle/oracle_arith.c"
#undef ac_dec_get

unsigned long long vd_digits[3];
unsigned long long vd_mismatch;

void vd_reset(void) {
  vd_digits[0] = vd_digits[1] = vd_digits[2] = 0;
  vd_mismatch = 0;
}

int ac_dec_get(ac_dec_t *dec, uint64_t r1) {
  if (dec->fixed_one != (1ull << 63) || dec->digit_base != 256) return ac_dec_get_oracle(dec, r1);
  ac_dec_t ref = *dec;
  const int ref_bin = ac_dec_get_oracle(&ref, r1);

  uint64_t d = dec->low - dec->range;            /* in [-2^63, -1] */
  uint64_t range = dec->range;
  const uint64_t sum = d + r1;                   /* low - r0 */
  const int c = (int32_t)(sum >> 32) >= 0;
  d = c ? d : sum;
  range = c ? r1 : range - r1;
  dec->range = range;
  dec->low = d + range;
  int k = 0;
  if ((uint32_t)(dec->range >> 32) < (1u << 19)) {
    renorm_consume(dec);                         /* d' = (d << 8) | digit */
    k = 1;
    if ((uint32_t)(dec->range >> 32) < (1u << 23)) {
      renorm_consume(dec);
      k = 2;
    }
  }
  vd_digits[k]++;
  if (c != ref_bin || dec->low != ref.low || dec->range != ref.range || dec->in != ref.in ||
      dec->next_digit != ref.next_digit)
    vd_mismatch++;
  return c;
}
