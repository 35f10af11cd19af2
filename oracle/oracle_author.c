/*
 * Oracle: the author.  TEST INFRASTRUCTURE ONLY (see avr_oracle.h).
 *
 * Writes H.264 streams whose CABAC statistics the tests choose.  The x264 fixtures and the device
 * generator stay in the middle of the syntax (cabac_init_idc 0, short exp-Golomb suffixes, short
 * mb_qp_delta, few references); the author goes to its edges.  It owns no syntax knowledge of
 * slice_data(): avr_walk_slice (oracle_walker.c) walks, and the hooks here ANSWER each bin the walker
 * asks for -- from a seeded xorshift and a per-profile policy keyed on (avr_walk_se, avr_walk_se_bin)
 * -- and code it with the CABAC re-encoder (cabac_enc_put*).  What the walker then does with the bin is
 * by construction what a decoder of the written bytes does, so every slice parses back.
 *
 * Own code: parameter sets and slice headers follow ITU-T H.264 7.3.2.1.1 (SPS), 7.3.2.2 (PPS), 7.3.3
 * (slice header), 7.3.2.8 / 7.4.1 (NAL unit, emulation prevention); each slice header is parsed back
 * with avr_parse_slice_header and must put slice_data() where the author did.
 *
 * The unary parts whose length matters (the prefix of a level / mvd escape's exp-Golomb suffix,
 * mb_qp_delta, ref_idx) are drawn as a length at their first bin, so a profile states a distribution
 * of lengths, and the forced profile an exact one for the n-th such element of a slice.  A forced
 * length past the walker's accept bound makes the walk fail there: the author finishes the arithmetic
 * code, pads the slice with random bytes and records it as refused.
 */
#include <stdlib.h>
#include <string.h>

#include "avr_oracle.h"

/* ------------------------------------------------------------------------------ bit writer */
typedef struct {
  obuf_t b;
  uint8_t cur;
  int k;
} bw_t;
static void bw_bit(bw_t *w, int v) {
  w->cur = (uint8_t)(w->cur << 1 | (v & 1));
  if (++w->k == 8) {
    ob_put(&w->b, w->cur);
    w->cur = 0;
    w->k = 0;
  }
}
static void bw_u(bw_t *w, uint32_t v, int n) {
  while (n--) bw_bit(w, (int)(v >> n));
}
static void bw_ue(bw_t *w, uint32_t v) {   /* 9.1 */
  v++;
  int n = 0;
  while (v >> (n + 1)) n++;
  bw_u(w, 0, n);
  bw_u(w, v, n + 1);
}
static void bw_se(bw_t *w, int v) { bw_ue(w, v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }
static void bw_trailing(bw_t *w) {   /* rbsp_trailing_bits() */
  bw_bit(w, 1);
  while (w->k) bw_bit(w, 0);
}

/* nal_unit() in byte stream format (Annex B), emulation_prevention_three_byte per 7.4.1; returns the
 * number of those bytes */
static uint32_t put_nal(obuf_t *f, int ref_idc, int type, const uint8_t *p, size_t n) {
  static const uint8_t start[4] = {0, 0, 0, 1};
  uint32_t epb = 0;
  ob_append(f, start, 4);
  ob_put(f, (uint8_t)(ref_idc << 5 | type));
  int z = 0;
  for (size_t i = 0; i < n; i++) {
    if (z >= 2 && p[i] <= 3) {
      ob_put(f, 3);
      epb++;
      z = 0;
    }
    ob_put(f, p[i]);
    z = p[i] == 0 ? z + 1 : 0;
  }
  return epb;
}

/* ------------------------------------------------------------------------------ the policy */
typedef struct {
  const avr_author_params_t *p;
  avr_author_census_t *c;
  uint64_t rng;
  cabac_enc_t enc;
  int slice, target_mbs;
  int len[4];              /* the length drawn for the unary part in progress, by AVR_FORCE_* element */
  int seen[4];             /* such elements so far in this slice */
  int forced_done[AVR_AUTHOR_MAX_FORCED];
  uint32_t bins;
} author_t;

static uint32_t rnd16(author_t *a) {   /* xorshift64 */
  a->rng ^= a->rng << 13;
  a->rng ^= a->rng >> 7;
  a->rng ^= a->rng << 17;
  return (uint32_t)(a->rng >> 16) & 0xffff;
}
static int uniform(author_t *a, int hi) { return hi > 0 ? (int)(rnd16(a) % (uint32_t)(hi + 1)) : 0; }
static int geometric(author_t *a, int hi) {   /* P(n) = 2^-(n+1), cut at hi */
  int n = 0;
  while (n < hi && (rnd16(a) & 1)) n++;
  return n;
}
static int imin(int x, int y) { return x < y ? x : y; }

/* the length of the unary part that starts now */
static int draw_length(author_t *a, int element, int limit) {
  const avr_author_params_t *p = a->p;
  const int n = a->seen[element]++;
  for (int i = 0; i < p->n_forced; i++) {
    const avr_author_force_t *f = &p->forced[i];
    if (f->slice != a->slice || f->element != element || a->forced_done[i] || n < f->nth) continue;
    /* ref_idx: only where the syntax has room for it (an MBAFF field macroblock doubles the limit) */
    if (element == AVR_FORCE_REF && limit < imin(f->length, 32)) continue;
    a->forced_done[i] = 1;
    return f->length;
  }
  const int wide = p->profile == AVR_AUTHOR_FORCED;
  switch (element) {
    case AVR_FORCE_LEVEL:
      return p->profile == AVR_AUTHOR_LEVELS || wide ? uniform(a, p->kmax_level) : geometric(a, p->kmax_level);
    case AVR_FORCE_MVD:
      return p->profile == AVR_AUTHOR_MOTION || wide ? uniform(a, p->kmax_mvd) : geometric(a, p->kmax_mvd);
    case AVR_FORCE_QPDELTA:   /* the legal range is -26..25: up to 52 bins of 1 */
      if (p->profile == AVR_AUTHOR_SPARSE) return uniform(a, 1);
      if (p->profile == AVR_AUTHOR_MOTION && (rnd16(a) & 7) == 0) return 52 - geometric(a, 52);   /* at the legal end */
      return geometric(a, 52);
    default:
      limit = imin(limit, 31);
      return p->profile == AVR_AUTHOR_MOTION || wide ? uniform(a, limit) : geometric(a, limit);
  }
}

/* P(bin = 1) in 1/65536 of a context-coded bin that is not part of a drawn length */
static int p_one(const author_t *a) {
  const int se = avr_walk_se;
  switch (a->p->profile) {
    case AVR_AUTHOR_LEVELS:
      if (se == SE_CBF) return 60000;
      if (se == SE_SIG) return 40000;
      if (se == SE_LAST) return 6000;
      if (se == SE_LEVEL_PREFIX) return 62000;
      if (se == SE_CBP) return 55000;
      if (se == SE_SKIP) return 3000;
      break;
    case AVR_AUTHOR_MOTION:
      if (se == SE_SKIP) return 5000;
      if (se == SE_MVD_PREFIX) return 60000;
      if (se == SE_CBF) return 8000;
      if (se == SE_CBP) return 20000;
      break;
    case AVR_AUTHOR_SPARSE:
      if (se == SE_SKIP) return 64000;
      if (se == SE_CBP) return 1500;
      if (se == SE_CBF) return 3000;
      break;
    case AVR_AUTHOR_FORCED:   /* levels and motion at once, so that every forced element occurs early */
      if (se == SE_SKIP) return 3000;
      if (se == SE_CBF) return 45000;
      if (se == SE_SIG) return 30000;
      if (se == SE_LAST) return 9000;
      if (se == SE_LEVEL_PREFIX) return 61000;
      if (se == SE_MVD_PREFIX) return 60000;
      if (se == SE_CBP) return 45000;
      break;
    default: break;
  }
  return 32768;
}

static int a_get(void *o, uint8_t *state, int ctx) {
  author_t *a = (author_t *)o;
  avr_author_census_t *c = a->c;
  const int se = avr_walk_se, k = avr_walk_se_bin;
  int b;
  if (se == SE_QPDELTA || se == SE_REF) {
    const int e = se == SE_QPDELTA ? AVR_FORCE_QPDELTA : AVR_FORCE_REF;
    if (k == 0) a->len[e] = draw_length(a, e, avr_walk_se_limit);
    b = k < a->len[e];
    if (se == SE_QPDELTA) {
      if (!b) c->qp_delta_len[k]++;
      else if (k == 102) c->qp_delta_len[103]++;   /* the walk ends here */
    } else {
      if (!b) c->ref_idx[k]++;
      else if (k == 31) c->ref_idx[32]++;
    }
  } else {
    b = (int)rnd16(a) < p_one(a);
    if (se == SE_SKIP) c->skipped_mbs += (uint32_t)b;
  }
  cabac_enc_put(&a->enc, b, state);
  a->bins++;
  return b;
}

static int a_get_bypass(void *o) {
  author_t *a = (author_t *)o;
  avr_author_census_t *c = a->c;
  const int se = avr_walk_se, k = avr_walk_se_bin;
  int b;
  if (se == SE_LEVEL_SUFFIX && k < 100) {
    if (k == 0) { a->len[AVR_FORCE_LEVEL] = draw_length(a, AVR_FORCE_LEVEL, 0); c->level_escapes++; }
    b = k < a->len[AVR_FORCE_LEVEL];
    if (!b) c->level_len[k]++;
    else if (k == 30) c->level_len[31]++;
  } else if (se == SE_MVD_SUFFIX && k < 100) {   /* bin k of the prefix: the order is 3 + k */
    if (k == 0) { a->len[AVR_FORCE_MVD] = draw_length(a, AVR_FORCE_MVD, 0); c->mvd_escapes++; }
    b = k < a->len[AVR_FORCE_MVD];
    if (!b) c->mvd_k[3 + k]++;
    else if (k == 21) c->mvd_k[25]++;
  } else {
    b = (int)(rnd16(a) & 1);
  }
  cabac_enc_put_bypass(&a->enc, b);
  a->bins++;
  return b;
}

static int a_get_terminate(void *o) {
  author_t *a = (author_t *)o;
  int b = 0;   /* pcm_flag: never */
  if (avr_walk_se == SE_EOS) b = avr_walk_mbs_done >= a->target_mbs || avr_walk_last_mb;
  cabac_enc_put_terminate(&a->enc, b);
  a->bins++;
  return b;
}
static void a_frame_spec(void *o, int f, int w, int h) {}
static void a_mb_xy(void *o, int x, int y) {}
static void a_sub_mb(void *o, int cat, int n, int max, int dc, int c422) {}
static void a_begin_ct(void *o, avr_coding_type t, int z, int p0, int p1) {}
static void a_end_ct(void *o, avr_coding_type t) {}

/* ------------------------------------------------------------------------------ the stream */
#define FRAME_NUM_BITS 4

static void write_sps(bw_t *s, const avr_author_params_t *p) {   /* 7.3.2.1.1 */
  const int cf = p->chroma_format_idc, frame_only = p->structure == 0;
  bw_u(s, cf == 3 ? 244 : cf == 2 ? 122 : 100, 8);   /* profile_idc: High, High 4:2:2, High 4:4:4 Predictive */
  bw_u(s, 0, 8);                                      /* constraint_set flags, reserved_zero_2bits */
  bw_u(s, 51, 8);                                     /* level_idc */
  bw_ue(s, 0);                                        /* seq_parameter_set_id */
  bw_ue(s, (uint32_t)cf);
  if (cf == 3) bw_u(s, 0, 1);                         /* separate_colour_plane_flag */
  bw_ue(s, 0);                                        /* bit_depth_luma_minus8 */
  bw_ue(s, 0);                                        /* bit_depth_chroma_minus8 */
  bw_u(s, 0, 1);                                      /* qpprime_y_zero_transform_bypass_flag */
  bw_u(s, 0, 1);                                      /* seq_scaling_matrix_present_flag */
  bw_ue(s, FRAME_NUM_BITS - 4);                                  /* log2_max_frame_num_minus4 */
  bw_ue(s, 2);                                        /* pic_order_cnt_type: nothing in the slice header */
  bw_ue(s, 16);                                       /* max_num_ref_frames */
  bw_u(s, 0, 1);                                      /* gaps_in_frame_num_value_allowed_flag */
  bw_ue(s, (uint32_t)p->mb_width - 1);
  bw_ue(s, (uint32_t)(frame_only ? p->mb_height : p->mb_height / 2) - 1);   /* pic_height_in_map_units_minus1 */
  bw_u(s, (uint32_t)frame_only, 1);                   /* frame_mbs_only_flag */
  if (!frame_only) bw_u(s, p->structure == 2, 1);     /* mb_adaptive_frame_field_flag */
  bw_u(s, 1, 1);                                      /* direct_8x8_inference_flag */
  bw_u(s, 0, 1);                                      /* frame_cropping_flag */
  bw_u(s, 0, 1);                                      /* vui_parameters_present_flag */
  bw_trailing(s);
}

static void write_pps(bw_t *q, const avr_author_params_t *p) {   /* 7.3.2.2 */
  bw_ue(q, 0);                                        /* pic_parameter_set_id */
  bw_ue(q, 0);                                        /* seq_parameter_set_id */
  bw_u(q, 1, 1);                                      /* entropy_coding_mode_flag */
  bw_u(q, 0, 1);                                      /* bottom_field_pic_order_in_frame_present_flag */
  bw_ue(q, 0);                                        /* num_slice_groups_minus1 */
  bw_ue(q, (uint32_t)p->num_ref_idx - 1);             /* num_ref_idx_l0_default_active_minus1 */
  bw_ue(q, (uint32_t)p->num_ref_idx - 1);
  bw_u(q, 0, 1);                                      /* weighted_pred_flag */
  bw_u(q, 0, 2);                                      /* weighted_bipred_idc */
  bw_se(q, 0);                                        /* pic_init_qp_minus26 */
  bw_se(q, 0);                                        /* pic_init_qs_minus26 */
  bw_se(q, 0);                                        /* chroma_qp_index_offset */
  bw_u(q, 1, 1);                                      /* deblocking_filter_control_present_flag */
  bw_u(q, 0, 1);                                      /* constrained_intra_pred_flag */
  bw_u(q, 0, 1);                                      /* redundant_pic_cnt_present_flag */
  bw_u(q, (uint32_t)(p->transform_8x8_mode != 0), 1);
  bw_u(q, 0, 1);                                      /* pic_scaling_matrix_present_flag */
  bw_se(q, 0);                                        /* second_chroma_qp_index_offset */
  bw_trailing(q);
}

/* 7.3.3 up to slice_data(); first: first_mb_in_slice (macroblock pairs in an MBAFF frame) */
static void write_slice_header(bw_t *h, const avr_author_params_t *p, int first, int st, int idr, int frame_num,
                               int idr_pic_id, int field, int bottom, int idc, int qp) {
  bw_ue(h, (uint32_t)first);
  bw_ue(h, (uint32_t)st + 5);                         /* slice_type: all slices of the picture alike */
  bw_ue(h, 0);                                        /* pic_parameter_set_id */
  bw_u(h, (uint32_t)frame_num, FRAME_NUM_BITS);
  if (p->structure != 0) {
    bw_u(h, (uint32_t)field, 1);                      /* field_pic_flag */
    if (field) bw_u(h, (uint32_t)bottom, 1);
  }
  if (idr) bw_ue(h, (uint32_t)idr_pic_id);
  if (st == AVR_SLICE_B) bw_u(h, 1, 1);               /* direct_spatial_mv_pred_flag */
  if (st != AVR_SLICE_I) {
    bw_u(h, 1, 1);                                    /* num_ref_idx_active_override_flag */
    bw_ue(h, (uint32_t)p->num_ref_idx - 1);
    if (st == AVR_SLICE_B) bw_ue(h, (uint32_t)p->num_ref_idx - 1);
    bw_u(h, 0, 1);                                    /* ref_pic_list_modification_flag_l0 */
    if (st == AVR_SLICE_B) bw_u(h, 0, 1);
  }
  if (idr) {                                          /* dec_ref_pic_marking(): nal_ref_idc != 0 */
    bw_u(h, 0, 1);                                    /* no_output_of_prior_pics_flag */
    bw_u(h, 0, 1);                                    /* long_term_reference_flag */
  } else {
    bw_u(h, 0, 1);                                    /* adaptive_ref_pic_marking_mode_flag */
  }
  if (st != AVR_SLICE_I) bw_ue(h, (uint32_t)idc);     /* cabac_init_idc */
  bw_se(h, qp - 26);                                  /* slice_qp_delta */
  bw_ue(h, 1);                                        /* disable_deblocking_filter_idc */
  while (h->k) bw_bit(h, 1);                          /* cabac_alignment_one_bit */
}

int avr_author_stream(const avr_author_params_t *p, uint8_t **out, size_t *len, avr_author_census_t *census) {
  const int fields = p->structure == 1 || p->structure == 3;
  if (p->mb_width < 1 || p->mb_height < 1 || p->structure < 0 || p->structure > 3 ||
      (p->structure != 0 && (p->mb_height & 1)) || p->chroma_format_idc < 1 || p->chroma_format_idc > 3 ||
      p->num_ref_idx < 1 || p->num_ref_idx > 32 || p->pictures < 1 || p->slices_per_picture < 1 ||
      p->n_qp < 1 || p->n_qp > 8 || p->n_idc < 1 || p->n_idc > 4 || p->kmax_level < 0 || p->kmax_level > 30 ||
      p->kmax_mvd < 0 || p->kmax_mvd > 21 || p->n_forced < 0 || p->n_forced > AVR_AUTHOR_MAX_FORCED ||
      p->profile < AVR_AUTHOR_LEVELS || p->profile > AVR_AUTHOR_FORCED)
    return -1;
  for (int i = 0; i < p->n_qp; i++)
    if (p->qp[i] < 0 || p->qp[i] > 51) return -1;
  for (int i = 0; i < p->n_idc; i++)
    if (p->idc[i] < 0 || p->idc[i] > 2) return -1;
  avr_author_census_t *c = census ? census : (avr_author_census_t *)malloc(sizeof(*c));
  memset(c, 0, sizeof(*c));
  author_t *a = (author_t *)calloc(1, sizeof(*a));
  a->p = p;
  a->c = c;
  a->rng = 88172645463325252ull ^ (p->seed + 1) * 0x9E3779B97F4A7C15ull;
  avr_param_sets_t *ps = (avr_param_sets_t *)calloc(1, sizeof(*ps));
  obuf_t f;
  ob_init(&f);
  bw_t s, q;
  memset(&s, 0, sizeof(s));
  memset(&q, 0, sizeof(q));
  ob_init(&s.b);
  ob_init(&q.b);
  write_sps(&s, p);
  write_pps(&q, p);
  c->emulation_bytes += put_nal(&f, 3, 7, s.b.data, s.b.len);
  c->emulation_bytes += put_nal(&f, 3, 8, q.b.data, q.b.len);
  int ret = avr_parse_sps(ps, s.b.data, s.b.len) == 0 && avr_parse_pps(ps, q.b.data, q.b.len) == 0 ? 0 : -2;
  ob_free(&s.b);
  ob_free(&q.b);
  avr_hooks_t hk = {a, a_get, a_get_bypass, a_get_terminate, a_frame_spec, a_mb_xy, a_sub_mb, a_sub_mb,
                    a_begin_ct, a_end_ct, NULL};
  /* units a slice is measured in: macroblocks of the frame or field, macroblock pairs of an MBAFF frame */
  const int units = p->structure == 0 ? p->mb_width * p->mb_height : p->mb_width * p->mb_height / 2;
  const int per = (units + p->slices_per_picture - 1) / p->slices_per_picture;
  int n = 0, n_of_type[3] = {0, 0, 0};
  for (int pic = 0; pic < p->pictures && ret == 0; pic++) {
    const int st = p->with_i ? (pic % 3 == 0 ? AVR_SLICE_I : pic % 3 == 1 ? AVR_SLICE_P : AVR_SLICE_B)
                             : (pic == 0 ? AVR_SLICE_I : (pic & 1) ? AVR_SLICE_P : AVR_SLICE_B);
    for (int fld = 0; fld < (fields ? 2 : 1) && ret == 0; fld++) {
      const int bottom = fields ? (p->structure == 3) ^ fld : 0;
      /* an IDR picture's second field is a non-IDR picture of the same frame_num (7.4.1.2.4) */
      const int idr = st == AVR_SLICE_I && fld == 0;
      for (int first = 0; first < units && ret == 0; first += per, n++) {
        if (n >= AVR_AUTHOR_MAX_SLICES) { ret = -1; break; }
        const int idc = st == AVR_SLICE_I ? 0 : p->idc[n_of_type[st] % p->n_idc], qp = p->qp[n % p->n_qp];
        n_of_type[st]++;
        bw_t h;
        memset(&h, 0, sizeof(h));
        ob_init(&h.b);
        write_slice_header(&h, p, first, st, idr, st == AVR_SLICE_I ? 0 : pic & ((1 << FRAME_NUM_BITS) - 1),
                           pic & 0xffff, fields, bottom, idc, qp);
        const size_t hn = h.b.len;
        /* the header parses back, and slice_data() begins where this wrote it */
        avr_slice_hdr_t sh;
        uint8_t *tmp = (uint8_t *)malloc(hn + 8);
        memcpy(tmp, h.b.data, hn);
        memset(tmp + hn, 0x80, 8);
        const int nal_type = idr ? 5 : 1;
        if (avr_parse_slice_header(ps, tmp, hn + 8, nal_type, 2, &sh) != 0 || sh.cabac_start != hn || !sh.supported ||
            sh.slice_type != st || sh.slice_qp != qp || sh.cabac_init_idc != (st == AVR_SLICE_I ? -1 : idc) ||
            sh.field_pic != fields || sh.bottom_field != bottom || sh.mbaff != (p->structure == 2))
          ret = -3;
        free(tmp);
        if (ret) { ob_free(&h.b); break; }
        sh.x264_build = -1;
        cabac_enc_init(&a->enc, &h.b);   /* slice_data() follows the header in the same buffer */
        a->slice = n;
        a->target_mbs = p->structure == 2 ? 2 * per : per;
        a->bins = 0;
        memset(a->seen, 0, sizeof(a->seen));
        const int r = avr_walk_slice(&sh, &hk, pic);
        avr_author_slice_t *rec = &c->slice[n];
        if (r != 0) {
          /* only a forced length may stop the walk: finish the code, pad with random bytes, and end on
           * a byte that holds a stop bit */
          int forced_here = 0;
          for (int i = 0; i < p->n_forced; i++) forced_here |= p->forced[i].slice == n && a->forced_done[i];
          if (!forced_here) ret = -4;
          ac_enc_finish(&a->enc.e);
          for (int i = 0; i < 24; i++) ob_put(&h.b, (uint8_t)rnd16(a));
          ob_put(&h.b, 0x80);
          rec->refused = 1;
          c->refused_slices++;
        }
        cabac_enc_free(&a->enc);
        c->mbs += (uint32_t)avr_walk_mbs_done;
        rec->slice_type = st;
        rec->slice_qp = qp;
        rec->cabac_init_idc = sh.cabac_init_idc;
        rec->first_mb = sh.first_mb;
        rec->structure = p->structure == 2 ? 3 : fields ? 1 + bottom : 0;
        rec->payload_bytes = (uint32_t)(h.b.len - hn);
        rec->bins = a->bins;
        c->payload_bytes += rec->payload_bytes;
        c->bins += a->bins;
        c->qp_used[qp]++;
        if (st != AVR_SLICE_I) c->idc_used[st == AVR_SLICE_B][idc]++;
        c->emulation_bytes += put_nal(&f, 2, nal_type, h.b.data, h.b.len);
        ob_free(&h.b);
      }
    }
  }
  c->slices = (uint32_t)n;
  free(ps);
  free(a);
  if (!census) free(c);
  if (ret) {
    ob_free(&f);
    return ret;
  }
  *out = f.data;
  *len = f.len;
  return 0;
}
