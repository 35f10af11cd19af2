// Section profiling of the slice kernels: cycle and bin counters per walker section (avr_prof) and
// the wave placement of each slice (avr_place), compiled in with -DAVR_PROFILE only -- every macro
// here is empty otherwise -- and the host helpers that read them back.  First header of the device
// chain (avr_slice_lds.h -> avr_walker.h -> avr_coder.h -> avr_slice_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define AVR_FI __device__ __forceinline__

// Cycle accounting per walker section, compiled in with -DAVR_PROFILE only (scripts/prof_sections):
// 0 slice, 1 macroblock syntax, 2 residual, 3 map decode, 4 nnz bins, 5 map re-code, 6 levels,
// 7 per-macroblock bookkeeping; [8 + i] bins coded in section i.  Summed over slices into avr_prof (one copy per TU).
#ifdef AVR_PROFILE
#define PROF_T() ((uint64_t)__builtin_readcyclecounter())
#define PROF_BEGIN(v) const uint64_t v = PROF_T(); const uint32_t v##_b = bins
#define PROF_BEGINW(v) const uint64_t v = PROF_T(); const uint32_t v##_b = w.bins
#define PROF_END(i, v) prof[i] += PROF_T() - (v), profb[i] += bins - v##_b
#define PROF_ENDW(i, v) w.prof[i] += PROF_T() - (v), w.profb[i] += w.bins - v##_b
// macroblock-layer sub-sections (avr_prof[32 + i] cycles, [40 + i] bins): 0 macroblock start,
// 1 mb_skip_flag, 2 mb_type + sub_mb_type, 3 intra prediction modes, 4 ref_idx, 5 mvd,
// 6 coded_block_pattern + transform_size_8x8_flag + mb_qp_delta, 7 end_of_slice + publish
#define SPROF_END(i, v) sprof[i] += PROF_T() - (v), sprofb[i] += bins - v##_b
#define SPROF_ENDW(i, v) w.sprof[i] += PROF_T() - (v), w.sprofb[i] += w.bins - v##_b
#else
#define SPROF_END(i, v)
#define SPROF_ENDW(i, v)
#define PROF_BEGINW(v)
#define PROF_ENDW(i, v)
#define PROF_BEGIN(v)
#define PROF_END(i, v)
#endif

namespace avr {

#ifdef AVR_PROFILE
static __device__ unsigned long long avr_prof[64];
#endif
#ifdef AVR_PROFILE
// wave placement per slice (AVR_PROFILE builds): HW_ID of waves 0..2, XCC_ID, walker start / end
// (s_memtime low 32 bits), walker start / end (s_memrealtime, 100 MHz) -- scripts/placement.py
constexpr int kPlaceSlices = 4096;
static __device__ uint32_t avr_place[kPlaceSlices][8];
AVR_FI void record_placement(int s, int wave) {
  if (s < kPlaceSlices && __lane_id() == 0) {
    avr_place[s][wave] = __builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_REG_HW_ID
    if (wave == 0) avr_place[s][3] = __builtin_amdgcn_s_getreg(20 | (15 << 11));  // HW_REG_XCC_ID
  }
}
#define AVR_PLACE(s, wave) record_placement(s, wave)
#define AVR_PLACE_T(s, k) if ((s) < kPlaceSlices && __lane_id() == 0) { \
    avr_place[s][4 + (k)] = (uint32_t)__builtin_readcyclecounter(); \
    avr_place[s][6 + (k)] = (uint32_t)__builtin_amdgcn_s_memrealtime(); }
#else
#define AVR_PLACE(s, wave)
#define AVR_PLACE_T(s, k)
#endif

// Host side of the avr_k_*.hip entry points (avr_kernels.h profile_* / placement_*): read (and
// clear) the section counters / read the placement records of an AVR_PROFILE build; zeros
// otherwise.  The caller names its own translation unit's copy (AVR_PROF_SYM / AVR_PLACE_SYM), so
// only a unit that exports such an entry point references the symbols from host code.
#ifdef AVR_PROFILE
#define AVR_PROF_SYM (&avr::avr_prof)
#define AVR_PLACE_SYM (&avr::avr_place)
#else
#define AVR_PROF_SYM nullptr
#define AVR_PLACE_SYM nullptr
#endif
static inline hipError_t read_clear_prof(const void* prof_sym, unsigned long long* out64) {
  if (!prof_sym) {
    for (int i = 0; i < 64; i++) out64[i] = 0;
    return hipSuccess;
  }
  hipError_t e = hipMemcpyFromSymbol(out64, prof_sym, sizeof(unsigned long long) * 64);
  unsigned long long z[64] = {};
  if (e == hipSuccess) e = hipMemcpyToSymbol(prof_sym, z, sizeof(z));
  return e;
}
static inline hipError_t read_placement(const void* place_sym, uint32_t* out, int n) {
  if (n > 4096) n = 4096;
  if (!place_sym) {
    for (int i = 0; i < 8 * n; i++) out[i] = 0;
    return hipSuccess;
  }
  return hipMemcpyFromSymbol(out, place_sym, sizeof(uint32_t) * 8 * n);
}

}  // namespace avr
