// Device-side history (noahmp_hip_history_step / _finish): the per-element arithmetic of the interval accumulators.
// __host__ __device__ like the other nmp_dev_*.hpp: tests/host_emul/history_check.hip compiles the same functions for the CPU.
//
// The arithmetic is the reference's own (phys/module_sf_noahmpdrv.F90, "drv"):
//   drv:733-734  SFCRUNOFF = SFCRUNOFF + RUNSF * DT      float32, the product rounded, then the sum rounded
//   drv:736-739  ACCPRCP / ACCECAN / ACCETRAN / ACCEDIR = ACC + X * DT   (the WRF_HYDRO block)
//   drv:426-441  a column is advanced unless it is open water (XLAND - 1.5 >= 0) or sea ice (XICE >= XICE_THRES)
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "noahmp_hip.h"

namespace nmp {

#ifndef NMP_DEV
#define NMP_DEV __host__ __device__ __forceinline__
#endif

constexpr float kHistHuge = 3.40282347e+38f;          // Fortran HUGE(1.0): the identity of MIN (+) and MAX (-)

// drv:426-441, the reference's own test with its own comparisons (a NaN in XLAND or XICE fails both: the column is advanced)
NMP_DEV bool hist_takes_part(float xland, float xice, float xice_thres) {
  return !((xland - 1.5f) >= 0.f) && !(xice >= xice_thres);
}

// one sample into one accumulator.  SUM_DT is two roundings whatever the compiler's contraction setting.
NMP_DEV float hist_apply(int op, float acc, float x, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  switch (op) {
    case NOAHMP_HIST_SUM:    return acc + x;
    case NOAHMP_HIST_SUM_DT: { const float prod = x * scale; return acc + prod; }
    case NOAHMP_HIST_MIN:    return (x < acc) ? x : acc;      // a NaN sample never replaces; a NaN acc stays
    case NOAHMP_HIST_MAX:    return (x > acc) ? x : acc;
    default:                 return x;                        // NOAHMP_HIST_LAST
  }
}

// what NOAHMP_HIST_FIN_RESET leaves behind
NMP_DEV float hist_identity(int op, float acc) {
  switch (op) {
    case NOAHMP_HIST_SUM: case NOAHMP_HIST_SUM_DT: return 0.f;
    case NOAHMP_HIST_MIN: return kHistHuge;
    case NOAHMP_HIST_MAX: return -kHistHuge;
    default: return acc;                                      // LAST: unchanged
  }
}

// the value an output plane receives: the accumulator, or its mean over the steps that advanced the column
NMP_DEV float hist_finish(float acc, int count, bool mean, float fill) {
  if (!mean) return acc;
  return count == 0 ? fill : acc / (float)count;              // IEEE float32 division
}

}  // namespace nmp
