// Budget-preserving regrid (noahmp_hip_forcing_regrid_conserve): the per-cell and per-group arithmetic.
// __host__ __device__ like the other nmp_dev_*.hpp: tests/host_emul/regrid_conserve_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  The bilinear value
// is nmp_dev_regrid.hpp's; terms and sums are float64 (a product of two float32 values is exact there), the ratio is one float64 product
// and one float64 division rounded once to float32, and nothing may contract into an FMA whatever the compiler's setting.
#pragma once
#include "nmp_dev_regrid.hpp"

namespace nmp {

// what a group hands to its members: out = kind == RC_SCALE ? v * val : val
enum { RC_ZERO = 0, RC_SCALE = 1, RC_SOURCE = 2 };

// the owner of a window cell, or -1: a cell that BILINEAR fills, or whose near is out of range, is no member
NMP_DEV int rc_group(int base, int near, const float* w, int nx, int nxny, int periodic, int* idx) {
  if (!regrid_corners(base, w, nx, nxny, periodic, idx)) return -1;
  return regrid_near_ok(near, nxny) ? near : -1;
}

// q = g * pattern (one rounding), v = (q > 0) ? q : +0.0f: NaN and negatives become +0.0
NMP_DEV float rc_value(float g, bool has_pattern, float pattern) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float q = has_pattern ? g * pattern : g;
  return (q > 0.f) ? q : 0.f;
}

// the term of a member: exact in float64
NMP_DEV double rc_term(float area, float v) { return (double)area * (double)v; }

NMP_DEV bool rc_area_ok(float area) { return area > 0.f && area < INFINITY; }

// what group s gives its members, from p = src[s], D_s and N_s
NMP_DEV int rc_group_result(float p, double D, double N, float* val) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(p > 0.f)) { *val = 0.f; return RC_ZERO; }
  if (N > 0.0) {
    const double num = (double)p * D;
    const double ratio = num / N;
    *val = (float)ratio;
    return RC_SCALE;
  }
  *val = p;
  return RC_SOURCE;
}

NMP_DEV float rc_out(int kind, float val, float v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return kind == RC_SCALE ? v * val : val;
}

}  // namespace nmp
