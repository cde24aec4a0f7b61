// Depression filling and flat resolution for the D8 network (noahmp_hip_flow_fill_init / noahmp_hip_flow_fill): the per-cell functions.
// __host__ __device__ like nmp_dev_routing.hpp: tests/host_emul/flow_fill_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one
// rounded float32 operation of that text, nothing may contract into an FMA, and float32 denormals are kept.  Minimum and maximum are
// written as ONE comparison and a select each (fill_min, fill_max), never fminf / fmaxf: which of two equal operands (+0 and -0) comes
// back is then fixed by the text and is the same on the host and on the device.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#endif
#include "nmp_dev_routing.hpp"

namespace nmp {

NMP_DEV uint32_t fill_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(x);
#else
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
#endif
}

NMP_DEV float fill_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float x;
  memcpy(&x, &b, 4);
  return x;
#endif
}

NMP_DEV float fill_inf() { return fill_float(0x7F800000u); }

// min(a, b) = (b < a) ? b : a and max(a, b) = (b > a) ? b : a: a NaN b never wins, equal operands give a
NMP_DEV float fill_min(float a, float b) { return (b < a) ? b : a; }
NMP_DEV float fill_max(float a, float b) { return (b > a) ? b : a; }

// the smallest float32 greater than m, in integer arithmetic on the bits; up(+-0) is the smallest subnormal, up(+inf) = +inf,
// up(-inf) = -FLT_MAX, a NaN keeps its bits
NMP_DEV float fill_up(float m) {
  const uint32_t b = fill_bits(m);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return m;                   // NaN
  if (b == 0x7F800000u) return m;                                  // +inf
  if ((b & 0x7FFFFFFFu) == 0u) return fill_float(1u);              // +-0
  return fill_float((b & 0x80000000u) ? b - 1u : b + 1u);
}

// lift(m) = max(fl32(m + eps), up(m)): strictly above every finite m, monotone
NMP_DEV float fill_lift(float m, float eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = m + eps;
  return fill_max(a, fill_up(m));
}

// what one cell becomes from its own w, its height and the minimum m of its neighbours' w
NMP_DEV float fill_relax(float w, float z, float m, float eps) {
  const float cand = fill_max(z, fill_lift(m, eps));
  return fill_min(w, cand);
}

// the side flags as noahmp_hip.h names them: bits 0..3 = OUTLET_W, _E, _S, _N; bits 4..7 = RING_W, _E, _S, _N
NMP_DEV unsigned fill_side_bits(int ni, int nj, int i, int j) {
  return (i == 0 ? 1u : 0u) | (i == ni - 1 ? 2u : 0u) | (j == 0 ? 4u : 0u) | (j == nj - 1 ? 8u : 0u);
}

// one window cell of noahmp_hip_flow_fill_init: writes fixed[c] and w_old[c]
NMP_DEV void fill_init_cell(int ni, int nj, const float* __restrict__ height, const uint8_t* __restrict__ outlet, uint8_t* __restrict__ fixed,
                            float* __restrict__ w_old, int flags, int i, int j) {
  const long c = (long)j * ni + i;
  const unsigned side = fill_side_bits(ni, nj, i, j);
  const float z = height[c];
  uint8_t f = 0;
  if (side & ((unsigned)flags >> 4)) {
    f = 2;
  } else {
    bool out = (z != z) || (side & (unsigned)flags) != 0u;
    if (outlet) out = out || outlet[c] != 0;
#pragma unroll
    for (int k = 1; k <= 8; k++) {
      const int di = flow_di(k), dj = flow_dj(k);
      const bool in = flow_inside(ni, nj, i + di, j + dj);
      const float zn = height[in ? c + (long)dj * ni + di : c];
      out = out || (in && zn != zn);
    }
    f = out ? 1 : 0;
  }
  fixed[c] = f;
  w_old[c] = f == 1 ? z : fill_inf();
}

// one window cell of the pinned form of noahmp_hip_flow_fill (sweeps == 1): one Jacobi application from w_old.  All eight words are
// loaded from an address made legal (the cell's own where the neighbour is outside) and the minimum selects, as in flow_accumulate_cell.
NMP_DEV float fill_pass_cell(int ni, int nj, const float* __restrict__ height, const uint8_t* __restrict__ fixed,
                             const float* __restrict__ w_old, float eps, int i, int j) {
  const long c = (long)j * ni + i;
  const float w = w_old[c];
  float v[8];
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const int di = flow_di(k), dj = flow_dj(k);
    v[k - 1] = w_old[flow_inside(ni, nj, i + di, j + dj) ? c + (long)dj * ni + di : c];
  }
  if (fixed[c]) return w;
  float m = fill_inf();
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const float mk = fill_min(m, v[k - 1]);
    m = flow_inside(ni, nj, i + flow_di(k), j + flow_dj(k)) ? mk : m;
  }
  return fill_relax(w, height[c], m, eps);
}

}  // namespace nmp
