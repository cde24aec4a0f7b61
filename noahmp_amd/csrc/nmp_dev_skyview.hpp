// Sky-view factor of the radiation forcing (noahmp_hip_skyview): the per-cell functions of the horizon scan.
// __host__ __device__ like nmp_dev_shadow.hpp: tests/host_emul/skyview_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one
// rounded float32 operation of that text, nothing may contract into an FMA, and there are no guards beyond those of the text.  The ray of a
// direction is shadow_ray and a step is shadow_step / shadow_terrain of nmp_dev_shadow.hpp with a ray that never rises and no height_max:
// the same march, the same window tests before an index is formed, the same bits.  Every exit of a step ends the scan of its direction and
// keeps the steepest slope seen so far.
#pragma once
#include <math.h>
#include "nmp_dev_shadow.hpp"

namespace nmp {

// one direction of the scan, uniform over the window: the march of shadow_ray (major 0 = a zero or NaN direction: term 1) and L2, the
// squared metres of ground per cell of the dominant axis
struct SkyDir {
  int major, d;
  float t, L2;
};

NMP_DEV SkyDir sky_dir(float gx, float gy, float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const ShadowRay r = shadow_ray(gx, gy, 0.f, dx, dy);
  SkyDir s;
  s.major = r.major; s.d = r.d; s.t = r.t; s.L2 = 0.f;
  if (r.major == 0) return s;
  const float sp = r.major == 1 ? dx : dy;
  const float so = r.major == 1 ? dy : dx;
  const float td = r.t * so;
  const float td2 = td * td;
  const float sp2 = sp * sp;
  s.L2 = sp2 + td2;
  return s;
}

// the steepest slope [metres per cell of the dominant axis] from window cell (i, j) of height z0 along dir: +0.0 where nothing stands
// above the cell.  NF steps are prepared and their heights loaded before the first of them is compared; no step's heights decide whether
// the next one runs, so the result is that of the steps taken one by one.
template <int NF>
NMP_DEV float sky_scan(const float* __restrict__ height, int ni, int nj, int i, int j, float z0, const SkyDir& dir, int nstep) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float smax = 0.f;
  if (dir.major == 0) return smax;
  ShadowRay r;
  r.major = dir.major; r.d = dir.d; r.t = dir.t; r.rise = 0.f;
  const bool xm = r.major == 1;
  const int pos_m = xm ? i : j, pos_o = xm ? j : i;
  const int M = xm ? ni : nj, O = xm ? nj : ni;
  const int room = r.d > 0 ? (M - 1) - pos_m : pos_m;           // steps that stay inside the window along the dominant axis
  const int kmax = nstep < room ? nstep : room;
  for (int k0 = 1; k0 <= kmax; k0 += NF) {
    ShadowStep s[NF];
    float h0[NF], h1[NF];
#pragma unroll
    for (int q = 0; q < NF; q++) {
      if (k0 + q <= kmax) {
        s[q] = shadow_step(r, k0 + q, pos_m, pos_o, O, ni, z0, INFINITY);
      } else {                                                   // past the last step: nothing is read
        s[q].exit = SHADOW_NSTEP; s[q].c0 = s[q].c1 = 0; s[q].w = s[q].ray = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < NF; q++) {
      h0[q] = h1[q] = 0.f;
      if (s[q].exit < 0) { h0[q] = height[s[q].c0]; h1[q] = height[s[q].c1]; }
    }
#pragma unroll
    for (int q = 0; q < NF; q++) {
      if (s[q].exit >= 0) return smax;                           // the window's edge, a NaN / Inf offset, or past kmax
      const float zt = shadow_terrain(h0[q], h1[q], s[q].w);
      const float dz = zt - z0;
      const float sl = dz / (float)(k0 + q);
      if (sl > smax) smax = sl;                                  // a NaN is ignored
    }
  }
  return smax;
}

// cos^2 of the horizon's elevation angle in one direction
NMP_DEV float sky_term(float smax, float L2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (smax == 0.f) return 1.0f;
  const float s2 = smax * smax;
  const float den = L2 + s2;
  return L2 / den;
}

// one window cell of noahmp_hip_skyview: the mean of sky_term over the directions, summed in their order
template <int NF>
NMP_DEV float sky_cell(const float* __restrict__ height, int ni, int nj, int i, int j, int nstep, int ndir, const SkyDir* dirs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float z0 = height[(long)j * ni + i];
  float acc = 0.f;
  for (int q = 0; q < ndir; q++) {
    const float smax = sky_scan<NF>(height, ni, nj, i, j, z0, dirs[q], nstep);
    const float term = dirs[q].major == 0 ? 1.0f : sky_term(smax, dirs[q].L2);
    acc = acc + term;
  }
  return acc / (float)ndir;
}

}  // namespace nmp
