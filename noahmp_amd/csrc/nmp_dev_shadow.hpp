// Cast shadows of the shortwave forcing (noahmp_hip_forcing_shadow): the per-cell functions of the terrain ray march.
// __host__ __device__ like nmp_dev_shortwave.hpp: tests/host_emul/shadow_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them (WRF pairs slope_rad with topo_shading; the form here is a march along the dominant grid axis):
// the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one rounded float32 operation of that text,
// nothing may contract into an FMA, and there are no guards beyond those of the text.  The sun of a cell is sun_vector of
// nmp_dev_shortwave.hpp.  Every index is tested against the window BEFORE it is formed, so no sum of indices can overflow and no cell
// outside the window is ever read.
#pragma once
#include "nmp_dev_shortwave.hpp"

namespace nmp {

// how a march ended; only SHADOW_CAST gives lit = +0.0
enum ShadowExit {
  SHADOW_CAST = 0,       // the terrain stands above the ray
  SHADOW_LOW_SUN = 1,    // max0(u) < mu_min: not marched
  SHADOW_NO_AXIS = 2,    // sun at the zenith, or a NaN direction
  SHADOW_LEFT = 3,       // the ray left the window (either axis)
  SHADOW_ABOVE = 4,      // the ray is above height_max
  SHADOW_BAD_T = 5,      // NaN / Inf in the cross-axis offset
  SHADOW_NSTEP = 6,      // nstep steps without an obstacle
};

// the parameters of noahmp_hip_forcing_shadow that are uniform over the window
struct ShadowParams {
  SunTime now;
  int ni, nj, nstep, has_rot;
  float dx, dy, mu_min, height_max;
};

// the march of one cell: 0 = no march (lit), 1 = x-major, 2 = y-major; d = +-1 along the dominant axis, t = cells of the other axis per
// cell of the dominant one, rise = metres the ray climbs per cell of the dominant axis
struct ShadowRay {
  int major, d;
  float t, rise;
};

NMP_DEV ShadowRay shadow_ray(float gx, float gy, float u, float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ShadowRay r;
  r.major = 0; r.d = 0; r.t = 0.f; r.rise = 0.f;
  const float ax = fabsf(gx) / dx;
  const float ay = fabsf(gy) / dy;
  float a;
  if (ax >= ay && ax > 0.f) {
    r.major = 1;
    a = ax;
    r.d = gx > 0.f ? 1 : -1;
    const float q = gy / dy;
    r.t = q / a;
  } else if (ay > ax) {
    r.major = 2;
    a = ay;
    r.d = gy > 0.f ? 1 : -1;
    const float q = gx / dx;
    r.t = q / a;
  } else {
    return r;                                                  // both zero, or a NaN
  }
  r.rise = u / a;
  return r;
}

// step k of a march, everything but the two heights: the exit it takes without them (or -1), the cells to read and the weight
struct ShadowStep {
  int exit;              // a ShadowExit, or -1: read the heights and compare
  long c0, c1;           // window cells (m, o) and (m, o+1); c1 == c0 when w == 0: the second cell is never read
  float w, ray;
};

// pos_m / pos_o: the cell's index along the dominant / the other axis; M is tested by the caller (k <= room).  O: limit of the other axis.
NMP_DEV ShadowStep shadow_step(const ShadowRay& r, int k, int pos_m, int pos_o, int O, int ni, float z0, float height_max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ShadowStep s;
  s.exit = -1; s.c0 = s.c1 = 0; s.w = 0.f; s.ray = 0.f;
  const float kf = (float)k;
  const float kr = kf * r.rise;
  s.ray = z0 + kr;
  if (s.ray > height_max) { s.exit = SHADOW_ABOVE; return s; }
  const float fo = kf * r.t;
  if (!(fo >= -kf && fo <= kf)) { s.exit = SHADOW_BAD_T; return s; }
  const float jf = floorf(fo);
  s.w = fo - jf;
  const int jo = (int)jf;                                       // |jo| <= k <= 4096
  const int room_hi = (O - 1) - pos_o;                          // >= 0
  if (jo < 0 ? -jo > pos_o : jo > room_hi) { s.exit = SHADOW_LEFT; return s; }
  const bool one = s.w == 0.f;
  if (!one && jo >= room_hi) { s.exit = SHADOW_LEFT; return s; }
  const int m = pos_m + k * r.d, o = pos_o + jo;               // both inside the window now
  if (r.major == 1) {
    s.c0 = (long)o * ni + m;
    s.c1 = one ? s.c0 : s.c0 + ni;
  } else {
    s.c0 = (long)m * ni + o;
    s.c1 = one ? s.c0 : s.c0 + 1;
  }
  return s;
}

// the terrain under the ray at a step whose heights were read
NMP_DEV float shadow_terrain(float h0, float h1, float w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (w == 0.f) return h0;
  const float w0 = 1.0f - w;
  const float a = h0 * w0;
  const float b = h1 * w;
  return a + b;
}

// the march of window cell (i, j) along r.  NF steps are prepared and their heights loaded before the first of them is compared; the
// result is that of the first k, in order, that ends the march.
template <int NF>
NMP_DEV int shadow_march(const float* __restrict__ height, int ni, int nj, int i, int j, const ShadowRay& r, int nstep, float height_max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (r.major == 0) return SHADOW_NO_AXIS;
  const bool xm = r.major == 1;
  const int pos_m = xm ? i : j, pos_o = xm ? j : i;
  const int M = xm ? ni : nj, O = xm ? nj : ni;
  const int room = r.d > 0 ? (M - 1) - pos_m : pos_m;           // steps that stay inside the window along the dominant axis
  const int kmax = nstep < room ? nstep : room;
  const float z0 = height[(long)j * ni + i];
  for (int k0 = 1; k0 <= kmax; k0 += NF) {
    ShadowStep s[NF];
    float h0[NF], h1[NF];
#pragma unroll
    for (int q = 0; q < NF; q++) {
      if (k0 + q <= kmax) {
        s[q] = shadow_step(r, k0 + q, pos_m, pos_o, O, ni, z0, height_max);
      } else {                                                   // past the last step: nothing is read, the end is decided after the loop
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
      if (k0 + q > kmax) break;
      if (s[q].exit >= 0) return s[q].exit;
      if (shadow_terrain(h0[q], h1[q], s[q].w) > s[q].ray) return SHADOW_CAST;
    }
  }
  return nstep > room ? SHADOW_LEFT : SHADOW_NSTEP;
}

// grid components of the sun's horizontal direction: the inverse of the rotation in normal_from_height
NMP_DEV void shadow_grid_dir(const SunVec& v, int has_rot, float ca, float sa, float* gx, float* gy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!has_rot) { *gx = v.e; *gy = v.n; return; }
  const float eca = v.e * ca;
  const float nsa = v.n * sa;
  *gx = eca + nsa;
  const float nca = v.n * ca;
  const float esa = v.e * sa;
  *gy = nca - esa;
}

// one window cell of noahmp_hip_forcing_shadow from its own loaded operands: how its march ends
template <int NF>
NMP_DEV int shadow_cell(const ShadowParams& p, const float* __restrict__ height, float lat, float lon, float ca, float sa, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float phi = lat * NMP_DEGRAD;
  const float sinphi = libm::sinf_(phi), cosphi = libm::cosf_(phi);
  const float hrang = sun_hrang(lon, p.now.hour_utc);
  const SunVec v = sun_vector(sinphi, cosphi, hrang, p.now.sin_declin, p.now.cos_declin);
  const float mu = sw_max0(v.u);
  if (mu < p.mu_min) return SHADOW_LOW_SUN;
  float gx, gy;
  shadow_grid_dir(v, p.has_rot, ca, sa, &gx, &gy);
  const ShadowRay r = shadow_ray(gx, gy, v.u, p.dx, p.dy);
  return shadow_march<NF>(height, p.ni, p.nj, i, j, r, p.nstep, p.height_max);
}

NMP_DEV float shadow_lit(int exit) { return exit == SHADOW_CAST ? 0.f : 1.0f; }

}  // namespace nmp
