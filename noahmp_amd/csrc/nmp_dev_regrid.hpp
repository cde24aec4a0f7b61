// Forcing regrid (noahmp_hip_regrid_plan_latlon / noahmp_hip_forcing_regrid): the per-cell functions of the plan and of the value.
// __host__ __device__ like the other nmp_dev_*.hpp: tests/host_emul/regrid_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them (the reference reads forcing already on the model grid, netcdf_io:1140): the contract is the
// text in include/noahmp_hip.h, every rounding included.  Index arithmetic is float64, weights and values are float32, and nothing may
// contract into an FMA whatever the compiler's setting.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#endif
#include "noahmp_hip.h"
#include "nmp_libm.hpp"

namespace nmp {

#ifndef NMP_DEV
#define NMP_DEV __host__ __device__ __forceinline__
#endif

struct RegridCell {
  int base, near;
  float w[4];
};

// nearest valid source cell in the Chebyshev window of `radius` around (round(fx), round(fy)); -1 if there is none.
// Distance in float64 index space, wrapped in i when periodic; equal distances: the lowest linear index.
__host__ __device__ inline int regrid_search(double fx, double fy, int nx, int ny, int periodic, const unsigned char* valid, int radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int ri = (int)floor(fx + 0.5), rj = (int)floor(fy + 0.5);
  int best = -1;
  double bestd = 0.0;
  for (int j = rj - radius; j <= rj + radius; j++) {
    if (j < 0 || j >= ny) continue;
    for (int ii = ri - radius; ii <= ri + radius; ii++) {
      int i = ii;
      if (periodic) { i = ii % nx; if (i < 0) i += nx; }
      else if (i < 0 || i >= nx) continue;
      const int idx = j * nx + i;
      if (!valid[idx]) continue;
      double dx = fabs((double)i - fx);
      if (periodic) { const double other = (double)nx - dx; if (other < dx) dx = other; }
      const double dy = (double)j - fy;
      const double xx = dx * dx, yy = dy * dy;
      const double d = xx + yy;
      if (best < 0 || d < bestd || (d == bestd && idx < best)) { best = idx; bestd = d; }
    }
  }
  return best;
}

// the plan of one target cell
__host__ __device__ inline RegridCell regrid_plan_cell(float lat, float lon, int nx, int ny, double lon0, double lat0, double dlon, double dlat,
                                                       int periodic, const unsigned char* valid, int radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RegridCell c;
  c.base = c.near = -1;
  c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0.f;
  double fx = ((double)lon - lon0) / dlon;
  if (periodic) {
    const double turns = floor(fx / (double)nx) * (double)nx;
    fx = fx - turns;
    if (fx < 0.0) fx = fx + (double)nx;
    if (fx >= (double)nx) fx = fx - (double)nx;
  }
  double fy = ((double)lat - lat0) / dlat;
  const double xlo = periodic ? 0.0 : -0.5, xhi = periodic ? (double)nx : (double)nx - 0.5;
  if (!(fx >= xlo && fx <= xhi) || !(fy >= -0.5 && fy <= (double)ny - 0.5)) return c;      // NaN fails every comparison: outside
  if (!periodic) { if (fx < 0.0) fx = 0.0; if (fx > (double)(nx - 1)) fx = (double)(nx - 1); }
  if (fy < 0.0) fy = 0.0;
  if (fy > (double)(ny - 1)) fy = (double)(ny - 1);
  int j0 = (int)floor(fy);
  if (j0 > ny - 2) j0 = ny - 2;
  int i0 = (int)floor(fx);
  if (!periodic && i0 > nx - 2) i0 = nx - 2;
  int i1 = i0 + 1;
  if (periodic && i1 == nx) i1 = 0;
  const int j1 = j0 + 1;
  const float tx = (float)(fx - (double)i0), ty = (float)(fy - (double)j0);
  const float ux = 1.f - tx, uy = 1.f - ty;
  float w[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
  const int idx[4] = {j0 * nx + i0, j0 * nx + i1, j1 * nx + i0, j1 * nx + i1};
  bool ok[4] = {true, true, true, true};
  int nvalid = 4, found = -1;
  bool replaced = false;
  c.base = idx[0];
  if (valid) {
    nvalid = 0;
    for (int k = 0; k < 4; k++) {
      ok[k] = valid[idx[k]] != 0;
      if (ok[k]) nvalid++; else w[k] = 0.f;
    }
    if (nvalid < 4) {
      const float s = ((w[0] + w[1]) + w[2]) + w[3];
      if (s > 0.f) {
        for (int k = 0; k < 4; k++) w[k] = w[k] / s;
      } else {
        found = regrid_search(fx, fy, nx, ny, periodic, valid, radius);
        c.base = found;
        replaced = true;
      }
    }
  }
  const int pk = (tx > 0.5f ? 1 : 0) + (ty > 0.5f ? 2 : 0);
  if (ok[pk]) c.near = idx[pk];
  else if (nvalid > 0) {
    int bk = -1;
    for (int k = 0; k < 4; k++)
      if (ok[k] && (bk < 0 || w[k] > w[bk])) bk = k;
    c.near = idx[bk];
  } else c.near = found;
  if (replaced) { w[0] = found >= 0 ? 1.f : 0.f; w[1] = w[2] = w[3] = 0.f; }
  for (int k = 0; k < 4; k++) c.w[k] = w[k];
  return c;
}

// BILINEAR: the corner indices of a column from its base; false = the column receives fill.  Corners of weight zero are not tested:
// they are never read.
NMP_DEV bool regrid_corners(int base, const float* w, int nx, int nxny, int periodic, int* idx) {
  if ((unsigned)base >= (unsigned)nxny) return false;
  int c1 = base + 1;
  if (periodic && base % nx == nx - 1) c1 -= nx;
  idx[0] = base; idx[1] = c1; idx[2] = base + nx; idx[3] = c1 + nx;
  bool ok = true;
  for (int k = 1; k < 4; k++) ok = ok && (w[k] == 0.f || idx[k] < nxny);
  return ok;
}

// the weighted sum over the corners that are read: each product rounded, then the sum
NMP_DEV float regrid_bilinear(const float* w, const float* s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float acc = 0.f;
  bool any = false;
  for (int k = 0; k < 4; k++) {
    if (w[k] == 0.f) continue;
    const float prod = w[k] * s[k];
    acc = any ? acc + prod : prod;
    any = true;
  }
  return acc;
}

NMP_DEV bool regrid_near_ok(int near, int nxny) { return (unsigned)near < (unsigned)nxny; }

// v + scale * adjust: the product rounded, then the sum
NMP_DEV float regrid_adjust(float v, float scale, float adj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float prod = scale * adj;
  return v + prod;
}

// ---- the met group of noahmp_hip_forcing_regrid_met: t, p, q, lw moved from the source's terrain height to the model's (Cosgrove et
// al. 2003).  Every line is one rounded float32 operation of the header text; expf_ / powf_ are the checked forms of nmp_libm.hpp
// (glibc's bits).  No guards: what the arithmetic gives for unphysical operands is the result.
struct RegridMet {
  float t, p, q, lw;
};

// saturation vapour pressure over water [Pa]
NMP_DEV float regrid_met_esat(float t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = t - 273.15f;
  const float num = 17.67f * a;
  const float den = t - 29.65f;
  const float x = num / den;
  return 611.2f * libm::expf_(x);
}

// saturation specific humidity from esat(t) and the pressure
NMP_DEV float regrid_met_qsat(float es, float p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float num = 0.622f * es;
  const float part = 0.378f * es;
  const float den = p - part;
  return num / den;
}

// clear-sky emissivity (Satterlund 1979) from specific humidity, pressure and temperature
NMP_DEV float regrid_met_emis(float q, float p, float t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float qp = q * p;
  const float e = qp / 0.622f;
  const float mb = e / 100.0f;
  const float ex = t / 2016.0f;
  const float pw = libm::powf_(mb, ex);
  const float en = libm::expf_(-pw);
  const float one = 1.0f - en;
  return 1.08f * one;
}

// (tc, pc, qc, lc) at the source's height -> the four values d metres higher; has_lw false: lc is passed through and no emissivity is made
NMP_DEV RegridMet regrid_met(float tc, float pc, float qc, float lc, float d, float lapse, bool has_lw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RegridMet r;
  r.t = tc; r.p = pc; r.q = qc; r.lw = lc;
  if (d == 0.f) return r;                                    // either sign; a NaN d goes on and makes NaN
  const float tf = regrid_adjust(tc, lapse, d);
  const float tsum = tc + tf;
  const float tbar = tsum * 0.5f;
  const float gd = 9.81f * d;
  const float rt = 287.0f * tbar;
  const float hx = gd / rt;
  const float pf = pc / libm::expf_(hx);
  const float esc = regrid_met_esat(tc), esf = regrid_met_esat(tf);
  const float rh = qc / regrid_met_qsat(esc, pc);
  const float qf = rh * regrid_met_qsat(esf, pf);
  r.t = tf; r.p = pf; r.q = qf;
  if (has_lw) {
    const float er = regrid_met_emis(qf, pf, tf) / regrid_met_emis(qc, pc, tc);
    const float le = lc * er;
    const float tf2 = tf * tf, tc2 = tc * tc;
    const float tf4 = tf2 * tf2, tc4 = tc2 * tc2;
    const float tr = tf4 / tc4;
    r.lw = le * tr;
  }
  return r;
}

}  // namespace nmp
