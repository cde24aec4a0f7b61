// Terrain-adjusted wind of the forcing (noahmp_hip_wind_terrain / noahmp_hip_forcing_wind): the per-cell functions.
// __host__ __device__ like nmp_dev_skyview.hpp: tests/host_emul/wind_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h (the MicroMet wind model, Liston and Elder
// 2006, with the two maxima given by the caller), every rounding included.  Every line is one rounded float32 operation of that text,
// nothing may contract into an FMA, and there are no guards beyond those of the text.  The libm forms are libm::atanf_ / sinf_ / cosf_
// (glibc's bits), which hold no table: nothing is staged in LDS.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#endif
#include "nmp_libm.hpp"

namespace nmp {

#ifndef NMP_DEV
#define NMP_DEV __host__ __device__ __forceinline__
#endif

// what a window fixes for every cell: the curvature distances of the text, made once (IEEE float32 operations: the same bits on either side)
struct WindTerrainParams {
  int ni, nj, ncurv, has_rot;
  float dx, dy;
  float den_x, den_y, den_d;             // 2.0f*lx, 2.0f*ly, 2.0f*d
};

NMP_DEV WindTerrainParams wind_terrain_params(int ni, int nj, int ncurv, int has_rot, float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  WindTerrainParams p;
  p.ni = ni; p.nj = nj; p.ncurv = ncurv; p.has_rot = has_rot; p.dx = dx; p.dy = dy;
  const float nc = (float)ncurv;
  const float lx = nc * dx;
  const float ly = nc * dy;
  const float dx2 = dx * dx;
  const float dy2 = dy * dy;
  const float d2 = dx2 + dy2;
  const float d = nc * sqrtf(d2);
  p.den_x = 2.0f * lx;
  p.den_y = 2.0f * ly;
  p.den_d = 2.0f * d;
  return p;
}

struct WindSlope {
  float sx, sy, curv;
};

// one curvature term: (z - 0.5f*(a + b)) / den
NMP_DEV float wind_curv_term(float z, float a, float b, float den) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s = a + b;
  const float h = 0.5f * s;
  const float n = z - h;
  return n / den;
}

// one window cell of noahmp_hip_wind_terrain; every index is clamped into the window before it is formed
NMP_DEV WindSlope wind_terrain_cell(const WindTerrainParams& p, const float* __restrict__ height, float ca, float sa, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int ni = p.ni, nj = p.nj;
  const long row = (long)j * ni;
  const float z = height[row + i];
  const int ie = i + 1 < ni - 1 ? i + 1 : ni - 1, iw = i - 1 > 0 ? i - 1 : 0;
  const int jn = j + 1 < nj - 1 ? j + 1 : nj - 1, js = j - 1 > 0 ? j - 1 : 0;
  float gx = 0.f, gy = 0.f;
  if (ie != iw) {
    const float dz = height[row + ie] - height[row + iw];
    const float len = (float)(ie - iw) * p.dx;
    gx = dz / len;
  }
  if (jn != js) {
    const float dz = height[(long)jn * ni + i] - height[(long)js * ni + i];
    const float len = (float)(jn - js) * p.dy;
    gy = dz / len;
  }
  float ge = gx, gn = gy;
  if (p.has_rot) {
    const float p1 = gx * ca;
    const float p2 = gy * sa;
    const float p3 = gy * ca;
    const float p4 = gx * sa;
    ge = p1 - p2;
    gn = p3 + p4;
  }
  const float ge2 = ge * ge;
  const float gn2 = gn * gn;
  const float g2 = ge2 + gn2;
  const float g = sqrtf(g2);
  const float beta = libm::atanf_(g);
  const float q = beta / g;
  WindSlope s;
  s.sx = g == 0.f ? 0.f : ge * q;
  s.sy = g == 0.f ? 0.f : gn * q;
  const int nc = p.ncurv;                                         // 1 .. 64 and i, j < 2^31 / ni: no overflow
  const int E = (long)i + nc < ni - 1 ? i + nc : ni - 1, W = i - nc > 0 ? i - nc : 0;
  const int N = (long)j + nc < nj - 1 ? j + nc : nj - 1, S = j - nc > 0 ? j - nc : 0;
  const long rowN = (long)N * ni, rowS = (long)S * ni;
  const float t1 = wind_curv_term(z, height[row + W], height[row + E], p.den_x);
  const float t2 = wind_curv_term(z, height[rowS + i], height[rowN + i], p.den_y);
  const float t3 = wind_curv_term(z, height[rowS + W], height[rowN + E], p.den_d);
  const float t4 = wind_curv_term(z, height[rowN + W], height[rowS + E], p.den_d);
  const float t12 = t1 + t2;
  const float t123 = t12 + t3;
  const float t1234 = t123 + t4;
  s.curv = 0.25f * t1234;
  return s;
}

struct WindParams {
  float ds, dc;                          // slope_max + slope_max, curv_max + curv_max
  float gamma_s, gamma_c;
  int turn;
};

NMP_DEV float wind_clamp_half(float x) {                         // a NaN stays a NaN
  if (x < -0.5f) x = -0.5f;
  if (x > 0.5f) x = 0.5f;
  return x;
}

// one column of noahmp_hip_forcing_wind, in place; false: the column keeps its bits and *up, *vp are untouched
NMP_DEV bool wind_column(const WindParams& k, float sx, float sy, float curv, float* up, float* vp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (sx == 0.f && sy == 0.f && curv == 0.f) return false;
  const float u = *up, v = *vp;
  const float uu = u * u;
  const float vv = v * v;
  const float W2 = uu + vv;
  const float W = sqrtf(W2);
  if (W == 0.f) return false;
  const float d1 = u * sx;
  const float d2 = v * sy;
  const float dot = d1 + d2;
  const float r = dot / W;
  const float os = wind_clamp_half(r / k.ds);
  const float oc = wind_clamp_half(curv / k.dc);
  const float a = k.gamma_s * os;
  const float b = k.gamma_c * oc;
  const float wa = 1.0f + a;
  const float ww = wa + b;
  if (!k.turn) {
    *up = ww * u;
    *vp = ww * v;
    return true;
  }
  const float sx2 = sx * sx;
  const float sy2 = sy * sy;
  const float b2 = sx2 + sy2;
  const float c1 = sx * v;
  const float c2 = sy * u;
  const float cr = c1 - c2;
  const float n0 = 2.0f * dot;
  const float n = n0 * cr;
  const float m = W2 * b2;
  const float s2 = b2 == 0.f ? 0.f : n / m;
  const float h = -0.5f * os;
  const float td = h * s2;
  const float ct = libm::cosf_(td), st = libm::sinf_(td);
  const float uc = u * ct;
  const float vs = v * st;
  const float vc = v * ct;
  const float us = u * st;
  const float ur = uc + vs;
  const float vr = vc - us;
  *up = ww * ur;
  *vp = ww * vr;
  return true;
}

}  // namespace nmp
