// Diffusive-wave routing on the D8 network (noahmp_hip_flow_drop / noahmp_hip_route_diffusive): the per-cell functions.  __host__
// __device__ like nmp_dev_channel.hpp: tests/host_emul/diffusive_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one
// rounded float32 operation of that text, nothing may contract into an FMA, and there are no guards beyond those of the text;
// libm::powf_ is the one exception, as in nmp_dev_channel.hpp.  Where the kinematic cell releases Manning's discharge at its BED slope,
// here the friction slope is the slope of the water surface to the downstream cell: the bed drop plus the difference of the two depths,
// the downstream one read from the plane the call before wrote.  A cell whose surface does not stand above its downstream cell's
// releases nothing (backwater), and a release never exceeds `limit` times the volume that would level the two surfaces.  The gather is
// the kinematic one: no float atomics, and the bits do not depend on who runs first.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#endif
#include "nmp_dev_channel.hpp"

namespace nmp {

struct FlowDropArgs {
  const float* height; const float* slope;                         // exactly one of the two
  const uint8_t* dir;
  float* drop;
  int ni, nj;
  float dx, dy, d;
};

// one window cell of noahmp_hip_flow_drop: the bed drop to the downstream cell [m].  With heights the `drop` line of channel_geom_cell,
// +0 where the cell has no downstream cell inside the window; with slopes slope*len, len by channel_geom_cell's rule.
NMP_DEV void flow_drop_cell(const FlowDropArgs& g, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long c = (long)j * g.ni + i;
  const int kb = (int)g.dir[c];
  const int k = kb > 8 ? 0 : kb;                                   // a byte above 8 counts as 0
  float drop = 0.f;
  if (g.slope) {
    const float len = (k & 1) ? ((k & 2) ? g.dy : g.dx) : (k ? g.d : g.dx);
    drop = g.slope[c] * len;
  } else {
    const int kk = k ? k : 1;                                      // k == 0: any legal k, the select below drops it
    const int di = flow_di(kk), dj = flow_dj(kk);
    const bool in = k != 0 && flow_inside(g.ni, g.nj, i + di, j + dj);
    const float z0 = g.height[c];
    const float zn = g.height[in ? c + (long)dj * g.ni + di : c];
    const float dz = z0 - zn;
    drop = in ? dz : 0.f;
  }
  g.drop[c] = drop;
}

struct DiffusiveCellArgs {
  const uint8_t* inmask; const int32_t* col_index; const uint8_t* dir;
  const float* area; const float* width; const float* length; const float* conv; const float* manning; const float* drop;
  float* storage; const float* out_old; float* out_new;
  const float* runoff_a; const float* runoff_b;
  const float* depth_old; float* depth_new;
  float scale, dt, limit;
  int ni, nj;
  long ncol;
};

// what a cell reports to the four diag words: the float32 bits of its cr where cr > 0 or cr is a NaN (else 0), and the three counts
struct DiffusiveReport {
  uint32_t cr_bits;
  uint32_t capped;                                                 // released all it held, and was not limited
  uint32_t limited;
  uint32_t blocked;
};

// One window cell of noahmp_hip_route_diffusive.  A ring cell reports nothing and writes nothing.  The gather and the plane loads are
// those of kinematic_cell.  LOAD_ALL_HD = false: the downstream depth is one load whose address depends on dir[c]; true: all eight
// neighbours' depths are loaded from an address made legal and k selects -- the same word either way.
template <bool PIN, bool LOAD_ALL_HD>
NMP_DEV DiffusiveReport diffusive_cell(const DiffusiveCellArgs& r, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  DiffusiveReport rep;
  rep.cr_bits = 0u; rep.capped = 0u; rep.limited = 0u; rep.blocked = 0u;
  const long c = (long)j * r.ni + i;
  const long d = (long)r.col_index[c];
  if (d < -1 || d >= r.ncol) return rep;                           // a ring cell: read by others and never written
  const unsigned m = r.inmask[c];
  const int kb = (int)r.dir[c];
  const int k = kb > 8 ? 0 : kb;                                   // a byte above 8 counts as 0
  float on[8];
#pragma unroll
  for (int n = 1; n <= 8; n++) {
    const int di = flow_di(n), dj = flow_dj(n);
    const bool in = flow_inside(r.ni, r.nj, i + di, j + dj);
    on[n - 1] = r.out_old[in ? c + (long)dj * r.ni + di : c];
  }
  const int kk = k ? k : 1;                                        // k == 0: any legal k, `has` drops it
  const bool has = k != 0 && flow_inside(r.ni, r.nj, i + flow_di(kk), j + flow_dj(kk));
  float hd;
  if (LOAD_ALL_HD) {
    float dn[8];
#pragma unroll
    for (int n = 1; n <= 8; n++) {
      const int di = flow_di(n), dj = flow_dj(n);
      const bool in = flow_inside(r.ni, r.nj, i + di, j + dj);
      dn[n - 1] = r.depth_old[in ? c + (long)dj * r.ni + di : c];
    }
    hd = dn[0];
#pragma unroll
    for (int n = 2; n <= 8; n++) hd = (kk == n) ? dn[n - 1] : hd;
  } else {
    hd = r.depth_old[has ? c + (long)flow_dj(kk) * r.ni + flow_di(kk) : c];
  }
  const float st = r.storage[c];
  const float width = r.width[c];
  const float length = r.length[c];
  const float conv = r.conv[c];
  const float manning = r.manning[c];
  const float drop = r.drop[c];
  float v = 0.f;
  if (d >= 0) {
    float x = r.runoff_a[d];
    if (r.runoff_b) x = x + r.runoff_b[d];
    const float xs = x * r.scale;
    v = xs * r.area[c];
  }
#if defined(__HIP_DEVICE_COMPILE__)
  if (PIN) __builtin_amdgcn_sched_barrier(0);                      // the loads above are in flight before the libm call
#endif
  float q = 0.f;
#pragma unroll
  for (int n = 1; n <= 8; n++) {
    const bool take = ((m >> (n - 1)) & 1u) && flow_inside(r.ni, r.nj, i + flow_di(n), j + flow_dj(n));
    const float qk = q + on[n - 1];
    q = take ? qk : q;
  }
  const float sv = st + v;
  const float s1 = sv + q;
  const float wl = width * length;
  float o = 0.f, cr = 0.f;
  bool capped = false, limited = false, blocked = false;
  if (s1 > 0.f && conv > 0.f) {                                    // a NaN s1 does not enter; conv == 0 holds the water (lakes)
    const float h = s1 / wl;
    bool open = true;
    float cvd = conv, lim = 0.f;                                   // an outlet: normal depth at the bed slope, the kinematic bits
    if (has) {
      const float dd = h - hd;
      const float dh = drop + dd;
      open = dh > 0.f;                                             // a NaN is not open
      const float sf = dh / length;
      const float rt = sqrtf(sf);
      cvd = rt / manning;
      const float half = r.limit * dh;
      lim = half * wl;
    }
    if (open) {
      const float a = width * h;
      const float h2 = h + h;
      const float p = width + h2;
      const float R = a / p;
      const float r23 = libm::powf_(R, kTwoThirds);
      const float vel = cvd * r23;
      const float qa = vel * a;
      const float od = qa * r.dt;
      capped = !(od < s1);
      o = capped ? s1 : od;
      limited = has && lim < o;
      o = limited ? lim : o;
      const float vd = vel * r.dt;
      cr = vd / length;
    } else {
      blocked = true;
    }
  }
  const float s2 = s1 - o;
  r.storage[c] = s2;
  r.out_new[c] = o;
  const float h1 = s2 / wl;
  r.depth_new[c] = (s2 > 0.f) ? h1 : 0.f;
  rep.cr_bits = (cr > 0.f || cr != cr) ? libm::asuint(cr) : 0u;
  rep.capped = (capped && !limited) ? 1u : 0u;
  rep.limited = limited ? 1u : 0u;
  rep.blocked = blocked ? 1u : 0u;
  return rep;
}

}  // namespace nmp
