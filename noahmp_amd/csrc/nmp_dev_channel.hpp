// Kinematic-wave routing with Manning friction on the D8 network (noahmp_hip_flow_channel / noahmp_hip_route_kinematic): the per-cell
// functions.  __host__ __device__ like nmp_dev_routing.hpp: tests/host_emul/channel_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one
// rounded float32 operation of that text, nothing may contract into an FMA, and there are no guards beyond those of the text.  The one
// exception is libm::powf_, glibc's algorithm in float64 with the fused mad() it uses on purpose (nmp_libm.hpp): the contract-off pragma
// governs the float32 lines only.  A cell GATHERS from its neighbours in ascending k, as route_cell does (the gather is restated here):
// no float atomics, and the bits do not depend on who runs first.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#endif
#include "nmp_dev_routing.hpp"
#include "nmp_libm.hpp"

namespace nmp {

// the exponent 2/3 of Manning's hydraulic radius as the float32 word 0x3F2AAAAB, (float)(2.0/3.0): a hex float, so nothing depends on a
// compiler's decimal conversion
constexpr float kTwoThirds = 0x1.555556p-1f;
static_assert(__builtin_bit_cast(uint32_t, kTwoThirds) == 0x3F2AAAABu, "2/3 rounded to float32");

// the diagonal of a cell, with the three roundings of flow_params (made once on the host)
NMP_DEV float channel_diagonal(float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dx2 = dx * dx;
  const float dy2 = dy * dy;
  const float d2 = dx2 + dy2;
  return sqrtf(d2);
}

struct ChannelGeomArgs {
  const float* height; const float* slope;                         // exactly one of the two
  const uint8_t* dir; const float* manning;
  float* length; float* conv;
  FlowParams p;
  float dx, dy, d, smin;
};

// one window cell of noahmp_hip_flow_channel: the flow length along the cell's direction and conv = sqrt(max(s, smin)) / n
NMP_DEV void channel_geom_cell(const ChannelGeomArgs& g, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long c = (long)j * g.p.ni + i;
  const int kb = (int)g.dir[c];
  const int k = kb > 8 ? 0 : kb;                                   // a byte above 8 counts as 0
  const float len = (k & 1) ? ((k & 2) ? g.dy : g.dx) : (k ? g.d : g.dx);
  float s = g.smin;
  if (g.slope) {
    s = g.slope[c];
  } else {
    const int kk = k ? k : 1;                                      // k == 0: any legal k, the select below drops it
    const int di = flow_di(kk), dj = flow_dj(kk);
    const bool in = k != 0 && flow_inside(g.p.ni, g.p.nj, i + di, j + dj);
    const float z0 = g.height[c];
    const float zn = g.height[in ? c + (long)dj * g.p.ni + di : c];
    const float inv = (k & 1) ? ((k & 2) ? g.p.inv_y : g.p.inv_x) : g.p.inv_d;
    const float drop = z0 - zn;
    const float sk = drop * inv;
    s = in ? sk : g.smin;
  }
  const float sf = (s > g.smin) ? s : g.smin;                      // a NaN gives smin
  const float r = sqrtf(sf);
  const float n = g.manning[c];
  const float cv = r / n;
  g.length[c] = len;
  g.conv[c] = (n > 0.f) ? cv : 0.f;
}

struct KinematicCellArgs {
  const uint8_t* inmask; const int32_t* col_index;
  const float* area; const float* width; const float* length; const float* conv;
  float* storage; const float* out_old; float* out_new;
  const float* runoff_a; const float* runoff_b;
  float* depth;                                                    // or NULL
  float scale, dt;
  int ni, nj;
  long ncol;
};

// what a cell reports to the two diag words: the float32 bits of its cr where cr > 0 or cr is a NaN (else 0), and whether it was capped
struct KinematicReport {
  uint32_t cr_bits;
  uint32_t capped;
};

// One window cell of noahmp_hip_route_kinematic.  A ring cell reports nothing and writes nothing.  All eight neighbours are loaded from an
// address made legal (the cell's own where the neighbour is outside) and the sum selects, as route_cell<true>; the plane loads are issued
// with them, in front of the powf_.
template <bool PIN>
NMP_DEV KinematicReport kinematic_cell(const KinematicCellArgs& r, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  KinematicReport rep;
  rep.cr_bits = 0u; rep.capped = 0u;
  const long c = (long)j * r.ni + i;
  const long d = (long)r.col_index[c];
  if (d < -1 || d >= r.ncol) return rep;                           // a ring cell: read by others and never written
  const unsigned m = r.inmask[c];
  float on[8];
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const int di = flow_di(k), dj = flow_dj(k);
    const bool in = flow_inside(r.ni, r.nj, i + di, j + dj);
    on[k - 1] = r.out_old[in ? c + (long)dj * r.ni + di : c];
  }
  const float st = r.storage[c];
  const float width = r.width[c];
  const float length = r.length[c];
  const float conv = r.conv[c];
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
  for (int k = 1; k <= 8; k++) {
    const bool take = ((m >> (k - 1)) & 1u) && flow_inside(r.ni, r.nj, i + flow_di(k), j + flow_dj(k));
    const float qk = q + on[k - 1];
    q = take ? qk : q;
  }
  const float sv = st + v;
  const float s1 = sv + q;
  float o = 0.f, h = 0.f, cr = 0.f;
  bool capped = false;
  if (s1 > 0.f && conv > 0.f) {                                    // a NaN s1 does not enter
    const float wl = width * length;
    h = s1 / wl;
    const float a = width * h;
    const float h2 = h + h;
    const float p = width + h2;
    const float R = a / p;
    const float r23 = libm::powf_(R, kTwoThirds);
    const float vel = conv * r23;
    const float qa = vel * a;
    const float od = qa * r.dt;
    capped = !(od < s1);
    o = capped ? s1 : od;
    const float vd = vel * r.dt;
    cr = vd / length;
  }
  r.storage[c] = s1 - o;
  r.out_new[c] = o;
  if (r.depth) r.depth[c] = h;
  rep.cr_bits = (cr > 0.f || cr != cr) ? libm::asuint(cr) : 0u;
  rep.capped = capped ? 1u : 0u;
  return rep;
}

}  // namespace nmp
