// Lakes on the D8 network (noahmp_hip_lake_take / noahmp_hip_lake_release): the per-item functions.  __host__ __device__ like
// nmp_dev_channel.hpp: tests/host_emul/lakes_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them: the contract is the text in include/noahmp_hip.h, every rounding included.  Lake water is kept
// in INTEGER QUANTA of a power-of-two volume q: taking the whole quanta out of a float32 cell and putting n*q back into a float32 cell is
// exact, and the sum over the members of a lake is an integer sum -- the same words in every order, padding, schedule and decomposition.
// The level-pool release is float64, every line one rounded operation of the text, nothing may contract into an FMA.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#endif

namespace nmp {

#ifndef NMP_DEV
#define NMP_DEV __host__ __device__ __forceinline__
#endif

constexpr double kLakeCap = 0x1p62;                                // a count of quanta at or above it is not taken / is clamped to it
constexpr long long kLakeCapWords = 1LL << 62;
constexpr double kLakeTwoG = 19.6133;                              // 2 g of the orifice [m s^-2]

struct LakeTakeArgs {
  const int32_t* member_cell; const int32_t* member_lake;
  float* storage;
  long long* inflow;
  long long nmember, ncell;
  double q, invq;                                                  // q a power of two: invq = 1/q is exact
  float qf;                                                        // (float)q, exact
  int nlake;
};

// what an entry gives to its lake: lake < 0 where the entry is skipped by the pad rule (or lies past the list)
struct LakeTaken {
  int lake;
  long long n;
};

// One entry of noahmp_hip_lake_take: the whole quanta leave storage[c]; the caller adds n to inflow[lake].
NMP_DEV LakeTaken lake_take_entry(const LakeTakeArgs& t, long long e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  LakeTaken r;
  r.lake = -1; r.n = 0;
  if (e >= t.nmember) return r;
  const long long c = (long long)t.member_cell[e];
  const int l = (int)t.member_lake[e];
  if (c < 0 || c >= t.ncell || l < 0 || l >= t.nlake) return r;    // the pad value rule
  r.lake = l;
  const float s = t.storage[c];
  if (!(s >= t.qf)) return r;                                      // NaN, negative, less than a quantum: stay in the cell
  const double sd = (double)s;
  const double tq = sd * t.invq;
  if (!(tq < kLakeCap)) return r;                                  // Inf and absurd values stay and stay visible
  const long long n = (long long)floor(tq);
  const double nq = (double)n * t.q;
  const double rem = sd - nq;
  t.storage[c] = (float)rem;
  r.n = n;
  return r;
}

struct LakeReleaseArgs {
  long long* volume; long long* inflow;
  const double* area; const double* weir_h; const double* weir_c; const double* weir_l;
  const double* orifice_h; const double* orifice_c; const double* orifice_a;
  const int32_t* outlet_cell;
  float* out_new;
  double* level;                                                   // or NULL
  float* outflow;                                                  // or NULL
  long long ncell;
  double q, invq, dt;
  int nlake;
};

// One lake of noahmp_hip_lake_release; returns 1 where the lake released all it held.
NMP_DEV uint32_t lake_release_one(const LakeReleaseArgs& r, int l) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long long v0 = (long long)((unsigned long long)r.volume[l] + (unsigned long long)r.inflow[l]);
  r.inflow[l] = 0;
  const double area = r.area[l];
  const double vol = (double)v0 * r.q;
  const double hq = vol / area;
  const double h = (area > 0.0) ? hq : 0.0;
  const double hw = h - r.weir_h[l];
  double qw = 0.0;
  if (hw > 0.0) {
    const double rt = sqrt(hw);
    const double a = r.weir_c[l] * r.weir_l[l];
    const double b = a * hw;
    qw = b * rt;
  }
  const double ho = h - r.orifice_h[l];
  double qo = 0.0;
  if (ho > 0.0) {
    const double g = kLakeTwoG * ho;
    const double rt = sqrt(g);
    const double a = r.orifice_c[l] * r.orifice_a[l];
    qo = a * rt;
  }
  const double qt = qw + qo;
  const double od = qt * r.dt;
  const double t = od * r.invq;
  long long n = 0;
  if (t >= 1.0) n = (t < kLakeCap) ? (long long)floor(t) : kLakeCapWords;      // a NaN gives 0
  if (v0 <= 0) n = 0;
  else if (n > v0) n = v0;
  const uint32_t emptied = (n > 0 && n == v0) ? 1u : 0u;
  if (n >= (1LL << 24)) {                                          // 24 significant bits: n*q is a float32 value; what is cut stays
    const int sh = (64 - __builtin_clzll((unsigned long long)n)) - 24;
    n = (n >> sh) << sh;
  }
  r.volume[l] = v0 - n;
  const double oq = (double)n * r.q;
  const float o = (float)oq;
  const long long oc = (long long)r.outlet_cell[l];
  if (oc >= 0 && oc < r.ncell) r.out_new[oc] = o;
  if (r.level) r.level[l] = h;
  if (r.outflow) r.outflow[l] = o;
  return emptied;
}

struct LakeDepthArgs {
  const int32_t* member_cell; const int32_t* member_lake;
  const long long* volume;
  const double* area; const double* datum;
  const float* bed;
  float* depth;
  long long nmember, ncell;
  double q;
  int nlake;
};

// One entry of noahmp_hip_lake_depth: the lake's surface above the member's bed goes into the depth plane of the diffusive routing call,
// 0 where the bed stands above the surface.  The pad rule is the take's.
NMP_DEV void lake_depth_entry(const LakeDepthArgs& t, long long e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (e >= t.nmember) return;
  const long long c = (long long)t.member_cell[e];
  const int l = (int)t.member_lake[e];
  if (c < 0 || c >= t.ncell || l < 0 || l >= t.nlake) return;      // the pad value rule
  const double area = t.area[l];
  const double vol = (double)t.volume[l] * t.q;
  const double hq = vol / area;
  const double h = (area > 0.0) ? hq : 0.0;
  const double el = t.datum[l] + h;
  const double d = el - (double)t.bed[c];
  t.depth[c] = (d > 0.0) ? (float)d : 0.f;
}

}  // namespace nmp
