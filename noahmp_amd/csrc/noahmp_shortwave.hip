// Shortwave forcing of a device-resident run (no reference counterpart: the reference interpolates SWDOWN linearly between two records,
// netcdf_io:1369-1403; the contract is the text in include/noahmp_hip.h, the arithmetic is nmp_dev_shortwave.hpp).
//
// noahmp_hip_forcing_cosz_mean: once per forcing record.  One thread per column: latitude and longitude are read once, sin / cos of the
// latitude made once, then the 1..64 sample suns -- which ride in the kernel arguments, 12 bytes each -- are walked from scalar registers.
//
// noahmp_hip_forcing_shortwave: ONE launch per step, after noahmp_hip_forcing_interpolate[_prep], whose linear SWDOWN it overwrites.  A pure
// stream of 12 (LINEAR) to 36 bytes per column.  All loads of a column are issued before the first libm call; sinf_ / cosf_ hold no table,
// so there is no LDS and no barrier.  One column per thread wherever a sun is made: see the note at the kernel.  Arguments go by value,
// nothing is allocated, nothing waits on the host.
//
// noahmp_hip_forcing_shortwave_lit: the same step with the lit plane of noahmp_hip_forcing_shadow (noahmp_shadow.hip) on the direct beam;
// a kernel of its own, so the call above keeps its kernels and its bits.
//
// noahmp_hip_forcing_radiation_sky: the lit step plus the sky-view terms of the shortwave plus the longwave of the closed part of the
// hemisphere, in ONE launch -- again a kernel of its own.  The sky-view plane is that of noahmp_hip_skyview (noahmp_skyview.hip).
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_shortwave.hpp"
#include "nmp_engine_host.hpp"
#include "nmp_forcing_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::stream_of, nmp_host::grid_1d, nmp_host::sun_of;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxSamples = NOAHMP_SW_MAX_SAMPLES;

struct MeanKArgs {                       // by value (< 1 KB)
  const float* xlat; const float* lon;
  float* mean;
  long ncell;
  int nsample;
  SunTime t[kMaxSamples];
};

__global__ void __launch_bounds__(kBlock) noahmp_cosz_mean_kernel(const MeanKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const float lat = k.xlat[c], lon = k.lon[c];
  k.mean[c] = sun_interval_mean(lat, lon, k.nsample, k.t);
}

struct SwKArgs {
  const float* sw_a; const float* sw_b; const float* mean_a;
  const float* xlat; const float* lon;
  const float* ne; const float* nn; const float* nu;
  float* swdown;
  long ncell;
  SwParams p;
};

// VEC: NOAHMP_SW_LINEAR without normals -- no sun is made, the call is a pure stream of 8 or 12 bytes per column -- with sw_a, sw_b and
// swdown 16-byte aligned and ncell a multiple of four: a thread owns four consecutive columns (16-byte loads and stores).  Every call
// that makes a sun runs one column per thread whatever the alignment.  Registers would have allowed four there too (gfx950, the
// compiler's own figures: one column 36 VGPRs, four columns 60, both without scratch and at 8 waves per SIMD), but the measurement did
// not (tools/shortwave_bench.py with both forms built in, medians, 7 077 888 columns / the 884 736-column tile): ZENITH 0.0308 / 0.0088 ms
// with four columns against 0.0337 / 0.0070 with one, ZENITH with terrain 0.0473 / 0.0117 against 0.0449 / 0.0089 -- four lose up to 31 %
// on the tile, where a quarter of the threads no longer fills the chip, and win 9 % at most; LINEAR 0.0158 / 0.0044 against 0.0195 / 0.0044.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) noahmp_shortwave_kernel(const SwKArgs k) {
  constexpr int NC = VEC ? 4 : 1;
  const long c = ((long)blockIdx.x * kBlock + threadIdx.x) * NC;
  if (c >= k.ncell) return;
  if constexpr (VEC) {
    const float4 a = *(const float4*)(k.sw_a + c);
    float4 o = a;
    if (k.p.has_b) {
      const float4 b = *(const float4*)(k.sw_b + c);
      o.x = interp2(a.x, b.x, k.p.fraction, k.p.one_minus);
      o.y = interp2(a.y, b.y, k.p.fraction, k.p.one_minus);
      o.z = interp2(a.z, b.z, k.p.fraction, k.p.one_minus);
      o.w = interp2(a.w, b.w, k.p.fraction, k.p.one_minus);
    }
    *(float4*)(k.swdown + c) = o;
  } else {
    const bool zenith = k.p.mode == NOAHMP_SW_ZENITH;
    const bool sun = zenith || k.p.has_normal;
    const float sw_a = k.sw_a[c];
    float sw_b = 0.f, mean_a = 0.f, lat = 0.f, lon = 0.f, ne = 0.f, nn = 0.f, nu = 0.f;
    if (k.p.has_b) sw_b = k.sw_b[c];
    if (zenith) mean_a = k.mean_a[c];
    if (sun) { lat = k.xlat[c]; lon = k.lon[c]; }
    if (k.p.has_normal) { ne = k.ne[c]; nn = k.nn[c]; nu = k.nu[c]; }
    __builtin_amdgcn_sched_barrier(0);   // the loads above are in flight before the first libm call
    k.swdown[c] = sw_column(k.p, sw_a, sw_b, mean_a, lat, lon, ne, nn, nu);
  }
}

// noahmp_hip_forcing_shortwave_lit: the one-column form above plus the 4 bytes of the lit plane; a sun may be needed in every column
// (a shadowed one scales its beam whatever the mode), so latitude and longitude are always loaded.
__global__ void __launch_bounds__(kBlock) noahmp_shortwave_lit_kernel(const SwKArgs k, const float* __restrict__ lit_plane) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const bool zenith = k.p.mode == NOAHMP_SW_ZENITH;
  const float lit = lit_plane[c];
  const float sw_a = k.sw_a[c];
  const float lat = k.xlat[c], lon = k.lon[c];
  float sw_b = 0.f, mean_a = 0.f, ne = 0.f, nn = 0.f, nu = 0.f;
  if (k.p.has_b) sw_b = k.sw_b[c];
  if (zenith) mean_a = k.mean_a[c];
  if (k.p.has_normal) { ne = k.ne[c]; nn = k.nn[c]; nu = k.nu[c]; }
  __builtin_amdgcn_sched_barrier(0);   // the loads above are in flight before the first libm call
  k.swdown[c] = sw_column_lit(k.p, lit, sw_a, sw_b, mean_a, lat, lon, ne, nn, nu);
}

// noahmp_hip_forcing_radiation_sky: the lit form plus 4 bytes of sky view, up to 8 of lit and albedo, and the longwave group (GLW in and
// out, surface temperature, up to 4 of emissivity).  Every load of the column is issued before the first libm call; the longwave itself
// holds no libm.  A column with an open sky (svf == 1.0f) keeps its GLW without a store.
struct SkyKArgs {
  const float* svf; const float* lit; const float* albedo; const float* tsurf; const float* emiss;
  float* glw;
  float albedo_const, emiss_const, sigma;
};

__global__ void __launch_bounds__(kBlock) noahmp_radiation_sky_kernel(const SwKArgs k, const SkyKArgs y) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const bool zenith = k.p.mode == NOAHMP_SW_ZENITH;
  const float svf = y.svf[c];
  const float sw_a = k.sw_a[c];
  const float lat = k.xlat[c], lon = k.lon[c];
  float lit = 1.0f, albedo = y.albedo_const, emiss = y.emiss_const, g = 0.f, tsurf = 0.f;
  float sw_b = 0.f, mean_a = 0.f, ne = 0.f, nn = 0.f, nu = 0.f;
  if (y.lit) lit = y.lit[c];
  if (y.albedo) albedo = y.albedo[c];
  if (k.p.has_b) sw_b = k.sw_b[c];
  if (zenith) mean_a = k.mean_a[c];
  if (k.p.has_normal) { ne = k.ne[c]; nn = k.nn[c]; nu = k.nu[c]; }
  if (y.glw) {
    g = y.glw[c]; tsurf = y.tsurf[c];
    if (y.emiss) emiss = y.emiss[c];
  }
  __builtin_amdgcn_sched_barrier(0);   // the loads above are in flight before the first libm call
  k.swdown[c] = sw_column_sky(k.p, svf, lit, albedo, sw_a, sw_b, mean_a, lat, lon, ne, nn, nu);
  if (y.glw && !(svf == 1.0f)) y.glw[c] = lw_column_sky(svf, g, tsurf, emiss, y.sigma);
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }      // NULL counts as aligned: the plane is not read

// the checks of both shortwave calls and their kernel arguments; 0, or the refusal
int sw_prepare(const char* who, const noahmp_shortwave* sw, int64_t ncell, const noahmp_sun_time* now, SwKArgs* out) {
  if (!sw) return refuse(-105, "%s: the argument block is NULL", who);
  if (!now) return refuse(-105, "%s: now is NULL", who);
  if (sw->mode != NOAHMP_SW_LINEAR && sw->mode != NOAHMP_SW_ZENITH)
    return refuse(-105, "%s: mode %d (NOAHMP_SW_LINEAR, NOAHMP_SW_ZENITH)", who, sw->mode);
  if (bad_count(ncell)) return refuse(-105, "%s: 0 .. 2^31 - 1 columns", who);
  if (!sw->sw_a || !sw->xlat || !sw->lon || !sw->swdown) return refuse(-105, "%s: sw_a, xlat, lon and swdown are required", who);
  const bool zenith = sw->mode == NOAHMP_SW_ZENITH;
  if (zenith && !sw->mean_a) return refuse(-105, "%s: NOAHMP_SW_ZENITH needs mean_a (noahmp_hip_forcing_cosz_mean)", who);
  const int nnormal = (sw->normal_e ? 1 : 0) + (sw->normal_n ? 1 : 0) + (sw->normal_u ? 1 : 0);
  if (nnormal != 0 && nnormal != 3) return refuse(-105, "%s: normal_e, normal_n and normal_u go together: all three or none", who);
  const bool has_b = !zenith && sw->sw_b;
  if (has_b && (sw->idts2 <= 0 || sw->idts < 0 || sw->idts > sw->idts2))
    return refuse(-105, "%s: target date outside the bracketing records (idts, idts2)", who);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  SwKArgs& k = *out;
  memset(&k, 0, sizeof(k));
  k.sw_a = sw->sw_a; k.sw_b = sw->sw_b; k.mean_a = sw->mean_a; k.xlat = sw->xlat; k.lon = sw->lon;
  k.ne = sw->normal_e; k.nn = sw->normal_n; k.nu = sw->normal_u; k.swdown = sw->swdown; k.ncell = ncell;
  k.p.now = sun_of(*now);
  k.p.fraction = has_b ? (float)(sw->idts2 - sw->idts) / (float)sw->idts2 : 1.0f;      // netcdf_io:1390
  k.p.one_minus = 1.0f - k.p.fraction;
  k.p.max_ratio = sw->max_ratio; k.p.mu_min = sw->mu_min; k.p.max_terrain_ratio = sw->max_terrain_ratio;
  k.p.solar_constant = sw->solar_constant;
  k.p.mode = sw->mode; k.p.has_b = has_b ? 1 : 0; k.p.has_normal = nnormal == 3 ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" {

int noahmp_hip_forcing_cosz_mean(const float* xlat, const float* lon, int64_t ncell, int nsample, const noahmp_sun_time* times, float* mean,
                                 void* stream) {
  static const char* who = "noahmp_hip_forcing_cosz_mean";
  if (nsample < 1 || nsample > kMaxSamples) return refuse(-107, "%s: 1..%d samples per interval (nsample = %d)", who, kMaxSamples, nsample);
  if (!times) return refuse(-105, "%s: times is NULL", who);
  if (bad_count(ncell)) return refuse(-105, "%s: 0 .. 2^31 - 1 columns", who);
  if (!xlat || !lon || !mean) return refuse(-105, "%s: xlat, lon and mean are required", who);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  MeanKArgs k;
  memset(&k, 0, sizeof(k));
  k.xlat = xlat; k.lon = lon; k.mean = mean; k.ncell = ncell; k.nsample = nsample;
  for (int i = 0; i < nsample; i++) k.t[i] = sun_of(times[i]);
  hipLaunchKernelGGL(noahmp_cosz_mean_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_forcing_shortwave(const noahmp_shortwave* sw, int64_t ncell, const noahmp_sun_time* now, void* stream) {
  static const char* who = "noahmp_hip_forcing_shortwave";
  SwKArgs k;
  int rc = sw_prepare(who, sw, ncell, now, &k);
  if (rc) return rc;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  const bool zenith = k.p.mode == NOAHMP_SW_ZENITH;
  const bool vec = !zenith && !k.p.has_normal && (ncell & 3) == 0 && aligned16(k.sw_a) && aligned16(k.p.has_b ? k.sw_b : nullptr) && aligned16(k.swdown);
  const long nthread = vec ? ncell / 4 : ncell;
  const dim3 grid = grid_1d(nthread, kBlock);
  if (vec) hipLaunchKernelGGL(noahmp_shortwave_kernel<true>, grid, dim3(kBlock), 0, s, k);
  else hipLaunchKernelGGL(noahmp_shortwave_kernel<false>, grid, dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_forcing_shortwave_lit(const noahmp_shortwave* sw, const float* lit, int64_t ncell, const noahmp_sun_time* now, void* stream) {
  static const char* who = "noahmp_hip_forcing_shortwave_lit";
  if (!lit) return refuse(-105, "%s: lit is NULL (noahmp_hip_forcing_shadow makes it)", who);
  SwKArgs k;
  int rc = sw_prepare(who, sw, ncell, now, &k);
  if (rc) return rc;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  hipLaunchKernelGGL(noahmp_shortwave_lit_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k, lit);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_forcing_radiation_sky(const noahmp_shortwave* sw, const noahmp_sky* sky, int64_t ncell, const noahmp_sun_time* now, void* stream) {
  static const char* who = "noahmp_hip_forcing_radiation_sky";
  if (!sky) return refuse(-105, "%s: the sky block is NULL", who);
  if (!sky->svf) return refuse(-105, "%s: svf is NULL (noahmp_hip_skyview makes it)", who);
  if (sky->glw && !sky->tsurf) return refuse(-105, "%s: glw needs tsurf", who);
  SwKArgs k;
  int rc = sw_prepare(who, sw, ncell, now, &k);
  if (rc) return rc;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  SkyKArgs y;
  memset(&y, 0, sizeof(y));
  y.svf = sky->svf; y.lit = sky->lit; y.albedo = sky->albedo; y.glw = sky->glw; y.tsurf = sky->tsurf; y.emiss = sky->emiss;
  y.albedo_const = sky->albedo_const; y.emiss_const = sky->emiss_const; y.sigma = sky->sigma;
  hipLaunchKernelGGL(noahmp_radiation_sky_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k, y);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
