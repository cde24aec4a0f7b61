// Cast shadows of the shortwave forcing (no reference counterpart; the contract is the text in include/noahmp_hip.h, the arithmetic is
// nmp_dev_shadow.hpp).
//
// noahmp_hip_forcing_shadow: ONE launch per call, before noahmp_hip_forcing_shortwave_lit, which reads the plane it writes.  One thread per
// window cell in row-major order: the lanes of a wave are neighbours along i and march nearly parallel rays, so at step k an x-major wave
// reads one or two row segments shifted by k, a y-major wave one or two row segments of row j +- k -- coalesced either way, and the rows a
// workgroup touches are shared with its neighbours through the L2.  No LDS, no barrier, no atomics.  A lane leaves at its first ending
// step, a wave when its last lane has left; where the sun is below mu_min the wave leaves right after the sun is made.  Arguments go by
// value, nothing is allocated, nothing waits on the host.
//
// Steps in flight.  The loads of a step do not depend on the outcome of the step before, so shadow_march<NF> can prepare NF steps and
// request their (up to two) heights each before the first compare; the result stays that of the first step, in order, that ends the march.
// The registers allowed it (gfx950, the compiler's own figures: 34 / 34 / 46 VGPRs with 1 / 2 / 4 steps, no scratch, 8 waves per SIMD
// each), the measurement did not (tools/shadow_bench.py with the three forms as libraries of their own, medians, 7 077 888 cells / the
// 884 736-cell tile, nstep 25): at mu ~ 0.10, the worst case, 0.176 / 0.0284 ms with one step, 0.199 / 0.0318 with two, 0.194 / 0.0308 with
// four; at mu ~ 0.5 0.0693 / 0.0123, 0.0725 / 0.0128, 0.0709 / 0.0126.  Eight waves per SIMD already hide the latency of heights that
// mostly come from the L2, and a group pays the address work and the loads of the steps behind the one that ends the march.  One step it is;
// -DNMP_SHADOW_INFLIGHT=2 or 4 builds the others.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_shadow.hpp"
#include "nmp_engine_host.hpp"
#include "nmp_forcing_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d,
    nmp_host::sun_of;

#ifndef NMP_SHADOW_INFLIGHT
#define NMP_SHADOW_INFLIGHT 1
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kInFlight = NMP_SHADOW_INFLIGHT;
constexpr int kMaxStep = 4096;

struct ShadowKArgs {
  const float* height; const float* xlat; const float* lon;
  const float* cosalpha; const float* sinalpha;
  const int* dst_index;
  float* lit;
  long ncell, ndst;
  ShadowParams p;
};

__global__ void __launch_bounds__(kBlock) noahmp_shadow_kernel(const ShadowKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const long d = k.dst_index ? (long)k.dst_index[c] : c;
  if (d < 0 || d >= k.ndst) return;                              // a margin cell: read by others, neither marched nor written
  const float lat = k.xlat[c], lon = k.lon[c];
  float ca = 1.f, sa = 0.f;
  if (k.p.has_rot) { ca = k.cosalpha[c]; sa = k.sinalpha[c]; }
  const int j = (int)(c / k.p.ni), i = (int)(c - (long)j * k.p.ni);
  k.lit[d] = shadow_lit(shadow_cell<kInFlight>(k.p, k.height, lat, lon, ca, sa, i, j));
}

}  // namespace

extern "C" {

int noahmp_hip_forcing_shadow(const noahmp_shadow* sh, int64_t ndst, const noahmp_sun_time* now, void* stream) {
  static const char* who = "noahmp_hip_forcing_shadow";
  if (!sh) return refuse(-105, "%s: the argument block is NULL", who);
  if (!now) return refuse(-105, "%s: now is NULL", who);
  if (!sh->height || !sh->xlat || !sh->lon || !sh->lit) return refuse(-105, "%s: height, xlat, lon and lit are required", who);
  if ((sh->cosalpha != nullptr) != (sh->sinalpha != nullptr)) return refuse(-105, "%s: cosalpha and sinalpha go together: both or none", who);
  if (bad_window(sh->ni, sh->nj)) return refuse(-105, "%s: window: ni, nj >= 0 and ni*nj <= 2^31 - 1", who);
  if (sh->nstep < 1 || sh->nstep > kMaxStep) return refuse(-105, "%s: nstep %d (1 .. %d cells)", who, sh->nstep, kMaxStep);
  if (bad_spacing(sh->dx, sh->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", who);
  if (bad_count(ndst)) return refuse(-105, "%s: ndst: 0 .. 2^31 - 1", who);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const long ncell = (long)sh->ni * sh->nj;
  if (ndst == 0 || ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  ShadowKArgs k;
  memset(&k, 0, sizeof(k));
  k.height = sh->height; k.xlat = sh->xlat; k.lon = sh->lon; k.cosalpha = sh->cosalpha; k.sinalpha = sh->sinalpha;
  k.dst_index = sh->dst_index; k.lit = sh->lit; k.ncell = ncell; k.ndst = ndst;
  k.p.now = sun_of(*now);
  k.p.ni = sh->ni; k.p.nj = sh->nj; k.p.nstep = sh->nstep; k.p.has_rot = sh->cosalpha ? 1 : 0;
  k.p.dx = sh->dx; k.p.dy = sh->dy; k.p.mu_min = sh->mu_min; k.p.height_max = sh->height_max;
  hipLaunchKernelGGL(noahmp_shadow_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
