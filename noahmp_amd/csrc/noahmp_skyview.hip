// Sky-view factor of the radiation forcing (no reference counterpart; the contract is the text in include/noahmp_hip.h, the arithmetic is
// nmp_dev_skyview.hpp).
//
// noahmp_hip_skyview: ONE launch per call, once per terrain; noahmp_hip_forcing_radiation_sky (noahmp_shortwave.hip) reads the plane it
// writes at every step.  One thread per window cell in row-major order, the direction loop outside the step loop: the lanes of a wave are
// neighbours along i and march the SAME direction, so at step k an x-major wave reads one or two row segments shifted by k, a y-major wave
// one or two row segments of row j +- k -- coalesced either way.  What a direction fixes (major axis, sign, t, L2) is made once per
// direction on the host with the functions of nmp_dev_skyview.hpp (IEEE float32 operations: the same bits on either side) and rides in the
// kernel arguments, 16 bytes per direction, read from scalar registers.  No LDS, no barrier, no atomics, no scratch.  Arguments go by
// value, nothing is allocated, nothing waits on the host.
//
// Steps in flight.  Unlike the shadow march no step's heights decide whether the next step runs, so sky_scan<NF> prepares NF steps and
// requests their heights before the first slope is made, and nothing of that is wasted before the window's edge.  The registers allow it
// (gfx950, the compiler's own figures: 24 / 29 / 37 VGPRs with 1 / 2 / 4 steps, no scratch, 8 waves per SIMD each) and the measurement
// chose four (tools/skyview_bench.py with the three forms as libraries of their own, medians, 7 077 888 cells / the 884 736-cell tile,
// nstep 25, ndir 16): 3.31 / 0.482 ms with one step, 3.17 / 0.463 with two, 3.10 / 0.450 with four -- 6 to 7 % for four over one, five
// inter-quartile ranges of the run; 2 to 3 % over two (profiles/skyview_bench.md).  -DNMP_SKYVIEW_INFLIGHT=1 or 2 builds the others; every form gives the
// same bits.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_skyview.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d;

#ifndef NMP_SKYVIEW_INFLIGHT
#define NMP_SKYVIEW_INFLIGHT 4
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kInFlight = NMP_SKYVIEW_INFLIGHT;
constexpr int kMaxDir = NOAHMP_SKYVIEW_MAX_NDIR;

struct SkyKArgs {                        // by value (about 1 KB)
  const float* height;
  const int* dst_index;
  float* svf;
  long ncell, ndst;
  int ni, nj, nstep, ndir;
  SkyDir dirs[kMaxDir];
};

__global__ void __launch_bounds__(kBlock) noahmp_skyview_kernel(const SkyKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const long d = k.dst_index ? (long)k.dst_index[c] : c;
  if (d < 0 || d >= k.ndst) return;                              // a margin cell: read by others, neither scanned nor written
  const int j = (int)(c / k.ni), i = (int)(c - (long)j * k.ni);
  k.svf[d] = sky_cell<kInFlight>(k.height, k.ni, k.nj, i, j, k.nstep, k.ndir, k.dirs);
}

}  // namespace

extern "C" {

int noahmp_hip_skyview(const noahmp_skyview* sv, int64_t ndst, void* stream) {
  static const char* who = "noahmp_hip_skyview";
  if (!sv) return refuse(-105, "%s: the argument block is NULL", who);
  if (!sv->height || !sv->svf || !sv->dir_x || !sv->dir_y) return refuse(-105, "%s: height, svf, dir_x and dir_y are required", who);
  if (bad_window(sv->ni, sv->nj)) return refuse(-105, "%s: window: ni, nj >= 0 and ni*nj <= 2^31 - 1", who);
  if (sv->nstep < 1 || sv->nstep > NOAHMP_SHADOW_MAX_NSTEP)
    return refuse(-105, "%s: nstep %d (1 .. %d cells)", who, sv->nstep, NOAHMP_SHADOW_MAX_NSTEP);
  if (sv->ndir < 1 || sv->ndir > kMaxDir) return refuse(-105, "%s: ndir %d (1 .. %d directions)", who, sv->ndir, kMaxDir);
  if (bad_spacing(sv->dx, sv->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", who);
  if (bad_count(ndst)) return refuse(-105, "%s: ndst: 0 .. 2^31 - 1", who);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const long ncell = (long)sv->ni * sv->nj;
  if (ndst == 0 || ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  SkyKArgs k;
  memset(&k, 0, sizeof(k));
  k.height = sv->height; k.dst_index = sv->dst_index; k.svf = sv->svf; k.ncell = ncell; k.ndst = ndst;
  k.ni = sv->ni; k.nj = sv->nj; k.nstep = sv->nstep; k.ndir = sv->ndir;
  for (int q = 0; q < sv->ndir; q++) k.dirs[q] = sky_dir(sv->dir_x[q], sv->dir_y[q], sv->dx, sv->dy);
  hipLaunchKernelGGL(noahmp_skyview_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
