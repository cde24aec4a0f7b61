// TEST INFRASTRUCTURE: the met group of the forcing regrid (noahmp_amd/csrc/nmp_dev_regrid.hpp::regrid_met and the per-column functions
// in front of it) compiled for the host, applied to whole arrays.  tests/test_regrid_met.py builds this file on demand (-ffp-contract=off,
// like the engine) and compares with numpy + glibc.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "nmp_dev_regrid.hpp"

extern "C" {

// dst_*[c] <- the met group of noahmp_hip_forcing_regrid_met, composed of the per-column functions exactly as the kernel composes them.
// src[0..3] = t, p, q, lw planes (src[3] may be NULL: no longwave, dst[3] is not touched); reads[0..3] (each may be NULL) count how often
// each source cell of that plane was read: a corner of weight zero must not be.
void regrid_met_values(const int32_t* plan, long ncell, const noahmp_regrid_source* g, const float* const* src, float* const* dst,
                       const float* dz, float lapse, float fill, int32_t* const* reads) {
  const int nxny = g->nx * g->ny;
  const int nsrc = src[3] ? 4 : 3;
  for (long c = 0; c < ncell; c++) {
    float w[4];
    int idx[4];
    for (int q = 0; q < 4; q++) memcpy(&w[q], &plan[(2 + q) * ncell + c], 4);
    if (!nmp::regrid_corners(plan[c], w, g->nx, nxny, g->periodic_x ? 1 : 0, idx)) {
      for (int f = 0; f < nsrc; f++) dst[f][c] = fill;
      continue;
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < nsrc; f++) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < 4; q++)
        if (w[q] != 0.f) { s[q] = src[f][idx[q]]; if (reads && reads[f]) reads[f][idx[q]]++; }
      v[f] = nmp::regrid_bilinear(w, s);
    }
    const nmp::RegridMet r = nmp::regrid_met(v[0], v[1], v[2], v[3], dz[c], lapse, nsrc == 4);
    dst[0][c] = r.t; dst[1][c] = r.p; dst[2][c] = r.q;
    if (nsrc == 4) dst[3][c] = r.lw;
  }
}

// the chain alone over arrays of already regridded values (the float64 agreement and property tests)
void regrid_met_chain(long n, const float* tc, const float* pc, const float* qc, const float* lc, const float* dz, float lapse,
                      float* tf, float* pf, float* qf, float* lf) {
  for (long c = 0; c < n; c++) {
    const nmp::RegridMet r = nmp::regrid_met(tc[c], pc[c], qc[c], lc ? lc[c] : 0.f, dz[c], lapse, lc != nullptr);
    tf[c] = r.t; pf[c] = r.p; qf[c] = r.q;
    if (lc) lf[c] = r.lw;
  }
}

}  // extern "C"
