// TEST INFRASTRUCTURE: the per-cell functions of the forcing regrid (noahmp_amd/csrc/nmp_dev_regrid.hpp) compiled for the host, applied
// to whole arrays.  tests/test_regrid.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "nmp_dev_regrid.hpp"

extern "C" {

// plan[k*ncell + c] <- plane k (base, near, w0..w3 as bits) of target cell c; returns the number of cells with base < 0
long regrid_plan(const float* xlat, const float* xlon, long ncell, const noahmp_regrid_source* g, const unsigned char* valid, int radius,
                 int32_t* plan) {
  long unfilled = 0;
  for (long c = 0; c < ncell; c++) {
    const nmp::RegridCell r = nmp::regrid_plan_cell(xlat[c], xlon[c], g->nx, g->ny, g->lon0, g->lat0, g->dlon, g->dlat, g->periodic_x ? 1 : 0,
                                                    valid, radius);
    plan[c] = r.base;
    plan[ncell + c] = r.near;
    for (int q = 0; q < 4; q++) memcpy(&plan[(2 + q) * ncell + c], &r.w[q], 4);
    if (r.base < 0) unfilled++;
  }
  return unfilled;
}

// dst[c] <- one entry of noahmp_hip_forcing_regrid, composed of the per-column functions exactly as the kernel composes them.  `reads`
// (may be NULL) counts how often each source cell was read: a corner of weight zero must not be.
void regrid_values(const int32_t* plan, long ncell, const noahmp_regrid_source* g, const float* src, float* dst, const float* adjust,
                   float scale, float fill, int mode, int32_t* reads) {
  const int nxny = g->nx * g->ny;
  for (long c = 0; c < ncell; c++) {
    float w[4], s[4] = {0.f, 0.f, 0.f, 0.f}, v;
    for (int q = 0; q < 4; q++) memcpy(&w[q], &plan[(2 + q) * ncell + c], 4);
    if (mode == NOAHMP_REGRID_BILINEAR) {
      int idx[4];
      if (!nmp::regrid_corners(plan[c], w, g->nx, nxny, g->periodic_x ? 1 : 0, idx)) { dst[c] = fill; continue; }
      for (int q = 0; q < 4; q++)
        if (w[q] != 0.f) { s[q] = src[idx[q]]; if (reads) reads[idx[q]]++; }
      v = nmp::regrid_bilinear(w, s);
    } else {
      const int nr = plan[ncell + c];
      if (!nmp::regrid_near_ok(nr, nxny)) { dst[c] = fill; continue; }
      v = src[nr];
      if (reads) reads[nr]++;
    }
    dst[c] = adjust ? nmp::regrid_adjust(v, scale, adjust[c]) : v;
  }
}

}  // extern "C"
