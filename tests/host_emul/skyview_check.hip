// TEST INFRASTRUCTURE: the per-cell functions of the horizon scan (noahmp_amd/csrc/nmp_dev_skyview.hpp) and the sky column of the
// radiation step (nmp_dev_shortwave.hpp) compiled for the host, applied to whole windows.  tests/test_skyview.py builds this file on
// demand (-ffp-contract=off, like the engine) and compares with numpy + glibc.  NF: the number of steps whose heights are read before the
// first slope is made, as the kernel does it; every NF gives the same result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "nmp_dev_skyview.hpp"

namespace {

template <int NF>
void scan_window(int ni, int nj, const float* height, const int32_t* dst_index, long ndst, int nstep, int ndir, const nmp::SkyDir* dirs,
                 float* smax, float* svf) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const long c = (long)j * ni + i;
      const long d = dst_index ? (long)dst_index[c] : c;
      if (d < 0 || d >= ndst) continue;
      const float z0 = height[c];
      for (int q = 0; q < ndir; q++) smax[(long)q * ni * nj + c] = nmp::sky_scan<NF>(height, ni, nj, i, j, z0, dirs[q], nstep);
      svf[d] = nmp::sky_cell<NF>(height, ni, nj, i, j, nstep, ndir, dirs);
    }
}

}  // namespace

extern "C" {

// noahmp_hip_skyview over a window: smax (ndir planes in WINDOW order, untouched where a cell is not scanned) and svf through dst_index
void skyview_cells(int ni, int nj, const float* height, const int32_t* dst_index, long ndst, int nstep, int ndir, const float* dir_x,
                   const float* dir_y, float dx, float dy, int nf, float* smax, float* svf) {
  nmp::SkyDir dirs[64];
  for (int q = 0; q < ndir; q++) dirs[q] = nmp::sky_dir(dir_x[q], dir_y[q], dx, dy);
  if (nf == 1) scan_window<1>(ni, nj, height, dst_index, ndst, nstep, ndir, dirs, smax, svf);
  else if (nf == 2) scan_window<2>(ni, nj, height, dst_index, ndst, nstep, ndir, dirs, smax, svf);
  else scan_window<4>(ni, nj, height, dst_index, ndst, nstep, ndir, dirs, smax, svf);
}

// noahmp_hip_forcing_radiation_sky: as shadow_lit_values of shadow_check.hip, with the planes of noahmp_sky (NULL as in the call); sky holds
// albedo_const, emiss_const, sigma
void skyview_radiation_values(long ncell, const float* svf, const float* lit, const float* albedo, float* glw, const float* tsurf,
                              const float* emiss, const float* sky, const float* sw_a, const float* sw_b, const float* mean_a, const float* lat,
                              const float* lon, const float* ne, const float* nn, const float* nu, int mode, float fraction, float one_minus,
                              float hour_utc, float sin_declin, float cos_declin, const float* par, float* swdown) {
  nmp::SwParams k;
  memset(&k, 0, sizeof(k));
  k.now.hour_utc = hour_utc; k.now.sin_declin = sin_declin; k.now.cos_declin = cos_declin;
  k.fraction = fraction; k.one_minus = one_minus;
  k.max_ratio = par[0]; k.mu_min = par[1]; k.max_terrain_ratio = par[2]; k.solar_constant = par[3];
  k.mode = mode; k.has_b = (mode == NOAHMP_SW_LINEAR && sw_b) ? 1 : 0; k.has_normal = ne ? 1 : 0;
  for (long c = 0; c < ncell; c++) {
    swdown[c] = nmp::sw_column_sky(k, svf[c], lit ? lit[c] : 1.0f, albedo ? albedo[c] : sky[0], sw_a[c], k.has_b ? sw_b[c] : 0.f,
                                   mean_a ? mean_a[c] : 0.f, lat[c], lon[c], ne ? ne[c] : 0.f, nn ? nn[c] : 0.f, nu ? nu[c] : 0.f);
    if (glw) glw[c] = nmp::lw_column_sky(svf[c], glw[c], tsurf[c], emiss ? emiss[c] : sky[1], sky[2]);
  }
}

}  // extern "C"
