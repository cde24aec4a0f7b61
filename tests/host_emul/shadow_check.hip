// TEST INFRASTRUCTURE: the per-cell functions of the cast-shadow march (noahmp_amd/csrc/nmp_dev_shadow.hpp) and the lit column of the
// shortwave step (nmp_dev_shortwave.hpp) compiled for the host, applied to whole windows.  tests/test_shadow.py builds this file on
// demand (-ffp-contract=off, like the engine) and compares with numpy + glibc.  The sun of a time (hour_utc, sin_declin, cos_declin)
// comes in as numbers: making it is host code of the library.  NF: the number of steps whose heights are read before the first compare,
// as the kernel does it; every NF gives the same result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "nmp_dev_shadow.hpp"

namespace {

template <int NF>
int march_dir(const float* height, int ni, int nj, int i, int j, float gx, float gy, float u, float dx, float dy, int nstep, float height_max) {
  const nmp::ShadowRay r = nmp::shadow_ray(gx, gy, u, dx, dy);
  return nmp::shadow_march<NF>(height, ni, nj, i, j, r, nstep, height_max);
}

}  // namespace

extern "C" {

// the march of every window cell from a direction given per cell: exit = how it ended (nmp::ShadowExit), lit = the plane
void shadow_march_dir(int ni, int nj, const float* height, const float* gx, const float* gy, const float* u, float dx, float dy, int nstep,
                      float height_max, int nf, int32_t* exit, float* lit) {
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const long c = (long)j * ni + i;
      int e;
      if (nf == 1) e = march_dir<1>(height, ni, nj, i, j, gx[c], gy[c], u[c], dx, dy, nstep, height_max);
      else if (nf == 2) e = march_dir<2>(height, ni, nj, i, j, gx[c], gy[c], u[c], dx, dy, nstep, height_max);
      else e = march_dir<4>(height, ni, nj, i, j, gx[c], gy[c], u[c], dx, dy, nstep, height_max);
      exit[c] = e;
      lit[c] = nmp::shadow_lit(e);
    }
}

// noahmp_hip_forcing_shadow over a window: cosalpha / sinalpha and dst_index may be NULL as in the call; cells whose dst_index is
// negative or >= ndst are neither marched nor written.  exit is in WINDOW order (-1 where not marched), lit through dst_index.
void shadow_cells(int ni, int nj, const float* height, const float* lat, const float* lon, const float* cosalpha, const float* sinalpha,
                  const int32_t* dst_index, long ndst, float hour_utc, float sin_declin, float cos_declin, float dx, float dy, int nstep,
                  float mu_min, float height_max, int32_t* exit, float* lit) {
  nmp::ShadowParams p;
  memset(&p, 0, sizeof(p));
  p.now.hour_utc = hour_utc; p.now.sin_declin = sin_declin; p.now.cos_declin = cos_declin;
  p.ni = ni; p.nj = nj; p.nstep = nstep; p.has_rot = cosalpha ? 1 : 0;
  p.dx = dx; p.dy = dy; p.mu_min = mu_min; p.height_max = height_max;
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const long c = (long)j * ni + i;
      const long d = dst_index ? (long)dst_index[c] : c;
      exit[c] = -1;
      if (d < 0 || d >= ndst) continue;
      const int e = nmp::shadow_cell<1>(p, height, lat[c], lon[c], cosalpha ? cosalpha[c] : 1.f, sinalpha ? sinalpha[c] : 0.f, i, j);
      exit[c] = e;
      lit[d] = nmp::shadow_lit(e);
    }
}

// noahmp_hip_forcing_shortwave_lit: as shortwave_values of shortwave_check.hip, with the lit plane
void shadow_lit_values(long ncell, const float* lit, const float* sw_a, const float* sw_b, const float* mean_a, const float* lat,
                       const float* lon, const float* ne, const float* nn, const float* nu, int mode, float fraction, float one_minus,
                       float hour_utc, float sin_declin, float cos_declin, const float* par, float* swdown) {
  nmp::SwParams k;
  memset(&k, 0, sizeof(k));
  k.now.hour_utc = hour_utc; k.now.sin_declin = sin_declin; k.now.cos_declin = cos_declin;
  k.fraction = fraction; k.one_minus = one_minus;
  k.max_ratio = par[0]; k.mu_min = par[1]; k.max_terrain_ratio = par[2]; k.solar_constant = par[3];
  k.mode = mode; k.has_b = (mode == NOAHMP_SW_LINEAR && sw_b) ? 1 : 0; k.has_normal = ne ? 1 : 0;
  for (long c = 0; c < ncell; c++)
    swdown[c] = nmp::sw_column_lit(k, lit[c], sw_a[c], k.has_b ? sw_b[c] : 0.f, mean_a ? mean_a[c] : 0.f, lat[c], lon[c], ne ? ne[c] : 0.f,
                                   nn ? nn[c] : 0.f, nu ? nu[c] : 0.f);
}

}  // extern "C"
