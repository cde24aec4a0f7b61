// TEST INFRASTRUCTURE: the per-cell functions of the terrain-adjusted wind (noahmp_amd/csrc/nmp_dev_wind.hpp) compiled for the host, applied
// to whole windows and planes.  tests/test_wind.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy
// + glibc.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_wind.hpp"

extern "C" {

// noahmp_hip_wind_terrain over a window: sx, sy, curv through dst_index (untouched where a cell is not written); cosalpha / sinalpha NULL
// as in the call
void wind_terrain_cells(int ni, int nj, const float* height, const float* cosalpha, const float* sinalpha, const int32_t* dst_index, long ndst,
                        int ncurv, float dx, float dy, float* sx, float* sy, float* curv) {
  const nmp::WindTerrainParams p = nmp::wind_terrain_params(ni, nj, ncurv, cosalpha ? 1 : 0, dx, dy);
  for (int j = 0; j < nj; j++)
    for (int i = 0; i < ni; i++) {
      const long c = (long)j * ni + i;
      const long d = dst_index ? (long)dst_index[c] : c;
      if (d < 0 || d >= ndst) continue;
      const nmp::WindSlope s = nmp::wind_terrain_cell(p, height, cosalpha ? cosalpha[c] : 1.f, sinalpha ? sinalpha[c] : 0.f, i, j);
      sx[d] = s.sx; sy[d] = s.sy; curv[d] = s.curv;
    }
}

// noahmp_hip_forcing_wind over ncell columns, in place; changed[c] = 1 where the column function wrote
void wind_columns(long ncell, float* u, float* v, const float* sx, const float* sy, const float* curv, float slope_max, float curv_max,
                  float gamma_s, float gamma_c, int flags, unsigned char* changed) {
  nmp::WindParams k;
  k.ds = slope_max + slope_max; k.dc = curv_max + curv_max; k.gamma_s = gamma_s; k.gamma_c = gamma_c; k.turn = flags & 1;
  for (long c = 0; c < ncell; c++) changed[c] = nmp::wind_column(k, sx[c], sy[c], curv[c], &u[c], &v[c]) ? 1 : 0;
}

}  // extern "C"
