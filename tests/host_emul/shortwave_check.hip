// TEST INFRASTRUCTURE: the per-column functions of the shortwave forcing (noahmp_amd/csrc/nmp_dev_shortwave.hpp) compiled for the host,
// applied to whole arrays.  tests/test_shortwave.py builds this file on demand (-ffp-contract=off, like the engine) and compares with
// numpy + glibc.  The sun of a time (hour_utc, sin_declin, cos_declin) comes in as numbers: making it is host code of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "nmp_dev_shortwave.hpp"

extern "C" {

// (e, n, u) of every column at one time, composed as the kernels compose it
void shortwave_sun(long ncell, const float* lat, const float* lon, float hour_utc, float sin_declin, float cos_declin, float* e, float* n,
                   float* u, float* u_alone) {
  for (long c = 0; c < ncell; c++) {
    const float phi = lat[c] * nmp::NMP_DEGRAD;
    const float sinphi = nmp::libm::sinf_(phi), cosphi = nmp::libm::cosf_(phi);
    const float h = nmp::sun_hrang(lon[c], hour_utc);
    const nmp::SunVec v = nmp::sun_vector(sinphi, cosphi, h, sin_declin, cos_declin);
    e[c] = v.e; n[c] = v.n; u[c] = v.u;
    u_alone[c] = nmp::sun_up(sinphi, cosphi, h, sin_declin, cos_declin);
  }
}

// forcing_cosz itself (nmp_dev_forcing.hpp), what noahmp_hip_forcing_prep writes to COSZIN
void shortwave_forcing_cosz(long ncell, const float* lat, const float* lon, float hour_utc, float sin_declin, float cos_declin, float* cosz) {
  for (long c = 0; c < ncell; c++) cosz[c] = nmp::forcing_cosz(lat[c], lon[c], hour_utc, sin_declin, cos_declin);
}

// noahmp_hip_forcing_cosz_mean: suns = nsample x (hour_utc, sin_declin, cos_declin)
void shortwave_mean(long ncell, const float* lat, const float* lon, int nsample, const float* suns, float* mean) {
  nmp::SunTime t[NOAHMP_SW_MAX_SAMPLES];
  for (int s = 0; s < nsample; s++) { t[s].hour_utc = suns[3 * s]; t[s].sin_declin = suns[3 * s + 1]; t[s].cos_declin = suns[3 * s + 2]; }
  for (long c = 0; c < ncell; c++) mean[c] = nmp::sun_interval_mean(lat[c], lon[c], nsample, t);
}

// noahmp_hip_forcing_shortwave: sw_b, mean_a and the normals may be NULL as in the call; par = max_ratio, mu_min, max_terrain_ratio,
// solar_constant
void shortwave_values(long ncell, const float* sw_a, const float* sw_b, const float* mean_a, const float* lat, const float* lon,
                      const float* ne, const float* nn, const float* nu, int mode, float fraction, float one_minus, float hour_utc,
                      float sin_declin, float cos_declin, const float* par, float* swdown) {
  nmp::SwParams k;
  memset(&k, 0, sizeof(k));
  k.now.hour_utc = hour_utc; k.now.sin_declin = sin_declin; k.now.cos_declin = cos_declin;
  k.fraction = fraction; k.one_minus = one_minus;
  k.max_ratio = par[0]; k.mu_min = par[1]; k.max_terrain_ratio = par[2]; k.solar_constant = par[3];
  k.mode = mode; k.has_b = (mode == NOAHMP_SW_LINEAR && sw_b) ? 1 : 0; k.has_normal = ne ? 1 : 0;
  for (long c = 0; c < ncell; c++)
    swdown[c] = nmp::sw_column(k, sw_a[c], k.has_b ? sw_b[c] : 0.f, mean_a ? mean_a[c] : 0.f, lat[c], lon[c], ne ? ne[c] : 0.f, nn ? nn[c] : 0.f,
                               nu ? nu[c] : 0.f);
}

// the Erbs diffuse fraction alone
void shortwave_kd(long n, const float* kt, float* kd) {
  for (long c = 0; c < n; c++) kd[c] = nmp::sw_erbs_kd(kt[c]);
}

}  // extern "C"
