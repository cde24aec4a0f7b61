// Shortwave forcing of a device-resident run (noahmp_hip_forcing_cosz_mean / noahmp_hip_forcing_shortwave): the per-column functions.
// __host__ __device__ like nmp_dev_regrid.hpp: tests/host_emul/shortwave_check.hip compiles the same functions for the CPU.
//
// No reference routine stands behind them (the reference reads forcing already prepared on the model grid and interpolates SWDOWN
// linearly, netcdf_io:1369-1403): the contract is the text in include/noahmp_hip.h, every rounding included.  Every line is one rounded
// float32 operation of that text, nothing may contract into an FMA whatever the compiler's setting, and there are no guards: what the
// arithmetic gives for NaN / Inf / unphysical operands is the result.  The only libm forms are libm::sinf_ / libm::cosf_ (glibc's bits
// for |x| < 120, NaN beyond), which hold no table: nothing is staged in LDS.
#pragma once
#include "nmp_dev_forcing.hpp"
#include "nmp_libm.hpp"

namespace nmp {

// the sun of one sample time, uniform over the grid: what fill_forcing_args makes for a forcing_prep call at that time
struct SunTime {
  float hour_utc, sin_declin, cos_declin;
};

// the sun vector of a column in local east / north / up coordinates; u has the bits of forcing_cosz
struct SunVec {
  float e, n, u;
};

// x > 0 ? x : +0.0 -- a NaN and -0.0 give +0.0
NMP_DEV float sw_max0(float x) { return x > 0.f ? x : 0.f; }
// a < b ? a : b -- a NaN a gives b, a NaN b gives b
NMP_DEV float sw_min(float a, float b) { return a < b ? a : b; }

// the hour angle of forcing_cosz (hdrv:856-858), the same operations in the same order
NMP_DEV float sun_hrang(float lon, float hour_utc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float q = lon / 15.0f;
  const float t0 = hour_utc + q;
  const float t1 = t0 + 24.0f;
  const float tloctim = fmodf(t1, 24.0f);
  const float d = tloctim - 12.f;
  const float a = 15.f * d;
  return a * NMP_DEGRAD;
}

// u alone: forcing_cosz with sin / cos of the latitude made by the caller, once per column (hdrv:859)
NMP_DEV float sun_up(float sinphi, float cosphi, float hrang, float sin_declin, float cos_declin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float ss = sinphi * sin_declin;
  const float cc = cosphi * cos_declin;
  const float cch = cc * libm::cosf_(hrang);
  return ss + cch;
}

// all three components; u by the same operations as sun_up
NMP_DEV SunVec sun_vector(float sinphi, float cosphi, float hrang, float sin_declin, float cos_declin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SunVec v;
  const float ch = libm::cosf_(hrang);
  const float sh = libm::sinf_(hrang);
  const float ss = sinphi * sin_declin;
  const float cc = cosphi * cos_declin;
  const float cch = cc * ch;
  v.u = ss + cch;
  const float pe = cos_declin * sh;
  v.e = -pe;
  const float cs = cosphi * sin_declin;
  const float sc = sinphi * cos_declin;
  const float sch = sc * ch;
  v.n = cs - sch;
  return v;
}

// mean of max(u, 0) over the samples of an interval: a sequential float32 sum in sample order, one IEEE division
NMP_DEV float sun_interval_mean(float lat, float lon, int nsample, const SunTime* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float phi = lat * NMP_DEGRAD;
  const float sinphi = libm::sinf_(phi), cosphi = libm::cosf_(phi);
  float acc = 0.f;
  for (int s = 0; s < nsample; s++) {
    const float u = sun_up(sinphi, cosphi, sun_hrang(lon, t[s].hour_utc), t[s].sin_declin, t[s].cos_declin);
    acc = acc + sw_max0(u);
  }
  return acc / (float)nsample;
}

// diffuse fraction of the global irradiance from the clearness index: Erbs, Klein and Duffie (1982), Horner form
NMP_DEV float sw_erbs_kd(float kt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (kt <= 0.22f) {
    const float a = 0.09f * kt;
    return 1.0f - a;
  }
  if (kt <= 0.80f) {
    float p = 12.336f * kt;
    p = p - 16.638f;
    p = p * kt;
    p = p + 4.388f;
    p = p * kt;
    p = p - 0.1604f;
    p = p * kt;
    return p + 0.9511f;
  }
  return 0.165f;                                               // kt > 0.80, and a NaN kt
}

// NOAHMP_SW_ZENITH: record a's value, which holds over [a, b), weighted by the cosine of the zenith angle now over its interval mean
NMP_DEV float sw_zenith(float sw_a, float mean, float mu, float max_ratio) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(mean > 0.f)) return 0.f;
  const float ratio = sw_min(mu / mean, max_ratio);
  return sw_a * ratio;
}

// slope and aspect: s on the horizontal -> the flux per unit map area on the surface with unit normal (ne, nn, nu); the form of WRF's
// topo_rad_adj.  Self-shading through cosi <= 0; cast shadows come in through sw_column_lit (the plane of nmp_dev_shadow.hpp) only; no
// terrain-reflected light.
NMP_DEV float sw_terrain(float s, const SunVec& v, float mu, float ne, float nn, float nu, float mu_min, float max_terrain_ratio,
                         float solar_constant) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (ne == 0.f && nn == 0.f) return s;                        // flat, either sign of the zeros: the bits of s
  if (mu < mu_min) return s;                                   // sun low or down: the bits of s
  const float pe = v.e * ne;
  const float pn = v.n * nn;
  const float pu = v.u * nu;
  const float pen = pe + pn;
  const float cosi = pen + pu;
  const float top = solar_constant * mu;
  const float kt = s / top;
  const float kd = sw_erbs_kd(kt);
  const float r = sw_min(sw_max0(cosi) / mu, max_terrain_ratio);
  const float beam = 1.0f - kd;
  const float br = beam * r;
  const float f = kd + br;
  return s * f;
}

// the parameters of noahmp_hip_forcing_shortwave that are uniform over the grid
struct SwParams {
  SunTime now;
  float fraction, one_minus;         // LINEAR with sw_b, as noahmp_hip_forcing_interpolate makes them (netcdf_io:1390)
  float max_ratio, mu_min, max_terrain_ratio, solar_constant;
  int mode, has_b, has_normal;
};

// one column of noahmp_hip_forcing_shortwave from its loaded operands (those its mode does not use are not looked at)
NMP_DEV float sw_column(const SwParams& k, float sw_a, float sw_b, float mean_a, float lat, float lon, float ne, float nn, float nu) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool zenith = k.mode == NOAHMP_SW_ZENITH;
  if (!zenith && !k.has_normal) return k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;
  const float phi = lat * NMP_DEGRAD;
  const float sinphi = libm::sinf_(phi), cosphi = libm::cosf_(phi);
  const float hrang = sun_hrang(lon, k.now.hour_utc);
  SunVec v;
  v.e = v.n = 0.f;
  if (k.has_normal) v = sun_vector(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  else v.u = sun_up(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  const float mu = sw_max0(v.u);
  float s;
  if (zenith) s = sw_zenith(sw_a, mean_a, mu, k.max_ratio);
  else s = k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;
  if (k.has_normal) s = sw_terrain(s, v, mu, ne, nn, nu, k.mu_min, k.max_terrain_ratio, k.solar_constant);
  return s;
}

// one column of noahmp_hip_forcing_shortwave_lit.  lit == 1.0f gives the bits of sw_column: the same functions on the same operands in
// the same order, and r0*1.0f is r0; every other value (a cast shadow, a fraction, a NaN) scales the direct beam, with or without
// normals.  One body for both, so that a wave with lit and shadowed lanes runs the sun, the time stage and the Erbs fraction once, not
// once per kind of lane (the first form called sw_column for the lit lanes: 1.41 of the unshaded call at mu ~ 0.10 with 13 % of the
// columns in shadow, tools/shadow_bench.py).
NMP_DEV float sw_column_lit(const SwParams& k, float lit, float sw_a, float sw_b, float mean_a, float lat, float lon, float ne, float nn,
                            float nu) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool zenith = k.mode == NOAHMP_SW_ZENITH;
  const bool shaded = !(lit == 1.0f);                          // a NaN is shaded
  if (!shaded && !zenith && !k.has_normal) return k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;      // sw_column makes no sun here
  const float phi = lat * NMP_DEGRAD;
  const float sinphi = libm::sinf_(phi), cosphi = libm::cosf_(phi);
  const float hrang = sun_hrang(lon, k.now.hour_utc);
  SunVec v;
  v.e = v.n = 0.f;
  if (k.has_normal) v = sun_vector(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  else v.u = sun_up(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  const float mu = sw_max0(v.u);
  float s;
  if (zenith) s = sw_zenith(sw_a, mean_a, mu, k.max_ratio);
  else s = k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;
  const bool sloped = k.has_normal && !(ne == 0.f && nn == 0.f);
  if (!shaded && !sloped) return s;                            // no normals, or flat: the bits of s, as sw_column / sw_terrain
  if (mu < k.mu_min) return s;                                 // sun low or down: the bits of s
  float r0 = 1.0f;
  if (sloped) {                                                // the lines of sw_terrain
    const float pe = v.e * ne;
    const float pn = v.n * nn;
    const float pu = v.u * nu;
    const float pen = pe + pn;
    const float cosi = pen + pu;
    r0 = sw_min(sw_max0(cosi) / mu, k.max_terrain_ratio);
  }
  const float top = k.solar_constant * mu;
  const float kt = s / top;
  const float kd = sw_erbs_kd(kt);
  const float r = r0 * lit;                                    // lit == 1.0f: the bits of r0
  const float beam = 1.0f - kd;
  const float br = beam * r;
  const float f = kd + br;
  return s * f;
}

// one column of noahmp_hip_forcing_radiation_sky, the shortwave: svf == 1.0f gives the bits of sw_column_lit, all its shortcuts included,
// and albedo is not looked at; every other value (a NaN included) narrows the diffuse part to the visible sky and adds the light the
// closed part reflects, for which the column's own horizontal global flux stands in for that of the surrounding slopes.  One body for both
// kinds of lane, for the reason given at sw_column_lit.
NMP_DEV float sw_column_sky(const SwParams& k, float svf, float lit, float albedo, float sw_a, float sw_b, float mean_a, float lat, float lon,
                            float ne, float nn, float nu) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool zenith = k.mode == NOAHMP_SW_ZENITH;
  const bool open = svf == 1.0f;                               // a NaN is not open
  const bool shaded = !(lit == 1.0f);
  if (open && !shaded && !zenith && !k.has_normal) return k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;
  const float phi = lat * NMP_DEGRAD;
  const float sinphi = libm::sinf_(phi), cosphi = libm::cosf_(phi);
  const float hrang = sun_hrang(lon, k.now.hour_utc);
  SunVec v;
  v.e = v.n = 0.f;
  if (k.has_normal) v = sun_vector(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  else v.u = sun_up(sinphi, cosphi, hrang, k.now.sin_declin, k.now.cos_declin);
  const float mu = sw_max0(v.u);
  float s;
  if (zenith) s = sw_zenith(sw_a, mean_a, mu, k.max_ratio);
  else s = k.has_b ? interp2(sw_a, sw_b, k.fraction, k.one_minus) : sw_a;
  const bool sloped = k.has_normal && !(ne == 0.f && nn == 0.f);
  const bool low = mu < k.mu_min;
  if (open && ((!shaded && !sloped) || low)) return s;         // the shortcuts of sw_column_lit: the bits of s
  float r = 1.0f, kd = 0.f;
  if (!low) {
    float r0 = 1.0f;
    if (sloped) {                                              // the lines of sw_terrain
      const float pe = v.e * ne;
      const float pn = v.n * nn;
      const float pu = v.u * nu;
      const float pen = pe + pn;
      const float cosi = pen + pu;
      r0 = sw_min(sw_max0(cosi) / mu, k.max_terrain_ratio);
    }
    const float top = k.solar_constant * mu;
    const float kt = s / top;
    kd = sw_erbs_kd(kt);
    r = r0 * lit;
  }
  const float beam = 1.0f - kd;
  const float br = beam * r;
  if (open) {                                                  // not low here: the last lines of sw_column_lit
    const float f = kd + br;
    return s * f;
  }
  float f0 = svf;                                              // sun low or down: whatever s holds is diffuse
  if (!low) {
    const float dif = kd * svf;
    f0 = dif + br;
  }
  const float o = 1.0f - svf;
  const float refl = albedo * o;
  const float f = f0 + refl;
  return s * f;
}

// one column of noahmp_hip_forcing_radiation_sky, the longwave: the visible sky's share of g plus what the closed part of the hemisphere
// emits at the column's own surface temperature and emissivity; svf == 1.0f keeps the bits of g
NMP_DEV float lw_column_sky(float svf, float g, float tsurf, float emiss, float sigma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (svf == 1.0f) return g;
  const float o = 1.0f - svf;
  const float t2 = tsurf * tsurf;
  const float t4 = t2 * t2;
  const float b = sigma * t4;
  const float eb = emiss * b;
  const float up = o * eb;
  const float dn = svf * g;
  return dn + up;
}

}  // namespace nmp
