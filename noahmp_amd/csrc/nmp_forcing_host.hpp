// Host-side helper of the forcing units that make a sun (noahmp_shortwave.hip, noahmp_shadow.hip).
#pragma once
#include "noahmp_hip.h"
#include "nmp_dev_shortwave.hpp"

namespace nmp_host {

// what fill_forcing_args makes of a time (noahmp_forcing.hip, which also needs the Julian day and so keeps its own lines): the declination
// with the host's libm, hour_utc left to right (hdrv:856)
inline nmp::SunTime sun_of(const noahmp_sun_time& t) {
  nmp::SunTime s;
  noahmp_hip_declination(t.iday, t.ihour, &s.sin_declin, &s.cos_declin);
  s.hour_utc = (float)t.ihour + (float)t.iminute / 60.0f + (float)t.isecond / 3600.0f;
  return s;
}

}  // namespace nmp_host
