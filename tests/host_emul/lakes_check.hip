// TEST INFRASTRUCTURE: the per-item functions of the lakes (noahmp_amd/csrc/nmp_dev_lakes.hpp) compiled for the host, applied to whole
// lists.  tests/test_lakes.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_lakes.hpp"

extern "C" {

// one call of noahmp_hip_lake_take over a member list, the entries in list order
void lake_take_entries(const int32_t* member_cell, const int32_t* member_lake, long long nmember, float* storage, long long* inflow, int nlake,
                       long long ncell, double q) {
  nmp::LakeTakeArgs t;
  t.member_cell = member_cell; t.member_lake = member_lake; t.storage = storage; t.inflow = inflow;
  t.nmember = nmember; t.ncell = ncell; t.nlake = nlake; t.q = q; t.invq = 1.0 / q; t.qf = (float)q;
  for (long long e = 0; e < nmember; e++) {
    const nmp::LakeTaken r = nmp::lake_take_entry(t, e);
    if (r.lake >= 0) inflow[r.lake] += r.n;
  }
}

// one call of noahmp_hip_lake_release over the lakes; level, outflow and diag (one word) or NULL
void lake_release_lakes(long long* volume, long long* inflow, const double* area, const double* weir_h, const double* weir_c, const double* weir_l,
                        const double* orifice_h, const double* orifice_c, const double* orifice_a, const int32_t* outlet_cell, float* out_new,
                        long long ncell, double* level, float* outflow, uint32_t* diag, int nlake, double q, double dt) {
  nmp::LakeReleaseArgs r;
  r.volume = volume; r.inflow = inflow; r.area = area; r.weir_h = weir_h; r.weir_c = weir_c; r.weir_l = weir_l;
  r.orifice_h = orifice_h; r.orifice_c = orifice_c; r.orifice_a = orifice_a; r.outlet_cell = outlet_cell; r.out_new = out_new;
  r.level = level; r.outflow = outflow; r.ncell = ncell; r.q = q; r.invq = 1.0 / q; r.dt = dt; r.nlake = nlake;
  for (int l = 0; l < nlake; l++) {
    const uint32_t emptied = nmp::lake_release_one(r, l);
    if (diag) diag[0] += emptied;
  }
}

}  // extern "C"
