// TEST INFRASTRUCTURE: the per-member functions of the region series (noahmp_amd/csrc/nmp_dev_regions.hpp) compiled for the host, applied
// to whole arrays.  tests/test_regions.py builds this file on demand (-ffp-contract=off, like the engine) and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nmp_dev_regions.hpp"

extern "C" {

// out[i] <- the float64 term of member i: takes part iff hist_takes_part(xland[i], xice[i], xice_thres)
void regions_term(int op, const float* xland, const float* xice, float xice_thres, const float* w, const float* x, double* out, long n) {
  for (long i = 0; i < n; i++) out[i] = nmp::reg_term(op, nmp::hist_takes_part(xland[i], xice[i], xice_thres), w[i], x[i]);
}

void regions_takes_part(const float* xland, const float* xice, float xice_thres, unsigned char* out, long n) {
  for (long i = 0; i < n; i++) out[i] = nmp::hist_takes_part(xland[i], xice[i], xice_thres) ? 1 : 0;
}

// out[i] <- one node of the tree
void regions_combine(int op, const double* a, const double* b, double* out, long n) {
  for (long i = 0; i < n; i++) out[i] = nmp::reg_combine(op, a[i], b[i]);
}

double regions_identity(int op) { return nmp::reg_identity(op); }

// the terms of a list reduced one after the other from the identity: for MIN / MAX the order must not matter
double regions_reduce(int op, const double* t, long n) {
  double v = nmp::reg_identity(op);
  for (long i = 0; i < n; i++) v = nmp::reg_combine(op, v, t[i]);
  return v;
}

}  // extern "C"
