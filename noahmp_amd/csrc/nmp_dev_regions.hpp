// Region series (noahmp_hip_region_step): the term of one member cell and the combination of two partial results.
// __host__ __device__ like the other nmp_dev_*.hpp: tests/host_emul/regions_check.hip compiles the same functions for the CPU.
//
// Everything is carried as float64.  A SUM term is (double)w * (double)x: the product of two float32 values has at most 48 significant
// bits, so it is exact and no contraction setting can change it.  MIN / MAX terms are float32 values (exact in float64) that went through
// hist_apply against the identity of the op, so a NaN sample -- which never wins there -- has already become the identity and the
// minimum / maximum of the terms does not depend on their order.
#pragma once
#include "nmp_dev_history.hpp"

namespace nmp {

NMP_DEV int reg_hist_op(int op) { return op == NOAHMP_REG_MIN ? NOAHMP_HIST_MIN : NOAHMP_HIST_MAX; }

// what an empty list gives, and what pads a chunk: +0.0, +HUGE, -HUGE
NMP_DEV double reg_identity(int op) {
  return op == NOAHMP_REG_SUM ? 0.0 : (op == NOAHMP_REG_MIN ? (double)kHistHuge : -(double)kHistHuge);
}

// the term of one member: takes = hist_takes_part(xland, xice, xice_thres) of the cell at this step
NMP_DEV double reg_term(int op, bool takes, float w, float x) {
  if (op == NOAHMP_REG_SUM) return takes ? (double)w * (double)x : 0.0;
  const float id = (op == NOAHMP_REG_MIN) ? kHistHuge : -kHistHuge;
  return (double)(takes ? hist_apply(reg_hist_op(op), id, x, 0.f) : id);
}

// one node of the tree: v[i] = v[i] + v[i+h], or the comparison of hist_apply on values that are never NaN
NMP_DEV double reg_combine(int op, double a, double b) {
  switch (op) {
    case NOAHMP_REG_SUM: return a + b;
    case NOAHMP_REG_MIN: return (b < a) ? b : a;
    default:             return (b > a) ? b : a;
  }
}

}  // namespace nmp
