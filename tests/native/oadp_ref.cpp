// oadp_ref.cpp — the CPU statement of the OADP projection over bigsnpr_amd/csrc/oadp_step.hpp: the header the kernel
// compiles from, instantiated for a group of one lane, sample after sample.  Built by oadp_ref.py.
#include <stdint.h>

#include <vector>

#include "oadp_step.hpp"

using namespace bsn::oadp;

extern "C" {

int oadp_max_k() { return kMaxK; }
int oadp_sweep_cap() { return kSweepCap; }

// NULL when (K, sval) is accepted, else the message the library fails with
const char *oadp_check(int64_t K, const double *sval) { return check_args(K, sval); }

// XV, out: n x K column-major; X_norm: n; sweeps (n, may be NULL): the sweep count of each sample (-1: a NaN row).
// Returns 0, or 1 when check_args refuses (nothing is written then).
int oadp_proj(const double *XV, const double *X_norm, const double *sval, int64_t n, int64_t K, double *out, int32_t *sweeps) {
  if (check_args(K, sval)) return 1;
  std::vector<double> ws(work_doubles((int)K));
  const Solo g;
  for (int64_t i = 0; i < n; i++) {
    const int s = project_one(g, (int)K, sval, XV + i, n, X_norm[i], ws.data(), out + i, n);
    if (sweeps) sweeps[i] = s;
  }
  return 0;
}

}  // extern "C"
