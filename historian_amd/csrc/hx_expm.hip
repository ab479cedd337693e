// exp(R t) of a batch of (branch, component) matrices on the device, written where the resident history reads them.
//
// k_branch_expm: one workgroup per (changed node, component), hx_expm.h's routine - the bits of the host mirror's
// RateModel::getSubProbMatrix - into the idle slot of the node's matrix (bit 1 of its info word), the address
// k_history_scatter would have copied an uploaded matrix to.  The series' shape arrives from the host per (node, component).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "../../include/historian_hip.h"
#include "hx_kernels.h"
#include "hx_expm.h"

namespace hx {

namespace {

template <int R>
__global__ void __launch_bounds__(512) k_branch_expm(const double* __restrict__ rate, const ExpmShape* __restrict__ shape, const int* __restrict__ nodes,
                                                     const int* __restrict__ info, const int A, const int C, const int N, double* __restrict__ mats) {
  extern __shared__ double sh_expm[];               // b [A * A], then eB [A * A]
  const int AA = A * A;
  const int k = (int)blockIdx.x / C, cpt = (int)blockIdx.x - k * C, r = nodes[k];
  ExpmTile<R> tile;
  tile.init(A);
  tile.expm(rate + (long long)cpt * AA, shape[blockIdx.x], sh_expm, sh_expm + AA, mats + ((((long long)(info[r] >> 1) & 1) * C + cpt) * N + r) * AA);
}

int forced_waves() {
  const char* e = getenv("HX_EXPM_WAVES");
  return e ? atoi(e) : 0;
}

}  // namespace

// static + dynamic LDS of the instance that serves the plan, asked of the runtime: once per set of rates, not per launch (the
// query costs the host some 0.1 ms, which a launch made between two events would count as kernel time)
static int check_lds(const ExpmPlan& p) {
#define HX_EXPM_CASE(R_) case R_: HX_CHECK_LDS(k_branch_expm<R_>, p.lds, "k_branch_expm"); break;
  switch (p.per_lane) {
    HX_EXPM_CASE(1) HX_EXPM_CASE(2) HX_EXPM_CASE(3) HX_EXPM_CASE(4) HX_EXPM_CASE(5) HX_EXPM_CASE(6) HX_EXPM_CASE(7) HX_EXPM_CASE(8)
    default: return launch_fail("k_branch_expm has no instance for %d entries a lane", p.per_lane);
  }
#undef HX_EXPM_CASE
  return 0;
}

bool branch_expm_plan(const int A, ExpmPlan* plan) {
  if (A < 1 || A > 64) return false;
  *plan = expm_plan(A, forced_waves());
  return plan->lds <= (size_t)HX_LDS_LIMIT && check_lds(*plan) == 0;
}

int launch_branch_expm(const ExpmPlan& p, const double* rate, const ExpmShape* shape, const int* nodes, const int* info, const int n, const int A,
                       const int C, const int N, double* mats, hipStream_t st) {
  if (n <= 0) return 0;
  // (the plan was checked when it was made; what is checked here is that it is a plan for this alphabet)
  if (A < 1 || A > 64 || p.waves < 1 || p.waves > 8 || p.per_lane < 1 || p.per_lane > 8 || 64 * p.waves * p.per_lane < A * A ||
      p.lds != 2 * sizeof(double) * (size_t)A * A || p.lds > (size_t)HX_LDS_LIMIT)
    return launch_fail("k_branch_expm: no plan for an alphabet of %d symbols", A);
  const dim3 grid((unsigned)n * (unsigned)C), block(64u * (unsigned)p.waves);
#define HX_EXPM_CASE(R_) \
  case R_: hipLaunchKernelGGL(k_branch_expm<R_>, grid, block, p.lds, st, rate, shape, nodes, info, A, C, N, mats); break;
  switch (p.per_lane) {
    HX_EXPM_CASE(1) HX_EXPM_CASE(2) HX_EXPM_CASE(3) HX_EXPM_CASE(4) HX_EXPM_CASE(5) HX_EXPM_CASE(6) HX_EXPM_CASE(7) HX_EXPM_CASE(8)
  }
#undef HX_EXPM_CASE
  return 0;
}

}  // namespace hx

extern "C" int hx_expm_shape(double max_abs_rate, double t, int32_t* terms, int32_t* squarings, double* shrink) {
  if (!terms || !squarings || !shrink) return hx::api_fail(HX_ERR_INVALID_ARG, "hx_expm_shape: null argument");
  if (!(max_abs_rate >= 0.) || !hx::expm_length_ok(t) || !hx::expm_norm_ok(max_abs_rate, t))
    return hx::api_fail(HX_ERR_RANGE, "hx_expm_shape: a rate or a length that is negative, NaN or infinite, or their product overflows");
  const hx::ExpmShape s = hx::expm_shape(max_abs_rate, t);
  *terms = s.terms;
  *squarings = s.squarings;
  *shrink = s.shrink;
  return HX_OK;
}
