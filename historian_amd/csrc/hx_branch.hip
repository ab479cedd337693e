// Per-branch pair DPs: the three-state (Match / Insert / Delete) alignment of a parent sequence
// profile with a child sequence profile across one tree branch, inside a GuideAlignmentEnvelope.
//
// Reference: Refiner::BranchMatrix::BranchMatrix (src/refiner.cpp:10-60: Viterbi, what `historian reconstruct -refine` runs on
// every branch) and Sampler::BranchMatrix::BranchMatrix (src/sampler.cpp:1034-1084: the same lattice with log_sum_exp, the
// MCMC sampler's branch move); cell storage and envelope of TreeAlignFuncs::SparseDPMatrix<3> (src/sampler.h:66-166), the
// per-cell emission BranchMatrixBase::logMatch (src/sampler.h:207-209).
//
// The kernels are hx_pairdp.h's: k_pair_emission evaluates logMatch(i, j) = logInnerProduct(xSeq[i-1], ySub[j-1]) for every
// in-envelope cell up front, k_pair_fill sweeps the strips; this file has the lattice (BranchCell) and the job.  Max-plus is
// exact in any order, the log_sum_exp form uses the reference's operator in the reference's left-nested order: cells and lpEnd
// are bit-identical to the restatement (oracle/branch_oracle.py) in both forms.
//
// Storage: three state planes per pair, strip-skewed like the Forward matrices (hx_device.h cell_slot), -inf outside the
// envelope; hx_branch_batch_read_matrix returns the dense [x_len + 1][y_len + 1][3] array.
#include <hip/hip_runtime.h>
#include "hx_pairbatch.h"
#include "hx_branch_inputs.h"

namespace hx {
namespace {

struct DevBranch {
  static constexpr const char* abi = "hx_branch_batch";
  int32_t X, Y;                 // positions 0 .. x_len, 0 .. y_len
  int32_t CA, C;                // components * alphabet; components
  int32_t max_dist;             // < 0: no band
  const double* x_pwm;          // [x_len][CA]
  const double* y_sub;          // [y_len][CA]
  const double* y_emit;         // [y_len]
  const int32_t* x_env;         // [X] or nullptr
  const int32_t* y_env;         // [Y]
  double T[3][4];
  double* cells;                // [3][plane]
  double* emis;                 // [plane]: logMatch in the matrix layout
  int64_t plane, strip_stride;
  double* lp_end;
  const int32_t* win;           // banded: [n_strips][3][2] step windows of the strips (half-open, merged, in order; empty ones last), or nullptr
};

// The three-state lattice as the sweep and the walks of hx_pairdp.h see it (the fill: src/refiner.cpp:24-50 /
// src/sampler.cpp:1049-1072; BranchMatrixBase::getColumn / lpEmit: src/sampler.cpp:1166-1183).  States 0 Match, 1 Insert,
// 2 Delete; a cell reads all three of the cell above and of the diagonal cell.
template <bool VITERBI>
struct BranchCell {
  typedef DevBranch Job;
  enum { NS = 3, ND = 4, END = 3, NUP = 3, NDG = 3 };
  static __device__ __forceinline__ constexpr int up_plane(const int k) { return k; }
  // wavefronts of a launch above which a job gets fewer than one per strip: ~8 per SIMD
  static constexpr int64_t BATCH_WAVES = 8192 * 2;
  static constexpr const char* WAVES_ENV = "HX_BRANCH_WAVES";

  double mm, mi, md, im, ii, id, dm, dd;
  __device__ __forceinline__ explicit BranchCell(const DevBranch& J)
      : mm(J.T[0][0]), mi(J.T[0][1]), md(J.T[0][2]), im(J.T[1][0]), ii(J.T[1][1]), id(J.T[1][2]), dm(J.T[2][0]), dd(J.T[2][2]) {}
  static __device__ __forceinline__ double x_emit(const DevBranch&, const int) { return 0.0; }      // (a deletion scores nothing of its own)
  static __device__ __forceinline__ double combine(const double a, const double b, const double* __restrict__ tab) {
    return VITERBI ? vmax(a, b) : lse(a, b, tab);
  }
  __device__ __forceinline__ void cell(double (&now)[3], const double (&up)[3], const double (&diag)[3], const double (&left)[3], const double,
                                       const double yem, const double e_now, const bool start, const double* __restrict__ tab) const {
    now[2] = combine(combine(up[0] + md, up[1] + id, tab), up[2] + dd, tab);
    now[1] = yem + combine(left[0] + mi, left[1] + ii, tab);
    now[0] = e_now + combine(combine(diag[0] + mm, diag[1] + im, tab), diag[2] + dm, tab);
    if (start) now[0] = 0.0;                        // lpStart() = 0
  }
  template <class At>
  static __device__ __forceinline__ double lp_end(const DevBranch& J, const At at, const double* __restrict__ tab) {
    return combine(combine(at(0) + J.T[0][3], at(1) + J.T[1][3], tab), at(2) + J.T[2][3], tab);
  }

  static __device__ __forceinline__ void column(const int i, const int j, const int state, bool& x, bool& y) {
    const bool m = state == 0 && i > 0 && j > 0;
    x = m || state == 2;
    y = m || state == 1;
  }
  // lpEmit: where the term lies (p, left alone when it lies nowhere) and its value when it lies nowhere
  struct Emit {
    const double *emis, *y_emit;
    int64_t ss;
    __device__ __forceinline__ explicit Emit(const DevBranch& J) : emis(J.emis), y_emit(J.y_emit), ss(J.strip_stride) {}
    __device__ __forceinline__ double from(const int i, const int j, const int state, const double*& p) const {
      if (state == 0 && i > 0 && j > 0) p = emis + cell_slot(ss, i, j);
      if (state == 1 && j > 0) p = y_emit + (j - 1);
      return (state == 0 || state == 1) ? HX_NEG_INF : 0.0;
    }
  };
  static __device__ __forceinline__ bool self_loop(const int) { return false; }
};

// one job of the ABI -> its device job and its arrays in the arena; `reserved`: the per-position inputs have no host copy,
// the device fills their space
int fill_job(DevBranch& J, const hx_branch_job& j, Arena& a, const bool reserved) {
  if (j.x_len >= 64 * HXBR_MAX_STRIPS)
    return api_fail(HX_ERR_RANGE, "hx_branch_batch_create: a parent profile of more than 65535 positions");
  if (j.x_len < 0 || j.y_len < 0 || j.components < 1 || j.alphabet < 1 ||
      (!reserved && ((j.x_len && !j.x_pwm) || (j.y_len && (!j.y_sub || !j.y_emit)))) || (j.max_distance >= 0 && (!j.x_env || !j.y_env)))
    return api_fail(HX_ERR_INVALID_ARG, "hx_branch_batch_create: inconsistent job (lengths, components, missing arrays)");
  J.X = j.x_len + 1; J.Y = j.y_len + 1;
  J.CA = j.components * j.alphabet;
  J.C = j.components;
  J.max_dist = j.max_distance;
  for (int s = 0; s < 3; ++s)
    for (int d = 0; d < 4; ++d) J.T[s][d] = j.trans[s][d];
  if (reserved) {
    a.reserve(J.x_pwm, (size_t)j.x_len * J.CA);
    a.reserve(J.y_sub, (size_t)j.y_len * J.CA);
    a.reserve(J.y_emit, (size_t)j.y_len);
  } else {
    a.put(J.x_pwm, j.x_pwm, (size_t)j.x_len * J.CA);
    a.put(J.y_sub, j.y_sub, (size_t)j.y_len * J.CA);
    a.put(J.y_emit, j.y_emit, (size_t)j.y_len);
  }
  put_env(a, J, j.x_env, j.y_env, !getenv("HX_BRANCH_NO_WINDOWS"));
  return HX_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

struct hx_branch_batch : PairBatch<DevBranch, 3> {
  bool viterbi = false;             // the form of the last run
};

long long hx::branch_max_x_len() { return 64LL * HXBR_MAX_STRIPS; }

int hx::branch_batch_reserve(const hx_branch_job* jobs, const double* const* log_sub, const double* const* log_ins, const int32_t n_jobs,
                             hx_branch_batch** out, BranchInputs* where) {
  const int rc = hx_branch_batch::create(jobs, n_jobs, out, [&](DevBranch& J, const hx_branch_job& j, Arena& a) {
    if (const int bad = fill_job(J, j, a, true)) return bad;
    BranchInputs& w = where[&j - jobs];
    a.put(w.log_sub, log_sub[&j - jobs], (size_t)j.components * j.alphabet * j.alphabet);
    a.put(w.log_ins, log_ins[&j - jobs], (size_t)j.components * j.alphabet);
    return (int)HX_OK;
  });
  if (rc != HX_OK) return rc;
  for (int k = 0; k < n_jobs; ++k) {
    const DevBranch& J = (*out)->jobs[k];
    where[k].x_pwm = const_cast<double*>(J.x_pwm);
    where[k].y_sub = const_cast<double*>(J.y_sub);
    where[k].y_emit = const_cast<double*>(J.y_emit);
  }
  return HX_OK;
}

extern "C" {

int hx_branch_batch_destroy(hx_branch_batch* b) { delete b; return HX_OK; }

int hx_branch_batch_create(const hx_branch_job* jobs, int32_t n_jobs, hx_branch_batch** out) {
  return hx_branch_batch::create(jobs, n_jobs, out, [](DevBranch& J, const hx_branch_job& j, Arena& a) { return fill_job(J, j, a, false); });
}

int hx_branch_batch_read_inputs(hx_branch_batch* b, int32_t job, double* x_pwm, double* y_sub, double* y_emit) {
  if (!b) return api_fail(HX_ERR_INVALID_ARG, "batch is null");
  if (job < 0 || job >= b->n_jobs) return api_fail(HX_ERR_RANGE, "job out of range");
  const DevBranch& J = b->jobs[job];
  const size_t nx = sizeof(double) * (size_t)(J.X - 1) * J.CA, ny = sizeof(double) * (size_t)(J.Y - 1) * J.CA, ne = sizeof(double) * (size_t)(J.Y - 1);
  if (hipSetDevice(b->device) != hipSuccess || (x_pwm && nx && hipMemcpy(x_pwm, J.x_pwm, nx, hipMemcpyDeviceToHost) != hipSuccess) ||
      (y_sub && ny && hipMemcpy(y_sub, J.y_sub, ny, hipMemcpyDeviceToHost) != hipSuccess) ||
      (y_emit && ne && hipMemcpy(y_emit, J.y_emit, ne, hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "hx_branch_batch_read_inputs: HIP call failed");
  return HX_OK;
}

int hx_branch_batch_run(hx_branch_batch* b, int32_t viterbi, void* stream) {
  const int rc = viterbi ? hx_branch_batch::run<BranchCell<true>>(b, stream) : hx_branch_batch::run<BranchCell<false>>(b, stream);
  if (rc == HX_OK) b->viterbi = viterbi != 0;
  return rc;
}

int hx_branch_batch_results(hx_branch_batch* b, double* lp_end) { return hx_branch_batch::results(b, lp_end); }

int hx_branch_batch_read_matrix(hx_branch_batch* b, int32_t job, double* out) { return hx_branch_batch::read_matrix(b, job, out); }

int64_t hx_branch_batch_total_cells(const hx_branch_batch* b) { return hx_branch_batch::total_cells(b); }

int hx_branch_batch_last_kernel_ms(hx_branch_batch* b, float* ms) { return hx_branch_batch::last_kernel_ms(b, ms, nullptr); }

int hx_branch_batch_best_paths(hx_branch_batch* b, uint8_t* states, int64_t cap, int32_t* n_steps) {
  if (b && b->done && !b->viterbi) return api_fail(HX_ERR_STATE, "hx_branch_batch_best_paths: the batch last ran with viterbi = 0");
  return pair_walk_paths<BranchCell<true>, true>(b, nullptr, nullptr, states, cap, n_steps, nullptr);
}

int hx_branch_batch_sample_paths(hx_branch_batch* b, const uint32_t* words, const int64_t* word_off, uint8_t* states, int64_t cap,
                                 int32_t* n_steps, int32_t* words_used) {
  if (b && b->done && b->viterbi) return api_fail(HX_ERR_STATE, "hx_branch_batch_sample_paths: the batch last ran with viterbi != 0");
  return pair_walk_paths<BranchCell<false>, false>(b, words, word_off, states, cap, n_steps, words_used);
}

int64_t hx_branch_batch_max_steps(const hx_branch_batch* b) {
  int64_t most = 0;
  if (b)
    for (const DevBranch& J : b->jobs) most = std::max<int64_t>(most, (int64_t)(J.X - 1) + (J.Y - 1) + 1);      // (every state but End moves: header)
  return most;
}

int hx_branch_batch_read_cells(hx_branch_batch* b, int32_t job, int64_t n, const hx_pair_cell* at, double* cells, double* log_match) {
  return pair_read_cells<3>(b, job, n, at, cells, log_match);
}

int hx_branch_batch_last_walk_ms(hx_branch_batch* b, float* ms) { return pair_last_walk_ms(b, ms); }

}  // extern "C"
