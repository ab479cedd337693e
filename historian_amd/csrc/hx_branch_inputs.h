// A branch batch whose per-position inputs are computed on the device (hx_history_branch_batch_create, hx_history.hip): what
// hx_branch.hip, which owns hx_branch_batch, offers the resident history.
#pragma once
#include <cstdint>
#include "../../include/historian_hip.h"

namespace hx {

// where a job's inputs lie in the batch's arena (device addresses; null where the length is 0 ... never read then)
struct BranchInputs {
  double *x_pwm, *y_sub, *y_emit;
  const double *log_sub, *log_ins;      // [C][A][A], [C][A]: the caller's logs, copied with the host image
};

// hx_branch_batch_create for jobs whose x_pwm, y_sub and y_emit are not read: their space is reserved in the arena and
// reported in where[k], with log_sub[k] and log_ins[k] uploaded beside the small inputs.  The jobs are valid already.
int branch_batch_reserve(const hx_branch_job* jobs, const double* const* log_sub, const double* const* log_ins, int32_t n_jobs,
                         hx_branch_batch** out, BranchInputs* where);

// the parent rows hx_branch_batch_create accepts: fewer positions than this
long long branch_max_x_len();

}  // namespace hx
