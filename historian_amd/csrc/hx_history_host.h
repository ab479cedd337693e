// The host's share of a branch-length proposal to the resident history (hx_history.hip), free of HIP so that a stand-alone
// program can run it under a sanitizer on the CPU (host/t/testhistoryhost.cpp): the shape of the series of exp(R t), the
// validation of the lengths, the closure of the changed nodes over their ancestors, the launch plan of k_branch_expm.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/historian_hip.h"

namespace hx {

// What k_branch_expm is told about one (node, component): everything of gsl_linalg_exponential_ss that is not a multiply,
// an add or 1. / integer.
struct ExpmShape {
  double t, shrink;
  int terms, squarings;
};

// RateModel::getSubProbMatrix's (terms, squarings, shrink) for a matrix R t whose largest |element| is fl(max_abs_rate * t):
// rounding is monotone and t >= 0, so max_ij |fl(R_ij t)| == fl(max_ij |R_ij| * t).  The double-precision row of the table
// in GSL's linalg/exponential.c; the host's libm for log, ceil and exp, as the mirror (hx_host_base.cpp) takes them.
inline ExpmShape expm_shape(const double max_abs_rate, const double t) {
  static const int table[6][2] = {{5, 1}, {5, 4}, {7, 5}, {9, 7}, {10, 10}, {8, 14}};
  static const double below[6] = {0.01, 0.1, 1., 10., 100., 1000.};
  const double norm = max_abs_rate * t;
  ExpmShape s;
  s.t = t;
  s.terms = table[5][0];
  s.squarings = -1;
  for (int r = 0; r < 6 && s.squarings < 0; ++r)
    if (norm < below[r]) { s.terms = table[r][0]; s.squarings = table[r][1]; }
  if (s.squarings < 0) s.squarings = table[5][1] + (int)ceil(log(1.01 * norm / 1000.) / log(2.));
  s.shrink = 1. / exp(log(2.) * s.squarings);
  return s;
}

// a branch length the series can be shaped for: not negative, not NaN, not infinite
inline bool expm_length_ok(const double t) { return t >= 0. && t < INFINITY; }
// ... and not so large that the table's last row (log(1.01 norm / 1000)) sees an infinite norm
inline bool expm_norm_ok(const double max_abs_rate, const double t) { return 1.01 * (max_abs_rate * t) < INFINITY; }

// the largest |element| of an A x A rate matrix; false when an element is NaN or infinite
inline bool expm_max_abs(const double* rate, const int AA, double* max_abs) {
  double m = 0.;
  for (int e = 0; e < AA; ++e) {
    const double v = fabs(rate[e]);
    if (!(v < INFINITY)) return false;
    if (v > m) m = v;
  }
  *max_abs = m;
  return true;
}

// k_branch_expm's workgroup: W waves share the A x A entries, entry e with thread e mod 64 W.  A lone matrix is a chain of
// dependent products, so the waves are what shortens it: one entry a lane while eight waves allow (A = 20: W = 7, measured
// against 1, 2, 4 and 8 waves in DESIGN.md section 19), at most 8 entries a lane (A = 64: W = 8).  forced_waves in 1 .. 8 takes that
// many instead (HX_EXPM_WAVES, a measurement hook) if 8 entries a lane still do.  The result does not depend on W.
struct ExpmPlan { int waves, per_lane; size_t lds; };
inline ExpmPlan expm_plan(const int A, const int forced_waves) {
  const int AA = A * A;
  ExpmPlan p;
  p.waves = (AA + 63) / 64 < 8 ? (AA + 63) / 64 : 8;
  if (forced_waves >= 1 && forced_waves <= 8 && AA <= 512 * forced_waves) p.waves = forced_waves;
  p.per_lane = (AA + 64 * p.waves - 1) / (64 * p.waves);
  p.lds = 2 * sizeof(double) * (size_t)AA;
  return p;
}

// A proposal's nodes.  0: fine - `changed` holds them in the caller's order, `walked` them and their ancestors ascending
// (children before parents); 1: a node outside 0 .. N - 2; 2: a node named twice.  parent: [N], children before parents.
inline int history_closure(const std::vector<int>& parent, const int n_changed, const int* nodes, std::vector<int>& changed, std::vector<int>& walked) {
  const int N = (int)parent.size();
  std::vector<unsigned char> mark(N, 0);
  changed.clear();
  walked.clear();
  for (int k = 0; k < n_changed; ++k) {
    if (nodes[k] < 0 || nodes[k] >= N - 1) return 1;
    if (mark[nodes[k]]) return 2;
    mark[nodes[k]] = 1;
    changed.push_back(nodes[k]);
  }
  for (int r : changed)
    for (int p = parent[r]; p >= 0 && !mark[p]; p = parent[p]) mark[p] = 2;
  for (int r = 0; r < N; ++r)
    if (mark[r]) walked.push_back(r);
  return 0;
}

// ---- excluded-neighbour profiles (k_history_excluded): the host's share of a query ----

// The positions of every node - the columns in which it is not a gap - and, per block of 64 columns, the position of the
// block's first column.  tokT: [N][ncp] transposed tokens, -2 a gap (the padding past n_cols is gaps).
// len: [N]; block_off: [N][ncp / 64].
inline void history_positions(const signed char* tokT, const int N, const long long ncp, std::vector<long long>& len, std::vector<long long>& block_off) {
  const long long n_blocks = ncp / 64;
  len.assign(N, 0);
  block_off.assign((size_t)N * n_blocks, 0);
  for (int r = 0; r < N; ++r) {
    long long at = 0;
    for (long long b = 0; b < n_blocks; ++b) {
      block_off[(size_t)r * n_blocks + b] = at;
      const signed char* t = tokT + (size_t)r * ncp + b * 64;
      for (int l = 0; l < 64; ++l) at += t[l] != -2;
    }
    len[r] = at;
  }
}

// The plan of one query.  Per pair four words: the node, the excluded neighbour, where its path starts in `path` (-1: the
// excluded neighbour is the parent, no way down is needed) and the path's length; the path runs from the tree's root to
// the node, both included.  out_off / out_len: where the pair's [len][C][A] block starts in the output (in doubles) and
// its rows.
struct ExcludedPlan {
  std::vector<int> pair, path;
  std::vector<long long> out_off, out_len;
  long long total = 0;               // doubles of output
  long long max_len = 0;
};
// 0: fine; 1: a node or neighbour outside 0 .. N - 1; 2: a neighbour that is neither the node's parent nor its child.
// parent: [N], children before parents, the root last; len: history_positions'; row: C * A.
inline int history_excluded_plan(const std::vector<int>& parent, const std::vector<long long>& len, const long long row, const int n_pairs, const int* node,
                                 const int* exclude, ExcludedPlan& plan) {
  const int N = (int)parent.size();
  plan = ExcludedPlan();
  for (int k = 0; k < n_pairs; ++k)
    if (node[k] < 0 || node[k] >= N || exclude[k] < 0 || exclude[k] >= N) return 1;
  for (int k = 0; k < n_pairs; ++k)
    if (parent[node[k]] != exclude[k] && parent[exclude[k]] != node[k]) return 2;
  std::vector<int> up;
  for (int k = 0; k < n_pairs; ++k) {
    const int r = node[k];
    const bool down = parent[r] != exclude[k];
    plan.pair.push_back(r);
    plan.pair.push_back(exclude[k]);
    plan.pair.push_back(down ? (int)plan.path.size() : -1);
    up.clear();
    for (int p = r; down && p >= 0; p = parent[p]) up.push_back(p);
    plan.pair.push_back((int)up.size());
    plan.path.insert(plan.path.end(), up.rbegin(), up.rend());
    plan.out_off.push_back(plan.total);
    plan.out_len.push_back(len[r]);
    plan.total += len[r] * row;
    if (len[r] > plan.max_len) plan.max_len = len[r];
  }
  return 0;
}

// ---- the hand-off to the branch DP (hx_history_branch_batch_create): the host's share ----

// The query's pairs - (parent, node) then (node, parent) per branch: x_pwm and the child's profile - and the jobs of the
// batch with their lengths, transition scores and envelopes; the per-position arrays stay null, the device fills them.
struct BranchHandoffPlan {
  std::vector<int> node, exclude;
  std::vector<hx_branch_job> jobs;
};
// 0: fine; 1: a node outside 0 .. N - 2; 2: a null log_sub or log_ins, or a band without both envelopes; 3: a parent row of
// max_x_len positions or more (or a child row beyond 32 bits).  parent, len: as history_excluded_plan.
inline int history_branch_plan(const std::vector<int>& parent, const std::vector<long long>& len, const int A, const int C, const hx_history_branch* br,
                               const int n_branches, const long long max_x_len, BranchHandoffPlan& plan) {
  const int N = (int)parent.size();
  plan = BranchHandoffPlan();
  for (int k = 0; k < n_branches; ++k)
    if (br[k].node < 0 || br[k].node >= N - 1) return 1;
  for (int k = 0; k < n_branches; ++k)
    if (!br[k].log_sub || !br[k].log_ins || (br[k].max_distance >= 0 && (!br[k].x_env || !br[k].y_env))) return 2;
  for (int k = 0; k < n_branches; ++k)
    if (len[parent[br[k].node]] >= max_x_len || len[br[k].node] > 0x7ffffffe) return 3;
  for (int k = 0; k < n_branches; ++k) {
    const int r = br[k].node, p = parent[r];
    plan.node.push_back(p); plan.exclude.push_back(r);
    plan.node.push_back(r); plan.exclude.push_back(p);
    hx_branch_job j = {};
    j.x_len = (int32_t)len[p];
    j.y_len = (int32_t)len[r];
    j.components = C;
    j.alphabet = A;
    for (int s = 0; s < 3; ++s)
      for (int d = 0; d < 4; ++d) j.trans[s][d] = br[k].trans[s][d];
    j.x_env = br[k].x_env;
    j.y_env = br[k].y_env;
    j.max_distance = br[k].max_distance;
    plan.jobs.push_back(j);
  }
  return 0;
}

}  // namespace hx
