// What the envelope-bounded pair DPs over TreeAlignFuncs::SparseDPMatrix share (hx_branch.hip: three states, hx_sibling.hip:
// eleven): the envelope test, the emission pre-pass, the hand-off of a strip's last row to the strip below, and the step
// windows of a banded job's strips.
//
// A job type has: X, Y (positions 0 .. len of the row / column profile), C, CA, max_dist, x_pwm [X-1][CA], y_sub [Y-1][CA],
// x_env [X], y_env [Y], cells, emis, plane, strip_stride.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <utility>
#include <vector>
#include "hx_device.h"
#include "hx_lse.h"

namespace hx {

// columns of the strip above's last row fetched at a time / strips whose progress a workgroup keeps in LDS
#define HXBR_BLK 16
#define HXBR_MAX_STRIPS 1024

template <class Job>
__device__ __forceinline__ bool pair_in_env(const Job& J, const int i, const int j) {
  // TreeAlignFuncs::SparseDPMatrix::inEnvelope (src/sampler.h:146-149)
  if (i == 0 || j == 0 || i == J.X - 1 || j == J.Y - 1 || J.max_dist < 0) return true;
  int d = J.x_env[i] - J.y_env[j];
  d = d < 0 ? -d : d;
  return d <= J.max_dist;
}

// logMatch for every in-envelope cell with i, j >= 1: the nested logInnerProduct of src/logsumexp.h:132-151 - over the
// components, of the sum over the residues - in the reference's table arithmetic.  grid (jobs, row slices)
template <class Job>
__global__ void k_pair_emission(const Job* __restrict__ jobs, const double* __restrict__ tab) {
  const Job& J = jobs[blockIdx.x];
  const int C = J.C, A = J.CA / C;
  const int64_t n = (int64_t)J.X * J.Y;
  for (int64_t c = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.y * blockDim.x) {
    const int i = (int)(c / J.Y), j = (int)(c % J.Y);
    if (i == 0 || j == 0 || !pair_in_env(J, i, j)) continue;
    const double* xs = J.x_pwm + (size_t)(i - 1) * J.CA;
    const double* ys = J.y_sub + (size_t)(j - 1) * J.CA;
    double lip = HX_NEG_INF;
    for (int cpt = 0; cpt < C; ++cpt) {
      double inner = HX_NEG_INF;
      for (int a = 0; a < A; ++a) inner = lse(inner, xs[cpt * A + a] + ys[cpt * A + a], tab);
      lip = lse(lip, inner, tab);
    }
    J.emis[cell_slot(J.strip_stride, i, j)] = lip;
  }
}

// value of lane `src` (wave-uniform)
__device__ __forceinline__ double read_lane64(const double v, const int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// The strip hand-off: a strip publishes how many columns of its last row are stored (a monotonic count in LDS, written
// behind a drain of the wavefront's stores); the strip below waits until the count covers the columns it is about to load
// with agent-scope loads.  Strip s waits for strip s - 1 only, so waits cannot form a cycle.
__device__ __forceinline__ void strip_wait(volatile int* prog, const int above, int& seen, const int need) {
  while (seen < need) {
    seen = __builtin_amdgcn_readfirstlane(prog[above]);
    if (seen < need) __builtin_amdgcn_s_sleep(2);
  }
  asm volatile("" ::: "memory");
}

// Step windows of a banded job's strips (steps t = column + row-in-strip): what is always inside the envelope - the first
// and the last column (SparseDPMatrix::inEnvelope, src/sampler.h:146-149) - and the band, as up to three half-open ranges that
// together hold every in-envelope cell of the strip's rows (supersets are harmless: a cell is tested again).  The strips of
// the first and the last row sweep everything.  Any envelope coordinates (not only non-decreasing ones): the columns of a
// coordinate value are bracketed once, a row takes the brackets of the values within max_distance of its own.
inline std::vector<int32_t> branch_windows(const int32_t* xenv, const int32_t* yenv, int X, int Y, int band) {
  const int n_strips = (X + HX_STRIP - 1) / HX_STRIP, nsteps = Y + HX_STRIP - 1;
  std::vector<int32_t> w(6 * (size_t)n_strips, 0);
  int V = 0;
  for (int j = 0; j < Y; ++j) V = std::max(V, (int)yenv[j]);
  std::vector<int> minj(V + 1, INT_MAX), maxj(V + 1, -1);
  for (int j = 0; j < Y; ++j) {
    const int v = yenv[j] < 0 ? 0 : yenv[j];
    minj[v] = std::min(minj[v], j);
    maxj[v] = std::max(maxj[v], j);
  }
  // (prefix brackets would make a row O(1); bands are tens of values wide)
  for (int s = 0; s < n_strips; ++s) {
    int32_t* o = &w[6 * (size_t)s];
    const int rows = std::min(HX_STRIP, X - s * HX_STRIP);
    if (s == 0 || s == n_strips - 1) { o[0] = 0; o[1] = (nsteps + 1) & ~1; continue; }
    int lo = INT_MAX, hi = -1;
    for (int l = 0; l < rows; ++l) {
      const int xe = xenv[s * HX_STRIP + l] < 0 ? 0 : xenv[s * HX_STRIP + l];
      int jmin = INT_MAX, jmax = -1;
      for (int v = std::max(0, xe - band); v <= std::min(V, xe + band); ++v) {
        jmin = std::min(jmin, minj[v]);
        jmax = std::max(jmax, maxj[v]);
      }
      if (jmax < 0) continue;
      lo = std::min(lo, jmin + l);
      hi = std::max(hi, jmax + l);
    }
    std::pair<int, int> r[3] = {{0, rows}, {lo, hi + 1}, {Y - 1, Y - 1 + rows}};
    if (hi < 0) r[1] = {INT_MAX, INT_MAX};         // (no band cell in the strip)
    // in order, merged where they touch
    std::sort(r, r + 3);
    int n = 0;
    for (int k = 0; k < 3; ++k) {
      if (r[k].second <= r[k].first) continue;
      if (n > 0 && r[k].first <= o[2 * (n - 1) + 1]) o[2 * (n - 1) + 1] = std::max(o[2 * (n - 1) + 1], r[k].second);
      else { o[2 * n] = r[k].first; o[2 * n + 1] = r[k].second; ++n; }
    }
    // whole step pairs (the fill stores a row's cells of steps 2m, 2m + 1 together), merged again where they now touch
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const int a = o[2 * k] & ~1, b = std::min((o[2 * k + 1] + 1) & ~1, (nsteps + 1) & ~1);
      if (m > 0 && a <= o[2 * (m - 1) + 1]) o[2 * (m - 1) + 1] = std::max(o[2 * (m - 1) + 1], b);
      else { o[2 * m] = a; o[2 * m + 1] = b; ++m; }
    }
    for (int k = m; k < 3; ++k) o[2 * k] = o[2 * k + 1] = 0;
  }
  return w;
}

}  // namespace hx
