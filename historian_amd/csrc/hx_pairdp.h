// What the envelope-bounded pair DPs over TreeAlignFuncs::SparseDPMatrix share (hx_branch.hip: three states, hx_sibling.hip:
// eleven): the envelope test, the emission pre-pass, the hand-off of a strip's last row to the strip below, and the step
// windows of a banded job's strips.
//
// And what consumes a filled matrix where it lies: the walks (best path, sampled path: one wavefront per job, all jobs of a
// batch side by side) and the gather of cells along a path.
//
// A job type has: X, Y (positions 0 .. len of the row / column profile), C, CA, max_dist, x_pwm [X-1][CA], y_sub [Y-1][CA],
// x_env [X], y_env [Y], cells, emis, plane, strip_stride.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <type_traits>
#include <utility>
#include <vector>
#include "hx_device.h"
#include "hx_lse.h"
#include "hx_policy.h"
#include "../../include/historian_hip.h"

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

// ---- walks through a filled matrix ------------------------------------------------------------------------------------------
// Refiner::BranchMatrix::best (src/refiner.cpp:62-104), Sampler::BranchMatrix::sample (src/sampler.cpp:1088-1120) and
// Sampler::SiblingMatrix::sample (:1343-1386) are one loop: from (X - 1, Y - 1, End) back to cell (0, 0), a step takes the
// present cell's column (getColumn), steps to the source cell, and weighs that cell's states s by
// w[s] = (cell(s) + T[s][state]) + lpEmit(present cell) - lane s holds w[s], the states of a cell being NS planes at one slot -
// then picks the first maximal one (best) or draws one with random_key_log (src/util.h:220-236) from the next 32-bit word.
// A lattice L gives: Job, NS, ND (columns of T, the last one End), END, column(), Emit (where lpEmit's terms lie), self_loop().
// One wavefront per job.  A step is one round trip to memory - the source cell's states and the present cell's emission
// term are independent loads issued together - and that latency is what a walk costs: the arithmetic behind it (NS lane
// reads, one exp per lane, two passes of NS additions) is wave-uniform and short.
struct PairWalkIO {
  const uint32_t* words;        // sampled walks: the engine's words of all jobs, job k's at word_off[k] .. word_off[k + 1]
  const int64_t* word_off;      // [n_jobs + 1]
  uint8_t* states;              // [n_jobs][cap] the state chosen at every step, End side first
  int64_t cap;
  int32_t* n_steps;             // [n_jobs] steps taken, or < 0: the walk failed (historian_hip.h)
  int32_t* words_used;          // [n_jobs] (sampled walks)
};

template <class L, bool BEST>
__global__ void __launch_bounds__(64) k_pair_walk(const typename L::Job* __restrict__ jobs, const int job0, const PairWalkIO o) {
  constexpr int NS = L::NS, ND = L::ND;
  __shared__ double Tl[NS * ND];
  const int k = job0 + (int)blockIdx.x;
  const typename L::Job& J = jobs[k];
  const int lane = threadIdx.x;
  for (int q = lane; q < NS * ND; q += 64) Tl[q] = J.T[q / ND][q % ND];
  __syncthreads();
  uint8_t* out = o.states + (int64_t)k * o.cap;
  const uint32_t* words = BEST ? nullptr : o.words + o.word_off[k];
  const int64_t n_words = BEST ? 0 : o.word_off[k + 1] - o.word_off[k];
  const int64_t plane = J.plane, ss = J.strip_stride;
  const typename L::Emit em(J);                       // (where the emission terms lie: read once, not at every step)
  const double* const nowhere = J.lp_end;
  const HX_GLOBAL double* const cells = as_global((const double*)J.cells);
  int i = J.X - 1, j = J.Y - 1, state = L::END;
  int n = 0, code = 0;
  int64_t used = 0;
  if (!(*J.lp_end > HX_NEG_INF)) code = -1;
  while (code == 0 && (i > 0 || j > 0)) {
    bool dx, dy;
    L::column(i, j, state, dx, dy);
    if (!BEST && L::self_loop(state)) {
      // the geometric draw of the self-loop the fill eliminated: two words, the host's to interpret
      if (used + 2 > n_words) { code = -6; break; }
      used += 2;
    }
    const int si = i - (dx ? 1 : 0), sj = j - (dy ? 1 : 0);
    if (si < 0 || sj < 0) { code = -2; break; }       // (a state that emits what is not there: its cell is -inf, nothing chooses it)
    // the step's loads - the source cell's states, one per lane, the present cell's emission term and the step's word - are
    // independent and issued together, without a branch between them: one round trip per step
    const double* ep = nowhere;                        // (somewhere valid when the state emits nothing)
    double e = em.from(i, j, state, ep);               // ep: where the term is, if anywhere; e: what it is otherwise
    const bool loaded = ep != nowhere;
    const double v = cells[(lane < NS ? lane : 0) * plane + cell_slot(ss, si, sj)];
    const double el = *as_global(ep);
    const uint32_t word = (!BEST && used < n_words) ? as_global(words)[used] : 0u;
    e = loaded ? el : e;
    const double w = lane < NS ? (v + Tl[lane * ND + state]) + e : HX_NEG_INF;
    int pick = -1;
    if (BEST) {
      double best = HX_NEG_INF;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double ws = read_lane64(w, s);
        if (ws > best) { best = ws; pick = s; }
      }
      if (pick < 0) { code = -2; break; }
    } else {
      double top = HX_NEG_INF;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double ws = read_lane64(w, s);
        top = ws > top ? ws : top;
      }
      if (!(top > HX_NEG_INF)) { code = -2; break; }
      if (used >= n_words) { code = -6; break; }
      const double p = lane < NS ? exp(w - top) : 0.0;
      double norm = 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) norm += read_lane64(p, s);
      ++used;
      double variate = ((double)word / 4294967296.0) * norm;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        variate -= read_lane64(p, s);
        if (pick < 0 && variate <= 0) pick = s;
      }
      if (pick < 0) { code = -5; break; }
    }
    if (n >= o.cap) { code = -3; break; }
    if (lane == 0) out[n] = (uint8_t)pick;
    ++n;
    i = si; j = sj; state = __builtin_amdgcn_readfirstlane(pick);      // (wave-uniform: coordinates and state stay scalar)
  }
  if (lane == 0) {
    o.n_steps[k] = code ? code : n;
    if (!BEST) o.words_used[k] = (int32_t)used;
  }
}

// cells along a path: value of (xpos, ypos, state) and logMatch(xpos, ypos) for a list of coordinates the host has checked
template <class Job>
__global__ void k_pair_gather(const Job* __restrict__ jobs, const int job, const int64_t n, const hx_pair_cell* __restrict__ at,
                              double* __restrict__ cells, double* __restrict__ log_match) {
  const Job& J = jobs[job];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const hx_pair_cell c = at[q];
    const int64_t sl = cell_slot(J.strip_stride, c.xpos, c.ypos);
    cells[q] = J.cells[c.state * J.plane + sl];
    if (log_match) log_match[q] = (c.xpos > 0 && c.ypos > 0 && pair_in_env(J, c.xpos, c.ypos)) ? J.emis[sl] : HX_NEG_INF;
  }
}

int api_fail(int code, const char* what);                  // hx_api.hip

// device buffers of one call, freed when it returns
struct PairScratch {
  std::vector<void*> p;
  ~PairScratch() { for (void* q : p) (void)hipFree(q); }
  template <class T> T* get(const size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(T) * (n ? n : 1)) != hipSuccess) return nullptr;
    p.push_back(q);
    return static_cast<T*>(q);
  }
};

// hx_*_batch_best_paths / hx_*_batch_sample_paths
template <class L, bool BEST, class Batch>
int pair_walk_paths(Batch* b, const uint32_t* words, const int64_t* word_off, uint8_t* states, const int64_t cap, int32_t* n_steps,
                    int32_t* words_used) {
  if (!b || !states || !n_steps || cap < 1 || (!BEST && (!word_off || !words_used)))
    return api_fail(HX_ERR_INVALID_ARG, "pair walk: bad arguments");
  if (!b->done) return api_fail(HX_ERR_STATE, "pair walk: the batch has not been run");
  const int n = b->n_jobs;
  int64_t n_words = 0;
  if (!BEST) {
    if (word_off[0] < 0) return api_fail(HX_ERR_INVALID_ARG, "pair walk: word_off must start at or above 0");
    for (int k = 0; k < n; ++k)
      if (word_off[k + 1] < word_off[k]) return api_fail(HX_ERR_INVALID_ARG, "pair walk: word_off must not decrease");
    n_words = word_off[n];
    if (n_words > 0 && !words) return api_fail(HX_ERR_INVALID_ARG, "pair walk: words is null");
  }
  if (hipSetDevice(b->device) != hipSuccess) return api_fail(HX_ERR_HIP, "hipSetDevice failed");
  PairScratch sc;
  PairWalkIO o{};
  o.cap = cap;
  o.states = sc.get<uint8_t>((size_t)n * cap);
  o.n_steps = sc.get<int32_t>(n);
  uint32_t* d_words = BEST ? nullptr : sc.get<uint32_t>((size_t)n_words);
  int64_t* d_off = BEST ? nullptr : sc.get<int64_t>((size_t)n + 1);
  o.words_used = BEST ? nullptr : sc.get<int32_t>(n);
  o.words = d_words;
  o.word_off = d_off;
  if (!o.states || !o.n_steps || (!BEST && (!d_words || !d_off || !o.words_used)))
    return api_fail(HX_ERR_OUT_OF_MEMORY, "pair walk: device allocation failed");
  if (!BEST && ((n_words && hipMemcpy(d_words, words, sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice) != hipSuccess) ||
                hipMemcpy(d_off, word_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice) != hipSuccess))
    return api_fail(HX_ERR_HIP, "pair walk: copy to the device failed");
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess &&
                     hipEventRecord(ev[0], b->last_stream) == hipSuccess;
  for (int j0 = 0; j0 < n; j0 += 65536) {
    const int m = n - j0 < 65536 ? n - j0 : 65536;
    hipLaunchKernelGGL((k_pair_walk<L, BEST>), dim3(m), dim3(64), 0, b->last_stream, b->d_jobs, j0, o);
  }
  b->walk_ms = -1.f;
  if (timed && hipEventRecord(ev[1], b->last_stream) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess)
    (void)hipEventElapsedTime(&b->walk_ms, ev[0], ev[1]);
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess ||
      hipMemcpy(states, o.states, (size_t)n * cap, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(n_steps, o.n_steps, sizeof(int32_t) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      (!BEST && hipMemcpy(words_used, o.words_used, sizeof(int32_t) * n, hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "pair walk: HIP call failed");
  return HX_OK;
}

// hx_*_batch_last_walk_ms
template <class Batch>
int pair_last_walk_ms(const Batch* b, float* ms) {
  if (!b || !ms) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
  if (b->walk_ms < 0) return api_fail(HX_ERR_STATE, "no walk has run on the batch");
  *ms = b->walk_ms;
  return HX_OK;
}

// hx_*_batch_read_cells
template <int NS, class Batch>
int pair_read_cells(Batch* b, const int32_t job, const int64_t n, const hx_pair_cell* at, double* cells, double* log_match) {
  if (!b || n < 0 || (n && (!at || !cells))) return api_fail(HX_ERR_INVALID_ARG, "read_cells: bad arguments");
  if (job < 0 || job >= b->n_jobs) return api_fail(HX_ERR_RANGE, "job out of range");
  if (!b->done) return api_fail(HX_ERR_STATE, "read_cells: the batch has not been run");
  const auto& J = b->jobs[job];
  for (int64_t q = 0; q < n; ++q)
    if (at[q].xpos < 0 || at[q].xpos >= J.X || at[q].ypos < 0 || at[q].ypos >= J.Y || at[q].state < 0 || at[q].state >= NS)
      return api_fail(HX_ERR_RANGE, "read_cells: a coordinate outside the matrix");
  if (n == 0) return HX_OK;
  if (hipSetDevice(b->device) != hipSuccess) return api_fail(HX_ERR_HIP, "hipSetDevice failed");
  PairScratch sc;
  hx_pair_cell* d_at = sc.get<hx_pair_cell>((size_t)n);
  double* d_cells = sc.get<double>((size_t)n);
  double* d_lm = log_match ? sc.get<double>((size_t)n) : nullptr;
  if (!d_at || !d_cells || (log_match && !d_lm)) return api_fail(HX_ERR_OUT_OF_MEMORY, "read_cells: device allocation failed");
  if (hipMemcpy(d_at, at, sizeof(hx_pair_cell) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
    return api_fail(HX_ERR_HIP, "read_cells: copy to the device failed");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_pair_gather<std::remove_cv_t<std::remove_reference_t<decltype(J)>>>, dim3(blocks), dim3(256), 0, b->last_stream,
                     b->d_jobs, job, n, d_at, d_cells, d_lm);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess ||
      hipMemcpy(cells, d_cells, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
      (log_match && hipMemcpy(log_match, d_lm, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "read_cells: HIP call failed");
  return HX_OK;
}

}  // namespace hx
