// The host side of the envelope-bounded pair DPs (hx_pairdp.h has the kernels): the step windows of a banded job's strips, the
// batch object behind hx_branch_batch_* and hx_sibling_batch_* - arena, device allocations, the launches of a step, results,
// dense copy - and the host halves of the walks and of the gather.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>
#include "hx_arena.h"
#include "hx_devmem.h"
#include "hx_pairdp.h"

namespace hx {

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

int api_fail(int code, const char* what);                  // hx_api.hip: sets hx_last_error()
const double* device_lse_table(int device);               // hx_api.hip: the table hx_init uploaded, or nullptr

// ---- the batch ---------------------------------------------------------------------------------------------------------------
// Envelope coordinates of a banded job into the batch's arena (hx_arena.h: 16-byte pieces) and, with `windows`, the step
// windows of its strips
template <class Job> void put_env(Arena& a, Job& J, const int32_t* x_env, const int32_t* y_env, bool windows) {
  if (J.max_dist < 0) return;
  a.put(J.x_env, x_env, (size_t)J.X);
  a.put(J.y_env, y_env, (size_t)J.Y);
  if (!windows) return;
  const std::vector<int32_t> w = branch_windows(x_env, y_env, J.X, J.Y, J.max_dist);
  a.put(J.win, w.data(), w.size());
}

// What hx_branch_batch and hx_sibling_batch are: n jobs of one lattice family resident on the device - inputs, NS state
// planes and an emission plane per job, lpEnd - and the C ABI's calls on them but for what a lattice validates and fills in
// itself.  The functions take the batch as the ABI passes it (possibly null).  Job::abi names the ABI's prefix in messages.
template <class Job, int NS>
struct PairBatch {
  int device = 0, n_jobs = 0;
  std::vector<Job> jobs;
  DevBuf d_jobs;                    // [n_jobs] Job
  DevBuf d_arena;                   // inputs + lpEnd, then what the jobs reserved
  DevBuf d_cells;                   // matrices + emission planes
  size_t lp_off = 0;
  int max_x = 0, max_y = 0;         // rows / columns of the longest job
  DevEvents<3> ev;                  // before the step, before the fill, after it
  Job* device_jobs() const { return d_jobs.template as<Job>(); }
  hipStream_t last_stream = nullptr;
  bool done = false;
  float walk_ms = -1.f;             // the walk kernel of the last best_paths / sample_paths (HIP events)

  static int fail(int code, const char* what) {       // (no allocation: called inside extern "C" entry points)
    char msg[192];
    snprintf(msg, sizeof(msg), "%s%s", Job::abi, what);
    return api_fail(code, msg);
  }

  ~PairBatch() { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }      // (the members release after it: nothing is in flight by then)

  // fill(J, abi_job, arena): validates one job of the ABI, sets X, Y, CA, C, max_dist and T and puts the job's arrays; returns
  // HX_OK or what api_fail returned
  template <class Batch, class AbiJob, class Fill>
  static int create(const AbiJob* abi_jobs, int32_t n_jobs, Batch** out, Fill fill) {
    if (out) *out = nullptr;
    if (!abi_jobs || !out || n_jobs < 1) return fail(HX_ERR_INVALID_ARG, "_create: need at least one job");
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return api_fail(HX_ERR_NO_DEVICE, "no HIP device");
    if (!device_lse_table(device)) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the current device");
    std::unique_ptr<Batch> b(new (std::nothrow) Batch);
    if (!b) return api_fail(HX_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->device = device;
    b->n_jobs = n_jobs;
    Arena a(16);
    int64_t cells_total = 0;
    try {
      b->jobs.resize(n_jobs);                       // (zeroed: what a job does not put stays null)
      for (int k = 0; k < n_jobs; ++k) {
        Job& J = b->jobs[k];
        if (const int rc = fill(J, abi_jobs[k], a)) return rc;
        J.strip_stride = strip_stride_for(J.Y);
        J.plane = (int64_t)((J.X + HX_STRIP - 1) / HX_STRIP) * J.strip_stride;
        cells_total += (NS + 1) * J.plane;
        b->max_x = std::max(b->max_x, (int)J.X);
        b->max_y = std::max(b->max_y, (int)J.Y);
      }
      b->lp_off = a.reserve(sizeof(double) * n_jobs);
    } catch (const std::bad_alloc&) {
      return api_fail(HX_ERR_OUT_OF_MEMORY, "host allocation failed while building the batch");
    }
    if (!b->d_arena.alloc(a.device_bytes()) || !b->d_cells.alloc(sizeof(double) * (size_t)cells_total) || !b->d_jobs.alloc(sizeof(Job) * n_jobs))
      return fail(HX_ERR_OUT_OF_MEMORY, "_create: device allocation failed");
    a.bind(b->d_arena.template as<char>());
    int64_t at = 0;
    for (int k = 0; k < n_jobs; ++k) {
      Job& J = b->jobs[k];
      J.cells = b->d_cells.template as<double>() + at;
      J.emis = J.cells + NS * J.plane;
      at += (NS + 1) * J.plane;
      J.lp_end = reinterpret_cast<double*>(b->d_arena.template as<char>() + b->lp_off) + k;
    }
    if (hipMemcpy(b->d_arena.template as<void>(), a.host.data(), a.host.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->d_jobs.template as<void>(), b->jobs.data(), sizeof(Job) * n_jobs, hipMemcpyHostToDevice) != hipSuccess || !b->ev.create())
      return fail(HX_ERR_HIP, "_create: copy to the device failed");
    *out = b.release();
    return HX_OK;
  }

  // one step: clearing, emission pre-pass and the fill of lattice L, on `stream`
  template <class L>
  static int run(PairBatch* b, void* stream) {
    static_assert(std::is_same<typename L::Job, Job>::value && L::NS == NS, "a lattice of this batch's jobs");
    if (!b) return api_fail(HX_ERR_INVALID_ARG, "batch is null");
    if (hipSetDevice(b->device) != hipSuccess) return api_fail(HX_ERR_HIP, "hipSetDevice failed");
    const double* tab = device_lse_table(b->device);
    if (!tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the batch's device");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipEventRecord(b->ev[0], st) != hipSuccess) return api_fail(HX_ERR_HIP, "hipEventRecord failed");
    for (int j0 = 0; j0 < b->n_jobs; j0 += 16384) {        // (grid.x of at most 16384 jobs per launch)
      const int n = b->n_jobs - j0 < 16384 ? b->n_jobs - j0 : 16384;
      hipLaunchKernelGGL((k_pair_clear<Job, NS>), dim3(n, 16), dim3(256), 0, st, b->device_jobs() + j0);
      hipLaunchKernelGGL(k_pair_emission<Job>, dim3(n, 16), dim3(256), 0, st, b->device_jobs() + j0, tab);
    }
    if (hipEventRecord(b->ev[1], st) != hipSuccess) return api_fail(HX_ERR_HIP, "hipEventRecord failed");
    for (int j0 = 0; j0 < b->n_jobs; j0 += 65536) {
      const int n = b->n_jobs - j0 < 65536 ? b->n_jobs - j0 : 65536;
      // wavefronts per job: as many as the longest job has strips, at most HXBR_MAX_WAVES (a workgroup of 1024) - fewer when
      // the batch alone fills the chip (L::BATCH_WAVES: what the lattice's register count lets the chip hold)
      int waves = (b->max_x + 63) / 64;
      waves = waves < 1 ? 1 : (waves > HXBR_MAX_WAVES ? HXBR_MAX_WAVES : waves);
      if (const char* e = getenv(L::WAVES_ENV)) { const int v = atoi(e); if (v >= 1 && v <= HXBR_MAX_WAVES) waves = v; }
      else while (waves > 1 && (int64_t)n * waves > L::BATCH_WAVES) waves = (waves + 1) / 2;
      // the column sides in LDS when the longest one fits (12 bytes per position beside the progress counters)
      const bool yl = (size_t)b->max_y * 12 <= 96 * 1024;
      const size_t dyn = yl ? (size_t)b->max_y * 12 + 16 : 0;
      const int y_cap = yl ? (b->max_y + 1) & ~1 : 0;
      if (yl) hipLaunchKernelGGL((k_pair_fill<L, true>), dim3(n), dim3(64 * waves), dyn, st, b->device_jobs() + j0, tab, y_cap);
      else hipLaunchKernelGGL((k_pair_fill<L, false>), dim3(n), dim3(64 * waves), 0, st, b->device_jobs() + j0, tab, 0);
    }
    if (hipEventRecord(b->ev[2], st) != hipSuccess || hipGetLastError() != hipSuccess) return fail(HX_ERR_HIP, "_run: launch failed");
    b->done = true;
    b->last_stream = st;
    return HX_OK;
  }

  static int results(PairBatch* b, double* lp_end) {
    if (!b || !lp_end) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
    if (!b->done) return fail(HX_ERR_STATE, "_run has not been launched");
    if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess ||
        hipMemcpy(lp_end, b->d_arena.template as<char>() + b->lp_off, sizeof(double) * b->n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(HX_ERR_HIP, "_results: HIP call failed");
    return HX_OK;
  }

  // the dense [X][Y][NS] matrix of one job
  static int read_matrix(PairBatch* b, int32_t job, double* out) {
    if (!b || !out) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
    if (job < 0 || job >= b->n_jobs) return api_fail(HX_ERR_RANGE, "job out of range");
    if (!b->done) return fail(HX_ERR_STATE, "_run has not been launched");
    const Job& J = b->jobs[job];
    const size_t bytes = sizeof(double) * NS * (size_t)J.X * J.Y;
    DevBuf dense;
    if (hipSetDevice(b->device) != hipSuccess || !dense.alloc(bytes))
      return fail(HX_ERR_OUT_OF_MEMORY, "_read_matrix: device allocation failed");
    hipLaunchKernelGGL((k_pair_dense<Job, NS>), dim3(256), dim3(256), 0, b->last_stream, b->device_jobs(), job, dense.as<double>());
    if (hipStreamSynchronize(b->last_stream) != hipSuccess || hipMemcpy(out, dense.as<double>(), bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(HX_ERR_HIP, "_read_matrix: HIP call failed");
    return HX_OK;
  }

  static int64_t total_cells(const PairBatch* b) {
    int64_t n = 0;
    if (b)
      for (const Job& J : b->jobs) n += (int64_t)J.X * J.Y;
    return n;
  }

  // the fill kernel(s) of the last run and, where asked for, the whole step
  static int last_kernel_ms(PairBatch* b, float* fill_ms, float* step_ms) {
    if (!b || !fill_ms) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
    if (!b->done) return fail(HX_ERR_STATE, "_run has not been launched");
    if (hipSetDevice(b->device) != hipSuccess || hipEventSynchronize(b->ev[2]) != hipSuccess ||
        hipEventElapsedTime(fill_ms, b->ev[1], b->ev[2]) != hipSuccess ||
        (step_ms && hipEventElapsedTime(step_ms, b->ev[0], b->ev[2]) != hipSuccess))
      return fail(HX_ERR_HIP, "_last_kernel_ms: HIP call failed");
    return HX_OK;
  }
};

// a device buffer of n elements (at least one byte: an address also for none), or null
template <class T> T* scratch(DevBuf& b, const size_t n) {
  return b.alloc(sizeof(T) * (n ? n : 1)) ? b.as<T>() : nullptr;
}

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
  DevBuf b_states, b_steps, b_words, b_off, b_used;
  PairWalkIO o{};
  o.cap = cap;
  o.states = scratch<uint8_t>(b_states, (size_t)n * cap);
  o.n_steps = scratch<int32_t>(b_steps, n);
  uint32_t* d_words = BEST ? nullptr : scratch<uint32_t>(b_words, (size_t)n_words);
  int64_t* d_off = BEST ? nullptr : scratch<int64_t>(b_off, (size_t)n + 1);
  o.words_used = BEST ? nullptr : scratch<int32_t>(b_used, n);
  o.words = d_words;
  o.word_off = d_off;
  if (!o.states || !o.n_steps || (!BEST && (!d_words || !d_off || !o.words_used)))
    return api_fail(HX_ERR_OUT_OF_MEMORY, "pair walk: device allocation failed");
  if (!BEST && ((n_words && hipMemcpy(d_words, words, sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice) != hipSuccess) ||
                hipMemcpy(d_off, word_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice) != hipSuccess))
    return api_fail(HX_ERR_HIP, "pair walk: copy to the device failed");
  DevEvents<2> ev;
  const bool timed = ev.create() && hipEventRecord(ev[0], b->last_stream) == hipSuccess;
  for (int j0 = 0; j0 < n; j0 += 65536) {
    const int m = n - j0 < 65536 ? n - j0 : 65536;
    hipLaunchKernelGGL((k_pair_walk<L, BEST>), dim3(m), dim3(64), 0, b->last_stream, b->device_jobs(), j0, o);
  }
  b->walk_ms = -1.f;
  if (timed && hipEventRecord(ev[1], b->last_stream) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess)
    (void)hipEventElapsedTime(&b->walk_ms, ev[0], ev[1]);
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
  using Job = std::remove_cv_t<std::remove_reference_t<decltype(b->jobs[job])>>;
  const Job& J = b->jobs[job];
  for (int64_t q = 0; q < n; ++q)
    if (at[q].xpos < 0 || at[q].xpos >= J.X || at[q].ypos < 0 || at[q].ypos >= J.Y || at[q].state < 0 || at[q].state >= NS)
      return api_fail(HX_ERR_RANGE, "read_cells: a coordinate outside the matrix");
  if (n == 0) return HX_OK;
  if (hipSetDevice(b->device) != hipSuccess) return api_fail(HX_ERR_HIP, "hipSetDevice failed");
  DevBuf b_at, b_cells, b_lm;
  hx_pair_cell* d_at = scratch<hx_pair_cell>(b_at, (size_t)n);
  double* d_cells = scratch<double>(b_cells, (size_t)n);
  double* d_lm = log_match ? scratch<double>(b_lm, (size_t)n) : nullptr;
  if (!d_at || !d_cells || (log_match && !d_lm)) return api_fail(HX_ERR_OUT_OF_MEMORY, "read_cells: device allocation failed");
  if (hipMemcpy(d_at, at, sizeof(hx_pair_cell) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
    return api_fail(HX_ERR_HIP, "read_cells: copy to the device failed");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_pair_gather<Job>, dim3(blocks), dim3(256), 0, b->last_stream, b->device_jobs(), job, n, d_at, d_cells,
                     d_lm);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess ||
      hipMemcpy(cells, d_cells, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
      (log_match && hipMemcpy(log_match, d_lm, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "read_cells: HIP call failed");
  return HX_OK;
}

}  // namespace hx
