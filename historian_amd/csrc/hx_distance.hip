// Maximum-likelihood pairwise distances on the device: RateModel::distanceMatrix (reference src/model.cpp:506-655).
//
// One wavefront owns one pair of alignment rows and runs DistanceMatrixParams::tML for it from start to end: the
// bracket test at tJC, the four-step scan, and GSL's golden-section iteration (restated from its published
// min/golden.c and min/convergence.c; GSL is not among the reference's sources).  Every value the control flow
// looks at is computed by all lanes from the same operands in the same order, so every branch is wave-uniform.
//
// f(t) = -sum_ab n_ab log(sum_c w_c exp(R_c t)[a][b]).  exp(R t) is gsl_linalg_exponential_ss as the host mirror's
// RateModel::getSubProbMatrix restates it: scale by 2^-j, a k-term series in Horner form, j squarings, (k, j) by the
// largest |element| of R t.  The A x A matrices live in LDS; a lane owns the entries lane, lane + 64, ... of a
// product and accumulates each over the inner index in increasing order, multiply and add rounded separately (the
// file is built with -ffp-contract=off), skipping a zero left factor - the host's operations in the host's order, so
// exp(R t) has the host's bits.  log(p_ab) is taken by the lanes in parallel; the terms are then added by one serial
// pass in (a, b) order over the non-zero counts, the order of the reference's std::map.  No floating-point atomics.
//
// tJC needs one log per pair.  It is taken on the host, from the (same, different) column counts that a first small
// kernel returns, so that the search starts from the host's bits and the log inside f is the only operation whose
// rounding can differ from a host run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/historian_hip.h"
#include "hx_devmem.h"

namespace hx {
namespace {

constexpr int kShrinkEntries = 1100;     // squarings <= 14 + ceil(log2(1.01 * DBL_MAX / 1000)) < 1100

struct DistModel {
  int A, C;
  const double* rate;      // [C][A][A]
  const double* weight;    // [C]
  const double* shrink;    // [kShrinkEntries] 1 / exp(log(2) s) by the host's libm, as getSubProbMatrix computes it
};

__device__ inline double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// (terms, squarings): the double-precision row of the table in GSL's linalg/exponential.c
__device__ inline void series_shape(double norm, int& terms, int& squarings) {
  if (norm < 0.01) { terms = 5; squarings = 1; }
  else if (norm < 0.1) { terms = 5; squarings = 4; }
  else if (norm < 1.) { terms = 7; squarings = 5; }
  else if (norm < 10.) { terms = 9; squarings = 7; }
  else if (norm < 100.) { terms = 10; squarings = 10; }
  else if (norm < 1000.) { terms = 8; squarings = 14; }
  else { terms = 8; squarings = 14 + (int)ceil(log(1.01 * norm / 1000.) / log(2.)); }
}

// The likelihood evaluation of one wavefront.  R = entries of an A x A matrix per lane.
template <int R>
struct Eval {
  DistModel m;
  int AA;
  double* Bm;       // LDS [AA]: R t / 2^j; then the terms log(p_ab)
  double* Em;       // LDS [AA]: the running series / power
  const int* cnt;   // LDS [AA]: n_ab
  int row[R], col[R], ent[R];   // row * A, column and index of the lane's entries (0 for an entry past the matrix)
  bool live[R], diag[R];
  int evaluations;
  int products;     // A x A matrix products taken so far (what a flop count multiplies by 2 A^3)

  __device__ void init(const DistModel& model, double* bm, double* em, const int* counts) {
    m = model; AA = m.A * m.A; Bm = bm; Em = em; cnt = counts; evaluations = 0; products = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = (int)threadIdx.x + 64 * r;
      live[r] = e < AA;
      const int i = live[r] ? e / m.A : 0, j = live[r] ? e % m.A : 0;
      row[r] = i * m.A; col[r] = j; ent[r] = live[r] ? e : 0;
      diag[r] = live[r] && i == j;
    }
  }

  // acc = P Q, inner index increasing, product and sum rounded separately, a zero left factor skipped
  __device__ void matmul(const double* P, const double* Q, double (&acc)[R]) const {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.;
    for (int k = 0; k < m.A; ++k) {
      const double* qk = Q + k * m.A;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double p = P[row[r] + k];
        const double s = acc[r] + p * qk[col[r]];
        acc[r] = p != 0. ? s : acc[r];
      }
    }
  }

  __device__ void store(double* M, const double (&v)[R]) const {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) M[ent[r]] = v[r];
  }

  __device__ double f(double t) {
    ++evaluations;
    double p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = 0.;
    for (int c = 0; c < m.C; ++c) {
      const double* rc = m.rate + (size_t)c * AA;
      double b[R], acc[R];
      double norm = 0.;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        b[r] = live[r] ? rc[ent[r]] * t : 0.;
        norm = fmax(norm, fabs(b[r]));
      }
      norm = wave_max(norm);
      if (!(norm < std::numeric_limits<double>::infinity())) return std::numeric_limits<double>::quiet_NaN();
      int terms, squarings;
      series_shape(norm, terms, squarings);
      products += terms - 1 + squarings;
      const double shrink = m.shrink[squarings < kShrinkEntries ? squarings : kShrinkEntries - 1];
      const double first = 1. / terms;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        b[r] *= shrink;
        acc[r] = b[r] * first;
        if (diag[r]) acc[r] += 1.;
      }
      store(Bm, b);
      store(Em, acc);
      __syncthreads();
      for (int count = terms - 1; count >= 1; --count) {
        matmul(Bm, Em, acc);
        __syncthreads();
        const double inv = 1. / count;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          acc[r] *= inv;
          if (diag[r]) acc[r] += 1.;
        }
        store(Em, acc);
        __syncthreads();
      }
      for (int s = 0; s < squarings; ++s) {
        matmul(Em, Em, acc);
        __syncthreads();
        store(Em, acc);
        __syncthreads();
      }
      const double w = m.weight[c];
#pragma unroll
      for (int r = 0; r < R; ++r) p[r] += w * acc[r];
    }
    // the terms in parallel, their sum in one fixed order
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) Bm[ent[r]] = cnt[ent[r]] != 0 ? log(p[r]) : 0.;
    __syncthreads();
    double ll = 0.;
    for (int e = 0; e < AA; ++e) {
      const int n = cnt[e];
      if (n != 0) ll += Bm[e] * (double)n;
    }
    __syncthreads();
    return -ll;
  }
};

// DistanceMatrixParams::tML from the clamped tJC on (src/model.cpp:587-655).  The reference's nested loops are laid
// out as one loop around a single evaluation (the evaluation is then inlined once and its index tables stay in
// registers); `phase` says which of the reference's call sites the value belongs to.
template <int R>
__device__ double search(Eval<R>& ev, double tjc, int max_iterations) {
  const double tMin = 1e-9, tMax = 10;
  const double tLower = tMin < tjc / 2 ? tMin : tjc / 2;        // std::min(tMin, tjc / 2)
  const double tUpper = tMax < tjc * 2 ? tjc * 2 : tMax;        // std::max(tMax, tjc * 2)
  const double golden = 0.3819660;                              // GSL's literal
  enum { AtLower, AtUpper, AtJC, Scan, Golden } phase = AtLower;
  double llLower = 0., llUpper = 0., f_min = 0.;
  double lo = tLower, hi = tUpper, step = 0.;                   // the scan's window
  double x_min = tjc, x_lo = tLower, x_up = tUpper;             // the minimiser's state
  int iter = 0;
  double x = tLower;
  for (;;) {
    const double v = ev.f(x);
    if (phase == AtLower) { llLower = v; x = tUpper; phase = AtUpper; continue; }
    if (phase == AtUpper) { llUpper = v; x = tjc; phase = AtJC; continue; }
    if (phase == Golden) {
      // gsl_min_fminimizer_goldensection's step; its GSL_FAILURE (neither branch) is ignored as the reference ignores it
      if (v < f_min) { x_min = x; f_min = v; }
      else if (x < x_min && v > f_min) x_lo = x;
      else if (x > x_min && v > f_min) x_up = x;
      // gsl_min_test_interval(a, b, 0, .01)
      const double al = fabs(x_lo), au = fabs(x_up);
      const bool same_sign = (x_lo > 0. && x_up > 0.) || (x_lo < 0. && x_up < 0.);
      const double tolerance = .01 * (same_sign ? (al < au ? al : au) : 0.);
      if (fabs(x_up - x_lo) < tolerance || ++iter >= max_iterations) return x_min;
    } else if (v < llLower && v < llUpper) {                    // AtJC or Scan: a point below both ends starts the minimiser
      x_min = x; f_min = v;
      phase = Golden;
    } else {
      if (phase == Scan) {
        x += step;
        if (x < hi) continue;
        if (llLower < llUpper) hi = (lo + hi) / 2;
        else lo = (lo + hi) / 2;
      }
      phase = Scan;
      if (!(hi - lo > tLower)) return llLower < llUpper ? tLower : tUpper;
      step = (hi - lo) / 4.;
      x = lo;
      continue;
    }
    const double w_lo = x_min - x_lo, w_up = x_up - x_min;
    x = x_min + golden * (w_up > w_lo ? w_up : -w_lo);
  }
}

// pair index in the order (0,1), (0,2) ... (n-2,n-1) -> rows
__device__ inline void pair_rows(long long p, int n, int& i, int& j) {
  const double b = 2. * n - 1.;
  long long r = (long long)((b - sqrt(b * b - 8. * (double)p)) / 2.);
  if (r < 0) r = 0;
  if (r > n - 2) r = n - 2;
  auto first = [n](long long row) { return row * n - row * (row + 1) / 2; };   // index of (row, row + 1)
  while (r > 0 && first(r) > p) --r;
  while (r < n - 2 && first(r + 1) <= p) ++r;
  i = (int)r;
  j = (int)(p - first(r)) + i + 1;
}

// columns in which both rows hold a residue: how many with the same one, how many with different ones
__global__ void __launch_bounds__(64) k_same_diff(const signed char* tok, int n_seqs, long long n_cols, int2* out) {
  int i, j;
  pair_rows(blockIdx.x, n_seqs, i, j);
  const signed char* x = tok + (size_t)i * n_cols;
  const signed char* y = tok + (size_t)j * n_cols;
  int same = 0, diff = 0;
  for (long long c = threadIdx.x; c < n_cols; c += 64) {
    const int a = x[c], b = y[c];
    if (a >= 0 && b >= 0) { same += a == b; diff += a != b; }
  }
  same = wave_sum(same);
  diff = wave_sum(diff);
  if (threadIdx.x == 0) out[blockIdx.x] = make_int2(same, diff);
}

template <int R>
__global__ void __launch_bounds__(64) k_distance_search(DistModel m, const signed char* tok, int n_seqs, long long n_cols,
                                                        const double* tjc, int max_iterations, double* dist, int* evaluations,
                                                        unsigned long long* products) {
  extern __shared__ double lds[];
  const int AA = m.A * m.A;
  double* Bm = lds;
  double* Em = lds + AA;
  int* cnt = reinterpret_cast<int*>(lds + 2 * AA);
  int i, j;
  pair_rows(blockIdx.x, n_seqs, i, j);
  for (int e = threadIdx.x; e < AA; e += 64) cnt[e] = 0;
  __syncthreads();
  const signed char* x = tok + (size_t)i * n_cols;
  const signed char* y = tok + (size_t)j * n_cols;
  for (long long c = threadIdx.x; c < n_cols; c += 64) {
    const int a = x[c], b = y[c];
    if (a >= 0 && b >= 0) atomicAdd(&cnt[a * m.A + b], 1);      // tokens < A: checked by the host before the launch
  }
  __syncthreads();
  Eval<R> ev;
  ev.init(m, Bm, Em, cnt);
  const double t = search(ev, tjc[blockIdx.x], max_iterations);
  if (threadIdx.x == 0) {
    dist[(size_t)i * n_seqs + j] = t;
    dist[(size_t)j * n_seqs + i] = t;
    if (evaluations) evaluations[blockIdx.x] = ev.evaluations;
    atomicAdd(products, (unsigned long long)ev.products);          // an integer sum: any order gives the same total
  }
}

template <int R>
__global__ void __launch_bounds__(64) k_distance_nll(DistModel m, const int* counts, const double* t, double* f) {
  extern __shared__ double lds[];
  const int AA = m.A * m.A;
  int* cnt = reinterpret_cast<int*>(lds + 2 * AA);
  for (int e = threadIdx.x; e < AA; e += 64) cnt[e] = counts[(size_t)blockIdx.x * AA + e];
  __syncthreads();
  Eval<R> ev;
  ev.init(m, lds, lds + AA, cnt);
  const double v = ev.f(t[blockIdx.x]);
  if (threadIdx.x == 0) f[blockIdx.x] = v;
}

thread_local float g_dist_ms = 0.f;
thread_local long long g_dist_products = 0;

const std::vector<double>& shrink_table() {
  static const std::vector<double> tab = [] {
    std::vector<double> v(kShrinkEntries);
    for (int s = 0; s < kShrinkEntries; ++s) v[s] = 1. / exp(log(2.) * s);
    return v;
  }();
  return tab;
}

// RateModel::DistanceMatrixParams::tJC (src/model.cpp:570-582), clamped as tML clamps it (:586)
double clamped_tjc(int same, int diff, int alph, double expected_sub_rate) {
  const double tMin = 1e-9, tMax = 10;
  const double pDiff = diff / (double)(same + diff);           // 0 / 0 = NaN for a pair without a counted column
  const double A = (double)alph;
  const double tjc = pDiff >= (A - 1) / A ? std::numeric_limits<double>::infinity()
                                          : -((A - 1) / A) * log(1 - (A / (A - 1)) * pDiff) / expected_sub_rate;
  const double floored = tMin < tjc ? tjc : tMin;              // std::max(tMin, tjc): tMin for NaN
  return floored < tMax ? floored : tMax;                      // std::min(tMax, .)
}

}  // namespace

int api_fail(int code, const char* what);       // hx_api.hip: sets hx_last_error()

}  // namespace hx

using namespace hx;

namespace {

// the model's arrays on the device; false with `rc` set on failure
struct DeviceModel {
  DevBuf rate, weight, shrink;
  DistModel m;
  int upload(const hx_distance_model* hm, hipStream_t st) {
    const int A = hm->alph_size, C = hm->n_components;
    const size_t AA = (size_t)A * A;
    if (!rate.alloc(C * AA * sizeof(double)) || !weight.alloc(C * sizeof(double)) || !shrink.alloc(kShrinkEntries * sizeof(double)))
      return HX_ERR_OUT_OF_MEMORY;
    if (hipMemcpyAsync(rate.as<void>(), hm->sub_rate, C * AA * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(weight.as<void>(), hm->cpt_weight, C * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(shrink.as<void>(), shrink_table().data(), kShrinkEntries * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
      return HX_ERR_HIP;
    m.A = A; m.C = C;
    m.rate = rate.as<const double>();
    m.weight = weight.as<const double>();
    m.shrink = shrink.as<const double>();
    return HX_OK;
  }
};

int check_model(const hx_distance_model* hm, const char* who, char* msg, size_t cap) {
  if (!hm || !hm->sub_rate || !hm->cpt_weight) { snprintf(msg, cap, "%s: null model or model array", who); return HX_ERR_INVALID_ARG; }
  if (hm->alph_size < 1 || hm->alph_size > 32) { snprintf(msg, cap, "%s: alphabet size %d outside 1 .. 32 (larger alphabets take the host path)", who, hm->alph_size); return HX_ERR_RANGE; }
  if (hm->n_components < 1) { snprintf(msg, cap, "%s: a model needs at least one mixture component", who); return HX_ERR_RANGE; }
  return HX_OK;
}

size_t lds_bytes(int A) { return (size_t)A * A * (2 * sizeof(double) + sizeof(int)); }

}  // namespace

extern "C" {

int hx_distance_matrix(const hx_distance_model* hm, const int8_t* tokens, int32_t n_seqs, int64_t n_cols, int32_t max_iterations,
                       double* dist, int32_t* evaluations, void* stream) {
  char msg[160];
  if (int rc = check_model(hm, "hx_distance_matrix", msg, sizeof msg)) return api_fail(rc, msg);
  if (!tokens || !dist || n_seqs < 2 || n_cols < 0)
    return api_fail(HX_ERR_INVALID_ARG, "hx_distance_matrix: null argument, fewer than two sequences or a negative number of columns");
  const int A = hm->alph_size;
  for (int64_t k = 0; k < (int64_t)n_seqs * n_cols; ++k)
    if (tokens[k] >= A) return api_fail(HX_ERR_RANGE, "hx_distance_matrix: a token outside the alphabet");
  const long long pairs = (long long)n_seqs * (n_seqs - 1) / 2;
  if (pairs > 0x7fffffffLL) return api_fail(HX_ERR_RANGE, "hx_distance_matrix: more pairs than one launch holds");
  hipStream_t st = static_cast<hipStream_t>(stream);
  g_dist_ms = 0.f;
  DeviceModel dm;
  if (int rc = dm.upload(hm, st)) return api_fail(rc, "hx_distance_matrix: device allocation or copy failed");
  DevBuf b_tok, b_sd, b_tjc, b_dist, b_ev, b_prod;
  g_dist_products = 0;
  if (!b_tok.alloc(n_cols ? (size_t)n_seqs * n_cols : 1) || !b_sd.alloc(pairs * sizeof(int2)) || !b_tjc.alloc(pairs * sizeof(double)) ||
      !b_dist.alloc((size_t)n_seqs * n_seqs * sizeof(double)) || !b_ev.alloc(pairs * sizeof(int)) || !b_prod.alloc(sizeof(unsigned long long)))
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_distance_matrix: device allocation failed");
  DevEvents<4> ev;
  if (!ev.create()) return api_fail(HX_ERR_HIP, "hx_distance_matrix: HIP call failed");
  if ((size_t)n_seqs * n_cols &&
      hipMemcpyAsync(b_tok.as<void>(), tokens, (size_t)n_seqs * n_cols, hipMemcpyHostToDevice, st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_matrix: copy failed");
  const signed char* d_tok = b_tok.as<const signed char>();
  (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL(k_same_diff, dim3((unsigned)pairs), dim3(64), 0, st, d_tok, n_seqs, (long long)n_cols, b_sd.as<int2>());
  (void)hipEventRecord(ev[1], st);
  std::vector<int2> sd(pairs);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(sd.data(), b_sd.as<void>(), pairs * sizeof(int2), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_matrix: counting kernel or copy failed");
  std::vector<double> tjc(pairs);
  for (long long p = 0; p < pairs; ++p) tjc[p] = clamped_tjc(sd[p].x, sd[p].y, A, hm->expected_sub_rate);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
  g_dist_ms = ms;
  if (max_iterations <= 0) {
    long long p = 0;
    for (int i = 0; i < n_seqs; ++i) {
      dist[(size_t)i * n_seqs + i] = 0.;
      for (int j = i + 1; j < n_seqs; ++j, ++p) dist[(size_t)i * n_seqs + j] = dist[(size_t)j * n_seqs + i] = tjc[p];
    }
    if (evaluations)
      for (long long q = 0; q < pairs; ++q) evaluations[q] = 0;
    return HX_OK;
  }
  if (hipMemcpyAsync(b_tjc.as<void>(), tjc.data(), pairs * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(b_dist.as<void>(), 0, (size_t)n_seqs * n_seqs * sizeof(double), st) != hipSuccess ||
      hipMemsetAsync(b_prod.as<void>(), 0, sizeof(unsigned long long), st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_matrix: copy failed");
  const int R = (A * A + 63) / 64;
  const size_t lds = lds_bytes(A);
  (void)hipEventRecord(ev[2], st);
#define HX_DIST_GO(R_) hipLaunchKernelGGL((k_distance_search<R_>), dim3((unsigned)pairs), dim3(64), lds, st, dm.m, d_tok, n_seqs, (long long)n_cols, \
                                          b_tjc.as<const double>(), max_iterations, b_dist.as<double>(), b_ev.as<int>(), \
                                          b_prod.as<unsigned long long>())
  if (R <= 1) HX_DIST_GO(1);
  else if (R <= 4) HX_DIST_GO(4);
  else if (R <= 7) HX_DIST_GO(7);
  else HX_DIST_GO(16);
#undef HX_DIST_GO
  (void)hipEventRecord(ev[3], st);
  unsigned long long products = 0;
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(dist, b_dist.as<void>(), (size_t)n_seqs * n_seqs * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
      (evaluations && hipMemcpyAsync(evaluations, b_ev.as<void>(), pairs * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipMemcpyAsync(&products, b_prod.as<void>(), sizeof products, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_matrix: search kernel or copy failed");
  (void)hipEventElapsedTime(&ms, ev[2], ev[3]);
  g_dist_ms += ms;
  g_dist_products = (long long)products;
  return HX_OK;
}

int hx_distance_neg_log_like(const hx_distance_model* hm, const int32_t* counts, const double* t, int32_t n, double* f, void* stream) {
  char msg[160];
  if (int rc = check_model(hm, "hx_distance_neg_log_like", msg, sizeof msg)) return api_fail(rc, msg);
  if (!counts || !t || !f || n < 1) return api_fail(HX_ERR_INVALID_ARG, "hx_distance_neg_log_like: null argument or nothing to evaluate");
  const int A = hm->alph_size;
  const size_t AA = (size_t)A * A;
  for (size_t k = 0; k < (size_t)n * AA; ++k)
    if (counts[k] < 0) return api_fail(HX_ERR_RANGE, "hx_distance_neg_log_like: a negative count");
  hipStream_t st = static_cast<hipStream_t>(stream);
  g_dist_ms = 0.f;
  DeviceModel dm;
  if (int rc = dm.upload(hm, st)) return api_fail(rc, "hx_distance_neg_log_like: device allocation or copy failed");
  DevBuf b_cnt, b_t, b_f;
  if (!b_cnt.alloc(n * AA * sizeof(int)) || !b_t.alloc(n * sizeof(double)) || !b_f.alloc(n * sizeof(double)))
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_distance_neg_log_like: device allocation failed");
  DevEvents<2> ev;
  if (!ev.create()) return api_fail(HX_ERR_HIP, "hx_distance_neg_log_like: HIP call failed");
  if (hipMemcpyAsync(b_cnt.as<void>(), counts, n * AA * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(b_t.as<void>(), t, n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_neg_log_like: copy failed");
  const int R = (A * A + 63) / 64;
  const size_t lds = lds_bytes(A);
  (void)hipEventRecord(ev[0], st);
#define HX_NLL_GO(R_) hipLaunchKernelGGL((k_distance_nll<R_>), dim3((unsigned)n), dim3(64), lds, st, dm.m, b_cnt.as<const int>(), \
                                         b_t.as<const double>(), b_f.as<double>())
  if (R <= 1) HX_NLL_GO(1);
  else if (R <= 4) HX_NLL_GO(4);
  else if (R <= 7) HX_NLL_GO(7);
  else HX_NLL_GO(16);
#undef HX_NLL_GO
  (void)hipEventRecord(ev[1], st);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(f, b_f.as<void>(), n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_distance_neg_log_like: kernel or copy failed");
  (void)hipEventElapsedTime(&g_dist_ms, ev[0], ev[1]);
  return HX_OK;
}

int hx_distance_last_products(int64_t* products) {
  if (!products) return HX_ERR_INVALID_ARG;
  *products = g_dist_products;
  return HX_OK;
}

int hx_distance_last_kernel_ms(float* ms) {
  if (!ms) return HX_ERR_INVALID_ARG;
  *ms = g_dist_ms;
  return HX_OK;
}

}  // extern "C"
