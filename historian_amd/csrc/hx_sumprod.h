// What the column sum-product kernels share (hx_sumprod.hip: counts; hx_ancestors.hip: node posteriors; hx_history.hip:
// the resident history of the tree-height MCMC).  Device side: the 64-column block layout of the messages, the steps of
// the reference's tip-to-root pass (SumProduct::fillUp, src/sumprod.cpp:99-161: residue, wildcard, root) with its
// rescaling below 1e-30, the flow of the root-to-tip pass (fillDown, src/sumprod.cpp:163-198), the matrix-vector product
// with a matrix in LDS or behind the scalar cache, the column's root and the combination of the components' likelihoods.
// Every step exists once: the three kernels give the same bits wherever they run the same (TA, LM) form.  Host side: the
// launchers' prologue - model and tree checks, the device model block, the LDS plan, the chunk size, the event pair.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/historian_hip.h"
#include "hx_devmem.h"
#include "hx_lse.h"
#include "hx_policy.h"

namespace hx {

#define HX_SP_RESCALE 1e-30        // SUMPROD_RESCALE_THRESHOLD (src/sumprod.cpp:8)

// Model matrices are read through the constant address space: their addresses are uniform over the wavefront and
// nothing writes them, so the compiler fetches them with scalar loads and feeds the FMAs from SGPRs.
typedef const __attribute__((address_space(4))) double* CMat;
__device__ __forceinline__ CMat cmat(const double* p) { return (CMat)(unsigned long long)p; }

// Matrix-vector products with a matrix that a wave keeps in LDS (row-major, A x A, 16-byte aligned rows: A even).  Every
// lane reads the same entries (broadcast reads, two entries per ds_read_b128); half a row is fetched half a row ahead of
// its use into registers of its own, so that no read is waited for - written the plain way the compiler, short of
// registers, reused one register pair for every read and waited for each (one multiply-add per ~50 cycles).  Products
// with the transposed matrix (y = x M) use the same routine on a transposed LDS copy: one vector in registers, results
// handed out as they are complete - the kernel stays within 128 registers, four waves per SIMD.
typedef double sp_d2 __attribute__((ext_vector_type(2)));
template <int H>                                    // H entries (H even)
struct LdsPiece {
  sp_d2 v[H / 2];
  __device__ __forceinline__ void fetch(const HX_LDS double* p) {
#pragma unroll
    for (int q = 0; q < H / 2; ++q) v[q] = reinterpret_cast<const HX_LDS sp_d2*>(p)[q];
  }
  __device__ __forceinline__ double at(const int b) const { return (b & 1) ? v[b >> 1].y : v[b >> 1].x; }
};
// y[a] = sum_b M[a][b] x[b], handed out two rows at a time (A even), the way the scratch stores them; two partial sums per
// row and half (the additions do not wait for one another)
template <int A, class Emit>
__device__ __forceinline__ void lds_mat_vec(const HX_LDS double* M, const double (&x)[A], const Emit& emit) {
  constexpr int H0 = ((A / 2) + 1) & ~1, H1 = A - H0;      // a row in two pieces of even length (20 = 10 + 10, 4 = 2 + 2)
  static_assert(H1 >= 0 && (H1 & 1) == 0, "even alphabet sizes");
  LdsPiece<H0> lo;
  LdsPiece<(H1 > 0 ? H1 : 2)> hi;
  lo.fetch(M);
  double ya = 0.;
#pragma unroll
  for (int a = 0; a < A; ++a) {
    if (H1 > 0) hi.fetch(M + a * A + H0);
    double p0 = 0., p1 = 0.;
#pragma unroll
    for (int b = 0; b < H0; b += 2) {
      p0 = __builtin_fma(lo.at(b), x[b], p0);
      p1 = __builtin_fma(lo.at(b + 1), x[b + 1], p1);
    }
    if (a + 1 < A) lo.fetch(M + (a + 1) * A);
    if (H1 > 0) {
#pragma unroll
      for (int b = 0; b < H1; b += 2) {
        p0 = __builtin_fma(hi.at(b), x[H0 + b], p0);
        p1 = __builtin_fma(hi.at(b + 1), x[H0 + b + 1], p1);
      }
    }
    const double y = p0 + p1;
    if (a & 1) emit(a >> 1, ya, y);
    else ya = y;
  }
}

// ---- the column kernels' steps ----
// TA: the alphabet size as a compile-time constant (message vectors live in registers, loops unrolled), or 0 for any
// alphabet of up to 64 symbols (vectors in private memory).  LM: a wave keeps the matrix it multiplies with in LDS and reads
// its entries as broadcasts; without it they come through the scalar cache.  The row routine (lds_mat_vec, 16-byte
// accesses to the scratch) runs where sp_rows<TA>.
template <int TA> constexpr int sp_ax = TA ? TA : 64;
template <int TA> constexpr bool sp_rows = TA != 0 && TA % 2 == 0;

// the lanes of a wave hand values to one another through LDS: the writes have landed before the reads are issued
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// an A x A matrix into a wave's LDS; TR: transposed (y = x M through the row routine)
template <bool TR>
__device__ __forceinline__ void lds_stage(HX_LDS double* L, const double* __restrict__ g, const int A, const int lane) {
  for (int k = lane; k < A * A; k += 64) L[TR ? (k % A) * A + k / A : k] = g[k];
}

// A lane's view of one block of 64 columns.  Messages [block][cpt][node][a / 2][64][2]: a vector is stored two entries per
// lane and row, so that a lane moves 16 bytes per memory instruction (AP = A rounded up to even); scale factors
// [block][cpt][node][64].  Everything a wavefront touches in a pass lies in one contiguous stretch.
struct SpBlock {
  long long cb;                    // the block
  int C, N, AP, lane;
  __device__ __forceinline__ long long node(const int cpt, const int r) const { return (cb * C + cpt) * N + r; }
  template <class T> __device__ __forceinline__ T* row(T* P, const long long idx) const { return P + idx * (long long)(AP * 64) + lane * 2; }
  template <class T> __device__ __forceinline__ T& lg(T* P, const long long idx) const { return P[idx * 64 + lane]; }
};
template <class T> __device__ __forceinline__ T& sp_at(T* rp, const int a) { return rp[(a >> 1) * 128 + (a & 1)]; }

template <int TA, class Gen>
__device__ __forceinline__ void put_row(double* rp, const int A, Gen&& gen) {
  if constexpr (sp_rows<TA>) {
#pragma unroll
    for (int q = 0; q < TA / 2; ++q) *reinterpret_cast<sp_d2*>(rp + q * 128) = sp_d2{gen(2 * q), gen(2 * q + 1)};
  } else {
    for (int a = 0; a < A; ++a) sp_at(rp, a) = gen(a);
  }
}
// use(a, entry a of the row), a = 0 .. A - 1
template <int TA, class Use>
__device__ __forceinline__ void get_row(const double* rp, const int A, Use&& use) {
  if constexpr (sp_rows<TA>) {
#pragma unroll
    for (int q = 0; q < TA / 2; ++q) {
      const sp_d2 t2 = *reinterpret_cast<const sp_d2*>(rp + q * 128);
      use(2 * q, t2.x); use(2 * q + 1, t2.y);
    }
  } else {
    for (int a = 0; a < A; ++a) use(a, sp_at(rp, a));
  }
}

// v = the product of two message vectors, each all ones where absent (a gap, no child); -> its largest entry.  Vectors in
// registers: both are loaded, then multiplied.  Vectors in private memory (TA = 0): a second one would be 512 bytes of
// scratch per lane, so the product is taken in place and an absent vector is not multiplied with (its factor 1 is exact:
// the same bits).
template <int TA>
__device__ __forceinline__ double row_product(const bool h0, const double* r0, const bool h1, const double* r1, const int A, double (&v)[sp_ax<TA>]) {
  double vmax = 0.;
  if constexpr (TA == 0) {
    for (int a = 0; a < A; ++a) v[a] = 1.;
    if (h0) get_row<TA>(r0, A, [&](const int a, const double e) { v[a] = e; });
    if (h1) get_row<TA>(r1, A, [&](const int a, const double e) { v[a] *= e; });
    for (int a = 0; a < A; ++a) vmax = v[a] > vmax ? v[a] : vmax;
  } else {
    double e1[TA];
#pragma unroll
    for (int a = 0; a < TA; ++a) v[a] = e1[a] = 1.;
    if (h0) get_row<TA>(r0, A, [&](const int a, const double e) { v[a] = e; });
    if (h1) get_row<TA>(r1, A, [&](const int a, const double e) { e1[a] = e; });
#pragma unroll
    for (int a = 0; a < TA; ++a) {
      v[a] *= e1[a];
      vmax = v[a] > vmax ? v[a] : vmax;
    }
  }
  return vmax;
}

// The way up at a residue tk: F is one-hot, the product of the children's entries tk (h0, h1: the child sends a message),
// rescaled as the reference does (src/sumprod.cpp:135-138); the logarithm of a factor taken out is added to lf.  -> F[tk]
__device__ __forceinline__ double residue_f(const bool h0, const double* r0, const bool h1, const double* r1, const int tk, double& lf) {
  double f = (h0 ? sp_at(r0, tk) : 1.) * (h1 ? sp_at(r1, tk) : 1.);
  if (f < HX_SP_RESCALE) { lf += log(f); f = 1.; }
  return f;
}
// The way up at a wildcard: F is the product of the children's messages, rescaled as the reference does
// (src/sumprod.cpp:120-124).  -> the largest entry of F (1 after a rescaling)
template <int TA>
__device__ __forceinline__ double wild_f(const bool h0, const double* r0, const bool h1, const double* r1, const int A, double (&f)[sp_ax<TA>], double& lf) {
  const double fmax = row_product<TA>(h0, r0, h1, r1, A, f);
  if (fmax < HX_SP_RESCALE) {
#pragma unroll
    for (int a = 0; a < A; ++a) f[a] /= fmax;
    lf += log(fmax);
    return 1.;
  }
  return fmax;
}
// the component's likelihood of a column whose root is a wildcard
template <int TA>
__device__ __forceinline__ double wild_root_ll(const double (&f)[sp_ax<TA>], const CMat ins, const int A, const double lf) {
  double ip = 0.;
#pragma unroll
  for (int a = 0; a < A; ++a) ip += f[a] * ins[a];
  return lf + log(ip);
}

// rp[a] = out(a, y[a]), y = M x (TR: y = x M).  With LM the matrix is L, in a wave's LDS - staged transposed for TR where
// the row routine runs; without, g behind the scalar cache.  The row routine and the loop add in different orders: every
// (TA, LM) form has its own bits.
template <int TA, bool LM, bool TR, class Out>
__device__ __forceinline__ void mat_vec_store(const HX_LDS double* L, const CMat g, const int A, const double (&x)[sp_ax<TA>], double* rp, const Out& out) {
  if constexpr (LM && sp_rows<TA>) {
    lds_mat_vec<TA>(L, x, [&](const int q, const double ya, const double yb) { *reinterpret_cast<sp_d2*>(rp + q * 128) = sp_d2{out(2 * q, ya), out(2 * q + 1, yb)}; });
  } else {
#pragma unroll
    for (int a = 0; a < A; ++a) {
      double y = 0.;
#pragma unroll
      for (int b = 0; b < A; ++b) y += (LM ? L[TR ? b * A + a : a * A + b] : g[TR ? b * A + a : a * A + b]) * x[b];
      sp_at(rp, a) = out(a, y);
    }
  }
}
template <int TA, bool LM, bool TR>
__device__ __forceinline__ void mat_vec_store(const HX_LDS double* L, const CMat g, const int A, const double (&x)[sp_ax<TA>], double* rp) {
  mat_vec_store<TA, LM, TR>(L, g, A, x, rp, [](int, const double y) { return y; });
}

// the root of a column in [column][node] tokens (-2: a gap): the ungapped node whose parent is a gap or absent (one per
// column: the caller's contract), -1 in a column of gaps
__device__ __forceinline__ int column_root(const signed char* t, const int* parent, const int N) {
  int root = -1;
  for (int r = 0; r < N; ++r)
    if (t[r] != -2 && (parent[r] < 0 || t[parent[r]] == -2)) root = r;
  return root;
}
// the column's likelihood: the components' ([C][64] in LDS), combined in component order with the table log_sum_exp
__device__ __forceinline__ double combine_components(const double* sh_ll, const double* log_cpt_weight, const int C, const int lane, const double* lse_tab) {
  double cll = HX_NEG_INF;
  for (int cpt = 0; cpt < C; ++cpt) cll = lse(cll, log_cpt_weight[cpt] + sh_ll[cpt * 64 + lane], lse_tab);
  return cll;
}

// ---- the launchers' prologue ----
extern thread_local float g_sp_ms;             // hx_sumprod.hip: what hx_sumprod_last_kernel_ms reports
const double* device_lse_table(int device);    // hx_api.hip: the 8-byte log_sum_exp table of an initialised device, or null
int api_fail(int code, const char* what);       // hx_api.hip: sets hx_last_error()

inline int sp_fail(const int code, const char* fn, const char* what) { return api_fail(code, (std::string(fn) + ": " + what).c_str()); }

// The model's sizes, the current device and its log_sum_exp table.  size_code: what an alphabet or a mixture too large is.
inline int sp_check_model(const char* fn, const bool complete, const int A, const int C, const int size_code, int* device, const double** lse_tab) {
  if (!complete) return sp_fail(HX_ERR_INVALID_ARG, fn, "incomplete model");
  if (A > 64) return sp_fail(size_code, fn, "alphabets of more than 64 symbols are not supported");
  if (C > 128) return sp_fail(size_code, fn, "more than 128 mixture components are not supported");
  if (hipGetDevice(device) != hipSuccess) return api_fail(HX_ERR_NO_DEVICE, "no HIP device");
  *lse_tab = device_lse_table(*device);
  if (!*lse_tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the current device");
  return HX_OK;
}
// Children from parents: a binary tree, children before parents.  root_last: the last node is the root and the only one.
// third_code: what a third child is.
inline int sp_children(const char* fn, const int* parent, const int N, const bool root_last, const int third_code, std::vector<int>& child) {
  child.assign(2 * (size_t)N, -1);
  for (int r = 0; r < N; ++r) {
    const int p = parent[r];
    if (root_last && r == N - 1) {
      if (p >= 0) return sp_fail(HX_ERR_NOT_TOPOSORTED, fn, "the last node is not the root");
      continue;
    }
    if (!root_last && p < 0) continue;
    if (p <= r || p >= N) return sp_fail(HX_ERR_NOT_TOPOSORTED, fn, root_last ? "a node precedes its child, or a second root" : "a node precedes its child");
    if (child[2 * p] < 0) child[2 * p] = r;
    else if (child[2 * p + 1] < 0) child[2 * p + 1] = r;
    else return sp_fail(third_code, fn, "a node has more than two children");
  }
  return HX_OK;
}
// tokens index the alphabet on the device: refuse anything else on the host, not with a fault there
inline bool sp_token_ok(const int8_t t, const int A) { return t >= -2 && t < A; }
inline int sp_check_tokens(const char* fn, const int8_t* tokens, const int64_t n, const int A) {
  for (int64_t k = 0; k < n; ++k)
    if (!sp_token_ok(tokens[k], A)) return sp_fail(HX_ERR_RANGE, fn, "a token outside -2 .. alphabet size - 1");
  return HX_OK;
}

// The model on the device: one allocation, filled front to back (every piece 16-byte aligned).
struct SpUpload {
  DevBuf buf;
  char* q = nullptr;
  bool copied = true;
  static size_t room(const size_t bytes) { return (bytes + 15) & ~(size_t)15; }
  bool alloc(const size_t bytes) { return buf.alloc(bytes) && (q = buf.as<char>()); }
  template <class T> T* reserve(const size_t n) {
    T* at = reinterpret_cast<T*>(q);
    q += room(n * sizeof(T));
    return at;
  }
  template <class T> T* put(const T* src, const size_t n) {
    T* at = reserve<T>(n);
    copied = copied && hipMemcpy(at, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    return at;
  }
};
// what every column kernel reads: the tree and the mixture.  Bytes: sp_tree_room; branch_sub (or null) goes with it
struct SpTree { const int* parent; const int* child; const double* ins_prob; const double* log_cpt_weight; const double* branch_sub; };
inline size_t sp_tree_room(const int A, const int C, const int N, const bool with_sub) {
  return SpUpload::room(N * sizeof(int)) + SpUpload::room(2 * (size_t)N * sizeof(int)) + SpUpload::room((size_t)C * A * sizeof(double)) +
         SpUpload::room(C * sizeof(double)) + (with_sub ? SpUpload::room((size_t)C * N * A * A * sizeof(double)) : 0);
}
inline SpTree sp_put_tree(SpUpload& up, const int A, const int C, const int N, const int* parent, const std::vector<int>& child, const double* ins_prob,
                          const double* log_cpt_weight, const double* branch_sub) {
  SpTree t;
  t.parent = up.put(parent, N);
  t.child = up.put(child.data(), 2 * (size_t)N);
  t.ins_prob = up.put(ins_prob, (size_t)C * A);
  t.log_cpt_weight = up.put(log_cpt_weight, C);
  t.branch_sub = branch_sub ? up.put(branch_sub, (size_t)C * N * A * A) : nullptr;
  return t;
}

// The column kernel's workgroup: a wave per mixture component, up to eight; in LDS the components' likelihoods ([C][64])
// and, if they fit 96 KB with them, `mats` A x A matrices per wave (lm).  shed_waves: waves are given up until the matrices
// fit (one wave's do: 64 KB + 32 KB) - the history's kernel has no form without them.
struct SpPlan { int waves; bool lm; size_t lds; };
inline SpPlan sp_column_plan(const int A, const int C, const int mats, const bool shed_waves) {
  const size_t ll_lds = sizeof(double) * 64 * (size_t)C, mat_lds = sizeof(double) * mats * (size_t)A * A;
  SpPlan p;
  p.waves = C < 8 ? C : 8;
  while (shed_waves && p.waves > 1 && ll_lds + p.waves * mat_lds > 96 * 1024) --p.waves;
  p.lm = ll_lds + p.waves * mat_lds <= 96 * 1024;
  p.lds = ll_lds + (p.lm ? p.waves * mat_lds : 0);
  return p;
}
// columns per chunk: the scratch of a chunk (per_col doubles a column) stays within the budget (HX_SUMPROD_SCRATCH_MB,
// default 16 GiB); whole blocks of 64 columns
inline long long sp_chunk(const size_t per_col, const long long n_cols) {
  size_t budget = (size_t)16 << 30;
  if (const char* e = getenv("HX_SUMPROD_SCRATCH_MB")) budget = (size_t)atoll(e) << 20;
  long long chunk = (long long)(budget / (per_col * sizeof(double)));
  chunk &= ~63LL;
  if (chunk < 64) chunk = 64;
  return chunk > n_cols ? n_cols : chunk;
}

}  // namespace hx
