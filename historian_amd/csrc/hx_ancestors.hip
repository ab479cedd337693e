// Ancestral sequence prediction (-ancseq, -ancprob): the residue posterior of EVERY node of every alignment column, and
// the most probable residue of every wildcard - the reference's SumProduct::logNodePostProb and maxPostState
// (src/sumprod.cpp:208-217, 259-262) behind AlignColSumProduct::appendAncestralReconstructedColumn and
// appendAncestralPostProbColumn (src/sumprod.cpp:401-426), for a BATCH of columns.
//
// Two kernels.  k_ancestor_columns is the column sum-product of hx_sumprod.hip without the counts: a lane per column, a wave
// per mixture component, exp(R t) of the branch at hand in LDS, the messages E, G and their scale factors in a scratch of
// 64-column blocks - and no eigen basis, neither its two matrix-vector products per node nor its half of the traffic.  On
// the way down, at every wildcard, it recomputes F from the children's E (with the reference's rescaling: logF was stored on
// the way up and includes it) and writes the component's posterior terms
//   logCptWeight + logF + log F[a] + logG + log G[a] - colLogLike
// to the scratch, [block][node][cpt][a][64].  Components live in different waves, so k_ancestor_combine, a wave per (block
// of columns, node), adds them with the table log_sum_exp in component order, clamps at 0 and takes the first maximum.  No
// atomics: a call's results do not depend on how the columns are chunked or scheduled.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <vector>
#include "../../include/historian_hip.h"
#include "hx_lse.h"
#include "hx_policy.h"
#include "hx_kernels.h"
#include "hx_sumprod.h"

namespace hx {

namespace {

struct AnModel {
  int A, C, N;
  const int* parent;               // [N] post-order: children before parents, root last; -1 for the root
  const int* child;                // [N][2] children or -1
  const double* ins_prob;          // [C][A]
  const double* log_cpt_weight;    // [C]
  const double* branch_sub;        // [C][N][A][A] exp(R t_r)
};

// scratch of one chunk of columns, in blocks of 64 columns: messages E, G [block][cpt][node][a][64]; scale factors
// [block][cpt][node][64]; posterior terms [block][node][cpt][a][64] (wildcard nodes only: the rest is never read)
struct AnScratch { double* E; double* G; double* T; double* logE; double* logF; double* logG; };

// the lanes of a wave hand values to one another through LDS: the writes have landed before the reads are issued
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// TA, LM: as k_sumprod_columns (hx_sumprod.hip) - the alphabet size at compile time or 0 for any alphabet up to 64
// symbols; with LM a wave keeps exp(R t) of the branch at hand in LDS and reads it as broadcasts (without: through the
// scalar cache - large alphabets only, whose matrices of eight waves exceed the LDS plan).
template <int TA, bool LM>
__global__ void __launch_bounds__(512) k_ancestor_columns(const AnModel m, const signed char* __restrict__ tok, const long long n_cols, const AnScratch s,
                                                          const double* __restrict__ lse_tab, double* __restrict__ col_log_like) {
  constexpr int AX = TA ? TA : 64;
  const int A = TA ? TA : m.A, C = m.C, N = m.N, AA = A * A, AP = (A + 1) & ~1;
  // message vectors are stored two entries per lane and row, [a / 2][64][2] (see k_sumprod_columns)
#define ROWP(P, idx) ((P) + (idx) * (long long)(AP * 64) + lane * 2)
#define EROW(P, cpt, r) ROWP(P, (cb * C + (cpt)) * N + (r))
#define AT(P, cpt, r, a) EROW(P, cpt, r)[((a) >> 1) * 128 + ((a) & 1)]
#define LG(P, cpt, r) P[((cb * C + (cpt)) * N + (r)) * 64 + lane]
  extern __shared__ double sh_ll[];                 // [C][64], then per wave [A * A]: exp(R t)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  HX_LDS double* Lsub = (HX_LDS double*)(sh_ll + 64 * C + (LM ? AA * wave : 0));
  for (long long base = (long long)blockIdx.x * 64; base < n_cols; base += (long long)gridDim.x * 64) {
    const bool busy = base + lane < n_cols;
    const long long col = busy ? base + lane : 0;
    const long long cb = base >> 6;
    auto put_row = [&](double* rp, auto&& gen) {
      if constexpr (TA != 0 && TA % 2 == 0) {
#pragma unroll
        for (int q = 0; q < TA / 2; ++q) *reinterpret_cast<sp_d2*>(rp + q * 128) = sp_d2{gen(2 * q), gen(2 * q + 1)};
      } else {
        for (int a = 0; a < A; ++a) rp[(a >> 1) * 128 + (a & 1)] = gen(a);
      }
    };
    auto get_row = [&](const double* rp, double (&v)[AX]) {
      if constexpr (TA != 0 && TA % 2 == 0) {
#pragma unroll
        for (int q = 0; q < TA / 2; ++q) {
          const sp_d2 t2 = *reinterpret_cast<const sp_d2*>(rp + q * 128);
          v[2 * q] = t2.x; v[2 * q + 1] = t2.y;
        }
      } else {
        for (int a = 0; a < A; ++a) v[a] = rp[(a >> 1) * 128 + (a & 1)];
      }
    };
    // F of a wildcard: the product of the children's messages, rescaled as the reference does (src/sumprod.cpp:120-124);
    // -> the logarithm of the factor taken out (0 when none was)
    auto wild_f = [&](const int cpt, const int c0, const int c1, double (&f)[AX]) -> double {
      double e1[AX];
      double fmax = 0.;
#pragma unroll
      for (int a = 0; a < A; ++a) f[a] = e1[a] = 1.;
      if (c0 >= 0) get_row(EROW(s.E, cpt, c0), f);
      if (c1 >= 0) get_row(EROW(s.E, cpt, c1), e1);
#pragma unroll
      for (int a = 0; a < A; ++a) {
        f[a] *= e1[a];
        fmax = f[a] > fmax ? f[a] : fmax;
      }
      if (fmax < HX_SP_RESCALE) {
#pragma unroll
        for (int a = 0; a < A; ++a) f[a] /= fmax;
        return log(fmax);
      }
      return 0.;
    };
    const signed char* t = tok + col * N;       // -2 gap, -1 wildcard, else the residue's token
    int root = -1;
    for (int r = 0; r < N; ++r)
      if (t[r] != -2 && (m.parent[r] < 0 || t[m.parent[r]] == -2)) root = r;     // (one root per column: the caller's contract)
    // ---- tip-to-root (src/sumprod.cpp:99-161) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      double cpt_ll = 0.;
      CMat ins = cmat(m.ins_prob + cpt * A);
      for (int r = 0; r < N; ++r) {
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();                           // (the reads of the previous node's matrix are done)
          for (int k = lane; k < AA; k += 64) Lsub[k] = m.branch_sub[((long long)cpt * N + r) * AA + k];
          wave_lds_sync();
        }
        if (!busy) continue;
        const int tk = t[r];
        if (tk == -2) {
          // a gap: its message to the parent is all ones
          put_row(EROW(s.E, cpt, r), [](int) { return 1.; });
          LG(s.logE, cpt, r) = 0.;
          continue;
        }
        const int c0 = m.child[2 * r], c1 = m.child[2 * r + 1];
        double lf = (c0 >= 0 ? LG(s.logE, cpt, c0) : 0.) + (c1 >= 0 ? LG(s.logE, cpt, c1) : 0.);
        const double* subg = m.branch_sub + ((long long)cpt * N + r) * AA;
        if (tk >= 0) {
          // a residue: F is one-hot, E a column of the matrix
          double f = (c0 >= 0 ? AT(s.E, cpt, c0, tk) : 1.) * (c1 >= 0 ? AT(s.E, cpt, c1, tk) : 1.);
          if (f < HX_SP_RESCALE) { lf += log(f); f = 1.; }
          LG(s.logF, cpt, r) = lf;
          if (r == root) cpt_ll += lf + log(f * m.ins_prob[cpt * A + tk]);
          else {
            LG(s.logE, cpt, r) = lf;
            put_row(EROW(s.E, cpt, r), [&](const int a) { return (LM ? Lsub[a * A + tk] : subg[a * A + tk]) * f; });
          }
          continue;
        }
        // a wildcard: the full vector
        double f[AX];
        lf += wild_f(cpt, c0, c1, f);
        LG(s.logF, cpt, r) = lf;
        if (r == root) {
          double ip = 0.;
#pragma unroll
          for (int a = 0; a < A; ++a) ip += f[a] * ins[a];
          cpt_ll += lf + log(ip);
          continue;
        }
        LG(s.logE, cpt, r) = lf;
        if constexpr (LM && TA != 0 && TA % 2 == 0) {
          double* rp = EROW(s.E, cpt, r);
          lds_mat_vec<AX>(Lsub, f, [&](const int q, const double ea, const double eb) { *reinterpret_cast<sp_d2*>(rp + q * 128) = sp_d2{ea, eb}; });
        } else {
          CMat sub_s = cmat(subg);
#pragma unroll
          for (int a = 0; a < A; ++a) {
            double e = 0.;
#pragma unroll
            for (int b = 0; b < A; ++b) e += (LM ? Lsub[a * A + b] : sub_s[a * A + b]) * f[b];
            AT(s.E, cpt, r, a) = e;
          }
        }
      }
      sh_ll[cpt * 64 + lane] = cpt_ll;
    }
    __syncthreads();
    double cll = HX_NEG_INF;
    for (int cpt = 0; cpt < C; ++cpt) cll = lse(cll, m.log_cpt_weight[cpt] + sh_ll[cpt * 64 + lane], lse_tab);
    if (wave == 0 && busy) col_log_like[col] = cll;
    // ---- root-to-tip (src/sumprod.cpp:163-198), and the posterior terms of the wildcards (src/sumprod.cpp:213) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      CMat ins = cmat(m.ins_prob + cpt * A);
      const double lcw = m.log_cpt_weight[cpt];
      for (int r = N - 1; r >= 0; --r) {
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();
          for (int k = lane; k < AA; k += 64) {
            // (y = x M with the row routine: staged transposed)
            if constexpr (TA != 0 && TA % 2 == 0) Lsub[(k % A) * A + k / A] = m.branch_sub[((long long)cpt * N + r) * AA + k];
            else Lsub[k] = m.branch_sub[((long long)cpt * N + r) * AA + k];
          }
          wave_lds_sync();
        }
        if (!busy) continue;
        const int tk = t[r];
        if (tk == -2) continue;
        // a residue without children: nobody reads its G (no node below it; its posterior is defined, not computed)
        if (tk >= 0 && m.child[2 * r] < 0) continue;
        double g[AX];
        double lg;
        if (r == root) {
#pragma unroll
          for (int a = 0; a < A; ++a) g[a] = ins[a];
          put_row(EROW(s.G, cpt, r), [&](const int a) { return g[a]; });
          lg = 0.;
        } else {
          const int p = m.parent[r];
          const int sib = m.child[2 * p] == r ? m.child[2 * p + 1] : m.child[2 * p];
          lg = LG(s.logG, cpt, p) + (sib >= 0 ? LG(s.logE, cpt, sib) : 0.);
          // what flows down the branch: the parent's outside message times the sibling's subtree
          double d[AX];
          {
            double es[AX];
#pragma unroll
            for (int a = 0; a < A; ++a) es[a] = 1.;
            get_row(EROW(s.G, cpt, p), d);
            if (sib >= 0) get_row(EROW(s.E, cpt, sib), es);
#pragma unroll
            for (int a = 0; a < A; ++a) d[a] *= es[a];
          }
          if constexpr (LM && TA != 0 && TA % 2 == 0) {
            double* rp = EROW(s.G, cpt, r);
            lds_mat_vec<AX>(Lsub, d, [&](const int q, const double ga, const double gb) {
              *reinterpret_cast<sp_d2*>(rp + q * 128) = sp_d2{ga, gb};
              g[2 * q] = ga; g[2 * q + 1] = gb;
            });
          } else {
            CMat sub_s = cmat(m.branch_sub + ((long long)cpt * N + r) * AA);
#pragma unroll
            for (int b = 0; b < A; ++b) {
              double gb = 0.;
#pragma unroll
              for (int a = 0; a < A; ++a) gb += d[a] * (LM ? Lsub[a * A + b] : sub_s[a * A + b]);
              AT(s.G, cpt, r, b) = gb;
              g[b] = gb;
            }
          }
        }
        LG(s.logG, cpt, r) = lg;
        if (tk != -1) continue;
        // a wildcard: this component's term of every residue's posterior, in the reference's order of additions
        double f[AX];
        (void)wild_f(cpt, m.child[2 * r], m.child[2 * r + 1], f);
        const double lf = LG(s.logF, cpt, r);
        put_row(ROWP(s.T, (cb * N + r) * C + cpt), [&](const int a) { return lcw + lf + log(f[a]) + lg + log(g[a]) - cll; });
      }
    }
    __syncthreads();            // (sh_ll is rewritten by the next block of columns)
  }
#undef ROWP
#undef EROW
#undef AT
#undef LG
}

// A wave per (block of 64 columns, node), a lane per column: the posterior of every residue - the components' terms added in
// component order (log_accum_exp), clamped at 0 - and its first maximum (std::max_element).  A gap is -2 and -inf, a
// residue its token and 0 / -inf.  POST: the rows of A doubles go through LDS and leave the wave as contiguous stretches.
template <bool POST>
__global__ void __launch_bounds__(256) k_ancestor_combine(const AnModel m, const signed char* __restrict__ tok, const long long n_cols, const double* __restrict__ T,
                                                          const double* __restrict__ lse_tab, signed char* __restrict__ best, double* __restrict__ post) {
  extern __shared__ double sh_rows[];              // per wave [64][A | 1]
  const int A = m.A, C = m.C, N = m.N, AP = (A + 1) & ~1, S = A | 1;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  const long long gw = (long long)blockIdx.x * Wb + wave, n_blocks = (n_cols + 63) >> 6;
  if (gw >= n_blocks * N) return;                  // (whole waves; no workgroup barrier below)
  const long long cb = gw / N;
  const int r = (int)(gw - cb * N);
  const long long col = cb * 64 + lane;
  const bool busy = col < n_cols;
  const int tk = busy ? tok[col * N + r] : -2;
  HX_LDS double* rows = (HX_LDS double*)(sh_rows + (POST ? wave * 64 * S : 0));
  const double* tp = T + ((cb * N + r) * C) * (long long)(AP * 64) + lane * 2;
  int arg = 0;
  double top = HX_NEG_INF;
  for (int a = 0; a < A; ++a) {
    double lp = HX_NEG_INF;
    if (tk >= 0) lp = a == tk ? 0. : HX_NEG_INF;
    else if (tk == -1) {
      for (int cpt = 0; cpt < C; ++cpt) lp = lse(lp, tp[cpt * (long long)(AP * 64) + (a >> 1) * 128 + (a & 1)], lse_tab);
      lp = lp < 0. ? lp : 0.;
      if (lp > top) { top = lp; arg = a; }
    }
    if (POST) rows[lane * S + a] = lp;
  }
  if (busy) best[col * N + r] = (signed char)(tk == -1 ? arg : tk);
  if (POST) {
    wave_lds_sync();
    for (int k = lane; k < 64 * A; k += 64) {
      const int c = k / A, a = k - c * A;
      if (cb * 64 + c < n_cols) post[((cb * 64 + c) * N + r) * A + a] = rows[c * S + a];
    }
  }
}

}  // namespace

}  // namespace hx

using namespace hx;

extern "C" {

// See include/historian_hip.h.  One call = upload, the two kernels over chunks of columns that fit the scratch budget, download.
int hx_sumprod_ancestors(const hx_sumprod_model* hm, const int8_t* tokens, int64_t n_cols, double* col_log_like, int8_t* best,
                         double* node_post, void* stream) {
  if (!hm || !tokens || n_cols <= 0 || !best) return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: null argument or no columns");
  const int A = hm->alph_size, C = hm->components, N = hm->n_nodes, AA = A * A;
  if (A <= 0 || C <= 0 || N <= 0 || !hm->parent || !hm->ins_prob || !hm->log_cpt_weight || !hm->branch_sub)
    return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: incomplete model");
  if (A > 64) return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: alphabets of more than 64 symbols are not supported");
  if (C > 128) return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: more than 128 mixture components are not supported");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return api_fail(HX_ERR_NO_DEVICE, "no HIP device");
  const double* lse_tab = device_lse_table(device);
  if (!lse_tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the current device");
  // children from parents; binary, children before parents
  std::vector<int> child(2 * (size_t)N, -1);
  for (int r = 0; r < N; ++r) {
    const int p = hm->parent[r];
    if (p < 0) continue;
    if (p <= r || p >= N) return api_fail(HX_ERR_NOT_TOPOSORTED, "hx_sumprod_ancestors: a node precedes its child");
    if (child[2 * p] < 0) child[2 * p] = r;
    else if (child[2 * p + 1] < 0) child[2 * p + 1] = r;
    else return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: a node has more than two children");
  }
  // tokens index the alphabet on the device: refuse anything else here, not with a fault there
  for (int64_t k = 0; k < n_cols * N; ++k)
    if (tokens[k] < -2 || tokens[k] >= A) return api_fail(HX_ERR_RANGE, "hx_sumprod_ancestors: a token outside -2 .. alphabet size - 1");
  // the LDS plans, checked before anything is allocated or launched
  const int tpb = 64 * (C < 8 ? C : 8);            // a wave per mixture component, up to eight
  const size_t ll_lds = sizeof(double) * 64 * (size_t)C, mat_lds = sizeof(double) * (size_t)AA * (tpb / 64);
  const bool lm = ll_lds + mat_lds <= 96 * 1024;
  const size_t col_lds = ll_lds + (lm ? mat_lds : 0);
  const int cwaves = A <= 20 ? 4 : 1;              // waves per workgroup of the combining kernel
  const size_t row_lds = node_post ? sizeof(double) * 64 * (size_t)(A | 1) * cwaves : 0;
  if (col_lds > HX_LDS_LIMIT || row_lds > HX_LDS_LIMIT) return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_ancestors: the LDS plan exceeds the LDS of a CU");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SpBuf b_int, b_dbl, b_tok, b_scr, b_out, b_best;
  const size_t dbls = (size_t)C * A + C + (size_t)C * N * AA;
  if (hipMalloc(&b_int.p, 3 * (size_t)N * sizeof(int)) != hipSuccess || hipMalloc(&b_dbl.p, dbls * sizeof(double)) != hipSuccess ||
      hipMalloc(&b_tok.p, (size_t)n_cols * N) != hipSuccess || hipMalloc(&b_best.p, (size_t)n_cols * N) != hipSuccess)
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_sumprod_ancestors: device allocation failed");
  int* d_int = static_cast<int*>(b_int.p);
  double* d_dbl = static_cast<double*>(b_dbl.p);
  AnModel m;
  m.A = A; m.C = C; m.N = N; m.parent = d_int; m.child = d_int + N;
  m.ins_prob = d_dbl; m.log_cpt_weight = d_dbl + (size_t)C * A; m.branch_sub = d_dbl + (size_t)C * A + C;
  if (hipMemcpy(d_int, hm->parent, N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_int + N, child.data(), 2 * (size_t)N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_dbl, hm->ins_prob, (size_t)C * A * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_dbl + (size_t)C * A, hm->log_cpt_weight, C * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_dbl + (size_t)C * A + C, hm->branch_sub, (size_t)C * N * AA * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(b_tok.p, tokens, (size_t)n_cols * N, hipMemcpyHostToDevice) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_sumprod_ancestors: copy failed");
  // columns per chunk: the scratch of a chunk stays within the budget (HX_SUMPROD_SCRATCH_MB, default 16 GiB)
  const int AP = (A + 1) & ~1;                     // message vectors are stored in pairs of entries
  const size_t per_col = 3 * (size_t)C * N * AP + 3 * (size_t)C * N;
  size_t budget = (size_t)16 << 30;
  if (const char* e = getenv("HX_SUMPROD_SCRATCH_MB")) budget = (size_t)atoll(e) << 20;
  long long chunk = (long long)(budget / (per_col * sizeof(double)));
  chunk &= ~63LL;                                   // whole blocks of 64 columns
  if (chunk < 64) chunk = 64;
  if (chunk > n_cols) chunk = n_cols;
  const size_t n_out = (size_t)n_cols * (1 + (node_post ? (size_t)N * A : 0));
  if (hipMalloc(&b_scr.p, per_col * (((size_t)chunk + 63) & ~(size_t)63) * sizeof(double)) != hipSuccess || hipMalloc(&b_out.p, n_out * sizeof(double)) != hipSuccess)
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_sumprod_ancestors: device allocation failed");
  double* d_cll = static_cast<double*>(b_out.p);
  double* d_post = node_post ? d_cll + n_cols : nullptr;
  signed char* d_best = static_cast<signed char*>(b_best.p);
  struct Events {                                   // destroyed on every way out
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } ev;
  if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return api_fail(HX_ERR_HIP, "hx_sumprod_ancestors: HIP call failed");
  (void)hipEventRecord(ev.a, st);
  for (long long first = 0; first < n_cols; first += chunk) {
    const long long nc = n_cols - first < chunk ? n_cols - first : chunk;
    double* scr = static_cast<double*>(b_scr.p);
    const size_t nc64 = ((size_t)nc + 63) & ~(size_t)63;         // the scratch holds whole blocks of 64 columns
    const size_t msg = (size_t)C * N * AP * nc64, lg = (size_t)C * N * nc64;
    AnScratch s;
    s.E = scr; s.G = scr + msg; s.T = scr + 2 * msg;
    s.logE = scr + 3 * msg; s.logF = s.logE + lg; s.logG = s.logF + lg;
    const long long blocks64 = (nc + 63) / 64;
    const long long blocks = blocks64 > 65535 ? 65535 : blocks64;
    const signed char* d_tok = static_cast<const signed char*>(b_tok.p) + first * N;
#define HX_AN_GO(TA_, LM_) hipLaunchKernelGGL((k_ancestor_columns<TA_, LM_>), dim3((unsigned)blocks), dim3(tpb), col_lds, st, m, d_tok, nc, s, lse_tab, d_cll + first)
    // (eight waves' matrices of A = 4 or 20 and 128 components' likelihoods fit the LDS plan: the fixed-size forms always have them)
    if (A == 4 && lm) HX_AN_GO(4, true);
    else if (A == 20 && lm) HX_AN_GO(20, true);
    else if (lm) HX_AN_GO(0, true);
    else HX_AN_GO(0, false);
#undef HX_AN_GO
    const unsigned cgrid = (unsigned)((blocks64 * N + cwaves - 1) / cwaves);
    if (d_post)
      hipLaunchKernelGGL(k_ancestor_combine<true>, dim3(cgrid), dim3(64 * cwaves), row_lds, st, m, d_tok, nc, s.T, lse_tab, d_best + first * N,
                         d_post + (size_t)first * N * A);
    else
      hipLaunchKernelGGL(k_ancestor_combine<false>, dim3(cgrid), dim3(64 * cwaves), 0, st, m, d_tok, nc, s.T, lse_tab, d_best + first * N, (double*)nullptr);
  }
  (void)hipEventRecord(ev.b, st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_sumprod_ancestors: kernel launch or execution failed");
  (void)hipEventElapsedTime(&g_sp_ms, ev.a, ev.b);
  if (hipMemcpy(best, d_best, (size_t)n_cols * N, hipMemcpyDeviceToHost) != hipSuccess ||
      (col_log_like && hipMemcpy(col_log_like, d_cll, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
      (node_post && hipMemcpy(node_post, d_post, (size_t)n_cols * N * A * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "hx_sumprod_ancestors: copy failed");
  return HX_OK;
}

}  // extern "C"
