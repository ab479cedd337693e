// Ancestral sequence prediction (-ancseq, -ancprob): the residue posterior of EVERY node of every alignment column, and
// the most probable residue of every wildcard - the reference's SumProduct::logNodePostProb and maxPostState
// (src/sumprod.cpp:208-217, 259-262) behind AlignColSumProduct::appendAncestralReconstructedColumn and
// appendAncestralPostProbColumn (src/sumprod.cpp:401-426), for a BATCH of columns.
//
// Two kernels.  k_ancestor_columns runs the two passes of the column sum-product through the steps of hx_sumprod.h, the ones
// k_sumprod_columns (hx_sumprod.hip) runs: a lane per column, a wave per mixture component, exp(R t) of the branch at hand in
// LDS, the messages E, G and their scale factors in a scratch of 64-column blocks - and no eigen basis, neither its two
// matrix-vector products per node nor its half of the traffic.  On the way down, at every wildcard, it recomputes F from the children's E (with the reference's rescaling: logF was stored on
// the way up and includes it) and writes the component's posterior terms
//   logCptWeight + logF + log F[a] + logG + log G[a] - colLogLike
// to the scratch, [block][node][cpt][a][64].  Components live in different waves, so k_ancestor_combine, a wave per (block
// of columns, node), adds them with the table log_sum_exp in component order, clamps at 0 and takes the first maximum.  No
// atomics: a call's results do not depend on how the columns are chunked or scheduled.
#include <hip/hip_runtime.h>
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

// TA, LM: see hx_sumprod.h; LM: exp(R t) of the branch at hand (without it: large alphabets only, whose matrices of eight
// waves exceed the LDS plan).
template <int TA, bool LM>
__global__ void __launch_bounds__(512) k_ancestor_columns(const AnModel m, const signed char* __restrict__ tok, const long long n_cols, const AnScratch s,
                                                          const double* __restrict__ lse_tab, double* __restrict__ col_log_like) {
  constexpr int AX = sp_ax<TA>;
  const int A = TA ? TA : m.A, C = m.C, N = m.N, AA = A * A;
  extern __shared__ double sh_ll[];                 // [C][64], then per wave [A * A]: exp(R t)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  HX_LDS double* Lsub = (HX_LDS double*)(sh_ll + 64 * C + (LM ? AA * wave : 0));
  for (long long base = (long long)blockIdx.x * 64; base < n_cols; base += (long long)gridDim.x * 64) {
    const bool busy = base + lane < n_cols;
    const long long col = busy ? base + lane : 0;
    const SpBlock blk{base >> 6, C, N, (A + 1) & ~1, lane};
    const signed char* t = tok + col * N;       // -2 gap, -1 wildcard, else the residue's token
    const int root = column_root(t, m.parent, N);
    // ---- tip-to-root (src/sumprod.cpp:99-161) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      double cpt_ll = 0.;
      CMat ins = cmat(m.ins_prob + cpt * A);
      for (int r = 0; r < N; ++r) {
        const double* subg = m.branch_sub + ((long long)cpt * N + r) * AA;
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();                           // (the reads of the previous node's matrix are done)
          lds_stage<false>(Lsub, subg, A, lane);
          wave_lds_sync();
        }
        if (!busy) continue;
        const int tk = t[r];
        const long long at = blk.node(cpt, r);
        if (tk == -2) {
          // a gap: its message to the parent is all ones
          put_row<TA>(blk.row(s.E, at), A, [](int) { return 1.; });
          blk.lg(s.logE, at) = 0.;
          continue;
        }
        const int c0 = m.child[2 * r], c1 = m.child[2 * r + 1];
        const long long at0 = blk.node(cpt, c0), at1 = blk.node(cpt, c1);
        double lf = (c0 >= 0 ? blk.lg(s.logE, at0) : 0.) + (c1 >= 0 ? blk.lg(s.logE, at1) : 0.);
        if (tk >= 0) {
          // a residue: E is a column of the matrix
          const double f = residue_f(c0 >= 0, blk.row(s.E, at0), c1 >= 0, blk.row(s.E, at1), tk, lf);
          blk.lg(s.logF, at) = lf;
          if (r == root) cpt_ll += lf + log(f * m.ins_prob[cpt * A + tk]);
          else {
            blk.lg(s.logE, at) = lf;
            put_row<TA>(blk.row(s.E, at), A, [&](const int a) { return (LM ? Lsub[a * A + tk] : subg[a * A + tk]) * f; });
          }
          continue;
        }
        double f[AX];
        wild_f<TA>(c0 >= 0, blk.row(s.E, at0), c1 >= 0, blk.row(s.E, at1), A, f, lf);
        blk.lg(s.logF, at) = lf;
        if (r == root) {
          cpt_ll += wild_root_ll<TA>(f, ins, A, lf);
          continue;
        }
        blk.lg(s.logE, at) = lf;
        mat_vec_store<TA, LM, false>(Lsub, cmat(subg), A, f, blk.row(s.E, at));
      }
      sh_ll[cpt * 64 + lane] = cpt_ll;
    }
    __syncthreads();
    const double cll = combine_components(sh_ll, m.log_cpt_weight, C, lane, lse_tab);
    if (wave == 0 && busy) col_log_like[col] = cll;
    // ---- root-to-tip (src/sumprod.cpp:163-198), and the posterior terms of the wildcards (src/sumprod.cpp:213) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      CMat ins = cmat(m.ins_prob + cpt * A);
      const double lcw = m.log_cpt_weight[cpt];
      for (int r = N - 1; r >= 0; --r) {
        const double* subg = m.branch_sub + ((long long)cpt * N + r) * AA;
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();
          lds_stage<sp_rows<TA>>(Lsub, subg, A, lane);
          wave_lds_sync();
        }
        if (!busy) continue;
        const int tk = t[r];
        if (tk == -2) continue;
        // a residue without children: nobody reads its G (no node below it; its posterior is defined, not computed)
        if (tk >= 0 && m.child[2 * r] < 0) continue;
        const long long at = blk.node(cpt, r);
        double g[AX];
        double lg;
        if (r == root) {
#pragma unroll
          for (int a = 0; a < A; ++a) g[a] = ins[a];
          put_row<TA>(blk.row(s.G, at), A, [&](const int a) { return g[a]; });
          lg = 0.;
        } else {
          const int p = m.parent[r];
          const int sib = m.child[2 * p] == r ? m.child[2 * p + 1] : m.child[2 * p];
          const long long atp = blk.node(cpt, p), ats = blk.node(cpt, sib);
          lg = blk.lg(s.logG, atp) + (sib >= 0 ? blk.lg(s.logE, ats) : 0.);
          // what flows down the branch: the parent's outside message times the sibling's subtree
          double d[AX];
          row_product<TA>(true, blk.row(s.G, atp), sib >= 0, blk.row(s.E, ats), A, d);
          mat_vec_store<TA, LM, true>(Lsub, cmat(subg), A, d, blk.row(s.G, at), [&](const int b, const double gb) { return g[b] = gb; });
        }
        blk.lg(s.logG, at) = lg;
        if (tk != -1) continue;
        // a wildcard: this component's term of every residue's posterior, in the reference's order of additions; F anew from
        // the children's E (logF was stored on the way up and includes the rescaling)
        double f[AX];
        double unused = 0.;
        const int c0 = m.child[2 * r], c1 = m.child[2 * r + 1];
        wild_f<TA>(c0 >= 0, blk.row(s.E, blk.node(cpt, c0)), c1 >= 0, blk.row(s.E, blk.node(cpt, c1)), A, f, unused);
        const double lf = blk.lg(s.logF, at);
        put_row<TA>(blk.row(s.T, (blk.cb * N + r) * C + cpt), A, [&](const int a) { return lcw + lf + log(f[a]) + lg + log(g[a]) - cll; });
      }
    }
    __syncthreads();            // (sh_ll is rewritten by the next block of columns)
  }
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
  const char* fn = "hx_sumprod_ancestors";
  const int A = hm->alph_size, C = hm->components, N = hm->n_nodes;
  const bool complete = A > 0 && C > 0 && N > 0 && hm->parent && hm->ins_prob && hm->log_cpt_weight && hm->branch_sub;
  int device = 0;
  const double* lse_tab = nullptr;
  std::vector<int> child;
  if (int rc = sp_check_model(fn, complete, A, C, HX_ERR_INVALID_ARG, &device, &lse_tab)) return rc;
  if (int rc = sp_children(fn, hm->parent, N, false, HX_ERR_INVALID_ARG, child)) return rc;
  if (int rc = sp_check_tokens(fn, tokens, n_cols * N, A)) return rc;
  // the LDS plans, checked before anything is allocated or launched
  const SpPlan plan = sp_column_plan(A, C, 1, false);            // exp(R t)
  const int cwaves = A <= 20 ? 4 : 1;              // waves per workgroup of the combining kernel
  const size_t row_lds = node_post ? sizeof(double) * 64 * (size_t)(A | 1) * cwaves : 0;
  if (plan.lds > HX_LDS_LIMIT || row_lds > HX_LDS_LIMIT) return sp_fail(HX_ERR_INVALID_ARG, fn, "the LDS plan exceeds the LDS of a CU");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SpUpload up;
  DevBuf b_tok, b_scr, b_out, b_best;
  if (!up.alloc(sp_tree_room(A, C, N, true)) || !b_tok.alloc((size_t)n_cols * N) || !b_best.alloc((size_t)n_cols * N))
    return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  const SpTree tr = sp_put_tree(up, A, C, N, hm->parent, child, hm->ins_prob, hm->log_cpt_weight, hm->branch_sub);
  AnModel m;
  m.A = A; m.C = C; m.N = N; m.parent = tr.parent; m.child = tr.child;
  m.ins_prob = tr.ins_prob; m.log_cpt_weight = tr.log_cpt_weight; m.branch_sub = tr.branch_sub;
  if (!up.copied || hipMemcpy(b_tok.as<void>(), tokens, (size_t)n_cols * N, hipMemcpyHostToDevice) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "copy failed");
  const int AP = (A + 1) & ~1;                     // message vectors are stored in pairs of entries
  const size_t per_col = 3 * (size_t)C * N * AP + 3 * (size_t)C * N;
  const long long chunk = sp_chunk(per_col, n_cols);
  const size_t n_out = (size_t)n_cols * (1 + (node_post ? (size_t)N * A : 0));
  if (!b_scr.alloc(per_col * (((size_t)chunk + 63) & ~(size_t)63) * sizeof(double)) || !b_out.alloc(n_out * sizeof(double)))
    return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  double* d_cll = b_out.as<double>();
  double* d_post = node_post ? d_cll + n_cols : nullptr;
  signed char* d_best = b_best.as<signed char>();
  DevEvents<2> ev;
  if (!ev.create()) return sp_fail(HX_ERR_HIP, fn, "HIP call failed");
  (void)hipEventRecord(ev[0], st);
  for (long long first = 0; first < n_cols; first += chunk) {
    const long long nc = n_cols - first < chunk ? n_cols - first : chunk;
    double* scr = b_scr.as<double>();
    const size_t nc64 = ((size_t)nc + 63) & ~(size_t)63;         // the scratch holds whole blocks of 64 columns
    const size_t msg = (size_t)C * N * AP * nc64, lg = (size_t)C * N * nc64;
    AnScratch s;
    s.E = scr; s.G = scr + msg; s.T = scr + 2 * msg;
    s.logE = scr + 3 * msg; s.logF = s.logE + lg; s.logG = s.logF + lg;
    const long long blocks64 = (nc + 63) / 64;
    const long long blocks = blocks64 > 65535 ? 65535 : blocks64;
    const signed char* d_tok = b_tok.as<const signed char>() + first * N;
#define HX_AN_GO(TA_, LM_) hipLaunchKernelGGL((k_ancestor_columns<TA_, LM_>), dim3((unsigned)blocks), dim3(64 * plan.waves), plan.lds, st, m, d_tok, nc, s, lse_tab, d_cll + first)
    // (eight waves' matrices of A = 4 or 20 and 128 components' likelihoods fit the LDS plan: the fixed-size forms always have them)
    if (A == 4 && plan.lm) HX_AN_GO(4, true);
    else if (A == 20 && plan.lm) HX_AN_GO(20, true);
    else if (plan.lm) HX_AN_GO(0, true);
    else HX_AN_GO(0, false);
#undef HX_AN_GO
    const unsigned cgrid = (unsigned)((blocks64 * N + cwaves - 1) / cwaves);
    if (d_post)
      hipLaunchKernelGGL(k_ancestor_combine<true>, dim3(cgrid), dim3(64 * cwaves), row_lds, st, m, d_tok, nc, s.T, lse_tab, d_best + first * N,
                         d_post + (size_t)first * N * A);
    else
      hipLaunchKernelGGL(k_ancestor_combine<false>, dim3(cgrid), dim3(64 * cwaves), 0, st, m, d_tok, nc, s.T, lse_tab, d_best + first * N, (double*)nullptr);
  }
  (void)hipEventRecord(ev[1], st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return sp_fail(HX_ERR_HIP, fn, "kernel launch or execution failed");
  (void)hipEventElapsedTime(&g_sp_ms, ev[0], ev[1]);
  if (hipMemcpy(best, d_best, (size_t)n_cols * N, hipMemcpyDeviceToHost) != hipSuccess ||
      (col_log_like && hipMemcpy(col_log_like, d_cll, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
      (node_post && hipMemcpy(node_post, d_post, (size_t)n_cols * N * A * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
    return sp_fail(HX_ERR_HIP, fn, "copy failed");
  return HX_OK;
}

}  // extern "C"
