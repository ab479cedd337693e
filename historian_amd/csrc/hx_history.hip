// A history resident on the device: what a tree-height MCMC on a fixed alignment accepts or rejects its moves on - the
// substitution log-likelihood of TreeAlignFuncs::substLogLikelihood (reference src/sampler.cpp:394-407), SumProduct::fillUp
// of every column (src/sumprod.cpp:99-161) - kept between proposals, and the indel transition counts of every branch
// (indelLogLikelihood's pairPath walk, src/sampler.cpp:150-189, 382-392, as twelve integers per branch).
//
// k_history_columns is the way up of the column sum-product, through the steps of hx_sumprod.h that k_sumprod_columns and
// k_ancestor_columns run (the same bits where the launch plans agree): a lane per column, a wave per mixture component,
// exp(R t) of the branch at hand in LDS.  What differs: the tokens (transposed: [node][column]), the tree, the branch
// matrices and the messages E, logE of every (column, component, node) stay on the device, every node in TWO slots.  A
// proposal names the nodes whose branch changed; the kernel walks only those and their ancestors, in post order, reads a
// node outside that set from its current slot and writes to the other slot; accepting flips the slot of the walked nodes
// (host bookkeeping, no copy), rejecting does nothing.  A column whose root lies outside the walked set keeps its
// likelihood.  A gap's message is all ones and is neither stored nor read.  The full evaluation is the proposal that walks
// every node, so both run the same instructions on the same operands: the same bits.
//
// A proposal brings its new matrices (k_history_scatter puts the upload in place) or only its new branch lengths: then
// k_branch_expm (hx_expm.hip) computes exp(R t) from the rate matrices the history was given once, straight into the idle
// slots, with the bits of the host mirror's RateModel::getSubProbMatrix.
//
// k_history_sum adds the column likelihoods in one workgroup, a fixed order for a given number of columns, whatever the
// grid of the column kernel and whichever columns were recomputed.  No atomics anywhere.
//
// k_history_excluded answers a query on the live history and writes nothing to it: the excluded-neighbour profiles that
// TreeAlignFuncs::getConditionalPWMs collects (src/sampler.cpp:356-370, SumProduct::logNodeExcludedPostProb) from the
// messages the history holds and a way down along the one path from each column's root to the node asked for.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/historian_hip.h"
#include "hx_lse.h"
#include "hx_policy.h"
#include "hx_kernels.h"
#include "hx_sumprod.h"
#include "hx_expm.h"
#include "hx_history_host.h"
#include "hx_branch_inputs.h"

namespace hx {

namespace {

struct HsArgs {
  int A, C, N, n_walk;
  long long n_cols, ncp;           // ncp: the columns rounded up to whole blocks of 64
  long long e_slot, lg_slot;       // doubles between the two slots of E and of logE
  const signed char* tok;          // [N][ncp] -2 gap, -1 wildcard, else the residue's token
  const int* root;                 // [ncp] the column's root, -1 in a column of gaps
  const int* child;                // [N][2] children or -1
  const int* walk;                 // [n_walk] the nodes to recompute, ascending (children before parents)
  const int* info;                 // [N] bit 0: the slot of the node's messages in this evaluation (read and, if walked,
                                   //     written); bit 1: the slot of its matrix; bit 2: walked
  const double* ins_prob;          // [C][A]
  const double* log_cpt_weight;    // [C]
  const double* mats;              // [2][C][N][A][A] exp(R t)
  double* E;                       // [2][block][cpt][node][A' / 2][64][2]
  double* logE;                    // [2][block][cpt][node][64]
  const double* cll_cur;           // [ncp]
  double* cll_new;                 // [ncp]
};

// TA: the alphabet size at compile time (even) or 0 for any alphabet up to 64 symbols (see hx_sumprod.h); the matrices
// are always in LDS (hx_history_create sheds waves until they fit)
template <int TA>
__global__ void __launch_bounds__(512) k_history_columns(const HsArgs h, const double* __restrict__ lse_tab) {
  constexpr int AX = sp_ax<TA>;
  const int A = TA ? TA : h.A, C = h.C, N = h.N, AA = A * A;
  extern __shared__ double sh_ll[];                 // [C][64], then per wave [A * A]: exp(R t)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  HX_LDS double* Lsub = (HX_LDS double*)(sh_ll + 64 * C + AA * wave);
  for (long long base = (long long)blockIdx.x * 64; base < h.n_cols; base += (long long)gridDim.x * 64) {
    const bool busy = base + lane < h.n_cols;
    const long long col = base + lane;               // (< ncp: the token and root arrays hold whole blocks)
    const SpBlock blk{base >> 6, C, N, (A + 1) & ~1, lane};
    const int root = h.root[col];
    // the column's likelihood changes when its root was walked (a column of gaps: the constant is written anew)
    const bool redo = busy && (root < 0 || (h.info[root] & 4));
    for (int cpt = wave; cpt < C; cpt += Wb) {
      double cpt_ll = 0.;
      CMat ins = cmat(h.ins_prob + cpt * A);
      for (int k = 0; k < h.n_walk; ++k) {
        const int r = h.walk[k], inf = h.info[r];
        const int tk = busy ? h.tok[r * h.ncp + col] : -2;
        if (!__any(tk != -2)) continue;              // (the whole wave: nobody needs this branch)
        if (r != N - 1) {
          wave_lds_sync();                           // (the reads of the previous node's matrix are done)
          lds_stage<false>(Lsub, h.mats + ((((long long)(inf >> 1) & 1) * C + cpt) * N + r) * AA, A, lane);
          wave_lds_sync();
        }
        if (tk == -2) continue;                      // a gap: its message to the parent is all ones, and nobody reads it
        // a node's two slots are two bases of the same block layout
        const int c0 = h.child[2 * r], c1 = h.child[2 * r + 1];
        const bool g0 = c0 >= 0 && h.tok[c0 * h.ncp + col] != -2, g1 = c1 >= 0 && h.tok[c1 * h.ncp + col] != -2;
        const int s0 = g0 ? h.info[c0] & 1 : 0, s1 = g1 ? h.info[c1] & 1 : 0, sr = inf & 1;
        const long long at0 = blk.node(cpt, c0), at1 = blk.node(cpt, c1), at = blk.node(cpt, r);
        const double* e0 = blk.row(h.E + s0 * h.e_slot, at0);
        const double* e1 = blk.row(h.E + s1 * h.e_slot, at1);
        double* rp = blk.row(h.E + sr * h.e_slot, at);
        double lf = (g0 ? blk.lg(h.logE + s0 * h.lg_slot, at0) : 0.) + (g1 ? blk.lg(h.logE + s1 * h.lg_slot, at1) : 0.);
        if (tk >= 0) {
          // a residue: E is a column of the matrix
          const double f = residue_f(g0, e0, g1, e1, tk, lf);
          if (r == root) { cpt_ll = lf + log(f * h.ins_prob[cpt * A + tk]); continue; }
          blk.lg(h.logE + sr * h.lg_slot, at) = lf;
          put_row<TA>(rp, A, [&](const int a) { return Lsub[a * A + tk] * f; });
          continue;
        }
        double f[AX];
        wild_f<TA>(g0, e0, g1, e1, A, f, lf);
        if (r == root) { cpt_ll = wild_root_ll<TA>(f, ins, A, lf); continue; }
        blk.lg(h.logE + sr * h.lg_slot, at) = lf;
        mat_vec_store<TA, true, false>(Lsub, CMat(), A, f, rp);
      }
      sh_ll[cpt * 64 + lane] = cpt_ll;
    }
    __syncthreads();
    if (wave == 0 && busy) h.cll_new[col] = redo ? combine_components(sh_ll, h.log_cpt_weight, C, lane, lse_tab) : h.cll_cur[col];
    __syncthreads();            // (sh_ll is rewritten by the next block of columns)
  }
}

// One workgroup of 1024 threads: thread t adds the columns t, t + 1024, ... in that order, then the 1024 partial sums are
// added pairwise, neighbours first.  The order depends on the number of columns alone.
__global__ void __launch_bounds__(1024) k_history_sum(const double* __restrict__ cll, const long long n_cols, double* __restrict__ out) {
  __shared__ double part[1024];
  const int t = (int)threadIdx.x;
  double s = 0.;
  for (long long c = t; c < n_cols; c += 1024) s += cll[c];
  part[t] = s;
  __syncthreads();
  for (int step = 1; step < 1024; step <<= 1) {
    if ((t & (2 * step - 1)) == 0) part[t] += part[t + step];
    __syncthreads();
  }
  if (t == 0) *out = part[0];
}

// The new matrices of a proposal, uploaded as one block [k][cpt][A][A], to the slot the current matrix of each changed node
// is not in (bit 1 of its info word): a workgroup per (changed node, component).
__global__ void __launch_bounds__(256) k_history_scatter(const double* __restrict__ stage, const int* __restrict__ changed, const int* __restrict__ info,
                                                         const int C, const int N, const int AA, double* __restrict__ mats) {
  const int k = (int)blockIdx.x / C, cpt = (int)blockIdx.x - k * C, r = changed[k];
  double* dst = mats + ((((long long)(info[r] >> 1) & 1) * C + cpt) * N + r) * AA;
  const double* src = stage + ((long long)k * C + cpt) * AA;
  for (int q = (int)threadIdx.x; q < AA; q += (int)blockDim.x) dst[q] = src[q];
}

// The indel transition counts of every branch: a wave per node, a lane per column of a block of 64, blocks in order.
// pairPath (src/sampler.cpp:150-189) drops the columns empty in both rows and defers deletions, so between two Match
// columns the path holds all its Insert columns, then all its Delete columns: a stretch of k inserts and m deletes that
// ends in X (Match or End) adds
//   k > 0: n[S][I] 1, n[I][I] k - 1, then m > 0: n[I][D] 1, n[D][D] m - 1, n[D][X] 1; m = 0: n[I][X] 1
//   k = 0: m > 0: n[S][D] 1, n[D][D] m - 1, n[D][X] 1; m = 0: n[S][X] 1
// with S the Start/Match row.  The lane of a Match column counts its stretch from the ballots of its block plus what
// earlier blocks left open (k_open, m_open: the same in every lane); integers, so the order of the additions is free.
__global__ void __launch_bounds__(256) k_history_indels(const signed char* __restrict__ tok, const int* __restrict__ parent, const int N,
                                                        const long long n_cols, const long long ncp, long long* __restrict__ counts) {
  __shared__ long long sh_n[4][64][12];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + wave;
  if (r >= N) return;                               // (whole waves; no workgroup barrier below)
  const int p = parent[r];
  long long n[12];
  for (int k = 0; k < 12; ++k) n[k] = 0;
  auto stretch = [&](const long long k, const long long m, const int x) {       // x: 0 Match, 3 End
    if (k > 0) {
      n[0 * 4 + 1] += 1; n[1 * 4 + 1] += k - 1;
      if (m > 0) { n[1 * 4 + 2] += 1; n[2 * 4 + 2] += m - 1; n[2 * 4 + x] += 1; }
      else n[1 * 4 + x] += 1;
    } else if (m > 0) { n[0 * 4 + 2] += 1; n[2 * 4 + 2] += m - 1; n[2 * 4 + x] += 1; }
    else n[0 * 4 + x] += 1;
  };
  if (p >= 0) {
    long long k_open = 0, m_open = 0;
    for (long long base = 0; base < n_cols; base += 64) {
      const long long col = base + lane;
      const bool in = col < n_cols;
      const bool c1 = in && tok[p * ncp + col] != -2, c2 = in && tok[r * ncp + col] != -2;
      const unsigned long long mat = __ballot(c1 && c2), ins = __ballot(!c1 && c2), del = __ballot(c1 && !c2);
      const unsigned long long below = (1ull << lane) - 1;
      if (c1 && c2) {
        const unsigned long long before = mat & below;                  // the Match columns of this block before mine
        // the columns of my stretch: after the last Match before mine
        const unsigned long long span = before ? below & ~((2ull << (63 - __builtin_clzll(before))) - 1) : below;
        stretch(__builtin_popcountll(ins & span) + (before ? 0 : k_open), __builtin_popcountll(del & span) + (before ? 0 : m_open), 0);
      }
      if (mat) {
        const int last = 63 - __builtin_clzll(mat);
        const unsigned long long after = last == 63 ? 0ull : ~((2ull << last) - 1);
        k_open = __builtin_popcountll(ins & after);
        m_open = __builtin_popcountll(del & after);
      } else {
        k_open += __builtin_popcountll(ins);
        m_open += __builtin_popcountll(del);
      }
    }
    if (lane == 0) stretch(k_open, m_open, 3);
  }
  for (int k = 0; k < 12; ++k) sh_n[wave][lane][k] = n[k];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane < 12) {
    long long s = 0;
    for (int l = 0; l < 64; ++l) s += sh_n[wave][l][lane];
    counts[r * 12 + lane] = s;
  }
}

// ---- excluded-neighbour profiles: SumProduct::logNodeExcludedPostProb (src/sumprod.cpp:219-250) of every column ----
struct HxArgs {
  int A, C, N, n_pairs;
  long long n_cols, ncp, n_blocks;
  long long e_slot, lg_slot;
  const signed char* tok;          // [N][ncp]
  const int* root;                 // [ncp]
  const int* child;                // [N][2]
  const int* info;                 // [N] bit 0: the slot of the node's messages in the state asked for; bit 1: of its matrix
  const int* pair;                 // [n_pairs][4] node, excluded neighbour, start of the path (-1: none), its length
  const int* path;                 // the paths, each from the tree's root to the node
  const long long* out_off;        // [n_pairs] the pair's block in `out`, in doubles
  const long long* block_off;      // [N][n_blocks] the position of a block's first column in the node's own coordinates
  const double* ins_prob;          // [C][A]
  const double* log_cpt_weight;    // [C]
  const double* mats;              // [2][C][N][A][A]
  const double* E;
  const double* logE;
  double* out;                     // per pair [len(node)][C][A]
};

// y = x M with M staged in a wave's LDS: transposed where the row routine runs (sp_rows<TA>), as it is otherwise
template <int TA>
__device__ __forceinline__ void vec_mat(const HX_LDS double* L, const int A, const double (&x)[sp_ax<TA>], double (&y)[sp_ax<TA>]) {
  if constexpr (sp_rows<TA>) {
    lds_mat_vec<TA>(L, x, [&](const int q, const double ya, const double yb) { y[2 * q] = ya; y[2 * q + 1] = yb; });
  } else {
    for (int b = 0; b < A; ++b) {
      double s = 0.;
      for (int a = 0; a < A; ++a) s += x[a] * L[a * A + b];
      y[b] = s;
    }
  }
}

// A lane per column, a wave per component, like k_history_columns; reads the history, writes `out` only.  Per pair the
// way down (SumProduct::fillDown, src/sumprod.cpp:163-198) along the one path from the tree's root to the node: every
// lane walks the same path and starts with insProb at the path node that is its column's root; the nodes between a
// column's root and an ungapped node are ungapped (hx_history_create's contract), so a started lane multiplies at every
// further step: G[r] = (G[parent] * E[sibling]) exp(R t)_r, logG[r] = logG[parent] + logE[sibling].  The branch matrix is
// staged once per (pair, path node) and wave, skipped where no lane of the wave has started.  Then the profile, in the
// reference's order of additions; row p of the pair's block is the node's p-th ungapped column.
template <int TA>
__global__ void __launch_bounds__(512) k_history_excluded(const HxArgs h) {
  constexpr int AX = sp_ax<TA>;
  const int A = TA ? TA : h.A, C = h.C, N = h.N, AA = A * A;
  // The launch plan is hx_history_create's (sp_column_plan: the same waves, the same bytes), so the [C][64] likelihoods of
  // k_history_columns lie in front of the matrices here too; this kernel does not touch them (512 C bytes idle: it costs
  // occupancy at large C, where a plan of its own would fit more workgroups to a CU).
  extern __shared__ double sh_ll[];                 // [C][64] (not used), then per wave [A * A]: exp(R t)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  HX_LDS double* Lsub = (HX_LDS double*)(sh_ll + 64 * C + AA * wave);
  for (long long base = (long long)blockIdx.x * 64; base < h.n_cols; base += (long long)gridDim.x * 64) {
    const bool busy = base + lane < h.n_cols;
    const long long col = base + lane;               // (< ncp)
    const SpBlock blk{base >> 6, C, N, (A + 1) & ~1, lane};
    const int root = h.root[col];
    for (int cpt = wave; cpt < C; cpt += Wb) {
      CMat ins = cmat(h.ins_prob + cpt * A);
      const double lcw = h.log_cpt_weight[cpt];
      for (int k = 0; k < h.n_pairs; ++k) {
        const int node = h.pair[4 * k], excl = h.pair[4 * k + 1], path_at = h.pair[4 * k + 2], path_len = h.pair[4 * k + 3];
        const int tk = busy ? h.tok[node * h.ncp + col] : -2;
        const bool live = tk != -2;
        const unsigned long long present = __ballot(live);
        if (!present) continue;                      // (the whole wave: the node is a gap in all 64 columns)
        double g[AX];
        double lg = 0.;
        bool started = false;
        for (int j = 0; path_at >= 0 && j < path_len; ++j) {
          const int r = h.path[path_at + j];
          const bool on = live && started;
          if (live && r == root) {
#pragma unroll
            for (int a = 0; a < A; ++a) g[a] = ins[a];
            started = true;
          }
          if (!__any(on)) continue;                  // (the whole wave; j = 0, the tree's root, always comes here)
          const int inf = h.info[r];
          wave_lds_sync();                           // (the reads of the previous matrix are done)
          lds_stage<sp_rows<TA>>(Lsub, h.mats + ((((long long)(inf >> 1) & 1) * C + cpt) * N + r) * AA, A, lane);
          wave_lds_sync();
          if (!on) continue;
          const int p = h.path[path_at + j - 1];
          const int sib = h.child[2 * p] == r ? h.child[2 * p + 1] : h.child[2 * p];
          double d[AX];
#pragma unroll
          for (int a = 0; a < A; ++a) d[a] = g[a];
          if (sib >= 0 && h.tok[sib * h.ncp + col] != -2) {
            const int ss = h.info[sib] & 1;
            const long long ats = blk.node(cpt, sib);
            lg += blk.lg(h.logE + ss * h.lg_slot, ats);
            get_row<TA>(blk.row(h.E + ss * h.e_slot, ats), A, [&](const int a, const double e) { d[a] *= e; });
          }
          vec_mat<TA>(Lsub, A, d, g);
        }
        if (!live) continue;
        const long long pos = h.block_off[node * h.n_blocks + blk.cb] + __builtin_popcountll(present & ((1ull << lane) - 1));
        double* o = h.out + h.out_off[k] + (pos * C + cpt) * A;
        // the children other than the excluded one that send a message (a gap's is all ones: log 1 + 0)
        const int c0 = h.child[2 * node], c1 = h.child[2 * node + 1];
        const bool h0 = c0 >= 0 && c0 != excl && h.tok[c0 * h.ncp + col] != -2, h1 = c1 >= 0 && c1 != excl && h.tok[c1 * h.ncp + col] != -2;
        const int s0 = h0 ? h.info[c0] & 1 : 0, s1 = h1 ? h.info[c1] & 1 : 0;
        const long long at0 = blk.node(cpt, c0), at1 = blk.node(cpt, c1);
        const double* e0 = blk.row(h.E + s0 * h.e_slot, at0);
        const double* e1 = blk.row(h.E + s1 * h.e_slot, at1);
        const double l0 = h0 ? blk.lg(h.logE + s0 * h.lg_slot, at0) : 0., l1 = h1 ? blk.lg(h.logE + s1 * h.lg_slot, at1) : 0.;
        const bool down = path_at >= 0;
        if (tk >= 0) {
          double v = 0. + lcw;
          if (h0) v += log(sp_at(e0, tk)) + l0;
          if (h1) v += log(sp_at(e1, tk)) + l1;
          if (down) {
            double gt = 0.;
#pragma unroll
            for (int a = 0; a < A; ++a) gt = a == tk ? g[a] : gt;
            v += log(gt) + lg;
          }
          for (int a = 0; a < A; ++a) o[a] = a == tk ? v : HX_NEG_INF;
          continue;
        }
        double v[AX];
#pragma unroll
        for (int a = 0; a < A; ++a) v[a] = 0. + lcw;
        if (h0) get_row<TA>(e0, A, [&](const int a, const double e) { v[a] += log(e) + l0; });
        if (h1) get_row<TA>(e1, A, [&](const int a, const double e) { v[a] += log(e) + l1; });
#pragma unroll
        for (int a = 0; a < A; ++a) o[a] = down ? v[a] + (log(g[a]) + lg) : v[a];
      }
    }
  }
}

// The normalisation of the compacted profiles, a lane per position: norm is log_accum_exp folded over v[c][i], c major and
// i minor, from -inf (src/sumprod.cpp:226, 242); then every entry has it subtracted.
__global__ void __launch_bounds__(256) k_history_excluded_norm(const long long* __restrict__ out_off, const long long* __restrict__ out_len, const int n_pairs,
                                                               const int row, double* __restrict__ out, const double* __restrict__ lse_tab) {
  for (int k = (int)blockIdx.y; k < n_pairs; k += (int)gridDim.y) {
    const long long len = out_len[k];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < len; p += (long long)gridDim.x * blockDim.x) {
      double* o = out + out_off[k] + p * row;
      double norm = HX_NEG_INF;
      for (int q = 0; q < row; ++q) norm = lse(norm, o[q], lse_tab);
      for (int q = 0; q < row; ++q) o[q] -= norm;
    }
  }
}

// ---- the hand-off to the branch DP (hx_history_branch_batch_create): TreeAlignFuncs::calcInsProbs and preMultiply
// (src/sampler.cpp:452-476) of a child's excluded-parent profile, which k_history_excluded wrote to the batch's y_sub ----
struct HbJob {
  const double* log_sub;           // [C][A][A] log exp(R t) of the branch, row = parent residue
  const double* log_ins;           // [C][A]
  double* y_sub;                   // [y_len][C][A]: the child's profile, then (in place) preMultiply of it
  double* y_emit;                  // [y_len]
  long long y_len;
};

// calcInsProbs, a lane per position: the table log_sum_exp folded over (lcw[c] + log_ins[c][a]) + child[c][a], c major
// and a minor, from -inf.  Runs before k_history_pre_multiply overwrites the profile.
__global__ void __launch_bounds__(256) k_history_ins_probs(const HbJob* __restrict__ jobs, const int n_jobs, const int C, const int A,
                                                           const double* __restrict__ log_cpt_weight, const double* __restrict__ lse_tab) {
  for (int k = (int)blockIdx.y; k < n_jobs; k += (int)gridDim.y) {
    const HbJob J = jobs[k];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < J.y_len; p += (long long)gridDim.x * blockDim.x) {
      const double* v = J.y_sub + p * C * A;
      double s = HX_NEG_INF;
      for (int c = 0; c < C; ++c) {
        const double lcw = log_cpt_weight[c];
        for (int a = 0; a < A; ++a) s = lse(s, (lcw + J.log_ins[c * A + a]) + v[c * A + a], lse_tab);
      }
      J.y_emit[p] = s;
    }
  }
}

// preMultiply in place: out[pos][c][a] = the table log_sum_exp folded over log_sub[c][a][b] + child[pos][c][b], b ascending,
// from -inf.  A workgroup takes (job, component, tile of P positions): log_sub[c] lies in LDS as [b][a], so the lanes of a
// wave - neighbouring a of one position - read neighbouring words while child[pos][c][b] is one word for all of them; the
// tile's rows are staged before any of them is overwritten, and no other workgroup touches them.  One component's matrix
// at a time: C does not enter the LDS plan (8 A (A + P) bytes).  Every output is one thread's serial chain of A sums.
__global__ void __launch_bounds__(256) k_history_pre_multiply(const HbJob* __restrict__ jobs, const int n_jobs, const int C, const int A, const int P,
                                                              const double* __restrict__ lse_tab) {
  extern __shared__ double sh_pm[];                  // [A][A] log_sub[c] transposed, then [P][A] the child rows of the tile
  double* Ls = sh_pm;
  double* Lc = sh_pm + A * A;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  // (every trip count below is uniform over the workgroup: the barriers are reached by all of it)
  for (int k = (int)blockIdx.z; k < n_jobs; k += (int)gridDim.z) {
    const HbJob J = jobs[k];
    const long long tiles = (J.y_len + P - 1) / P;
    if ((long long)blockIdx.x >= tiles) continue;
    for (int c = (int)blockIdx.y; c < C; c += (int)gridDim.y) {
      __syncthreads();                               // (the reads of the previous matrix are done)
      for (int e = tid; e < A * A; e += nt) Ls[(e % A) * A + e / A] = J.log_sub[(long long)c * A * A + e];
      for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * P;
        const int n = (int)(J.y_len - p0 < P ? J.y_len - p0 : P) * A;
        __syncthreads();                             // (the matrix is staged; the reads of the previous tile are done)
        for (int e = tid; e < n; e += nt) Lc[e] = J.y_sub[((p0 + e / A) * C + c) * A + e % A];
        __syncthreads();
        for (int e = tid; e < n; e += nt) {
          const int pl = e / A, a = e % A;
          double acc = HX_NEG_INF;
          for (int b = 0; b < A; ++b) acc = lse(acc, Ls[b * A + a] + Lc[pl * A + b], lse_tab);
          J.y_sub[((p0 + pl) * C + c) * A + a] = acc;
        }
      }
    }
  }
}

}  // namespace

}  // namespace hx

using namespace hx;

// (file scope: the opaque type of include/historian_hip.h)
struct hx_history {
  int A = 0, C = 0, N = 0, device = 0;
  long long n_cols = 0, ncp = 0;
  std::vector<int> parent, child;
  std::vector<unsigned char> eslot, mslot;           // per node: the current slot of its messages and of its matrix
  std::vector<int> changed, walked;                  // of the pending proposal
  bool pending = false, have_counts = false;
  int cur = 0;                                       // which of d_cll / d_sum is current
  SpUpload model;                                    // the roots, the tree, the info words, the walk and the changed nodes, the mixture
  DevBuf tok, mats, stage, E, logE, cll, sum, counts, rate;
  std::vector<double> max_abs;                       // [C] the largest |element| of each rate matrix; empty: no rates are set
  ExpmPlan expm = {};                                // k_branch_expm's workgroup, made when the rates were set
  const int *d_root = nullptr, *d_child = nullptr, *d_parent = nullptr;
  int *d_walk = nullptr, *d_info = nullptr;
  const double *d_ins = nullptr, *d_lcw = nullptr;
  long long e_slot = 0, lg_slot = 0;
  int tpb = 64;
  size_t lds = 0;
  float ms = 0.f, expm_ms = 0.f;                      // of the last evaluation: all its kernels; k_branch_expm alone
  float handoff_ms[3] = {0.f, 0.f, 0.f};             // of the last hx_history_branch_batch_create: profiles, insertion scores, preMultiply
  DevEvents<4> ev;                                   // around the kernels of the last call: first, last, and two in between
  // excluded-neighbour queries: the positions of every node (host, from the tokens at create), their block offsets on the
  // device from the first query on, the query's plan and its output (both grow to the largest query so far)
  std::vector<long long> row_len, block_off;
  DevBuf d_block_off, query, xout;
  size_t query_bytes = 0, xout_doubles = 0;
};

namespace {

// One evaluation: the slots of this proposal to the device, the column kernel over `walked`, the sum.  Returns when done.
// new_mats: [changed][C][A][A] on the host, or null; lengths: [changed] the new branch lengths (the root's is not read), or
// null: the matrices are computed in place from the history's rates.  Both null: the matrices are in place already.
int history_run(hx_history* h, const std::vector<int>& changed, const std::vector<int>& walked, const double* new_mats, const double* lengths, hipStream_t st,
                double* lp_sub) {
  const double* lse_tab = device_lse_table(h->device);
  if (!lse_tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_history: hx_init has not been called for the history's device");
  const int N = h->N;
  // the nodes whose matrix arrives: all the changed ones of an upload; of a proposal of lengths, those with a branch
  std::vector<int> arriving;
  if (new_mats) arriving = changed;
  else if (lengths)
    for (int r : changed)
      if (r != N - 1) arriving.push_back(r);
  // the words, then (8-byte aligned) the shape of the series of every (arriving node, component)
  const size_t n_words = (N + walked.size() + arriving.size() + 1) & ~(size_t)1;
  const size_t n_shapes = lengths ? arriving.size() * (size_t)h->C : 0;
  static_assert(sizeof(ExpmShape) == 6 * sizeof(int), "ExpmShape is counted in words below and in hx_history_create");
  std::vector<int> info(n_words + 6 * n_shapes);
  std::vector<unsigned char> is_changed(N, 0), is_walked(N, 0);
  for (int r : changed) is_changed[r] = 1;
  for (int r : walked) is_walked[r] = 1;
  for (int r = 0; r < N; ++r)
    info[r] = (is_walked[r] ? (h->eslot[r] ^ 1) : h->eslot[r]) | ((is_changed[r] ? (h->mslot[r] ^ 1) : h->mslot[r]) << 1) | (is_walked[r] << 2);
  std::copy(walked.begin(), walked.end(), info.begin() + N);
  std::copy(arriving.begin(), arriving.end(), info.begin() + N + walked.size());
  if (lengths) {
    size_t q = 0;
    for (size_t k = 0; k < changed.size(); ++k) {
      if (changed[k] == N - 1) continue;
      for (int cpt = 0; cpt < h->C; ++cpt, ++q) {
        const ExpmShape s = expm_shape(h->max_abs[cpt], lengths[k]);
        memcpy(info.data() + n_words + 6 * q, &s, sizeof s);
      }
    }
  }
  // (the info words, the walk, the arriving nodes and the shapes are adjacent on the device: one copy; the matrices: another)
  const size_t CAA = (size_t)h->C * h->A * h->A;
  if (hipMemcpy(h->d_info, info.data(), info.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      (new_mats && hipMemcpy(h->stage.as<void>(), new_mats, changed.size() * CAA * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
    return api_fail(HX_ERR_HIP, "hx_history: copy failed");
  HsArgs a;
  a.A = h->A; a.C = h->C; a.N = N; a.n_walk = (int)walked.size();
  a.n_cols = h->n_cols; a.ncp = h->ncp; a.e_slot = h->e_slot; a.lg_slot = h->lg_slot;
  a.tok = h->tok.as<const signed char>();
  a.root = h->d_root; a.child = h->d_child; a.walk = h->d_walk; a.info = h->d_info;
  a.ins_prob = h->d_ins; a.log_cpt_weight = h->d_lcw;
  a.mats = h->mats.as<const double>();
  a.E = h->E.as<double>(); a.logE = h->logE.as<double>();
  double* cll = h->cll.as<double>();
  double* sum = h->sum.as<double>();
  a.cll_cur = cll + h->cur * h->ncp;
  a.cll_new = cll + (h->cur ^ 1) * h->ncp;
  const long long blocks64 = h->ncp / 64;
  const unsigned blocks = (unsigned)(blocks64 > 65535 ? 65535 : blocks64);
  (void)hipEventRecord(h->ev[0], st);
  if (lengths && launch_branch_expm(h->expm, h->rate.as<const double>(), reinterpret_cast<const ExpmShape*>(h->d_info + n_words), h->d_walk + walked.size(),
                                    h->d_info, (int)arriving.size(), h->A, h->C, N, h->mats.as<double>(), st) != 0)
    return api_fail(HX_ERR_INVALID_ARG, launch_error());
  if (lengths) (void)hipEventRecord(h->ev[2], st);
  if (new_mats)
    hipLaunchKernelGGL(k_history_scatter, dim3((unsigned)(changed.size() * h->C)), dim3(256), 0, st, h->stage.as<const double>(),
                       h->d_walk + walked.size(), h->d_info, h->C, N, h->A * h->A, h->mats.as<double>());
  if (h->A == 4) hipLaunchKernelGGL(k_history_columns<4>, dim3(blocks), dim3(h->tpb), h->lds, st, a, lse_tab);
  else if (h->A == 20) hipLaunchKernelGGL(k_history_columns<20>, dim3(blocks), dim3(h->tpb), h->lds, st, a, lse_tab);
  else hipLaunchKernelGGL(k_history_columns<0>, dim3(blocks), dim3(h->tpb), h->lds, st, a, lse_tab);
  hipLaunchKernelGGL(k_history_sum, dim3(1), dim3(1024), 0, st, a.cll_new, h->n_cols, sum + (h->cur ^ 1));
  (void)hipEventRecord(h->ev[1], st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_history: kernel launch or execution failed");
  (void)hipEventElapsedTime(&h->ms, h->ev[0], h->ev[1]);
  h->expm_ms = 0.f;
  if (lengths) (void)hipEventElapsedTime(&h->expm_ms, h->ev[0], h->ev[2]);
  if (lp_sub && hipMemcpy(lp_sub, sum + (h->cur ^ 1), sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_history: copy failed");
  return HX_OK;
}

void history_commit(hx_history* h, const std::vector<int>& changed, const std::vector<int>& walked) {
  for (int r : changed) h->mslot[r] ^= 1;
  for (int r : walked) h->eslot[r] ^= 1;
  h->cur ^= 1;
}

// The rate matrices [C][A][A] to the device and the largest |element| of each to the host.  max_abs: checked by the caller
// (history_check_rates) before anything is allocated.
int history_put_rates(hx_history* h, const char* fn, const double* rate, const std::vector<double>& max_abs, const ExpmPlan& plan) {
  const size_t bytes = (size_t)h->C * h->A * h->A * sizeof(double);
  if (!h->rate && !h->rate.alloc(bytes)) return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  if (hipMemcpy(h->rate.as<void>(), rate, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    h->max_abs.clear();                              // (what the buffer holds is unknown: no rates are set)
    return sp_fail(HX_ERR_HIP, fn, "copy failed");
  }
  h->max_abs = max_abs;
  h->expm = plan;
  return HX_OK;
}

int history_check_rates(const char* fn, const double* rate, const int A, const int C, std::vector<double>& max_abs, ExpmPlan& plan) {
  max_abs.assign(C, 0.);
  for (int cpt = 0; cpt < C; ++cpt)
    if (!expm_max_abs(rate + (size_t)cpt * A * A, A * A, &max_abs[cpt])) return sp_fail(HX_ERR_RANGE, fn, "a rate that is NaN or infinite");
  if (!branch_expm_plan(A, &plan)) return sp_fail(HX_ERR_INVALID_ARG, fn, "the LDS plan of k_branch_expm exceeds the LDS of a CU");
  return HX_OK;
}

// a length the series of every component can be shaped for
bool history_length_ok(const std::vector<double>& max_abs, const double t) {
  if (!expm_length_ok(t)) return false;
  for (const double m : max_abs)
    if (!expm_norm_ok(m, t)) return false;
  return true;
}

// hx_history_create (branch_sub) and hx_history_create_from_lengths (rate, lengths)
int history_create(const char* fn, const hx_history_model* hm, const int8_t* tokens, int64_t n_cols, const double* branch_sub, const double* rate,
                   const double* lengths, void* stream, hx_history** out) {
  const int A = hm->alph_size, C = hm->components, N = hm->n_nodes, AA = A * A;
  int device = 0;
  const double* lse_tab = nullptr;
  std::vector<int> child;
  if (int rc = sp_check_model(fn, A > 0 && C > 0 && N > 0 && hm->parent && hm->ins_prob && hm->log_cpt_weight, A, C, HX_ERR_RANGE, &device, &lse_tab)) return rc;
  if (int rc = sp_children(fn, hm->parent, N, true, HX_ERR_RANGE, child)) return rc;
  std::vector<double> max_abs;
  ExpmPlan expm = {};
  if (rate) {
    if (int rc = history_check_rates(fn, rate, A, C, max_abs, expm)) return rc;
    for (int r = 0; r < N - 1; ++r)
      if (!history_length_ok(max_abs, lengths[r])) return sp_fail(HX_ERR_RANGE, fn, "a branch length that is negative, NaN or infinite");
  }
  // the token check in the same pass over the tokens as the transpose and the search for the roots
  const long long ncp = (n_cols + 63) & ~63LL;
  std::vector<signed char> tokT((size_t)N * ncp, (signed char)-2);
  std::vector<int> root((size_t)ncp, -1);
  for (int64_t c = 0; c < n_cols; ++c) {
    const int8_t* t = tokens + c * N;
    int roots = 0;
    for (int r = 0; r < N; ++r) {
      if (!sp_token_ok(t[r], A)) return sp_fail(HX_ERR_RANGE, fn, "a token outside -2 .. alphabet size - 1");
      tokT[(size_t)r * ncp + c] = t[r];
      if (t[r] != -2 && (r == N - 1 || t[hm->parent[r]] == -2)) { root[c] = r; ++roots; }
    }
    if (roots > 1) return sp_fail(HX_ERR_INVALID_ARG, fn, "the ungapped nodes of a column do not form one subtree");
  }
  // the LDS plans, checked before anything is allocated
  const SpPlan plan = sp_column_plan(A, C, 1, true);
  const size_t sum_lds = sizeof(double) * 1024, indel_lds = sizeof(long long) * 4 * 64 * 12;
  if (plan.lds > HX_LDS_LIMIT || sum_lds > HX_LDS_LIMIT || indel_lds > HX_LDS_LIMIT) return sp_fail(HX_ERR_INVALID_ARG, fn, "the LDS plan exceeds the LDS of a CU");
  hx_history* h = new (std::nothrow) hx_history;
  if (!h) return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "out of host memory");
  struct Guard { hx_history* h; ~Guard() { delete h; } } guard{h};
  h->A = A; h->C = C; h->N = N; h->device = device; h->n_cols = n_cols; h->ncp = ncp;
  h->parent.assign(hm->parent, hm->parent + N);
  h->child = child;
  history_positions(tokT.data(), N, ncp, h->row_len, h->block_off);
  h->eslot.assign(N, 0);
  h->mslot.assign(N, 1);                             // (the first evaluation "changes" every branch: its matrices go to slot 0)
  h->tpb = 64 * plan.waves;
  h->lds = plan.lds;
  const int AP = (A + 1) & ~1;
  h->e_slot = (ncp / 64) * (long long)C * N * AP * 64;
  h->lg_slot = (ncp / 64) * (long long)C * N * 64;
  const size_t n_mat = (size_t)C * N * AA;
  // [N] info words, the walk [<= N], the arriving nodes [<= N], a word of padding, six words per (node, component) of shapes
  const size_t n_info = 3 * (size_t)N + 2 + 6 * (size_t)N * C;
  SpUpload& up = h->model;
  if (!h->tok.alloc((size_t)N * ncp) ||
      !up.alloc(SpUpload::room((size_t)ncp * sizeof(int)) + sp_tree_room(A, C, N, false) + SpUpload::room(n_info * sizeof(int))) ||
      !h->mats.alloc(2 * n_mat * sizeof(double)) || !h->stage.alloc(n_mat * sizeof(double)) ||
      !h->E.alloc(2 * (size_t)h->e_slot * sizeof(double)) || !h->logE.alloc(2 * (size_t)h->lg_slot * sizeof(double)) ||
      !h->cll.alloc(2 * (size_t)ncp * sizeof(double)) || !h->sum.alloc(2 * sizeof(double)) ||
      !h->counts.alloc((size_t)N * 12 * sizeof(long long)))
    return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  h->d_root = up.put(root.data(), root.size());
  const SpTree tr = sp_put_tree(up, A, C, N, hm->parent, child, hm->ins_prob, hm->log_cpt_weight, nullptr);
  h->d_child = tr.child; h->d_parent = tr.parent; h->d_ins = tr.ins_prob; h->d_lcw = tr.log_cpt_weight;
  h->d_info = up.reserve<int>(n_info);
  h->d_walk = h->d_info + N;
  // the root's matrix is never read; the caller's [C][N][A][A] goes to slot 0 whole, or exp(R t) of every branch is computed there
  if (!up.copied || hipMemcpy(h->tok.as<void>(), tokT.data(), tokT.size(), hipMemcpyHostToDevice) != hipSuccess ||
      (branch_sub && hipMemcpy(h->mats.as<void>(), branch_sub, n_mat * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemset(h->cll.as<void>(), 0, 2 * (size_t)ncp * sizeof(double)) != hipSuccess)
    return sp_fail(HX_ERR_HIP, fn, "copy failed");
  if (rate)
    if (int rc = history_put_rates(h, fn, rate, max_abs, expm)) return rc;
  if (!h->ev.create())
    return sp_fail(HX_ERR_HIP, fn, "HIP call failed");
  // the full evaluation: the proposal that changes and walks every node, accepted
  std::vector<int> all(N);
  for (int r = 0; r < N; ++r) all[r] = r;
  const int rc = history_run(h, all, all, nullptr, rate ? lengths : nullptr, static_cast<hipStream_t>(stream), nullptr);
  if (rc != HX_OK) return rc;
  history_commit(h, all, all);
  guard.h = nullptr;
  *out = h;
  return HX_OK;
}

// hx_history_propose (branch_sub) and hx_history_propose_lengths (lengths): every refusal comes before anything is launched
int history_propose(const char* fn, hx_history* h, const int n_changed, const int32_t* nodes, const double* branch_sub, const double* lengths, double* lp_sub,
                    void* stream) {
  if (h->pending) return sp_fail(HX_ERR_STATE, fn, "a proposal is pending (accept or reject it first)");
  if (lengths && h->max_abs.empty()) return sp_fail(HX_ERR_STATE, fn, "no rates are set (hx_history_set_rates)");
  // the nodes to recompute: the changed ones and their ancestors, ascending (children before parents)
  std::vector<int> changed, walked;
  switch (history_closure(h->parent, n_changed, nodes, changed, walked)) {
    case 1: return sp_fail(HX_ERR_RANGE, fn, "a node outside 0 .. N - 2 (the root has no branch)");
    case 2: return sp_fail(HX_ERR_INVALID_ARG, fn, "a node named twice");
    default: break;
  }
  for (int k = 0; lengths && k < n_changed; ++k)
    if (!history_length_ok(h->max_abs, lengths[k])) return sp_fail(HX_ERR_RANGE, fn, "a branch length that is negative, NaN or infinite");
  // (the new matrices go to the slot the current ones are not in: history_run)
  const int rc = history_run(h, changed, walked, branch_sub, lengths, static_cast<hipStream_t>(stream), lp_sub);
  if (rc != HX_OK) return rc;
  h->changed.swap(changed);
  h->walked.swap(walked);
  h->pending = true;
  return HX_OK;
}

// The kernels of an excluded-neighbour query on `st`, not waited for: the plan to the device (with `extra`, which the
// caller's further kernels read at *d_extra), k_history_excluded and, if asked for, the normalisation.  The pairs' blocks
// lie at out_base + plan.out_off (doubles); out_base null: in the history's own buffer, grown to plan.total.  ev[0] is recorded
// in front.  Nothing of the history's state is written.
int history_excluded_launch(hx_history* h, const char* fn, const int which, const int n_pairs, const ExcludedPlan& plan, const int normalize, double* out_base,
                            const void* extra, const size_t extra_bytes, const void** d_extra, const SpPlan& col_plan, const double* lse_tab, hipStream_t st) {
  const int N = h->N, C = h->C, A = h->A;
  // the slots of the state asked for: the pending proposal's messages of the walked nodes and matrices of the changed ones
  // lie in the other slot (history_run's info words)
  std::vector<int> info(N);
  for (int r = 0; r < N; ++r) info[r] = h->eslot[r] | (h->mslot[r] << 1);
  if (which == 1) {
    for (int r : h->walked) info[r] ^= 1;
    for (int r : h->changed) info[r] ^= 2;
  }
  // one block: the offsets and lengths (8-byte words first), the info words, the pairs, the paths
  const size_t n_ll = 2 * (size_t)n_pairs, n_int = info.size() + plan.pair.size() + plan.path.size();
  std::vector<long long> block(n_ll + (n_int + 1) / 2);
  std::copy(plan.out_off.begin(), plan.out_off.end(), block.begin());
  std::copy(plan.out_len.begin(), plan.out_len.end(), block.begin() + n_pairs);
  int* words = reinterpret_cast<int*>(block.data() + n_ll);
  std::copy(info.begin(), info.end(), words);
  std::copy(plan.pair.begin(), plan.pair.end(), words + N);
  std::copy(plan.path.begin(), plan.path.end(), words + N + plan.pair.size());
  const size_t extra_at = block.size() * sizeof(long long);
  block.resize(block.size() + (extra_bytes + 7) / 8);
  if (extra_bytes) memcpy(reinterpret_cast<char*>(block.data()) + extra_at, extra, extra_bytes);
  const size_t bytes = block.size() * sizeof(long long);
  if (bytes > h->query_bytes) {
    h->query.reset(); h->query_bytes = 0;
    if (!h->query.alloc(bytes)) return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
    h->query_bytes = bytes;
  }
  if (!out_base && (size_t)plan.total > h->xout_doubles) {
    h->xout.reset(); h->xout_doubles = 0;
    if (!h->xout.alloc((size_t)plan.total * sizeof(double))) return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
    h->xout_doubles = (size_t)plan.total;
  }
  if (!h->d_block_off) {
    const size_t off_bytes = h->block_off.size() * sizeof(long long);
    if (!h->d_block_off.alloc(off_bytes)) return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
    if (hipMemcpy(h->d_block_off.as<void>(), h->block_off.data(), off_bytes, hipMemcpyHostToDevice) != hipSuccess) {
      h->d_block_off.reset();
      return sp_fail(HX_ERR_HIP, fn, "copy failed");
    }
  }
  if (hipMemcpy(h->query.as<void>(), block.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "copy failed");
  const long long* d_ll = h->query.as<const long long>();
  if (d_extra) *d_extra = h->query.as<const char>() + extra_at;
  const int* d_words = reinterpret_cast<const int*>(d_ll + n_ll);
  HxArgs a;
  a.A = A; a.C = C; a.N = N; a.n_pairs = n_pairs;
  a.n_cols = h->n_cols; a.ncp = h->ncp; a.n_blocks = h->ncp / 64; a.e_slot = h->e_slot; a.lg_slot = h->lg_slot;
  a.tok = h->tok.as<const signed char>();
  a.root = h->d_root; a.child = h->d_child;
  a.info = d_words; a.pair = d_words + N; a.path = d_words + N + plan.pair.size();
  a.out_off = d_ll; a.block_off = h->d_block_off.as<const long long>();
  a.ins_prob = h->d_ins; a.log_cpt_weight = h->d_lcw;
  a.mats = h->mats.as<const double>();
  a.E = h->E.as<const double>(); a.logE = h->logE.as<const double>();
  a.out = out_base ? out_base : h->xout.as<double>();
  const long long blocks64 = h->ncp / 64;
  const unsigned blocks = (unsigned)(blocks64 > 65535 ? 65535 : blocks64);
  const unsigned tpb = 64 * (unsigned)col_plan.waves;
  (void)hipEventRecord(h->ev[0], st);
  if (A == 4) hipLaunchKernelGGL(k_history_excluded<4>, dim3(blocks), dim3(tpb), col_plan.lds, st, a);
  else if (A == 20) hipLaunchKernelGGL(k_history_excluded<20>, dim3(blocks), dim3(tpb), col_plan.lds, st, a);
  else hipLaunchKernelGGL(k_history_excluded<0>, dim3(blocks), dim3(tpb), col_plan.lds, st, a);
  if (normalize) {
    const long long nb = (plan.max_len + 255) / 256;
    hipLaunchKernelGGL(k_history_excluded_norm, dim3((unsigned)(nb > 65535 ? 65535 : nb), (unsigned)(n_pairs > 65535 ? 65535 : n_pairs)), dim3(256), 0, st, d_ll,
                       d_ll + n_pairs, n_pairs, C * A, a.out, lse_tab);
  }
  return HX_OK;
}

}  // namespace

extern "C" {

int hx_history_create(const hx_history_model* hm, const int8_t* tokens, int64_t n_cols, const double* branch_sub, void* stream, hx_history** out) {
  if (!out) return api_fail(HX_ERR_INVALID_ARG, "hx_history_create: null argument");
  *out = nullptr;
  if (!hm || !tokens || !branch_sub || n_cols <= 0) return api_fail(HX_ERR_INVALID_ARG, "hx_history_create: null argument or no columns");
  return history_create("hx_history_create", hm, tokens, n_cols, branch_sub, nullptr, nullptr, stream, out);
}

int hx_history_create_from_lengths(const hx_history_model* hm, const int8_t* tokens, int64_t n_cols, const double* rate, const double* lengths, void* stream,
                                   hx_history** out) {
  if (!out) return api_fail(HX_ERR_INVALID_ARG, "hx_history_create_from_lengths: null argument");
  *out = nullptr;
  if (!hm || !tokens || !rate || !lengths || n_cols <= 0) return api_fail(HX_ERR_INVALID_ARG, "hx_history_create_from_lengths: null argument or no columns");
  return history_create("hx_history_create_from_lengths", hm, tokens, n_cols, nullptr, rate, lengths, stream, out);
}

int hx_history_set_rates(hx_history* h, const double* rate) {
  const char* fn = "hx_history_set_rates";
  if (!h || !rate) return sp_fail(HX_ERR_INVALID_ARG, fn, "null argument");
  if (h->pending) return sp_fail(HX_ERR_STATE, fn, "a proposal is pending (accept or reject it first)");
  std::vector<double> max_abs;
  ExpmPlan plan = {};
  if (int rc = history_check_rates(fn, rate, h->A, h->C, max_abs, plan)) return rc;
  return history_put_rates(h, fn, rate, max_abs, plan);
}

int hx_history_destroy(hx_history* h) {
  delete h;
  return HX_OK;
}

int hx_history_propose(hx_history* h, int32_t n_changed, const int32_t* nodes, const double* branch_sub, double* lp_sub, void* stream) {
  if (!h || !nodes || !branch_sub || n_changed <= 0) return api_fail(HX_ERR_INVALID_ARG, "hx_history_propose: null argument or no nodes");
  return history_propose("hx_history_propose", h, n_changed, nodes, branch_sub, nullptr, lp_sub, stream);
}

int hx_history_propose_lengths(hx_history* h, int32_t n_changed, const int32_t* nodes, const double* lengths, double* lp_sub, void* stream) {
  if (!h || !nodes || !lengths || n_changed <= 0) return api_fail(HX_ERR_INVALID_ARG, "hx_history_propose_lengths: null argument or no nodes");
  return history_propose("hx_history_propose_lengths", h, n_changed, nodes, nullptr, lengths, lp_sub, stream);
}

int hx_history_branch_matrix(hx_history* h, int32_t which, int32_t node, double* out) {
  const char* fn = "hx_history_branch_matrix";
  if (!h || !out || (which != 0 && which != 1)) return sp_fail(HX_ERR_INVALID_ARG, fn, "null argument, or `which` not 0 or 1");
  if (node < 0 || node >= h->N - 1) return sp_fail(HX_ERR_RANGE, fn, "a node outside 0 .. N - 2 (the root has no branch)");
  if (which == 1 && !h->pending) return sp_fail(HX_ERR_STATE, fn, "no proposal is pending");
  int slot = h->mslot[node];
  if (which == 1 && std::find(h->changed.begin(), h->changed.end(), (int)node) != h->changed.end()) slot ^= 1;
  // the node's C matrices lie N matrices apart
  const size_t mat = (size_t)h->A * h->A * sizeof(double);
  const double* src = h->mats.as<const double>() + ((size_t)slot * h->C * h->N + node) * h->A * h->A;
  if (hipMemcpy2D(out, mat, src, mat * h->N, mat, (size_t)h->C, hipMemcpyDeviceToHost) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "copy failed");
  return HX_OK;
}

int hx_history_accept(hx_history* h) {
  if (!h) return api_fail(HX_ERR_INVALID_ARG, "hx_history_accept: null argument");
  if (!h->pending) return api_fail(HX_ERR_STATE, "hx_history_accept: no proposal is pending");
  history_commit(h, h->changed, h->walked);
  h->pending = false;
  return HX_OK;
}

int hx_history_reject(hx_history* h) {
  if (!h) return api_fail(HX_ERR_INVALID_ARG, "hx_history_reject: null argument");
  if (!h->pending) return api_fail(HX_ERR_STATE, "hx_history_reject: no proposal is pending");
  h->pending = false;
  return HX_OK;
}

int hx_history_log_like(hx_history* h, int32_t which, double* lp_sub, double* col_log_like) {
  if (!h || (which != 0 && which != 1)) return api_fail(HX_ERR_INVALID_ARG, "hx_history_log_like: null argument, or `which` not 0 or 1");
  if (which == 1 && !h->pending) return api_fail(HX_ERR_STATE, "hx_history_log_like: no proposal is pending");
  const int s = h->cur ^ which;
  if ((lp_sub && hipMemcpy(lp_sub, h->sum.as<double>() + s, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
      (col_log_like && hipMemcpy(col_log_like, h->cll.as<double>() + s * h->ncp, (size_t)h->n_cols * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
    return api_fail(HX_ERR_HIP, "hx_history_log_like: copy failed");
  return HX_OK;
}

int hx_history_indel_counts(hx_history* h, int64_t* counts) {
  if (!h || !counts) return api_fail(HX_ERR_INVALID_ARG, "hx_history_indel_counts: null argument");
  if (!h->have_counts) {                             // (the alignment is fixed: counted once, on the null stream)
    hipLaunchKernelGGL(k_history_indels, dim3((unsigned)((h->N + 3) / 4)), dim3(256), 0, (hipStream_t) nullptr, h->tok.as<const signed char>(),
                       h->d_parent, h->N, h->n_cols, h->ncp, h->counts.as<long long>());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
      return api_fail(HX_ERR_HIP, "hx_history_indel_counts: kernel launch or execution failed");
    h->have_counts = true;
  }
  if (hipMemcpy(counts, h->counts.as<void>(), (size_t)h->N * 12 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_history_indel_counts: copy failed");
  return HX_OK;
}

int hx_history_row_lengths(hx_history* h, int64_t* len) {
  if (!h || !len) return api_fail(HX_ERR_INVALID_ARG, "hx_history_row_lengths: null argument");
  for (int r = 0; r < h->N; ++r) len[r] = h->row_len[r];
  return HX_OK;
}

int hx_history_excluded_profiles(hx_history* h, int32_t which, int32_t n_pairs, const int32_t* node, const int32_t* exclude, int32_t normalize, double* const* out,
                                 void* stream) {
  const char* fn = "hx_history_excluded_profiles";
  if (!h || !node || !exclude || !out || n_pairs <= 0 || (which != 0 && which != 1)) return sp_fail(HX_ERR_INVALID_ARG, fn, "null argument, no pairs, or `which` not 0 or 1");
  const int C = h->C, A = h->A;
  ExcludedPlan plan;
  switch (history_excluded_plan(h->parent, h->row_len, (long long)C * A, n_pairs, node, exclude, plan)) {
    case 1: return sp_fail(HX_ERR_RANGE, fn, "a node or neighbour outside 0 .. N - 1");
    case 2: return sp_fail(HX_ERR_INVALID_ARG, fn, "an excluded neighbour that is neither the node's parent nor its child");
    default: break;
  }
  for (int k = 0; k < n_pairs; ++k)
    if (plan.out_len[k] > 0 && !out[k]) return sp_fail(HX_ERR_INVALID_ARG, fn, "null argument");
  if (which == 1 && !h->pending) return sp_fail(HX_ERR_STATE, fn, "no proposal is pending");
  const double* lse_tab = device_lse_table(h->device);
  if (!lse_tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_history: hx_init has not been called for the history's device");
  const SpPlan col_plan = sp_column_plan(A, C, 1, true);
  if (col_plan.lds > HX_LDS_LIMIT) return sp_fail(HX_ERR_INVALID_ARG, fn, "the LDS plan exceeds the LDS of a CU");
  if (plan.total == 0) {                             // (no node has a position: nothing to compute)
    h->ms = h->expm_ms = 0.f;
    return HX_OK;
  }
  const int rc = history_excluded_launch(h, fn, which, n_pairs, plan, normalize, nullptr, nullptr, 0, nullptr, col_plan, lse_tab, static_cast<hipStream_t>(stream));
  if (rc != HX_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double* xout = h->xout.as<const double>();
  (void)hipEventRecord(h->ev[1], st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "kernel launch or execution failed");
  (void)hipEventElapsedTime(&h->ms, h->ev[0], h->ev[1]);
  h->expm_ms = 0.f;
  for (int k = 0; k < n_pairs; ++k)
    if (plan.out_len[k] > 0 &&
        hipMemcpy(out[k], xout + plan.out_off[k], (size_t)plan.out_len[k] * C * A * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return sp_fail(HX_ERR_HIP, fn, "copy failed");
  return HX_OK;
}

int hx_history_branch_batch_create(hx_history* h, int32_t which, int32_t normalize, const hx_history_branch* branches, int32_t n_branches, void* stream,
                                   hx_branch_batch** out) {
  const char* fn = "hx_history_branch_batch_create";
  if (out) *out = nullptr;
  if (!h || !branches || !out || n_branches <= 0 || (which != 0 && which != 1))
    return sp_fail(HX_ERR_INVALID_ARG, fn, "null argument, no branches, or `which` not 0 or 1");
  const int C = h->C, A = h->A;
  BranchHandoffPlan bp;
  switch (history_branch_plan(h->parent, h->row_len, A, C, branches, n_branches, branch_max_x_len(), bp)) {
    case 1: return sp_fail(HX_ERR_RANGE, fn, "a node outside 0 .. N - 2 (the root has no branch)");
    case 2: return sp_fail(HX_ERR_INVALID_ARG, fn, "a null log_sub or log_ins, or a band without both envelopes");
    case 3: return sp_fail(HX_ERR_RANGE, fn, "a parent row of more than 65535 positions");
    default: break;
  }
  if (which == 1 && !h->pending) return sp_fail(HX_ERR_STATE, fn, "no proposal is pending");
  const double* lse_tab = device_lse_table(h->device);
  if (!lse_tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_history: hx_init has not been called for the history's device");
  const SpPlan col_plan = sp_column_plan(A, C, 1, true);
  // k_history_pre_multiply's tile: 64 positions, 32 of a large alphabet (48 KB of LDS at A = 64)
  const int P = A > 32 ? 32 : 64;
  const size_t pm_lds = sizeof(double) * (size_t)A * (A + P);
  if (col_plan.lds > HX_LDS_LIMIT || pm_lds > HX_LDS_LIMIT) return sp_fail(HX_ERR_INVALID_ARG, fn, "the LDS plan exceeds the LDS of a CU");
  ExcludedPlan plan;
  const int n_pairs = 2 * n_branches;
  if (history_excluded_plan(h->parent, h->row_len, (long long)C * A, n_pairs, bp.node.data(), bp.exclude.data(), plan) != 0)
    return sp_fail(HX_ERR_INVALID_ARG, fn, "the branches do not make a plan");
  if (hipSetDevice(h->device) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "hipSetDevice failed");
  // the batch: the small inputs and the caller's logs through the host image, room for what the kernels write
  std::vector<const double*> log_sub(n_branches), log_ins(n_branches);
  for (int k = 0; k < n_branches; ++k) { log_sub[k] = branches[k].log_sub; log_ins[k] = branches[k].log_ins; }
  std::vector<BranchInputs> where(n_branches);
  hx_branch_batch* b = nullptr;
  if (const int rc = branch_batch_reserve(bp.jobs.data(), log_sub.data(), log_ins.data(), n_branches, &b, where.data())) return rc;
  struct Guard { hx_branch_batch* b; ~Guard() { if (b) (void)hx_branch_batch_destroy(b); } } guard{b};
  // the profiles go straight to x_pwm and y_sub: the pairs' blocks as offsets from the first job's x_pwm
  double* base = where[0].x_pwm;
  std::vector<HbJob> jobs(n_branches);
  long long max_y = 0;
  for (int k = 0; k < n_branches; ++k) {
    plan.out_off[2 * k] = where[k].x_pwm - base;
    plan.out_off[2 * k + 1] = where[k].y_sub - base;
    jobs[k] = HbJob{where[k].log_sub, where[k].log_ins, where[k].y_sub, where[k].y_emit, plan.out_len[2 * k + 1]};
    max_y = std::max(max_y, jobs[k].y_len);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  h->handoff_ms[0] = h->handoff_ms[1] = h->handoff_ms[2] = 0.f;
  if (plan.total == 0) {                             // (no row has a position: nothing to compute)
    h->ms = h->expm_ms = 0.f;
    guard.b = nullptr;
    *out = b;
    return HX_OK;
  }
  const void* d_jobs_v = nullptr;
  if (const int rc = history_excluded_launch(h, fn, which, n_pairs, plan, normalize, base, jobs.data(), sizeof(HbJob) * jobs.size(), &d_jobs_v, col_plan, lse_tab, st))
    return rc;
  const HbJob* d_jobs = static_cast<const HbJob*>(d_jobs_v);
  (void)hipEventRecord(h->ev[2], st);
  if (max_y > 0) {
    const unsigned gz = (unsigned)(n_branches > 65535 ? 65535 : n_branches);
    const long long nb = (max_y + 255) / 256, tiles = (max_y + P - 1) / P;
    hipLaunchKernelGGL(k_history_ins_probs, dim3((unsigned)(nb > 65535 ? 65535 : nb), gz), dim3(256), 0, st, d_jobs, n_branches, C, A, h->d_lcw, lse_tab);
    (void)hipEventRecord(h->ev[3], st);
    hipLaunchKernelGGL(k_history_pre_multiply, dim3((unsigned)(tiles > 65535 ? 65535 : tiles), (unsigned)C, gz), dim3(256), pm_lds, st, d_jobs, n_branches, C, A, P,
                       lse_tab);
  } else {
    (void)hipEventRecord(h->ev[3], st);
  }
  (void)hipEventRecord(h->ev[1], st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "kernel launch or execution failed");
  (void)hipEventElapsedTime(&h->ms, h->ev[0], h->ev[1]);
  (void)hipEventElapsedTime(&h->handoff_ms[0], h->ev[0], h->ev[2]);
  (void)hipEventElapsedTime(&h->handoff_ms[1], h->ev[2], h->ev[3]);
  (void)hipEventElapsedTime(&h->handoff_ms[2], h->ev[3], h->ev[1]);
  h->expm_ms = 0.f;
  guard.b = nullptr;
  *out = b;
  return HX_OK;
}

int hx_history_last_handoff_ms(hx_history* h, float* ms) {
  if (!h || !ms) return api_fail(HX_ERR_INVALID_ARG, "hx_history_last_handoff_ms: null argument");
  for (int k = 0; k < 3; ++k) ms[k] = h->handoff_ms[k];
  return HX_OK;
}

int hx_history_last_kernel_ms(hx_history* h, float* ms) {
  if (!h || !ms) return api_fail(HX_ERR_INVALID_ARG, "hx_history_last_kernel_ms: null argument");
  *ms = h->ms;
  return HX_OK;
}

int hx_history_last_expm_ms(hx_history* h, float* ms) {
  if (!h || !ms) return api_fail(HX_ERR_INVALID_ARG, "hx_history_last_expm_ms: null argument");
  *ms = h->expm_ms;
  return HX_OK;
}

}  // extern "C"
