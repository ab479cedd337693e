// Column sum-product on a phylogenetic tree and the eigen-basis substitution-count accumulation of counts mode
// (SURVEY 8f row N3): the reference's SumProduct::initColumn / fillUp / fillDown (src/sumprod.cpp:58-198),
// accumulateRootCounts and accumulateEigenCounts (src/sumprod.cpp:264-271, 294-372), for a BATCH of alignment columns.
//
// In the reference one SumProduct object walks the columns one after the other (AlignColSumProduct, and once per
// posterior-weighted DP cell in BackwardMatrix::getCounts).  Columns and mixture components are independent, so here a
// (column, component) is a thread (k_sumprod_columns): every thread runs the tip-to-root and root-to-tip passes of its column - tiny tree recursions,
// A x A matrix-vector products per branch and mixture component, the steps of hx_sumprod.h - with its messages E, F, G in a global scratch laid out
// in blocks of 64 columns ([block][.][64 lanes], two vector entries per lane and access), then turns the messages of every branch
// into the eigen basis (D_k, U_l).  The reference adds weight x D_k J_kl U_l to the count matrix column by column; J_kl
// (eigenSubCount of the branch) does not depend on the column, so the sum over columns is an outer-product sum
// J_kl x sum_col D_k(col) U_l(col): a second kernel (k_outer_counts) reduces the columns of one (component, branch) per
// workgroup, A x A accumulators in registers, the bases staged through LDS, and multiplies by J once at the end.  When
// every eigenvector is real (reversible models: all the reference's presets) the imaginary halves are neither written nor
// read.  Root counts are written per column and summed by rows (k_row_sums).
//
// Arithmetic follows the reference: linear-space messages with per-node log scale factors, rescaling below 1e-30, the
// column likelihood combined over components with the table log_sum_exp.  Sums over columns are taken in a different
// order from the reference's: results agree to rounding (tests/test_gpu_sumprod.py: 1e-10), not bit for bit.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/historian_hip.h"
#include "hx_lse.h"
#include "hx_policy.h"
#include "hx_kernels.h"
#include "hx_sumprod.h"

namespace hx {

namespace {

#define HX_SP_TILE 32              // columns per LDS tile of k_outer_counts
#ifndef HX_SP_WAVES_PER_SIMD
#define HX_SP_WAVES_PER_SIMD 2    // the column kernel's register budget: 512 / this.  Four waves per SIMD (128 registers, 49 spilled doubles)
                                  // run at the same rate: the kernel is bound by the traffic it moves, not by the latency it hides
#endif
#define HX_SP_PAIRS 16             // (k,l) pairs per thread of k_outer_counts: A*A <= 256 * 16, A <= 64

struct SpModel {
  int A, C, N, real_basis;
  const int* parent;               // [N] post-order: children before parents, root last; -1 for the root
  const int* child;                // [N][2] children or -1 (binary trees, as the reconstruction builds them)
  const double* ins_prob;          // [C][A]
  const double* log_cpt_weight;    // [C]
  const double* branch_sub;        // [C][N][A][A] exp(R t_r)
  const double* evec_re;           // [C][A][A] right eigenvectors, and their inverse
  const double* evec_im;
  const double* einv_re;
  const double* einv_im;
  const double* esc_re;            // [C][N][A][A] eigenSubCount(t_r)
  const double* esc_im;
};

// scratch of one chunk of columns, in blocks of 64 columns: messages E, G [block][cpt][node][a][64]; scale factors and max U
// [block][cpt][node][64]; F at the column's root and the root-count terms [block][cpt][a][64]; bases
// [block][cpt][node][Ur, Dr, (Ui, Di)][a][64]
struct SpScratch { double* E; double* G; double* logE; double* logF; double* logG; double* maxU; double* Froot; double* rootc; double* basis; };

// TA, LM: see hx_sumprod.h.  With LM a wave keeps three matrices in LDS - exp(R t) of the branch at hand (re-staged per
// node), the real parts of the eigenvectors and of their inverse (per component); through the scalar cache the 3 KB per
// matrix-vector product overrun it (2.9 TFLOP/s, one FMA per ~100 cycles).
template <int TA, bool LM>
__global__ void __launch_bounds__(512, HX_SP_WAVES_PER_SIMD) k_sumprod_columns(const SpModel m, const signed char* __restrict__ tok, const double* __restrict__ weight,
                                                         const long long n_cols, const SpScratch s, const double* __restrict__ lse_tab,
                                                         double* __restrict__ col_log_like, double* __restrict__ root_post) {
  constexpr int AX = sp_ax<TA>;
  const int A = TA ? TA : m.A, C = m.C, N = m.N, AA = A * A;
  const int parts = m.real_basis ? 2 : 4;
  // a wavefront is 64 columns of one mixture component (the component is uniform over the wave, so the model's matrices
  // still come through scalar loads); the waves of a workgroup share the columns and split the components.  They meet
  // twice: for the column likelihood (through LDS) and for the root posterior (through the scratch).
  extern __shared__ double sh_ll[];                 // [C][64], then per wave [3][A * A]: exp(R t), evecInv, evec (real parts)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, Wb = (int)blockDim.x >> 6;
  HX_LDS double* Lsub = (HX_LDS double*)(sh_ll + 64 * C + (LM ? 3 * AA * wave : 0));
  HX_LDS double* Linv = Lsub + AA;
  HX_LDS double* Lvec = Linv + AA;
  for (long long base = (long long)blockIdx.x * 64; base < n_cols; base += (long long)gridDim.x * 64) {
    const bool busy = base + lane < n_cols;
    const long long col = busy ? base + lane : 0;
    const SpBlock blk{base >> 6, C, N, (A + 1) & ~1, lane};
    // the bases of a node: parts rows, U then D (real, then imaginary); F at the root and the root-count terms [cpt][a][64]
    auto basis = [&](const long long at, const int part) { return blk.row(s.basis, at * parts + part); };
    auto froot = [&](const int cpt, const int a) -> double& { return s.Froot[((blk.cb * C + cpt) * A + a) * 64 + lane]; };
    const signed char* t = tok + col * N;       // -2 gap, -1 wildcard, else the residue's token
    const double w = weight ? weight[col] : 1.;
    const int root = column_root(t, m.parent, N);
    // ---- tip-to-root (src/sumprod.cpp:99-161); U of every branch in the eigen basis on the way (src/sumprod.cpp:318-340) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      double cpt_ll = 0.;
      CMat ins = cmat(m.ins_prob + cpt * A);
      const double* invg = m.einv_re + (long long)cpt * AA;
      CMat ii = cmat(m.einv_im + (long long)cpt * AA);
      if (LM) {
        wave_lds_sync();
        lds_stage<false>(Linv, invg, A, lane);
        lds_stage<sp_rows<TA>>(Lvec, m.evec_re + (long long)cpt * AA, A, lane);     // (the root-to-tip pass multiplies with the transposed matrices)
      }
      for (int r = 0; r < N; ++r) {
        const double* subg = m.branch_sub + ((long long)cpt * N + r) * AA;
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();                               // (the reads of the previous node's matrix are done)
          lds_stage<false>(Lsub, subg, A, lane);
          wave_lds_sync();
        }
        if (!busy) continue;
        const int c0 = m.child[2 * r], c1 = m.child[2 * r + 1];
        const long long at = blk.node(cpt, r), at0 = blk.node(cpt, c0), at1 = blk.node(cpt, c1);
        double lf = (c0 >= 0 ? blk.lg(s.logE, at0) : 0.) + (c1 >= 0 ? blk.lg(s.logE, at1) : 0.);
        const int tk = t[r];
        if (tk == -2) {
          // a gap: its message to the parent is all ones, and no counts on the branch above it
          put_row<TA>(blk.row(s.E, at), A, [](int) { return 1.; });
          blk.lg(s.logE, at) = 0.;
          blk.lg(s.logF, at) = lf;
          put_row<TA>(basis(at, 0), A, [](int) { return 0.; });
          if (parts == 4)
            for (int l = 0; l < A; ++l) sp_at(basis(at, 2), l) = 0.;
          continue;
        }
        if (tk >= 0) {
          // a residue: E and U are columns of the matrices
          const double f = residue_f(c0 >= 0, blk.row(s.E, at0), c1 >= 0, blk.row(s.E, at1), tk, lf);
          blk.lg(s.logF, at) = lf;
          if (r == root) {
#pragma unroll
            for (int a = 0; a < A; ++a) froot(cpt, a) = a == tk ? f : 0.;
            cpt_ll += lf + log(f * m.ins_prob[cpt * A + tk]);
          } else {
            blk.lg(s.logE, at) = lf;
            blk.lg(s.maxU, at) = f;
            put_row<TA>(blk.row(s.E, at), A, [&](const int a) { return (LM ? Lsub[a * A + tk] : subg[a * A + tk]) * f; });
            put_row<TA>(basis(at, 0), A, [&](const int l) { return (LM ? Linv[l * A + tk] : invg[l * A + tk]) * (f / f); });
            if (parts == 4)
              for (int l = 0; l < A; ++l) sp_at(basis(at, 2), l) = m.einv_im[(long long)cpt * AA + l * A + tk] * (f / f);
          }
          continue;
        }
        double f[AX];
        const double fmax = wild_f<TA>(c0 >= 0, blk.row(s.E, at0), c1 >= 0, blk.row(s.E, at1), A, f, lf);
        blk.lg(s.logF, at) = lf;
        if (r == root) {
#pragma unroll
          for (int a = 0; a < A; ++a) froot(cpt, a) = f[a];
          cpt_ll += wild_root_ll<TA>(f, ins, A, lf);
          continue;
        }
        blk.lg(s.logE, at) = lf;
        blk.lg(s.maxU, at) = fmax;
        mat_vec_store<TA, LM, false>(Lsub, cmat(subg), A, f, blk.row(s.E, at));
        // U = evecInv F / max F (the row routine multiplies with the inverse; the loop divides, as it always did)
        if constexpr (LM && sp_rows<TA>) {
          const double inv_fmax = 1. / fmax;
#pragma unroll
          for (int a = 0; a < A; ++a) f[a] *= inv_fmax;
        } else {
#pragma unroll
          for (int a = 0; a < A; ++a) f[a] /= fmax;
        }
        mat_vec_store<TA, LM, false>(Linv, cmat(invg), A, f, basis(at, 0));
        if (parts == 4)
          for (int l = 0; l < A; ++l) {
            double ui = 0.;
#pragma unroll
            for (int b = 0; b < A; ++b) ui += ii[l * A + b] * f[b];
            sp_at(basis(at, 2), l) = ui;
          }
      }
      sh_ll[cpt * 64 + lane] = cpt_ll;
    }
    __syncthreads();
    const double cll = combine_components(sh_ll, m.log_cpt_weight, C, lane, lse_tab);
    if (wave == 0 && busy) col_log_like[col] = cll;
    // ---- root-to-tip (src/sumprod.cpp:163-198); D of every branch in the eigen basis on the way (src/sumprod.cpp:341-360) ----
    for (int cpt = wave; cpt < C; cpt += Wb) {
      CMat ins = cmat(m.ins_prob + cpt * A);
      if (LM && C > Wb) {                            // (with a wave per component the eigenvectors are still there)
        wave_lds_sync();
        lds_stage<sp_rows<TA>>(Lvec, m.evec_re + (long long)cpt * AA, A, lane);
      }
      for (int r = N - 1; r >= 0; --r) {
        if (LM && m.parent[r] >= 0) {
          wave_lds_sync();
          lds_stage<sp_rows<TA>>(Lsub, m.branch_sub + ((long long)cpt * N + r) * AA, A, lane);
          wave_lds_sync();
        }
        if (!busy) continue;
        const long long at = blk.node(cpt, r);
        if (t[r] == -2 || r == root) {
          if (r == root) {
            put_row<TA>(blk.row(s.G, at), A, [&](const int a) { return ins[a]; });
            blk.lg(s.logG, at) = 0.;
            put_row<TA>(basis(at, 0), A, [](int) { return 0.; });         // no branch above the root: U was not written on the way up
            if (parts == 4)
              for (int l = 0; l < A; ++l) sp_at(basis(at, 2), l) = 0.;
          }
          put_row<TA>(basis(at, 1), A, [](int) { return 0.; });
          if (parts == 4)
            for (int l = 0; l < A; ++l) sp_at(basis(at, 3), l) = 0.;
          continue;
        }
        const int p = m.parent[r];
        const int sib = m.child[2 * p] == r ? m.child[2 * p + 1] : m.child[2 * p];
        const long long atp = blk.node(cpt, p), ats = blk.node(cpt, sib);
        const double le_sib = sib >= 0 ? blk.lg(s.logE, ats) : 0.;
        const double lg_p = blk.lg(s.logG, atp);
        blk.lg(s.logG, at) = lg_p + le_sib;
        // (the matrices' addresses are formed here, per node: formed once per component, above the loop over the nodes, they
        // cost the A = 4 form ten registers and its third wave per SIMD)
        CMat sub_s = cmat(m.branch_sub + ((long long)cpt * N + r) * AA);
        CMat vr_s = cmat(m.evec_re + (long long)cpt * AA);
        CMat vi = cmat(m.evec_im + (long long)cpt * AA);
        // what flows down the branch: the parent's outside message times the sibling's subtree
        double d[AX];
        const double max_d = row_product<TA>(true, blk.row(s.G, atp), sib >= 0, blk.row(s.E, ats), A, d);
        mat_vec_store<TA, LM, true>(Lsub, sub_s, A, d, blk.row(s.G, at));
        const double norm = exp(cll - m.log_cpt_weight[cpt] - blk.lg(s.logF, at) - lg_p - le_sib) / (blk.lg(s.maxU, at) * max_d);
        const double scale = w / norm;
        // D = (d / max d) evec, weighted
        if constexpr (LM && sp_rows<TA>) {
          const double inv_max = 1. / max_d;
#pragma unroll
          for (int a = 0; a < A; ++a) d[a] *= inv_max;
        } else {
#pragma unroll
          for (int a = 0; a < A; ++a) d[a] /= max_d;
        }
        mat_vec_store<TA, LM, true>(Lvec, vr_s, A, d, basis(at, 1), [&](int, const double dr) { return dr * scale; });
        if (parts == 4)
          for (int k = 0; k < A; ++k) {
            double di = 0.;
#pragma unroll
            for (int a = 0; a < A; ++a) di += vi[a * A + k] * d[a];
            sp_at(basis(at, 3), k) = di * scale;
          }
      }
    }
    __syncthreads();            // (the other components' F, G at the root, written to the scratch by the neighbouring threads)
    // ---- posterior of the root's residue (src/sumprod.cpp:208-217) ----
    if (root_post && busy && wave == 0)
      for (int a = 0; a < A; ++a) {
        double lp = HX_NEG_INF;
        if (root >= 0)
          for (int cpt = 0; cpt < C; ++cpt) {
            const long long at = blk.node(cpt, root);
            lp = lse(lp, m.log_cpt_weight[cpt] + blk.lg(s.logF, at) + log(froot(cpt, a)) + blk.lg(s.logG, at) + log(sp_at(blk.row(s.G, at), a)) - cll, lse_tab);
          }
        root_post[col * A + a] = lp < 0. ? lp : 0.;
      }
    // ---- this column's terms of the root counts (src/sumprod.cpp:264-271) ----
    for (int cpt = wave; cpt < C && busy; cpt += Wb) {
      const double norm = root >= 0 ? exp(m.log_cpt_weight[cpt] + blk.lg(s.logF, blk.node(cpt, root)) - cll) : 0.;
      for (int a = 0; a < A; ++a)
        s.rootc[((blk.cb * C + cpt) * A + a) * 64 + lane] = root >= 0 ? w * m.ins_prob[cpt * A + a] * froot(cpt, a) * norm : 0.;
    }
    __syncthreads();
  }
}

// eigenCounts[cpt][k][l] += J[cpt][node][k][l] * sum over this chunk's columns of D_k(col) U_l(col)   (src/sumprod.cpp:361-370)
// grid (C * N branches, column slices); 256 threads, thread t owns the pairs (k,l) = t, t + 256, ...
template <bool REAL>
__global__ void __launch_bounds__(256) k_outer_counts(const SpModel m, const double* __restrict__ basis, const long long n_cols,
                                                      double* __restrict__ eig_re, double* __restrict__ eig_im) {
  extern __shared__ double tile[];                 // [parts * A][HX_SP_TILE + 1]
  constexpr int PARTS = REAL ? 2 : 4, TS = HX_SP_TILE + 1;
  const int A = m.A, AA = A * A, N = m.N;
  const int branch = blockIdx.x, cpt = branch / N, r = branch - cpt * N;
  if (m.parent[r] < 0) return;
  const int AP = (A + 1) & ~1;
  const long long blk_doubles = (long long)m.C * N * PARTS * AP * 64;     // one 64-column block of the scratch (see k_sumprod_columns)
  const double* bs = basis + (long long)branch * PARTS * AP * 64;
  double acc_re[HX_SP_PAIRS], acc_im[HX_SP_PAIRS];
#pragma unroll
  for (int q = 0; q < HX_SP_PAIRS; ++q) acc_re[q] = acc_im[q] = 0.;
  const long long n_tiles = (n_cols + HX_SP_TILE - 1) / HX_SP_TILE;
  for (long long tl = blockIdx.y; tl < n_tiles; tl += gridDim.y) {
    const long long c0 = tl * HX_SP_TILE;
    for (int e = threadIdx.x; e < PARTS * A * HX_SP_TILE; e += 256) {
      const int row = e / HX_SP_TILE, c = e - row * HX_SP_TILE;
      const long long cc = c0 + c;
      const int part = row / A, l = row - part * A;      // (rows of a part are stored in pairs: [l / 2][64][2])
      tile[row * TS + c] = cc < n_cols ? bs[(cc >> 6) * blk_doubles + (long long)part * AP * 64 + ((l >> 1) * 64 + (cc & 63)) * 2 + (l & 1)] : 0.;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < HX_SP_PAIRS; ++q) {
      const int pr = q * 256 + threadIdx.x;
      if (q * 256 >= AA) break;
      if (pr < AA) {
        const int k = pr / A, l = pr - k * A;
        const double* u_re = tile + l * TS;
        const double* d_re = tile + (A + k) * TS;
        double sr = acc_re[q], si = acc_im[q];
        if (REAL) {
#pragma unroll 8
          for (int c = 0; c < HX_SP_TILE; ++c) sr += d_re[c] * u_re[c];
        } else {
          const double* u_im = tile + (2 * A + l) * TS;
          const double* d_im = tile + (3 * A + k) * TS;
#pragma unroll 4
          for (int c = 0; c < HX_SP_TILE; ++c) {
            sr += d_re[c] * u_re[c] - d_im[c] * u_im[c];
            si += d_re[c] * u_im[c] + d_im[c] * u_re[c];
          }
        }
        acc_re[q] = sr;
        acc_im[q] = si;
      }
    }
    __syncthreads();
  }
  const double* jr = m.esc_re + (long long)branch * AA;
  const double* ji = m.esc_im + (long long)branch * AA;
#pragma unroll
  for (int q = 0; q < HX_SP_PAIRS; ++q) {
    const int pr = q * 256 + threadIdx.x;
    if (pr < AA) {
      atomicAdd(&eig_re[(long long)cpt * AA + pr], acc_re[q] * jr[pr] - acc_im[q] * ji[pr]);
      atomicAdd(&eig_im[(long long)cpt * AA + pr], acc_re[q] * ji[pr] + acc_im[q] * jr[pr]);
    }
  }
}

// The same sum for real bases on the matrix cores: sum_col D_k(col) U_l(col) is the product D (A x columns) times U^T
// (columns x A).  A workgroup takes one (component, branch) and a slice of the 64-column blocks; a block's 2 A rows of 64
// columns are one contiguous piece of the scratch (see k_sumprod_columns), copied to LDS with rows padded to 65 entries; the
// four waves share the 16 x 16 tiles of the A x A result, sixteen v_mfma_f64_16x16x4_f64 per tile and block (k = the block's
// columns, four at a time).  Operand maps of that instruction: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; result
// register q of lane l is C[(l >> 4) + 4 q][l & 15].  Rows past A are zero in LDS.
typedef double sp_d4 __attribute__((ext_vector_type(4)));
#define HX_SP_MAX_TILES 4          // tiles per wave: A <= 64 -> (A / 16)^2 <= 16 tiles over four waves
template <int PER>                                  // 16-byte entries of a block per thread: >= ceil(A / 2) * 2 * 64 / 256
__global__ void __launch_bounds__(256) k_outer_counts_mfma(const SpModel m, const double* __restrict__ basis, const long long n_cols,
                                                           double* __restrict__ eig_re) {
  extern __shared__ double tile[];                 // [2][Mp][65]: U rows, then D rows
  const int A = m.A, AA = A * A, N = m.N;
  const int tm = (A + 15) >> 4, Mp = tm << 4, n_tiles = tm * tm;
  const int branch = blockIdx.x, cpt = branch / N, r = branch - cpt * N;
  if (m.parent[r] < 0) return;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int AP = (A + 1) & ~1;
  const long long blk_doubles = (long long)m.C * N * 2 * AP * 64;
  const double* bs = basis + (long long)branch * 2 * AP * 64;
  for (int e = threadIdx.x; e < 2 * Mp * 65; e += 256) tile[e] = 0.;
  sp_d4 acc[HX_SP_MAX_TILES];
#pragma unroll
  for (int q = 0; q < HX_SP_MAX_TILES; ++q) acc[q] = sp_d4{0., 0., 0., 0.};
  const long long n_blocks = (n_cols + 63) >> 6;
  // a block's entries travel through registers, two blocks ahead: the blocks after this one are in flight while it is multiplied
  sp_d2 bufA[PER], bufB[PER];
  const int total = AP * 64;                        // a block's U and D rows: AP / 2 row pairs of 64 lanes each, 16 bytes per entry
  const auto fetch = [&](sp_d2 (&buf)[PER], const long long b) {
    if (b >= n_blocks) return;
    const sp_d2* src = reinterpret_cast<const sp_d2*>(bs + b * blk_doubles);
    const long long c0 = b << 6;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = q * 256 + (int)threadIdx.x;
      if (q * 256 < total) {
        sp_d2 v = e < total ? src[e] : sp_d2{0., 0.};
        if (c0 + (e & 63) >= n_cols) v = sp_d2{0., 0.};
        buf[q] = v;
      }
    }
  };
  const auto multiply = [&](const sp_d2 (&buf)[PER]) {
    __syncthreads();                               // (the previous block's products are done; the first time: the zero fill)
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = q * 256 + (int)threadIdx.x;
      if (q * 256 < total && e < total) {
        // entry e: row pair e / 64 (pairs 0 .. AP/2 - 1: U, then D), column e % 64; its two values are rows 2 p and 2 p + 1
        const int pr = e >> 6, c = e & 63;
        const int part = pr >= AP / 2, l0 = 2 * (pr - part * (AP / 2));
        const int trow = part * Mp + l0;
        tile[trow * 65 + c] = buf[q].x;
        if (l0 + 1 < A) tile[(trow + 1) * 65 + c] = buf[q].y;
      }
    }
    __syncthreads();
  };
  const auto products = [&]() {
#pragma unroll
    for (int q = 0; q < HX_SP_MAX_TILES; ++q) {
      const int t = wave + 4 * q;
      if (t >= n_tiles) break;
      const int tk = t / tm, tl = t - tk * tm;
      const double* drow = tile + (Mp + 16 * tk + (lane & 15)) * 65 + (lane >> 4);
      const double* urow = tile + (16 * tl + (lane & 15)) * 65 + (lane >> 4);
      sp_d4 c = acc[q];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(drow[4 * s4], urow[4 * s4], c, 0, 0, 0);
      acc[q] = c;
    }
  };
  const long long step = gridDim.y;
  fetch(bufA, blockIdx.y);
  fetch(bufB, blockIdx.y + step);
  for (long long b = blockIdx.y; b < n_blocks; b += 2 * step) {
    multiply(bufA);
    fetch(bufA, b + 2 * step);
    products();
    if (b + step >= n_blocks) break;
    multiply(bufB);
    fetch(bufB, b + 3 * step);
    products();
  }
  const double* jr = m.esc_re + (long long)branch * AA;
#pragma unroll
  for (int q = 0; q < HX_SP_MAX_TILES; ++q) {
    const int t = wave + 4 * q;
    if (t >= n_tiles) break;
    const int tk = t / tm, tl = t - tk * tm;
    const int l = 16 * tl + (lane & 15);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = 16 * tk + (lane >> 4) + 4 * g;
      if (k < A && l < A) atomicAdd(&eig_re[(long long)cpt * AA + k * A + l], acc[q][g] * jr[k * A + l]);
    }
  }
}

// out[row] += sum of the row's n_cols entries; one workgroup per row
__global__ void __launch_bounds__(256) k_row_sums(const double* __restrict__ rows, const long long n_cols, double* __restrict__ out) {
  __shared__ double part[256];
  // rows are laid out in blocks of 64 columns: [block][row][64]
  const double* row = rows + (long long)blockIdx.x * 64;
  const long long blk_doubles = (long long)gridDim.x * 64;
  double sum = 0.;
  // grid (rows, slices of the columns): a slice's partial sum is added with one atomic
  for (long long c = (long long)blockIdx.y * 256 + threadIdx.x; c < n_cols; c += (long long)gridDim.y * 256)
    sum += row[(c >> 6) * blk_doubles + (c & 63)];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(&out[blockIdx.x], part[0]);
}

}  // namespace

thread_local float g_sp_ms = 0.f;

}  // namespace hx

using namespace hx;

extern "C" {

// See include/historian_hip.h.  One call = upload, the kernels over chunks of columns that fit the scratch budget, download.
int hx_sumprod_columns(const hx_sumprod_model* hm, const int8_t* tokens, const double* weight, int64_t n_cols, double* col_log_like,
                       double* root_counts, double* eigen_re, double* eigen_im, double* root_post, void* stream) {
  if (!hm || !tokens || n_cols <= 0 || !col_log_like || !root_counts || !eigen_re || !eigen_im)
    return api_fail(HX_ERR_INVALID_ARG, "hx_sumprod_columns: null argument or no columns");
  const char* fn = "hx_sumprod_columns";
  const int A = hm->alph_size, C = hm->components, N = hm->n_nodes, AA = A * A;
  const bool complete = A > 0 && C > 0 && N > 0 && hm->parent && hm->ins_prob && hm->log_cpt_weight && hm->branch_sub && hm->evec_re && hm->evec_im &&
                        hm->evec_inv_re && hm->evec_inv_im && hm->esc_re && hm->esc_im;
  int device = 0;
  const double* lse_tab = nullptr;
  std::vector<int> child;
  if (int rc = sp_check_model(fn, complete, A, C, HX_ERR_INVALID_ARG, &device, &lse_tab)) return rc;
  if (int rc = sp_children(fn, hm->parent, N, false, HX_ERR_INVALID_ARG, child)) return rc;
  if (int rc = sp_check_tokens(fn, tokens, n_cols * N, A)) return rc;
  bool real_basis = true;
  for (size_t k = 0; k < (size_t)C * AA && real_basis; ++k) real_basis = hm->evec_im[k] == 0. && hm->evec_inv_im[k] == 0.;
  for (size_t k = 0; k < (size_t)C * N * AA && real_basis; ++k) real_basis = hm->esc_im[k] == 0.;
  const int parts = real_basis ? 2 : 4;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SpUpload up;
  DevBuf b_tok, b_w, b_scr, b_out;
  const size_t eig = SpUpload::room((size_t)C * AA * sizeof(double)), esc = SpUpload::room((size_t)C * N * AA * sizeof(double));
  if (!up.alloc(sp_tree_room(A, C, N, true) + 4 * eig + 2 * esc) || !b_tok.alloc((size_t)n_cols * N) ||
      (weight && !b_w.alloc(n_cols * sizeof(double))))
    return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  const SpTree tr = sp_put_tree(up, A, C, N, hm->parent, child, hm->ins_prob, hm->log_cpt_weight, hm->branch_sub);
  SpModel m;
  m.A = A; m.C = C; m.N = N; m.real_basis = real_basis; m.parent = tr.parent; m.child = tr.child;
  m.ins_prob = tr.ins_prob; m.log_cpt_weight = tr.log_cpt_weight; m.branch_sub = tr.branch_sub;
  m.evec_re = up.put(hm->evec_re, (size_t)C * AA);
  m.evec_im = up.put(hm->evec_im, (size_t)C * AA);
  m.einv_re = up.put(hm->evec_inv_re, (size_t)C * AA);
  m.einv_im = up.put(hm->evec_inv_im, (size_t)C * AA);
  m.esc_re = up.put(hm->esc_re, (size_t)C * N * AA);
  m.esc_im = up.put(hm->esc_im, (size_t)C * N * AA);
  if (!up.copied || hipMemcpy(b_tok.as<void>(), tokens, (size_t)n_cols * N, hipMemcpyHostToDevice) != hipSuccess ||
      (weight && hipMemcpy(b_w.as<void>(), weight, n_cols * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
    return sp_fail(HX_ERR_HIP, fn, "copy failed");
  const int AP = (A + 1) & ~1;                     // message vectors are stored in pairs of entries
  const size_t per_col = (2 + (size_t)parts) * C * N * AP + 4 * (size_t)C * N + 2 * (size_t)C * A;
  const long long chunk = sp_chunk(per_col, n_cols);
  const size_t n_out = (size_t)n_cols * (1 + (root_post ? A : 0)) + (size_t)C * A + 2 * (size_t)C * AA;
  if (!b_scr.alloc(per_col * (((size_t)chunk + 63) & ~(size_t)63) * sizeof(double)) || !b_out.alloc(n_out * sizeof(double)))
    return sp_fail(HX_ERR_OUT_OF_MEMORY, fn, "device allocation failed");
  double* out = b_out.as<double>();
  double* d_cll = out;
  double* d_post = root_post ? out + n_cols : nullptr;
  double* d_root = out + (size_t)n_cols * (1 + (root_post ? A : 0));
  double* d_re = d_root + (size_t)C * A;
  double* d_im = d_re + (size_t)C * AA;
  if (hipMemsetAsync(d_root, 0, ((size_t)C * A + 2 * (size_t)C * AA) * sizeof(double), st) != hipSuccess)
    return sp_fail(HX_ERR_HIP, fn, "HIP call failed");
  const size_t lds = sizeof(double) * (size_t)parts * A * (HX_SP_TILE + 1);
  if (lds > HX_LDS_LIMIT) return sp_fail(HX_ERR_INVALID_ARG, fn, "basis tile exceeds the LDS of a CU");
  const SpPlan plan = sp_column_plan(A, C, 3, false);           // exp(R t), evecInv, evec
  DevEvents<2> ev;
  if (!ev.create()) return sp_fail(HX_ERR_HIP, fn, "HIP call failed");
  (void)hipEventRecord(ev[0], st);
  for (long long first = 0; first < n_cols; first += chunk) {
    const long long nc = n_cols - first < chunk ? n_cols - first : chunk;
    double* scr = b_scr.as<double>();
    SpScratch s;
    const size_t nc64 = ((size_t)nc + 63) & ~(size_t)63;         // the scratch holds whole blocks of 64 columns
    const size_t msg = (size_t)C * N * AP * nc64, lg = (size_t)C * N * nc64;
    s.E = scr; s.G = scr + msg;
    s.logE = scr + 2 * msg; s.logF = s.logE + lg; s.logG = s.logF + lg; s.maxU = s.logG + lg;
    s.Froot = s.maxU + lg;
    s.rootc = s.Froot + (size_t)C * A * nc64;
    s.basis = s.rootc + (size_t)C * A * nc64;
    long long blocks = (nc + 63) / 64;
    if (blocks > 65535) blocks = 65535;
    const signed char* d_tok = b_tok.as<const signed char>() + first * N;
    const double* d_w = b_w ? b_w.as<const double>() + first : nullptr;
    double* d_p = d_post ? d_post + first * A : nullptr;
#define HX_SP_GO(TA_, LM_) hipLaunchKernelGGL((k_sumprod_columns<TA_, LM_>), dim3((unsigned)blocks), dim3(64 * plan.waves), plan.lds, st, m, d_tok, d_w, nc, s, lse_tab, d_cll + first, d_p)
    // (A = 4 has its matrices in LDS whatever C <= 128: 512 C + 24 * 16 * min(C, 8) <= 65536 + 3072 < 98304 - no <4, false> form)
    if (A == 4) HX_SP_GO(4, true);
    else if (A == 20) { if (plan.lm) HX_SP_GO(20, true); else HX_SP_GO(20, false); }
    else { if (plan.lm) HX_SP_GO(0, true); else HX_SP_GO(0, false); }
#undef HX_SP_GO
    const long long tiles = (nc + HX_SP_TILE - 1) / HX_SP_TILE;
    long long slices = 4096 / ((long long)C * N) + 1;
    if (const char* e = getenv("HX_SUMPROD_SLICES")) slices = atoll(e);
    if (slices < 1) slices = 1;
    if (slices > tiles) slices = tiles;
    if (real_basis && sizeof(double) * 2 * (((A + 15) / 16) * 16) * 65 <= 64 * 1024 && !getenv("HX_SUMPROD_NO_MFMA")) {
      const int mp = ((A + 15) / 16) * 16;
      const long long blocks64 = (nc + 63) / 64;
      long long sl = 8192 / ((long long)C * N) + 1;          // (measured: 4.46 / 4.35 / 4.23 ms per 100 000 columns at 8 / 34 / 68 slices)
      if (const char* e = getenv("HX_SUMPROD_SLICES")) sl = atoll(e);
      if (sl < 1) sl = 1;
      if (sl > blocks64) sl = blocks64;
      const size_t tile_lds = sizeof(double) * 2 * mp * 65;
      const dim3 og((unsigned)(C * N), (unsigned)sl);
      if (AP <= 4) hipLaunchKernelGGL(k_outer_counts_mfma<1>, og, dim3(256), tile_lds, st, m, s.basis, nc, d_re);
      else if (AP <= 20) hipLaunchKernelGGL(k_outer_counts_mfma<5>, og, dim3(256), tile_lds, st, m, s.basis, nc, d_re);
      else hipLaunchKernelGGL(k_outer_counts_mfma<16>, og, dim3(256), tile_lds, st, m, s.basis, nc, d_re);
    } else if (real_basis)
      hipLaunchKernelGGL(k_outer_counts<true>, dim3((unsigned)(C * N), (unsigned)slices), dim3(256), lds, st, m, s.basis, nc, d_re, d_im);
    else
      hipLaunchKernelGGL(k_outer_counts<false>, dim3((unsigned)(C * N), (unsigned)slices), dim3(256), lds, st, m, s.basis, nc, d_re, d_im);
    {
      long long rs = (nc + 4095) / 4096;                      // at least 4 096 columns per slice
      if (rs > 64) rs = 64;
      hipLaunchKernelGGL(k_row_sums, dim3((unsigned)(C * A), (unsigned)rs), dim3(256), 0, st, s.rootc, nc, d_root);
    }
  }
  (void)hipEventRecord(ev[1], st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return sp_fail(HX_ERR_HIP, fn, "kernel launch or execution failed");
  (void)hipEventElapsedTime(&g_sp_ms, ev[0], ev[1]);
  auto down = [](double* dst, const double* src, const size_t n) { return hipMemcpy(dst, src, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess; };
  if (!down(col_log_like, d_cll, (size_t)n_cols) || (root_post && !down(root_post, d_post, (size_t)n_cols * A)) || !down(root_counts, d_root, (size_t)C * A) ||
      !down(eigen_re, d_re, (size_t)C * AA) || !down(eigen_im, d_im, (size_t)C * AA))
    return sp_fail(HX_ERR_HIP, fn, "copy failed");
  return HX_OK;
}

int hx_sumprod_last_kernel_ms(float* ms) {
  if (!ms) return HX_ERR_INVALID_ARG;
  *ms = g_sp_ms;
  return HX_OK;
}

}  // extern "C"
