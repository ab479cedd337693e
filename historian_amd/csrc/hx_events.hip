// Expected indel events of a pair DP whose profiles carry event counts of their own (hx_batch_event_counts).
//
// BackwardMatrix::getCounts restricted to the IndelCounts members (reference src/forward.cpp:1183-1214) with the carried
// terms of transitionEigenCounts (:579-584): every source transition of every in-envelope cell is weighted with its
// posterior probability w = exp(F(src) + lp + B(dest) - lpEnd); it adds its pair-HMM events (the dest.state switch,
// :585-649) and, where it moves along a transition of a child profile, that transition's carried counts.  The carried
// part is linear in the weights, so it is taken as a contraction: the posterior of each profile transition (the sum of
// the weights of the source transitions that use it) times its six carried numbers.
//
// No floating-point atomics: every sum runs in an order fixed by the pair's shape, so two runs agree bit for bit.
//   k_event_posts, blockIdx.y = 0: a workgroup per row dx (grid-stride over rows).  x-transitions end at row dx; for each
//     in-slot of state dx in turn, the workgroup's threads walk the row's columns and add the weights of the sources that
//     move along that slot (dest states IMM, IMD, IIW), then reduce them in a fixed tree.  The events of those sources are
//     summed on the way.
//   blockIdx.y = 1: a workgroup per column dy, the same for y-transitions (dest states IMM, IDM, IMI); the events of the
//     sources that move y but not x are summed there (the others were counted by the rows), so every source transition
//     adds its events exactly once.
//   k_event_finish: one workgroup adds the per-workgroup event partials in order and contracts the posteriors with the
//     carried tables.
// Transitions into the profiles' END states get no posterior: getCounts stops before the end cell (its carried counts are
// zero in every profile makeProfile builds).
#include <hip/hip_runtime.h>
#include "hx_common.h"
#include "hx_kernels.h"

namespace hx {

namespace {

constexpr int EV_THREADS = 256;

// which factors a source cell of (dx, dy, ds) may differ in, and lpCellEmitOrAbsorb of the destination: the case analysis of
// sourceTransitionsWithoutEmitOrAbsorb (src/forward.cpp:326-398), as k_indel_counts has it
struct Moves {
  bool move_x, move_y, hmm, any;
  double lp_abs;
};

__device__ __forceinline__ Moves dest_moves(const DevJob& J, const FwdPack& xp, const FwdPack& yp, int dx, int dy, int ds,
                                            const double* __restrict__ tab, int plane_valid) {
  const int xf = xp.meta & 0xFF, yf = yp.meta & 0xFF;
  const bool x_null = xf & F_NULL, y_null = yf & F_NULL;
  const bool x_ready = (xf & F_READY) || J.x.empty, y_ready = (yf & F_READY) || J.y.empty;
  Moves m{false, false, false, false, 0.};
  if (ds == 1 || ds == 4) {
    m.move_x = true;
    if (x_null) m.any = y_ready && dx < J.x.n - 1;
    else { m.any = y_ready; m.hmm = true; m.lp_abs = ds == 1 ? xp.rootsub : xp.ins; }
  } else if (ds == 2 || ds == 3) {
    m.move_y = true;
    if (y_null) m.any = dy < J.y.n - 1;
    else { m.any = x_ready; m.hmm = true; m.lp_abs = ds == 2 ? yp.rootsub : yp.ins; }
  } else {
    if (y_null && (xf & F_EMIT_OR_START)) { m.move_y = true; m.any = dy < J.y.n - 1; }
    else if (x_null) { m.move_x = true; m.any = y_ready && dx < J.x.n - 1; }
    else if (!y_null) {
      m.move_x = m.move_y = m.hmm = m.any = true;
      if (J.emis) {
        const int cx = xp.cls, cy = yp.cls;
        m.lp_abs = (cx < 0 || cy < 0) ? HX_NEG_INF : J.emis[(size_t)cx * J.y.n_cls + cy];
      } else if (plane_valid)
        m.lp_abs = J.emis_plane[cell_slot(J.strip_stride, dx, dy)];
      else
        m.lp_abs = emission(J, dx, dy, tab);
    }
  }
  return m;
}

// in-slot k of a state: source state and lpTrans (the first HX_DAG_INLINE inline in the record, the others in the CSR)
__device__ __forceinline__ void in_slot(const DevProfile& P, const FwdPack& p, int k, int& src, double& lp) {
  if (k < HX_DAG_INLINE) { src = k == 0 ? p.s0 : k == 1 ? p.s1 : p.s2; lp = k == 0 ? p.lp0 : k == 1 ? p.lp1 : p.lp2; }
  else { src = P.in_src[p.in_b + k]; lp = P.in_lp[p.in_b + k]; }
}

// a stored Forward cell, or -inf outside the storage or the envelope (as the traceback reads it)
__device__ __forceinline__ double fwd_cell(const DevJob& J, int i, int j, int s) {
  if (i < 0 || j < 0 || i >= J.n_rows || j >= J.n_cols || !in_envelope(J, i, j)) return HX_NEG_INF;
  const int64_t slot = stored_slot(J, i, j);
  return slot < 0 ? HX_NEG_INF : J.fwd[(int64_t)s * J.plane + slot];
}

// transitionEigenCounts, dest.state switch (src/forward.cpp:585-649), weighted with w
__device__ __forceinline__ void add_events(double* c, double w, int s, int ds, bool x_null, bool y_null, const double* tm) {
  const double l_t = tm[0], r_t = tm[1], l_iw = tm[2], l_dw = tm[3], r_iw = tm[4], r_dw = tm[5];
  if (ds == 0) {
    if (!x_null && !y_null) {
      if (s == 0 || s == 1) { c[4] += w * l_t; c[5] += w * l_t; }
      if (s == 0 || s == 2) { c[4] += w * r_t; c[5] += w * r_t; }
    }
  } else if (ds == 1) {
    if (!x_null) {
      if (s == 0 || s == 1) { c[4] += w * l_t; c[5] += w * l_t; }
      if (s == 1) c[3] += w;
      else { c[1] += w; c[5] += w * r_dw; }
    }
  } else if (ds == 4) {
    if (!x_null) {
      if (s == 4) c[2] += w;
      else { c[0] += w; c[4] += w * l_iw; }
    }
  } else if (ds == 2) {
    if (!y_null) {
      if (s == 0 || s == 2) { c[4] += w * r_t; c[5] += w * r_t; }
      if (s == 2) c[3] += w;
      else { c[1] += w; c[5] += w * l_dw; }
    }
  } else {
    if (!y_null) {
      if (s == 3) c[2] += w;
      else { c[0] += w; c[4] += w * r_iw; }
    }
  }
}

// sum of v over the workgroup in a fixed tree; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = EV_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

}  // namespace

// posts: blockIdx.y = 0 rows (x-transitions), 1 columns (y-transitions).  x_post / y_post [T] are zero on entry; in_idx maps a
// CSR in-slot to its transition index.  part: [2][gridDim.x][6] event partials.
__global__ __launch_bounds__(EV_THREADS) void k_event_posts(const DevJob* __restrict__ jobs, const int job, const double* __restrict__ tm,
                                                            const int32_t* __restrict__ x_in_idx, const int32_t* __restrict__ y_in_idx,
                                                            double* __restrict__ x_post, double* __restrict__ y_post,
                                                            double* __restrict__ part, const double* __restrict__ tab, const int plane_valid) {
  __shared__ double red[EV_THREADS];
  const DevJob& J = jobs[job];
  const int R = J.n_rows, Cc = J.n_cols;
  const double lp_end = *J.lp_end;
  const bool by_rows = blockIdx.y == 0;
  const int n_lines = by_rows ? R : Cc, line_len = by_rows ? Cc : R;
  double c[6] = {0., 0., 0., 0., 0., 0.};
  for (int line = blockIdx.x; line < n_lines && lp_end > HX_NEG_INF; line += gridDim.x) {
    const DevProfile& P = by_rows ? J.x : J.y;
    const FwdPack lp_rec = P.fpack[line];
    const int deg = lp_rec.meta >> 8;
    for (int k = 0; k < deg; ++k) {
      int ksrc;
      double klp;
      in_slot(P, lp_rec, k, ksrc, klp);
      double acc = 0.;
      for (int o = threadIdx.x; o < line_len; o += EV_THREADS) {
        const int dx = by_rows ? line : o, dy = by_rows ? o : line;
        if (!in_envelope(J, dx, dy)) continue;
        const FwdPack xp = J.x.fpack[dx], yp = J.y.fpack[dy];
        const bool x_null = (xp.meta & 0xFF) & F_NULL, y_null = (yp.meta & 0xFF) & F_NULL;
        const int64_t bslot = cell_slot_blk(J.strip_stride, J.blk, R - 1 - dx, Cc - 1 - dy);   // mirrored (hx_layout)
        for (int ds = 0; ds < 5; ++ds) {
          if (by_rows ? (ds == 2 || ds == 3) : (ds == 1 || ds == 4)) continue;
          const double lp_dest = J.bwd[(int64_t)ds * J.plane + bslot];
          if (!(lp_dest > HX_NEG_INF)) continue;
          const Moves m = dest_moves(J, xp, yp, dx, dy, ds, tab, plane_valid);
          if (!m.any || !(by_rows ? m.move_x : m.move_y)) continue;
          // events: rows take every source that moves x, columns the ones that move y only
          const bool events = by_rows || !m.move_x;
          const int n_other = by_rows ? (m.move_y ? (yp.meta >> 8) : 1) : (m.move_x ? (xp.meta >> 8) : 1);
          const int ns = m.hmm ? 5 : 1;
          for (int q = 0; q < n_other; ++q) {
            int sx = dx, sy = dy;
            double xlp = 0., ylp = 0.;
            if (by_rows) {
              sx = ksrc; xlp = klp;
              if (m.move_y) in_slot(J.y, yp, q, sy, ylp);
            } else {
              sy = ksrc; ylp = klp;
              if (m.move_x) in_slot(J.x, xp, q, sx, xlp);
            }
            for (int si = 0; si < ns; ++si) {
              const int s = m.hmm ? si : ds;
              const double h = m.hmm ? J.T[si][ds] : 0.;
              const double f = fwd_cell(J, sx, sy, s);
              const double lw = (f + ((((h + xlp) + ylp) + m.lp_abs))) + lp_dest - lp_end;
              if (!(lw > HX_NEG_INF)) continue;
              const double w = exp(lw);
              acc += w;
              if (events) add_events(c, w, s, ds, x_null, y_null, tm);
            }
          }
        }
      }
      const double post = block_sum(acc, red);
      if (threadIdx.x == 0) {
        const int slot = lp_rec.in_b + k;
        if (by_rows) x_post[x_in_idx[slot]] = post;
        else y_post[y_in_idx[slot]] = post;
      }
    }
  }
  double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
#pragma unroll
  for (int e = 0; e < 6; ++e) {   // (unrolled: the counts stay in registers, no scratch)
    const double v = block_sum(c[e], red);
    if (threadIdx.x == 0) out[e] = v;
  }
}

// out[6] = the event partials of both halves in order + sum_t x_post[t] * x_counts[t][.] + sum_t y_post[t] * y_counts[t][.]
// (x_counts / y_counts may be null: no carried counts on that side)
__global__ __launch_bounds__(EV_THREADS) void k_event_finish(const double* __restrict__ part, const int n_part,
                                                             const double* __restrict__ x_post, const double* __restrict__ x_counts, const int x_T,
                                                             const double* __restrict__ y_post, const double* __restrict__ y_counts, const int y_T,
                                                             double* __restrict__ out) {
  __shared__ double red[EV_THREADS];
  for (int e = 0; e < 6; ++e) {
    double v = 0.;
    for (int p = threadIdx.x; p < n_part; p += EV_THREADS) v += part[(size_t)p * 6 + e];
    if (x_counts)
      for (int t = threadIdx.x; t < x_T; t += EV_THREADS) v += x_post[t] * x_counts[(size_t)t * 6 + e];
    if (y_counts)
      for (int t = threadIdx.x; t < y_T; t += EV_THREADS) v += y_post[t] * y_counts[(size_t)t * 6 + e];
    const double s = block_sum(v, red);
    if (threadIdx.x == 0) out[e] = s;
  }
}

int event_counts_grid(int n_rows, int n_cols) {
  const int m = n_rows > n_cols ? n_rows : n_cols;
  return m < 1 ? 1 : (m > 1024 ? 1024 : m);
}

void launch_event_counts(const DevJob* d_jobs, int job, const double* d_tm, const int32_t* x_in_idx, const int32_t* y_in_idx,
                         double* d_x_post, double* d_y_post, const double* d_x_counts, int x_T, const double* d_y_counts, int y_T,
                         double* d_part, int grid, double* d_out, Tab8 tab8, bool plane_valid, hipStream_t st) {
  hipLaunchKernelGGL(k_event_posts, dim3((unsigned)grid, 2), dim3(EV_THREADS), 0, st, d_jobs, job, d_tm, x_in_idx, y_in_idx, d_x_post,
                     d_y_post, d_part, tab8.p, plane_valid ? 1 : 0);
  hipLaunchKernelGGL(k_event_finish, dim3(1), dim3(EV_THREADS), 0, st, d_part, 2 * grid, d_x_post, d_x_counts, x_T, d_y_post,
                     d_y_counts, y_T, d_out);
}

}  // namespace hx
