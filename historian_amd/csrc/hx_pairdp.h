// What the envelope-bounded pair DPs over TreeAlignFuncs::SparseDPMatrix share on the device (hx_branch.hip: three states,
// hx_sibling.hip: eleven): the envelope test, the emission pre-pass, the clearing of a banded job's planes, the fill - one
// strip sweep, k_pair_fill, for every lattice - and what consumes a filled matrix where it lies: the dense copy, the walks (best
// path, sampled path: one wavefront per job, all jobs of a batch side by side) and the gather of cells along a path.  The host
// side - step windows, the batch object, the launches - is hx_pairbatch.h.
//
// A job type has: X, Y (positions 0 .. len of the row / column profile), C, CA, max_dist, x_pwm [X-1][CA], y_sub [Y-1][CA],
// y_emit [Y-1], x_env [X], y_env [Y], T, cells, emis, plane, strip_stride, lp_end, win.
//
// A lattice L is one struct per recursion (BranchCell<VITERBI>, SiblingCell).  What the sweep and the walks ask of it:
//   Job, NS (states = planes), ND (columns of T, the last one End), END
//   NUP, up_plane(k)   the planes a cell reads of the cell above, k < NUP; the last NDG of them are also what it reads of the
//   NDG                diagonal cell (what a lane received as "above" one step earlier: no second exchange).  Of its own
//                      previous cell it may read every state.
//   L(J)               the transition scores the cell uses, read once per wavefront
//   x_emit(J, i)       the score of entering row i (0 where rows have none)
//   cell(...)          the states of one cell from those three sources, in the reference's order of operations
//   lp_end(J, at, tab) lpEnd from the last cell's states; at(s) reads state s - the lattice asks for the states that feed End
//   column(), Emit, self_loop()      the walks: what a state emits, where lpEmit's terms lie, whether the fill eliminated a self-loop
//   BATCH_WAVES, WAVES_ENV           the launch (hx_pairbatch.h)
#pragma once
#include <hip/hip_runtime.h>
#include "hx_device.h"
#include "hx_lse.h"
#include "hx_policy.h"
#include "hx_handoff.h"
#include "../../include/historian_hip.h"

namespace hx {

// columns of the strip above's last row fetched at a time / strips whose progress a workgroup keeps in LDS / wavefronts of a
// workgroup
#define HXBR_BLK 16
#define HXBR_MAX_STRIPS 1024
#define HXBR_MAX_WAVES 16

template <class Job>
__device__ __forceinline__ bool pair_in_env(const Job& J, const int i, const int j) {
  // TreeAlignFuncs::SparseDPMatrix::inEnvelope (src/sampler.h:146-149)
  if (i == 0 || j == 0 || i == J.X - 1 || j == J.Y - 1 || J.max_dist < 0) return true;
  int d = J.x_env[i] - J.y_env[j];
  d = d < 0 ? -d : d;
  return d <= J.max_dist;
}

// logMatch for every in-envelope cell with i, j >= 1: the nested logInnerProduct of src/logsumexp.h:132-151 - over the
// components, of the sum over the residues - in the reference's table arithmetic.  It does not depend on DP values and is
// fully parallel.  grid (jobs, row slices)
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

// a banded job's planes are -inf wherever the fill does not write (as XYCell's constructor leaves a cell outside the
// envelope); an unbanded job's fill writes every cell.  grid (jobs, slices)
template <class Job, int NS>
__global__ void k_pair_clear(const Job* __restrict__ jobs) {
  const Job& J = jobs[blockIdx.x];
  if (J.max_dist < 0) return;
  const int64_t n = NS * J.plane;
  for (int64_t c = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.y * blockDim.x) J.cells[c] = HX_NEG_INF;
}

// value of lane `src` (wave-uniform)
__device__ __forceinline__ double read_lane64(const double v, const int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

typedef double d2v __attribute__((ext_vector_type(2)));

// ---- the fill ----------------------------------------------------------------------------------------------------------------
// One workgroup per job; its 64-row strips are dealt to the workgroup's wavefronts round-robin, each wavefront sweeps its
// strip on its own clock (lane <-> row, step <-> anti-diagonal): a cell's left source is the lane's own previous cell, up and
// diagonal are the previous lane's cells of one and two steps ago (DPP wave_shr:1), and what a strip needs of the strip above -
// that strip's last row - it reads from the matrix, HXBR_BLK columns at a time, handed out by v_readlane, once the wavefront
// above has said that those columns are stored: a monotonic column count per strip in LDS, published behind a drain of the
// producer's stores (the consumer's loads are agent-scope: served by L2, where the stores are by then).  A strip therefore
// starts ~HXBR_BLK + 64 steps behind the one above, and a job of S strips takes columns + ~80 (S - 1) steps instead of the
// S (columns + 63) of one wavefront per job.  Waits cannot form a cycle: strip s waits for strip s - 1 only.  The batch
// supplies the rest of the parallelism: a refinement sweep aligns every branch of a tree, the sampler many moves.
// YL: the column side of a step - the score of entering its column and the column's envelope coordinate - out of LDS (staged
// once per workgroup; the launcher checks that the longest column profile of the launch fits), not fetched from memory inside
// the step; the step's emission term is fetched one step ahead either way.
// Nothing here depends on which lattice is swept: what differs is a member of L (header of this file).  Per-cell state is
// held in small arrays with constant bounds, fully unrolled: registers.
template <class L, bool YL>
__global__ void __launch_bounds__(64 * HXBR_MAX_WAVES) k_pair_fill(const typename L::Job* __restrict__ jobs, const double* __restrict__ tab,
                                                                   const int y_cap) {
  constexpr int NS = L::NS, NUP = L::NUP, NDG = L::NDG;
  __shared__ int progress[HXBR_MAX_STRIPS];         // columns of the strip's last row that are stored
  extern __shared__ __attribute__((aligned(16))) unsigned char ydyn[];
  double* yemitL = reinterpret_cast<double*>(ydyn);                 // [y_cap]
  int* yenvL = reinterpret_cast<int*>(ydyn + 8 * (size_t)y_cap);    // [y_cap]
  const typename L::Job& J = jobs[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
  const int X = J.X, Y = J.Y;
  const int64_t plane = J.plane, ss = J.strip_stride;
  HX_GLOBAL double* __restrict__ M = as_global(J.cells);
  const HX_GLOBAL double* __restrict__ E = as_global((const double*)J.emis);
  const L lat(J);
  const int n_strips = (X + 63) >> 6;
  for (int q = threadIdx.x; q < n_strips && q < HXBR_MAX_STRIPS; q += blockDim.x) progress[q] = 0;
  if (YL)
    for (int j = threadIdx.x; j < Y; j += blockDim.x) {
      yemitL[j] = j > 0 ? J.y_emit[j - 1] : 0.0;    // (the score of entering column j: y_emit of column position j - 1)
      yenvL[j] = J.max_dist >= 0 ? J.y_env[j] : 0;
    }
  __syncthreads();
  volatile int* prog = progress;
  const double ninf = HX_NEG_INF;
  // a state of a cell as a wavefront of this workgroup stored it
  auto stored = [&](const int plane_of, const int64_t sl) -> double {
    return __hip_atomic_load(M + plane_of * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  for (int s = wave; s < n_strips; s += n_waves) {
    const int i = (s << 6) + lane;
    const bool rvalid = i < X;
    const int xe = (rvalid && J.max_dist >= 0) ? J.x_env[i] : 0;
    const double xem = (rvalid && i > 0) ? L::x_emit(J, i) : 0.0;
    const bool xedge = i == 0 || i == X - 1;
    const bool feeds = s + 1 < n_strips;            // a strip below reads this strip's last row
    double left[NS], up[NUP], diag[NDG];            // (i, j-1); (i-1, j) and (i-1, j-1) of the step being computed
    double bnd[NUP];                                // lane l < HXBR_BLK: cell (row above the strip, column c0 + l) of the current block of columns
    double held[NS];                                // the lane's cell of the even step of the current step pair
#pragma unroll
    for (int k = 0; k < NUP; ++k) bnd[k] = ninf;
#pragma unroll
    for (int k = 0; k < NS; ++k) held[k] = ninf;
    bool held_in = false;
    int seen = 0;
    // logMatch of the lane's cell of the NEXT step (column t + 1 - lane), fetched a step ahead
    auto emis_at = [&](const int jj) -> double {
      return (rvalid && i > 0 && jj > 0 && jj < Y) ? E[cell_slot(ss, i, jj)] : 0.0;
    };
    // a banded strip sweeps its step windows only (hx_pairbatch.h: branch_windows); between them nothing of the strip is
    // inside the envelope, so a window starts from -inf registers, and the strip below is told that the columns up to the
    // next window are final (they hold the -inf the planes were cleared to)
    const int32_t* wn = J.win ? J.win + 6 * s : nullptr;
    for (int wi = 0; wi < (wn ? 3 : 1); ++wi) {
    const int t0 = wn ? wn[2 * wi] : 0, t1 = wn ? wn[2 * wi + 1] : (Y + 63 + 1) & ~1;      // (whole step pairs)
    if (t1 <= t0) break;
#pragma unroll
    for (int k = 0; k < NS; ++k) left[k] = ninf;
#pragma unroll
    for (int k = 0; k < NUP; ++k) up[k] = ninf;
#pragma unroll
    for (int k = 0; k < NDG; ++k) diag[k] = ninf;
    if (s > 0 && t0 >= 1 && t0 - 1 < Y) {
      // ... except lane 0's diagonal source of the window's first step: cell (row above, column t0 - 1) belongs to the strip
      // above, whose band may well hold it
      lds_wait<2>(prog, s - 1, seen, t0);
      if (lane == 0) {
        const int64_t sl = cell_slot(ss, (s << 6) - 1, t0 - 1);
#pragma unroll
        for (int k = 0; k < NDG; ++k) diag[k] = stored(L::up_plane(NUP - NDG + k), sl);
      }
    }
    double e_next = emis_at(t0 - lane);
    for (int t = t0; t < t1; ++t) {
      const double e_now = e_next;
      e_next = emis_at(t + 1 - lane);
      if (s > 0 && ((t & (HXBR_BLK - 1)) == 0 || t == t0) && t < Y) {
        // the strip above's last row, HXBR_BLK columns at a time
        const int c0 = t & ~(HXBR_BLK - 1);
        const int need = c0 + HXBR_BLK < Y ? c0 + HXBR_BLK : Y;
        lds_wait<2>(prog, s - 1, seen, need);
        const int c = c0 + lane;
        const bool take = lane < HXBR_BLK && c < Y;
        const int64_t sl = cell_slot(ss, (s << 6) - 1, take ? c : 0);
#pragma unroll
        for (int k = 0; k < NUP; ++k) bnd[k] = take ? stored(L::up_plane(k), sl) : ninf;
      }
      // lane 0's upper neighbour of this step is column t of the row above: lane t mod HXBR_BLK of the block
      if (s > 0) {
        const int src = t & (HXBR_BLK - 1);
        double b[NUP];
#pragma unroll
        for (int k = 0; k < NUP; ++k) b[k] = read_lane64(bnd[k], src);
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < NUP; ++k) up[k] = t < Y ? b[k] : ninf;
        }
      }
      const int j = t - lane;
      const bool jv = rvalid && j >= 0 && j < Y;
      const int jc = j < 0 ? 0 : (j < Y ? j : Y - 1);
      const int ye = J.max_dist < 0 ? 0 : (YL ? yenvL[jc] : J.y_env[jc]);
      const double yem = YL ? yemitL[jc] : (jc > 0 ? J.y_emit[jc - 1] : 0.0);
      const int dxy = xe - ye;
      const bool in = jv && (xedge || j == 0 || j == Y - 1 || J.max_dist < 0 || (dxy <= J.max_dist && -dxy <= J.max_dist));
      // The cell, straight-line: sources that do not exist (row / column -1, cells outside the envelope) are -inf in the
      // registers they come from, and -inf through the sums is what the reference's unassigned cell is; only the stores are
      // conditional.  Cell (0, 0) is the start: lpStart() = 0 in the lattice's start state, and what follows from it.
      double now[NS];
      lat.cell(now, up, diag, left, xem, yem, e_now, i == 0 && j == 0, tab);
      if (!in) {
#pragma unroll
        for (int k = 0; k < NS; ++k) now[k] = ninf;
      }
      // The cells of steps 2m and 2m + 1 of a row lie side by side in a plane: stored together, 16 bytes per lane and
      // plane, a wavefront's store is whole 64-byte lines (stored one by one, every line was written in two halves - two
      // read-modify-writes; a build without stores ran 45 % faster).  A cell of the pair that is outside the envelope is
      // written as the -inf the plane was cleared to; windows are whole step pairs (branch_windows).
      if (!(t & 1)) {
#pragma unroll
        for (int k = 0; k < NS; ++k) held[k] = now[k];
        held_in = in;
      } else if (rvalid && (in || held_in)) {
        HX_GLOBAL d2v* P2 = (HX_GLOBAL d2v*)(M + cell_slot(ss, i, j - 1));
        const int64_t plane2 = plane >> 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) P2[k * plane2] = d2v{held[k], now[k]};
      }
      // next step: the lane's own cell is its left source; the previous lane's cell of this step its upper, of the last its diagonal
#pragma unroll
      for (int k = 0; k < NDG; ++k) diag[k] = up[NUP - NDG + k];
#pragma unroll
      for (int k = 0; k < NS; ++k) left[k] = now[k];
#pragma unroll
      for (int k = 0; k < NUP; ++k) up[k] = wave_shr1(now[L::up_plane(k)]);
      if (lane == 0) {                              // (row 0 has no row above; strips below take it from the block)
#pragma unroll
        for (int k = 0; k < NUP; ++k) up[k] = ninf;
      }
      // the last row's columns 0 .. t - 63 are computed; say so once their stores have left the wavefront
      if (feeds && (t & 1)) {                       // (behind the store of a step pair)
        const int done = t - 63 + 1;                // columns of lane 63's row computed and stored so far (odd)
        if (done > 0 && ((done & (HXBR_BLK - 1)) == 1 || done >= Y)) {
          drain_stores();
          if (lane == 0) prog[s] = done < Y ? done : Y;
        }
      }
    }
    // behind a window: the last row is final up to where the next window takes it up
    {
      const int nt0 = (wn && wi + 1 < 3 && wn[2 * wi + 3] > wn[2 * wi + 2]) ? wn[2 * wi + 2] : Y + 63;
      drain_stores();
      int fin = nt0 - 63;
      fin = fin < 0 ? 0 : (fin > Y ? Y : fin);
      if (feeds && lane == 0 && fin > 0) prog[s] = fin;
    }
    }
    drain_stores();
    if (feeds && lane == 0) prog[s] = Y;
    if (s == n_strips - 1 && lane == 0) {
      const int64_t sl = cell_slot(ss, X - 1, Y - 1);
      *J.lp_end = L::lp_end(J, [&](const int state) { return stored(state, sl); }, tab);
    }
  }
}

// the skewed planes of one job -> dense [X][Y][NS]
template <class Job, int NS>
__global__ void k_pair_dense(const Job* __restrict__ jobs, const int job, double* __restrict__ out) {
  const Job& J = jobs[job];
  const int64_t n = (int64_t)J.X * J.Y;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sl = cell_slot(J.strip_stride, (int)(c / J.Y), (int)(c % J.Y));
    for (int s = 0; s < NS; ++s) out[NS * c + s] = J.cells[s * J.plane + sl];
  }
}

// ---- walks through a filled matrix ------------------------------------------------------------------------------------------
// Refiner::BranchMatrix::best (src/refiner.cpp:62-104), Sampler::BranchMatrix::sample (src/sampler.cpp:1088-1120) and
// Sampler::SiblingMatrix::sample (:1343-1386) are one loop: from (X - 1, Y - 1, End) back to cell (0, 0), a step takes the
// present cell's column (getColumn), steps to the source cell, and weighs that cell's states s by
// w[s] = (cell(s) + T[s][state]) + lpEmit(present cell) - lane s holds w[s], the states of a cell being NS planes at one slot -
// then picks the first maximal one (best) or draws one with random_key_log (src/util.h:220-236) from the next 32-bit word.
// Of a lattice L (header of this file) they use Job, NS, ND, END, column(), Emit and self_loop().
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

}  // namespace hx
