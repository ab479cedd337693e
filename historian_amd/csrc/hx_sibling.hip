// Sibling-pair parent-proposal DP: the eleven-state alignment of a left child profile and a
// right child profile under their unobserved parent, inside a GuideAlignmentEnvelope.
//
// Reference: Sampler::SiblingMatrix::SiblingMatrix (src/sampler.cpp:1185-1342; states and the 35 transition members
// src/sampler.h:226-325) over TreeAlignFuncs::SparseDPMatrix<11> (src/sampler.h:66-166).  The MCMC sampler fills two of
// these per node-resampling move and four per prune-and-regraft move, before any three-state branch matrix.
//
// The schedule is k_branch_fill's (hx_branch.hip): k_pair_emission evaluates logMatch for every in-envelope cell up front,
// k_sibling_fill gives a job one workgroup whose wavefronts take the 64-row strips round-robin, lane <-> row of the left
// child, step <-> anti-diagonal.  A cell reads nine states of the cell above (IMM, IMI, IIW, IMD, IIX, WWW, WWX, WXW, IDD:
// DPP wave_shr:1 of the previous lane's cell), four of the diagonal cell (WWW, WWX, WXW, IDD: what the lane received as
// "above" one step earlier - no second exchange) and eight of its own previous cell.  Sources that do not exist are -inf
// and the cell is straight-line; inside a cell the reference's order is kept (left block, right block, diagonal block, IDD
// last from the wait states of the same cell) because it fixes the bits of WWW and IDD.  Only the reference's table
// log_sum_exp, left-nested: cells and lpEnd are bit-identical to the restatement (tests/sibling_ref.py), which is pinned by
// enumeration, not by a reference fixture (no fixture holds a sibling matrix).
//
// Storage: eleven state planes per job, strip-skewed (hx_device.h cell_slot), -inf outside the envelope;
// hx_sibling_batch_read_matrix returns the dense [l_len + 1][r_len + 1][11] array.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include "hx_device.h"
#include "hx_lse.h"
#include "hx_common.h"
#include "hx_policy.h"
#include "hx_kernels.h"
#include "hx_pairdp.h"
#include "../../include/historian_hip.h"

namespace hx {

int api_fail(int code, const char* what);                  // hx_api.hip: sets hx_last_error()
const double* device_lse_table(int device);               // hx_api.hip: the table hx_init uploaded, or nullptr

namespace {

// SiblingMatrix::State (src/sampler.h:227-234)
enum { IMM = 0, IMD = 1, IDM = 2, IDD = 3, WWW = 4, WWX = 5, WXW = 6, IMI = 7, IIW = 8, IDI = 9, IIX = 10, EEE = 11, NS = 11 };

struct DevSibling {
  int32_t X, Y;                 // positions 0 .. l_len (rows), 0 .. r_len (columns)
  int32_t CA, C;
  int32_t max_dist;             // < 0: no band
  const double* x_pwm;          // [l_len][CA] logRoot + lSub: the left two factors of logMatch, added on the host
  const double* y_sub;          // [r_len][CA] rSub
  const double* x_emit;         // [l_len] lEmit
  const double* y_emit;         // [r_len] rEmit
  const int32_t* x_env;         // [X] or nullptr
  const int32_t* y_env;         // [Y]
  double T[NS][12];             // lpTransElimSelfLoopIDD(source, destination); -inf where the reference has no member
  double* cells;                // [11][plane]
  double* emis;                 // [plane]: logMatch in the matrix layout
  int64_t plane, strip_stride;
  double* lp_end;
  const int32_t* win;           // banded: [n_strips][3][2] step windows of the strips (branch_windows), or nullptr
};

// a banded job's planes are -inf wherever the fill does not write; an unbanded job's fill writes every cell
__global__ void k_sibling_clear(const DevSibling* __restrict__ jobs) {
  const DevSibling& J = jobs[blockIdx.x];
  if (J.max_dist < 0) return;
  const int64_t n = NS * J.plane;
  for (int64_t c = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.y * blockDim.x) J.cells[c] = HX_NEG_INF;
}

typedef double d2v __attribute__((ext_vector_type(2)));
struct S11 { double v[NS]; };
struct Up9 { double imm, imi, iiw, imd, iix, www, wwx, wxw, idd; };     // what a cell reads of the cell above
struct Dg4 { double www, wwx, wxw, idd; };                               // ... of the diagonal cell
struct Lf8 { double imm, imi, idm, idi, www, wwx, wxw, idd; };           // ... of the cell to its left

#define HXSB_MAX_WAVES 16

// One workgroup per job, strips dealt to its wavefronts round-robin, the strip hand-off of hx_pairdp.h; see k_branch_fill
// for the schedule.  YL: the right child's side of a step (rEmit and envelope coordinate of its column) out of LDS.
template <bool YL>
__global__ void __launch_bounds__(64 * HXSB_MAX_WAVES) k_sibling_fill(const DevSibling* __restrict__ jobs, const double* __restrict__ tab,
                                                                      const int y_cap) {
  __shared__ int progress[HXBR_MAX_STRIPS];         // columns of the strip's last row that are stored
  extern __shared__ __attribute__((aligned(16))) unsigned char ydyn[];
  double* yemitL = reinterpret_cast<double*>(ydyn);                 // [y_cap]
  int* yenvL = reinterpret_cast<int*>(ydyn + 8 * (size_t)y_cap);    // [y_cap]
  const DevSibling& J = jobs[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
  const int X = J.X, Y = J.Y;
  const int64_t plane = J.plane, ss = J.strip_stride;
  HX_GLOBAL double* __restrict__ M = as_global(J.cells);
  const HX_GLOBAL double* __restrict__ E = as_global((const double*)J.emis);
  // the 31 scores a cell uses (the four into EEE are read once, at the end)
  const double imm_www = J.T[IMM][WWW], imm_imi = J.T[IMM][IMI], imm_iiw = J.T[IMM][IIW];
  const double imd_wwx = J.T[IMD][WWX], imd_iix = J.T[IMD][IIX], idm_wxw = J.T[IDM][WXW], idm_idi = J.T[IDM][IDI];
  const double idd_imm = J.T[IDD][IMM], idd_imd = J.T[IDD][IMD], idd_idm = J.T[IDD][IDM];
  const double www_imm = J.T[WWW][IMM], www_imd = J.T[WWW][IMD], www_idm = J.T[WWW][IDM], www_idd = J.T[WWW][IDD];
  const double wwx_imm = J.T[WWX][IMM], wwx_imd = J.T[WWX][IMD], wwx_idm = J.T[WWX][IDM], wwx_idd = J.T[WWX][IDD];
  const double wxw_imm = J.T[WXW][IMM], wxw_imd = J.T[WXW][IMD], wxw_idm = J.T[WXW][IDM], wxw_idd = J.T[WXW][IDD];
  const double imi_www = J.T[IMI][WWW], imi_imi = J.T[IMI][IMI], imi_iiw = J.T[IMI][IIW];
  const double iiw_www = J.T[IIW][WWW], iiw_iiw = J.T[IIW][IIW], idi_wxw = J.T[IDI][WXW], idi_idi = J.T[IDI][IDI];
  const double iix_wwx = J.T[IIX][WWX], iix_iix = J.T[IIX][IIX];
  const int n_strips = (X + 63) >> 6;
  for (int q = threadIdx.x; q < n_strips && q < HXBR_MAX_STRIPS; q += blockDim.x) progress[q] = 0;
  if (YL)
    for (int j = threadIdx.x; j < Y; j += blockDim.x) {
      yemitL[j] = j > 0 ? J.y_emit[j - 1] : 0.0;    // (the score of entering column j: rEmit of position j - 1)
      yenvL[j] = J.max_dist >= 0 ? J.y_env[j] : 0;
    }
  __syncthreads();
  volatile int* prog = progress;
  const double ninf = HX_NEG_INF;
  const Up9 no_up{ninf, ninf, ninf, ninf, ninf, ninf, ninf, ninf, ninf};
  const Dg4 no_dg{ninf, ninf, ninf, ninf};
  const Lf8 no_lf{ninf, ninf, ninf, ninf, ninf, ninf, ninf, ninf};
  S11 none;
#pragma unroll
  for (int k = 0; k < NS; ++k) none.v[k] = ninf;
  // the planes a cell reads of the cell above, in Up9's order
  const int up_plane[9] = {IMM, IMI, IIW, IMD, IIX, WWW, WWX, WXW, IDD};
  for (int s = wave; s < n_strips; s += n_waves) {
    const int i = (s << 6) + lane;
    const bool rvalid = i < X;
    const int xe = (rvalid && J.max_dist >= 0) ? J.x_env[i] : 0;
    const double xem = (rvalid && i > 0) ? J.x_emit[i - 1] : 0.0;      // lEmit of the lane's row
    const bool xedge = i == 0 || i == X - 1;
    const bool feeds = s + 1 < n_strips;            // a strip below reads this strip's last row
    Lf8 left = no_lf;                               // (i, j-1)
    Up9 up = no_up;                                 // (i-1, j)
    Dg4 diag = no_dg;                               // (i-1, j-1)
    double bnd[9];                                  // lane l < HXBR_BLK: cell (row above the strip, column c0 + l), Up9's order
#pragma unroll
    for (int k = 0; k < 9; ++k) bnd[k] = ninf;
    S11 held = none;                                // the lane's cell of the even step of the current step pair
    bool held_in = false;
    int seen = 0;
    // logMatch of the lane's cell of the NEXT step (column t + 1 - lane), fetched a step ahead
    auto emis_at = [&](const int jj) -> double {
      return (rvalid && i > 0 && jj > 0 && jj < Y) ? E[cell_slot(ss, i, jj)] : 0.0;
    };
    // a banded strip sweeps its step windows only; between them nothing of the strip is inside the envelope, so a window
    // starts from -inf registers, and the strip below is told that the columns up to the next window are final
    const int32_t* wn = J.win ? J.win + 6 * s : nullptr;
    for (int wi = 0; wi < (wn ? 3 : 1); ++wi) {
    const int t0 = wn ? wn[2 * wi] : 0, t1 = wn ? wn[2 * wi + 1] : (Y + 63 + 1) & ~1;      // (whole step pairs)
    if (t1 <= t0) break;
    left = no_lf; up = no_up; diag = no_dg;
    if (s > 0 && t0 >= 1 && t0 - 1 < Y) {
      // ... except lane 0's diagonal source of the window's first step: cell (row above, column t0 - 1) belongs to the strip
      // above, whose band may well hold it
      strip_wait(prog, s - 1, seen, t0);
      if (lane == 0) {
        const int64_t sl = cell_slot(ss, (s << 6) - 1, t0 - 1);
        diag.www = __hip_atomic_load(M + WWW * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        diag.wwx = __hip_atomic_load(M + WWX * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        diag.wxw = __hip_atomic_load(M + WXW * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        diag.idd = __hip_atomic_load(M + IDD * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
        strip_wait(prog, s - 1, seen, need);
        const int c = c0 + lane;
        const bool take = lane < HXBR_BLK && c < Y;
        const int64_t sl = cell_slot(ss, (s << 6) - 1, take ? c : 0);
#pragma unroll
        for (int k = 0; k < 9; ++k)
          bnd[k] = take ? __hip_atomic_load(M + up_plane[k] * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ninf;
      }
      // lane 0's upper neighbour of this step is column t of the row above: lane t mod HXBR_BLK of the block
      if (s > 0) {
        const int src = t & (HXBR_BLK - 1);
        double b[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) b[k] = read_lane64(bnd[k], src);
        if (lane == 0) up = t < Y ? Up9{b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8]} : no_up;
      }
      const int j = t - lane;
      const bool jv = rvalid && j >= 0 && j < Y;
      const int jc = j < 0 ? 0 : (j < Y ? j : Y - 1);
      const int ye = J.max_dist < 0 ? 0 : (YL ? yenvL[jc] : J.y_env[jc]);
      const double yem = YL ? yemitL[jc] : (jc > 0 ? J.y_emit[jc - 1] : 0.0);
      const int dxy = xe - ye;
      const bool in = jv && (xedge || j == 0 || j == Y - 1 || J.max_dist < 0 || (dxy <= J.max_dist && -dxy <= J.max_dist));
      // The cell, straight-line (src/sampler.cpp:1263-1324): a source that does not exist (row / column -1, a cell outside the
      // envelope) is -inf in the registers it comes from, and a block over -inf sources leaves what the reference's skipped
      // block leaves - lse(-inf, -inf) = -inf and lse(a, -inf) = a (hx_lse.h); only the stores are conditional.
      S11 now;
      // left child advances: source (i - 1, j)
      now.v[IIW] = xem + lse(lse(up.imm + imm_iiw, up.imi + imi_iiw, tab), up.iiw + iiw_iiw, tab);
      now.v[IIX] = xem + lse(up.imd + imd_iix, up.iix + iix_iix, tab);
      now.v[IMD] = xem + lse(lse(lse(up.www + www_imd, up.wwx + wwx_imd, tab), up.wxw + wxw_imd, tab), up.idd + idd_imd, tab);
      double www = now.v[IIW] + iiw_www;
      now.v[WWX] = lse(now.v[IIX] + iix_wwx, now.v[IMD] + imd_wwx, tab);
      // right child advances: source (i, j - 1)
      now.v[IMI] = yem + lse(left.imm + imm_imi, left.imi + imi_imi, tab);
      now.v[IDI] = yem + lse(left.idm + idm_idi, left.idi + idi_idi, tab);
      now.v[IDM] = yem + lse(lse(lse(left.www + www_idm, left.wwx + wwx_idm, tab), left.wxw + wxw_idm, tab), left.idd + idd_idm, tab);
      www = lse(www, now.v[IMI] + imi_www, tab);
      now.v[WXW] = lse(now.v[IDI] + idi_wxw, now.v[IDM] + idm_wxw, tab);
      // both advance: source (i - 1, j - 1)
      now.v[IMM] = e_now + lse(lse(lse(diag.www + www_imm, diag.wwx + wwx_imm, tab), diag.wxw + wxw_imm, tab), diag.idd + idd_imm, tab);
      if (i == 0 && j == 0) now.v[IMM] = 0.0;       // lpStart() = 0; WWW(0, 0) = imm_www follows
      www = lse(www, now.v[IMM] + imm_www, tab);
      now.v[WWW] = www;
      // the parent column neither child sees, from the wait states of this cell
      now.v[IDD] = lse(lse(www + www_idd, now.v[WWX] + wwx_idd, tab), now.v[WXW] + wxw_idd, tab);
      if (!in) now = none;
      // The cells of steps 2m and 2m + 1 of a row lie side by side in a plane: stored together, 16 bytes per lane and plane
      // (whole 64-byte lines per wavefront).  A cell of the pair outside the envelope is written as -inf.
      if (!(t & 1)) { held = now; held_in = in; }
      else if (rvalid && (in || held_in)) {
        HX_GLOBAL d2v* P2 = (HX_GLOBAL d2v*)(M + cell_slot(ss, i, j - 1));
        const int64_t plane2 = plane >> 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) P2[k * plane2] = d2v{held.v[k], now.v[k]};
      }
      // next step: the lane's own cell is its left source; the previous lane's cell of this step its upper, of the last its diagonal
      diag = Dg4{up.www, up.wwx, up.wxw, up.idd};
      left = Lf8{now.v[IMM], now.v[IMI], now.v[IDM], now.v[IDI], now.v[WWW], now.v[WWX], now.v[WXW], now.v[IDD]};
      up = Up9{wave_shr1(now.v[IMM]), wave_shr1(now.v[IMI]), wave_shr1(now.v[IIW]), wave_shr1(now.v[IMD]), wave_shr1(now.v[IIX]),
               wave_shr1(now.v[WWW]), wave_shr1(now.v[WWX]), wave_shr1(now.v[WXW]), wave_shr1(now.v[IDD])};
      if (lane == 0) up = no_up;                    // (row 0 has no row above; strips below take it from the block)
      // the last row's columns 0 .. t - 63 are computed; say so once their stores have left the wavefront
      if (feeds && (t & 1)) {                       // (behind the store of a step pair)
        const int done = t - 63 + 1;                // columns of lane 63's row computed and stored so far (odd)
        if (done > 0 && ((done & (HXBR_BLK - 1)) == 1 || done >= Y)) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) prog[s] = done < Y ? done : Y;
        }
      }
    }
    // behind a window: the last row is final up to where the next window takes it up
    {
      const int nt0 = (wn && wi + 1 < 3 && wn[2 * wi + 3] > wn[2 * wi + 2]) ? wn[2 * wi + 2] : Y + 63;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int fin = nt0 - 63;
      fin = fin < 0 ? 0 : (fin > Y ? Y : fin);
      if (feeds && lane == 0 && fin > 0) prog[s] = fin;
    }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (feeds && lane == 0) prog[s] = Y;
    if (s == n_strips - 1 && lane == 0) {
      // lpEnd (src/sampler.cpp:1330-1333)
      const int64_t sl = cell_slot(ss, X - 1, Y - 1);
      const double ed = __hip_atomic_load(M + IDD * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double e0 = __hip_atomic_load(M + WWW * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double e1 = __hip_atomic_load(M + WWX * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double e2 = __hip_atomic_load(M + WXW * plane + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *J.lp_end = lse(lse(lse(ed + J.T[IDD][EEE], e0 + J.T[WWW][EEE], tab), e1 + J.T[WWX][EEE], tab), e2 + J.T[WXW][EEE], tab);
    }
  }
}

// the skewed planes of one job -> dense [X][Y][11]
__global__ void k_sibling_dense(const DevSibling* __restrict__ jobs, const int job, double* __restrict__ out) {
  const DevSibling& J = jobs[job];
  const int64_t n = (int64_t)J.X * J.Y;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sl = cell_slot(J.strip_stride, (int)(c / J.Y), (int)(c % J.Y));
    for (int s = 0; s < NS; ++s) out[NS * c + s] = J.cells[s * J.plane + sl];
  }
}

// the eleven-state lattice as the walks of hx_pairdp.h see it (SiblingMatrix::getColumn / lpEmit, src/sampler.cpp:1414-1449)
struct SiblingLattice {
  typedef DevSibling Job;
  enum { NS = 11, ND = 12, END = EEE };
  static __device__ __forceinline__ void column(const int i, const int j, const int state, bool& l, bool& r) {
    l = (state == IMM && i > 0 && j > 0) || state == IMD || ((state == IIW || state == IIX) && i > 0);
    r = (state == IMM && i > 0 && j > 0) || state == IDM || ((state == IMI || state == IDI) && j > 0);
  }
  // lpEmit: where the term lies (p, left alone when it lies nowhere) and its value when it lies nowhere
  struct Emit {
    const double *emis, *x_emit, *y_emit;
    int64_t ss;
    __device__ __forceinline__ explicit Emit(const DevSibling& J) : emis(J.emis), x_emit(J.x_emit), y_emit(J.y_emit), ss(J.strip_stride) {}
    __device__ __forceinline__ double from(const int i, const int j, const int state, const double*& p) const {
      const bool right = state == IDM || state == IMI || state == IDI, left = state == IMD || state == IIW || state == IIX;
      if (state == IMM && i > 0 && j > 0) p = emis + cell_slot(ss, i, j);
      if (right && j > 0) p = y_emit + (j - 1);
      if (left && i > 0) p = x_emit + (i - 1);
      return (state == IMM || right || left) ? HX_NEG_INF : 0.0;
    }
  };
  static __device__ __forceinline__ bool self_loop(const int state) { return state == IDD; }
};

}  // namespace
}  // namespace hx

using namespace hx;

struct hx_sibling_batch {
  int device = 0, n_jobs = 0;
  std::vector<DevSibling> jobs;
  DevSibling* d_jobs = nullptr;
  char* d_arena = nullptr;          // inputs + lpEnd
  double* d_cells = nullptr;        // matrices + emission planes
  size_t lp_off = 0;
  int max_x = 0, max_y = 0;         // rows / columns of the longest job
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};       // before the step, before the fill, after it
  hipStream_t last_stream = nullptr;
  bool done = false;
  float walk_ms = -1.f;             // the walk kernel of the last best_paths / sample_paths (HIP events)
};

extern "C" {

int hx_sibling_batch_destroy(hx_sibling_batch* b) {
  if (!b) return HX_OK;
  (void)hipSetDevice(b->device);
  (void)hipDeviceSynchronize();
  for (int e = 0; e < 3; ++e)
    if (b->ev[e]) (void)hipEventDestroy(b->ev[e]);
  if (b->d_jobs) (void)hipFree(b->d_jobs);
  if (b->d_arena) (void)hipFree(b->d_arena);
  if (b->d_cells) (void)hipFree(b->d_cells);
  delete b;
  return HX_OK;
}

int hx_sibling_batch_create(const hx_sibling_job* jobs, int32_t n_jobs, hx_sibling_batch** out) {
  if (out) *out = nullptr;
  if (!jobs || !out || n_jobs < 1) return api_fail(HX_ERR_INVALID_ARG, "hx_sibling_batch_create: need at least one job");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return api_fail(HX_ERR_NO_DEVICE, "no HIP device");
  if (!device_lse_table(device)) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the current device");
  hx_sibling_batch* b = new (std::nothrow) hx_sibling_batch;
  if (!b) return api_fail(HX_ERR_OUT_OF_MEMORY, "host allocation failed");
  b->device = device;
  b->n_jobs = n_jobs;
  std::vector<char> host;
  auto put = [&](const void* p, size_t bytes) -> size_t {
    const size_t off = (host.size() + 15) & ~(size_t)15;
    host.resize(off + bytes);
    if (bytes) memcpy(host.data() + off, p, bytes);
    return off;
  };
  struct Off { size_t x, y, xm, ym, xe, ye, win; bool env; };
  std::vector<Off> offs(n_jobs);
  int64_t cells_total = 0;
  try {
    b->jobs.resize(n_jobs);
    std::vector<double> rooted;
    for (int k = 0; k < n_jobs; ++k) {
      const hx_sibling_job& j = jobs[k];
      if (j.l_len >= 64 * HXBR_MAX_STRIPS) {
        hx_sibling_batch_destroy(b);
        return api_fail(HX_ERR_RANGE, "hx_sibling_batch_create: a left child profile of more than 65535 positions");
      }
      if (j.l_len < 0 || j.r_len < 0 || j.components < 1 || j.alphabet < 1 || (j.l_len && (!j.l_sub || !j.l_emit || !j.log_root)) ||
          (j.r_len && (!j.r_sub || !j.r_emit)) || (j.max_distance >= 0 && (!j.l_env || !j.r_env))) {
        hx_sibling_batch_destroy(b);
        return api_fail(HX_ERR_INVALID_ARG, "hx_sibling_batch_create: inconsistent job (lengths, components, missing arrays)");
      }
      DevSibling& J = b->jobs[k];
      memset(&J, 0, sizeof(J));
      J.X = j.l_len + 1; J.Y = j.r_len + 1;
      J.CA = j.components * j.alphabet;
      J.C = j.components;
      J.max_dist = j.max_distance;
      for (int s = 0; s < NS; ++s)
        for (int d = 0; d < 12; ++d) J.T[s][d] = j.trans[s][d];
      J.strip_stride = strip_stride_for(J.Y);
      J.plane = (int64_t)((J.X + HX_STRIP - 1) / HX_STRIP) * J.strip_stride;
      // logInnerProduct's three-vector term is (logRoot + lSub) + rSub (src/logsumexp.h:139-144): the first sum here
      rooted.resize((size_t)j.l_len * J.CA);
      for (size_t p = 0; p < (size_t)j.l_len; ++p)
        for (int q = 0; q < J.CA; ++q) rooted[p * J.CA + q] = j.log_root[q] + j.l_sub[p * J.CA + q];
      offs[k].x = put(rooted.data(), sizeof(double) * rooted.size());
      offs[k].y = put(j.r_sub, sizeof(double) * (size_t)j.r_len * J.CA);
      offs[k].xm = put(j.l_emit, sizeof(double) * (size_t)j.l_len);
      offs[k].ym = put(j.r_emit, sizeof(double) * (size_t)j.r_len);
      offs[k].env = j.max_distance >= 0;
      offs[k].xe = offs[k].env ? put(j.l_env, sizeof(int32_t) * (size_t)J.X) : 0;
      offs[k].ye = offs[k].env ? put(j.r_env, sizeof(int32_t) * (size_t)J.Y) : 0;
      offs[k].win = 0;
      if (offs[k].env) {
        const std::vector<int32_t> w = branch_windows(j.l_env, j.r_env, J.X, J.Y, j.max_distance);
        offs[k].win = put(w.data(), sizeof(int32_t) * w.size()) + 1;      // (+1: 0 means none)
      }
      cells_total += (NS + 1) * J.plane;
      if (J.X > b->max_x) b->max_x = J.X;
      if (J.Y > b->max_y) b->max_y = J.Y;
    }
    b->lp_off = put(nullptr, 0);
    host.resize(b->lp_off + sizeof(double) * n_jobs);
  } catch (const std::bad_alloc&) {
    hx_sibling_batch_destroy(b);
    return api_fail(HX_ERR_OUT_OF_MEMORY, "host allocation failed while building the batch");
  }
  if (hipMalloc(reinterpret_cast<void**>(&b->d_arena), host.size()) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&b->d_cells), sizeof(double) * (size_t)cells_total) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&b->d_jobs), sizeof(DevSibling) * n_jobs) != hipSuccess) {
    hx_sibling_batch_destroy(b);
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_sibling_batch_create: device allocation failed");
  }
  int64_t at = 0;
  for (int k = 0; k < n_jobs; ++k) {
    DevSibling& J = b->jobs[k];
    J.x_pwm = reinterpret_cast<const double*>(b->d_arena + offs[k].x);
    J.y_sub = reinterpret_cast<const double*>(b->d_arena + offs[k].y);
    J.x_emit = reinterpret_cast<const double*>(b->d_arena + offs[k].xm);
    J.y_emit = reinterpret_cast<const double*>(b->d_arena + offs[k].ym);
    J.x_env = offs[k].env ? reinterpret_cast<const int32_t*>(b->d_arena + offs[k].xe) : nullptr;
    J.y_env = offs[k].env ? reinterpret_cast<const int32_t*>(b->d_arena + offs[k].ye) : nullptr;
    J.win = offs[k].win ? reinterpret_cast<const int32_t*>(b->d_arena + (offs[k].win - 1)) : nullptr;
    J.cells = b->d_cells + at;
    J.emis = b->d_cells + at + NS * J.plane;
    at += (NS + 1) * J.plane;
    J.lp_end = reinterpret_cast<double*>(b->d_arena + b->lp_off) + k;
  }
  if (hipMemcpy(b->d_arena, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(b->d_jobs, b->jobs.data(), sizeof(DevSibling) * n_jobs, hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreate(&b->ev[0]) != hipSuccess || hipEventCreate(&b->ev[1]) != hipSuccess || hipEventCreate(&b->ev[2]) != hipSuccess) {
    hx_sibling_batch_destroy(b);
    return api_fail(HX_ERR_HIP, "hx_sibling_batch_create: copy to the device failed");
  }
  *out = b;
  return HX_OK;
}

int hx_sibling_batch_run(hx_sibling_batch* b, void* stream) {
  if (!b) return api_fail(HX_ERR_INVALID_ARG, "batch is null");
  if (hipSetDevice(b->device) != hipSuccess) return api_fail(HX_ERR_HIP, "hipSetDevice failed");
  const double* tab = device_lse_table(b->device);
  if (!tab) return api_fail(HX_ERR_NOT_INITIALIZED, "hx_init has not been called for the batch's device");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipEventRecord(b->ev[0], st) != hipSuccess) return api_fail(HX_ERR_HIP, "hipEventRecord failed");
  for (int j0 = 0; j0 < b->n_jobs; j0 += 16384) {        // (grid.x of at most 16384 jobs per launch)
    const int n = b->n_jobs - j0 < 16384 ? b->n_jobs - j0 : 16384;
    hipLaunchKernelGGL(k_sibling_clear, dim3(n, 16), dim3(256), 0, st, b->d_jobs + j0);
    hipLaunchKernelGGL(k_pair_emission<DevSibling>, dim3(n, 16), dim3(256), 0, st, b->d_jobs + j0, tab);
  }
  if (hipEventRecord(b->ev[1], st) != hipSuccess) return api_fail(HX_ERR_HIP, "hipEventRecord failed");
  for (int j0 = 0; j0 < b->n_jobs; j0 += 65536) {
    const int n = b->n_jobs - j0 < 65536 ? b->n_jobs - j0 : 65536;
    // wavefronts per job: as many as the longest job has strips, at most HXSB_MAX_WAVES - fewer when the batch alone fills
    // the chip (120 VGPRs: four wavefronts per SIMD, 4096 on the chip)
    int waves = (b->max_x + 63) / 64;
    waves = waves < 1 ? 1 : (waves > HXSB_MAX_WAVES ? HXSB_MAX_WAVES : waves);
    if (const char* e = getenv("HX_SIBLING_WAVES")) { const int v = atoi(e); if (v >= 1 && v <= HXSB_MAX_WAVES) waves = v; }
    else while (waves > 1 && (int64_t)n * waves > 2048 * 2) waves = (waves + 1) / 2;
    // the right child's side in LDS when the longest one fits (12 bytes per position beside the progress counters)
    const bool yl = (size_t)b->max_y * 12 <= 96 * 1024;
    const size_t dyn = yl ? (size_t)b->max_y * 12 + 16 : 0;
    const int y_cap = yl ? (b->max_y + 1) & ~1 : 0;
    if (yl) hipLaunchKernelGGL((k_sibling_fill<true>), dim3(n), dim3(64 * waves), dyn, st, b->d_jobs + j0, tab, y_cap);
    else hipLaunchKernelGGL((k_sibling_fill<false>), dim3(n), dim3(64 * waves), 0, st, b->d_jobs + j0, tab, 0);
  }
  if (hipEventRecord(b->ev[2], st) != hipSuccess || hipGetLastError() != hipSuccess) return api_fail(HX_ERR_HIP, "hx_sibling_batch_run: launch failed");
  b->done = true;
  b->last_stream = st;
  return HX_OK;
}

int hx_sibling_batch_results(hx_sibling_batch* b, double* lp_end) {
  if (!b || !lp_end) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
  if (!b->done) return api_fail(HX_ERR_STATE, "hx_sibling_batch_run has not been launched");
  if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess ||
      hipMemcpy(lp_end, b->d_arena + b->lp_off, sizeof(double) * b->n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return api_fail(HX_ERR_HIP, "hx_sibling_batch_results: HIP call failed");
  return HX_OK;
}

int hx_sibling_batch_read_matrix(hx_sibling_batch* b, int32_t job, double* out) {
  if (!b || !out) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
  if (job < 0 || job >= b->n_jobs) return api_fail(HX_ERR_RANGE, "job out of range");
  if (!b->done) return api_fail(HX_ERR_STATE, "hx_sibling_batch_run has not been launched");
  const DevSibling& J = b->jobs[job];
  const size_t bytes = sizeof(double) * NS * (size_t)J.X * J.Y;
  double* dense = nullptr;
  if (hipSetDevice(b->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dense), bytes) != hipSuccess)
    return api_fail(HX_ERR_OUT_OF_MEMORY, "hx_sibling_batch_read_matrix: device allocation failed");
  hipLaunchKernelGGL(k_sibling_dense, dim3(256), dim3(256), 0, b->last_stream, b->d_jobs, job, dense);
  const bool ok = hipStreamSynchronize(b->last_stream) == hipSuccess && hipMemcpy(out, dense, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(dense);
  return ok ? HX_OK : api_fail(HX_ERR_HIP, "hx_sibling_batch_read_matrix: HIP call failed");
}

int64_t hx_sibling_batch_total_cells(const hx_sibling_batch* b) {
  if (!b) return 0;
  int64_t n = 0;
  for (const DevSibling& J : b->jobs) n += (int64_t)J.X * J.Y;
  return n;
}

int hx_sibling_batch_last_kernel_ms(hx_sibling_batch* b, float* fill_ms, float* step_ms) {
  if (!b || !fill_ms) return api_fail(HX_ERR_INVALID_ARG, "bad arguments");
  if (!b->done) return api_fail(HX_ERR_STATE, "hx_sibling_batch_run has not been launched");
  if (hipSetDevice(b->device) != hipSuccess || hipEventSynchronize(b->ev[2]) != hipSuccess ||
      hipEventElapsedTime(fill_ms, b->ev[1], b->ev[2]) != hipSuccess ||
      (step_ms && hipEventElapsedTime(step_ms, b->ev[0], b->ev[2]) != hipSuccess))
    return api_fail(HX_ERR_HIP, "hx_sibling_batch_last_kernel_ms: HIP call failed");
  return HX_OK;
}

int hx_sibling_batch_sample_paths(hx_sibling_batch* b, const uint32_t* words, const int64_t* word_off, uint8_t* states, int64_t cap,
                                  int32_t* n_steps, int32_t* words_used) {
  return pair_walk_paths<SiblingLattice, false>(b, words, word_off, states, cap, n_steps, words_used);
}

int64_t hx_sibling_batch_max_steps(const hx_sibling_batch* b) {
  int64_t most = 0;
  if (b)
    for (const DevSibling& J : b->jobs) most = std::max<int64_t>(most, 3 * ((int64_t)(J.X - 1) + (J.Y - 1)) + 3);      // (wait states and IDD stay: header)
  return most;
}

int hx_sibling_batch_read_cells(hx_sibling_batch* b, int32_t job, int64_t n, const hx_pair_cell* at, double* cells, double* log_match) {
  return pair_read_cells<NS>(b, job, n, at, cells, log_match);
}

int hx_sibling_batch_last_walk_ms(hx_sibling_batch* b, float* ms) { return pair_last_walk_ms(b, ms); }

}  // extern "C"
