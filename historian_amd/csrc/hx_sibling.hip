// Sibling-pair parent-proposal DP: the eleven-state alignment of a left child profile and a
// right child profile under their unobserved parent, inside a GuideAlignmentEnvelope.
//
// Reference: Sampler::SiblingMatrix::SiblingMatrix (src/sampler.cpp:1185-1342; states and the 35 transition members
// src/sampler.h:226-325) over TreeAlignFuncs::SparseDPMatrix<11> (src/sampler.h:66-166).  The MCMC sampler fills two of
// these per node-resampling move and four per prune-and-regraft move, before any three-state branch matrix.
//
// The kernels are hx_pairdp.h's (k_pair_emission, then k_pair_fill: lane <-> row of the left child, step <-> anti-diagonal);
// this file has the lattice (SiblingCell) and the job.  A cell reads nine states of the cell above (IMM, IMI, IIW, IMD, IIX,
// WWW, WWX, WXW, IDD), four of the diagonal cell (WWW, WWX, WXW, IDD) and eight of its own previous cell.  Sources that do not
// exist are -inf and the cell is straight-line; inside a cell the reference's order is kept (left block, right block, diagonal
// block, IDD last from the wait states of the same cell) because it fixes the bits of WWW and IDD.  Only the reference's table
// log_sum_exp, left-nested: cells and lpEnd are bit-identical to the restatement (tests/sibling_ref.py), which is pinned by
// enumeration, not by a reference fixture (no fixture holds a sibling matrix).
//
// Storage: eleven state planes per job, strip-skewed (hx_device.h cell_slot), -inf outside the envelope;
// hx_sibling_batch_read_matrix returns the dense [l_len + 1][r_len + 1][11] array.
#include <hip/hip_runtime.h>
#include "hx_pairbatch.h"

namespace hx {
namespace {

// SiblingMatrix::State (src/sampler.h:227-234)
enum { IMM = 0, IMD = 1, IDM = 2, IDD = 3, WWW = 4, WWX = 5, WXW = 6, IMI = 7, IIW = 8, IDI = 9, IIX = 10, EEE = 11, NS = 11 };

struct DevSibling {
  static constexpr const char* abi = "hx_sibling_batch";
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

// The eleven-state lattice as the sweep and the walks of hx_pairdp.h see it (the fill: src/sampler.cpp:1263-1333;
// SiblingMatrix::getColumn / lpEmit: src/sampler.cpp:1414-1449)
struct SiblingCell {
  typedef DevSibling Job;
  enum { NS = 11, ND = 12, END = EEE, NUP = 9, NDG = 4 };
  // what a cell reads of the cell above; the last four also of the diagonal cell
  enum { U_IMM, U_IMI, U_IIW, U_IMD, U_IIX, U_WWW, U_WWX, U_WXW, U_IDD };
  enum { D_WWW, D_WWX, D_WXW, D_IDD };
  static __device__ __forceinline__ constexpr int up_plane(const int k) {
    constexpr int p[NUP] = {IMM, IMI, IIW, IMD, IIX, WWW, WWX, WXW, IDD};
    return p[k];
  }
  // wavefronts of a launch above which a job gets fewer than one per strip (120 VGPRs: four wavefronts per SIMD, 4096 on
  // the chip)
  static constexpr int64_t BATCH_WAVES = 2048 * 2;
  static constexpr const char* WAVES_ENV = "HX_SIBLING_WAVES";

  // the 31 scores a cell uses (the four into EEE are read once, at the end)
  double imm_www, imm_imi, imm_iiw, imd_wwx, imd_iix, idm_wxw, idm_idi, idd_imm, idd_imd, idd_idm;
  double www_imm, www_imd, www_idm, www_idd, wwx_imm, wwx_imd, wwx_idm, wwx_idd, wxw_imm, wxw_imd, wxw_idm, wxw_idd;
  double imi_www, imi_imi, imi_iiw, iiw_www, iiw_iiw, idi_wxw, idi_idi, iix_wwx, iix_iix;
  __device__ __forceinline__ explicit SiblingCell(const DevSibling& J)
      : imm_www(J.T[IMM][WWW]), imm_imi(J.T[IMM][IMI]), imm_iiw(J.T[IMM][IIW]), imd_wwx(J.T[IMD][WWX]), imd_iix(J.T[IMD][IIX]),
        idm_wxw(J.T[IDM][WXW]), idm_idi(J.T[IDM][IDI]), idd_imm(J.T[IDD][IMM]), idd_imd(J.T[IDD][IMD]), idd_idm(J.T[IDD][IDM]),
        www_imm(J.T[WWW][IMM]), www_imd(J.T[WWW][IMD]), www_idm(J.T[WWW][IDM]), www_idd(J.T[WWW][IDD]), wwx_imm(J.T[WWX][IMM]),
        wwx_imd(J.T[WWX][IMD]), wwx_idm(J.T[WWX][IDM]), wwx_idd(J.T[WWX][IDD]), wxw_imm(J.T[WXW][IMM]), wxw_imd(J.T[WXW][IMD]),
        wxw_idm(J.T[WXW][IDM]), wxw_idd(J.T[WXW][IDD]), imi_www(J.T[IMI][WWW]), imi_imi(J.T[IMI][IMI]), imi_iiw(J.T[IMI][IIW]),
        iiw_www(J.T[IIW][WWW]), iiw_iiw(J.T[IIW][IIW]), idi_wxw(J.T[IDI][WXW]), idi_idi(J.T[IDI][IDI]), iix_wwx(J.T[IIX][WWX]),
        iix_iix(J.T[IIX][IIX]) {}
  static __device__ __forceinline__ double x_emit(const DevSibling& J, const int i) { return J.x_emit[i - 1]; }      // lEmit of row i
  // The cell (src/sampler.cpp:1263-1324): a block over -inf sources leaves what the reference's skipped block leaves -
  // lse(-inf, -inf) = -inf and lse(a, -inf) = a (hx_lse.h).
  __device__ __forceinline__ void cell(double (&now)[NS], const double (&up)[NUP], const double (&diag)[NDG], const double (&left)[NS],
                                       const double xem, const double yem, const double e_now, const bool start,
                                       const double* __restrict__ tab) const {
    // left child advances: source (i - 1, j)
    now[IIW] = xem + lse(lse(up[U_IMM] + imm_iiw, up[U_IMI] + imi_iiw, tab), up[U_IIW] + iiw_iiw, tab);
    now[IIX] = xem + lse(up[U_IMD] + imd_iix, up[U_IIX] + iix_iix, tab);
    now[IMD] = xem + lse(lse(lse(up[U_WWW] + www_imd, up[U_WWX] + wwx_imd, tab), up[U_WXW] + wxw_imd, tab), up[U_IDD] + idd_imd, tab);
    double www = now[IIW] + iiw_www;
    now[WWX] = lse(now[IIX] + iix_wwx, now[IMD] + imd_wwx, tab);
    // right child advances: source (i, j - 1)
    now[IMI] = yem + lse(left[IMM] + imm_imi, left[IMI] + imi_imi, tab);
    now[IDI] = yem + lse(left[IDM] + idm_idi, left[IDI] + idi_idi, tab);
    now[IDM] = yem + lse(lse(lse(left[WWW] + www_idm, left[WWX] + wwx_idm, tab), left[WXW] + wxw_idm, tab), left[IDD] + idd_idm, tab);
    www = lse(www, now[IMI] + imi_www, tab);
    now[WXW] = lse(now[IDI] + idi_wxw, now[IDM] + idm_wxw, tab);
    // both advance: source (i - 1, j - 1)
    now[IMM] = e_now + lse(lse(lse(diag[D_WWW] + www_imm, diag[D_WWX] + wwx_imm, tab), diag[D_WXW] + wxw_imm, tab), diag[D_IDD] + idd_imm, tab);
    if (start) now[IMM] = 0.0;                      // lpStart() = 0; WWW(0, 0) = imm_www follows
    www = lse(www, now[IMM] + imm_www, tab);
    now[WWW] = www;
    // the parent column neither child sees, from the wait states of this cell
    now[IDD] = lse(lse(www + www_idd, now[WWX] + wwx_idd, tab), now[WXW] + wxw_idd, tab);
  }
  // lpEnd (src/sampler.cpp:1330-1333)
  template <class At>
  static __device__ __forceinline__ double lp_end(const DevSibling& J, const At at, const double* __restrict__ tab) {
    const double ed = at(IDD), e0 = at(WWW), e1 = at(WWX), e2 = at(WXW);
    return lse(lse(lse(ed + J.T[IDD][EEE], e0 + J.T[WWW][EEE], tab), e1 + J.T[WWX][EEE], tab), e2 + J.T[WXW][EEE], tab);
  }

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

// one job of the ABI -> its device job and its arrays in the arena
int fill_job(DevSibling& J, const hx_sibling_job& j, Arena& a) {
  if (j.l_len >= 64 * HXBR_MAX_STRIPS)
    return api_fail(HX_ERR_RANGE, "hx_sibling_batch_create: a left child profile of more than 65535 positions");
  if (j.l_len < 0 || j.r_len < 0 || j.components < 1 || j.alphabet < 1 || (j.l_len && (!j.l_sub || !j.l_emit || !j.log_root)) ||
      (j.r_len && (!j.r_sub || !j.r_emit)) || (j.max_distance >= 0 && (!j.l_env || !j.r_env)))
    return api_fail(HX_ERR_INVALID_ARG, "hx_sibling_batch_create: inconsistent job (lengths, components, missing arrays)");
  J.X = j.l_len + 1; J.Y = j.r_len + 1;
  J.CA = j.components * j.alphabet;
  J.C = j.components;
  J.max_dist = j.max_distance;
  for (int s = 0; s < NS; ++s)
    for (int d = 0; d < 12; ++d) J.T[s][d] = j.trans[s][d];
  // logInnerProduct's three-vector term is (logRoot + lSub) + rSub (src/logsumexp.h:139-144): the first sum here
  std::vector<double> rooted((size_t)j.l_len * J.CA);
  for (size_t p = 0; p < (size_t)j.l_len; ++p)
    for (int q = 0; q < J.CA; ++q) rooted[p * J.CA + q] = j.log_root[q] + j.l_sub[p * J.CA + q];
  a.put(J.x_pwm, rooted.data(), rooted.size());
  a.put(J.y_sub, j.r_sub, (size_t)j.r_len * J.CA);
  a.put(J.x_emit, j.l_emit, (size_t)j.l_len);
  a.put(J.y_emit, j.r_emit, (size_t)j.r_len);
  put_env(a, J, j.l_env, j.r_env, true);
  return HX_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

struct hx_sibling_batch : PairBatch<DevSibling, NS> {};

extern "C" {

int hx_sibling_batch_destroy(hx_sibling_batch* b) { delete b; return HX_OK; }

int hx_sibling_batch_create(const hx_sibling_job* jobs, int32_t n_jobs, hx_sibling_batch** out) {
  return hx_sibling_batch::create(jobs, n_jobs, out, fill_job);
}

int hx_sibling_batch_run(hx_sibling_batch* b, void* stream) { return hx_sibling_batch::run<SiblingCell>(b, stream); }

int hx_sibling_batch_results(hx_sibling_batch* b, double* lp_end) { return hx_sibling_batch::results(b, lp_end); }

int hx_sibling_batch_read_matrix(hx_sibling_batch* b, int32_t job, double* out) { return hx_sibling_batch::read_matrix(b, job, out); }

int64_t hx_sibling_batch_total_cells(const hx_sibling_batch* b) { return hx_sibling_batch::total_cells(b); }

int hx_sibling_batch_last_kernel_ms(hx_sibling_batch* b, float* fill_ms, float* step_ms) {
  return hx_sibling_batch::last_kernel_ms(b, fill_ms, step_ms);
}

int hx_sibling_batch_sample_paths(hx_sibling_batch* b, const uint32_t* words, const int64_t* word_off, uint8_t* states, int64_t cap,
                                  int32_t* n_steps, int32_t* words_used) {
  return pair_walk_paths<SiblingCell, false>(b, words, word_off, states, cap, n_steps, words_used);
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
