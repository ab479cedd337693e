// Host mirror of the sibling-pair parent-proposal DP: Sampler::SiblingMatrix (reference
// src/sampler.h:226-325, src/sampler.cpp:1185-1608) over TreeAlignFuncs::SparseDPMatrix<11>.  What is per position - the two
// child profiles through their branches' substitution matrices, their insertion scores, the root distribution - and the 35
// transition scores are prepared here in the reference's arithmetic; the lattice is filled on the device (hx_sibling.hip), one
// matrix or several in one batch, and stays there, the matrices of a fill sharing their batch: sample and logPostProb go
// through the device's walks and gather (hx_pairdp.h), the dense copy is read only when cell() is called (or with
// HX_HOST_WALKS=1, which keeps the host walks over it).
#include <cmath>
#include <limits>
#include <random>
#include "hx_host.h"
#include "../../../include/historian_hip.h"

namespace historian {

static const double kNegInf = -std::numeric_limits<double>::infinity();
typedef Sampler::SiblingMatrix SM;

static vguard<Mat> logOf(const vguard<Mat>& subMat) {
  vguard<Mat> out = subMat;
  for (Mat& m : out)
    for (Vec& row : m)
      for (double& v : row) v = log(v);
  return out;
}

SM::SiblingMatrix(const RateModel& rates, const Args& a, Deferred)
    : model(rates), lProbModel(rates, std::max(1e-9 /* Tree::minBranchLength, src/tree.h:24 */, a.plDist)),
      rProbModel(rates, std::max(1e-9, a.prDist)), lLogProbModel(lProbModel), rLogProbModel(rProbModel), lRow(a.lRow), rRow(a.rRow),
      pRow(a.pRow), lSub(preMultiply(*a.lSeq, logOf(lProbModel.subMat))), rSub(preMultiply(*a.rSeq, logOf(rProbModel.subMat))),
      lEmit(calcInsProbs(*a.lSeq, lLogProbModel.logInsProb, lLogProbModel.logCptWeight)),
      rEmit(calcInsProbs(*a.rSeq, rLogProbModel.logInsProb, rLogProbModel.logCptWeight)), xSize((SeqIdx)a.lEnvPos->size()),
      ySize((SeqIdx)a.rEnvPos->size()), lpEnd(kNegInf), env(*a.env), xEnvPos(*a.lEnvPos), yEnvPos(*a.rEnvPos) {
  Assert(xSize == a.lSeq->size() + 1 && ySize == a.rSeq->size() + 1, "Envelope positions do not match the profiles");
  for (int cpt = 0; cpt < rates.components(); ++cpt) {
    logRoot.push_back(log_vector(rates.insProb[cpt]));
    for (double& lp : logRoot.back()) lp += log(rates.cptWeight[cpt]);
  }
  imm_www = lpTransElimSelfLoopIDD(IMM, WWW); imm_imi = lpTransElimSelfLoopIDD(IMM, IMI); imm_iiw = lpTransElimSelfLoopIDD(IMM, IIW);
  imd_wwx = lpTransElimSelfLoopIDD(IMD, WWX); imd_iix = lpTransElimSelfLoopIDD(IMD, IIX);
  idm_wxw = lpTransElimSelfLoopIDD(IDM, WXW); idm_idi = lpTransElimSelfLoopIDD(IDM, IDI);
  idd_imm = lpTransElimSelfLoopIDD(IDD, IMM); idd_imd = lpTransElimSelfLoopIDD(IDD, IMD); idd_idm = lpTransElimSelfLoopIDD(IDD, IDM);
  idd_eee = lpTransElimSelfLoopIDD(IDD, EEE);
  www_imm = lpTransElimSelfLoopIDD(WWW, IMM); www_imd = lpTransElimSelfLoopIDD(WWW, IMD); www_idm = lpTransElimSelfLoopIDD(WWW, IDM);
  www_idd = lpTransElimSelfLoopIDD(WWW, IDD); www_eee = lpTransElimSelfLoopIDD(WWW, EEE);
  wwx_imm = lpTransElimSelfLoopIDD(WWX, IMM); wwx_imd = lpTransElimSelfLoopIDD(WWX, IMD); wwx_idm = lpTransElimSelfLoopIDD(WWX, IDM);
  wwx_idd = lpTransElimSelfLoopIDD(WWX, IDD); wwx_eee = lpTransElimSelfLoopIDD(WWX, EEE);
  wxw_imm = lpTransElimSelfLoopIDD(WXW, IMM); wxw_imd = lpTransElimSelfLoopIDD(WXW, IMD); wxw_idm = lpTransElimSelfLoopIDD(WXW, IDM);
  wxw_idd = lpTransElimSelfLoopIDD(WXW, IDD); wxw_eee = lpTransElimSelfLoopIDD(WXW, EEE);
  imi_www = lpTransElimSelfLoopIDD(IMI, WWW); imi_imi = lpTransElimSelfLoopIDD(IMI, IMI); imi_iiw = lpTransElimSelfLoopIDD(IMI, IIW);
  iiw_www = lpTransElimSelfLoopIDD(IIW, WWW); iiw_iiw = lpTransElimSelfLoopIDD(IIW, IIW);
  idi_wxw = lpTransElimSelfLoopIDD(IDI, WXW); idi_idi = lpTransElimSelfLoopIDD(IDI, IDI);
  iix_wwx = lpTransElimSelfLoopIDD(IIX, WWX); iix_iix = lpTransElimSelfLoopIDD(IIX, IIX);
}

static SM::Args argsOf(const TreeAlignFuncs::PosWeightMatrix& lSeq, const TreeAlignFuncs::PosWeightMatrix& rSeq, double plDist,
                       double prDist, const GuideAlignmentEnvelope& env, const vguard<SeqIdx>& lEnvPos, const vguard<SeqIdx>& rEnvPos,
                       AlignRowIndex l, AlignRowIndex r, AlignRowIndex p) {
  return SM::Args{&lSeq, &rSeq, plDist, prDist, &env, &lEnvPos, &rEnvPos, l, r, p};
}

SM::SiblingMatrix(const RateModel& rates, const PosWeightMatrix& lSeq, const PosWeightMatrix& rSeq, double plDist, double prDist,
                  const GuideAlignmentEnvelope& envelope, const vguard<SeqIdx>& lEnvPos, const vguard<SeqIdx>& rEnvPos, AlignRowIndex l,
                  AlignRowIndex r, AlignRowIndex p)
    : SiblingMatrix(rates, argsOf(lSeq, rSeq, plDist, prDist, envelope, lEnvPos, rEnvPos, l, r, p), Deferred()) {
  fillOnDevice(vguard<SiblingMatrix*>(1, this));
}

vguard<std::unique_ptr<SM>> SM::fillBatch(const RateModel& rates, const vguard<Args>& args) {
  vguard<std::unique_ptr<SiblingMatrix>> made;
  vguard<SiblingMatrix*> raw;
  for (const Args& a : args) {
    made.emplace_back(new SiblingMatrix(rates, a, Deferred()));
    raw.push_back(made.back().get());
  }
  if (!raw.empty()) fillOnDevice(raw);
  return made;
}

void SM::transTable(double out[11][12]) const {
  for (int s = 0; s < 11; ++s)
    for (int d = 0; d < 12; ++d) out[s][d] = lpTransElimSelfLoopIDD((State)s, (State)d);
}

// the matrices as jobs of one hx_sibling_batch: fill, lpEnd, the dense copies
void SM::fillOnDevice(const vguard<SiblingMatrix*>& matrices) {
  struct Flat { vguard<double> lSub, rSub, root; vguard<int32_t> le, re; };
  vguard<Flat> flat(matrices.size());
  vguard<hx_sibling_job> jobs(matrices.size());
  for (size_t k = 0; k < matrices.size(); ++k) {
    SiblingMatrix& m = *matrices[k];
    Flat& f = flat[k];
    for (const auto& col : m.lSub) for (const auto& cpt : col) f.lSub.insert(f.lSub.end(), cpt.begin(), cpt.end());
    for (const auto& col : m.rSub) for (const auto& cpt : col) f.rSub.insert(f.rSub.end(), cpt.begin(), cpt.end());
    for (const auto& cpt : m.logRoot) f.root.insert(f.root.end(), cpt.begin(), cpt.end());
    f.le.assign(m.xSize, 0);
    f.re.assign(m.ySize, 0);
    if (m.env.initialized()) {
      for (SeqIdx i = 0; i < m.xSize; ++i) f.le[i] = m.env.cumulativeMatches[m.env.row1PosToCol[m.xEnvPos[i]]];
      for (SeqIdx j = 0; j < m.ySize; ++j) f.re[j] = m.env.cumulativeMatches[m.env.row2PosToCol[m.yEnvPos[j]]];
    }
    hx_sibling_job& job = jobs[k];
    job.l_len = (int32_t)m.lSub.size(); job.r_len = (int32_t)m.rSub.size();
    job.components = m.model.components(); job.alphabet = (int32_t)m.model.alphabetSize();
    job.l_sub = f.lSub.data(); job.r_sub = f.rSub.data(); job.log_root = f.root.data();
    job.l_emit = m.lEmit.data(); job.r_emit = m.rEmit.data();
    m.transTable(job.trans);
    job.l_env = m.env.initialized() ? f.le.data() : nullptr;
    job.r_env = m.env.initialized() ? f.re.data() : nullptr;
    job.max_distance = m.env.maxDistance;
  }
  detail::ensureDevice();
  hx_sibling_batch* b = nullptr;
  detail::check(hx_sibling_batch_create(jobs.data(), (int32_t)jobs.size(), &b), "hx_sibling_batch_create");
  detail::check(hx_sibling_batch_run(b, nullptr), "hx_sibling_batch_run");
  vguard<double> lp(jobs.size());
  detail::check(hx_sibling_batch_results(b, lp.data()), "hx_sibling_batch_results");
  const std::shared_ptr<hx_sibling_batch> shared(b, [](hx_sibling_batch* p) { hx_sibling_batch_destroy(p); });
  for (size_t k = 0; k < matrices.size(); ++k) {
    SiblingMatrix& m = *matrices[k];
    m.lpEnd = lp[k];
    m.batch = shared;
    m.jobIndex = (int)k;
    m.batchJobs = (int)matrices.size();
  }
}

LogProb SM::cell(SeqIdx xpos, SeqIdx ypos, unsigned int state) const {
  if (state == EEE) return (xpos == xSize - 1 && ypos == ySize - 1) ? lpEnd : kNegInf;
  Assert(xpos < xSize && ypos < ySize && state < 11, "cell out of range");
  if (cells.empty()) {
    cells.resize((size_t)11 * xSize * ySize);
    detail::check(hx_sibling_batch_read_matrix(batch.get(), jobIndex, cells.data()), "hx_sibling_batch_read_matrix");
    detail::countDenseMatrixRead();
  }
  return cells[((size_t)xpos * ySize + ypos) * 11 + state];
}

bool SM::inEnvelope(SeqIdx xpos, SeqIdx ypos) const {
  return xpos == 0 || ypos == 0 || xpos == xSize - 1 || ypos == ySize - 1 || env.inRange(xEnvPos[xpos], yEnvPos[ypos]);
}

// over the components, the three-vector logInnerProduct: terms (logRoot + lSub) + rSub (src/logsumexp.h:139-144)
LogProb SM::logMatch(SeqIdx xpos, SeqIdx ypos) const {
  LogProb total = kNegInf;
  for (size_t cpt = 0; cpt < logRoot.size(); ++cpt) {
    LogProb lip = kNegInf;
    const vguard<LogProb>&root = logRoot[cpt], &ls = lSub[xpos - 1][cpt], &rs = rSub[ypos - 1][cpt];
    for (size_t a = 0; a < root.size(); ++a) log_accum_exp(lip, root[a] + ls[a] + rs[a]);
    log_accum_exp(total, lip);
  }
  return total;
}

LogProb SM::lpEmit(const CellCoords& at) const {
  switch ((State)at.state) {
    case IMM: return at.xpos > 0 && at.ypos > 0 ? logMatch(at.xpos, at.ypos) : kNegInf;
    case IDM: case IMI: case IDI: return at.ypos > 0 ? rEmit[at.ypos - 1] : kNegInf;
    case IMD: case IIW: case IIX: return at.xpos > 0 ? lEmit[at.xpos - 1] : kNegInf;
    default: break;
  }
  return 0;
}

SM::State SM::getState(State src, bool leftUngapped, bool rightUngapped, bool parentUngapped) {
  if (parentUngapped) return leftUngapped ? (rightUngapped ? IMM : IMD) : (rightUngapped ? IDM : IDD);
  if (leftUngapped) return (src == IMD || src == IIX) ? IIX : IIW;
  if (rightUngapped) return (src == IDM || src == IDI) ? IDI : IMI;
  if (src == IDM || src == IDD || src == IDI) return WXW;
  if (src == IMD || src == IIX) return WWX;
  return WWW;
}

void SM::getColumn(const CellCoords& at, bool& l, bool& r, bool& p) {
  p = l = r = false;
  switch ((State)at.state) {
    case IMM: if (at.xpos > 0 && at.ypos > 0) p = l = r = true; break;
    case IMD: p = l = true; break;
    case IDM: p = r = true; break;
    case IDD: p = true; break;
    case IIW: case IIX: if (at.xpos > 0) l = true; break;
    case IMI: case IDI: if (at.ypos > 0) r = true; break;
    default: break;
  }
}

LogProb SM::lpTransElimSelfLoopIDD(State src, State dest) const {
  if (src != IDD) return lpTrans(src, dest);
  return dest == IDD ? kNegInf : lpTrans(src, dest) + iddExit();
}

LogProb SM::lpTrans(State src, State dest) const {
  const ProbModel &L = lProbModel, &R = rProbModel;
  const LogProb rootExt = log(model.insExtProb), rootNoExt = log(1 - model.insExtProb);
  const LogProb lIns = log(L.ins), lDel = log(L.del), lInsExt = log(L.insExt), lDelExt = log(L.delExt);
  const LogProb lNoIns = log(1 - L.ins), lNoDel = log(1 - L.del), lNoInsExt = log(1 - L.insExt), lNoDelExt = log(1 - L.delExt);
  const LogProb rIns = log(R.ins), rDel = log(R.del), rInsExt = log(R.insExt), rDelExt = log(R.delExt);
  const LogProb rNoIns = log(1 - R.ins), rNoDel = log(1 - R.del), rNoInsExt = log(1 - R.insExt), rNoDelExt = log(1 - R.delExt);
  switch (src) {
    case IMM:
      if (dest == WWW) return lNoIns + rNoIns;
      if (dest == IMI) return rIns;
      if (dest == IIW) return lIns + rNoIns;
      break;
    case IMD:
      if (dest == WWX) return lNoIns;
      if (dest == IIX) return lIns;
      break;
    case IDM:
      if (dest == WXW) return rNoIns;
      if (dest == IDI) return rIns;
      break;
    case IDD:
      if (dest == IDD) return iddStay();
      if (dest == IMM) return rootExt + lNoDelExt + rNoDelExt;
      if (dest == IMD) return rootExt + lNoDelExt + rDelExt;
      if (dest == IDM) return rootExt + lDelExt + rNoDelExt;
      if (dest == EEE) return rootNoExt + lNoDelExt + rNoDelExt;
      break;
    case WWW:
      if (dest == IMM) return rootExt + lNoDel + rNoDel;
      if (dest == IMD) return rootExt + lNoDel + rDel;
      if (dest == IDM) return rootExt + lDel + rNoDel;
      if (dest == IDD) return rootExt + lDel + rDel;
      if (dest == EEE) return 0;
      break;
    case WWX:
      if (dest == IMM) return rootExt + lNoDel + rNoDelExt;
      if (dest == IMD) return rootExt + lNoDel + rDelExt;
      if (dest == IDM) return rootExt + lDel + rNoDelExt;
      if (dest == IDD) return rootExt + lDel + rDelExt;
      if (dest == EEE) return rNoDelExt;
      break;
    case WXW:
      if (dest == IMM) return rootExt + lNoDelExt + rNoDel;
      if (dest == IMD) return rootExt + lNoDelExt + rDel;
      if (dest == IDM) return rootExt + lDelExt + rNoDel;
      if (dest == IDD) return rootExt + lDelExt + rDel;
      if (dest == EEE) return lNoDelExt;
      break;
    case IMI:
      if (dest == WWW) return lNoIns + rNoInsExt;
      if (dest == IMI) return rInsExt;
      if (dest == IIW) return lIns + rNoInsExt;
      break;
    case IIW:
      if (dest == WWW) return lNoInsExt;
      if (dest == IIW) return lInsExt;
      break;
    case IDI:
      if (dest == WXW) return rNoInsExt;
      if (dest == IDI) return rInsExt;
      break;
    case IIX:
      if (dest == WWX) return lNoInsExt;
      if (dest == IIX) return lInsExt;
      break;
    default: break;
  }
  return kNegInf;
}

LogProb SM::lpTransElimWait(State src, State dest) const {
  return log_sum_exp(lpTrans(src, dest), lpTrans(src, WWW) + lpTrans(WWW, dest), lpTrans(src, WWX) + lpTrans(WWX, dest),
                     lpTrans(src, WXW) + lpTrans(WXW, dest));
}

// From EEE at the last cell back to the start (src/sampler.cpp:1343-1386): at every step one of the eleven source states of
// the source cell, drawn by its share of the cell's sum (random_key_log, src/util.h:220-236: one 32-bit draw); an IDD column
// is repeated a geometric number of times, the self-loop the fill eliminated.
AlignPath SM::sample(random_engine& generator) const {
  if (detail::hostWalks()) return sampleOnHost(generator);
  return sampleBatch(vguard<const SiblingMatrix*>(1, this), vguard<random_engine*>(1, &generator))[0];
}

// The device's walk of every matrix given (hx_sibling_batch_sample_paths: one wavefront per job), matrices of one fill in one
// launch.  A walk takes its words from a copy of the matrix's generator, drawn ahead: one per step, two more at every visit
// of IDD - at most 3 (l + r) + 3 steps of which at most l + r + 1 stand in IDD.  The recorded states are then replayed
// against the real generator, which draws the IDD self-loop counts with the real distribution and ends where the host walk
// would leave it.
vguard<AlignPath> SM::sampleBatch(const vguard<const SiblingMatrix*>& matrices, const vguard<random_engine*>& generators) {
  Assert(matrices.size() == generators.size(), "sampleBatch: one generator per matrix");
  vguard<AlignPath> paths(matrices.size());
  vguard<bool> done(matrices.size(), false);
  for (size_t first = 0; first < matrices.size(); ++first) {
    if (done[first]) continue;
    if (detail::hostWalks()) {
      paths[first] = matrices[first]->sampleOnHost(*generators[first]);
      done[first] = true;
      continue;
    }
    // every matrix given that lives in this one's batch
    hx_sibling_batch* b = matrices[first]->batch.get();
    const int nJobs = matrices[first]->batchJobs;
    vguard<int> which(nJobs, -1);
    for (size_t k = first; k < matrices.size(); ++k)
      if (!done[k] && matrices[k]->batch.get() == b && which[matrices[k]->jobIndex] < 0) which[matrices[k]->jobIndex] = (int)k;
    const int64_t cap = std::max<int64_t>(1, hx_sibling_batch_max_steps(b));
    vguard<int64_t> off(nJobs + 1, 0);
    vguard<uint32_t> words;
    for (int j = 0; j < nJobs; ++j) {
      if (which[j] >= 0) {       // (a job nobody asked for gets no words: its walk ends at once)
        const SiblingMatrix& m = *matrices[which[j]];
        const size_t need = 5 * ((size_t)m.xSize + m.ySize) + 8;
        random_engine ahead = *generators[which[j]];
        for (size_t w = 0; w < need; ++w) words.push_back((uint32_t)ahead());
      }
      off[j + 1] = (int64_t)words.size();
    }
    vguard<unsigned char> states((size_t)nJobs * cap);
    vguard<int32_t> nSteps(nJobs), used(nJobs);
    detail::check(hx_sibling_batch_sample_paths(b, words.data(), off.data(), states.data(), cap, nSteps.data(), used.data()),
                  "hx_sibling_batch_sample_paths");
    for (int j = 0; j < nJobs; ++j) {
      if (which[j] < 0) continue;
      const size_t k = which[j];
      Assert(nSteps[j] != -2, "Traceback state has zero probability (sibling matrix %zu)", k);
      Assert(nSteps[j] >= 0, "The device walk of sibling matrix %zu failed (code %d)", k, nSteps[j]);
      const random_engine before = *generators[k];
      if (!matrices[k]->replay(&states[(size_t)j * cap], nSteps[j], *generators[k], paths[k])) {
        *generators[k] = before;
        paths[k] = matrices[k]->sampleOnHost(*generators[k]);
      }
      done[k] = true;
    }
  }
  return paths;
}

bool SM::replay(const unsigned char* states, int nSteps, random_engine& generator, AlignPath& path) const {
  CellCoords at{(SeqIdx)(xSize - 1), (SeqIdx)(ySize - 1), EEE};
  vguard<bool> lBack, rBack, pBack;
  for (int k = 0; k < nSteps; ++k) {
    bool l, r, p;
    getColumn(at, l, r, p);
    if (l || r || p) { lBack.push_back(l); rBack.push_back(r); pBack.push_back(p); }
    if ((State)at.state == IDD) {
      // the device walk skipped two words here: what libstdc++'s geometric_distribution takes unless its rejection loop runs
      random_engine expected = generator;
      expected.discard(2);
      std::geometric_distribution<int> loops(iddSelfLoopProb());
      for (int n = loops(generator); n > 0; --n) { lBack.push_back(l); rBack.push_back(r); pBack.push_back(p); }
      if (!(expected == generator)) return false;
    }
    generator();      // the step's draw
    at = CellCoords{(SeqIdx)(at.xpos - (l ? 1 : 0)), (SeqIdx)(at.ypos - (r ? 1 : 0)), states[k]};
  }
  Assert(at.xpos == 0 && at.ypos == 0, "A device walk stopped at cell (%u,%u)", at.xpos, at.ypos);
  path[lRow] = AlignRowPath(lBack.rbegin(), lBack.rend());
  path[rRow] = AlignRowPath(rBack.rbegin(), rBack.rend());
  path[pRow] = AlignRowPath(pBack.rbegin(), pBack.rend());
  return true;
}

AlignPath SM::sampleOnHost(random_engine& generator) const {
  CellCoords at{(SeqIdx)(xSize - 1), (SeqIdx)(ySize - 1), EEE};
  vguard<bool> lBack, rBack, pBack;
  while (at.xpos > 0 || at.ypos > 0) {
    bool l, r, p;
    getColumn(at, l, r, p);
    if (l || r || p) { lBack.push_back(l); rBack.push_back(r); pBack.push_back(p); }
    if ((State)at.state == IDD) {
      std::geometric_distribution<int> loops(iddSelfLoopProb());
      for (int n = loops(generator); n > 0; --n) { lBack.push_back(l); rBack.push_back(r); pBack.push_back(p); }
    }
    const SeqIdx px = at.xpos - (l ? 1 : 0), py = at.ypos - (r ? 1 : 0);
    const LogProb emit = lpEmit(at);
    double via[11], top = kNegInf;
    for (int s = 0; s < 11; ++s) {
      via[s] = cell(px, py, s) + lpTransElimSelfLoopIDD((State)s, (State)at.state) + emit;
      top = std::max(top, via[s]);
    }
    Assert(top > kNegInf, "Traceback state has zero probability at cell (%u,%u,%u)", at.xpos, at.ypos, at.state);
    double total = 0;
    for (int s = 0; s < 11; ++s) total += exp(via[s] - top);
    double left = generator() / (((double)random_engine::max()) + 1) * total;
    int from = -1;
    for (int s = 0; s < 11 && from < 0; ++s)
      if ((left -= exp(via[s] - top)) <= 0) from = s;
    Assert(from >= 0, "random_key_log failed");
    at = CellCoords{px, py, (unsigned)from};
  }
  AlignPath path;
  path[lRow] = AlignRowPath(lBack.rbegin(), lBack.rend());
  path[rRow] = AlignRowPath(rBack.rbegin(), rBack.rend());
  path[pRow] = AlignRowPath(pBack.rbegin(), pBack.rend());
  return path;
}

LogProb SM::logPostProb(const AlignPath& lrpPath) const {
  const AlignColIndex cols = alignPathColumns(lrpPath);
  const AlignRowPath &lPath = lrpPath.at(lRow), &rPath = lrpPath.at(rRow), &pPath = lrpPath.at(pRow);
  // the cells the path visits, then their values - one gather on the device, or the dense copy - then the reference's sum
  vguard<hx_pair_cell> at;
  CellCoords c{0, 0, SSS};
  for (AlignColIndex col = 0; col < cols; ++col) {
    const bool dl = lPath[col], dr = rPath[col], dp = pPath[col];
    if (dl) ++c.xpos;
    if (dr) ++c.ypos;
    c.state = getState((State)c.state, dl, dr, dp);
    if (c.xpos >= xSize || c.ypos >= ySize || !inEnvelope(c.xpos, c.ypos)) return kNegInf;
    at.push_back(hx_pair_cell{(int32_t)c.xpos, (int32_t)c.ypos, (int32_t)c.state});
  }
  vguard<double> value(at.size()), match(at.size());
  if (detail::hostWalks())
    for (size_t q = 0; q < at.size(); ++q) {
      value[q] = cell(at[q].xpos, at[q].ypos, at[q].state);
      match[q] = (at[q].state == IMM && at[q].xpos > 0 && at[q].ypos > 0) ? logMatch(at[q].xpos, at[q].ypos) : kNegInf;
    }
  else
    detail::check(hx_sibling_batch_read_cells(batch.get(), jobIndex, (int64_t)at.size(), at.data(), value.data(), match.data()),
                  "hx_sibling_batch_read_cells");
  LogProb lp = 0;
  State state = SSS;
  for (size_t q = 0; q < at.size(); ++q) {
    const State before = state;
    state = (State)at[q].state;
    const CellCoords here{(SeqIdx)at[q].xpos, (SeqIdx)at[q].ypos, (unsigned)at[q].state};
    lp += lpTransElimWait(before, state) + (state == IMM ? match[q] : lpEmit(here));
    lp = std::min(lp, value[q]);      // "mitigate precision errors"
  }
  lp += lpTransElimWait(state, EEE);
  lp = std::min(lp, lpEnd);
  return lp - lpEnd;
}

// the parent's profile: per parent column the product of what the children show there, normalised
// (src/sampler.cpp:1576-1608; as there, a child's position advances only inside parent columns)
TreeAlignFuncs::PosWeightMatrix SM::parentSeq(const AlignPath& lrpPath) const {
  PosWeightMatrix pwm;
  const AlignColIndex cols = alignPathColumns(lrpPath);
  const AlignRowPath &lPath = lrpPath.at(lRow), &rPath = lrpPath.at(rRow), &pPath = lrpPath.at(pRow);
  SeqIdx lPos = 0, rPos = 0;
  for (AlignColIndex col = 0; col < cols; ++col) {
    if (!pPath[col]) continue;
    vguard<vguard<LogProb>> prof(model.components(), vguard<LogProb>(model.alphabetSize(), 0));
    if (lPath[col]) {
      for (size_t cpt = 0; cpt < prof.size(); ++cpt)
        for (size_t a = 0; a < prof[cpt].size(); ++a) prof[cpt][a] += lSub[lPos][cpt][a];
      ++lPos;
    }
    if (rPath[col]) {
      for (size_t cpt = 0; cpt < prof.size(); ++cpt)
        for (size_t a = 0; a < prof[cpt].size(); ++a) prof[cpt][a] += rSub[rPos][cpt][a];
      ++rPos;
    }
    LogProb norm = kNegInf;
    for (const auto& cpt : prof)
      for (LogProb v : cpt) log_accum_exp(norm, v);
    for (auto& cpt : prof)
      for (LogProb& v : cpt) v -= norm;
    pwm.push_back(prof);
  }
  return pwm;
}

}  // namespace historian
