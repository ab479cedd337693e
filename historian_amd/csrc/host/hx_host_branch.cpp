// Host mirror of the per-branch pair DPs: Refiner::BranchMatrix (reference src/refiner.cpp:10-104)
// and Sampler::BranchMatrix (src/sampler.cpp:1005-1084) over TreeAlignFuncs::SparseDPMatrix<3> (src/sampler.h:66-215).
// Everything that is per position - the child profile through the branch's substitution matrix, its insertion scores, the
// eleven transition scores - is prepared here in the reference's arithmetic; the lattice is filled on the device
// (hx_branch.hip) and stays there: the best path, the sampled path and the cells along a path come from the device
// (hx_pairdp.h), the dense copy is read only when cell() is called (or with HX_HOST_WALKS=1, which keeps the host walks).
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "hx_host.h"
#include "../../../include/historian_hip.h"

namespace historian {

static const double kNegInf = -std::numeric_limits<double>::infinity();

namespace detail {
static std::atomic<long> g_denseReads(0);
bool hostWalks() {
  const char* e = getenv("HX_HOST_WALKS");
  return e && strcmp(e, "1") == 0;
}
long denseMatrixReads() { return g_denseReads.load(); }
void countDenseMatrixRead() { ++g_denseReads; }
}  // namespace detail

double TreeAlignFuncs::transProb(const ProbModel& p, State src, State dest) {
  // rows: leaving Match, leaving Insert, leaving Delete; columns: into Match, Insert, Delete, End
  const double table[3][4] = {
      {(1 - p.ins) * (1 - p.del), p.ins, (1 - p.ins) * p.del, 1 - p.ins},
      {(1 - p.insExt) * (1 - p.del), p.insExt, (1 - p.insExt) * p.del, 1 - p.insExt},
      {1 - p.delExt, 0., p.delExt, 1 - p.delExt}};
  return table[src][dest];
}

TreeAlignFuncs::PosWeightMatrix TreeAlignFuncs::preMultiply(const PosWeightMatrix& child, const vguard<Mat>& logSubProb) {
  PosWeightMatrix through(child.size());
  for (size_t pos = 0; pos < child.size(); ++pos) {
    through[pos].resize(logSubProb.size());
    for (size_t cpt = 0; cpt < logSubProb.size(); ++cpt) {
      const Mat& sub = logSubProb[cpt];
      Vec& out = through[pos][cpt];
      out.assign(sub.size(), kNegInf);
      for (size_t a = 0; a < sub.size(); ++a)
        for (size_t b = 0; b < child[pos][cpt].size(); ++b) log_accum_exp(out[a], sub[a][b] + child[pos][cpt][b]);
    }
  }
  return through;
}

vguard<LogProb> TreeAlignFuncs::calcInsProbs(const PosWeightMatrix& child, const vguard<vguard<LogProb>>& logInsProb,
                                             const vguard<LogProb>& logCptWeight) {
  vguard<LogProb> scores(child.size(), kNegInf);
  for (size_t pos = 0; pos < child.size(); ++pos)
    for (size_t cpt = 0; cpt < logInsProb.size(); ++cpt)
      for (size_t a = 0; a < child[pos][cpt].size(); ++a)
        log_accum_exp(scores[pos], logCptWeight[cpt] + logInsProb[cpt][a] + child[pos][cpt][a]);
  return scores;
}

TreeAlignFuncs::PosWeightMatrix TreeAlignFuncs::leafPWM(const FastSeq& seq, const string& alphabet, int components) {
  PosWeightMatrix pwm(seq.seq.size(), vguard<vguard<LogProb>>(components, vguard<LogProb>(alphabet.size(), kNegInf)));
  for (size_t pos = 0; pos < seq.seq.size(); ++pos) {
    const int tok = tokenize(seq.seq[pos], alphabet);
    for (int cpt = 0; cpt < components; ++cpt)
      for (size_t a = 0; a < alphabet.size(); ++a)
        if (tok < 0 || (size_t)tok == a) pwm[pos][cpt][a] = 0;        // (a wildcard is every residue)
  }
  return pwm;
}

static vguard<Mat> logOf(const vguard<Mat>& subMat) {
  vguard<Mat> out = subMat;
  for (Mat& m : out)
    for (Vec& row : m)
      for (double& v : row) v = log(v);
  return out;
}

TreeAlignFuncs::BranchMatrixBase::BranchMatrixBase(const RateModel& rates, const PosWeightMatrix& parent, const PosWeightMatrix& child,
                                                   double branchLength, const GuideAlignmentEnvelope& envelope,
                                                   const vguard<SeqIdx>& xEnvelopePos, const vguard<SeqIdx>& yEnvelopePos,
                                                   AlignRowIndex parentRow, AlignRowIndex childRow, bool viterbi)
    : model(rates), probModel(rates, std::max(1e-9 /* Tree::minBranchLength, src/tree.h:24 */, branchLength)), logProbModel(probModel),
      xRow(parentRow), yRow(childRow), xSeq(parent), ySub(preMultiply(child, logOf(probModel.subMat))),
      yEmit(calcInsProbs(child, logProbModel.logInsProb, logProbModel.logCptWeight)),
      xSize((SeqIdx)xEnvelopePos.size()), ySize((SeqIdx)yEnvelopePos.size()), lpEnd(kNegInf), env(envelope), xEnvPos(xEnvelopePos),
      yEnvPos(yEnvelopePos) {
  Assert(xSize == parent.size() + 1 && ySize == child.size() + 1, "Envelope positions do not match the profiles");
  setTransitions();

  // flatten for the C ABI
  const int C = probModel.components(), A = (int)rates.alphabetSize();
  vguard<double> xFlat, yFlat;
  for (const auto& col : parent) for (const auto& cpt : col) xFlat.insert(xFlat.end(), cpt.begin(), cpt.end());
  for (const auto& col : ySub) for (const auto& cpt : col) yFlat.insert(yFlat.end(), cpt.begin(), cpt.end());
  vguard<int32_t> xe(xSize, 0), ye(ySize, 0);
  if (env.initialized()) {
    for (SeqIdx i = 0; i < xSize; ++i) xe[i] = env.cumulativeMatches[env.row1PosToCol[xEnvPos[i]]];
    for (SeqIdx j = 0; j < ySize; ++j) ye[j] = env.cumulativeMatches[env.row2PosToCol[yEnvPos[j]]];
  }
  hx_branch_job job;
  job.x_len = (int32_t)parent.size(); job.y_len = (int32_t)child.size();
  job.components = C; job.alphabet = A;
  job.x_pwm = xFlat.data(); job.y_sub = yFlat.data(); job.y_emit = yEmit.data();
  const LogProb t[3][4] = {{mm, mi, md, me}, {im, ii, id, ie}, {dm, lpTrans(Delete, Insert), dd, de}};
  for (int s = 0; s < 3; ++s)
    for (int d = 0; d < 4; ++d) job.trans[s][d] = t[s][d];
  job.x_env = env.initialized() ? xe.data() : nullptr;
  job.y_env = env.initialized() ? ye.data() : nullptr;
  job.max_distance = env.maxDistance;
  detail::ensureDevice();
  hx_branch_batch* b = nullptr;
  detail::check(hx_branch_batch_create(&job, 1, &b), "hx_branch_batch_create");
  detail::check(hx_branch_batch_run(b, viterbi ? 1 : 0, nullptr), "hx_branch_batch_run");
  batch.reset(b, [](hx_branch_batch* p) { hx_branch_batch_destroy(p); });
  detail::check(hx_branch_batch_results(b, &lpEnd), "hx_branch_batch_results");
}

void TreeAlignFuncs::BranchMatrixBase::setTransitions() {
  mm = lpTrans(Match, Match); mi = lpTrans(Match, Insert); md = lpTrans(Match, Delete); me = lpTrans(Match, End);
  im = lpTrans(Insert, Match); ii = lpTrans(Insert, Insert); id = lpTrans(Insert, Delete); ie = lpTrans(Insert, End);
  dm = lpTrans(Delete, Match); dd = lpTrans(Delete, Delete); de = lpTrans(Delete, End);
}

// ---- the matrix of a branch of a resident history: nothing per position is computed or held on the host ----

// the batch of the one branch above `node`: the logs of the branch's model (the host's libm), the transition scores and the
// envelope's coordinates go in, the profiles stay on the device
static std::shared_ptr<hx_branch_batch> residentBranchBatch(hx_history* resident, const ProbModel& probModel, const LogProbModel& logProbModel,
                                                            TreeNodeIndex node, const GuideAlignmentEnvelope& env, const vguard<SeqIdx>& xEnvPos,
                                                            const vguard<SeqIdx>& yEnvPos, bool normalize) {
  vguard<double> logSub, logIns;
  for (const Mat& m : logOf(probModel.subMat))
    for (const Vec& row : m) logSub.insert(logSub.end(), row.begin(), row.end());
  for (const auto& cpt : logProbModel.logInsProb) logIns.insert(logIns.end(), cpt.begin(), cpt.end());
  vguard<int32_t> xe(xEnvPos.size(), 0), ye(yEnvPos.size(), 0);
  if (env.initialized()) {
    for (size_t i = 0; i < xe.size(); ++i) xe[i] = env.cumulativeMatches[env.row1PosToCol[xEnvPos[i]]];
    for (size_t j = 0; j < ye.size(); ++j) ye[j] = env.cumulativeMatches[env.row2PosToCol[yEnvPos[j]]];
  }
  hx_history_branch br = {};
  br.node = (int32_t)node;
  br.log_sub = logSub.data();
  br.log_ins = logIns.data();
  const TreeAlignFuncs::State states[4] = {TreeAlignFuncs::Match, TreeAlignFuncs::Insert, TreeAlignFuncs::Delete, TreeAlignFuncs::End};
  for (int s = 0; s < 3; ++s)
    for (int d = 0; d < 4; ++d) br.trans[s][d] = log(TreeAlignFuncs::transProb(probModel, states[s], states[d]));
  br.x_env = env.initialized() ? xe.data() : nullptr;
  br.y_env = env.initialized() ? ye.data() : nullptr;
  br.max_distance = env.maxDistance;
  detail::ensureDevice();
  hx_branch_batch* b = nullptr;
  detail::check(hx_history_branch_batch_create(resident, 0, normalize ? 1 : 0, &br, 1, nullptr, &b), "hx_history_branch_batch_create");
  return std::shared_ptr<hx_branch_batch>(b, [](hx_branch_batch* p) { hx_branch_batch_destroy(p); });
}

// [len][C][A] of job 0's x_pwm or y_sub, read back for the host walks; empty otherwise
static TreeAlignFuncs::PosWeightMatrix residentProfile(hx_branch_batch* b, bool ofParent, size_t len, size_t C, size_t A) {
  TreeAlignFuncs::PosWeightMatrix pwm;
  if (!detail::hostWalks()) return pwm;
  vguard<double> flat(len * C * A);
  detail::check(hx_branch_batch_read_inputs(b, 0, ofParent ? flat.data() : nullptr, ofParent ? nullptr : flat.data(), nullptr), "hx_branch_batch_read_inputs");
  pwm.assign(len, vguard<vguard<LogProb>>(C, vguard<LogProb>(A)));
  const double* v = flat.data();
  for (auto& pos : pwm)
    for (auto& cpt : pos)
      for (auto& lp : cpt) lp = *v++;
  return pwm;
}

static vguard<LogProb> residentInsertions(hx_branch_batch* b, size_t len) {
  vguard<LogProb> yEmit(len);
  detail::check(hx_branch_batch_read_inputs(b, 0, nullptr, nullptr, yEmit.data()), "hx_branch_batch_read_inputs");
  return yEmit;
}

TreeAlignFuncs::BranchMatrixBase::BranchMatrixBase(hx_history* resident, const RateModel& rates, const ReconTree& tree, TreeNodeIndex node,
                                                   double branchLength, const GuideAlignmentEnvelope& envelope, const vguard<SeqIdx>& xEnvelopePos,
                                                   const vguard<SeqIdx>& yEnvelopePos, bool viterbi, bool normalize)
    : model(rates), probModel(rates, std::max(1e-9 /* Tree::minBranchLength, src/tree.h:24 */, branchLength)), logProbModel(probModel),
      xRow((AlignRowIndex)tree.parent[node]), yRow((AlignRowIndex)node),
      batch(residentBranchBatch(resident, probModel, logProbModel, node, envelope, xEnvelopePos, yEnvelopePos, normalize)),
      xRead(residentProfile(batch.get(), true, xEnvelopePos.size() - 1, (size_t)probModel.components(), rates.alphabetSize())), xSeq(xRead),
      ySub(residentProfile(batch.get(), false, yEnvelopePos.size() - 1, (size_t)probModel.components(), rates.alphabetSize())),
      yEmit(residentInsertions(batch.get(), yEnvelopePos.size() - 1)), xSize((SeqIdx)xEnvelopePos.size()), ySize((SeqIdx)yEnvelopePos.size()),
      lpEnd(kNegInf), env(envelope), xEnvPos(xEnvelopePos), yEnvPos(yEnvelopePos) {
  vguard<int64_t> len((size_t)tree.nodes());
  detail::check(hx_history_row_lengths(resident, len.data()), "hx_history_row_lengths");
  Assert((int64_t)xSize == len[tree.parent[node]] + 1 && (int64_t)ySize == len[node] + 1, "Envelope positions do not match the rows of the history");
  setTransitions();
  detail::check(hx_branch_batch_run(batch.get(), viterbi ? 1 : 0, nullptr), "hx_branch_batch_run");
  detail::check(hx_branch_batch_results(batch.get(), &lpEnd), "hx_branch_batch_results");
}

LogProb TreeAlignFuncs::BranchMatrixBase::cell(SeqIdx xpos, SeqIdx ypos, unsigned int state) const {
  if (state == End) return (xpos == xSize - 1 && ypos == ySize - 1) ? lpEnd : kNegInf;
  Assert(xpos < xSize && ypos < ySize && state < 3, "cell out of range");
  if (cells.empty()) {
    cells.resize((size_t)3 * xSize * ySize);
    detail::check(hx_branch_batch_read_matrix(batch.get(), 0, cells.data()), "hx_branch_batch_read_matrix");
    detail::countDenseMatrixRead();
  }
  return cells[((size_t)xpos * ySize + ypos) * 3 + state];
}

bool TreeAlignFuncs::BranchMatrixBase::inEnvelope(SeqIdx xpos, SeqIdx ypos) const {
  return xpos == 0 || ypos == 0 || xpos == xSize - 1 || ypos == ySize - 1 || env.inRange(xEnvPos[xpos], yEnvPos[ypos]);
}

LogProb TreeAlignFuncs::BranchMatrixBase::logMatch(SeqIdx xpos, SeqIdx ypos) const {
  LogProb total = kNegInf;      // over the components, of the sum over the residues (src/logsumexp.h:146-151)
  for (size_t cpt = 0; cpt < xSeq[xpos - 1].size(); ++cpt) log_accum_exp(total, logInnerProduct(xSeq[xpos - 1][cpt], ySub[ypos - 1][cpt]));
  return total;
}

LogProb TreeAlignFuncs::BranchMatrixBase::lpTrans(State src, State dest) const { return log(transProb(probModel, src, dest)); }

LogProb TreeAlignFuncs::BranchMatrixBase::lpEmit(const CellCoords& at) const {
  if (at.state == Match) return (at.xpos > 0 && at.ypos > 0) ? logMatch(at.xpos, at.ypos) : kNegInf;
  if (at.state == Insert) return at.ypos > 0 ? yEmit[at.ypos - 1] : kNegInf;
  return 0;
}

void TreeAlignFuncs::BranchMatrixBase::getColumn(const CellCoords& at, bool& xUngapped, bool& yUngapped) {
  xUngapped = at.state == Delete || (at.state == Match && at.xpos > 0 && at.ypos > 0);
  yUngapped = at.state == Insert || (at.state == Match && at.xpos > 0 && at.ypos > 0);
}

// The best alignment: from the End state back to the start, at every cell the source state whose score plus transition plus
// this cell's emission is largest (the first such state in the order Match, Insert, Delete), src/refiner.cpp:62-104.
AlignPath TreeAlignFuncs::BranchMatrixBase::pathOfStates(const unsigned char* states, int nSteps) const {
  CellCoords at{(SeqIdx)(xSize - 1), (SeqIdx)(ySize - 1), End};
  vguard<bool> xBack, yBack;
  for (int k = 0; k < nSteps; ++k) {
    bool xHere, yHere;
    getColumn(at, xHere, yHere);
    if (xHere || yHere) { xBack.push_back(xHere); yBack.push_back(yHere); }
    at = CellCoords{(SeqIdx)(at.xpos - (xHere ? 1 : 0)), (SeqIdx)(at.ypos - (yHere ? 1 : 0)), states[k]};
  }
  Assert(at.xpos == 0 && at.ypos == 0, "A device walk stopped at cell (%u,%u)", at.xpos, at.ypos);
  AlignPath path;
  path[xRow] = AlignRowPath(xBack.rbegin(), xBack.rend());
  path[yRow] = AlignRowPath(yBack.rbegin(), yBack.rend());
  return path;
}

static void walkFailed(int code, const char* what) {
  Assert(code != -2, "%s: traceback state has zero probability", what);
  Assert(code != -1, "%s: the matrix's end score is -inf", what);
  Assert(code >= 0, "%s: the device walk failed (code %d)", what, code);
}

AlignPath Refiner::BranchMatrix::best() const {
  if (!detail::hostWalks()) {
    const int64_t cap = std::max<int64_t>(1, hx_branch_batch_max_steps(batch.get()));
    vguard<unsigned char> states((size_t)cap);
    int32_t nSteps = 0;
    detail::check(hx_branch_batch_best_paths(batch.get(), states.data(), cap, &nSteps), "hx_branch_batch_best_paths");
    walkFailed(nSteps, "Refiner::BranchMatrix::best");
    return pathOfStates(states.data(), nSteps);
  }
  CellCoords at{(SeqIdx)(xSize - 1), (SeqIdx)(ySize - 1), End};
  vguard<bool> xBack, yBack;
  while (at.xpos > 0 || at.ypos > 0) {
    bool xHere, yHere;
    getColumn(at, xHere, yHere);
    if (xHere || yHere) { xBack.push_back(xHere); yBack.push_back(yHere); }
    const SeqIdx px = at.xpos - (xHere ? 1 : 0), py = at.ypos - (yHere ? 1 : 0);
    const LogProb emit = lpEmit(at);
    LogProb top = kNegInf;
    int from = -1;
    for (int s = 0; s < 3; ++s) {
      const LogProb via = cell(px, py, s) + lpTrans((State)s, (State)at.state) + emit;
      if (via > top) { top = via; from = s; }
    }
    Assert(from >= 0, "Could not find traceback state from cell (%u,%u,%u)", at.xpos, at.ypos, at.state);
    at = CellCoords{px, py, (unsigned)from};
  }
  AlignPath path;
  path[xRow] = AlignRowPath(xBack.rbegin(), xBack.rend());
  path[yRow] = AlignRowPath(yBack.rbegin(), yBack.rend());
  return path;
}

// Sampler::BranchMatrix::sample (src/sampler.cpp:1088-1120): from End back to the start, at every step one of the three source
// states drawn by its share (random_key_log, src/util.h:220-236: one 32-bit draw).  On the device the walk takes its words
// from a copy of the generator; the real generator is then advanced by what the walk used.
AlignPath Sampler::BranchMatrix::sample(random_engine& generator) const {
  if (!detail::hostWalks()) {
    const int64_t cap = std::max<int64_t>(1, hx_branch_batch_max_steps(batch.get()));
    random_engine ahead = generator;
    vguard<uint32_t> words((size_t)cap);
    for (uint32_t& w : words) w = (uint32_t)ahead();
    const int64_t off[2] = {0, cap};
    vguard<unsigned char> states((size_t)cap);
    int32_t nSteps = 0, used = 0;
    detail::check(hx_branch_batch_sample_paths(batch.get(), words.data(), off, states.data(), cap, &nSteps, &used), "hx_branch_batch_sample_paths");
    walkFailed(nSteps, "Sampler::BranchMatrix::sample");
    generator.discard((unsigned long long)used);
    return pathOfStates(states.data(), nSteps);
  }
  CellCoords at{(SeqIdx)(xSize - 1), (SeqIdx)(ySize - 1), End};
  vguard<bool> xBack, yBack;
  while (at.xpos > 0 || at.ypos > 0) {
    bool xHere, yHere;
    getColumn(at, xHere, yHere);
    if (xHere || yHere) { xBack.push_back(xHere); yBack.push_back(yHere); }
    const SeqIdx px = at.xpos - (xHere ? 1 : 0), py = at.ypos - (yHere ? 1 : 0);
    const LogProb emit = lpEmit(at);
    double via[3], top = kNegInf;
    for (int s = 0; s < 3; ++s) {
      via[s] = cell(px, py, s) + lpTrans((State)s, (State)at.state) + emit;
      top = std::max(top, via[s]);
    }
    Assert(top > kNegInf, "Traceback state has zero probability at cell (%u,%u,%u)", at.xpos, at.ypos, at.state);
    double total = 0;
    for (int s = 0; s < 3; ++s) total += exp(via[s] - top);
    double left = generator() / (((double)random_engine::max()) + 1) * total;
    int from = -1;
    for (int s = 0; s < 3 && from < 0; ++s)
      if ((left -= exp(via[s] - top)) <= 0) from = s;
    Assert(from >= 0, "random_key_log failed");
    at = CellCoords{px, py, (unsigned)from};
  }
  AlignPath path;
  path[xRow] = AlignRowPath(xBack.rbegin(), xBack.rend());
  path[yRow] = AlignRowPath(yBack.rbegin(), yBack.rend());
  return path;
}

// The score of one alignment through the matrix (src/sampler.cpp:1122-1154), summed here in the reference's order; the cells
// along the path and their logMatch come from the device in one gather (or, with HX_HOST_WALKS=1, from the dense copy).
LogProb TreeAlignFuncs::BranchMatrixBase::logPathProb(const AlignPath& path) const {
  const AlignRowPath &xPath = path.at(xRow), &yPath = path.at(yRow);
  const AlignColIndex cols = alignPathColumns(path);
  vguard<hx_pair_cell> at;
  CellCoords c{0, 0, Start};
  bool left = false;
  for (AlignColIndex col = 0; col < cols && !left; ++col) {
    if (xPath[col]) ++c.xpos;
    if (yPath[col]) ++c.ypos;
    c.state = getState(xPath[col], yPath[col]);
    if (c.xpos >= xSize || c.ypos >= ySize || !inEnvelope(c.xpos, c.ypos)) left = true;
    else at.push_back(hx_pair_cell{(int32_t)c.xpos, (int32_t)c.ypos, (int32_t)c.state});
  }
  if (left) return kNegInf;
  vguard<double> value(at.size()), match(at.size());
  if (detail::hostWalks())
    for (size_t q = 0; q < at.size(); ++q) {
      value[q] = cell(at[q].xpos, at[q].ypos, at[q].state);
      match[q] = at[q].state == Match ? logMatch(at[q].xpos, at[q].ypos) : 0;
    }
  else
    detail::check(hx_branch_batch_read_cells(batch.get(), 0, (int64_t)at.size(), at.data(), value.data(), match.data()), "hx_branch_batch_read_cells");
  LogProb lp = 0;
  unsigned int state = Start;
  for (size_t q = 0; q < at.size(); ++q) {
    const unsigned int before = state;
    state = at[q].state;
    const LogProb lpe = state == Match ? match[q] : (state == Insert ? yEmit[at[q].ypos - 1] : 0);
    lp += lpTrans((State)before, (State)state) + lpe;
    lp = std::min(lp, value[q]);      // "mitigate precision errors"
  }
  return lp + lpTrans((State)state, End);
}

LogProb Sampler::BranchMatrix::logPostProb(const AlignPath& path) const {
  const LogProb lp = logPathProb(path);
  return std::min(lp, lpEnd) - lpEnd;
}

}  // namespace historian
