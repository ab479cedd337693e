// The tree-height chain on a fixed alignment: SimpleTreePrior, TreeAlignFuncs::logLikelihood of a whole history and its
// parts, Sampler::Move / NodeHeightMove / RescaleMove and Sampler::sample / run (reference src/sampler.cpp:9-31, 150-189,
// 372-450, 478-557, 927-1003, 1608-1746).
//
// Host code: the prior, the root term, pairPath and the indel term added in path order (the reference's bits), the moves'
// tree arithmetic and their draws from std::mt19937.  Device: the substitution term.  The current history is resident
// there (hx_history.hip through hx_history_*); a move proposes the branches it changed, and sample() accepts or rejects.
// exp(R t) of a branch is ProbModel(model, t).subMat, as in SumProduct's constructor (src/sumprod.cpp:37-43): the history
// takes the rate matrices once and computes it on the device from the branch lengths (hx_history_create_from_lengths,
// hx_history_propose_lengths), bit for bit RateModel::getSubProbMatrix; HX_HISTORY_HOST_EXPM=1 computes it with
// getSubProbMatrix on the host and uploads the matrices (hx_history_create, hx_history_propose) - the same output.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <numeric>
#include <sstream>

#include "../../../include/historian_hip.h"
#include "hx_host.h"

namespace historian {

// ---- Tree (src/tree.cpp:692-704) and a Newick reader -------------------------------------------

vguard<double> ReconTree::distanceFromRoot() const {
  vguard<double> dist(nodes(), 0.);
  for (TreeNodeIndex n = nodes() - 2; n >= 0; --n) dist[n] = std::max(0., branchLen[n]) + dist[parent[n]];
  return dist;
}

namespace {

struct NewickReader {
  const string& text;
  size_t pos = 0;
  ReconTree tree;
  explicit NewickReader(const string& newick) : text(newick) {}
  bool more() const { return pos < text.size(); }
  TreeNodeIndex node() {
    vguard<TreeNodeIndex> kids;
    Require(more(), "Newick: unexpected end");
    if (text[pos] == '(') {
      ++pos;
      while (true) {
        kids.push_back(node());
        Require(more(), "Newick: unexpected end");
        if (text[pos] == ',') { ++pos; continue; }
        Require(text[pos] == ')', "Newick: expected ) at position %u", (unsigned)pos);
        ++pos;
        break;
      }
    }
    size_t start = pos;
    while (more() && !strchr(",():;", text[pos])) ++pos;
    string label = text.substr(start, pos - start);
    double len = 0;
    if (more() && text[pos] == ':') {
      start = ++pos;
      while (more() && !strchr(",();", text[pos])) ++pos;
      len = atof(text.substr(start, pos - start).c_str());
    }
    const TreeNodeIndex me = tree.nodes();
    tree.addNode(-1, len, label.empty() ? "node" + std::to_string(me) : label);
    for (TreeNodeIndex k : kids) tree.parent[k] = me;
    return me;
  }
};

}  // namespace

ReconTree ReconTree::parse(const string& newick) {
  string trimmed;
  for (char c : newick)
    if (!isspace((unsigned char)c)) trimmed.push_back(c);
  NewickReader reader(trimmed);
  reader.node();
  reader.tree.finish();
  return reader.tree;
}

// ---- SimpleTreePrior (src/sampler.cpp:9-31) -----------------------------------------------------

double SimpleTreePrior::coalescenceRate(int lineages) const { return (((double)lineages * (lineages - 1)) / 2) / (double)populationSize; }

LogProb SimpleTreePrior::treeLogLikelihood(const ReconTree& tree) const {
  const vguard<double> distanceFromRoot = tree.distanceFromRoot();
  vguard<size_t> nodesByDistanceFromRoot(distanceFromRoot.size());           // orderedIndices (src/util.h:242-255)
  std::iota(nodesByDistanceFromRoot.begin(), nodesByDistanceFromRoot.end(), (size_t)0);
  std::sort(nodesByDistanceFromRoot.begin(), nodesByDistanceFromRoot.end(), [&](size_t a, size_t b) { return distanceFromRoot[a] < distanceFromRoot[b]; });
  size_t lineages = 0;
  LogProb lp = 0;
  double lastEventTime = 0;
  for (auto iter = nodesByDistanceFromRoot.rbegin(); iter != nodesByDistanceFromRoot.rend(); ++iter) {
    const double eventTime = distanceFromRoot[*iter];
    if (lineages > 1) lp -= coalescenceRate((int)lineages) * (lastEventTime - eventTime);
    lastEventTime = eventTime;
    if (tree.isLeaf((TreeNodeIndex)*iter)) ++lineages;
    else --lineages;
  }
  return lp;
}

// ---- TreeAlignFuncs: the likelihood of a history (src/sampler.cpp:150-189, 372-450) -----------------

AlignPath TreeAlignFuncs::pairPath(const AlignPath& path, TreeNodeIndex node1, TreeNodeIndex node2) {
  AlignPath p;
  size_t nDel = 0;
  const AlignColIndex cols = alignPathColumns(path);
  const AlignRowPath& row1 = path.at(node1);
  const AlignRowPath& row2 = path.at(node2);
  AlignRowPath& r1 = p[node1];
  AlignRowPath& r2 = p[node2];
  for (AlignColIndex col = 0; col < cols; ++col) {
    const bool c1 = row1[col], c2 = row2[col];
    if (!(c1 || c2)) continue;
    if (c1 && !c2) { ++nDel; continue; }             // a deletion waits for the next Match
    if (c1)                                          // Match: the deferred deletions first
      for (; nDel > 0; --nDel) { r1.push_back(true); r2.push_back(false); }
    r1.push_back(c1);
    r2.push_back(c2);
  }
  for (; nDel > 0; --nDel) { r1.push_back(true); r2.push_back(false); }
  Assert(alignPathResiduesInRow(r1) == alignPathResiduesInRow(row1) && alignPathResiduesInRow(r2) == alignPathResiduesInRow(row2), "Rows don't match");
  return p;
}

LogProb TreeAlignFuncs::rootLogLikelihood(const RateModel& model, const History& history) {
  size_t rootLen = 0;
  for (char c : history.gapped[history.tree.root()].seq)
    if (!Alignment::isGap(c)) ++rootLen;
  const double rootExt = rootExtProb(model);
  return log(1. - rootExt) + log(rootExt) * rootLen;
}

LogProb TreeAlignFuncs::logBranchPathLikelihood(const ProbModel& probModel, const AlignPath& path, TreeNodeIndex parent, TreeNodeIndex child) {
  const AlignColIndex cols = alignPathColumns(path);
  State state = Start;
  LogProb lp = 0;
  for (AlignColIndex col = 0; col < cols; ++col) {
    const State nextState = BranchMatrixBase::getState(path.at(parent)[col], path.at(child)[col]);
    lp += log(transProb(probModel, state, nextState));
    state = nextState;
  }
  lp += log(transProb(probModel, state, End));
  return lp;
}

namespace {

// ProbModel without exp(R t): the indel term reads the four indel probabilities only
struct IndelProbs : ProbModel {
  IndelProbs(const RateModel& model, double t) : ProbModel(indelOnly(model), t) {}
  static RateModel indelOnly(const RateModel& model) {
    RateModel m;
    m.alphabet = model.alphabet;
    m.insRate = model.insRate; m.delRate = model.delRate;
    m.insExtProb = model.insExtProb; m.delExtProb = model.delExtProb;
    return m;
  }
};

LogProb indelTerm(const RateModel& model, const AlignPath& alignPath, const ReconTree& tree) {
  LogProb lpGaps = 0;
  for (TreeNodeIndex node = 0; node < tree.root(); ++node) {
    const TreeNodeIndex parent = tree.parent[node];
    const IndelProbs probModel(model, tree.branchLength(node));
    lpGaps += TreeAlignFuncs::logBranchPathLikelihood(probModel, TreeAlignFuncs::pairPath(alignPath, parent, node), parent, node);
  }
  return lpGaps;
}

void flatMatrices(const RateModel& model, double t, double* out) {           // [C][A][A]
  const size_t A = model.alphabetSize();
  const vguard<Mat> sub = model.getSubProbMatrix(t);
  for (size_t c = 0; c < sub.size(); ++c)
    for (size_t i = 0; i < A; ++i)
      for (size_t j = 0; j < A; ++j) out[(c * A + i) * A + j] = sub[c][i][j];
}

bool hostExpm() {
  const char* e = getenv("HX_HISTORY_HOST_EXPM");
  return e && atoi(e) != 0;
}

}  // namespace

LogProb TreeAlignFuncs::indelLogLikelihood(const RateModel& model, const History& history) {
  return indelTerm(model, Alignment(history.gapped).path, history.tree);
}

hx_history* TreeAlignFuncs::residentHistory(const RateModel& model, const History& history) {
  const ReconTree& tree = history.tree;
  const size_t N = (size_t)tree.nodes(), A = model.alphabetSize(), C = (size_t)model.components();
  Assert(N == history.gapped.size(), "Number of nodes in tree (%d) does not match number of sequences (%d)", (int)N, (int)history.gapped.size());
  const size_t cols = history.gapped[0].seq.size();
  vguard<int8_t> tokens(cols * N);
  for (size_t r = 0; r < N; ++r) {
    Assert(history.gapped[r].seq.size() == cols, "Alignment rows differ in length");
    for (size_t c = 0; c < cols; ++c) {
      const char g = history.gapped[r].seq[c];
      tokens[c * N + r] = Alignment::isGap(g) ? (int8_t)-2 : (int8_t)tokenize(g, model.alphabet);
    }
  }
  vguard<int32_t> parent(N);
  vguard<double> insProb(C * A), logCptWeight(C);
  for (size_t r = 0; r < N; ++r) parent[r] = (int32_t)tree.parent[r];
  for (size_t c = 0; c < C; ++c) {
    logCptWeight[c] = log(model.cptWeight[c]);
    for (size_t i = 0; i < A; ++i) insProb[c * A + i] = model.insProb[c][i];
  }
  hx_history_model m = {};
  m.alph_size = (int32_t)A;
  m.components = (int32_t)C;
  m.n_nodes = (int32_t)N;
  m.parent = parent.data();
  m.ins_prob = insProb.data();
  m.log_cpt_weight = logCptWeight.data();
  hx_history* h = nullptr;
  detail::ensureDevice();
  if (hostExpm()) {
    vguard<double> branchSub(C * N * A * A, 0.), one(C * A * A);
    for (size_t r = 0; r + 1 < N; ++r) {
      flatMatrices(model, tree.branchLength((TreeNodeIndex)r), one.data());
      for (size_t c = 0; c < C; ++c) std::copy(one.begin() + c * A * A, one.begin() + (c + 1) * A * A, branchSub.begin() + (c * N + r) * A * A);
    }
    detail::check(hx_history_create(&m, tokens.data(), (int64_t)cols, branchSub.data(), nullptr, &h), "hx_history_create");
    return h;
  }
  vguard<double> rate(C * A * A), lengths(N, 0.);
  for (size_t c = 0; c < C; ++c)
    for (size_t i = 0; i < A; ++i)
      for (size_t j = 0; j < A; ++j) rate[(c * A + i) * A + j] = model.subRate[c][i][j];
  for (size_t r = 0; r + 1 < N; ++r) lengths[r] = tree.branchLength((TreeNodeIndex)r);
  detail::check(hx_history_create_from_lengths(&m, tokens.data(), (int64_t)cols, rate.data(), lengths.data(), nullptr, &h), "hx_history_create_from_lengths");
  return h;
}

LogProb TreeAlignFuncs::substLogLikelihood(const RateModel& model, const History& history) {
  std::shared_ptr<hx_history> h(residentHistory(model, history), hx_history_destroy);
  double lpSub = 0;
  detail::check(hx_history_log_like(h.get(), 0, &lpSub, nullptr), "hx_history_log_like");
  return lpSub;
}

// the maps getConditionalPWMs serves name a neighbour for every node; PruneAndRegraftMove's (on a detached tree: a node with
// nothing excluded, neighbours of another tree) is not among them
static void neighboursOnly(const ReconTree& tree, const map<TreeNodeIndex, TreeNodeIndex>& exclude) {
  const TreeNodeIndex N = tree.nodes();
  for (const auto& ne : exclude) {
    const TreeNodeIndex node = ne.first, ex = ne.second;
    const bool inside = node >= 0 && node < N && ex >= 0 && ex < N;
    if (!inside || (tree.parent[node] != ex && tree.parent[ex] != node)) Abort("%s moves are not built", Sampler::Move::typeName(Sampler::Move::PruneAndRegraft));
  }
}

map<TreeNodeIndex, TreeAlignFuncs::PosWeightMatrix> TreeAlignFuncs::getConditionalPWMs(hx_history* resident, const RateModel& model, const ReconTree& tree,
                                                                                      const map<TreeNodeIndex, TreeNodeIndex>& exclude, bool normalize) {
  const TreeNodeIndex N = tree.nodes();
  const size_t A = model.alphabetSize(), C = (size_t)model.components();
  neighboursOnly(tree, exclude);
  map<TreeNodeIndex, PosWeightMatrix> pwms;
  if (exclude.empty()) return pwms;
  vguard<int64_t> len((size_t)N);
  detail::check(hx_history_row_lengths(resident, len.data()), "hx_history_row_lengths");
  vguard<int32_t> nodes, excluded;
  vguard<vguard<double>> flat;
  vguard<double*> out;
  for (const auto& ne : exclude) {
    nodes.push_back((int32_t)ne.first);
    excluded.push_back((int32_t)ne.second);
    flat.emplace_back((size_t)len[ne.first] * C * A);
  }
  for (auto& f : flat) out.push_back(f.empty() ? nullptr : f.data());
  detail::check(hx_history_excluded_profiles(resident, 0, (int32_t)nodes.size(), nodes.data(), excluded.data(), normalize ? 1 : 0, out.data(), nullptr),
                "hx_history_excluded_profiles");
  for (size_t k = 0; k < nodes.size(); ++k) {
    if (flat[k].empty()) continue;                   // (the reference's map has no entry for a node without positions)
    PosWeightMatrix& pwm = pwms[nodes[k]];
    pwm.assign((size_t)len[nodes[k]], vguard<vguard<LogProb>>(C, vguard<LogProb>(A)));
    const double* v = flat[k].data();
    for (auto& pos : pwm)
      for (auto& cpt : pos)
        for (auto& lp : cpt) lp = *v++;
  }
  return pwms;
}

map<TreeNodeIndex, TreeAlignFuncs::PosWeightMatrix> TreeAlignFuncs::getConditionalPWMs(const RateModel& model, const ReconTree& tree, const vguard<FastSeq>& gapped,
                                                                                      const map<TreeNodeIndex, TreeNodeIndex>& exclude, const set<TreeNodeIndex>&,
                                                                                      const set<TreeNodeIndex>&, bool normalize) {
  neighboursOnly(tree, exclude);                     // (before a history is made for nothing)
  History history;
  history.gapped = gapped;
  history.tree = tree;
  std::shared_ptr<hx_history> h(residentHistory(model, history), hx_history_destroy);
  return getConditionalPWMs(h.get(), model, tree, exclude, normalize);
}

LogProb TreeAlignFuncs::logLikelihood(const SimpleTreePrior& treePrior, const RateModel& model, const History& history, const char*) {
  const LogProb lpTree = treePrior.treeLogLikelihood(history.tree);
  const LogProb lpRoot = rootLogLikelihood(model, history);
  const LogProb lpGaps = indelLogLikelihood(model, history);
  const LogProb lpSub = substLogLikelihood(model, history);
  return lpTree + lpRoot + lpGaps + lpSub;
}

// ---- Sampler::Move (src/sampler.cpp:478-557) ------------------------------------------------------

Sampler::Move::Move(Type type, const History& history, LogProb oldLogLikelihood, const string& samplerName)
    : type(type), oldHistory(history), oldLogLikelihood(oldLogLikelihood), samplerName(samplerName) {}

void Sampler::Move::initNewHistory(const ReconTree& tree, const vguard<FastSeq>& gapped) {
  newHistory.tree = tree;
  newHistory.gapped = gapped;
}

void Sampler::Move::initRatio(const Sampler& sampler) {
  LogProb terms[4];
  sampler.proposedTerms(*this, terms);
  newLogLikelihood = terms[0] + terms[1] + terms[2] + terms[3];
  const LogProb logOddsRatio = newLogLikelihood - oldLogLikelihood;
  const LogProb logHastingsRatio = logReverseProposal - logForwardProposal + logJacobian;
  logAcceptProb = logOddsRatio + logHastingsRatio;
}

void Sampler::Move::nullify(const char* reason) {
  newHistory = oldHistory;
  newLogLikelihood = oldLogLikelihood;
  logAcceptProb = logJacobian = logForwardProposal = logReverseProposal = 0;
  nullified = true;
  comment = string("(") + reason + ")";
}

const char* Sampler::Move::typeName(Type t) {
  switch (t) {
    case BranchAlign: return "Branch alignment";
    case NodeAlign: return "Node alignment";
    case PruneAndRegraft: return "Prune-and-regraft";
    case NodeHeight: return "Node height";
    case Rescale: return "Rescale";
    default: break;
  }
  return "Unknown";
}

bool Sampler::Move::accept(random_engine& generator) const {
  if (nullified) return false;
  if (logAcceptProb >= 0) return true;                // (no draw)
  std::bernoulli_distribution distribution(exp(logAcceptProb));
  return distribution(generator);
}

// ---- the two moves (src/sampler.cpp:927-1003) -------------------------------------------------------

TreeNodeIndex Sampler::randomInternalNode(const ReconTree& tree, random_engine& generator) {
  vguard<TreeNodeIndex> intNodes;
  intNodes.reserve(tree.nodes() / 2);
  for (TreeNodeIndex n = 0; n < tree.nodes(); ++n)
    if (!tree.isLeaf(n)) intNodes.push_back(n);
  Assert(!intNodes.empty(), "No internal nodes in tree");
  // random_element takes its generator by value (src/util.h:165-173): the draw works on a copy, the caller's does not advance
  random_engine copy = generator;
  std::uniform_int_distribution<int> distribution(0, (int)intNodes.size() - 1);
  return intNodes[(size_t)distribution(copy)];
}

LogProb Sampler::NodeHeightMove::propose(ReconTree& newTree, random_engine& generator, TreeNodeIndex& node, vguard<TreeNodeIndex>& changed) {
  LogProb logJacobian = 0;
  node = Sampler::randomInternalNode(newTree, generator);
  Assert(newTree.child[node].size() == 2, "Tree is not binary");
  const TreeNodeIndex leftChild = newTree.getChild(node, 0), rightChild = newTree.getChild(node, 1), parent = newTree.parent[node];
  const double lChildDist = newTree.branchLength(leftChild), rChildDist = newTree.branchLength(rightChild);
  const double minChildDist = std::min(lChildDist, rChildDist);
  if (parent < 0) {
    const double maxLogMultiplier = log(2);
    std::uniform_real_distribution<double> distribution(-maxLogMultiplier, maxLogMultiplier);
    const double logMultiplier = distribution(generator);
    const double multiplier = exp(logMultiplier);
    const double newMinChildDist = minChildDist * multiplier;
    newTree.branchLen[leftChild] = lChildDist - minChildDist + newMinChildDist;
    newTree.branchLen[rightChild] = rChildDist - minChildDist + newMinChildDist;
    logJacobian += logMultiplier;
    changed = {leftChild, rightChild};
  } else {
    const double pDist = std::max(0., newTree.branchLength(node));
    const double pDistRange = pDist + minChildDist;
    std::uniform_real_distribution<double> distribution(0, pDistRange);
    const double pDistNew = distribution(generator);
    const double cDistNew = pDistRange - pDistNew;
    newTree.branchLen[node] = pDistNew;
    newTree.branchLen[leftChild] = (lChildDist - minChildDist) + cDistNew;
    newTree.branchLen[rightChild] = (rChildDist - minChildDist) + cDistNew;
    changed = {leftChild, rightChild, node};
  }
  return logJacobian;
}

Sampler::NodeHeightMove::NodeHeightMove(const History& history, LogProb oldLogLikelihood, const Sampler& sampler, random_engine& generator)
    : Move(NodeHeight, history, oldLogLikelihood, sampler.name) {
  ReconTree newTree = history.tree;
  logForwardProposal = logReverseProposal = 0;
  logJacobian = propose(newTree, generator, node, changed);
  leftChild = newTree.getChild(node, 0);
  rightChild = newTree.getChild(node, 1);
  parent = newTree.parent[node];
  initNewHistory(newTree, oldHistory.gapped);
  initRatio(sampler);
}

LogProb Sampler::RescaleMove::propose(ReconTree& newTree, random_engine& generator, vguard<TreeNodeIndex>& changed) {
  const double maxLogMultiplier = log(2);
  std::uniform_real_distribution<double> distribution(-maxLogMultiplier, maxLogMultiplier);
  const double logMultiplier = distribution(generator);
  const double multiplier = exp(logMultiplier);
  for (double& d : newTree.branchLen) d *= multiplier;
  changed.clear();
  for (TreeNodeIndex n = 0; n < newTree.root(); ++n) changed.push_back(n);
  return logMultiplier;
}

Sampler::RescaleMove::RescaleMove(const History& history, LogProb oldLogLikelihood, const Sampler& sampler, random_engine& generator)
    : Move(Rescale, history, oldLogLikelihood, sampler.name) {
  ReconTree newTree = history.tree;
  logForwardProposal = logReverseProposal = 0;
  logJacobian = propose(newTree, generator, changed);
  initNewHistory(newTree, oldHistory.gapped);
  initRatio(sampler);
}

// ---- Sampler (src/sampler.cpp:1608-1746) ----------------------------------------------------------------

Sampler::Sampler(const RateModel& model, const SimpleTreePrior& treePrior)
    : model(&model), treePrior(&treePrior), moveRate(Move::TotalMoveTypes, 1.), movesProposed(Move::TotalMoveTypes, 0),
      movesAccepted(Move::TotalMoveTypes, 0), moveNanosecs(Move::TotalMoveTypes, 0.) {}

size_t Sampler::randomIndex(const vguard<double>& weights, random_engine& generator) {
  double norm = 0;
  for (double w : weights) {
    Assert(w >= 0, "Negative weights in random_index");
    norm += w;
  }
  Assert(norm > 0, "Zero weights in random_index");
  // random_double (src/util.h:138-142) divides by numeric_limits<result_type>::max() + 1.  For std::mt19937 result_type is
  // uint_fast32_t - 64 bits on LP64 - so there the variate stays below 2^-32 and the first type with a positive rate is
  // always drawn.  Here the divisor is the generator's own range, which is what the expression means.
  double variate = generator() / (((double)random_engine::max()) + 1) * norm;
  for (size_t n = 0; n < weights.size(); ++n)
    if ((variate -= weights[n]) <= 0) return n;
  return weights.size();
}

Sampler::Move Sampler::proposeMove(const History& oldHistory, LogProb oldLogLikelihood, random_engine& generator) const {
  const Move::Type type = (Move::Type)randomIndex(moveRate, generator);
  switch (type) {
    case Move::NodeHeight: return NodeHeightMove(oldHistory, oldLogLikelihood, *this, generator);
    case Move::Rescale: return RescaleMove(oldHistory, oldLogLikelihood, *this, generator);
    default: break;
  }
  Abort("%s moves are not built", Move::typeName(type));
  return Move();
}

LogProb Sampler::logLikelihood(const History& history, const char* suffix) const {
  return TreeAlignFuncs::logLikelihood(*treePrior, *model, history, suffix);
}

void Sampler::proposedTerms(const Move& move, LogProb terms[4]) const {
  Assert((bool)resident, "Sampler::initialize has not been called");
  const History& h = move.newHistory;
  const size_t A = model->alphabetSize(), C = (size_t)model->components(), n = move.changed.size();
  vguard<int32_t> nodes(n);
  for (size_t k = 0; k < n; ++k) nodes[k] = (int32_t)move.changed[k];
  terms[0] = treePrior->treeLogLikelihood(h.tree);
  terms[1] = currentTerms[1];                         // (the alignment is fixed: the root's row does not change)
  terms[2] = indelLogLikelihood(*model, h);
  if (hostExpm()) {
    vguard<double> mats(n * C * A * A);
    for (size_t k = 0; k < n; ++k) flatMatrices(*model, h.tree.branchLength(move.changed[k]), &mats[k * C * A * A]);
    detail::check(hx_history_propose(resident.get(), (int32_t)n, nodes.data(), mats.data(), &terms[3], nullptr), "hx_history_propose");
    return;
  }
  vguard<double> lengths(n);
  for (size_t k = 0; k < n; ++k) lengths[k] = h.tree.branchLength(move.changed[k]);
  detail::check(hx_history_propose_lengths(resident.get(), (int32_t)n, nodes.data(), lengths.data(), &terms[3], nullptr), "hx_history_propose_lengths");
}

void Sampler::initialize(const History& initialHistory, const string& samplerName) {
  name = samplerName;
  currentHistory = initialHistory;
  Assert(currentHistory.gapped.size() == (size_t)currentHistory.tree.nodes(), "Number of rows does not match the tree");
  for (TreeNodeIndex n = 0; n < currentHistory.tree.nodes(); ++n)
    Assert(currentHistory.gapped[n].name == currentHistory.tree.nodeName[n], "Row %d is %s, tree node %d is %s", n, currentHistory.gapped[n].name.c_str(), n,
           currentHistory.tree.nodeName[n].c_str());
  isUltrametric = currentHistory.tree.isUltrametric();
  if (!isUltrametric) Warn("WARNING: initial tree is not ultrametric");
  bestHistory = currentHistory;
  resident.reset(residentHistory(*model, currentHistory), hx_history_destroy);
  currentTerms[0] = treePrior->treeLogLikelihood(currentHistory.tree);
  currentTerms[1] = rootLogLikelihood(*model, currentHistory);
  currentTerms[2] = indelLogLikelihood(*model, currentHistory);
  detail::check(hx_history_log_like(resident.get(), 0, &currentTerms[3], nullptr), "hx_history_log_like");
  currentLogLikelihood = bestLogLikelihood = currentTerms[0] + currentTerms[1] + currentTerms[2] + currentTerms[3];
  // Sampler::initialize's rates; the moves that are not built stay at 0
  moveRate.assign(Move::TotalMoveTypes, 0.);
  moveRate[Move::NodeHeight] = 2;
  moveRate[Move::Rescale] = 2;
}

void Sampler::fixAlignment() {
  moveRate[Move::BranchAlign] = 0;
  moveRate[Move::NodeAlign] = 0;
}

void Sampler::sample(random_engine& generator) {
  const auto before = std::chrono::system_clock::now();
  Move move = proposeMove(currentHistory, currentLogLikelihood, generator);
  const auto after = std::chrono::system_clock::now();
  moveNanosecs[move.type] += (double)std::chrono::duration_cast<std::chrono::nanoseconds>(after - before).count();
  ++movesProposed[move.type];
  if (isUltrametric && !move.newHistory.tree.isUltrametric()) Warn("Move generated a non-ultrametric tree");
  const bool accepted = move.accept(generator);
  if (accepted) {
    detail::check(hx_history_accept(resident.get()), "hx_history_accept");
    currentHistory = move.newHistory;
    currentLogLikelihood = move.newLogLikelihood;
    ++movesAccepted[move.type];
  } else {
    detail::check(hx_history_reject(resident.get()), "hx_history_reject");
  }
  if (move.newLogLikelihood > bestLogLikelihood) {
    bestHistory = move.newHistory;
    bestLogLikelihood = move.newLogLikelihood;
  }
  if (keepMoveLog) {
    move.comment = accepted ? "accepted" : "rejected";
    move.oldHistory = History();
    move.newHistory.gapped.clear();
    moveLog.push_back(move);
  }
}

void Sampler::run(vguard<Sampler>& samplers, random_engine& generator, unsigned int nSamples) {
  vguard<double> nodes;
  for (const auto& sampler : samplers) nodes.push_back(sampler.currentHistory.tree.nodes());
  for (unsigned int n = 0; n < nSamples; ++n) samplers[randomIndex(nodes, generator)].sample(generator);
}

string Sampler::moveStats() const {
  std::ostringstream out;
  for (int t = 0; t < (int)Move::TotalMoveTypes; ++t)
    out << std::setw((int)Move::typeNameWidth()) << Move::typeName((Move::Type)t) << ": " << std::setw(5) << movesProposed[t] << " moves, " << std::setw(5)
        << movesAccepted[t] << " accepted, " << std::setw(12) << (moveNanosecs[t] / 1e9) << " seconds, " << std::setw(12)
        << ((double)movesAccepted[t] / (moveNanosecs[t] / 1e9)) << " accepted/sec" << std::endl;
  return out.str();
}

}  // namespace historian
