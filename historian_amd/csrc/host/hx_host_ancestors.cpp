// Ancestral sequence prediction after a reconstruction: Reconstructor::predictAncestors (reference src/recon.cpp:1072-1090)
// over AlignColSumProduct::appendAncestralReconstructedColumn / appendAncestralPostProbColumn (src/sumprod.cpp:401-426).
//
// The reference walks the alignment column by column with one SumProduct object.  Here the gapped reconstruction is
// tokenised once and every column goes through the device in one hx_sumprod_ancestors call (hx_ancestors.hip), which
// hands back the most probable residue of every wildcard and, for -ancprob, the log posteriors of every node.  exp(R t) of
// a branch is ProbModel(model, t).subMat, the reference's own choice in SumProduct's constructor (src/sumprod.cpp:37-43).
#include <cmath>

#include "../../../include/historian_hip.h"
#include "hx_host.h"

namespace historian {

void Reconstructor::predictAncestors(Dataset& dataset) {
  if (!predictAncestralSequence) return;
  const vguard<FastSeq> gapped = dataset.gappedRecon();
  const ReconTree& tree = dataset.tree;
  const size_t N = (size_t)tree.nodes(), A = model.alphabetSize(), C = (size_t)model.components();
  Assert(N == gapped.size(), "Number of nodes in tree (%d) does not match number of sequences (%d)", (int)N, (int)gapped.size());
  dataset.gappedAncestralRecon = gapped;
  dataset.gappedAncestralReconPostProb.clear();
  const size_t cols = N ? gapped[0].seq.size() : 0;
  if (cols == 0) return;
  vguard<int8_t> tokens(cols * N);
  for (size_t r = 0; r < N; ++r) {
    Assert(gapped[r].seq.size() == cols, "Alignment rows differ in length");
    for (size_t c = 0; c < cols; ++c) {
      const char g = gapped[r].seq[c];
      // (SumProduct::initColumn: whatever the alphabet does not hold is a wildcard)
      tokens[c * N + r] = Alignment::isGap(g) ? (int8_t)-2 : (int8_t)tokenize(g, model.alphabet);
    }
  }
  vguard<int32_t> parent(N);
  vguard<double> insProb(C * A), logCptWeight(C), branchSub(C * N * A * A, 0.);
  for (size_t r = 0; r < N; ++r) parent[r] = (int32_t)tree.parent[r];
  for (size_t c = 0; c < C; ++c) {
    logCptWeight[c] = log(model.cptWeight[c]);
    for (size_t i = 0; i < A; ++i) insProb[c * A + i] = model.insProb[c][i];
  }
  for (size_t r = 0; r + 1 < N; ++r) {
    const ProbModel pm(model, tree.branchLength((TreeNodeIndex)r));
    for (size_t c = 0; c < C; ++c)
      for (size_t i = 0; i < A; ++i)
        for (size_t j = 0; j < A; ++j) branchSub[((c * N + r) * A + i) * A + j] = pm.subMat[c][i][j];
  }
  hx_sumprod_model m = {};                          // (no eigen basis: those pointers stay null)
  m.alph_size = (int32_t)A;
  m.components = (int32_t)C;
  m.n_nodes = (int32_t)N;
  m.parent = parent.data();
  m.ins_prob = insProb.data();
  m.log_cpt_weight = logCptWeight.data();
  m.branch_sub = branchSub.data();
  vguard<int8_t> best(cols * N);
  vguard<double> post(reportAncestralSequenceProbability ? cols * N * A : 0);
  detail::ensureDevice();
  detail::check(hx_sumprod_ancestors(&m, tokens.data(), (int64_t)cols, nullptr, best.data(), post.empty() ? nullptr : post.data(), nullptr),
                "hx_sumprod_ancestors");
  const LogProb lpMin = log(ancestralSequenceMinProb), lpMax = log(1.);
  for (size_t r = 0; r < N; ++r)
    for (size_t c = 0; c < cols; ++c) {
      if (!Alignment::isWildcard(gapped[r].seq[c])) continue;
      dataset.gappedAncestralRecon[r].seq[c] = model.alphabet[(size_t)best[c * N + r]];
      if (!reportAncestralSequenceProbability) continue;
      const double* lp = &post[(c * N + r) * A];
      for (size_t tok = 0; tok < A; ++tok)
        if (lp[tok] >= lpMin && lp[tok] <= lpMax) dataset.gappedAncestralReconPostProb[r][c][model.alphabet[tok]] = exp(lp[tok]);
    }
}

void Reconstructor::predictAllAncestors(vguard<Dataset*>& datasets) {
  for (Dataset* d : datasets) predictAncestors(*d);
}

}  // namespace historian
