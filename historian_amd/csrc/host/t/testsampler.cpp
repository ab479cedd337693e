// The host-only parts of the sampler mirror (hx_host_sampler.cpp), stand-alone: the coalescent prior, pairPath and the indel
// sum, the two tree-height proposals on fixed generators, Move::accept.  No device call is made, so the program runs on a
// machine without a GPU - also as `make sanitize` builds it, under AddressSanitizer and UBSan.  tests/test_sampler_mirror.py
// compares what it prints with historian_amd/treesampler.py.
//   testsampler <model.json>
#include <cstdio>
#include <cstdlib>
#include "../hx_host.h"
using namespace historian;

static void printTree(const char* tag, const ReconTree& tree) {
  printf("%s", tag);
  for (TreeNodeIndex n = 0; n < tree.nodes(); ++n) printf(" %d:%a", tree.parent[n], tree.branchLen[n]);
  printf("\n");
}

int main(int argc, char** argv) {
  Require(argc == 2, "Usage: %s <model.json>", argv[0]);
  RateModel model;
  model.readFile(argv[1]);
  // ---- the prior ----
  const ReconTree three = ReconTree::parse("((a:1,b:1)ab:2,c:3)root;");
  printTree("three", three);
  SimpleTreePrior prior;
  printf("prior %a", prior.treeLogLikelihood(three));
  prior.populationSize = 2;
  printf(" %a\n", prior.treeLogLikelihood(three));
  // ---- a history of five rows: pairPath, the indel and root terms ----
  const ReconTree tree = ReconTree::parse("((a:0.25,b:0.25)ab:0.5,(c:0.4,d:0.4)cd:0.35)root:0;");
  printTree("tree", tree);
  const char* rows[7] = {"ac-gt--a-cgt", "a-tgtca--c-t", "a**gt-*a-c*t", "--cgtaac-g--", "t-cg-aacgg--", "*-cg*aac*g--", "****-****-*-"};
  TreeAlignFuncs::History history;
  history.tree = tree;
  for (TreeNodeIndex n = 0; n < tree.nodes(); ++n) {
    FastSeq fs;
    fs.name = tree.nodeName[n];
    fs.seq = rows[n];
    history.gapped.push_back(fs);
    printf("row %s %s\n", fs.name.c_str(), fs.seq.c_str());
  }
  const Alignment align(history.gapped);
  for (TreeNodeIndex n = 0; n < tree.root(); ++n) {
    const TreeNodeIndex p = tree.parent[n];
    const AlignPath pp = TreeAlignFuncs::pairPath(align.path, p, n);
    printf("pairpath %d ", n);
    for (size_t col = 0; col < pp.at(p).size(); ++col) putchar("MID"[TreeAlignFuncs::BranchMatrixBase::getState(pp.at(p)[col], pp.at(n)[col])]);
    RateModel indelOnly;
    indelOnly.alphabet = model.alphabet;
    indelOnly.insRate = model.insRate; indelOnly.delRate = model.delRate;
    indelOnly.insExtProb = model.insExtProb; indelOnly.delExtProb = model.delExtProb;
    const ProbModel probs(indelOnly, tree.branchLength(n));
    printf(" %a\n", TreeAlignFuncs::logBranchPathLikelihood(probs, pp, p, n));
  }
  printf("indels %a\nroot %a\n", TreeAlignFuncs::indelLogLikelihood(model, history), TreeAlignFuncs::rootLogLikelihood(model, history));
  // ---- the proposals: seeds until the root and another node have both been drawn ----
  for (unsigned seed = 1; seed <= 8; ++seed) {
    Sampler::random_engine generator(seed), before(seed);
    const TreeNodeIndex drawn = Sampler::randomInternalNode(tree, generator);
    const bool untouched = generator == before;       // random_element's generator by value
    ReconTree proposed = tree;
    TreeNodeIndex node = -1;
    vguard<TreeNodeIndex> changed;
    const LogProb logJacobian = Sampler::NodeHeightMove::propose(proposed, generator, node, changed);
    printf("nodeheight seed %u node %d drawn %d untouched %d jacobian %a changed", seed, node, drawn, (int)untouched, logJacobian);
    for (TreeNodeIndex c : changed) printf(" %d", c);
    printf("\n");
    printTree("proposed", proposed);
  }
  {
    Sampler::random_engine generator(3);
    ReconTree proposed = tree;
    vguard<TreeNodeIndex> changed;
    const LogProb logJacobian = Sampler::RescaleMove::propose(proposed, generator, changed);
    printf("rescale jacobian %a changed %zu\n", logJacobian, changed.size());
    printTree("proposed", proposed);
  }
  // ---- Move::accept ----
  {
    Sampler::random_engine generator(5), before(5);
    Sampler::Move move;
    move.logAcceptProb = 0.;
    const bool a0 = move.accept(generator);
    move.logAcceptProb = 1.5;
    const bool a1 = move.accept(generator);
    const bool noDraw = generator == before;
    move.logAcceptProb = -std::numeric_limits<double>::infinity();
    const bool a2 = move.accept(generator);
    move.nullify("test");
    const bool a3 = move.accept(generator);
    printf("accept %d %d nodraw %d minusinf %d nullified %d\n", (int)a0, (int)a1, (int)noDraw, (int)a2, (int)a3);
    const vguard<double> rates = {0, 0, 0, 2, 2};
    int seen[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 200; ++k) ++seen[Sampler::randomIndex(rates, generator)];
    printf("randomindex %d %d %d %d %d %d\n", seen[0], seen[1], seen[2], seen[3], seen[4], seen[5]);
  }
  return 0;
}
