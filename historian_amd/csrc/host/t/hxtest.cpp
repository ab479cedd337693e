// One driver for the small checks of the host mirror; every sub-command prints what the reference's golden file for it holds
// (tests/test_host_mirror.py diffs the output byte for byte):
//   hxtest logsumexp [-slow|-fast]                 the 20 x 20 grid of data/logsumexp.txt (reference Makefile:206-208)
//   hxtest seqprofile <alphabet> <sequence>        leaf Profile as JSON (Makefile:239-240)
//   hxtest quickalign <pair.fa> <model.json> <t>   guide-alignment Viterbi of two sequences as gapped FASTA (Makefile:278-279)
//   hxtest expm <model.json> <t>                   exp(R t) of every mixture component as hex floats, row by row
//   hxtest expmtime <model.json> <t> <calls>       the host clock around <calls> calls of getSubProbMatrix near t
//   hxtest branch <pair.fa> <model.json> <t>       the two sequences as parent and child of one branch (next row N4): Viterbi
//                                                  and Forward log-likelihoods as hex floats, then the best alignment
//   hxtest sibling <pair.fa> <model.json> <tl> <tr> [band]   the two sequences as left and right child of an unobserved parent
//                                                  (N4, Sampler::SiblingMatrix; band: envelope around the ungapped diagonal):
//                                                  lpEnd as a hex float, a seeded sampled alignment, its logPostProb, the first
//                                                  rows of the parent profile, and fillBatch of two envelopes against single fills
//   hxtest walks <pair.fa> <model.json> <tl> <tr> [band]     the walks through the sibling matrix of the pair and through a branch
//                                                  matrix over it (left sequence as parent, right as child, branch tl): a
//                                                  seeded sampled alignment of either, its logPostProb, the generator's next
//                                                  word, best() of the Viterbi matrix, sampleBatch of a fillBatch against
//                                                  single samples, and the number of dense matrix copies read (0 unless
//                                                  HX_HOST_WALKS=1)
//   hxtest walktime <pair.fa> <model.json> <tl> <tr> <n> [band]   timing (tools/walks_bench.py): fillBatch of n copies of the
//                                                  pair's sibling matrix, then - timed apart - what a walk needs first (the dense
//                                                  copies with HX_HOST_WALKS=1, nothing otherwise), sampleBatch and logPostProb
//   hxtest treemoves <rows.fa> <tree.nh> <model.json> <steps> <seed>   a tree-height chain on a fixed alignment (node-height and
//                                                  rescale moves, hx_host_sampler.cpp): the four likelihood parts of the initial
//                                                  history, one line per step, the final tree
//   hxtest condpwm <rows.fa> <tree.nh> <model.json> <node> <normalize> [device]   the two excluded-neighbour profiles of the branch above
//                                                  <node> (TreeAlignFuncs::getConditionalPWMs), lpEnd of the unbanded
//                                                  Sampler::BranchMatrix built from them, a seeded sample and its logPostProb
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include "../hx_host.h"
#include "../../../../include/historian_hip.h"
using namespace historian;

namespace {

struct Command {
  const char* name;
  int minArgs, maxArgs;
  const char* usage;
  int (*run)(int nArgs, char** args);
};

int lseGrid(int nArgs, char** args) {
  const bool exactSum = nArgs == 1 && strcmp(args[0], "-slow") == 0;
  if (nArgs == 1 && !exactSum && strcmp(args[0], "-fast") != 0) return -1;
  std::cerr << "(running in " << (exactSum ? "slow" : "fast") << " mode)" << std::endl;
  // twenty values per axis, accumulated exactly as the golden file's producer did: repeated addition of 0.1
  vguard<double> axis;
  for (double v = 0; v < 2; v += .1) axis.push_back(v);
  for (double a : axis)
    for (double b : axis)
      std::cout << a << ' ' << b << ' ' << (exactSum ? log_sum_exp_slow(a, b) : log_sum_exp(a, b)) << std::endl;
  return 0;
}

int leafProfileJson(int, char** args) {
  FastSeq leaf;
  leaf.seq = args[1];
  Profile(1, string(args[0]), leaf, 0).writeJson(std::cout);
  return 0;
}

int guidePair(int, char** args) {
  const vguard<FastSeq> two = readFastSeqs(args[0]);
  Require(two.size() == 2, "Sequence file must have exactly two sequences");
  RateModel rates;
  rates.readFile(args[1]);
  DiagonalEnvelope all(two[0], two[1]);
  all.initFull();
  writeFastaSeqs(std::cout, QuickAlignMatrix(all, rates, atof(args[2])).gappedSeq());
  return 0;
}

int substitutionMatrix(int, char** args) {
  RateModel rates;
  rates.readFile(args[0]);
  for (const Mat& m : rates.getSubProbMatrix(atof(args[1])))
    for (const Vec& row : m) {
      for (double v : row) printf("%a ", v);
      printf("\n");
    }
  return 0;
}

// expmtime <modelfile> <time> <calls>: the host clock around <calls> calls of getSubProbMatrix(time * (1 + k / calls)), every
// component each; prints "expmtime <calls> <components> <ms in all>" (tools/history_bench.py's host-side figure)
int substitutionMatrixTime(int, char** args) {
  RateModel rates;
  rates.readFile(args[0]);
  const double t = atof(args[1]);
  const int calls = atoi(args[2]);
  double keep = 0;
  const auto start = std::chrono::steady_clock::now();
  for (int k = 0; k < calls; ++k) keep += rates.getSubProbMatrix(t * (1. + (double)k / calls))[0][0][0];
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - start).count();
  printf("expmtime %d %d %.6f\n", calls, rates.components(), ms);
  return keep > 0 ? 0 : 1;
}

int branchPair(int, char** args) {
  const vguard<FastSeq> two = readFastSeqs(args[0]);
  Require(two.size() == 2, "Sequence file must have exactly two sequences");
  RateModel rates;
  rates.readFile(args[1]);
  const int C = (int)rates.subRate.size();
  const auto parent = TreeAlignFuncs::leafPWM(two[0], rates.alphabet, C), child = TreeAlignFuncs::leafPWM(two[1], rates.alphabet, C);
  vguard<SeqIdx> xPos(parent.size() + 1), yPos(child.size() + 1);
  for (size_t k = 0; k < xPos.size(); ++k) xPos[k] = (SeqIdx)k;
  for (size_t k = 0; k < yPos.size(); ++k) yPos[k] = (SeqIdx)k;
  const GuideAlignmentEnvelope everywhere;
  const Refiner::BranchMatrix viterbi(rates, parent, child, atof(args[2]), everywhere, xPos, yPos, 0, 1);
  const Sampler::BranchMatrix forward(rates, parent, child, atof(args[2]), everywhere, xPos, yPos, 0, 1);
  printf("viterbi %a\nforward %a\n", viterbi.lpEnd, forward.lpEnd);
  const AlignPath best = viterbi.best();
  for (AlignRowIndex row = 0; row < 2; ++row) {
    size_t next = 0;
    for (bool here : best.at(row)) putchar(here ? two[row].seq[next++] : '-');
    putchar('\n');
  }
  return 0;
}

int siblingPair(int nArgs, char** args) {
  const vguard<FastSeq> two = readFastSeqs(args[0]);
  Require(two.size() == 2, "Sequence file must have exactly two sequences");
  RateModel rates;
  rates.readFile(args[1]);
  const double tl = atof(args[2]), tr = atof(args[3]);
  const int C = rates.components();
  const auto left = TreeAlignFuncs::leafPWM(two[0], rates.alphabet, C), right = TreeAlignFuncs::leafPWM(two[1], rates.alphabet, C);
  vguard<SeqIdx> xPos(left.size() + 1), yPos(right.size() + 1);
  for (size_t k = 0; k < xPos.size(); ++k) xPos[k] = (SeqIdx)k;
  for (size_t k = 0; k < yPos.size(); ++k) yPos[k] = (SeqIdx)k;
  // the guide of a band: the two sequences side by side without gaps, the longer one's tail unmatched
  AlignPath diagonal;
  const size_t width = std::max(left.size(), right.size());
  for (size_t col = 0; col < width; ++col) {
    diagonal[0].push_back(col < left.size());
    diagonal[1].push_back(col < right.size());
  }
  const GuideAlignmentEnvelope everywhere, banded(diagonal, 0, 1, nArgs > 4 ? atoi(args[4]) : 10);
  const GuideAlignmentEnvelope& chosen = nArgs > 4 ? banded : everywhere;
  const Sampler::SiblingMatrix matrix(rates, left, right, tl, tr, chosen, xPos, yPos, 0, 1, 2);
  printf("lpEnd %a\n", matrix.lpEnd);
  Sampler::SiblingMatrix::random_engine generator(20);
  const AlignPath path = matrix.sample(generator);
  for (AlignRowIndex row = 0; row < 3; ++row) {
    size_t next = 0;
    for (bool here : path.at(row)) putchar(!here ? '-' : (row < 2 ? two[row].seq[next++] : '*'));
    putchar('\n');
  }
  printf("logPostProb %a\n", matrix.logPostProb(path));
  const auto parent = matrix.parentSeq(path);
  for (size_t pos = 0; pos < parent.size() && pos < 3; ++pos) {
    printf("parent %zu", pos);
    for (const auto& cpt : parent[pos])
      for (double v : cpt) printf(" %a", v);
    printf("\n");
  }
  // two envelopes in one device batch against two single fills
  typedef Sampler::SiblingMatrix::Args Args;
  const vguard<Args> both = {Args{&left, &right, tl, tr, &everywhere, &xPos, &yPos, 0, 1, 2}, Args{&left, &right, tl, tr, &banded, &xPos, &yPos, 0, 1, 2}};
  const auto batch = Sampler::SiblingMatrix::fillBatch(rates, both);
  const Sampler::SiblingMatrix single0(rates, left, right, tl, tr, everywhere, xPos, yPos, 0, 1, 2), single1(rates, left, right, tl, tr, banded, xPos, yPos, 0, 1, 2);
  const Sampler::SiblingMatrix* singles[2] = {&single0, &single1};
  size_t different = 0;
  for (int k = 0; k < 2; ++k)
    for (SeqIdx i = 0; i < singles[k]->xSize; ++i)
      for (SeqIdx j = 0; j < singles[k]->ySize; ++j)
        for (unsigned s = 0; s < 11; ++s) {
          const double a = batch[k]->cell(i, j, s), b = singles[k]->cell(i, j, s);
          if (memcmp(&a, &b, sizeof a) != 0) ++different;
        }
  printf("fillBatch lpEnd %a %a single %a %a cells that differ %zu\n", batch[0]->lpEnd, batch[1]->lpEnd, single0.lpEnd, single1.lpEnd, different);
  return 0;
}

void printRows(const AlignPath& path, const vguard<FastSeq>& two, AlignRowIndex rows) {
  for (AlignRowIndex row = 0; row < rows; ++row) {
    size_t next = 0;
    for (bool here : path.at(row)) putchar(!here ? '-' : (row < 2 ? two[row].seq[next++] : '*'));
    putchar('\n');
  }
}

int pairWalks(int nArgs, char** args) {
  const vguard<FastSeq> two = readFastSeqs(args[0]);
  Require(two.size() == 2, "Sequence file must have exactly two sequences");
  RateModel rates;
  rates.readFile(args[1]);
  const double tl = atof(args[2]), tr = atof(args[3]);
  const int C = rates.components();
  const auto left = TreeAlignFuncs::leafPWM(two[0], rates.alphabet, C), right = TreeAlignFuncs::leafPWM(two[1], rates.alphabet, C);
  vguard<SeqIdx> xPos(left.size() + 1), yPos(right.size() + 1);
  for (size_t k = 0; k < xPos.size(); ++k) xPos[k] = (SeqIdx)k;
  for (size_t k = 0; k < yPos.size(); ++k) yPos[k] = (SeqIdx)k;
  AlignPath diagonal;
  const size_t width = std::max(left.size(), right.size());
  for (size_t col = 0; col < width; ++col) {
    diagonal[0].push_back(col < left.size());
    diagonal[1].push_back(col < right.size());
  }
  const GuideAlignmentEnvelope everywhere, banded(diagonal, 0, 1, nArgs > 4 ? atoi(args[4]) : 10);
  const GuideAlignmentEnvelope& chosen = nArgs > 4 ? banded : everywhere;
  typedef Sampler::SiblingMatrix::random_engine Engine;
  {
    const Sampler::SiblingMatrix matrix(rates, left, right, tl, tr, chosen, xPos, yPos, 0, 1, 2);
    Engine generator(20);
    const AlignPath path = matrix.sample(generator);
    printf("sibling lpEnd %a\n", matrix.lpEnd);
    printRows(path, two, 3);
    printf("sibling logPostProb %a\nsibling next word %lu\n", matrix.logPostProb(path), (unsigned long)generator());
  }
  {
    const Sampler::BranchMatrix forward(rates, left, right, tl, chosen, xPos, yPos, 0, 1);
    Engine generator(21);
    const AlignPath path = forward.sample(generator);
    printf("branch lpEnd %a\n", forward.lpEnd);
    printRows(path, two, 2);
    printf("branch logPostProb %a\nbranch next word %lu\n", forward.logPostProb(path), (unsigned long)generator());
    const Refiner::BranchMatrix viterbi(rates, left, right, tl, chosen, xPos, yPos, 0, 1);
    printf("viterbi lpEnd %a\n", viterbi.lpEnd);
    printRows(viterbi.best(), two, 2);
  }
  {
    // two envelopes filled in one device batch and sampled in one launch, against two single matrices, generator for generator
    typedef Sampler::SiblingMatrix::Args Args;
    const vguard<Args> both = {Args{&left, &right, tl, tr, &everywhere, &xPos, &yPos, 0, 1, 2}, Args{&left, &right, tl, tr, &banded, &xPos, &yPos, 0, 1, 2}};
    const auto batch = Sampler::SiblingMatrix::fillBatch(rates, both);
    Engine g0(30), g1(31), h0(30), h1(31);
    const vguard<AlignPath> together = Sampler::SiblingMatrix::sampleBatch({batch[0].get(), batch[1].get()}, {&g0, &g1});
    const Sampler::SiblingMatrix single0(rates, left, right, tl, tr, everywhere, xPos, yPos, 0, 1, 2), single1(rates, left, right, tl, tr, banded, xPos, yPos, 0, 1, 2);
    const bool same = together[0] == single0.sample(h0) && together[1] == single1.sample(h1) && g0 == h0 && g1 == h1;
    printf("sampleBatch equals single samples: %s\n", same ? "yes" : "no");
    printRows(together[1], two, 3);
  }
  printf("dense matrix reads: %ld\n", detail::denseMatrixReads());
  return 0;
}

int walkTiming(int nArgs, char** args) {
  const vguard<FastSeq> two = readFastSeqs(args[0]);
  Require(two.size() == 2, "Sequence file must have exactly two sequences");
  RateModel rates;
  rates.readFile(args[1]);
  const double tl = atof(args[2]), tr = atof(args[3]);
  const int n = atoi(args[4]), C = rates.components();
  Require(n >= 1, "At least one matrix");
  const auto left = TreeAlignFuncs::leafPWM(two[0], rates.alphabet, C), right = TreeAlignFuncs::leafPWM(two[1], rates.alphabet, C);
  vguard<SeqIdx> xPos(left.size() + 1), yPos(right.size() + 1);
  for (size_t k = 0; k < xPos.size(); ++k) xPos[k] = (SeqIdx)k;
  for (size_t k = 0; k < yPos.size(); ++k) yPos[k] = (SeqIdx)k;
  AlignPath diagonal;
  for (size_t col = 0; col < std::max(left.size(), right.size()); ++col) {
    diagonal[0].push_back(col < left.size());
    diagonal[1].push_back(col < right.size());
  }
  const GuideAlignmentEnvelope everywhere, banded(diagonal, 0, 1, nArgs > 5 ? atoi(args[5]) : 10);
  const GuideAlignmentEnvelope& chosen = nArgs > 5 ? banded : everywhere;
  typedef Sampler::SiblingMatrix SM;
  typedef std::chrono::steady_clock Clock;
  auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const vguard<SM::Args> args1((size_t)n, SM::Args{&left, &right, tl, tr, &chosen, &xPos, &yPos, 0, 1, 2});
  for (int rep = 0; rep < 4; ++rep) {        // the first repetition warms up
    const auto t0 = Clock::now();
    const auto batch = SM::fillBatch(rates, args1);
    const auto t1 = Clock::now();
    if (detail::hostWalks())
      for (const auto& m : batch) (void)m->cell(0, 0, 0);       // the dense copy a host walk needs before it can start
    const auto t2 = Clock::now();
    vguard<SM::random_engine> engines;
    vguard<const SM*> matrices;
    vguard<SM::random_engine*> generators;
    for (int k = 0; k < n; ++k) engines.emplace_back(100 + k);
    for (int k = 0; k < n; ++k) { matrices.push_back(batch[k].get()); generators.push_back(&engines[k]); }
    const vguard<AlignPath> paths = SM::sampleBatch(matrices, generators);
    const auto t3 = Clock::now();
    double total = 0;
    for (int k = 0; k < n; ++k) total += batch[k]->logPostProb(paths[k]);
    const auto t4 = Clock::now();
    printf("%s %d matrices of %zu x %zu: fillBatch %.2f ms, dense copies %.2f ms, sampleBatch %.2f ms, logPostProb %.2f ms; columns of "
           "the first alignment %zu, sum of logPostProb %.6f, dense matrix reads %ld\n", rep ? "run" : "warm-up", n, left.size(), right.size(),
           ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), (size_t)alignPathColumns(paths[0]), total, detail::denseMatrixReads());
  }
  return 0;
}

// distances <alignfile> <modelfile> [max iterations [host pairs]]: RateModel::expectedSubstitutionRate and distanceMatrix over
// the rows of a gapped alignment as hex floats ("rate <hex>", then "d <i> <j> <hex> <%.9g>" per pair).  With `host pairs` only
// that many pairs, in the matrix's order, through mlDistance on the host, and "hostms <ms>": one core's time for them.
int distances(int nArgs, char** args) {
  const vguard<FastSeq> gapped = readFastSeqs(args[0]);
  RateModel rates;
  rates.readFile(args[1]);
  const int maxIterations = nArgs > 2 ? atoi(args[2]) : DefaultDistanceMatrixIterations;
  printf("rate %a\n", rates.expectedSubstitutionRate());
  if (nArgs > 3) {
    long left = atol(args[3]);
    const double t0 = wallSeconds();
    vguard<string> lines;
    for (size_t i = 0; i + 1 < gapped.size() && left > 0; ++i)
      for (size_t j = i + 1; j < gapped.size() && left > 0; ++j, --left) {
        const double d = rates.mlDistance(gapped[i], gapped[j], maxIterations);
        char text[96];
        snprintf(text, sizeof text, "d %zu %zu %a %.9g", i, j, d, d);
        lines.push_back(text);
      }
    const double ms = 1e3 * (wallSeconds() - t0);
    for (const auto& l : lines) puts(l.c_str());
    printf("hostms %.3f\n", ms);
    return 0;
  }
  const auto dist = rates.distanceMatrix(gapped, maxIterations);
  for (size_t i = 0; i + 1 < gapped.size(); ++i)
    for (size_t j = i + 1; j < gapped.size(); ++j) printf("d %zu %zu %a %.9g\n", i, j, dist[i][j], dist[i][j]);
  return 0;
}

// treemoves <rows.fa> <tree.nh> <model.json> <steps> <seed>: a tree-height chain on a fixed alignment (one gapped row per tree
// node, named as the Newick string names it).  Prints "parts <tree> <root> <indels> <substitutions>" of the initial history as
// hex floats; per step "step <k> <type> <node or -1> <logAcceptProb> <accepted> <logJacobian> <new log-likelihood>" and
// "proposed <branch length of every node>" (hex floats); then "final <branch lengths>", "newick <tree>" and moveStats' counts
// as "moves <type> <proposed> <accepted>".
int treeMoves(int, char** args) {
  vguard<FastSeq> rows = readFastSeqs(args[0]);
  std::ifstream treeFile(args[1]);
  Require(treeFile.good(), "Couldn't open %s", args[1]);
  std::stringstream newick;
  newick << treeFile.rdbuf();
  RateModel rates;
  rates.readFile(args[2]);
  const unsigned steps = (unsigned)atoi(args[3]);
  TreeAlignFuncs::History history;
  history.tree = ReconTree::parse(newick.str());
  for (TreeNodeIndex n = 0; n < history.tree.nodes(); ++n) {
    const auto row = std::find_if(rows.begin(), rows.end(), [&](const FastSeq& fs) { return fs.name == history.tree.nodeName[n]; });
    Require(row != rows.end(), "No row for tree node %s", history.tree.nodeName[n].c_str());
    history.gapped.push_back(*row);
  }
  const SimpleTreePrior prior;
  vguard<Sampler> samplers(1, Sampler(rates, prior));
  Sampler& sampler = samplers[0];
  sampler.keepMoveLog = true;
  sampler.initialize(history, "treemoves");
  sampler.fixAlignment();
  printf("parts %a %a %a %a\n", sampler.currentTerms[0], sampler.currentTerms[1], sampler.currentTerms[2], sampler.currentTerms[3]);
  printf("whole %a\n", TreeAlignFuncs::logLikelihood(prior, rates, history));
  Sampler::random_engine generator((unsigned)atoi(args[4]));
  Sampler::run(samplers, generator, steps);
  for (size_t k = 0; k < sampler.moveLog.size(); ++k) {
    const Sampler::Move& m = sampler.moveLog[k];
    string type = Sampler::Move::typeName(m.type);
    std::replace(type.begin(), type.end(), ' ', '_');
    printf("step %zu %s %d %a %d %a %a\nproposed", k, type.c_str(), m.node, m.logAcceptProb, (int)(m.comment == "accepted"), m.logJacobian, m.newLogLikelihood);
    for (double d : m.newHistory.tree.branchLen) printf(" %a", d);
    printf("\n");
  }
  printf("final");
  for (double d : sampler.currentHistory.tree.branchLen) printf(" %a", d);
  printf("\nnewick %s\ncurrent %a best %a\n", sampler.currentHistory.tree.toString().c_str(), sampler.currentLogLikelihood, sampler.bestLogLikelihood);
  for (int t = 0; t < (int)Sampler::Move::TotalMoveTypes; ++t) {
    string type = Sampler::Move::typeName((Sampler::Move::Type)t);
    std::replace(type.begin(), type.end(), ' ', '_');
    printf("moves %s %d %d\n", type.c_str(), sampler.movesProposed[t], sampler.movesAccepted[t]);
  }
  std::cerr << sampler.moveStats();
  return 0;
}

// condpwm <rows.fa> <tree.nh> <model.json> <node> <normalize>: what BranchAlignMove does first with the branch above <node>
// (src/sampler.cpp:582-594).  Prints "lengths <parent> <node>"; "parent <pos>" and "node <pos>" with the C x A entries of
// every row of the two profiles (hex floats); "lpEnd" of an unbanded Sampler::BranchMatrix built from them; a seeded sample
// as two rows of '*' and '-'; its "logPostProb".  <node> given as prune:<k> calls getConditionalPWMs with the map
// PruneAndRegraftMove builds for node k (src/sampler.cpp:843-848): it aborts, those moves are not built.  With a sixth
// argument `device` the matrix is built from one resident history without the profiles passing through the host
// (hx_history_branch_batch_create); the lines printed are the same.
int conditionalProfiles(int nArgs, char** args) {
  vguard<FastSeq> rows = readFastSeqs(args[0]);
  std::ifstream treeFile(args[1]);
  Require(treeFile.good(), "Couldn't open %s", args[1]);
  std::stringstream newick;
  newick << treeFile.rdbuf();
  RateModel rates;
  rates.readFile(args[2]);
  TreeAlignFuncs::History history;
  history.tree = ReconTree::parse(newick.str());
  const ReconTree& tree = history.tree;
  for (TreeNodeIndex n = 0; n < tree.nodes(); ++n) {
    const auto row = std::find_if(rows.begin(), rows.end(), [&](const FastSeq& fs) { return fs.name == tree.nodeName[n]; });
    Require(row != rows.end(), "No row for tree node %s", tree.nodeName[n].c_str());
    history.gapped.push_back(*row);
  }
  const bool prune = strncmp(args[3], "prune:", 6) == 0;
  Require(nArgs <= 5 || (strcmp(args[5], "device") == 0 && !prune), "The sixth argument is `device`, and not with prune:");
  const TreeNodeIndex node = (TreeNodeIndex)atoi(args[3] + (prune ? 6 : 0));
  Require(node >= 0 && node < tree.root(), "Node %d has no branch", (int)node);
  const TreeNodeIndex parent = tree.parent[node];
  const bool normalize = atoi(args[4]) != 0;
  map<TreeNodeIndex, TreeNodeIndex> exclude;
  const set<TreeNodeIndex> unused;
  if (prune) {
    exclude[node] = -1;
    for (TreeNodeIndex sib : tree.child[parent])
      if (sib != node) exclude[sib] = parent;
    if (tree.parent[parent] >= 0) exclude[tree.parent[parent]] = parent;
    (void)TreeAlignFuncs::getConditionalPWMs(rates, tree, history.gapped, exclude, unused, unused, normalize);
    return 0;
  }
  const bool device = nArgs > 5;
  exclude[node] = parent;
  exclude[parent] = node;
  std::shared_ptr<hx_history> resident;
  if (device) resident.reset(TreeAlignFuncs::residentHistory(rates, history), hx_history_destroy);
  const auto pwms = device ? TreeAlignFuncs::getConditionalPWMs(resident.get(), rates, tree, exclude, normalize)
                           : TreeAlignFuncs::getConditionalPWMs(rates, tree, history.gapped, exclude, unused, unused, normalize);
  const TreeAlignFuncs::PosWeightMatrix none;
  const auto& pSeq = pwms.count(parent) ? pwms.at(parent) : none;
  const auto& nSeq = pwms.count(node) ? pwms.at(node) : none;
  printf("lengths %zu %zu\n", pSeq.size(), nSeq.size());
  for (int which = 0; which < 2; ++which) {
    const auto& seq = which ? nSeq : pSeq;
    for (size_t pos = 0; pos < seq.size(); ++pos) {
      printf("%s %zu", which ? "node" : "parent", pos);
      for (const auto& cpt : seq[pos])
        for (double v : cpt) printf(" %a", v);
      printf("\n");
    }
  }
  vguard<SeqIdx> xPos(pSeq.size() + 1), yPos(nSeq.size() + 1);
  for (size_t k = 0; k < xPos.size(); ++k) xPos[k] = (SeqIdx)k;
  for (size_t k = 0; k < yPos.size(); ++k) yPos[k] = (SeqIdx)k;
  const GuideAlignmentEnvelope everywhere;
  const Sampler::BranchMatrix matrix = device ? Sampler::BranchMatrix(resident.get(), rates, tree, node, tree.branchLength(node), everywhere, xPos, yPos, normalize)
                                              : Sampler::BranchMatrix(rates, pSeq, nSeq, tree.branchLength(node), everywhere, xPos, yPos, 0, 1);
  printf("lpEnd %a\n", matrix.lpEnd);
  Sampler::BranchMatrix::random_engine generator(22);
  const AlignPath path = matrix.sample(generator);
  for (AlignRowIndex row : {matrix.xRow, matrix.yRow}) {
    for (bool here : path.at(row)) putchar(here ? '*' : '-');
    putchar('\n');
  }
  printf("logPostProb %a\n", matrix.logPostProb(path));
  return 0;
}

const Command commands[] = {
    {"logsumexp", 0, 1, "[-slow|-fast]", lseGrid},
    {"seqprofile", 2, 2, "<alphabet> <sequence>", leafProfileJson},
    {"quickalign", 3, 3, "<seqfile> <modelfile> <time>", guidePair},
    {"expm", 2, 2, "<modelfile> <time>", substitutionMatrix},
    {"expmtime", 3, 3, "<modelfile> <time> <calls>", substitutionMatrixTime},
    {"branch", 3, 3, "<seqfile> <modelfile> <time>", branchPair},
    {"sibling", 4, 5, "<seqfile> <modelfile> <left time> <right time> [band]", siblingPair},
    {"walks", 4, 5, "<seqfile> <modelfile> <left time> <right time> [band]", pairWalks},
    {"walktime", 5, 6, "<seqfile> <modelfile> <left time> <right time> <matrices> [band]", walkTiming},
    {"distances", 2, 4, "<alignfile> <modelfile> [max iterations [host pairs]]", distances},
    {"treemoves", 5, 5, "<rows.fa> <tree.nh> <modelfile> <steps> <seed>", treeMoves},
    {"condpwm", 5, 6, "<rows.fa> <tree.nh> <modelfile> <node | prune:node> <normalize> [device]", conditionalProfiles},
};

}  // namespace

int main(int argc, char** argv) {
  const Command* chosen = nullptr;
  for (const Command& c : commands)
    if (argc > 1 && strcmp(argv[1], c.name) == 0) chosen = &c;
  const int nArgs = argc - 2;
  if (!chosen || nArgs < chosen->minArgs || nArgs > chosen->maxArgs || chosen->run(nArgs, argv + 2) != 0) {
    std::cout << "Usage:\n";
    for (const Command& c : commands)
      if (!chosen || chosen == &c) std::cout << "  " << argv[0] << ' ' << c.name << ' ' << c.usage << "\n";
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
