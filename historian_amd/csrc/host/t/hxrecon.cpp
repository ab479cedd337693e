// Progressive reconstruction driver over the GPU-backed mirror.  Input is one small job file per family (the
// reference's own readers for Newick / Stockholm / guide files are outside this build's scope):
//   model <rate model json>
//   seqs <fasta of ungapped leaf sequences>
//   guide <fasta of the gapped guide alignment>      (optional)
//   band <n> | samples <n> | maxstates <n> | seed <n> | posterior <minPostProb> | batch <0|1>   (optional)
//   count indel                      (optional: `historian count` with fixed substitution rates - no root traceback; per
//                                     family "indelCounts <key> <hex> <%.9g>" for ins del insExt delExt insTime delTime lp,
//                                     then the same summed over families as "indelCountsTotal <key> ...")
//   fit <maxIter> [<minImprovement>] (optional: `historian fit -fixsubrates`, EM over the indel rates with Laplace pseudocounts;
//                                     prints "em <iteration> <hex> <%.9g>" per iteration, then insRate delRate insExtProb delExtProb)
//   ancseq | ancprob [<minProb>]     (optional: `historian recon -ancseq`, `-ancprob` - after a family's rows, "anc <node> <name>
//                                     <row>" for every row, its wildcards replaced by the most probable residue; with
//                                     ancprob, which implies ancseq, also "pp <node> <column, 1-based> <char> <hex> <%.6f>" for
//                                     every residue of a wildcard cell with a posterior of minProb, default .01, or more)
//   tree <N>   followed by N lines:  <parent index or -1> <branch length> <name>   (post-order, root last)
//   buildtree nj|upgma [jc]          (optional, instead of a tree block; needs guide: the tree is estimated from the guide's
//                                     rows by neighbour joining or UPGMA over the maximum-likelihood distance matrix, or with
//                                     jc over the Jukes-Cantor estimates - `historian recon -nj`, `-upgma`, `-jc`; an internal
//                                     node is printed under the name node<index>)
// Output: final Forward / trace log-likelihoods as hex floats, the band used per node, and the
// gapped reconstruction (one row per tree node on the root path).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <list>
#include <sstream>
#include "../hx_host.h"
using namespace historian;

// one job file -> the reconstruction parameters (the first file's stand for all) and one family
static bool fitting = false;   // a `fit` key was read

static void printCounts(const char* tag, const IndelCounts& c) {
  const std::pair<const char*, double> v[7] = {{"ins", c.ins}, {"del", c.del}, {"insExt", c.insExt}, {"delExt", c.delExt},
                                               {"insTime", c.insTime}, {"delTime", c.delTime}, {"lp", c.lp}};
  for (const auto& kv : v) printf("%s %s %a %.9g\n", tag, kv.first, kv.second, kv.second);
  fflush(stdout);
}

static void readJob(const char* file, Reconstructor& recon, bool setParams, Reconstructor::Dataset& ds) {
  std::ifstream in(file);
  Require(in.good(), "Couldn't open %s", file);
  Reconstructor scratch;
  Reconstructor& r = setParams ? recon : scratch;
  string key, seqFile, guideFile, buildTree;
  bool buildTreeJC = false;
  while (in >> key) {
    if (key == "model") { string f; in >> f; if (setParams) r.model.readFile(f.c_str()); }
    else if (key == "seqs") in >> seqFile;
    else if (key == "guide") in >> guideFile;
    else if (key == "band") in >> r.maxDistanceFromGuide;
    else if (key == "samples") in >> r.profileSamples;
    else if (key == "maxstates") in >> r.profileMaxStates;
    else if (key == "seed") in >> r.rndSeed;
    else if (key == "batch") { int b; in >> b; r.batchReadyNodes = b != 0; }
    else if (key == "posterior") { in >> r.minPostProb; r.usePosteriorsForProfile = true; }
    else if (key == "count") {
      string what; in >> what;
      Require(what == "indel", "Only indel counts are supported (count %s in %s)", what.c_str(), file);
      r.accumulateIndelCounts = true; r.reconstructRoot = false;
    } else if (key == "fit") {
      string rest; std::getline(in, rest);
      std::istringstream args(rest);
      Require((bool)(args >> r.maxEMIterations), "fit needs a maximum number of iterations in %s", file);
      double minInc;
      if (args >> minInc) r.minEMImprovement = minInc;
      r.accumulateIndelCounts = true; r.reconstructRoot = false; fitting = true;
    }
    else if (key == "ancseq") r.predictAncestralSequence = true;
    else if (key == "ancprob") {
      string rest; std::getline(in, rest);
      std::istringstream args(rest);
      double minProb;
      if (args >> minProb) r.ancestralSequenceMinProb = minProb;
      r.predictAncestralSequence = r.reportAncestralSequenceProbability = true;
    }
    else if (key == "buildtree") {
      string rest; std::getline(in, rest);
      std::istringstream args(rest);
      string jc;
      Require((bool)(args >> buildTree) && (buildTree == "nj" || buildTree == "upgma"), "buildtree needs nj or upgma in %s", file);
      if (args >> jc) { Require(jc == "jc", "Unknown buildtree option %s in %s", jc.c_str(), file); buildTreeJC = true; }
    }
    else if (key == "tree") {
      int n; in >> n;
      for (int k = 0; k < n; ++k) {
        int parent; double len; string name;
        in >> parent >> len >> name;
        ds.tree.addNode(parent, len, name);
      }
      ds.tree.finish();
    } else Fail("Unknown key %s in %s", key.c_str(), file);
  }
  if (ds.tree.nodes() == 0 && !buildTree.empty()) {
    Require(!guideFile.empty(), "buildtree needs a guide alignment in %s", file);
    recon.useUPGMA = buildTree == "upgma";
    recon.jukesCantorDistanceMatrix = buildTreeJC;
    recon.buildTree(ds, readFastSeqs(guideFile.c_str()));
    for (TreeNodeIndex n = 0; n < ds.tree.nodes(); ++n)
      if (!ds.tree.isLeaf(n) && ds.tree.nodeName[n].empty()) ds.tree.nodeName[n] = "node" + std::to_string(n);
  }
  map<string, string> ungapped, gapped;
  for (const auto& fs : readFastSeqs(seqFile.c_str())) ungapped[fs.name] = fs.seq;
  if (!guideFile.empty())
    for (const auto& fs : readFastSeqs(guideFile.c_str())) gapped[fs.name] = fs.seq;
  for (TreeNodeIndex n = 0; n < ds.tree.nodes(); ++n)
    if (ds.tree.isLeaf(n)) {
      const string& name = ds.tree.nodeName[n];
      Require(ungapped.count(name), "Can't find sequence for leaf node %s", name.c_str());
      FastSeq fs;
      fs.name = name;
      fs.seq = ungapped[name];
      ds.seqs[n] = fs;
      if (!guideFile.empty()) {
        Require(gapped.count(name), "Can't find guide row for leaf node %s", name.c_str());
        AlignRowPath row;
        for (char c : gapped[name]) row.push_back(!Alignment::isGap(c));
        ds.guide[n] = row;
      }
    }
  ds.prepareRecon();
}

static void printFamily(const Reconstructor::Dataset& ds) {
  printf("lpFinalFwd %a %.6f\n", ds.lpFinalFwd, ds.lpFinalFwd);
  printf("lpFinalTrace %a %.6f\n", ds.lpFinalTrace, ds.lpFinalTrace);
  for (const auto& nb : ds.bandUsed) printf("band %d %d\n", nb.first, nb.second);
  fflush(stdout);
  for (const auto& row_path : ds.path) {
    const TreeNodeIndex node = (TreeNodeIndex)row_path.first;
    std::cout << "row " << node << " " << ds.tree.nodeName[node] << " ";
    const bool leaf = ds.seqs.count(node) > 0;
    size_t k = 0;
    for (bool b : row_path.second) std::cout << (b ? (leaf ? ds.seqs.at(node).seq[k++] : Alignment::wildcardChar) : Alignment::gapChar);
    std::cout << "\n";
  }
  std::cout.flush();
  for (size_t r = 0; r < ds.gappedAncestralRecon.size(); ++r)
    std::cout << "anc " << r << " " << ds.tree.nodeName[r] << " " << ds.gappedAncestralRecon[r].seq << "\n";
  std::cout.flush();
  for (const auto& row : ds.gappedAncestralReconPostProb)
    for (const auto& col : row.second)
      for (const auto& cp : col.second) printf("pp %zu %zu %c %a %.6f\n", row.first, col.first + 1, cp.first, cp.second, cp.second);
  fflush(stdout);
}

// hxrecon [-devices d0,d1,...] <jobfile> [<jobfile> ...]
// Several job files = several families (the first file's parameters apply to all); with -devices they are farmed over
// those devices, one host thread each (an ordinal may be repeated: two threads sharing a device).  Output per family as
// for a single one, preceded by a line "family <k>" when there are several.
int main(int argc, char** argv) {
  vguard<int> devices;
  int first = 1;
  if (argc > 2 && string(argv[1]) == "-devices") {
    std::stringstream list(argv[2]);
    string tok;
    while (std::getline(list, tok, ',')) devices.push_back(atoi(tok.c_str()));
    first = 3;
  }
  if (argc <= first) {
    std::cout << "Usage: " << argv[0] << " [-devices d0,d1,...] <jobfile> [<jobfile> ...]\n";
    exit(EXIT_FAILURE);
  }
  Reconstructor recon;
  recon.devices = devices;
  std::list<Reconstructor::Dataset> families;
  vguard<Reconstructor::Dataset*> all;
  for (int k = first; k < argc; ++k) {
    families.emplace_back();
    readJob(argv[k], recon, k == first, families.back());
    all.push_back(&families.back());
  }
  const double t0 = wallSeconds();
  if (fitting) {
    recon.fit(all);
    for (size_t k = 0; k < recon.emLogLikelihood.size(); ++k)
      printf("em %zu %a %.9g\n", k + 1, recon.emLogLikelihood[k], recon.emLogLikelihood[k]);
    const std::pair<const char*, double> rates[4] = {{"insRate", recon.model.insRate}, {"delRate", recon.model.delRate},
                                                     {"insExtProb", recon.model.insExtProb}, {"delExtProb", recon.model.delExtProb}};
    for (const auto& kv : rates) printf("%s %a %.9g\n", kv.first, kv.second, kv.second);
    fflush(stdout);
    exit(EXIT_SUCCESS);
  }
  if (recon.accumulateIndelCounts) recon.countAll(all);
  else if (all.size() == 1) recon.reconstruct(*all[0]);
  else recon.reconstructAll(all);
  recon.predictAllAncestors(all);
  if (getenv("HX_TIMING")) {
    const double total = wallSeconds() - t0;
    const FillTiming& f = fillTiming;
    fprintf(stderr, "timing: reconstruct %.3f s = one-off HIP/device initialisation %.3f s + %.3f s; %ld fills over %lld lattice cells: "
                    "flatten+upload %.3f s, forward (launch..lpEnd) %.3f s of which fill kernels %.3f s, backward (launch..lpStart) %.3f s, matrix D2H %.3f s in %ld reads (page-locking beyond the warmed buffers: %.3f s for %ld buffers, while a fill runs where the size is known by then), "
                    "device best-path tracebacks %.3f s in %ld calls, cell gathers %.3f s in %ld calls; sorting sampled cells %.3f s, keeping their values %.3f s; envelopes %.3f s, prepared vectors (read + lpAbsorb) %.3f s; host traceback/profile building/other %.3f s\n",
            total, f.deviceInit, total - f.deviceInit, f.fills, f.cells, f.flattenAndUpload, f.forwardWait, f.forwardKernel, f.backwardWait, f.readMatrix,
            f.matrixReads, f.pinnedAlloc, f.pinnedAllocs, f.deviceTrace, f.deviceTraces, f.cellGather, f.cellGathers, f.cellSets, f.retain, f.construct, f.readPrepared,
            total - f.deviceInit - f.flattenAndUpload - f.forwardWait - f.readMatrix - f.backwardWait - f.deviceTrace - f.cellGather);    fprintf(stderr, "timing: best traces taken again from an exact-policy fill because the walk met a near tie (HX_TIE_REFILL=1): %ld, %.3f s\n",
            f.tieRefills, f.tieRefill);
  }
  for (size_t k = 0; k < all.size(); ++k) {
    if (all.size() > 1) { printf("family %zu\n", k); fflush(stdout); }
    printFamily(*all[k]);
    if (recon.accumulateIndelCounts) printCounts("indelCounts", all[k]->indelCounts);
  }
  if (recon.accumulateIndelCounts) printCounts("indelCountsTotal", recon.dataCounts);
  exit(EXIT_SUCCESS);
}
