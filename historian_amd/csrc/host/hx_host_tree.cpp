// Tree estimation between the guide alignment and the progressive pass: RateModel::distanceMatrix (reference
// src/model.cpp:336-347, 506-655), Tree::buildByNeighborJoining / buildByUPGMA / toString (src/tree.cpp:56-102, 191-212,
// 240-462) and Reconstructor::buildTree (src/recon.cpp:732-743).
//
// The distance matrix runs on the device (hx_distance_matrix: one wavefront per pair of rows).  HX_HOST_DISTANCES=1, or an
// alphabet of more than 32 symbols, takes the host restatement below instead: the reference's control flow with GSL's
// golden-section step restated from its published source (min/golden.c, min/convergence.c), over the restated
// exp(R t) of getSubProbMatrix.  tests/tree_ref.py is the same restatement in Python; the two agree bit for bit.
// Neighbour joining and UPGMA are O(N^3) scalar work over a matrix that is on the host already, and stay here.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../../include/historian_hip.h"
#include "hx_host.h"

namespace historian {

double RateModel::expectedSubstitutionRate() const {
  double R = 0;
  for (int c = 0; c < components(); ++c) {
    const Vec eqm = getEqmProbVector(subRate[c]);
    for (size_t i = 0; i < alphabetSize(); ++i)
      for (size_t j = 0; j < alphabetSize(); ++j)
        if (i != j) R += cptWeight[c] * eqm[i] * subRate[c][i][j];
  }
  return R;
}

namespace {

// src/model.h: DistanceMatrixParams
struct DistanceMatrixParams {
  const map<std::pair<AlphTok, AlphTok>, int>& pairCount;
  const RateModel& model;
  DistanceMatrixParams(const map<std::pair<AlphTok, AlphTok>, int>& counts, const RateModel& rates) : pairCount(counts), model(rates) {}

  double negLogLike(double t) const {                 // distanceMatrixNegLogLike, src/model.cpp:551-564
    const vguard<Mat> sub = model.getSubProbMatrix(t);
    double ll = 0;
    for (const auto& pc : pairCount) {
      double p = 0;
      for (int c = 0; c < model.components(); ++c) p += model.cptWeight[c] * sub[c][pc.first.first][pc.first.second];
      ll += log(p) * (double)pc.second;
    }
    return -ll;
  }

  double tJC() const {                                // src/model.cpp:570-582
    int same = 0, diff = 0;
    for (const auto& pc : pairCount)
      if (pc.first.first == pc.first.second) same += pc.second;
      else diff += pc.second;
    const double pDiff = diff / (double)(same + diff);
    const double A = (double)model.alphabetSize();
    if (pDiff >= (A - 1) / A) return std::numeric_limits<double>::infinity();
    return -((A - 1) / A) * log(1 - (A / (A - 1)) * pDiff) / model.expectedSubstitutionRate();
  }

  double tML(int maxIterations) const {               // src/model.cpp:584-655
    const double tMin = 1e-9, tMax = 10;
    const double tjc = std::min(tMax, std::max(tMin, tJC()));
    if (maxIterations <= 0) return tjc;
    double t;
    const double tLower = std::min(tMin, tjc / 2), tUpper = std::max(tMax, tjc * 2);
    const double llLower = negLogLike(tLower), llUpper = negLogLike(tUpper);
    const double lljc = negLogLike(tjc);
    double fMin;
    if (lljc < llLower && lljc < llUpper) {
      t = tjc;
      fMin = lljc;
    } else {
      bool foundGuess = false;
      double tScanLower = tLower, tScanUpper = tUpper;
      const double nScanSteps = 4;
      fMin = t = 0;
      while (!foundGuess && tScanUpper - tScanLower > tLower) {
        const double step = (tScanUpper - tScanLower) / nScanSteps;
        for (double x = tScanLower; x < tScanUpper && !foundGuess; x += step) {
          const double ll = negLogLike(x);
          if (ll < llLower && ll < llUpper) {
            foundGuess = true;
            t = x;
            fMin = ll;
          }
        }
        if (!foundGuess) {
          if (llLower < llUpper) tScanUpper = (tScanLower + tScanUpper) / 2;
          else tScanLower = (tScanLower + tScanUpper) / 2;
        }
      }
      if (!foundGuess) return llLower < llUpper ? tLower : tUpper;
    }
    // gsl_min_fminimizer_set(s, &F, t, tLower, tUpper), then per iteration gsl_min_fminimizer_iterate (goldensection: the
    // trial point 0.3819660 into the larger sub-interval; a new minimum does not move the bracket; GSL_FAILURE ignored)
    // and gsl_min_test_interval(a, b, 0, .01)
    const double golden = 0.3819660;
    double xMin = t, xLower = tLower, xUpper = tUpper;
    for (int iter = 0; iter < maxIterations; ++iter) {
      const double wLower = xMin - xLower, wUpper = xUpper - xMin;
      const double xNew = xMin + golden * ((wUpper > wLower) ? wUpper : -wLower);
      const double fNew = negLogLike(xNew);
      if (fNew < fMin) { xMin = xNew; fMin = fNew; }
      else if (xNew < xMin && fNew > fMin) xLower = xNew;
      else if (xNew > xMin && fNew > fMin) xUpper = xNew;
      t = xMin;
      const double absLower = fabs(xLower), absUpper = fabs(xUpper);
      const double minAbs = ((xLower > 0. && xUpper > 0.) || (xLower < 0. && xUpper < 0.)) ? std::min(absLower, absUpper) : 0;
      if (fabs(xUpper - xLower) < .01 * minAbs) break;
    }
    return t;
  }
};

bool counted(char c) { return !Alignment::isGap(c) && !Alignment::isWildcard(c); }

bool hostDistances() {
  const char* e = getenv("HX_HOST_DISTANCES");
  return e && atoi(e) != 0;
}

// gsl_fcmp (GSL sys/fcmp.c, after Knuth): are the two within epsilon, relative to the larger one's binade?
int fcmp(double x1, double x2, double epsilon) {
  int exponent;
  frexp(fabs(x1) > fabs(x2) ? x1 : x2, &exponent);
  const double delta = ldexp(epsilon, exponent), difference = x1 - x2;
  return difference > delta ? 1 : difference < -delta ? -1 : 0;
}

// a tree in the order its builder made the nodes: leaves, then one node per join
struct JoinTree {
  vguard<TreeNodeIndex> parent;
  vguard<double> d;
  vguard<string> name;
  vguard<vguard<TreeNodeIndex>> child;
  explicit JoinTree(const vguard<string>& leaves) : parent(leaves.size(), -1), d(leaves.size(), -1.), name(leaves), child(leaves.size()) {}
  TreeNodeIndex nodes() const { return (TreeNodeIndex)parent.size(); }
  TreeNodeIndex join(TreeNodeIndex i, TreeNodeIndex j, double di, double dj) {
    const TreeNodeIndex k = nodes();
    parent.push_back(-1);
    d.push_back(-1.);
    name.push_back(string());
    child.push_back({i, j});
    parent[i] = parent[j] = k;
    d[i] = std::max(0., di);
    d[j] = std::max(0., dj);
    return k;
  }
};

// What Tree::parse(toString()) leaves: nodes in the Newick reader's order (post-order, children left to right, root
// last), every branch length as its default-format text reads back, raised to the minimum (src/tree.cpp:27-28).
TreeNodeIndex reindex(const JoinTree& jt, TreeNodeIndex node, ReconTree& out) {
  vguard<TreeNodeIndex> kids;
  for (TreeNodeIndex c : jt.child[node]) kids.push_back(reindex(jt, c, out));
  double len = 0;                                     // the root: no branch above it
  if (jt.d[node] >= 0) {
    char text[64];
    snprintf(text, sizeof text, "%g", jt.d[node]);
    len = std::max(strtod(text, nullptr), ReconTree::minBranchLength);
  }
  const TreeNodeIndex slot = out.nodes();
  out.addNode(-1, len, jt.name[node]);
  for (TreeNodeIndex k : kids) out.parent[k] = slot;
  return slot;
}

void adopt(const JoinTree& jt, ReconTree& tree) {
  tree = ReconTree();
  reindex(jt, jt.nodes() - 1, tree);
  tree.finish();
}

string describe(const ReconTree& t, TreeNodeIndex n) {
  if (t.isLeaf(n)) return t.nodeName[n];
  string s = "(";
  for (size_t c = 0; c < t.child[n].size(); ++c) {
    const TreeNodeIndex k = t.child[n][c];
    if (c > 0) s += ",";
    s += describe(t, k);
    char text[64];                                    // Tree::branchLengthString: the stream's default format
    snprintf(text, sizeof text, ":%g", t.branchLen[k]);
    s += text;
  }
  return s + ")" + t.nodeName[n];
}

}  // namespace

double RateModel::mlDistance(const FastSeq& x, const FastSeq& y, int maxIterations) const {
  map<std::pair<AlphTok, AlphTok>, int> pairCount;
  Assert(x.length() == y.length(), "Sequences %s and %s have different lengths (%u, %u)", x.name.c_str(), y.name.c_str(),
         (unsigned)x.length(), (unsigned)y.length());
  for (size_t col = 0; col < x.seq.size(); ++col) {
    const char ci = x.seq[col], cj = y.seq[col];
    if (counted(ci) && counted(cj)) {
      const UnvalidatedAlphTok toki = tokenize(ci, alphabet), tokj = tokenize(cj, alphabet);
      if (toki >= 0 && tokj >= 0) ++pairCount[std::pair<AlphTok, AlphTok>((AlphTok)toki, (AlphTok)tokj)];
    }
  }
  return DistanceMatrixParams(pairCount, *this).tML(maxIterations);
}

vguard<vguard<double>> RateModel::distanceMatrix(const vguard<FastSeq>& gappedSeq, int maxIterations) const {
  const size_t n = gappedSeq.size();
  vguard<vguard<double>> dist(n, vguard<double>(n, 0.));
  if (n < 2) return dist;
  if (hostDistances() || alphabetSize() > 32) {
    for (size_t i = 0; i + 1 < n; ++i)
      for (size_t j = i + 1; j < n; ++j) dist[i][j] = dist[j][i] = mlDistance(gappedSeq[i], gappedSeq[j], maxIterations);
    return dist;
  }
  const size_t cols = gappedSeq[0].seq.size(), A = alphabetSize();
  vguard<int8_t> tokens(n * cols, (int8_t)-1);
  for (size_t r = 0; r < n; ++r) {
    Assert(gappedSeq[r].seq.size() == cols, "Sequences %s and %s have different lengths (%u, %u)", gappedSeq[0].name.c_str(),
           gappedSeq[r].name.c_str(), (unsigned)cols, (unsigned)gappedSeq[r].seq.size());
    for (size_t c = 0; c < cols; ++c)
      if (counted(gappedSeq[r].seq[c])) tokens[r * cols + c] = (int8_t)tokenize(gappedSeq[r].seq[c], alphabet);
  }
  vguard<double> rates((size_t)components() * A * A), flat(n * n);
  for (int c = 0; c < components(); ++c)
    for (size_t i = 0; i < A; ++i)
      for (size_t j = 0; j < A; ++j) rates[((size_t)c * A + i) * A + j] = subRate[c][i][j];
  hx_distance_model m;
  m.alph_size = (int32_t)A;
  m.n_components = components();
  m.sub_rate = rates.data();
  m.cpt_weight = cptWeight.data();
  m.expected_sub_rate = expectedSubstitutionRate();
  detail::ensureDevice();
  detail::check(hx_distance_matrix(&m, tokens.data(), (int32_t)n, (int64_t)cols, maxIterations, flat.data(), nullptr, nullptr),
                "hx_distance_matrix");
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) dist[i][j] = flat[i * n + j];
  return dist;
}

double ReconTree::minBranchLength = 1e-9;    // TREE_MIN_BRANCH_LEN

string ReconTree::toString() const { return describe(*this, root()) + ";"; }

bool ReconTree::isUltrametric(double epsilon) const {
  vguard<double> fromRoot(nodes(), 0.);
  for (TreeNodeIndex n = nodes() - 2; n >= 0; --n) fromRoot[n] = fromRoot[parent[n]] + std::max(branchLen[n], 0.);
  double minDist = std::numeric_limits<double>::infinity();
  for (TreeNodeIndex n = 0; n < nodes(); ++n)
    if (isLeaf(n)) minDist = std::min(minDist, fromRoot[n]);
  for (TreeNodeIndex n = 0; n < nodes(); ++n)
    if (isLeaf(n) && fcmp(fromRoot[n], minDist, epsilon) != 0) return false;
  return true;
}

void ReconTree::buildByNeighborJoining(const vguard<string>& names, const vguard<vguard<double>>& distanceMatrix) {
  Assert(names.size() >= 2, "Fewer than 2 nodes; can't make a binary tree");
  vguard<vguard<double>> dist = distanceMatrix;
  JoinTree jt(names);
  set<TreeNodeIndex> activeNodes;
  for (TreeNodeIndex n = 0; n < (TreeNodeIndex)names.size(); ++n) activeNodes.insert(n);
  vguard<double> avgDist;
  while (true) {
    const int nActiveNodes = (int)activeNodes.size();
    if (nActiveNodes == 2) break;
    Assert(nActiveNodes > 2, "Fewer than 2 nodes left -- should never get here");
    avgDist = vguard<double>(jt.nodes(), (double)0);
    for (auto ni : activeNodes) {
      double a_i = 0;
      for (auto nj : activeNodes)
        if (nj != ni) a_i += dist[ni][nj];
      avgDist[ni] = a_i / (double)(nActiveNodes - 2);
    }
    bool isFirstPair = true;
    double minDist = 0;
    TreeNodeIndex min_i = -1, min_j = -1;
    for (auto pi = activeNodes.begin(); pi != activeNodes.end(); ++pi) {
      auto pj = pi;
      for (++pj; pj != activeNodes.end(); ++pj) {
        const double compensatedDist = dist[*pi][*pj] - avgDist[*pi] - avgDist[*pj];
        if (isFirstPair || compensatedDist < minDist) {
          min_i = *pi;
          min_j = *pj;
          minDist = compensatedDist;
          isFirstPair = false;
        }
      }
    }
    const TreeNodeIndex k = jt.nodes();
    dist.push_back(vguard<double>(k + 1));
    dist[k][k] = 0;
    const double d_ij = dist[min_i][min_j];
    for (TreeNodeIndex m = 0; m < k; ++m) dist[m].push_back(dist[k][m] = 0.5 * (dist[min_i][m] + dist[min_j][m] - d_ij));
    double d_ik = 0.5 * (d_ij + avgDist[min_i] - avgDist[min_j]);
    double d_jk = d_ij - d_ik;
    if (d_ik < minBranchLength) {          // Kuhner-Felsenstein, and the minimum branch length
      d_jk -= d_ik - minBranchLength;
      d_ik = minBranchLength;
    }
    if (d_jk < 0) {
      d_ik -= d_jk - minBranchLength;
      d_jk = minBranchLength;
    }
    dist[min_i][k] = dist[k][min_i] = d_ik;
    dist[min_j][k] = dist[k][min_j] = d_jk;
    jt.join(min_i, min_j, d_ik, d_jk);
    activeNodes.erase(min_i);
    activeNodes.erase(min_j);
    activeNodes.insert(k);
  }
  auto iter = activeNodes.begin();
  const TreeNodeIndex i = *iter;
  const TreeNodeIndex j = *++iter;
  const double d = std::max(dist[i][j], 0.);
  jt.join(i, j, d / 2, d / 2);
  adopt(jt, *this);
}

void ReconTree::buildByUPGMA(const vguard<string>& names, const vguard<vguard<double>>& distanceMatrix) {
  Assert(names.size() >= 2, "Fewer than 2 nodes; can't make a binary tree");
  vguard<vguard<double>> dist = distanceMatrix;
  JoinTree jt(names);
  set<TreeNodeIndex> activeNodes;
  for (TreeNodeIndex n = 0; n < (TreeNodeIndex)names.size(); ++n) activeNodes.insert(n);
  vguard<double> nodeHeight(names.size(), 0);
  auto joinedHeight = [&](TreeNodeIndex i, TreeNodeIndex j) {
    return std::max(nodeHeight[i] + minBranchLength, std::max(nodeHeight[j] + minBranchLength, (nodeHeight[i] + nodeHeight[j] + dist[i][j]) / 2));
  };
  while (true) {
    const int nActiveNodes = (int)activeNodes.size();
    if (nActiveNodes == 2) break;
    Assert(nActiveNodes > 2, "Fewer than 2 nodes left -- should never get here");
    bool isFirstPair = true;
    double minDist = 0;
    TreeNodeIndex min_i = -1, min_j = -1;
    for (auto pi = activeNodes.begin(); pi != activeNodes.end(); ++pi) {
      auto pj = pi;
      for (++pj; pj != activeNodes.end(); ++pj) {
        const double d = dist[*pi][*pj];
        if (isFirstPair || d < minDist) {
          min_i = *pi;
          min_j = *pj;
          minDist = d;
          isFirstPair = false;
        }
      }
    }
    const TreeNodeIndex k = jt.nodes();
    dist.push_back(vguard<double>(k + 1));
    dist[k][k] = 0;
    nodeHeight.push_back(joinedHeight(min_i, min_j));
    const double d_ik = nodeHeight[k] - nodeHeight[min_i];
    const double d_jk = nodeHeight[k] - nodeHeight[min_j];
    for (TreeNodeIndex m = 0; m < k; ++m) dist[m].push_back(dist[k][m] = (dist[min_i][m] + dist[min_j][m]) / 2);
    dist[min_i][k] = dist[k][min_i] = d_ik;
    dist[min_j][k] = dist[k][min_j] = d_jk;
    jt.join(min_i, min_j, d_ik, d_jk);
    activeNodes.erase(min_i);
    activeNodes.erase(min_j);
    activeNodes.insert(k);
  }
  auto iter = activeNodes.begin();
  const TreeNodeIndex i = *iter;
  const TreeNodeIndex j = *++iter;
  const double h = joinedHeight(i, j);
  jt.join(i, j, h - nodeHeight[i], h - nodeHeight[j]);
  adopt(jt, *this);
  if (!isUltrametric()) {
    Abort("Tree is not ultrametric");
  }
}

void Reconstructor::buildTree(Dataset& dataset, const vguard<FastSeq>& gappedGuide) {
  const auto dist = model.distanceMatrix(gappedGuide, jukesCantorDistanceMatrix ? 0 : DefaultDistanceMatrixIterations);
  vguard<string> names;
  names.reserve(gappedGuide.size());
  for (const auto& s : gappedGuide) names.push_back(s.name);
  if (useUPGMA) dataset.tree.buildByUPGMA(names, dist);
  else dataset.tree.buildByNeighborJoining(names, dist);
}

}  // namespace historian
