// The host's share of an excluded-neighbour query on the resident history (csrc/hx_history_host.h: the positions of every node
// and their block offsets, the validation of the pairs, the paths, the output offsets), stand-alone: no device, no library.
// `make sanitize` builds this with -fsanitize=address,undefined and runs it on the CPU.  Prints one line per group of cases
// and returns the number of failures.
#include <cstdio>
#include <vector>

#include "../../hx_history_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

typedef std::vector<long long> LL;
typedef std::vector<int> II;

static void positionCases() {
  // three nodes, 130 columns in three blocks of 64 (padded with gaps): node 0 everywhere, node 1 nowhere in block 0 and in
  // every second column after it, node 2 in a 71-column stretch over the end of block 0 only
  const int N = 3;
  const long long n_cols = 130, ncp = 192;
  std::vector<signed char> tok((size_t)N * ncp, (signed char)-2);
  for (long long c = 0; c < n_cols; ++c) {
    tok[0 * ncp + c] = (signed char)(c % 4);
    if (c >= 64 && c % 2 == 0) tok[1 * ncp + c] = -1;
    if (c >= 30 && c <= 100) tok[2 * ncp + c] = 2;
  }
  LL len, off;
  hx::history_positions(tok.data(), N, ncp, len, off);
  EXPECT(len == LL({130, 33, 71}));
  EXPECT(off == LL({0, 64, 128, 0, 0, 32, 0, 34, 71}));
  // one column, one block
  std::vector<signed char> one(64, (signed char)-2);
  one[0] = 3;
  hx::history_positions(one.data(), 1, 64, len, off);
  EXPECT(len == LL({1}) && off == LL({0}));
  printf("positions: %d failures so far\n", failures);
}

static void planCases() {
  // leaves 0, 1 under 4; leaves 2, 3 under 5; 4, 5 under the root 6
  const II parent = {4, 4, 5, 5, 6, 6, -1};
  const LL len = {10, 0, 7, 7, 12, 9, 13};
  hx::ExcludedPlan p;
  // a branch: (parent, node) needs the way down to the parent, (node, parent) none
  const int node[] = {4, 0}, excl[] = {0, 4};
  EXPECT(hx::history_excluded_plan(parent, len, 8, 2, node, excl, p) == 0);
  EXPECT(p.pair == II({4, 0, 0, 2, 0, 4, -1, 0}) && p.path == II({6, 4}));
  EXPECT(p.out_off == LL({0, 96}) && p.out_len == LL({12, 10}) && p.total == 176 && p.max_len == 12);
  // NodeAlignMove's four pairs at node 4; a node without positions takes no room
  const int n4[] = {0, 1, 4, 6}, e4[] = {4, 4, 6, 4};
  EXPECT(hx::history_excluded_plan(parent, len, 8, 4, n4, e4, p) == 0);
  EXPECT(p.pair == II({0, 4, -1, 0, 1, 4, -1, 0, 4, 6, -1, 0, 6, 4, 0, 1}) && p.path == II({6}));
  EXPECT(p.out_off == LL({0, 80, 80, 176}) && p.out_len == LL({10, 0, 12, 13}) && p.total == 280 && p.max_len == 13);
  // the root without one child: a path of one node; a node named twice is two pairs with a path each
  const int twice[] = {6, 5, 5}, te[] = {5, 2, 3};
  EXPECT(hx::history_excluded_plan(parent, len, 1, 3, twice, te, p) == 0);
  EXPECT(p.path == II({6, 6, 5, 6, 5}) && p.pair == II({6, 5, 0, 1, 5, 2, 1, 2, 5, 3, 3, 2}) && p.total == 13 + 9 + 9);
  // refusals: out of range before anything else; then a neighbour that is none
  const int lo[] = {-1}, hi[] = {7}, ok[] = {0}, self[] = {0}, sib[] = {1}, far[] = {6}, par[] = {4}, root[] = {6}, none[] = {-1};
  EXPECT(hx::history_excluded_plan(parent, len, 8, 1, lo, par, p) == 1 && hx::history_excluded_plan(parent, len, 8, 1, hi, par, p) == 1);
  EXPECT(hx::history_excluded_plan(parent, len, 8, 1, ok, lo, p) == 1 && hx::history_excluded_plan(parent, len, 8, 1, ok, hi, p) == 1);
  EXPECT(hx::history_excluded_plan(parent, len, 8, 1, root, none, p) == 1);        // the root's parent is no node
  EXPECT(hx::history_excluded_plan(parent, len, 8, 1, ok, self, p) == 2 && hx::history_excluded_plan(parent, len, 8, 1, ok, sib, p) == 2);
  EXPECT(hx::history_excluded_plan(parent, len, 8, 1, ok, far, p) == 2 && hx::history_excluded_plan(parent, len, 8, 1, root, ok, p) == 2);
  const int mixed_n[] = {4, 0, 7}, mixed_e[] = {0, 1, 0};                            // a range error wins over a bad neighbour
  EXPECT(hx::history_excluded_plan(parent, len, 8, 3, mixed_n, mixed_e, p) == 1);
  EXPECT(hx::history_excluded_plan(parent, len, 8, 0, ok, par, p) == 0 && p.pair.empty() && p.total == 0);
  // a caterpillar of 40 leaves: the path to the deepest internal node holds the whole spine
  const int L = 40;
  II cat(2 * L - 1, -1);
  cat[0] = cat[1] = L;
  for (int k = 2; k < L; ++k) { cat[k] = L + k - 1; cat[L + k - 2] = L + k - 1; }
  const LL ones(cat.size(), 1);
  const int deep[] = {L}, leaf[] = {0};
  EXPECT(hx::history_excluded_plan(cat, ones, 4, 1, deep, leaf, p) == 0 && p.path.size() == (size_t)(L - 1) && p.path.front() == 2 * L - 2 && p.path.back() == L);
  for (size_t k = 1; k < p.path.size(); ++k) EXPECT(cat[p.path[k]] == p.path[k - 1]);
  printf("plan: %d failures so far\n", failures);
}

// hx_history_branch_batch_create's share: the branches checked, the query's pairs and the jobs of the batch
static void branchCases() {
  const II parent = {4, 4, 5, 5, 6, 6, -1};
  const LL len = {10, 0, 7, 7, 12, 9, 0};
  const double sub[2 * 4 * 4] = {0}, ins[2 * 4] = {0};
  const int32_t xe[13] = {0}, ye[11] = {0};
  auto branch = [&](int node, int md) {
    hx_history_branch b = {};
    b.node = node; b.log_sub = sub; b.log_ins = ins; b.max_distance = md;
    for (int s = 0; s < 3; ++s)
      for (int d = 0; d < 4; ++d) b.trans[s][d] = -(double)(4 * s + d);
    b.x_env = md >= 0 ? xe : nullptr;
    b.y_env = md >= 0 ? ye : nullptr;
    return b;
  };
  hx::BranchHandoffPlan p;
  // a leaf branch with a band, a node without positions, a branch under a parent (the root) without positions
  const hx_history_branch three[] = {branch(0, 2), branch(1, -1), branch(5, -1)};
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, three, 3, 65536, p) == 0);
  EXPECT(p.node == II({4, 0, 4, 1, 6, 5}) && p.exclude == II({0, 4, 1, 4, 5, 6}) && p.jobs.size() == 3);
  EXPECT(p.jobs[0].x_len == 12 && p.jobs[0].y_len == 10 && p.jobs[0].components == 2 && p.jobs[0].alphabet == 4);
  EXPECT(p.jobs[0].max_distance == 2 && p.jobs[0].x_env == xe && p.jobs[0].y_env == ye && p.jobs[0].trans[2][3] == -11. && !p.jobs[0].x_pwm && !p.jobs[0].y_sub);
  EXPECT(p.jobs[1].x_len == 12 && p.jobs[1].y_len == 0 && p.jobs[1].max_distance == -1 && !p.jobs[1].x_env);
  EXPECT(p.jobs[2].x_len == 0 && p.jobs[2].y_len == 9);
  // the pairs make a plan of the query
  hx::ExcludedPlan q;
  EXPECT(hx::history_excluded_plan(parent, len, 8, 6, p.node.data(), p.exclude.data(), q) == 0 && q.out_len == LL({12, 10, 12, 0, 0, 9}));
  // refusals: the root and what lies outside; a range error wins over a null pointer
  for (int node : {-1, 6, 7}) {
    const hx_history_branch bad[] = {branch(0, -1), branch(node, -1)};
    EXPECT(hx::history_branch_plan(parent, len, 4, 2, bad, 2, 65536, p) == 1 && p.jobs.empty());
  }
  hx_history_branch null_sub = branch(0, -1), null_ins = branch(0, -1), half = branch(0, 0), none = branch(0, 3), outside = branch(9, -1);
  null_sub.log_sub = nullptr; null_ins.log_ins = nullptr; half.y_env = nullptr; none.x_env = none.y_env = nullptr; outside.log_sub = nullptr;
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, &null_sub, 1, 65536, p) == 2 && hx::history_branch_plan(parent, len, 4, 2, &null_ins, 1, 65536, p) == 2);
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, &half, 1, 65536, p) == 2 && hx::history_branch_plan(parent, len, 4, 2, &none, 1, 65536, p) == 2);
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, &outside, 1, 65536, p) == 1);
  // a parent row at the limit: 12 positions are too many when fewer than 12 are allowed, fine when fewer than 13 are
  const hx_history_branch leaf = branch(0, -1);
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, &leaf, 1, 12, p) == 3 && hx::history_branch_plan(parent, len, 4, 2, &leaf, 1, 13, p) == 0);
  LL huge = len;
  huge[0] = 0x7fffffffLL;
  EXPECT(hx::history_branch_plan(parent, huge, 4, 2, &leaf, 1, 65536, p) == 3);
  EXPECT(hx::history_branch_plan(parent, len, 4, 2, &leaf, 0, 65536, p) == 0 && p.jobs.empty());
  printf("branches: %d failures so far\n", failures);
}

int main() {
  positionCases();
  planCases();
  branchCases();
  printf(failures ? "testcondpwmhost: %d FAILED\n" : "testcondpwmhost: ok\n", failures);
  return failures;
}
