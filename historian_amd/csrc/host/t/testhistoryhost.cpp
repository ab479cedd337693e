// The host's share of a branch-length proposal to the resident history (csrc/hx_history_host.h), stand-alone: no device, no
// library.  `make sanitize` builds this with -fsanitize=address,undefined and runs it on the CPU.  Prints one line per group
// of cases and returns the number of failures.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../hx_history_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static void shapeCases() {
  // every row of GSL's table, both sides of each threshold
  const double below[6] = {0.01, 0.1, 1., 10., 100., 1000.};
  const int table[7][2] = {{5, 1}, {5, 4}, {7, 5}, {9, 7}, {10, 10}, {8, 14}, {8, 15}};
  for (int r = 0; r < 6; ++r) {
    const hx::ExpmShape lo = hx::expm_shape(nextafter(below[r], 0.), 1.), hi = hx::expm_shape(below[r], 1.);
    EXPECT(lo.terms == table[r][0] && lo.squarings == table[r][1]);
    EXPECT(hi.terms == table[r + 1][0] && hi.squarings == table[r + 1][1]);
    EXPECT(lo.shrink == 1. / exp(log(2.) * lo.squarings));
  }
  const hx::ExpmShape zero = hx::expm_shape(3., 0.);
  EXPECT(zero.terms == 5 && zero.squarings == 1 && zero.t == 0.);
  const hx::ExpmShape big = hx::expm_shape(3000., 1.);
  EXPECT(big.terms == 8 && big.squarings == 14 + (int)ceil(log(1.01 * 3000. / 1000.) / log(2.)));
  // the largest finite norm: the squarings stay an int, the shrink factor a (subnormal or zero) double
  EXPECT(hx::expm_norm_ok(DBL_MAX / 2, 1.) && !hx::expm_norm_ok(DBL_MAX, 1.) && !hx::expm_norm_ok(DBL_MAX, 2.) && hx::expm_norm_ok(0., DBL_MAX));
  const hx::ExpmShape huge = hx::expm_shape(DBL_MAX / 2, 1.);
  EXPECT(huge.squarings > 1000 && huge.squarings < 1100 && huge.shrink >= 0.);
  printf("shape: %d failures so far\n", failures);
}

static void lengthCases() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  EXPECT(hx::expm_length_ok(0.) && hx::expm_length_ok(-0.) && hx::expm_length_ok(DBL_MIN) && hx::expm_length_ok(DBL_MAX));
  EXPECT(!hx::expm_length_ok(-DBL_MIN) && !hx::expm_length_ok(-1.) && !hx::expm_length_ok(nan) && !hx::expm_length_ok(inf) && !hx::expm_length_ok(-inf));
  const double rate[4] = {-1.5, 1.5, 0., -0.};
  double m = -1.;
  EXPECT(hx::expm_max_abs(rate, 4, &m) && m == 1.5);
  const double bad[2][2] = {{1., nan}, {-inf, 0.}};
  EXPECT(!hx::expm_max_abs(bad[0], 2, &m) && !hx::expm_max_abs(bad[1], 2, &m));
  EXPECT(hx::expm_max_abs(rate, 0, &m) && m == 0.);
  printf("lengths: %d failures so far\n", failures);
}

static void planCases() {
  for (int A = 1; A <= 64; ++A) {
    const hx::ExpmPlan p = hx::expm_plan(A, 0);
    EXPECT(p.waves >= 1 && p.waves <= 8 && p.per_lane >= 1 && p.per_lane <= 8);
    EXPECT(64 * p.waves * p.per_lane >= A * A && 64 * p.waves * (p.per_lane - 1) < A * A);
    EXPECT(p.lds == 16u * A * A);
  }
  EXPECT(hx::expm_plan(4, 0).waves == 1 && hx::expm_plan(8, 0).waves == 1 && hx::expm_plan(9, 0).waves == 2 && hx::expm_plan(9, 0).per_lane == 1);
  EXPECT(hx::expm_plan(20, 0).waves == 7 && hx::expm_plan(20, 0).per_lane == 1 && hx::expm_plan(21, 0).waves == 7 && hx::expm_plan(22, 0).waves == 8);
  EXPECT(hx::expm_plan(23, 0).per_lane == 2 && hx::expm_plan(32, 0).per_lane == 2 && hx::expm_plan(33, 0).waves == 8 && hx::expm_plan(33, 0).per_lane == 3);
  EXPECT(hx::expm_plan(64, 0).waves == 8 && hx::expm_plan(64, 0).per_lane == 8);
  EXPECT(hx::expm_plan(20, 1).waves == 1 && hx::expm_plan(20, 1).per_lane == 7 && hx::expm_plan(20, 8).per_lane == 1);
  EXPECT(hx::expm_plan(64, 2).waves == 8 && hx::expm_plan(20, 9).waves == 7 && hx::expm_plan(23, 1).waves == 8);      // a forced plan that cannot serve is not taken
  printf("plan: %d failures so far\n", failures);
}

static void closureCases() {
  // leaves 0, 1 under 4; leaves 2, 3 under 5; 4, 5 under the root 6
  const std::vector<int> parent = {4, 4, 5, 5, 6, 6, -1};
  std::vector<int> changed, walked;
  const int one[] = {0};
  EXPECT(hx::history_closure(parent, 1, one, changed, walked) == 0 && changed == std::vector<int>({0}) && walked == std::vector<int>({0, 4, 6}));
  const int three[] = {4, 1, 0};                                 // the caller's order is kept; the walk ascends
  EXPECT(hx::history_closure(parent, 3, three, changed, walked) == 0 && changed == std::vector<int>({4, 1, 0}) && walked == std::vector<int>({0, 1, 4, 6}));
  const int all[] = {0, 1, 2, 3, 4, 5};
  EXPECT(hx::history_closure(parent, 6, all, changed, walked) == 0 && walked.size() == 7);
  const int root[] = {6}, low[] = {-1}, high[] = {7}, twice[] = {2, 5, 2};
  EXPECT(hx::history_closure(parent, 1, root, changed, walked) == 1 && hx::history_closure(parent, 1, low, changed, walked) == 1);
  EXPECT(hx::history_closure(parent, 1, high, changed, walked) == 1 && hx::history_closure(parent, 3, twice, changed, walked) == 2);
  EXPECT(hx::history_closure(parent, 0, one, changed, walked) == 0 && changed.empty() && walked.empty());
  // a caterpillar: the marking stops at the first ancestor already marked
  std::vector<int> cat(9, -1);
  cat[0] = cat[1] = 5;
  for (int k = 2; k < 5; ++k) { cat[k] = 4 + k; cat[3 + k] = 4 + k; }
  const int two[] = {6, 0};
  EXPECT(hx::history_closure(cat, 2, two, changed, walked) == 0 && walked == std::vector<int>({0, 5, 6, 7, 8}));
  const std::vector<int> single = {-1};                          // a tree of one node has no branch
  EXPECT(hx::history_closure(single, 1, one, changed, walked) == 1);
  printf("closure: %d failures so far\n", failures);
}

int main() {
  shapeCases();
  lengthCases();
  planCases();
  closureCases();
  printf(failures ? "testhistoryhost: %d FAILED\n" : "testhistoryhost: ok\n", failures);
  return failures;
}
