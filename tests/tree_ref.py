"""Restatement of the reference's tree estimation (test infrastructure, as tests/sibling_ref.py is):

  RateModel::expectedSubstitutionRate   src/model.cpp:336-347
  RateModel::mlDistance, distanceMatrix src/model.cpp:506-549
  DistanceMatrixParams::tJC, tML        src/model.cpp:551-655
  Tree::buildByNeighborJoining, UPGMA   src/tree.cpp:240-462
  Tree::toString / parse                src/tree.cpp:15-37, 56-102

The reference minimises the pairwise negative log-likelihood over t with GSL's golden-section
minimiser.  GSL is not part of the reference's sources, so one step of it is restated from its
published source (min/golden.c, min/convergence.c): the trial point lies 0.3819660 (GSL's literal)
into the larger of the two sub-intervals; a trial below the current minimum becomes the minimum and
the bracket does NOT move; otherwise the bracket end on the trial's side moves to it.

exp(Rt) is oracle.historian_oracle.sub_prob_matrix_ss.  `_sub_prob` below performs the same IEEE
operations in the same order with numpy (an added product with a zero left factor adds +-0 to a sum
that started at +0, which changes no bit), so that the 43-row family takes seconds and not minutes;
tests/test_oracle_tree.py holds the two to the same bits.
"""
import functools
import math

import numpy as np

from oracle import historian_oracle as ho
from tests.recon_helpers import parse_newick

T_MIN, T_MAX = 1e-9, 10.
GOLDEN = 0.3819660            # GSL's literal, not (3 - sqrt 5) / 2
CONVERGENCE = .01             # tML_convergence: the bracket within 1 %
MIN_BRANCH_LENGTH = 1e-9      # TREE_MIN_BRANCH_LEN
INF = float("inf")


def series_shape(norm):
    """(terms, squarings) of gsl_linalg_exponential_ss by the largest |element| of R t"""
    for row, below in zip(ho._MVL_DOUBLE, (0.01, 0.1, 1., 10., 100., 1000.)):
        if norm < below:
            return row
    terms, squarings = ho._MVL_DOUBLE[5]
    return terms, squarings + int(math.ceil(math.log(1.01 * norm / 1000.) / math.log(2.)))


def _matmul(p, q):
    # all products, each rounded; then summed over k: a reduction over an axis that is not the last one adds whole
    # [i][j] planes one after another, k increasing (no pairwise regrouping), as the scalar loop does
    return np.add.reduce(p[:, :, None] * q[None, :, :], axis=1)


def _sub_prob(sr, t):
    """the bits of ho.sub_prob_matrix_ss(sr, t), as an array"""
    rt = np.asarray(sr, dtype=np.float64) * t
    terms, squarings = series_shape(float(np.max(np.abs(rt))) if rt.size else 0.)
    b = rt * (1. / math.exp(math.log(2.) * squarings))
    idx = np.arange(rt.shape[0])
    eb = b * (1. / terms)
    eb[idx, idx] += 1.
    for count in range(terms - 1, 0, -1):
        eb = _matmul(b, eb) * (1. / count)
        eb[idx, idx] += 1.
    for _ in range(squarings):
        eb = _matmul(eb, eb)
    return eb


def products_taken(sr, t):
    """matrix products of one exp(R t): terms - 1 in the Horner recurrence plus the squarings"""
    terms, squarings = series_shape(float(np.max(np.abs(np.asarray(sr) * t))))
    return terms - 1 + squarings


def expected_sub_rate(model):
    """RateModel::expectedSubstitutionRate, src/model.cpp:336-347"""
    r = 0.
    a = len(model.alphabet)
    for c in range(model.components()):
        eqm = ho.eqm_prob_vector(np.asarray(model.sub_rate[c], dtype=np.float64))
        for i in range(a):
            for j in range(a):
                if i != j:
                    r += model.cpt_weight[c] * float(eqm[i]) * float(model.sub_rate[c][i][j])
    return r


def pair_counts(model, x_gapped, y_gapped):
    """{(a, b): n} over the columns in which both rows hold a residue of the alphabet (src/model.cpp:508-518)"""
    assert len(x_gapped) == len(y_gapped)
    counts = {}
    for ci, cj in zip(x_gapped, y_gapped):
        if ci in "-.*" or cj in "-.*":
            continue
        ti, tj = ho.tokenize(ci, model.alphabet), ho.tokenize(cj, model.alphabet)
        if ti >= 0 and tj >= 0:
            counts[(ti, tj)] = counts.get((ti, tj), 0) + 1
    return counts


def tokens(model, rows):
    """[n_seqs][n_cols] int8 for hx_distance_matrix: the alphabet index, -1 where the character is not counted"""
    out = np.full((len(rows), len(rows[0]) if rows else 0), -1, dtype=np.int8)
    for r, row in enumerate(rows):
        for k, ch in enumerate(row):
            if ch not in "-.*":
                out[r, k] = ho.tokenize(ch, model.alphabet)
    return out


def counts_from_tokens(tx, ty):
    counts = {}
    for a, b in zip(tx, ty):
        if a >= 0 and b >= 0:
            counts[(int(a), int(b))] = counts.get((int(a), int(b)), 0) + 1
    return counts


class Search:
    """DistanceMatrixParams of one pair: counts, the model, and what the search did"""

    def __init__(self, model, counts, esr=None, sub_prob=None):
        self.model = model
        self.items = sorted((ab, n) for ab, n in counts.items() if n != 0)     # std::map order
        self.esr = expected_sub_rate(model) if esr is None else esr
        self.sub_prob = sub_prob or (lambda t: [_sub_prob(sr, t) for sr in model.sub_rate])
        self.evaluations = 0
        self.min_gap = INF           # smallest relative gap of two compared, unequal likelihoods
        self.t_lower = self.t_upper = None

    def neg_log_like(self, t):
        """distanceMatrixNegLogLike, src/model.cpp:551-564"""
        self.evaluations += 1
        sub = self.sub_prob(t)
        ll = 0.
        for (a, b), n in self.items:
            p = 0.
            for c in range(self.model.components()):
                p += self.model.cpt_weight[c] * float(sub[c][a][b])
            ll += (math.log(p) if p > 0 else (-INF if p == 0 else float("nan"))) * float(n)
        return -ll

    def less(self, u, v):
        if u != v and not (math.isnan(u) or math.isnan(v)):
            big = max(abs(u), abs(v))
            if big != INF:
                self.min_gap = min(self.min_gap, abs(u - v) / big)
        return u < v

    def t_jc(self):
        """src/model.cpp:570-582; NaN for a pair without a counted column (0 / 0)"""
        same = sum(n for (a, b), n in self.items if a == b)
        diff = sum(n for (a, b), n in self.items if a != b)
        if same + diff == 0:
            return float("nan")
        p_diff = diff / float(same + diff)
        a = float(len(self.model.alphabet))
        if p_diff >= (a - 1) / a:
            return INF
        return -((a - 1) / a) * math.log(1 - (a / (a - 1)) * p_diff) / self.esr

    def t_ml(self, max_iterations=100):
        """src/model.cpp:584-655"""
        tjc = self.t_jc()
        tjc = T_MIN if not T_MIN < tjc else tjc          # std::max(tMin, tJC): (tMin < tJC) ? tJC : tMin
        tjc = T_MAX if T_MAX < tjc else tjc              # std::min(tMax, .)
        if max_iterations <= 0:
            return tjc
        f, less = self.neg_log_like, self.less
        t_lower, t_upper = min(T_MIN, tjc / 2), max(T_MAX, tjc * 2)
        self.t_lower, self.t_upper = t_lower, t_upper
        ll_lower, ll_upper = f(t_lower), f(t_upper)
        lljc = f(tjc)
        if less(lljc, ll_lower) and less(lljc, ll_upper):
            t, f_min = tjc, lljc
        else:
            found = False
            lo, hi = t_lower, t_upper
            while not found and hi - lo > t_lower:
                step = (hi - lo) / 4.
                x = lo
                while x < hi and not found:
                    ll = f(x)
                    if less(ll, ll_lower) and less(ll, ll_upper):
                        found, t, f_min = True, x, ll
                    x += step
                if not found:
                    if less(ll_lower, ll_upper):
                        hi = (lo + hi) / 2
                    else:
                        lo = (lo + hi) / 2
            if not found:
                return t_lower if less(ll_lower, ll_upper) else t_upper
        # gsl_min_fminimizer_set(s, F, t, tLower, tUpper) evaluates f at the three points again: the same bits
        x_min, x_lo, x_up = t, t_lower, t_upper
        for _ in range(max_iterations):
            w_lo, w_up = x_min - x_lo, x_up - x_min
            x_new = x_min + GOLDEN * (w_up if w_up > w_lo else -w_lo)
            f_new = f(x_new)
            if less(f_new, f_min):
                x_min, f_min = x_new, f_new              # the bracket does not move
            elif x_new < x_min and less(f_min, f_new):
                x_lo = x_new
            elif x_new > x_min and less(f_min, f_new):
                x_up = x_new
            # else GSL_FAILURE, which the reference ignores
            t = x_min
            same_sign = (x_lo > 0 and x_up > 0) or (x_lo < 0 and x_up < 0)
            tolerance = CONVERGENCE * (min(abs(x_lo), abs(x_up)) if same_sign else 0.)
            if abs(x_up - x_lo) < tolerance:
                break
        return t


def ml_distance(model, x_gapped, y_gapped, max_iterations=100, esr=None, info=None):
    """RateModel::mlDistance.  esr: the expected substitution rate if the caller holds it already;
    info: a dict that receives evaluations, min_gap (the near-tie flag), t_lower, t_upper."""
    s = Search(model, pair_counts(model, x_gapped, y_gapped), esr)
    t = s.t_ml(max_iterations)
    if info is not None:
        info.update(evaluations=s.evaluations, min_gap=s.min_gap, t_lower=s.t_lower, t_upper=s.t_upper)
    return t


def distance_matrix(model, rows, max_iterations=100, esr=None, want_info=False):
    """RateModel::distanceMatrix over gapped rows (strings); with want_info also {(i, j): info}"""
    n = len(rows)
    esr = expected_sub_rate(model) if esr is None else esr
    dist = [[0.] * n for _ in range(n)]
    infos = {}
    for i in range(n - 1):
        for j in range(i + 1, n):
            infos[(i, j)] = {}
            dist[i][j] = dist[j][i] = ml_distance(model, rows[i], rows[j], max_iterations, esr, infos[(i, j)])
    return (dist, infos) if want_info else dist


class BuiltTree:
    """Tree as the builders leave it before parse(toString()): nodes in join order"""

    def __init__(self, names):
        self.name = list(names)
        self.parent = [-1] * len(names)
        self.d = [-1.] * len(names)
        self.child = [[] for _ in names]

    def join(self, i, j, d_i, d_j):
        k = len(self.name)
        self.name.append("")
        self.parent.append(-1)
        self.d.append(-1.)
        self.child.append([i, j])
        self.parent[i] = self.parent[j] = k
        self.d[i], self.d[j] = max(0., d_i), max(0., d_j)
        return k

    def to_newick(self):
        def length(d):
            return ":%g" % d if d >= 0 else ""

        def describe(n):
            if not self.child[n]:
                return self.name[n]
            return "(" + ",".join(describe(c) + length(self.d[c]) for c in self.child[n]) + ")" + self.name[n]
        return describe(len(self.name) - 1) + ";"


def neighbor_joining(names, distance):
    """Tree::buildByNeighborJoining, src/tree.cpp:240-352 -> BuiltTree"""
    assert len(names) >= 2
    n0 = len(names)
    dist = [list(row) for row in distance]
    tree = BuiltTree(names)
    active = list(range(n0))                      # std::set: increasing order
    while len(active) > 2:
        na = len(active)
        avg = [0.] * len(tree.name)
        for ni in active:
            a_i = 0.
            for nj in active:
                if nj != ni:
                    a_i += dist[ni][nj]
            avg[ni] = a_i / float(na - 2)
        first, best, min_i, min_j = True, 0., -1, -1
        for p, ni in enumerate(active):
            for nj in active[p + 1:]:
                comp = dist[ni][nj] - avg[ni] - avg[nj]
                if first or comp < best:
                    min_i, min_j, best, first = ni, nj, comp, False
        k = len(tree.name)
        d_ij = dist[min_i][min_j]
        new_row = [0.5 * (dist[min_i][m] + dist[min_j][m] - d_ij) for m in range(k)]
        for m in range(k):
            dist[m].append(new_row[m])
        dist.append(new_row + [0.])
        d_ik = 0.5 * (d_ij + avg[min_i] - avg[min_j])
        d_jk = d_ij - d_ik
        if d_ik < MIN_BRANCH_LENGTH:               # Kuhner-Felsenstein, and the minimum branch length
            d_jk -= d_ik - MIN_BRANCH_LENGTH
            d_ik = MIN_BRANCH_LENGTH
        if d_jk < 0:
            d_ik -= d_jk - MIN_BRANCH_LENGTH
            d_jk = MIN_BRANCH_LENGTH
        dist[min_i][k] = dist[k][min_i] = d_ik
        dist[min_j][k] = dist[k][min_j] = d_jk
        assert tree.join(min_i, min_j, d_ik, d_jk) == k
        active = sorted(set(active) - {min_i, min_j} | {k})
    i, j = active
    d = max(dist[i][j], 0.)
    tree.join(i, j, d / 2, d / 2)
    return tree


def upgma(names, distance):
    """Tree::buildByUPGMA, src/tree.cpp:362-454 -> BuiltTree"""
    assert len(names) >= 2
    dist = [list(row) for row in distance]
    tree = BuiltTree(names)
    active = list(range(len(names)))
    height = [0.] * len(names)

    def joined_height(i, j):
        return max(height[i] + MIN_BRANCH_LENGTH, max(height[j] + MIN_BRANCH_LENGTH, (height[i] + height[j] + dist[i][j]) / 2))
    while len(active) > 2:
        first, best, min_i, min_j = True, 0., -1, -1
        for p, ni in enumerate(active):
            for nj in active[p + 1:]:
                d = dist[ni][nj]
                if first or d < best:
                    min_i, min_j, best, first = ni, nj, d, False
        k = len(tree.name)
        height.append(joined_height(min_i, min_j))
        d_ik, d_jk = height[k] - height[min_i], height[k] - height[min_j]
        new_row = [(dist[min_i][m] + dist[min_j][m]) / 2 for m in range(k)]
        for m in range(k):
            dist[m].append(new_row[m])
        dist.append(new_row + [0.])
        dist[min_i][k] = dist[k][min_i] = d_ik
        dist[min_j][k] = dist[k][min_j] = d_jk
        assert tree.join(min_i, min_j, d_ik, d_jk) == k
        active = sorted(set(active) - {min_i, min_j} | {k})
    i, j = active
    h = joined_height(i, j)
    tree.join(i, j, h - height[i], h - height[j])
    return tree


def to_newick(tree):
    return tree.to_newick()


def parse_tree(newick):
    """Tree::parse of the string: the node numbering of the reference's Newick reader (post-order, children left to
    right, as tests/recon_helpers.parse_newick restates it), branch lengths raised to the minimum (src/tree.cpp:27-28)"""
    t = parse_newick(newick)
    root = t.root()
    t.branch_length = [b if n == root else max(b, MIN_BRANCH_LENGTH) for n, b in enumerate(t.branch_length)]
    return t


def build_tree(model, names, rows, upgma_tree=False, jukes_cantor=False, distance=None):
    """Reconstructor::buildTree, src/recon.cpp:732-743 -> (Newick string, parsed tree)"""
    if distance is None:
        distance = distance_matrix(model, rows, 0 if jukes_cantor else 100)
    text = (upgma if upgma_tree else neighbor_joining)(names, distance).to_newick()
    return text, parse_tree(text)


@functools.lru_cache(maxsize=None)
def family(model_file, fasta_file):
    """(model, names, rows, expected rate, distances, infos) of a fixture family under tests/golden/reference_data:
    computed once per process and shared by the tests that need it; treat it as read-only"""
    import os
    from oracle.ref_mains import read_fasta
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
    model = ho.RateModel.from_file(os.path.join(data, model_file))
    recs = read_fasta(os.path.join(data, fasta_file))
    names, rows = [r[0] for r in recs], [r[1] for r in recs]
    esr = expected_sub_rate(model)
    dist, infos = distance_matrix(model, rows, esr=esr, want_info=True)
    return model, names, rows, esr, dist, infos


RECORDED = "tests/golden/tree_ref/%s.distances.json"


def record(esr, dist, infos):
    """what family() found, as JSON-able data: floats as hex"""
    return {"expected_sub_rate": esr.hex(),
            "pairs": [[i, j, dist[i][j].hex(), info["evaluations"], info["min_gap"].hex(), info["t_lower"].hex(), info["t_upper"].hex()]
                      for (i, j), info in sorted(infos.items())]}


def recorded_family(model_file, fasta_file):
    """family() of the 43-row PF16593 fixture takes some twenty seconds, so its result is kept under tests/golden/tree_ref
    (tests/test_oracle_tree.py computes it again and compares every bit); this reads the record back in family()'s form"""
    import json
    import os
    from oracle.ref_mains import read_fasta
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = os.path.join(root, "tests", "golden", "reference_data")
    model = ho.RateModel.from_file(os.path.join(data, model_file))
    recs = read_fasta(os.path.join(data, fasta_file))
    names, rows = [r[0] for r in recs], [r[1] for r in recs]
    with open(os.path.join(root, RECORDED % os.path.splitext(fasta_file)[0])) as f:
        js = json.load(f)
    n = len(rows)
    dist = [[0.] * n for _ in range(n)]
    infos = {}
    for i, j, d, ev, gap, lo, hi in js["pairs"]:
        dist[i][j] = dist[j][i] = float.fromhex(d)
        infos[(i, j)] = dict(evaluations=ev, min_gap=float.fromhex(gap), t_lower=float.fromhex(lo), t_upper=float.fromhex(hi))
    return model, names, rows, float.fromhex(js["expected_sub_rate"]), dist, infos
