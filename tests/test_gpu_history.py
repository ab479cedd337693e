"""The history resident on the device (hx_history.hip behind capi.History): the full evaluation against the sum-product
oracle's fill_up, proposals against freshly created histories bit for bit, the indel transition counts against a plain
restatement of pairPath, every refusal, the stream contract.

Bounds.  A column's log-likelihood: 1e-12 relative, with the floor of tests/test_gpu_ancestors.py for the all-wildcard
column (the same arithmetic: the device's log() and the order of the sums in the matrix-vector products differ from
libm's and numpy's).  Their sum: those bounds added up, plus n_cols * 2^-53 * sum |cll| for the two orders of the sum."""
import functools
import json
import math
import os

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from oracle import c_oracle
from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from tests import history_ref as HR
from tests import stream_helpers as SH
from tests.test_gpu_ancestors import CYCLIC, PROT4, _recon_columns
from tests.test_gpu_sumprod import _random_model, _random_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def column_bound(want):
    return 1e-12 * abs(want) + (1e-13 if abs(want) < 1e-6 else 0.)


class Case:
    """A model, a tree, an alignment; the device's inputs and, computed once and never changed, the oracle's column
    log-likelihoods.  The device gets the oracle's exp(R t): the comparison is of the passes, not of two exponentials."""

    def __init__(self, js, parent, length, rows, probe=False):
        self.omodel, self.model = ho.RateModel(js), hostmodel.RateModel(js)
        self.parent, self.length, self.rows = list(parent), list(length), rows
        self.tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
        sp = so.SumProduct(self.omodel, self.tree)
        self.n, self.c, self.a = len(parent), sp.C, sp.A
        self.sub_prob = HR.oracle_sub_prob(self.omodel)
        self.branch_sub = self.matrices(length)
        for r in range(self.n - 1):
            for cpt in range(self.c):
                assert np.array_equal(self.branch_sub[cpt, r], sp.branch_sub[cpt][r])
        self.ins_prob = np.asarray(self.model.root, dtype=float).reshape(self.c, self.a)
        self.log_cpt_weight = np.log(np.asarray(self.model.cpt_weight, dtype=float))
        self.tokens = counts.tokenize_columns(self.model.alphabet, rows)
        self.want, self.wild_rescales, self.residue_rescales = [], 0, 0
        for seq in so.columns_of(self.tree, dict(enumerate(rows))):
            sp.init_column(seq)
            sp.fill_up()
            self.want.append(sp.col_log_like)
            if probe:
                self._probe(sp)

    def _probe(self, sp):
        """which of the reference's two rescaling rules fill_up took in this column (src/sumprod.cpp:120-124, 133-137)"""
        for cpt in range(sp.C):
            for r in sp.ungapped:
                f = np.ones(sp.A)
                for ch in self.tree.child[r]:
                    f = f * sp.E[cpt][ch]
                if sp.col[r] == so.WILD:
                    self.wild_rescales += float(f.max()) < so.RESCALE_THRESHOLD
                else:
                    self.residue_rescales += f[sp.tokenize(sp.col[r])] < so.RESCALE_THRESHOLD

    def matrices(self, length):
        out = np.zeros((self.c, self.n, self.a, self.a))
        for r in range(self.n - 1):
            out[:, r] = np.asarray(self.sub_prob(length[r]))
        return out

    def history(self, branch_sub=None, tokens=None, stream=None):
        return capi.History(self.parent, self.ins_prob, self.log_cpt_weight, self.tokens if tokens is None else tokens,
                            self.branch_sub if branch_sub is None else branch_sub, stream=stream)

    def check(self, lp_sub, cll, what):
        want = np.asarray(self.want)
        dev = np.abs(cll - want)
        bounds = np.asarray([column_bound(w) for w in self.want])
        worst = float(np.max(np.where(np.abs(want) >= 1e-6, dev / np.maximum(np.abs(want), 1e-300), 0.)))      # (but for the floor's columns)
        want_sum = HR._sum_in_order(self.want)
        sum_bound = float(bounds.sum()) + len(self.want) * 2. ** -53 * float(np.abs(want).sum())
        print("%s: %d columns, worst relative deviation of a column %.3g, lp_sub %.17g against %.17g: off by %.3g (bound %.3g)"
              % (what, len(self.want), worst, lp_sub, want_sum, abs(lp_sub - want_sum), sum_bound))
        assert np.all(dev <= bounds), int(np.argmax(dev - bounds))
        assert abs(lp_sub - want_sum) <= sum_bound


@functools.lru_cache(maxsize=None)
def case(name, n_cols=130):
    if name == "prot4":
        with open(PROT4) as f:
            js = json.load(f)
        rng = np.random.default_rng(21)
        parent, length = _random_tree(rng, 9)
        return Case(js, parent, length, _recon_columns(rng, parent, js["alphabet"], n_cols))
    if name == "acgt":
        rng = np.random.default_rng(22)
        parent, length = _random_tree(rng, 9)
        return Case(CYCLIC, parent, length, _recon_columns(rng, parent, "acgt", n_cols))
    rng = np.random.default_rng(len(name))
    js = _random_model(rng, name, True)
    parent, length = _random_tree(rng, 9)
    return Case(js, parent, length, _recon_columns(rng, parent, name, n_cols))


@pytest.mark.parametrize("name", ["prot4", "acgt", "acgtu", "abcdefghijklmnopqrstu"])
def test_the_full_evaluation_against_the_oracles_fill_up(name):
    """17 nodes, 130 columns (two blocks of 64 and a ragged third); the 4 x 20 mixture and DNA have kernels of their own,
    A = 5 and A = 21 take the general one"""
    c = case(name)
    assert (c.n, len(c.want)) == (17, 130) and (c.c, c.a) == {"prot4": (4, 20), "acgt": (1, 4)}.get(name, (1, len(name)))
    h = c.history()
    c.check(*h.log_like(), what=name)
    assert h.kernel_ms() > 0
    h.close()


def _caterpillar(leaves):
    """leaf 0 and leaf 1 under the first internal node, every further leaf joins the node before it"""
    parent = [-1] * (2 * leaves - 1)
    parent[0] = parent[1] = leaves
    for k in range(2, leaves):
        parent[k] = leaves + k - 1
        parent[leaves + k - 2] = leaves + k - 1
    return parent


@functools.lru_cache(maxsize=None)
def deep_case():
    # 48 leaves, chosen on the CPU: by then columns of unlike residues have passed 1e-30 under wildcard ancestors (3 times)
    # and under residue ancestors (9 times); the probe counts them and the test asserts both
    leaves = 48
    parent = _caterpillar(leaves)
    rng = np.random.default_rng(7)
    length = [float(rng.uniform(.05, .3)) for _ in parent]
    n = len(parent)
    rows = [[] for _ in range(n)]
    for k in range(6):
        for r in range(n):
            if r < leaves:
                rows[r].append("acgt"[(r + k) % 4] if (r + k) % 7 else "x")
            else:
                rows[r].append("*" if k % 2 == 0 else "acgt"[(r * 3 + k) % 4])
    return Case(CYCLIC, parent, length, ["".join(r) for r in rows], probe=True)


def test_both_rescaling_rules_on_a_deep_caterpillar():
    c = deep_case()
    print("the oracle rescaled %d wildcard vectors and %d residue entries" % (c.wild_rescales, c.residue_rescales))
    assert c.wild_rescales >= 1 and c.residue_rescales >= 1
    h = c.history()
    c.check(*h.log_like(), what="caterpillar")
    h.close()


# ---- edge columns: a balanced tree of four leaves; leaves 0, 1 under node 4; leaves 2, 3 under node 5; the root 6 ----
EDGE_PARENT, EDGE_LENGTH = [4, 4, 5, 5, 6, 6, -1], [.1, .2, .15, .3, .25, .05, 0.]
EDGE_COLUMNS = ["--g----",        # one ungapped leaf
                "a------",        # the column's root (leaf 0) lies below the changed node 4, which is a gap
                "ac--*--",        # the changed node is the column's root: its own branch is not used, its children's are
                "--gt-*-",        # the changed node is a gap, the column lives in the other subtree
                "ac-t***",        # the changed node inside the column
                "acgt***"]


def _edge_case(n_cols):
    cols = [EDGE_COLUMNS[k % len(EDGE_COLUMNS)] for k in range(n_cols)]
    rows = ["".join(col[r] for col in cols) for r in range(7)]
    return Case(CYCLIC, EDGE_PARENT, EDGE_LENGTH, rows)


@pytest.mark.parametrize("n_cols", [1, 6, 64, 65])
def test_edge_columns_full_and_after_a_proposal(n_cols):
    c = _edge_case(n_cols)
    h = c.history()
    c.check(*h.log_like(), what="edge columns")
    # node 4 and its children change: the proposal against the oracle on the new tree, and against a fresh history
    length = list(EDGE_LENGTH)
    length[4], length[0], length[1] = .07, .28, .38
    new = Case(CYCLIC, EDGE_PARENT, length, c.rows)
    lp = h.propose([4, 0, 1], new.branch_sub[:, [4, 0, 1]].transpose(1, 0, 2, 3))
    got_lp, got = h.log_like(1)
    assert lp == got_lp
    new.check(got_lp, got, what="edge columns, proposed")
    fresh = new.history()
    assert fresh.log_like()[1].tobytes() == got.tobytes() and fresh.log_like()[0] == lp
    # columns that do not contain the branches keep their bits
    old = h.log_like(0)[1]
    for k in range(n_cols):
        if k % len(EDGE_COLUMNS) in (0, 1, 3):
            assert got[k] == old[k], k
    fresh.close()
    h.close()


def test_incremental_is_full_bit_for_bit():
    c = case("prot4")
    child = so.Tree(c.parent, c.length, [""] * c.n).child
    rng = np.random.default_rng(5)
    h, again = c.history(), c.history()
    assert h.log_like()[0] == again.log_like()[0] and h.log_like()[1].tobytes() == again.log_like()[1].tobytes()      # two runs
    again.close()
    length = list(c.length)
    current = h.log_like()
    n_internal = 0
    for node in range(c.n):
        if not child[node]:
            continue
        n_internal += 1
        nodes = list(child[node]) + ([node] if node != c.n - 1 else [])
        proposed = list(length)
        for r in nodes:
            proposed[r] = float(rng.uniform(.01, .8))
        mats = np.asarray([c.sub_prob(proposed[r]) for r in nodes])
        lp = h.propose(nodes, mats)
        fresh = c.history(branch_sub=c.matrices(proposed))
        want = fresh.log_like()
        fresh.close()
        got = h.log_like(1)
        assert lp == got[0] == want[0] and got[1].tobytes() == want[1].tobytes(), node
        assert want[0] != current[0]
        # the current state is untouched until accept
        still = h.log_like(0)
        assert still[0] == current[0] and still[1].tobytes() == current[1].tobytes(), node
        if node % 2:
            h.reject()
            after = h.log_like(0)
            assert after[0] == current[0] and after[1].tobytes() == current[1].tobytes(), node
        else:
            h.accept()                             # the next proposal builds on this one
            after = h.log_like(0)
            assert after[0] == want[0] and after[1].tobytes() == want[1].tobytes(), node
            length, current = proposed, after
    assert n_internal == 8
    # every branch at once (the rescale move), on top of what was accepted
    nodes = list(range(c.n - 1))
    proposed = [t * 1.37 for t in length]
    lp = h.propose(nodes, np.asarray([c.sub_prob(proposed[r]) for r in nodes]))
    fresh = c.history(branch_sub=c.matrices(proposed))
    assert lp == fresh.log_like()[0] and h.log_like(1)[1].tobytes() == fresh.log_like()[1].tobytes()
    fresh.close()
    h.reject()
    h.close()


# ---- indel counts ----

def _subtree_column(child, root, dropped):
    """presence flags of the column rooted at `root` without the subtrees of `dropped`"""
    n = len(child)
    present, stack = [False] * n, [root]
    while stack:
        r = stack.pop()
        if r in dropped:
            continue
        present[r] = True
        stack.extend(child[r])
    return present


@functools.lru_cache(maxsize=None)
def indel_case():
    rng = np.random.default_rng(31)
    parent, _ = _random_tree(rng, 9)
    n = len(parent)
    child = so.Tree(parent, [0.] * n, [""] * n).child
    internal = [r for r in range(n - 1) if child[r]]
    # p -> r: the planted branch (r internal, so that the column can be rooted below p); e: a subtree absent everywhere
    r_node = next(r for r in internal if parent[r] != n - 1)
    p_node = parent[r_node]
    e_node = next(r for r in internal if r != r_node and r != p_node and r_node not in _descendants(child, r) and r not in _descendants(child, r_node)
                  and p_node not in _descendants(child, r))
    banned = _descendants(child, e_node) | {e_node}
    cols = []
    for _ in range(200):
        root = n - 1 if rng.random() < .6 else int(rng.choice([r for r in range(n) if r not in banned]))
        dropped = {int(r) for r in range(n) if rng.random() < .12 and r != root} | {e_node}
        cols.append(_subtree_column(child, root, dropped))
    match = lambda: _subtree_column(child, n - 1, {e_node})
    delete = lambda: _subtree_column(child, n - 1, {e_node, r_node})
    insert = lambda: _subtree_column(child, r_node, {e_node})
    empty = lambda: _subtree_column(child, e_node, {e_node})
    other = lambda: _subtree_column(child, next(c for c in child[p_node] if c != r_node), {e_node})
    cols[0] = insert()                                       # a leading insertion
    cols[1] = match()
    cols[10], cols[11], cols[12] = delete(), insert(), match()  # Delete then Insert: the deferral reorders it
    cols[59] = match()
    for k in range(60, 131):                                 # 71 columns without a Match, over the block boundaries 64 and 128
        cols[k] = (delete, insert, other, empty)[(k * 7 + k // 5) % 4]()
    cols[131] = match()
    cols[199] = delete()                                     # a trailing deletion
    return parent, child, cols, p_node, r_node, e_node


def _descendants(child, r):
    out, stack = set(), list(child[r])
    while stack:
        k = stack.pop()
        out.add(k)
        stack.extend(child[k])
    return out


def test_indel_counts_equal_as_integers():
    parent, child, cols, p_node, r_node, e_node = indel_case()
    n = len(parent)
    present = [[col[r] for col in cols] for r in range(n)]
    want = HR.indel_counts(parent, present)
    # the planted cases are there
    raw = [(present[p_node][k], present[r_node][k]) for k in range(200)]
    assert raw[0] == (False, True) and raw[199] == (True, False)
    assert raw[10] == (True, False) and raw[11] == (False, True) and raw[12] == (True, True)
    assert not any(a and b for a, b in raw[60:131]) and raw[59] == raw[131] == (True, True)
    assert sum(a != b for a, b in raw[60:64]) and sum(a != b for a, b in raw[64:128]) > 20 and sum(a != b for a, b in raw[128:131])
    assert want[r_node, HR.INSERT, HR.DELETE] >= 1 and want[r_node, HR.DELETE, HR.INSERT] == 0
    for r in child[e_node]:                                  # a branch empty in every column: Start -> End
        assert not any(present[r]) and not any(present[e_node])
        assert want[r].sum() == 1 and want[r, 0, HR.END] == 1
    tokens = np.full((200, n), -2, dtype=np.int8)
    for k, col in enumerate(cols):
        for r in range(n):
            if col[r]:
                tokens[k, r] = -1 if child[r] else (k + r) % 4
    model = hostmodel.RateModel(CYCLIC)
    h = capi.History(parent, np.asarray(model.root, dtype=float).reshape(1, 4), np.zeros(1), tokens, np.tile(np.eye(4), (1, n, 1, 1)))
    got = h.indel_counts()
    assert got.dtype == np.int64 and got.shape == (n, 3, 4)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(h.indel_counts(), want)            # (kept: the alignment is fixed)
    h.close()


# ---- refusals ----

def _code(fn):
    with pytest.raises(capi.HxError) as e:
        fn()
    return e.value.code


def test_every_refusal_and_that_nothing_ran():
    """create's refusals leave no history whose kernel time could be read: the code is what is checked (the launcher
    validates before it allocates); the refusals of an existing history also leave hx_history_last_kernel_ms and the
    stored results unchanged"""
    c = _edge_case(6)
    ok = dict(parent=c.parent, ins_prob=c.ins_prob, log_cpt_weight=c.log_cpt_weight, tokens=c.tokens, branch_sub=c.branch_sub)

    def create(**kw):
        return lambda: capi.History(**dict(ok, **kw))
    assert _code(create(parent=[-1, 0, 0, 1, 1, 2, 2])) == -5                      # parents before children
    assert _code(create(parent=[4, 4, 5, 5, 6, -1, -1])) == -5                     # a second root
    bad = c.tokens.copy()
    bad[3, 2] = 4
    assert _code(create(tokens=bad)) == -8                                         # a token >= A
    three = dict(parent=[3, 3, 3, -1], tokens=np.zeros((2, 4), dtype=np.int8), branch_sub=np.zeros((1, 4, 4, 4)))
    assert _code(create(**three)) == -8                                            # three children
    wide = dict(ins_prob=np.full((1, 65), 1 / 65.), tokens=np.zeros((1, 7), dtype=np.int8), branch_sub=np.zeros((1, 7, 65, 65)))
    assert _code(create(**wide)) == -8                                             # A > 64
    many = dict(ins_prob=np.full((129, 4), .25), log_cpt_weight=np.full(129, -math.log(129)), branch_sub=np.zeros((129, 7, 4, 4)))
    assert _code(create(**many)) == -8                                             # C > 128
    h = c.history()
    ms, state = h.kernel_ms(), h.log_like()
    assert ms > 0
    one = c.branch_sub[:, [0]].transpose(1, 0, 2, 3)
    for node in (-1, 6, 7):                                                        # outside 0 .. N - 2; 6 is the root
        assert _code(lambda: h.propose([node], one)) == -8
    assert _code(h.accept) == -7 and _code(h.reject) == -7                         # nothing pending
    assert _code(lambda: h.log_like(1)) == -7
    assert h.kernel_ms() == ms
    h.propose([0], one * 1.)
    ms2, proposed = h.kernel_ms(), h.log_like(1)
    assert _code(lambda: h.propose([1], one)) == -7                                # a proposal is pending
    assert h.kernel_ms() == ms2
    after = h.log_like(1)
    assert after[0] == proposed[0] and after[1].tobytes() == proposed[1].tobytes()
    h.reject()
    still = h.log_like()
    assert still[0] == state[0] and still[1].tobytes() == state[1].tobytes()
    h.close()


# ---- streams ----

def test_a_history_on_a_delayed_stream():
    """create and propose return when their kernels are done, so "still busy" is checked immediately before each"""
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    c = case("acgt")
    proposed = [t * .8 for t in c.length]
    nodes = [0, 1, c.parent[0]] if c.parent[0] == c.parent[1] else [0, c.parent[0]]
    mats = np.asarray([c.sub_prob(proposed[r]) for r in nodes])
    h = c.history()
    want = (h.log_like(), h.propose(nodes, mats), h.log_like(1))
    h.close()
    streams = SH.Streams()
    try:
        a = streams.new()
        streams.busy(a)
        SH.assert_busy(a, "History")
        h = c.history(stream=SH.handle(a))
        got0 = h.log_like()
        streams.busy(a)
        SH.assert_busy(a, "History.propose")
        lp = h.propose(nodes, mats, stream=SH.handle(a))
        got1 = h.log_like(1)
    finally:
        streams.release()
    h.close()
    assert got0[0] == want[0][0] and got0[1].tobytes() == want[0][1].tobytes()
    assert lp == want[1] == got1[0] and got1[1].tobytes() == want[2][1].tobytes()
