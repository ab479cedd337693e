"""The resident history (hx_history.hip behind capi.History) where it takes another path than on the shapes of
tests/test_gpu_history.py: the cases of tests/history_edge_cases.py (pinned without a device by
tests/test_oracle_history_edges.py) - a wave that takes several mixture components in turn, LDS plans that shed waves
down to one wave and exactly 96 KB, the general kernel at 16, 32, 46 and 64 symbols, both rescaling rules with more than
eight components and under proposals, proposals of other shapes than a node and its children, a random walk of accepts
and rejects that drives a node's message slot and matrix slot apart, a sum of more than one column per thread, the second
round of the column kernel's grid, columns of gaps, a node with one child, a node named twice.

Against the oracle: the bounds of tests/test_gpu_history.py, unchanged (column_bound, Case.check's bound of the sum).
Device against device, bit for bit: two histories of the same inputs; a proposal and a history created on the proposed
matrices; the columns whose root a proposal does not walk; lp_sub and tests/history_ref.py's restatement of
k_history_sum over the device's own column likelihoods; the history and hx_sumprod_ancestors, which run the same way up
(hx_sumprod.h), on the same inputs."""
import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import history_edge_cases as HE
from tests import history_ref as HR
from tests import sumprod_edge_cases as EC
from tests import test_gpu_history as TH
from tests.test_gpu_ancestors import CYCLIC, _recon_columns
from tests.test_gpu_sumprod import _random_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def same(a, b):
    """(lp_sub, col_log_like) twice: the same bits"""
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


def created(c):
    """(lp_sub, col_log_like) of a history created on the case's matrices"""
    h = c.history()
    out = h.log_like()
    h.close()
    return out


def propose(h, new, nodes):
    """propose `nodes` with the matrices of the case `new`; -> (lp_sub, col_log_like) of the proposal, checked against the
    sum restated and against a history created on `new`"""
    lp = h.propose(nodes, new.branch_sub[:, nodes].transpose(1, 0, 2, 3))
    got = h.log_like(1)
    assert lp == got[0] == HR.history_sum(got[1])
    assert same(got, created(new)), nodes
    return got


# ---- a. the full evaluation of every case ----

@pytest.mark.parametrize("name", list(HE.HISTORY))
def test_edge_cases_in_full_against_the_oracle(name):
    c = HE.case(name)
    plan = HE.history_plan(c.a, c.c)
    assert {k: plan[k] for k in c.plan} == c.plan
    h = c.history()
    lp, cll = h.log_like()
    print(plan, end=" ")
    c.check(lp, cll, what=name)
    assert h.kernel_ms() > 0
    assert same(created(c), (lp, cll))                       # two runs
    assert lp == HR.history_sum(cll)                         # the order of the sum, every column in it
    h.close()


# ---- b. proposals on the edge plans ----

@pytest.mark.parametrize("name", HE.DEEP)
def test_deep_proposals_under_both_rescaling_rules(name):
    """leaf 0 (the whole spine walked, every other leaf read from its current slot), accepted; the top leaf (only the
    root walked), rejected; a leaf in the middle with a spine node well above it, on the accepted state"""
    c = HE.case(name)
    roots = HE.column_roots(c)
    h = c.history()
    current = h.log_like()
    c.check(*current, what=name)
    for nodes, new, accepted in HE.deep_states(name):
        assert (new.wild_rescales if name.startswith("anc") else new.residue_rescales) >= 1
        got = propose(h, new, nodes)
        new.check(*got, what="%s, proposed %s" % (name, nodes))
        # columns whose root was not walked keep their bits; the others (full columns among them) change
        kept = ~np.isin(roots, HE.walked_nodes(c.parent, nodes))
        assert kept.sum() >= 3 and got[1][kept].tobytes() == current[1][kept].tobytes()
        assert np.any(got[1][~kept] != current[1][~kept])
        assert same(h.log_like(0), current)                  # the current state is untouched until accept
        if accepted:
            h.accept()
            current = got
        else:
            h.reject()
        assert same(h.log_like(0), current)
    h.close()


@pytest.mark.parametrize("name", HE.TWO_LEAVES)
def test_two_unrelated_leaves_then_every_branch(name):
    c = HE.case(name)
    (nodes, first), (every, second) = HE.two_leaf_states(name)
    roots = HE.column_roots(c)
    h = c.history()
    current = h.log_like()
    got = propose(h, first, nodes)
    first.check(*got, what="%s, proposed %s" % (name, nodes))
    kept = ~np.isin(roots, HE.walked_nodes(c.parent, nodes))
    assert got[1][kept].tobytes() == current[1][kept].tobytes() and np.any(got[1][~kept] != current[1][~kept])
    assert same(h.log_like(0), current)
    h.accept()
    assert same(h.log_like(0), got)
    current = got
    got = propose(h, second, every)
    second.check(*got, what="%s, every branch" % name)
    assert same(h.log_like(0), current)
    h.accept()
    assert same(h.log_like(0), got)
    h.close()


# ---- c. a random walk ----

def test_a_random_walk_of_sixty_proposals():
    """13 nodes, 70 columns, 9 components of 20 symbols.  Every step against a history created on the proposed matrices;
    the walk's coverage depends on the generator alone (tests/test_oracle_history_edges.py asserts it too)."""
    c = HE.case(HE.WALK)
    steps = HE.walk_steps(c.n)
    cover = HE.walk_coverage(c.parent, steps)
    assert len(steps) == 60 and cover["accepts"] >= 10 and cover["rejects"] >= 10
    assert cover["root_child"] >= 1 and cover["far_ancestor"] >= 1 and {1, 2, c.n - 1} <= cover["sizes"]
    assert min(cover["drift"]) >= 2          # every internal node: walked, its branch unchanged, accepted - twice or more
    h = c.history()
    current, mats, length = h.log_like(), c.branch_sub, list(c.length)
    for k, (nodes, ts, accepted) in enumerate(steps):
        new = np.asarray([c.sub_prob(t) for t in ts])
        proposed = mats.copy()
        proposed[:, nodes] = new.transpose(1, 0, 2, 3)
        lp = h.propose(nodes, new)
        fresh = c.history(branch_sub=proposed)
        want = fresh.log_like()
        fresh.close()
        got = h.log_like(1)
        assert lp == got[0] and same(got, want), (k, nodes)
        assert same(h.log_like(0), current), (k, nodes)
        if accepted:
            h.accept()
            current, mats = got, proposed
            for r, t in zip(nodes, ts):
                length[r] = t
        else:
            h.reject()
        assert same(h.log_like(0), current), (k, nodes, accepted)
    final = c.on(length)
    assert np.array_equal(final.branch_sub, mats)
    final.check(*h.log_like(), what="the walk's last state")
    h.close()


# ---- d. columns and trees the ABI accepts ----

def _gapped_edge_case(js, n_cols=130):
    """the edge columns of tests/test_gpu_history.py with columns of gaps first, at either side of the first block's end, last"""
    gaps = (0, 63, 64, n_cols - 1)
    cols = ["-------" if k in gaps else TH.EDGE_COLUMNS[k % len(TH.EDGE_COLUMNS)] for k in range(n_cols)]
    return (lambda length: TH.Case(js, TH.EDGE_PARENT, length, ["".join(col[r] for col in cols) for r in range(7)])), gaps


def _dna3():
    return EC.mixture(np.random.default_rng(33), "acgt", 3, False)


@pytest.mark.parametrize("model", ["cyclic", "mixture of 3"])
def test_columns_of_gaps(model):
    """the likelihood of a column of gaps is log sum w: 0.0 for one component; for three, what the reference's table of
    log(1 + exp(-x)) makes of it, 3e-10 in the oracle (the floor of column_bound applies).  A proposal writes it anew with
    the same bits; the sum counts it."""
    make, gaps = _gapped_edge_case(CYCLIC if model == "cyclic" else _dna3())
    c = make(TH.EDGE_LENGTH)
    assert HE.column_roots(c)[list(gaps)].tolist() == [-1] * 4
    if model == "cyclic":
        assert [c.want[k] for k in gaps] == [0.] * 4
    else:
        assert all(0. < abs(c.want[k]) < 1e-6 for k in gaps)
    h = c.history()
    current = h.log_like()
    c.check(*current, what="columns of gaps, " + model)
    assert current[0] == HR.history_sum(current[1])
    length = list(TH.EDGE_LENGTH)
    length[4], length[0], length[1] = .07, .28, .38
    new = make(length)
    got = propose(h, new, [4, 0, 1])
    new.check(*got, what="columns of gaps, %s, proposed" % model)
    for k in gaps:
        assert got[1][k].tobytes() == current[1][k].tobytes()
    present = [[t != -2 for t in c.tokens[:, r]] for r in range(c.n)]
    assert np.array_equal(h.indel_counts(), HR.indel_counts(c.parent, present))      # (pairPath drops the columns of gaps)
    h.close()


UNARY_PARENT, UNARY_LENGTH = [1, 3, 3, -1], [.1, .2, .3, 0.]        # leaf 0 under node 1, its only child; leaf 2; the root 3
UNARY_COLUMNS = ["acg*", "a*g*", "a*gt",     # a residue, a wildcard at the node with one child
                 "--g*", "a---",             # a gap there: the column lives beside it, or below it
                 "ac--", "a*--",             # the column's root
                 "-*g*", "-c-*"]             # its child is a gap: a leaf of the column


@pytest.mark.parametrize("model", ["cyclic", "mixture of 3"])
def test_a_node_with_one_child(model):
    js = CYCLIC if model == "cyclic" else _dna3()
    cols = [UNARY_COLUMNS[k % len(UNARY_COLUMNS)] for k in range(70)]
    rows = ["".join(col[r] for col in cols) for r in range(4)]
    c = TH.Case(js, UNARY_PARENT, UNARY_LENGTH, rows)
    assert sorted(set(HE.column_roots(c).tolist())) == [0, 1, 3]
    h = c.history()
    current = h.log_like()
    c.check(*current, what="one child, " + model)
    assert current[0] == HR.history_sum(current[1])
    new = TH.Case(js, UNARY_PARENT, [.35, .2, .3, 0.], rows)
    got = propose(h, new, [0])
    new.check(*got, what="one child, %s, proposed" % model)
    for k, col in enumerate(cols):                           # the columns without leaf 0: the same operands, the same bits
        assert (got[1][k] == current[1][k]) == (col[0] == "-" or col == "a---"), k
    h.accept()
    assert same(h.log_like(0), got)
    present = [[ch != "-" for ch in row] for row in rows]
    assert np.array_equal(h.indel_counts(), HR.indel_counts(UNARY_PARENT, present))
    h.close()


# ---- e. the second round of the column kernel's grid ----

def _within_bounds(c, cll):
    want = np.asarray(c.want)
    return np.all(np.abs(cll - want) <= np.asarray([TH.column_bound(w) for w in c.want]))


def test_more_blocks_of_columns_than_the_grid_has_workgroups():
    """65 536 blocks of 64 columns and 70 more: the grid is 65 535 workgroups, so workgroups 0, 1 and 2 take a second block
    (the last one ragged: 6 columns).  3 leaves, 5 nodes, Jukes-Cantor; a pattern of 192 reconstruction columns tiled.  Device memory:
    2 C N (A' + 1) = 50 doubles per column, 1.7 GB for the 4 194 374 columns (twice that while the proposal is compared
    with a freshly created history)."""
    period, n_cols = 192, 65536 * 64 + 70
    rng = np.random.default_rng(65536)
    parent, length = _random_tree(rng, 3)
    rows = _recon_columns(rng, parent, "acgt", period)
    c = TH.Case(EC.JUKES_CANTOR, parent, length, rows)
    tokens = np.tile(c.tokens, (-(-n_cols // period), 1))[:n_cols]
    assert tokens.shape == (n_cols, 5) and -(-n_cols // 64) == 65538 > 65535
    proposed = list(length)
    proposed[0] = .44
    new = TH.Case(EC.JUKES_CANTOR, parent, proposed, rows)
    assert new.want != c.want

    def check(case, lp, cll, what):
        assert _within_bounds(case, cll[:period]), what
        assert cll[period:].tobytes() == cll[:-period].tobytes(), what        # a lane's arithmetic does not depend on its block
        assert lp == HR.history_sum(cll), what

    h = c.history(tokens=tokens)
    check(c, *h.log_like(), what="created")
    lp = h.propose([0], new.branch_sub[:, [0]].transpose(1, 0, 2, 3))
    got = h.log_like(1)
    assert lp == got[0]
    check(new, *got, what="proposed")
    h.close()
    fresh = new.history(tokens=tokens)
    assert same(fresh.log_like(), got)
    fresh.close()


# ---- f. refusals ----

def test_a_node_named_twice_is_refused_and_nothing_ran():
    c = TH._edge_case(6)
    h = c.history()
    ms, state = h.kernel_ms(), h.log_like()
    two = c.branch_sub[:, [2, 2]].transpose(1, 0, 2, 3) * 1.
    assert TH._code(lambda: h.propose([2, 2], two)) == capi.HX_ERR_INVALID_ARG == -1
    assert TH._code(lambda: h.propose([0, 2, 0], c.branch_sub[:, [0, 2, 0]].transpose(1, 0, 2, 3))) == -1
    assert h.kernel_ms() == ms and same(h.log_like(), state)
    assert TH._code(lambda: h.log_like(1)) == -7             # nothing is pending
    length = list(TH.EDGE_LENGTH)
    length[2] = .4
    new = TH.Case(CYCLIC, TH.EDGE_PARENT, length, c.rows)
    got = propose(h, new, [2])                               # a valid proposal afterwards
    new.check(*got, what="after the refusal")
    assert same(h.log_like(0), state)
    h.close()


# ---- g. one way up: the history and hx_sumprod_ancestors on the same inputs ----

@pytest.mark.parametrize("name", ["anc cat64 mix12", "anc bal64 prot4", "anc alphabet 21 x 9"])
def test_the_history_and_the_ancestors_kernel_share_the_way_up(name):
    """Both kernels run the tip-to-root steps of hx_sumprod.h; where their launchers pick the same form (the alphabet's
    kernel, the matrices in LDS) the column likelihoods are the same bits, and lp_sub is their sum in k_history_sum's
    order.  70 columns each (a ragged second block): 4 symbols x 12 components on a caterpillar of 64 leaves under
    wildcards (two turns of a wave, rescaling), 20 x 4 on a balanced 64-leaf tree, 21 x 9 on seven leaves (the general
    kernel, two turns).  46 x 6 and 64 x 3 are not here: there the ancestors' matrices come through the scalar cache and
    the history sheds a wave, and the two forms add in different orders by design."""
    s = EC.spec(name)
    c = HE.case(name) if name in HE.HISTORY else TH.Case(s.js, s.parent, s.length, s.rows)
    hp, ap = HE.history_plan(c.a, c.c), EC.ancestors_plan(c.a, c.c)
    assert s.n_cols == 70 and ap["lm"] and hp["waves"] == ap["waves"] == min(c.c, 8) and hp["ta"] == ap["ta"]
    assert hp["lds"] == 512 * c.c + 8 * c.a * c.a * min(c.c, 8)       # every wave's matrix in LDS, as lm says of the ancestors' plan
    h = c.history()
    lp, cll = h.log_like()
    h.close()
    got = capi.sumprod_ancestors(c.parent, c.ins_prob, c.log_cpt_weight, c.branch_sub, c.tokens)[0]
    differ = np.flatnonzero(cll != got)
    assert cll.tobytes() == got.tobytes(), "first differing column %d: %r, %r" % (differ[0], cll[differ[0]], got[differ[0]])
    assert lp == HR.history_sum(got)
