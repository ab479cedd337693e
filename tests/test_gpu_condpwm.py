"""Excluded-neighbour profiles of a resident history (k_history_excluded behind capi.History.excluded_profiles) against the
restatement of SumProduct::logNodeExcludedPostProb (tests/condpwm_ref.py, pinned without a device by
tests/test_oracle_condpwm.py).

Bounds.  The -inf pattern is equal.  A finite unnormalised entry: 1e-12 * max(1, |v|), the column bound of
tests/test_gpu_history.py (the same arithmetic: the device's log() and the order inside the matrix-vector products differ
from libm's and the restatement's).  A normalised entry: 2e-12 * (max(1, |v|) + max(1, |norm|)) - the entry's bound and the
norm's, which is a fold of the table log_sum_exp over entries within the first bound.  Every pair, row and entry is
compared.  Device against device (two calls, one call for many pairs, the slots of a proposal): the same bytes."""
import functools

import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from oracle import sumprod_oracle as so
from tests import condpwm_ref as CR
from tests import history_edge_cases as HE
from tests import stream_helpers as SH
from tests import test_gpu_history as TH
from tests.test_gpu_ancestors import CYCLIC
from tests.test_gpu_history_edges import UNARY_COLUMNS, UNARY_LENGTH, UNARY_PARENT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


WORST = {"unnormalised": 0., "normalised": 0.}


@functools.lru_cache(maxsize=None)
def _maker(fn, *args):
    """fn(*args) as one object per (fn, args), so that _reference's cache finds it again"""
    return functools.partial(fn, *args)


@functools.lru_cache(maxsize=None)
def _reference(make, pairs):
    """the restatement over the case make() for a tuple of pairs, computed once: (v, norm, scaled reads of children,
    scaled reads along the paths)"""
    c = make()
    sp = HE._WayUp(c.omodel, c.tree, c.branch_sub)
    return CR.conditional_pwms_and_norms(sp, c.rows, list(pairs))


def compare(got, want, norm, normalized, what):
    """one pair's profile against the restatement's: shape, the -inf pattern, no NaN, every finite entry within its bound"""
    assert got.shape == want.shape, what
    if normalized:
        want = want - norm[:, None, None]
    assert not np.any(np.isnan(want)) and not np.any(np.isnan(got)), what
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    assert not np.any(np.isposinf(got)), what
    fin = np.isfinite(want)
    dev = np.abs(got[fin] - want[fin])
    if normalized:
        scale = np.maximum(1., np.abs(want)) + np.maximum(1., np.abs(norm))[:, None, None]
        bound, key = 2e-12 * scale[fin], "normalised"
    else:
        bound, key = 1e-12 * np.maximum(1., np.abs(want[fin])), "unnormalised"
    if dev.size:
        WORST[key] = max(WORST[key], float(np.max(dev / bound)))
        assert np.all(dev <= bound), (what, float(np.max(dev / bound)))


def check_pairs(h, make, pairs, what, which=0):
    """both forms of every pair in one call each against the restatement; -> the two lists of arrays"""
    v, norm, _, _ = _reference(make, tuple(pairs))
    lens = h.row_lengths()
    out = []
    for normalized in (False, True):
        got = h.excluded_profiles(pairs, normalize=normalized, which=which)
        assert len(got) == len(pairs)
        for k, (node, exclude) in enumerate(pairs):
            assert got[k].shape[0] == lens[node] == v[k].shape[0], (what, node)
            compare(got[k], v[k], norm[k], normalized, "%s (%d, %d) %s" % (what, node, exclude, "normalised" if normalized else ""))
        out.append(got)
    print("%s: %d pairs; worst so far, in units of the bound: unnormalised %.3g, normalised %.3g" % (what, len(pairs), WORST["unnormalised"], WORST["normalised"]))
    return out


def same_bytes(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- every branch of the 17-node cases ----

NAMED = {name: _maker(TH.case, name) for name in ["prot4", "acgt", "acgtu", "abcdefghijklmnopqrstu"]}


@pytest.mark.parametrize("name", list(NAMED))
def test_every_branch_per_call_and_all_at_once(name):
    make = NAMED[name]
    c = make()
    assert (c.n, len(c.want)) == (17, 130)
    h = c.history()
    before = h.log_like()
    pairs = CR.branch_pairs(c.parent)
    assert len(pairs) == 2 * (c.n - 1)
    raw, normed = check_pairs(h, make, pairs, name)
    assert h.kernel_ms() > 0
    # per branch: the same bytes as the call that names them all
    for node in range(c.n - 1):
        p = c.parent[node]
        for normalized, all_at_once in ((False, raw), (True, normed)):
            got = h.branch_profiles(node, normalize=normalized)
            assert same_bytes(got, all_at_once[2 * node:2 * node + 2]), (node, normalized)
            assert got[0].shape[0] == sum(ch != "-" for ch in c.rows[p]) and got[1].shape[0] == sum(ch != "-" for ch in c.rows[node])
    # the four pairs of NodeAlignMove at an internal node below the root
    child = so.Tree(c.parent, c.length, [""] * c.n).child
    node = next(r for r in range(c.n - 1) if child[r])
    left, right = child[node]
    four = [(left, node), (right, node), (node, c.parent[node]), (c.parent[node], node)]
    check_pairs(h, make, four, name + ", NodeAlignMove")
    after = h.log_like()
    assert after[0] == before[0] and after[1].tobytes() == before[1].tobytes()      # a query writes nothing to the history
    h.close()


# ---- compaction: blocks of 64 columns ----

@functools.lru_cache(maxsize=None)
def _edge(n_cols):
    return TH._edge_case(n_cols)


@pytest.mark.parametrize("n_cols", [1, 64, 65])
def test_one_column_one_block_one_block_and_a_column(n_cols):
    make = _maker(_edge, n_cols)
    h = make().history()
    check_pairs(h, make, CR.branch_pairs(TH.EDGE_PARENT), "edge columns x %d" % n_cols)
    h.close()


@functools.lru_cache(maxsize=None)
def _stretches():
    """200 edge columns: leaf 3 is a gap in all of block 0 and present in block 1; leaf 2 is a gap in the 71 columns
    100 .. 170, across the end of block 1"""
    without3, without2 = ["ac--*--", "a------", "acg-***"], ["ac--*--", "a------", "ac-t***"]
    cols = []
    for k in range(200):
        if k < 64:
            cols.append(without3[k % 3])
        elif 100 <= k <= 170:
            cols.append(without2[k % 3])
        else:
            cols.append(TH.EDGE_COLUMNS[k % len(TH.EDGE_COLUMNS)])
    return TH.Case(CYCLIC, TH.EDGE_PARENT, TH.EDGE_LENGTH, ["".join(col[r] for col in cols) for r in range(7)])


def test_gap_stretches_over_whole_blocks_and_block_boundaries():
    c = _stretches()
    assert set(c.rows[3][:64]) == {"-"} and set(c.rows[3][64:128]) != {"-"}
    assert set(c.rows[2][100:171]) == {"-"} and c.rows[2][99] != "-" and c.rows[2][171] != "-" and 100 < 128 < 170
    h = c.history()
    check_pairs(h, _stretches, CR.branch_pairs(TH.EDGE_PARENT), "gap stretches")
    h.close()


# ---- column roots and tree shapes ----

def _census(c):
    """how often the branches and columns of a case show each situation"""
    n = c.n
    child = so.Tree(c.parent, c.length, [""] * n).child
    roots = HE.column_roots(c)
    tok = np.asarray(c.tokens)
    out = dict(root_is_parent=0, root_between=0, node_is_root=0, sibling_gap=0, leaf_wildcard=0, single_child=0)
    for node in range(n - 1):
        p = c.parent[node]
        out["single_child"] += len(child[p]) == 1
        for k in range(tok.shape[0]):
            if tok[k, node] == -2:
                continue
            out["leaf_wildcard"] += tok[k, node] == -1 and not child[node]
            if tok[k, p] == -2:
                out["node_is_root"] += roots[k] == node
                continue
            out["root_is_parent"] += roots[k] == p
            out["root_between"] += roots[k] not in (p, n - 1)
            out["sibling_gap"] += any(tok[k, s] == -2 for s in child[p] if s != node)
    return out


@functools.lru_cache(maxsize=None)
def _unary():
    cols = [UNARY_COLUMNS[k % len(UNARY_COLUMNS)] for k in range(70)]
    return TH.Case(CYCLIC, UNARY_PARENT, UNARY_LENGTH, ["".join(col[r] for col in cols) for r in range(4)])


def test_the_chosen_alignments_hold_every_column_root_and_tree_shape():
    """a column whose root is the parent itself; one whose root is strictly between the tree's root and the parent; one in
    which the parent is a gap and the node the column's root (a row in the node's profile, none in the parent's); a sibling
    that is a gap; a leaf wildcard - all in `acgt`, which test_every_branch_per_call_and_all_at_once runs; a parent with a
    single child: here"""
    census = _census(TH.case("acgt"))
    print(census)
    assert all(census[k] >= 1 for k in ("root_is_parent", "root_between", "node_is_root", "sibling_gap", "leaf_wildcard")), census
    c = _unary()
    census = _census(c)
    assert census["single_child"] >= 1 and census["node_is_root"] >= 1 and census["root_is_parent"] >= 1, census
    h = c.history()
    raw, _ = check_pairs(h, _unary, CR.branch_pairs(UNARY_PARENT), "a parent with a single child")
    # the parent a gap, the node the column's root: the node's profile has a row more than the parent's per such column
    assert raw[1].shape[0] == sum(ch != "-" for ch in c.rows[0]) and raw[0].shape[0] == sum(ch != "-" for ch in c.rows[1])
    h.close()


# ---- deep paths under both rescaling rules ----

def _cat40():
    return HE.case("cat40 mix12")


@pytest.mark.parametrize("name", ["caterpillar 40, residues, 12 components", "caterpillar 48, wildcards"])
def test_the_deepest_branch_of_a_caterpillar(name):
    """The deepest branch: a path of 39 or more nodes.  The siblings that hang off a caterpillar's spine are leaves, whose
    scale factor is 0 whatever fillUp rescaled; the rescalings enter through the spine child of every branch above, so the
    branches at the top, in the middle and at the bottom of the spine are asked for in the same call, and the oracle
    confirms that rescaled messages were read."""
    make = _cat40 if name.startswith("caterpillar 40") else TH.deep_case
    c = make()
    leaves = (c.n + 1) // 2
    assert leaves == (40 if make is _cat40 else 48)
    assert (c.residue_rescales if make is _cat40 else c.wild_rescales) >= 1
    deepest = leaves                                         # the first internal node: leaves 0 and 1 below it
    depth, r = 1, deepest
    while c.parent[r] >= 0:
        depth, r = depth + 1, c.parent[r]
    assert depth >= 39
    spine = [deepest, leaves + leaves // 2, c.n - 2]
    pairs = []
    for node in [0] + spine:
        pairs += [(c.parent[node], node), (node, c.parent[node])]
    pairs.append((c.n - 1, leaves - 1))                     # the root without its leaf: what is left is the whole spine
    h = c.history()
    check_pairs(h, make, pairs, name)
    assert _reference(make, tuple(pairs))[2] >= 1            # messages with logE != 0 were read
    h.close()


@functools.lru_cache(maxsize=None)
def _double_caterpillar(inside_b):
    """two 48-leaf caterpillars under one root (tests/condpwm_ref.py), 4 columns; arm A with wildcards inside"""
    parent = CR.double_caterpillar(48)
    rng = np.random.default_rng(48)
    length = [float(rng.uniform(.05, .3)) for _ in parent]
    return TH.Case(CYCLIC, parent, length, CR.double_caterpillar_rows(48, "*", inside_b))


@pytest.mark.parametrize("inside", ["wildcards", "residues"])
def test_a_path_that_passes_a_deep_sibling(inside):
    """logG = logG[parent] + logE[sibling] with a scale factor that is not 0: the path from the root into arm A passes
    the top of arm B, below which fillUp rescaled - at wildcards in the one case, at residues in the other (arm B holds
    only the one or the other inside, so only that rule can have fired there).  The oracle confirms it column by column;
    tests/test_oracle_condpwm.py pins the restatement's logG on the same trees."""
    make = _maker(_double_caterpillar, "*" if inside == "wildcards" else "r")
    c = make()
    leaves, arm = 48, 95
    assert c.n == 2 * arm + 1 and c.parent[arm - 1] == c.parent[2 * arm - 1] == c.n - 1
    sp = HE._WayUp(c.omodel, c.tree, c.branch_sub)
    for seq in so.columns_of(c.tree, dict(enumerate(c.rows))):
        sp.init_column(seq)
        sp.fill_up()
        wild, residue, top = CR.arm_b_rescalings(sp, leaves)
        assert top[0] != 0. and ((wild >= 1 and residue == 0) if inside == "wildcards" else (residue >= 1 and wild == 0)), (wild, residue, top)
    depth, r = 1, leaves
    while c.parent[r] >= 0:
        depth, r = depth + 1, c.parent[r]
    assert depth >= 48
    pairs = []
    for node in (0, leaves, leaves + leaves // 2, arm - 1, arm + leaves, 2 * arm - 1):      # both arms: bottom, middle, top
        pairs += [(c.parent[node], node), (node, c.parent[node])]
    pairs += [(leaves, 0), (arm + leaves, arm + 1)]          # the deepest internal node of either arm without one leaf
    h = c.history()
    check_pairs(h, make, pairs, "two caterpillars under one root, %s inside arm B" % inside)
    scaled_children, scaled_path = _reference(make, tuple(pairs))[2:]
    print("scale factors other than 0: %d among the kept children, %d along the paths" % (scaled_children, scaled_path))
    assert scaled_path >= 4 * 4 and scaled_children >= 1      # (the four ways down into arm A, in each of the four columns)
    h.close()


# ---- more components than waves, LDS-limited plans ----

@pytest.mark.parametrize("name", ["anc prot x 9", "anc alphabet 21 x 9", "anc alphabet 64 x 3", "anc 46 x 6"])
def test_two_turns_of_a_wave_and_shed_waves(name):
    make = _maker(HE.case, name)
    c = make()
    plan = HE.history_plan(c.a, c.c)
    assert {k: plan[k] for k in c.plan} == c.plan and plan["turns"] == 2
    h = c.history()
    check_pairs(h, make, CR.branch_pairs(c.parent), name)
    h.close()


# ---- a zero-length branch ----

@functools.lru_cache(maxsize=None)
def _zero_lengths():
    length = list(TH.EDGE_LENGTH)
    length[0] = length[5] = 0.
    return TH.Case(CYCLIC, TH.EDGE_PARENT, length, _edge(65).rows)


def test_zero_length_branches():
    """exp(R 0) is the identity: log 0 in the messages of a residue leaf, -inf entries in the profiles of wildcards"""
    c = _zero_lengths()
    assert np.array_equal(c.branch_sub[0, 0], np.eye(4)) and np.array_equal(c.branch_sub[0, 5], np.eye(4))
    pairs = CR.branch_pairs(TH.EDGE_PARENT)
    v = _reference(_zero_lengths, tuple(pairs))[0]
    wild = [k for k, (node, _) in enumerate(pairs) if node >= 4]
    rows4 = np.asarray([ch == "*" for ch in c.rows[4] if ch != "-"])
    k40 = pairs.index((4, 1))                                # node 4 without leaf 1: what is left below it is leaf 0, at distance 0
    assert k40 in wild and np.any(np.isneginf(v[k40][rows4])) and np.all(np.isfinite(v[k40][rows4]).sum(axis=2) >= 1)
    h = c.history()
    check_pairs(h, _zero_lengths, pairs, "zero-length branches")
    h.close()


# ---- the slots of a proposal ----

def test_slots_after_the_random_walk():
    """The 60 proposals of tests/history_edge_cases.py drive message slots and matrix slots apart; then a proposal on an
    internal node and its children: which = 0 keeps the bytes from before, which = 1 has the bytes of a history created on
    the proposed matrices; accept moves them to which = 0, a rejected proposal leaves them there."""
    c = HE.case(HE.WALK)
    h = c.history()
    mats = c.branch_sub.copy()
    for nodes, ts, accepted in HE.walk_steps(c.n):
        new = np.asarray([c.sub_prob(t) for t in ts])
        h.propose(nodes, new)
        if accepted:
            h.accept()
            mats[:, nodes] = new.transpose(1, 0, 2, 3)
        else:
            h.reject()
    pairs = CR.branch_pairs(c.parent)

    def both(hist, which=0):
        return [hist.excluded_profiles(pairs, normalize=n, which=which) for n in (False, True)]

    def fresh(m):
        f = c.history(branch_sub=m)
        out = both(f)
        f.close()
        return out

    def same(a, b):
        return same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    state = h.log_like()
    old = both(h)
    assert same(old, fresh(mats))
    child = so.Tree(c.parent, c.length, [""] * c.n).child
    node = next(r for r in range(c.n - 1) if child[r])
    nodes = [node] + list(child[node])
    new = np.asarray([c.sub_prob(t) for t in (.27, .41, .13)][:len(nodes)])
    proposed = mats.copy()
    proposed[:, nodes] = new.transpose(1, 0, 2, 3)
    h.propose(nodes, new)
    pending = h.log_like(1)
    want = fresh(proposed)
    assert not same(old, want)
    assert same(both(h, 0), old) and same(both(h, 1), want)
    now = h.log_like(0), h.log_like(1)
    assert now[0][0] == state[0] and now[0][1].tobytes() == state[1].tobytes()
    assert now[1][0] == pending[0] and now[1][1].tobytes() == pending[1].tobytes()
    h.accept()
    assert same(both(h), want)
    again = np.asarray([c.sub_prob(t) for t in (.6, .05, .33)][:len(nodes)])
    h.propose(nodes, again)
    assert same(both(h, 0), want) and not same(both(h, 1), want)
    h.reject()
    assert same(both(h), want)
    after = h.log_like()
    assert after[0] == pending[0] and after[1].tobytes() == pending[1].tobytes()
    h.close()


# ---- determinism, streams ----

def test_two_calls_and_a_delayed_stream_give_the_same_bytes():
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    c = TH.case("acgt")
    pairs = CR.branch_pairs(c.parent)
    h = c.history()
    want = [h.excluded_profiles(pairs, normalize=n) for n in (False, True)]
    again = [h.excluded_profiles(pairs, normalize=n) for n in (False, True)]
    assert same_bytes(want[0], again[0]) and same_bytes(want[1], again[1])
    streams = SH.Streams()
    try:
        a = streams.new()
        got = []
        for n in (False, True):
            streams.busy(a)
            SH.assert_busy(a, "History.excluded_profiles")
            got.append(h.excluded_profiles(pairs, normalize=n, stream=SH.handle(a)))
    finally:
        streams.release()
    h.close()
    assert same_bytes(want[0], got[0]) and same_bytes(want[1], got[1])


# ---- refusals ----

def test_every_refusal_and_that_nothing_ran():
    c = _edge(6)
    h = c.history()
    ms, state = h.kernel_ms(), h.log_like()

    def code(pairs, **kw):
        return TH._code(lambda: h.excluded_profiles(pairs, **kw))
    for pair in ((-1, 4), (7, 4), (0, -1), (0, 7), (6, -1)):                      # outside 0 .. N - 1 (the root's parent is -1)
        assert code([pair]) == capi.HX_ERR_RANGE == -8
    assert TH._code(lambda: h.branch_profiles(6)) == -8                             # the root has no branch
    for pair in ((0, 1), (0, 6), (4, 5), (0, 0), (6, 0)):                         # neither parent nor child
        assert code([pair]) == capi.HX_ERR_INVALID_ARG == -1
    assert code([(4, 0), (0, 1)]) == -1                                           # one bad pair among good ones
    assert code([]) == -1                                                         # no pairs
    assert code([(4, 0)], which=2) == -1
    assert code([(4, 0)], which=1) == -7                     # nothing is pending
    lib = capi.load()
    assert lib.hx_history_excluded_profiles(h._h, 0, 1, None, None, 0, None, None) == -1
    assert lib.hx_history_row_lengths(h._h, None) == -1 and lib.hx_history_row_lengths(None, None) == -1
    assert h.kernel_ms() == ms
    still = h.log_like()
    assert still[0] == state[0] and still[1].tobytes() == state[1].tobytes()
    # a valid query afterwards, and the lengths
    assert h.row_lengths().tolist() == [sum(ch != "-" for ch in row) for row in c.rows]
    check_pairs(h, _maker(_edge, 6), CR.branch_pairs(TH.EDGE_PARENT), "after the refusals")
    assert h.kernel_ms() > 0
    h.close()


def test_print_the_worst_deviations():
    """(last in the file: what the tests above have seen, in units of their bounds)"""
    print("worst deviation / bound: unnormalised %.3g, normalised %.3g" % (WORST["unnormalised"], WORST["normalised"]))
    assert WORST["unnormalised"] <= 1. and WORST["normalised"] <= 1.
