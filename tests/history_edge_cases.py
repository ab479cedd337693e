"""The named cases of the resident history's edge tests: more than eight mixture components (a wave takes several), LDS
plans that shed waves down to the corner of the ABI (64 symbols x 128 components: one wave, exactly 96 KB), the general
kernel at even and large alphabets, trees deep enough for the reference's 1e-30 rescaling under a proposal, enough
columns for several additions per thread of the sum.  Shared by tests/test_oracle_history_edges.py (which pins the
yardstick without a device: every case takes the launch plan it names, the rescaling does fire before and after the deep
proposals, the random walk covers what it is there for) and by tests/test_gpu_history_edges.py.

Models, trees, columns and the 64 symbols are those of tests/sumprod_edge_cases.py; the oracle side is
tests/test_gpu_history.py's Case.  `history_plan` restates hx_history_create's decisions (historian_amd/csrc/hx_history.hip,
sp_column_plan in hx_sumprod.h); the names next to it are the functions and kernels it restates."""
import copy
import functools
import math

import numpy as np

from oracle import sumprod_oracle as so
from tests import sumprod_edge_cases as EC
from tests import test_gpu_history as TH
from tests.test_gpu_ancestors import _recon_columns
from tests.test_gpu_sumprod import _random_tree


def history_plan(a, c):
    """hx_history_create: the kernel, the waves of a workgroup, the components a wave takes in turn, the dynamic LDS"""
    waves = min(c, 8)                                                    # sp_column_plan: waves
    while waves > 1 and 512 * c + waves * 8 * a * a > 96 * 1024:         # sp_column_plan(shed_waves): ll_lds + waves mat_lds
        waves -= 1
    return dict(ta=a if a in (4, 20) else 0, waves=waves, turns=-(-c // waves),       # history_run's launch; k_history_columns: cpt += Wb
                lds=512 * c + waves * 8 * a * a)                         # sp_column_plan: lds


def sum_plan(n_cols):
    """k_history_sum: the additions of a thread, fewest and most; the blocks of the column kernel"""
    return dict(per_thread=(n_cols // 1024, -(-n_cols // 1024)), blocks=-(-n_cols // 64))


# name -> what hx_history_create must plan for it (a subset of history_plan's keys)
HISTORY = {
    "anc alphabet 64 x 3": dict(ta=0, waves=2, turns=2),                 # shed 3 -> 2; f and e1 of 64 entries
    "anc 46 x 6": dict(ta=0, waves=5, turns=2),                          # shed 6 -> 5; an even alphabet in the general kernel
    "anc prot x 9": dict(ta=20, waves=8, turns=2),
    "anc alphabet 21 x 9": dict(ta=0, waves=8, turns=2),                 # an odd alphabet: a padding entry per vector
    "anc cat64 mix12": dict(ta=4, waves=8, turns=2),                     # rescaling at wildcards with C > 8
    "cat40 mix12": dict(ta=4, waves=8, turns=2),                         # rescaling at residues with C > 8
    "alphabet 16": dict(ta=0, waves=1, turns=1),
    "alphabet 32": dict(ta=0, waves=1, turns=1),
    "limit 64 x 128": dict(ta=0, waves=1, turns=128, lds=96 * 1024),     # the corner of the ABI
    "dna x 128": dict(ta=4, waves=8, turns=16, lds=64 * 1024 + 8 * 8 * 16),
    "many columns": dict(ta=4, waves=1, turns=1),                        # sum_plan: 4 or 5 additions per thread, 66 blocks
}
NEW = {"limit 64 x 128": (EC.SYMBOLS, 128), "dna x 128": ("acgt", 128)}  # 128-component mixtures on "random 3", 70 columns
DEEP = ("anc cat64 mix12", "cat40 mix12")
TWO_LEAVES = ("anc alphabet 64 x 3", "anc 46 x 6", "limit 64 x 128", "dna x 128")
WALK = "anc prot x 9"
SEED = {name: 300 + k for k, name in enumerate(HISTORY)}


class _WayUp(so.SumProduct):
    """The oracle's SumProduct for init_column and fill_up alone, on given matrices exp(R t): without the eigenvector
    counts of every branch that its constructor prepares for the way down (seconds at 128 components of 64 symbols)."""

    def __init__(self, model, tree, branch_sub):
        self.model, self.tree = model, tree
        self.C, self.A, self.N = model.components(), len(model.alphabet), tree.nodes()
        self.pre = tree.preorder()
        self.post = self.pre[::-1]
        self.ins_prob = [np.asarray(p, dtype=float) for p in model.ins_prob]
        self.log_cpt_weight = [math.log(w) for w in model.cpt_weight]
        self.branch_sub = [[branch_sub[cpt, r] for r in range(self.N)] for cpt in range(self.C)]
        self.E = [[np.zeros(self.A) for _ in range(self.N)] for _ in range(self.C)]
        self.F = [[np.zeros(self.A) for _ in range(self.N)] for _ in range(self.C)]
        self.logE = [[0.] * self.N for _ in range(self.C)]
        self.logF = [[0.] * self.N for _ in range(self.C)]
        self.cpt_log_like = [0.] * self.C
        self.col_log_like = -math.inf


class EdgeCase(TH.Case):
    """Case with both rescaling rules counted and the plan the case is there for; `on` gives the same case on other
    branch lengths without building the model again."""

    def __init__(self, js, parent, length, rows, plan):
        super().__init__(js, parent, length, rows, probe=True)
        self.plan = plan

    def on(self, length):
        """the oracle's columns on other branch lengths: a copy that shares the model and the tokens"""
        new = copy.copy(self)
        new.length = list(length)
        new.tree = so.Tree(self.parent, new.length, ["n%d" % k for k in range(self.n)])
        new.branch_sub = self.matrices(new.length)
        sp = _WayUp(self.omodel, new.tree, new.branch_sub)
        new.want, new.wild_rescales, new.residue_rescales = [], 0, 0
        for seq in so.columns_of(new.tree, dict(enumerate(self.rows))):
            sp.init_column(seq)
            sp.fill_up()
            new.want.append(sp.col_log_like)
            new._probe(sp)
        return new


@functools.lru_cache(maxsize=None)
def case(name):
    """built once per process, never modified"""
    if name in NEW:
        alphabet, cpts = NEW[name]
        rng = np.random.default_rng(SEED[name])
        js = EC.mixture(rng, alphabet, cpts, True)
        parent, length = _random_tree(rng, 3)
        return EdgeCase(js, parent, length, _recon_columns(rng, parent, alphabet, 70), HISTORY[name])
    s = EC.spec(name)
    return EdgeCase(s.js, s.parent, s.length, s.rows, HISTORY[name])


# ---- proposals ----

def walked_nodes(parent, nodes):
    """hx_history_propose: the changed nodes and their ancestors, ascending"""
    out = set()
    for r in nodes:
        while r >= 0 and r not in out:
            out.add(r)
            r = parent[r]
    return sorted(out)


def column_roots(c):
    """the root of every column, -1 in a column of gaps"""
    tok = np.asarray(c.tokens)
    roots = np.full(tok.shape[0], -1)
    for r, p in enumerate(c.parent):
        here = (tok[:, r] != -2) & ((tok[:, p] == -2) if p >= 0 else True)
        roots[here] = r
    return roots


def deep_proposals(c):
    """Three proposals on a caterpillar (leaves 0 .. L - 1, the spine L .. 2 L - 2): leaf 0's branch (the whole spine is
    walked, every other leaf is read from its current slot), the top leaf's (only the root is walked), a leaf in the
    middle with a spine node a quarter of the tree above it (the marking of the leaf's ancestors stops at that node).
    -> [(nodes, new lengths, accepted)]: the first is accepted, the second rejected, the third made on the first."""
    leaves = (c.n + 1) // 2
    mid = leaves // 2
    above = c.parent[mid] + leaves // 4
    assert above < c.n - 1 and above in walked_nodes(c.parent, [mid])
    return [([0], [.45], True), ([leaves - 1], [.07], False), ([above, mid], [.38, .21], True)]


@functools.lru_cache(maxsize=None)
def deep_states(name):
    """the oracle after each of the deep proposals: [(nodes, proposed case, accepted)]"""
    c = case(name)
    length, out = list(c.length), []
    for nodes, ts, accepted in deep_proposals(c):
        proposed = list(length)
        for r, t in zip(nodes, ts):
            proposed[r] = t
        out.append((nodes, c.on(proposed), accepted))
        if accepted:
            length = proposed
    return out


@functools.lru_cache(maxsize=None)
def two_leaf_states(name):
    """two unrelated leaves (the first and the last), accepted, then every branch at once on top of that"""
    c = case(name)
    leaves = (c.n + 1) // 2
    first = list(c.length)
    first[0], first[leaves - 1] = .33, .09
    second = [t * 1.37 for t in first]
    return [([0, leaves - 1], c.on(first)), (list(range(c.n - 1)), c.on(second))]


WALK_STEPS, WALK_SEED = 60, 4


def walk_steps(n, seed=WALK_SEED, steps=WALK_STEPS):
    """The random walk: each step a non-empty subset of 0 .. n - 2 in the order drawn (one node, two nodes, all of them
    or any number), every branch length uniform in (.01, .8), accepted with probability 1/2.
    -> [(nodes, lengths, accepted)]; a function of the generator alone"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        size = (1, 2, n - 1, int(rng.integers(1, n)))[int(rng.integers(0, 4))]
        nodes = [int(r) for r in rng.choice(n - 1, size, replace=False)]
        out.append((nodes, [float(rng.uniform(.01, .8)) for _ in nodes], bool(rng.random() < .5)))
    return out


def walk_coverage(parent, steps):
    """what the walk is there for: accepts, rejects; the steps that name a single child of the root; those that name a
    node together with an ancestor other than its parent; per node, the accepted steps that walked it without changing
    its branch (after each of them the node's message slot and its matrix slot have moved apart by one more flip)"""
    n = len(parent)
    drift = [0] * n
    root_child = far_ancestor = 0
    for nodes, _, accepted in steps:
        root_child += len(nodes) == 1 and parent[nodes[0]] == n - 1
        named = set(nodes)
        far_ancestor += len(nodes) < n - 1 and any(set(walked_nodes(parent, [parent[r]])[1:]) & named for r in nodes)
        if accepted:
            for r in walked_nodes(parent, nodes):
                drift[r] += r not in named
    inner = sorted(set(p for p in parent if p >= 0))
    return dict(accepts=sum(s[2] for s in steps), rejects=sum(not s[2] for s in steps), root_child=root_child,
                far_ancestor=far_ancestor, sizes=set(len(s[0]) for s in steps), drift=[drift[r] for r in inner])
