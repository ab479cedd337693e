"""The named cases of the sum-product edge tests: trees deep enough for the reference's 1e-30 rescaling, more than eight
mixture components, matrices that do not fit the LDS plan, alphabet sizes at the edges of the outer-product kernels' plans,
enough columns for a second slice of the row sums.  Shared by tests/test_oracle_sumprod_edges.py (which pins the yardstick
on them: the rescaling does fire, the oracle itself does not underflow, every case takes the launch plan it names) and by
tests/test_gpu_sumprod_edges.py and tests/test_gpu_ancestors_edges.py.

`counts_plan` and `ancestors_plan` restate the launchers' decisions (hx_sumprod_columns in historian_amd/csrc/hx_sumprod.hip,
hx_sumprod_ancestors in hx_ancestors.hip; sp_column_plan and sp_chunk in hx_sumprod.h); the names next to them are
the functions and kernels they restate.

Alphabets of more than 36 symbols: tokenize_columns and the oracle's tokenizer fold case, and '-', '.', '*' and the
counts columns' wildcard 'x' have meanings of their own, so the 64 symbols are the lower-case letters without 'x', the
digits and the 29 punctuation characters that are left.  Both model loaders take them as they take letters."""
import functools
import json
import math
import os

import numpy as np

from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from tests.test_gpu_ancestors import CYCLIC, _recon_columns
from tests.test_gpu_sumprod import _random_columns, _random_model, _random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROT4 = os.path.join(ROOT, "tests", "golden", "models", "prot4.json")
AA = "arndcqeghilkmfpstwyv"
SYMBOLS = "abcdefghijklmnopqrstuvwyz0123456789" + "".join(chr(k) for k in range(33, 127) if not chr(k).isalnum() and chr(k) not in "-.*")
assert len(SYMBOLS) == 64 and len(set(SYMBOLS.lower())) == 64
JUKES_CANTOR = {"alphabet": "acgt", "insrate": .01, "delrate": .01, "insextprob": .5, "delextprob": .5,
                "rootprob": {c: .25 for c in "acgt"}, "subrate": {c: {d: 1. for d in "acgt" if d != c} for c in "acgt"}}


# ---- trees: children before parents, the root last; branch lengths uniform(.02, .6) ----

def _lengths(rng, n):
    return [float(rng.uniform(.02, .6)) for _ in range(n)]


def balanced(leaves, rng):
    parent, level = [-1] * leaves, list(range(leaves))
    while len(level) > 1:
        above = []
        for k in range(0, len(level) - 1, 2):
            parent.append(-1)
            parent[level[k]] = parent[level[k + 1]] = len(parent) - 1
            above.append(len(parent) - 1)
        level = above + level[len(level) & ~1:]              # (an odd one out joins the next level)
    return parent, _lengths(rng, len(parent))


def caterpillar(leaves, rng):
    """leaves 0 and 1 under the first spine node; every further leaf joins the spine one node higher"""
    parent = [-1] * leaves
    for leaf in range(1, leaves):
        parent.append(-1)
        below = 0 if leaf == 1 else len(parent) - 2
        parent[below] = parent[leaf] = len(parent) - 1
    return parent, _lengths(rng, len(parent))


# ---- models ----

def mixture(rng, alphabet, k, reversible):
    """k components of _random_model under Dirichlet weights, as the reference's "mixture" JSON"""
    weight = rng.dirichlet(np.ones(k) * 3.)
    cpts = [_random_model(rng, alphabet, reversible) for _ in range(k)]
    js = {key: cpts[0][key] for key in ("alphabet", "insrate", "delrate", "insextprob", "delextprob")}
    js["mixture"] = [{"subrate": c["subrate"], "rootprob": c["rootprob"], "weight": float(w)} for c, w in zip(cpts, weight)]
    return js


# ---- columns ----

def _full_columns(rng, parent, alphabet, n_cols, recon):
    """columns without a gap.  Counts: a residue at every node or, with probability .15, 'x'; a reconstruction's: '*' at
    the internal nodes, a residue or, with probability .03, 'x' at the leaves"""
    inner = set(p for p in parent if p >= 0)
    cols = []
    for _ in range(n_cols):
        col = []
        for r in range(len(parent)):
            if recon and r in inner:
                col.append("*")
            else:
                col.append("x" if rng.random() < (.03 if recon else .15) else alphabet[int(rng.integers(0, len(alphabet)))])
        cols.append(col)
    return cols


def deep_columns(rng, parent, alphabet, n_cols, recon=False):
    """Two columns of every five are full - only a full column of a deep tree multiplies enough messages to pass below
    1e-30 - and the others come from _random_columns / _recon_columns, which drop subtrees."""
    rows = (_recon_columns if recon else _random_columns)(rng, parent, alphabet, n_cols)
    full = iter(_full_columns(rng, parent, alphabet, n_cols, recon))
    cols = [next(full) if k % 5 in (0, 2) else [row[k] for row in rows] for k in range(n_cols)]
    return ["".join(col[r] for col in cols) for r in range(len(parent))]


# ---- the launchers' plans ----

def counts_plan(a, c, n, n_cols, real_basis, slices=None, no_mfma=False):
    """hx_sumprod_columns (hx_sumprod.hip): what it launches for A symbols, C components, N nodes and one chunk of columns.
    slices, no_mfma: HX_SUMPROD_SLICES, HX_SUMPROD_NO_MFMA."""
    waves = min(c, 8)                                                    # sp_column_plan: waves
    lm = 8 * 64 * c + 8 * 3 * a * a * waves <= 96 * 1024                 # sp_column_plan(mats = 3): ll_lds + waves mat_lds
    ap, mp = (a + 1) & ~1, (a + 15) // 16 * 16
    plan = dict(ta=a if a in (4, 20) else 0, lm=lm, waves=waves, turns=-(-c // waves),        # HX_SP_GO; k_sumprod_columns: cpt += Wb
                lds=8 * 64 * c + (8 * 3 * a * a * waves if lm else 0),
                row_slices=min(64, -(-n_cols // 4096)))                  # k_row_sums' grid
    if real_basis and 8 * 2 * mp * 65 <= 64 * 1024 and not no_mfma:      # k_outer_counts_mfma's condition
        blocks = -(-n_cols // 64)
        sl = 8192 // (c * n) + 1 if slices is None else slices           # its slices `sl`
        sl = min(max(sl, 1), blocks)
        plan.update(outer="matrix cores", per=1 if ap <= 4 else 5 if ap <= 20 else 16,         # its PER
                    groups=sl, blocks_per_group=sorted({len(range(g, blocks, sl)) for g in range(sl)}))
    else:
        tiles = -(-n_cols // 32)                                         # HX_SP_TILE
        s = 4096 // (c * n) + 1 if slices is None else slices            # k_outer_counts' `slices`
        s = min(max(s, 1), tiles)
        plan.update(outer="vector units, real" if real_basis else "vector units, complex", pairs=-(-a * a // 256),       # k_outer_counts: q * 256 < A A
                    groups=s, tiles_per_group=sorted({len(range(g, tiles, s)) for g in range(s)}))
    return plan


def counts_chunk(a, c, n, n_cols, real_basis, mb):
    """columns per chunk of hx_sumprod_columns under HX_SUMPROD_SCRATCH_MB = mb   (per_col there, sp_chunk)"""
    ap, parts = (a + 1) & ~1, 2 if real_basis else 4
    per_col = 8 * ((2 + parts) * c * n * ap + 4 * c * n + 2 * c * a)
    return min(n_cols, max(64, ((mb << 20) // per_col) & ~63))


def counts_chunk_mb(a, c, n, real_basis, columns):
    """the smallest HX_SUMPROD_SCRATCH_MB that holds `columns` columns per chunk"""
    ap, parts = (a + 1) & ~1, 2 if real_basis else 4
    return -(-columns * 8 * ((2 + parts) * c * n * ap + 4 * c * n + 2 * c * a) // (1 << 20))


def ancestors_plan(a, c):
    """hx_sumprod_ancestors (hx_ancestors.hip)"""
    waves = min(c, 8)                                                    # sp_column_plan: waves
    lm = 8 * 64 * c + 8 * a * a * waves <= 96 * 1024                     # sp_column_plan(mats = 1)
    return dict(ta=a if a in (4, 20) and lm else 0, lm=lm, waves=waves, turns=-(-c // waves),      # HX_AN_GO
                combine_waves=4 if a <= 20 else 1)                       # cwaves


# ---- the cases ----

class Spec:
    """A model (JSON), a tree, gapped rows (one per node), column weights or None; the plan the case is there for."""

    def __init__(self, js, tree, rows, reversible, plan, weight=None, root_post=False):
        self.js, (self.parent, self.length), self.rows, self.weight = js, tree, rows, weight
        self.reversible, self.plan, self.root_post = reversible, plan, root_post
        self.a, self.c = len(js["alphabet"]), len(js.get("mixture", [0]))
        self.n, self.n_cols = len(self.parent), len(rows[0])


MFMA5 = dict(outer="matrix cores", per=5)
MFMA16 = dict(outer="matrix cores", per=16)
# name -> what hx_sumprod_columns must plan for it (a subset of counts_plan's keys)
COUNTS = {
    "bal64 prot4": dict(ta=20, lm=True, turns=1, **MFMA5),
    "cat40 cyclic": dict(ta=4, lm=True, turns=1, outer="vector units, complex", pairs=1),
    "cat40 mix12": dict(ta=4, lm=True, waves=8, turns=2, outer="vector units, complex", pairs=1),
    "prot x 9": dict(ta=20, lm=True, waves=8, turns=2, **MFMA5),
    "prot x 42": dict(ta=20, lm=True, lds=96 * 1024, turns=6, **MFMA5),
    "prot x 43": dict(ta=20, lm=False, turns=6, **MFMA5),
    "alphabet 16": dict(ta=0, lm=True, **MFMA5),
    "alphabet 17": dict(ta=0, lm=True, **MFMA5),
    "alphabet 32": dict(ta=0, lm=True, **MFMA16),
    "alphabet 33": dict(ta=0, lm=True, **MFMA16),
    "alphabet 48": dict(ta=0, lm=True, **MFMA16),
    "alphabet 49": dict(ta=0, lm=True, outer="vector units, real", pairs=10),
    "alphabet 63": dict(ta=0, lm=True, lds=512 + 24 * 63 * 63, outer="vector units, real", pairs=16),
    "alphabet 64": dict(ta=0, lm=False, outer="vector units, real", pairs=16),
    "46 x 2": dict(ta=0, lm=False, waves=2, **MFMA16),
    "cyclic 21": dict(ta=0, lm=True, outer="vector units, complex", pairs=2),
    "cyclic 33": dict(ta=0, lm=True, outer="vector units, complex", pairs=5),
    "many columns": dict(ta=4, lm=True, row_slices=2, outer="matrix cores", per=1, groups=66),
}
# name -> what hx_sumprod_ancestors must plan for it
ANCESTORS = {
    "anc alphabet 64 x 3": dict(ta=0, lm=False, waves=3, combine_waves=1),
    "anc 46 x 6": dict(ta=0, lm=False, waves=6, combine_waves=1),
    "anc prot x 9": dict(ta=20, lm=True, waves=8, turns=2, combine_waves=4),
    "anc alphabet 21 x 9": dict(ta=0, lm=True, waves=8, turns=2, combine_waves=1),
    "anc bal64 prot4": dict(ta=20, lm=True, turns=1, combine_waves=4),
    "anc cat40 mix12": dict(ta=4, lm=True, waves=8, turns=2, combine_waves=4),
    # (forty leaves of DNA under wildcards stay above 1e-30 - the smallest E is 3e-27: sixty-four for C > 8 with rescaling)
    "anc cat64 mix12": dict(ta=4, lm=True, waves=8, turns=2, combine_waves=4),
}
# name -> (model kind, symbols, components, tree, columns).  All column counts leave a partly filled block of 64.
SHAPES = {
    "bal64 prot4": ("prot4", 20, 4, "balanced 64", 70),
    "cat40 cyclic": ("cyclic acgt", 4, 1, "caterpillar 40", 130),
    "cat40 mix12": ("cyclic", 4, 12, "caterpillar 40", 70),
    "prot x 9": ("reversible", 20, 9, "random 9", 130),
    "prot x 42": ("reversible", 20, 42, "random 3", 70),
    "prot x 43": ("reversible", 20, 43, "random 3", 70),
    "46 x 2": ("reversible", 46, 2, "random 7", 130),
    "cyclic 21": ("cyclic", 21, 1, "random 7", 130),
    "cyclic 33": ("cyclic", 33, 1, "random 7", 130),
    "many columns": ("jukes-cantor", 4, 1, "random 3", 4200),
    "anc alphabet 64 x 3": ("reversible", 64, 3, "random 7", 70),
    "anc 46 x 6": ("reversible", 46, 6, "random 7", 70),
    "anc prot x 9": ("reversible", 20, 9, "random 7", 70),
    "anc alphabet 21 x 9": ("reversible", 21, 9, "random 7", 70),
    "anc bal64 prot4": ("prot4", 20, 4, "balanced 64", 70),
    "anc cat40 mix12": ("cyclic", 4, 12, "caterpillar 40", 70),
    "anc cat64 mix12": ("cyclic", 4, 12, "caterpillar 64", 70),
}
SHAPES.update({"alphabet %d" % a: ("reversible", a, 1, "random 7", 130) for a in (16, 17, 32, 33, 48, 49, 63, 64)})
assert sorted(SHAPES) == sorted(list(COUNTS) + list(ANCESTORS))
DEEP = ("bal64 prot4", "cat40 cyclic", "cat40 mix12")           # counts cases whose rescaling the oracle test asserts
SEED = {name: 100 + k for k, name in enumerate(list(COUNTS) + list(ANCESTORS))}


@functools.lru_cache(maxsize=None)
def spec(name):
    """built once per process, never modified"""
    kind, a, cpts, shape, n_cols = SHAPES[name]
    rng = np.random.default_rng(SEED[name])
    recon = name in ANCESTORS
    alphabet = "acgt" if a == 4 else AA if a == 20 else SYMBOLS[:a]
    if kind == "prot4":
        with open(PROT4) as f:
            js = json.load(f)
    elif kind in ("cyclic acgt", "jukes-cantor"):
        js = CYCLIC if kind == "cyclic acgt" else JUKES_CANTOR
    else:
        js = _random_model(rng, alphabet, kind == "reversible") if cpts == 1 else mixture(rng, alphabet, cpts, kind == "reversible")
    assert js["alphabet"] == alphabet and len(js.get("mixture", [0])) == cpts
    form, leaves = shape.split()
    tree = {"balanced": balanced, "caterpillar": caterpillar, "random": lambda n, g: _random_tree(g, n)}[form](int(leaves), rng)
    if form == "random":
        rows = (_recon_columns if recon else _random_columns)(rng, tree[0], alphabet, n_cols)
    else:
        rows = deep_columns(rng, tree[0], alphabet, n_cols, recon)
    weight = rng.uniform(.1, 2., n_cols) if name == "bal64 prot4" else None
    return Spec(js, tree, rows, not kind.startswith("cyclic"), (ANCESTORS if recon else COUNTS)[name], weight, root_post=name == "prot x 9")


class Reference:
    """The oracle over every column of a case, once: column likelihoods, the counts accumulated column by column with the
    case's weights (counts cases), root posteriors where the case asks for them, and what tests/test_oracle_sumprod_edges.py
    asserts about the oracle itself."""

    def __init__(self, s, accumulate):
        self.omodel = ho.RateModel(s.js)
        self.tree = so.Tree(s.parent, s.length, ["n%d" % k for k in range(s.n)])
        sp = self.sp = so.SumProduct(self.omodel, self.tree)
        a, c = sp.A, sp.C
        # the device gets the oracle's exp(R t) so that the comparison is of the passes, not of two matrix exponentials
        self.branch_sub = [[sp.branch_sub[cpt][r] if s.parent[r] >= 0 else np.zeros((a, a)) for cpt in range(c)] for r in range(s.n)]
        self.root = [np.zeros(a) for _ in range(c)]
        self.eig = [np.zeros((a, a), dtype=complex) for _ in range(c)]
        self.col_log_like, self.roots = np.zeros(s.n_cols), np.zeros(s.n_cols, dtype=int)
        self.rescaled_wild, self.rescaled_residue = np.zeros(s.n_cols, dtype=int), np.zeros(s.n_cols, dtype=int)
        self.root_post, self.min_g, self.min_e = {}, math.inf, math.inf
        columns = list(so.columns_of(self.tree, dict(enumerate(s.rows))))
        for col in range(s.n_cols):
            sp.init_column(columns[col])
            self.roots[col] = len(sp.roots)
            sp.fill_up()
            sp.fill_down()
            self.col_log_like[col] = sp.col_log_like
            for cpt in range(c):
                for r in sp.ungapped:
                    # a rescaled node: logF is no longer the sum of its children's logE (src/sumprod.cpp:120-124, 135-138)
                    if sp.logF[cpt][r] != sum(sp.logE[cpt][k] for k in self.tree.child[r]):
                        if sp.col[r] == so.WILD:
                            self.rescaled_wild[col] += 1
                        else:
                            self.rescaled_residue[col] += 1
                    g = sp.G[cpt][r]
                    self.min_g = min(self.min_g, float(g[g > 0].min()))
                    if r not in sp.roots:
                        e = sp.E[cpt][r]
                        self.min_e = min(self.min_e, float(e[e > 0].min()))
            if accumulate:
                sp.accumulate_eigen_counts(self.root, self.eig, 1. if s.weight is None else s.weight[col])
                if s.root_post:
                    self.root_post[col] = sp.log_node_post_prob(sp.column_root())
        self.counts = sp.eigen.get_sub_counts(self.eig)


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(spec(name), name in COUNTS)
