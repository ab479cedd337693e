"""Pair-HMM fills at the edges of the model's parameter space: the cases and the checkers shared by
tests/test_oracle_param_edges.py (which pins the yardstick on them) and tests/test_gpu_param_edges.py.

Every other parity test takes a benign model (indel rates .01-.02, extension .6-.66, branches .05-.3) and a y sequence that
is a 10 % mutation of x.  Here the model and the sequences are the variables: zero and tiny rates, zero and saturated
branches, extension probabilities of 0 and nearly 1, indel rates so high that the states of one cell lie hundreds of nats
apart; identical, unrelated, homopolymer and dinucleotide-repeat sequences."""
import functools
import math
import random

import numpy as np

from oracle import c_oracle
from oracle import trace_oracle
from oracle import historian_oracle as ho
from tests import helpers as H

AA = "arndcqeghilkmfpstwyv"
DNA = "ACGT"
NEG_INF = float("-inf")

# name -> insertion rate, deletion rate, extension probability, left and right branch length
MODELS = {
    "t0": dict(ins=.01, dele=.01, ext=.66, tl=0., tr=0.),               # identity substitution, zero indel probability
    "t0_one_side": dict(ins=.01, dele=.01, ext=.66, tl=0., tr=.1),
    "tiny_t": dict(ins=.01, dele=.01, ext=.66, tl=1e-9, tr=1e-9),       # mismatch emissions near 1e-10
    "saturated": dict(ins=.01, dele=.01, ext=.66, tl=50., tr=50.),      # emissions at equilibrium, gap probabilities near 1
    "ins0": dict(ins=0., dele=.01, ext=.66, tl=.1, tr=.1),              # whole state planes -inf
    "indel0": dict(ins=0., dele=0., ext=.66, tl=.1, tr=.1),             # only the diagonal finite
    "tiny_indel": dict(ins=1e-12, dele=1e-12, ext=.66, tl=.1, tr=.1),   # ~27 nats per gap: nearly every second term truncated
    "ext0": dict(ins=.01, dele=.01, ext=0., tl=.1, tr=.1),              # no gap extension
    "ext_near_1": dict(ins=.01, dele=.01, ext=.999999, tl=.1, tr=.1),
    "wide": dict(ins=2., dele=2., ext=.66, tl=1., tr=1.),               # in-cell spread 518 nats at 129 x 129: inside fp64
    "beyond": dict(ins=5., dele=5., ext=.9, tl=1., tr=1.),              # in-cell spread 1305 nats at 65 x 130: outside it
}
# sequence kinds: "mut" y a 10 % mutation of x (the helpers' pairs), "unrel" y random, "same" y = x, "homo" one letter, "rep" a dinucleotide repeat

# (model, sequence kind, x residues, y residues, protein model); the cross product only where it means something
LEAF_CASES = (
    ("t0", "same", 64, 64, False), ("t0", "homo", 64, 64, False), ("t0", "unrel", 64, 64, False), ("t0", "mut", 70, 66, False),
    ("t0", "homo", 65, 63, False),
    ("t0_one_side", "mut", 70, 66, False), ("t0_one_side", "unrel", 65, 130, False), ("t0_one_side", "homo", 65, 63, False),
    ("t0_one_side", "rep", 64, 64, False), ("t0_one_side", "mut", 70, 66, True),
    ("tiny_t", "mut", 70, 66, False), ("tiny_t", "unrel", 65, 63, False), ("tiny_t", "same", 64, 64, False),
    ("tiny_t", "mut", 65, 130, True),
    ("saturated", "mut", 70, 66, False), ("saturated", "unrel", 65, 130, False), ("saturated", "homo", 64, 64, False),
    ("ins0", "mut", 70, 66, False), ("ins0", "unrel", 65, 130, False), ("ins0", "same", 64, 64, False), ("ins0", "rep", 1, 160, False),
    ("indel0", "same", 64, 64, False), ("indel0", "homo", 64, 64, False), ("indel0", "unrel", 64, 64, False),
    ("indel0", "mut", 70, 66, False), ("indel0", "rep", 65, 63, False),
    ("tiny_indel", "mut", 70, 66, False), ("tiny_indel", "unrel", 65, 130, False), ("tiny_indel", "rep", 65, 63, False),
    ("tiny_indel", "unrel", 1, 160, False),
    ("ext0", "mut", 70, 66, False), ("ext0", "unrel", 65, 130, False), ("ext0", "homo", 65, 63, False),
    ("ext_near_1", "mut", 70, 66, False), ("ext_near_1", "unrel", 65, 130, False), ("ext_near_1", "rep", 64, 64, False),
    ("wide", "unrel", 129, 129, False), ("wide", "mut", 70, 66, False), ("wide", "homo", 65, 63, False),
    ("beyond", "unrel", 65, 130, False), ("beyond", "mut", 65, 130, False), ("beyond", "unrel", 1, 160, False),
)
# Five and ten strips of 64 rows, so that two workgroups can share a pair (HX_CHAIN_MULTI=2) and hand rows to each other as
# logarithms: cells that are zero as a whole, zero state planes, terms 27 nats apart.  On the 600-residue diagonals the one
# finite cell per row falls to 2^-1200 (two bits per residue) next to all-zero cells: were a zero cell to keep an exponent
# (the `mx > 0.` test at renormalisation), its neighbours on the diagonal would be shifted out of fp64's range from residue ~510 on
MULTI_CASES = (("t0", "same", 600, 600, False), ("indel0", "same", 600, 600, False), ("indel0", "unrel", 290, 290, False),
               ("ins0", "mut", 300, 60, False), ("tiny_indel", "unrel", 300, 40, False))
# (model, kind, x residues, y residues, band): banded round the left-justified guide of the helpers
BANDED_CASES = tuple((m, "mut", lx, ly, 12) for m in ("t0_one_side", "tiny_indel", "ext0", "wide") for lx, ly in ((70, 66), (65, 63))
                     ) + (("beyond", "unrel", 65, 130, 12),)
# (model, x residues, events, band): banded round the true alignment of a simulated history, so that the envelope leaves row 0
# after a few columns and the row's far cells come from the prefix sum of hx_bandedge.h (events as in tests/band_geometry_cases.py)
GUIDED_CASES = (("tiny_indel", 70, {0: +30, 40: -20}, 4), ("wide", 70, {0: +30, 40: -20}, 4), ("ext0", 66, {20: +25}, 3),
                ("beyond", 65, {0: +65}, 4))
# (model, ancestral length): profile pairs built as H.dag_case builds them, every fill along the way under the same model
DAG_CASES = (("t0_one_side", 14), ("tiny_indel", 14), ("ext0", 14), ("wide", 14), ("wide", 90))
SEED = 20261019


def rate_model(name, aa=False):
    m = MODELS[name]
    if aa:
        return H.random_reversible_model(random.Random(SEED), AA, 1, m["ins"], m["dele"], m["ext"])
    return H.jc_model(DNA, m["ins"], m["dele"], m["ext"])


def sequences(kind, lx, ly, alphabet, rng):
    if kind == "homo":
        return alphabet[0] * lx, alphabet[0] * ly
    if kind == "rep":
        return (alphabet[:2] * lx)[:lx], (alphabet[:2] * ly)[:ly]
    sx = H.random_seq(rng, alphabet, lx)
    if kind == "same":
        assert lx == ly
        return sx, sx
    if kind == "unrel":
        return sx, H.random_seq(rng, alphabet, ly)
    assert kind == "mut"
    sy = H.mutate(rng, sx, alphabet)[:ly]
    while len(sy) < ly:
        sy += rng.choice(alphabet)
    return sx, sy


def leaf_name(model, kind, lx, ly, aa=False, band=None):
    return "%s/%s%s %dx%d%s" % (model, kind, "/aa" if aa else "", lx, ly, "" if band is None else " band %d" % band)


def guided_name(model, lx, events_items, band):
    return "%s/guided %d%s band %d" % (model, lx, "".join(" %d:%+d" % e for e in events_items), band)


def dag_name(model, n):
    return "%s/dag n=%d" % (model, n)


def _case(f, **attrs):
    img = H.job_images(f)
    return dict(f=f, img=img, **attrs)


@functools.lru_cache(maxsize=None)
def leaf_case(model, kind, lx, ly, aa=False, band=None):
    """One leaf pair -> dict(f = the unfilled oracle ForwardMatrix, img = its job image, model, kind, sx, sy, name); built
    once per process, never modified"""
    rm = rate_model(model, aa)
    rng = random.Random("%s/%s/%d/%d/%d" % (model, kind, lx, ly, aa))
    sx, sy = sequences(kind, lx, ly, rm.alphabet, rng)
    m = MODELS[model]
    env = ho.GuideAlignmentEnvelope()
    if band is not None:
        env = ho.GuideAlignmentEnvelope(H.left_justified_guide({1: sx, 2: sy}), 1, 2, band)
    f = ho.ForwardMatrix(H.leaf(rm, sx, 1, "x"), H.leaf(rm, sy, 2, "y"), H.make_hmm(rm, m["tl"], m["tr"]), 0, env, fill=False)
    return _case(f, model=model, kind=kind, sx=sx, sy=sy, name=leaf_name(model, kind, lx, ly, aa, band))


@functools.lru_cache(maxsize=None)
def guided_case(model, lx, events_items, band):
    rm = rate_model(model)
    rng = random.Random("%s/guided/%d" % (model, lx))
    sx = H.random_seq(rng, DNA, lx)
    cols = H.evolve(rng, sx, DNA, dict(events_items))
    sy = "".join(c for _, c in cols if c is not None)
    guide = {1: [a is not None for a, _ in cols], 2: [c is not None for _, c in cols]}
    m = MODELS[model]
    f = ho.ForwardMatrix(H.leaf(rm, sx, 1, "x"), H.leaf(rm, sy, 2, "y"), H.make_hmm(rm, m["tl"], m["tr"]), 0,
                         ho.GuideAlignmentEnvelope(guide, 1, 2, band), fill=False)
    return _case(f, model=model, kind="guided", sx=sx, sy=sy, name=guided_name(model, lx, events_items, band))


def _is_dag(prof):
    return any(len(st.in_) > 1 for st in prof.state)


@functools.lru_cache(maxsize=None)
def dag_case(model, n, samples=6):
    """H.dag_case with the model and the branch lengths from MODELS: four leaves mutated from one ancestor, two internal
    profiles sampled from their leaf fills (under the same model: the transition weights they carry are extreme too).  Where
    gaps are all but impossible every sample is the same path and the profile a chain, which the general kernels never see:
    the first ancestor whose two profiles both branch is taken"""
    rm = rate_model(model)
    m = MODELS[model]
    for attempt in range(50):
        rng = random.Random("%s/dag/%d/%d" % (model, n, attempt))
        anc = H.random_seq(rng, DNA[:2], n)           # (two letters: runs, in which the place of a gap is a toss-up)
        s = [H.mutate(rng, anc, DNA, .15, .06) or DNA[0] for _ in range(4)]
        p1 = H.internal_profile(rm, s[0], s[1], (0, 1), 4, n * 7 + 1, samples, tl=m["tl"], tr=m["tr"])
        p2 = H.internal_profile(rm, s[2], s[3], (2, 3), 5, n * 7 + 2, samples, tl=m["tl"], tr=m["tr"])
        if _is_dag(p1) and _is_dag(p2):
            break
    else:
        raise AssertionError("no branching profiles under " + model)
    f = ho.ForwardMatrix(p1, p2, H.make_hmm(rm, m["tl"], m["tr"]), 6, ho.GuideAlignmentEnvelope(), fill=False)
    return _case(f, model=model, kind="dag", name=dag_name(model, n))


def _specs():
    """(name, function of the cached builder, its arguments) of every case, in the order leaf, multi, banded, dag"""
    out = [("leaf", leaf_name(*c), leaf_case, c) for c in LEAF_CASES]
    out += [("multi", leaf_name(*c), leaf_case, c) for c in MULTI_CASES]
    out += [("banded", leaf_name(m, k, lx, ly, False, band), leaf_case, (m, k, lx, ly, False, band)) for m, k, lx, ly, band in BANDED_CASES]
    for m, lx, ev, band in GUIDED_CASES:
        items = tuple(sorted(ev.items()))
        out.append(("banded", guided_name(m, lx, items, band), guided_case, (m, lx, items, band)))
    out += [("dag", dag_name(*c), dag_case, c) for c in DAG_CASES]
    return out


def case_names(*groups):
    """the names of the cases of the given groups ("leaf", "multi", "banded", "dag"), without building one"""
    return [name for g, name, _, _ in _specs() if g in groups]


def case(name):
    for _, n, build, args in _specs():
        if n == name:
            return build(*args)
    raise KeyError(name)


def model_of_case(name):
    return name.split("/")[0]


def leaf_cases():
    return [leaf_case(*c) for c in LEAF_CASES]


def multi_cases():
    return [leaf_case(*c) for c in MULTI_CASES]


def banded_cases():
    return [leaf_case(m, k, lx, ly, False, band) for m, k, lx, ly, band in BANDED_CASES] + \
           [guided_case(m, lx, tuple(sorted(ev.items())), band) for m, lx, ev, band in GUIDED_CASES]


def dag_cases():
    return [dag_case(*c) for c in DAG_CASES]


# ---------------------------------------------------------------------------
# the yardstick: the C oracle in its three arithmetics (0 the reference's table, 1 libm, 2 libm with the reference's truncation)
# ---------------------------------------------------------------------------
_oracle_cache = {}


def oracle(case, which, tm=0):
    """c_oracle.forward (which = 0) / backward (1) of a case in arithmetic tm; computed once per process, read-only"""
    key = (case["name"], which, int(tm))
    if key not in _oracle_cache:
        r = (c_oracle.backward if which else c_oracle.forward)(*case["img"], true_math=tm)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle_cache[key] = r
    return _oracle_cache[key]


_path_cache = {}


def reference_path(case):
    """trace_oracle.best_trace through the table oracle's Forward matrix; None where the likelihood is zero"""
    if case["name"] not in _path_cache:
        fwd = oracle(case, 0)
        _path_cache[case["name"]] = trace_oracle.best_trace(*case["img"], fwd) if np.isfinite(fwd["lp_end"]) else None
    return _path_cache[case["name"]]


def lp_of(result, which):
    return result["lp_start"] if which else result["lp_end"]


def in_cell_spread(cells):
    """[R][Cc]: the largest difference between two finite states of each cell (0 with fewer than two)"""
    fin = np.isfinite(cells)
    hi = np.where(fin, cells, -np.inf).max(axis=-1)
    lo = np.where(fin, cells, np.inf).min(axis=-1)
    return np.where(fin.sum(axis=-1) >= 2, hi - lo, 0.)


def depth_below_cell_max(cells):
    """[R][Cc][5]: how far each state lies below the largest state of its own cell, in nats (inf for -inf states)"""
    with np.errstate(invalid="ignore"):
        d = cells.max(axis=-1, keepdims=True) - cells
    return np.where(np.isfinite(cells), d, np.inf)


# ---------------------------------------------------------------------------
# The dynamic range of a cell in the scaled-probability fills (hx_linear.hip, hx_band.hip, hx_band2.hip)
#
# A cell is five fp64 mantissas under ONE exponent, and the exponent follows the cell's LARGEST state.  A state that lies
# d nats below the largest state of its cell is the number m_max * e^-d, so it leaves fp64's normal range when
# m_max * e^-d < 2^-1022.  What m_max can be:
#   * a renormalisation brings the largest mantissa to [1/2, 1); it happens on two steps (anti-diagonals) out of eight, so a
#     cell's sources have been through up to six steps without one, and the cell's own sums are formed before its own
#     renormalisation: seven products in a row;
#   * each product is a transition probability times an emission.  The largest state s* of a source cell has a transition
#     into some state of the new cell in the direction of that source (every state has one to the left, upwards and
#     diagonally: src/pairhmm.cpp:117-140), so the new cell's largest mantissa is at least the source's times
#         phi_fwd = min over s, direction of  max over d in that direction of  P[s][d] * (smallest emission of d);
#     in the Backward fill the roles swap: the largest state d* of a destination cell is entered from some s, so
#         phi_bwd = min over d of  max over s of  P[s][d] * (smallest emission of d).
#     After k such steps the largest mantissa is at least phi^k / 2.
#   * the truncating sum (trunc_sum) lets a dropped term keep its low word, a number below 2^-1042; for that to stay below
#     2^-40 of the sum (9e-13 per sum, 1e-9 only after a thousand of them) the sum must be at least 2^-1002.
# A state therefore keeps full precision while  e^-d * phi^7 / 2 >= 2^-1002:
#         D = 1001 ln 2 - 7 ln(1 / phi),   phi = min(phi_fwd, phi_bwd) of the model.
# Deeper states may come out with reduced precision (subnormal mantissas) or as -inf.  For `beyond` (ins = del = 5, ext .9,
# t = 1, Jukes-Cantor) phi = e^-22.8 (match to match: four events that did not happen, at e^-5 each) and D = 534.4 nats; for
# the realistic long-branch model of DESIGN.md (ins = del = .1, t = 2) phi = e^-4.45 and D = 662.7.  The bound is deliberately
# the arithmetic's worst case: on row 0, where the spread arises, a step costs `beyond` 1.5 nats, not 22.8.
# ---------------------------------------------------------------------------
LN2 = math.log(2.)
_DIRECTION = {0: "diag", 1: "up", 4: "up", 2: "left", 3: "left"}      # destination state -> where its source cell lies


def per_step_floor(hmm):
    """(phi_fwd, phi_bwd) of a PairHMM over leaf sequences, as derived above"""
    T = np.array(hmm.trans_matrix())[:, :5]
    root = np.exp(np.array(hmm.log_root))                                    # [C][A], component weight included
    sl, sr = np.array(hmm.l.sub_mat), np.array(hmm.r.sub_mat)                # [C][A][A]
    pair = np.einsum("ca,cax,cay->xy", root, sl, sr)                         # IMM: both residues absorbed
    only_l, only_r = np.einsum("ca,cax->x", root, sl), np.einsum("ca,cay->y", root, sr)     # IMD / IDM: rootsubx / rootsuby
    insl = np.einsum("c,ca->a", np.exp(np.array(hmm.logl.log_cpt_weight)), np.array(hmm.l.ins_vec))
    insr = np.einsum("c,ca->a", np.exp(np.array(hmm.logr.log_cpt_weight)), np.array(hmm.r.ins_vec))
    emit = [pair[pair > 0].min(), only_l.min(), only_r.min(), insr.min(), insl.min()]
    with np.errstate(divide="ignore"):
        F = T + np.log(np.array(emit))[None, :]                              # [s][d] log factor of the move s -> d
    fwd = min(max(F[s][d] for d in range(5) if _DIRECTION[d] == way) for s in range(5) for way in ("diag", "up", "left")
              if np.isfinite(T[s]).any())
    bwd = min(F[:, d].max() for d in range(5) if np.isfinite(T[:, d]).any())
    return math.exp(fwd), math.exp(bwd)


def full_precision_depth(hmm):
    """D: states at most this many nats below the largest state of their cell keep full precision in the scaled fills"""
    phi = min(per_step_floor(hmm))
    assert phi > 0., "a state of this model cannot move in some direction: the derivation does not cover it"
    return 1001 * LN2 - 7 * math.log(1. / phi)


# ---------------------------------------------------------------------------
# checkers (got = a device matrix [R][Cc][5], want = the oracle's)
# ---------------------------------------------------------------------------
def assert_cells_close(got, want, tol, what, sel=None):
    """no NaN, the same -inf pattern, finite cells within tol (inside sel [R][Cc] when given)"""
    sel3 = np.ones(want.shape, dtype=bool) if sel is None else np.broadcast_to(sel[:, :, None], want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got[sel3]).any(), "%s: NaN" % what
    bad = np.argwhere((np.isneginf(got) != np.isneginf(want)) & sel3)
    assert len(bad) == 0, "%s: -inf pattern differs in %d values, first at %s: %r vs %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    fin = np.isfinite(want) & sel3
    err = np.abs(got[fin] - want[fin])
    worst = err.max(initial=0.)
    assert worst < tol, "%s: finite cells differ by %.3g (bound %.3g) at %s" % (what, worst, tol, tuple(np.argwhere(fin)[err.argmax()]))
    return worst


def assert_cells_close_within_depth(got, want, tol, depth, what, sel=None):
    """The narrowed contract of the scaled-probability fills: every state at most `depth` nats below the largest state of
    its own cell (in the oracle's matrix) is not NaN, -inf exactly where the oracle's is and finite within tol; a deeper
    state may deviate (-inf or reduced precision) but is never NaN, and never finite where the oracle has -inf.
    -> (the number of deviating states, the smallest depth among them)"""
    sel3 = np.ones(want.shape, dtype=bool) if sel is None else np.broadcast_to(sel[:, :, None], want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got[sel3]).any(), "%s: NaN" % what
    d = depth_below_cell_max(want)
    with np.errstate(invalid="ignore"):
        off = (np.isneginf(got) != np.isneginf(want)) | (np.isfinite(want) & np.isfinite(got) & ~(np.abs(got - want) < tol))
    off &= sel3
    shallow = off & ~(d > depth)
    assert not shallow.any(), "%s: %d states within %.1f nats of their cell's largest deviate, first at %s: %r vs %r (depth %.1f)" % (
        what, shallow.sum(), depth, tuple(np.argwhere(shallow)[0]), got[tuple(np.argwhere(shallow)[0])],
        want[tuple(np.argwhere(shallow)[0])], d[tuple(np.argwhere(shallow)[0])])
    assert not (np.isneginf(want) & ~np.isneginf(got) & sel3).any(), "%s: a finite value where the oracle has -inf" % what
    return int(off.sum()), float(d[off].min()) if off.any() else float("inf")


def assert_lp_close(got, want, rel, what):
    """a likelihood: -inf exactly when the oracle's is (never NaN), else within rel of it"""
    assert not np.isnan(got), "%s: NaN" % what
    if np.isfinite(want):
        assert abs(want - got) <= rel * abs(want), "%s: %r vs %r (%.3g relative, bound %.3g)" % (
            what, got, want, abs(want - got) / abs(want), rel)
    else:
        assert got == want, "%s: %r vs %r" % (what, got, want)
