"""Test-side glue: oracle objects -> C-ABI images, seeded workload generators."""
import random

import numpy as np

from historian_amd import capi
from oracle import historian_oracle as ho

NEG_INF = float("-inf")


def profile_image(prof, env=None, env_row=None):
    """oracle Profile -> capi.ProfileImage (POD image of the reference Profile)."""
    n = prof.size()
    C, A = prof.components, prof.alph_size
    is_null = np.array([1 if s.is_null() else 0 for s in prof.state], dtype=np.uint8)
    lpa = np.full((n, C, A), NEG_INF)
    for i, s in enumerate(prof.state):
        if not s.is_null():
            lpa[i] = np.array(s.lp_absorb)
    env_pos = None
    if env is not None and env.initialized():
        pos2col = env.row1_pos_to_col if env_row == env.row1 else env.row2_pos_to_col
        env_pos = np.zeros(n, dtype=np.int32)
        for i in range(1, n):
            env_pos[i] = env.cumulative_matches[pos2col[prof.state[i].seq_coords[env_row]]]
        env_pos[0] = env.cumulative_matches[pos2col[0]]
    return capi.ProfileImage([t.src for t in prof.trans], [t.dest for t in prof.trans],
                             [t.lp_trans for t in prof.trans],
                             [s.in_ for s in prof.state], [s.absorb_out for s in prof.state],
                             [s.null_out for s in prof.state], is_null, lpa, env_pos)


def hmm_image(hmm):
    """oracle PairHMM -> capi.HmmImage"""
    log = np.vectorize(ho.safe_log)
    return capi.HmmImage(np.array(hmm.trans_matrix()), np.array(hmm.log_root),
                         log(np.array(hmm.l.sub_mat)), log(np.array(hmm.r.sub_mat)),
                         np.array(hmm.logl.log_ins_prob), np.array(hmm.logr.log_ins_prob),
                         np.array(hmm.logl.log_cpt_weight), np.array(hmm.logr.log_cpt_weight))


def job_images(fwd):
    """(ProfileImage x, ProfileImage y, HmmImage, max_distance) for an oracle DPMatrix."""
    env = fwd.envelope
    x = profile_image(fwd.x, env, env.row1)
    y = profile_image(fwd.y, env, env.row2)
    return x, y, hmm_image(fwd.hmm), env.max_distance


def oracle_dense(dp):
    """oracle DPMatrix sparse cells -> dense [R][Cc][5] (-inf where absent)."""
    out = np.full((dp.x_size - 1, dp.y_size - 1, 5), NEG_INF)
    for (i, j), c in dp.cells.items():
        if i < dp.x_size - 1 and j < dp.y_size - 1:
            out[i, j] = c
    return out


def envelope_mask(dp):
    """[R][Cc] bool: the cells of an oracle DPMatrix that lie inside its envelope (reference src/forward.h:92-98)."""
    return np.array([[dp.in_envelope(i, j) for j in range(dp.y_size - 1)] for i in range(dp.x_size - 1)], dtype=bool)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_bits(a, b, what=""):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    # -0.0 never arises; NaN never arises
    assert len(bad) == 0, "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


# ---------------------------------------------------------------------------
# seeded synthetic workloads
# ---------------------------------------------------------------------------
def random_seq(rng, alphabet, n, weights=None):
    return "".join(rng.choices(alphabet, weights=weights, k=n))


def mutate(rng, seq, alphabet, sub=.1, indel=.03):
    out = []
    for ch in seq:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out.append(rng.choice(alphabet))
        out.append(rng.choice(alphabet) if rng.random() < sub else ch)
    return "".join(out)


def jc_model(alphabet="ACGT", ins=.01, dele=.01, ext=.66):
    a = alphabet
    return ho.RateModel({"alphabet": a, "insrate": ins, "delrate": dele, "insextprob": ext, "delextprob": ext,
                         "subrate": {c: {d: 1 for d in a if d != c} for c in a}})


def random_reversible_model(rng, alphabet, components=1, ins=.02, dele=.02, ext=.6):
    """A random GTR-like mixture: symmetric exchangeabilities x stationary frequencies."""
    a = len(alphabet)
    cpts = []
    for _ in range(components):
        pi = np.array([rng.random() + .2 for _ in range(a)])
        pi /= pi.sum()
        ex = np.zeros((a, a))
        for i in range(a):
            for j in range(i + 1, a):
                ex[i, j] = ex[j, i] = rng.random() + .05
        scale = rng.random() + .5
        sub = {alphabet[i]: {alphabet[j]: float(scale * ex[i, j] * pi[j]) for j in range(a) if j != i} for i in range(a)}
        cpts.append({"subrate": sub, "rootprob": {alphabet[i]: float(pi[i]) for i in range(a)},
                     "weight": rng.random() + .5})
    js = {"alphabet": alphabet, "insrate": ins, "delrate": dele, "insextprob": ext, "delextprob": ext}
    if components == 1:
        js.update({k: v for k, v in cpts[0].items() if k != "weight"})
    else:
        js["mixture"] = cpts
    return ho.RateModel(js)


def make_hmm(model, tl, tr):
    return ho.PairHMM(ho.ProbModel(model, tl), ho.ProbModel(model, tr), model.ins_prob)


def leaf(model, seq, row, name=None):
    return ho.Profile.from_seq(model.components(), model.alphabet, seq, row, name or ("s%d" % row))


def internal_profile(model, sx, sy, rows, parent_row, seed, samples=6, tl=.1, tr=.15, keep_all=False):
    """A real internal-node profile (DAG with null/wait/ready states) made the way
    Reconstructor::reconstruct makes them (reference src/recon.cpp:1010)."""
    hmm = make_hmm(model, tl, tr)
    x, y = leaf(model, sx, rows[0]), leaf(model, sy, rows[1])
    fwd = ho.ForwardMatrix(x, y, hmm, parent_row, ho.GuideAlignmentEnvelope())
    gen = ho.MT19937(seed)
    strat = (0 if keep_all else ho.DPMatrix.CollapseChains) | ho.DPMatrix.IncludeBestTrace
    return fwd.sample_profile(gen, samples, 0, strat)


def left_justified_guide(seqs):
    """A (bad but valid) guide alignment: all sequences left-justified."""
    cols = max(len(s) for s in seqs.values())
    return {row: [True] * len(s) + [False] * (cols - len(s)) for row, s in seqs.items()}


def dag_case(seed, n=14, alphabet="ACGT", components=1, band=None, samples=6, keep_all=False):
    """Forward DP of two internal (DAG) profiles; returns the oracle ForwardMatrix (unfilled)."""
    rng = random.Random(seed)
    model = jc_model(alphabet) if components == 1 and seed % 2 == 0 else random_reversible_model(rng, alphabet, components)
    anc = random_seq(rng, alphabet, n)
    s = [mutate(rng, anc, alphabet, .15, .06) for _ in range(4)]
    s = [t if t else alphabet[0] for t in s]
    p1 = internal_profile(model, s[0], s[1], (0, 1), 4, seed * 7 + 1, samples, keep_all=keep_all)
    p2 = internal_profile(model, s[2], s[3], (2, 3), 5, seed * 7 + 2, samples, keep_all=keep_all)
    hmm = make_hmm(model, .2, .05)
    if band is None:
        env = ho.GuideAlignmentEnvelope()
    else:
        guide = left_justified_guide({0: s[0], 1: s[1], 2: s[2], 3: s[3]})
        env = ho.GuideAlignmentEnvelope(guide, 0, 2, band)
    return ho.ForwardMatrix(p1, p2, hmm, 6, env, fill=False)


def leaf_case(seed, lx, ly, alphabet="ACGT", components=1, jc=True, tl=.1, tr=.1, band=None):
    rng = random.Random(seed)
    model = jc_model(alphabet) if jc else random_reversible_model(rng, alphabet, components)
    sx = random_seq(rng, alphabet, lx)
    sy = mutate(rng, sx, alphabet)[:ly] if lx else ""
    while len(sy) < ly:
        sy += rng.choice(alphabet)
    hmm = make_hmm(model, tl, tr)
    env = ho.GuideAlignmentEnvelope()
    if band is not None:
        env = ho.GuideAlignmentEnvelope(left_justified_guide({1: sx, 2: sy}), 1, 2, band)
    return ho.ForwardMatrix(leaf(model, sx, 1, "x"), leaf(model, sy, 2, "y"), hmm, 0, env, fill=False)


# ---------------------------------------------------------------------------
# pairs and profile pairs whose guide alignment is the TRUE alignment of a simulated history: long gap runs,
# leading / trailing gaps, blocks with no match at all (the envelope geometry a left-justified guide never has)
# ---------------------------------------------------------------------------
def evolve(rng, anc, alphabet, events, sub=.15):
    """Walk `anc`: `events` maps a position to n; +n puts an n-residue insertion before that residue (position len(anc): after
    the last one), -n deletes n residues starting at it (the position after the run takes its own event: a deletion directly
    followed by an insertion is a block with no match at all); every other residue is substituted with probability `sub`.
    -> the true alignment, one (ancestral residue index or None, descendant residue or None) per column."""
    cols, i = [], 0
    while i <= len(anc):
        n = events.get(i, 0)
        cols += [(None, rng.choice(alphabet)) for _ in range(n)]
        if i == len(anc):
            break
        if n < 0:
            gone = min(-n, len(anc) - i)
            cols += [(k, None) for k in range(i, i + gone)]
            i += gone
            continue
        cols.append((i, rng.choice(alphabet) if rng.random() < sub else anc[i]))
        i += 1
    return cols


def guided_leaf_case(seed, lx, events, band, alphabet="ACGT", components=1, jc=True, tl=.1, tr=.1):
    """A leaf pair banded round its true alignment: x random, y = evolve(x, events); the guide is that alignment's two rows.
    Returns the oracle ForwardMatrix (unfilled), with the guide as .guide"""
    rng = random.Random(seed)
    model = jc_model(alphabet) if jc else random_reversible_model(rng, alphabet, components)
    sx = random_seq(rng, alphabet, lx)
    cols = evolve(rng, sx, alphabet, events)
    sy = "".join(c for _, c in cols if c is not None)
    guide = {1: [a is not None for a, _ in cols], 2: [c is not None for _, c in cols]}
    env = ho.GuideAlignmentEnvelope(guide, 1, 2, band)
    f = ho.ForwardMatrix(leaf(model, sx, 1, "x"), leaf(model, sy, 2, "y"), make_hmm(model, tl, tr), 0, env, fill=False)
    f.guide, f.seqs = guide, {1: sx, 2: sy}
    return f


def guided_dag_case(seed, n, events_per_leaf, band, samples, keep_all=False):
    """Forward DP of two internal profiles over four leaves that evolved from one ancestor, each by its own events; the guide
    is their true multiple alignment (the ancestor's columns in order, each leaf's insertions in columns of their own).
    samples = 0: the profiles are the best paths alone, chains of states (with their null states when keep_all)."""
    rng = random.Random(seed)
    alphabet = "ACGT"
    model = jc_model(alphabet) if seed % 2 == 0 else random_reversible_model(rng, alphabet, 1)
    anc = random_seq(rng, alphabet, n)
    hist = [evolve(rng, anc, alphabet, ev, .15) for ev in events_per_leaf]
    assert len(hist) == 4
    s = ["".join(c for _, c in h if c is not None) for h in hist]
    # columns: before ancestral residue i (and after the last), leaf 0's insertions, then leaf 1's, ...; then residue i
    guide = {r: [] for r in range(4)}
    ptr = [0] * 4
    for i in range(n + 1):
        for r in range(4):
            while ptr[r] < len(hist[r]) and hist[r][ptr[r]][0] is None:
                for q in range(4):
                    guide[q].append(q == r)
                ptr[r] += 1
        if i == n:
            break
        for r in range(4):
            a, c = hist[r][ptr[r]]
            assert a == i
            guide[r].append(c is not None)
            ptr[r] += 1
    p1 = internal_profile(model, s[0], s[1], (0, 1), 4, seed * 7 + 1, samples, keep_all=keep_all)
    p2 = internal_profile(model, s[2], s[3], (2, 3), 5, seed * 7 + 2, samples, keep_all=keep_all)
    f = ho.ForwardMatrix(p1, p2, make_hmm(model, .2, .05), 6, ho.GuideAlignmentEnvelope(guide, 0, 2, band), fill=False)
    f.guide, f.seqs = guide, dict(enumerate(s))
    return f


def valid_guide(guide, seqs):
    """the guide is an alignment of the sequences: equal row lengths, one True per residue, no all-gap column"""
    cols = {len(r) for r in guide.values()}
    return (len(cols) == 1 and all(sum(guide[r]) == len(seqs[r]) for r in guide)
            and all(any(guide[r][c] for r in guide) for c in range(cols.pop())))


def with_plateaus(x_env, y_env, spec):
    """Envelope coordinates (non-decreasing match counts, [0] first) with long gap runs put in: spec = ("x", start, n) holds
    the x coordinate for n positions from `start`, ("y", start, n) the y coordinate, ("xy", start, nx, ny) an x run of nx
    directly followed, at the same coordinate, by a y run of ny (a block without a match).  The single steps already there stay."""
    fx, fy = [list(np.diff(np.asarray(e, dtype=np.int64)) > 0) for e in (x_env, y_env)]
    if spec[0] in ("x", "xy"):
        fx[spec[1]:spec[1] + spec[2]] = [False] * len(fx[spec[1]:spec[1] + spec[2]])
    if spec[0] == "y":
        fy[spec[1]:spec[1] + spec[2]] = [False] * len(fy[spec[1]:spec[1] + spec[2]])
    if spec[0] == "xy":
        v = sum(fx[:spec[1]])
        c = next(c for c in range(len(fy) + 1) if sum(fy[:c]) == v)
        fy[c:c + spec[3]] = [False] * len(fy[c:c + spec[3]])
    return [np.concatenate([[0], np.cumsum(f)]).astype(np.int32) for f in (fx, fy)]
