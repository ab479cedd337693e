"""Restatement (test infrastructure only) of the indel counts a profile carries through the tree: makeProfile under
CountIndelEvents (reference src/forward.cpp:764-830), the carried x/y.getTrans(..)->counts terms of transitionEigenCounts
(:579-584) and BackwardMatrix::getCounts on profiles that carry them (:1183-1214).  On top of oracle/historian_oracle and
oracle/counts_dp_oracle, which restate the same functions for profiles that carry nothing.

A profile built with CountIndelEvents keeps, for every transition, the expected events of the sub-alignment paths it
sums: {ins, del, insExt, delExt, insTime, delTime} (IndelCounts, src/model.h:165-178).  Where makeProfile eliminates a
cell it mixes the counts of the paths through it in proportion to their probabilities: counts *= 1 - pp;
counts += (src + dest) * pp.  Profile::addReadyStates copies the transitions with their counts and gives the new
wait -> ready transitions none.  The counts live beside the oracle's transitions, in Profile.trans_counts (one 6-tuple per
transition index; profiles without it carry zeros)."""
import contextlib
import math

from oracle import counts_dp_oracle as cd
from oracle import historian_oracle as ho

KEYS = cd.KEYS
ZERO = (0.,) * 6
NEG_INF = float("-inf")
EEE = ho.EEE


def _exact_log_sum_exp(a, b, *rest):
    mx, mn = (a, b) if a >= b else (b, a)
    ret = mx if mn == NEG_INF else mx + math.log1p(math.exp(mn - mx))
    for c in rest:
        ret = _exact_log_sum_exp(ret, c)
    return ret


@contextlib.contextmanager
def exact_log_sum_exp():
    """The oracle's fills and profile construction with log(e^a + e^b) in libm arithmetic instead of the reference's table
    (accurate to ~1e-5): what path enumeration is compared with at 1e-12."""
    saved = ho.log_sum_exp
    ho.log_sum_exp = _exact_log_sum_exp
    try:
        yield
    finally:
        ho.log_sum_exp = saved


def _add(a, b):
    return tuple(p + q for p, q in zip(a, b))


def trans_index(prof, src, dest):
    """the index of Profile::getTrans(src, dest) (src/profile.cpp:93-98)"""
    for t in prof.state[dest].in_:
        if prof.trans[t].src == src:
            return t
    raise KeyError((src, dest))


def carried(prof, t):
    tc = getattr(prof, "trans_counts", None)
    return ZERO if tc is None else tc[t]


def transition_counts(fwd, tm, src, dest):
    """transitionEigenCounts, indel members (src/forward.cpp:579-652): the carried counts of the child transitions the move
    takes, then the pair HMM's own events"""
    c = ZERO
    if src[0] != dest[0]:
        c = _add(c, carried(fwd.x, trans_index(fwd.x, src[0], dest[0])))
    if src[1] != dest[1]:
        c = _add(c, carried(fwd.y, trans_index(fwd.y, src[1], dest[1])))
    ev = cd.transition_indel_counts(tm, src[2], dest[2], fwd.x.state[dest[0]].is_null(), fwd.y.state[dest[1]].is_null())
    return _add(c, tuple(ev[k] for k in KEYS))


class CarryForwardMatrix(ho.ForwardMatrix):
    """ho.ForwardMatrix whose make_profile honours CountIndelEvents; model: the RateModel of the two branches (for the
    wait times of transitionEigenCounts)"""
    partial_mixes = 0      # mixing steps of make_profile (all instances) where a path met others already summed: pp < 1

    def __init__(self, x, y, hmm, parent_row_index, env, model, fill=True):
        self.tm = cd.branch_times(model, hmm.l.t, hmm.r.t)
        super().__init__(x, y, hmm, parent_row_index, env, fill)

    def make_profile(self, cells, strategy=ho.DPMatrix.CollapseChains):
        prof = super().make_profile(cells, strategy)
        if strategy & self.CountIndelEvents:
            prof.trans_counts = self._carried_counts(prof, cells, strategy)
        return prof

    def _carried_counts(self, prof, cells, strategy):
        """the effective transitions of makeProfile (src/forward.cpp:735-812) once more, with their counts"""
        ordered = sorted(set(cells))
        out_count = {}
        for dest in ordered:
            for src in self.source_transitions(dest):
                out_count[src] = out_count.get(src, 0) + 1
        kept = {}
        for c in ordered:
            if (self.is_absorbing(c) or c == self.start_cell or c == self.end_cell or out_count.get(c, 0) > 1
                    or (strategy & self.KeepGapsOpen) != 0 or (strategy & self.CollapseChains) == 0):
                kept[c] = len(kept)
        eff = {}                                   # eff[src][destIdx] = [lpPath, counts]
        for it in reversed(ordered):
            slp = self.source_transitions_without_emit_or_absorb(it)
            lp_ins = self.eliminated_log_prob_insert(it)
            if it in kept:
                for src in sorted(slp):
                    eff.setdefault(src, {})[kept[it]] = [slp[src] + lp_ins, transition_counts(self, self.tm, src, it)]
            else:
                cell_eff = eff.setdefault(it, {})
                for src in sorted(slp):
                    src_counts = transition_counts(self, self.tm, src, it)
                    src_eff = eff.setdefault(src, {})
                    for dest_idx in sorted(cell_eff):
                        cde = cell_eff[dest_idx]
                        sde = src_eff.setdefault(dest_idx, [NEG_INF, ZERO])
                        lp_path = slp[src] + lp_ins + cde[0]
                        sde[0] = ho.log_sum_exp(sde[0], lp_path)
                        pp = math.exp(lp_path - sde[0])
                        CarryForwardMatrix.partial_mixes += pp < 1
                        sde[1] = tuple(old * (1 - pp) for old in sde[1])
                        sde[1] = _add(sde[1], tuple(v * pp for v in _add(src_counts, cde[1])))
        counts = []
        for c in sorted(kept):
            for dest_idx in sorted(eff.get(c, {})):
                e = eff[c][dest_idx]
                t = len(counts)
                assert prof.trans[t].lp_trans == e[0], "effective transitions out of step with makeProfile"
                counts.append(e[1])
        # addReadyStates (src/profile.cpp:268-319): the transitions keep their indices and counts; wait -> ready ones carry none
        return counts + [ZERO] * (len(prof.trans) - len(counts))


def carried_table(prof):
    """[n_trans][6] of a profile, for hx_batch_event_counts"""
    return [list(carried(prof, t)) for t in range(len(prof.trans))]


def get_indel_counts(bwd, tm):
    """BackwardMatrix::getCounts, indel part, with the carried counts (src/forward.cpp:1183-1214) -> (dict of the six counts
    and lp, x_post, y_post): x_post[t] the posterior probability that the path moves along transition t of x (transitions
    into END, which getCounts does not visit, read 0)"""
    fwd = bwd.fwd
    out = dict.fromkeys(KEYS, 0.)
    out["lp"] = fwd.lp_end
    x_post, y_post = [0.] * len(fwd.x.trans), [0.] * len(fwd.y.trans)
    for i in range(fwd.x_size - 1):
        for j in range(fwd.y_size - 1):
            if not fwd.in_envelope(i, j):
                continue
            for s in (ho.IMM, ho.IMD, ho.IDM, ho.IMI, ho.IIW):
                dest = (i, j, s)
                lp_dest = bwd.cell(i, j, s)
                for src, lp in fwd.source_transitions(dest).items():
                    if not min(fwd.cellc(src), lp, lp_dest) > NEG_INF:
                        continue
                    w = math.exp(fwd.cellc(src) + lp + lp_dest - fwd.lp_end)
                    c = transition_counts(fwd, tm, src, dest)
                    for k, v in zip(KEYS, c):
                        out[k] += v * w
                    if src[0] != i:
                        x_post[trans_index(fwd.x, src[0], i)] += w
                    if src[1] != j:
                        y_post[trans_index(fwd.y, src[1], j)] += w
    return out, x_post, y_post


def brute_force_indel_counts(fwd, tm):
    """the expectation over every path from the start cell to the end cell of the counts along it, carried counts included
    (cd.brute_force_indel_counts with transition_counts); exponential: a few residues only"""
    end = (fwd.x_size - 1, fwd.y_size - 1, EEE)
    tot = [0.]
    acc = [0.] * 6

    def walk(cell, lp, counts):
        if cell[0] == 0 and cell[1] == 0:
            if cell[2] != ho.SSS:
                return
            p = math.exp(lp)
            tot[0] += p
            for k in range(6):
                acc[k] += p * counts[k]
            return
        for src, tlp in fwd.source_transitions(cell).items():
            if tlp == NEG_INF:
                continue
            walk(src, lp + tlp, _add(counts, transition_counts(fwd, tm, src, cell)))

    walk(end, 0., ZERO)
    out = {k: acc[n] / tot[0] for n, k in enumerate(KEYS)}
    out["lp"] = math.log(tot[0])
    return out


def all_cells(fwd, bwd):
    """every cell of the lattice with a finite posterior probability, and the start and end cells (the cell set of a
    KeepAll profile in which each profile transition is one lower-level cell transition)"""
    cells = {fwd.start_cell, fwd.end_cell}
    for i in range(fwd.x_size - 1):
        for j in range(fwd.y_size - 1):
            if not fwd.in_envelope(i, j):
                continue
            for s in (ho.IMM, ho.IMD, ho.IDM, ho.IMI, ho.IIW):
                if fwd.cell(i, j, s) + bwd.cell(i, j, s) > NEG_INF:
                    cells.add((i, j, s))
    return cells


def read_fasta(path):
    """[(name, ungapped sequence)] of a FASTA file (gaps and the ancestral wildcard dropped)"""
    out = []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            out.append([line[1:].split()[0], ""])
        elif line and out:
            out[-1][1] += "".join(c for c in line if c not in "-.*")
    return [(n, s) for n, s in out]


def root_pair(model, seqs, times, strategy, kind="all", seed=1, band=None, samples=6, min_post_prob=.01):
    """The root of ((a,b),c) (three sequences) or ((a,b),(c,d)) (four), unfilled: child profiles built with `strategy`
    (which should hold CountIndelEvents) from every cell with a finite posterior (kind "all", KeepAll-style cell sets), from
    sampled traces ("sampled") or from the posterior ("posterior"); band: a left-justified guide alignment around which the
    root's fill is banded.  times = (a, b, c or (c,d) side, root-pair right branch)."""
    leaves = [ho.Profile.from_seq(model.components(), model.alphabet, s, k, "n%d" % k) for k, s in enumerate(seqs)]

    def hmm(tl, tr):
        return ho.PairHMM(ho.ProbModel(model, tl), ho.ProbModel(model, tr), model.ins_prob)

    def child(a, b, node, tl, tr, sd):
        f = CarryForwardMatrix(a, b, hmm(tl, tr), node, ho.GuideAlignmentEnvelope(), model)
        if kind == "all":
            return f.make_profile(all_cells(f, ho.BackwardMatrix(f)), strategy)
        if kind == "sampled":
            return f.sample_profile(ho.MT19937(sd), samples, 0, strategy | ho.DPMatrix.IncludeBestTrace)
        return ho.BackwardMatrix(f).post_prob_profile(min_post_prob, 0, strategy | ho.DPMatrix.IncludeBestTrace)

    x = child(leaves[0], leaves[1], 10, times[0], times[1], seed)
    y = leaves[2] if len(seqs) == 3 else child(leaves[2], leaves[3], 11, times[1], times[0], seed + 1)
    env = ho.GuideAlignmentEnvelope()
    if band is not None:
        cols = max(len(s) for s in seqs)
        guide = {k: [True] * len(s) + [False] * (cols - len(s)) for k, s in enumerate(seqs)}
        env = ho.GuideAlignmentEnvelope(guide, 0, 2, band)
    return CarryForwardMatrix(x, y, hmm(times[2], times[3]), 12, env, model, fill=False)


# ---- the count / fit loop of the reconstructor with fixed substitution rates (src/recon.cpp:917-1050, 1373-1410) -----------
def reconstruct_counts(model, tree, seqs, profile_samples=10, seed=5489):
    """Reconstructor::reconstruct under accumulateIndelCounts, no guide, reconstructRoot = false: ho.reconstruct's loop with
    profiles that carry counts (sampled, CollapseChains | IncludeBestTrace | CountIndelEvents) and, at the root, Backward and
    getCounts.  Fills by the plain-C oracle (bit for bit what the exact policy computes).  -> counts dict with lp"""
    from tests import recon_helpers as RH
    gen = ho.MT19937(seed)
    strategy = ho.DPMatrix.CollapseChains | ho.DPMatrix.IncludeBestTrace | ho.DPMatrix.CountIndelEvents
    prof = {}
    for node in range(tree.nodes()):
        if tree.is_leaf(node):
            name, s = seqs[node]
            prof[node] = ho.Profile.from_seq(model.components(), model.alphabet, s, node, name)
            continue
        lc, rc = tree.child[node]
        pm = [ho.ProbModel(model, tree.branch_length[c], [ho.sub_prob_matrix_ss(sr, tree.branch_length[c]) for sr in model.sub_rate])
              for c in (lc, rc)]
        fwd = CarryArrayForward(prof[lc], prof[rc], ho.PairHMM(pm[0], pm[1], model.ins_prob), node, ho.GuideAlignmentEnvelope(), model)
        if node == tree.root():
            counts, _, _ = get_indel_counts(RH.ArrayBackward(fwd), fwd.tm)
            return counts
        prof[node] = fwd.sample_profile(gen, profile_samples, 0, strategy)


def log_prior(model, c):
    """IndelCounts::logPrior of the mirror (EventCounts::logPrior, src/model.cpp:1060-1067; the gamma and beta densities in
    lgamma form)"""
    def gamma(rate, events, wait):
        a = events + 1
        return (a - 1) * math.log(rate) - rate * wait - math.lgamma(a) + a * math.log(wait)

    def beta(p, yes, no):
        a, b = yes + 1, no + 1
        return math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + (a - 1) * math.log(p) + (b - 1) * math.log(1 - p)
    return (gamma(model.ins_rate, c["ins"], c["insTime"]) + gamma(model.del_rate, c["del"], c["delTime"])
            + beta(model.ins_ext_prob, c["insExt"], c["ins"]) + beta(model.del_ext_prob, c["delExt"], c["del"]))


def fit(model, families, max_iter=100, min_inc=.001):
    """Reconstructor::fit with the substitution rates fixed and Laplace pseudocounts IndelCounts(1, 1): families = [(tree,
    seqs)]; updates model's indel rates in place -> [log-likelihood + log-prior of every iteration]"""
    prior = dict.fromkeys(KEYS, 1.)
    lp_last, lps = NEG_INF, []
    for _ in range(max_iter):
        data = dict.fromkeys(KEYS + ("lp",), 0.)
        for tree, seqs in families:
            c = reconstruct_counts(model, tree, seqs)
            for k in data:
                data[k] += c[k]
        lp = data["lp"] + log_prior(model, prior)
        lps.append(lp)
        if lp <= lp_last + abs(lp_last) * min_inc:
            break
        dp = {k: data[k] + prior[k] for k in KEYS}
        model.ins_rate = dp["ins"] / dp["insTime"]
        model.del_rate = dp["del"] / dp["delTime"]
        model.ins_ext_prob = dp["insExt"] / (dp["insExt"] + dp["ins"])
        model.del_ext_prob = dp["delExt"] / (dp["delExt"] + dp["del"])
        lp_last = lp
    return lps


class CarryArrayForward(CarryForwardMatrix):
    """CarryForwardMatrix whose cells come from the plain-C oracle fill (tests/recon_helpers.ArrayForward)"""

    def __init__(self, x, y, hmm, node, env, model):
        from oracle import c_oracle
        from tests import helpers as H
        super().__init__(x, y, hmm, node, env, model, fill=False)
        r = c_oracle.forward(*H.job_images(self))
        self.arr = r["cells"]
        self.lp_end = r["lp_end"]

    def cell(self, i, j, s):
        if i >= self.arr.shape[0] or j >= self.arr.shape[1]:
            return NEG_INF
        return float(self.arr[i, j, s])

    def xy_cell(self, i, j):
        if i >= self.arr.shape[0] or j >= self.arr.shape[1]:
            return ho._EMPTY_CELL
        return [float(v) for v in self.arr[i, j]]
