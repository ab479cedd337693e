"""TEST INFRASTRUCTURE ONLY - CPU restatement of the sibling-pair parent-proposal DP of SURVEY.md section 8(f) row N4:
Sampler::SiblingMatrix (reference src/sampler.h:226-325, src/sampler.cpp:1185-1608), the eleven-state alignment of a left
child profile and a right child profile under their unobserved parent, over TreeAlignFuncs::SparseDPMatrix<11> inside a
GuideAlignmentEnvelope: the 35 transition scores (lpTrans / lpTransElimSelfLoopIDD / lpTransElimWait), the fill, lpEnd,
lpEmit, getState / getColumn, sample, logPostProb, parentSeq.

PARITY UNPINNED BY REFERENCE FIXTURES: no reference fixture holds a sibling matrix - the reference cannot be built for want
of GSL, and none of its tests drives the sampler.  The restatement is pinned by enumeration only
(tests/test_oracle_sibling.py): on tiny children every history is listed and scored in plain floating point; lpEnd is the
log of the summed history probabilities, the posteriors of the alignments sum to one, sampled alignments occur as often as
their posterior says."""
import math
from collections import namedtuple

from oracle.branch_oracle import calc_ins_probs, pre_multiply
from oracle.historian_oracle import NEG_INF, log_sum_exp, log_sum_exp_slow, safe_log

# SiblingMatrix::State (src/sampler.h:227-234); SSS = IMM, SSI = IMI, SIW = IIW
IMM, IMD, IDM, IDD, WWW, WWX, WXW, IMI, IIW, IDI, IIX, EEE = range(12)
SSS = IMM
N_STATES = 11
STATE_NAMES = ("IMM", "IMD", "IDM", "IDD", "WWW", "WWX", "WXW", "IMI", "IIW", "IDI", "IIX", "EEE")
EMPTY = (NEG_INF,) * N_STATES

# what the transition scores need of a branch's ProbModel (src/model.cpp:374-391); oracle.historian_oracle.ProbModel has
# the same attribute names
Indel = namedtuple("Indel", "ins dele ins_ext del_ext")


def log_sum_exp_libm(a, b, *rest):
    """the n-ary left-nested sum in libm arithmetic (log_sum_exp_slow, src/logsumexp.cpp:22-37)"""
    ret = log_sum_exp_slow(a, b)
    for c in rest:
        ret = log_sum_exp_slow(ret, c)
    return ret


def get_state(src, left, right, parent):
    """SiblingMatrix::getState (src/sampler.cpp:1424-1436): the state of a column after state src"""
    if parent:
        return (IMM if right else IMD) if left else (IDM if right else IDD)
    if left:
        return IIX if src in (IMD, IIX) else IIW
    if right:
        return IDI if src in (IDM, IDI) else IMI
    if src in (IDM, IDD, IDI):
        return WXW
    if src in (IMD, IIX):
        return WWX
    return WWW


def get_column(i, j, state):
    """SiblingMatrix::getColumn (src/sampler.cpp:1438-1449): (left, right, parent) ungapped in the column state emits at (i, j)"""
    if state == IMM:
        return (True, True, True) if i > 0 and j > 0 else (False, False, False)
    if state == IMD:
        return True, False, True
    if state == IDM:
        return False, True, True
    if state == IDD:
        return False, False, True
    if state in (IIW, IIX):
        return i > 0, False, False
    if state in (IMI, IDI):
        return False, j > 0, False
    return False, False, False


class SiblingMatrix:
    """l_sub, r_sub: the children's profiles through their branches' substitution matrices (pre_multiply), [pos][cpt][tok];
    log_root[cpt][tok]: log insProb with log cptWeight added (the constructor's loop, src/sampler.cpp:1203-1205);
    l_emit, r_emit: calc_ins_probs; l_pm, r_pm: the branches' ProbModels (ins, dele, ins_ext, del_ext); ins_ext_prob:
    RateModel::insExtProb = Sampler::rootExtProb; l_env / r_env: envelope coordinate of every position 0 .. len, or None with
    max_dist < 0; lse: the n-ary log_sum_exp of the fill and the walks - the reference's table operator unless told."""

    def __init__(self, l_sub, r_sub, log_root, l_emit, r_emit, l_pm, r_pm, ins_ext_prob, l_env=None, r_env=None, max_dist=-1,
                 lse=log_sum_exp, fill=True):
        self.l_sub, self.r_sub, self.log_root, self.l_emit, self.r_emit = l_sub, r_sub, log_root, l_emit, r_emit
        self.l_pm, self.r_pm, self.root_ext_prob = l_pm, r_pm, ins_ext_prob
        self.x_size, self.y_size = len(l_sub) + 1, len(r_sub) + 1
        self.l_env, self.r_env, self.max_dist = l_env, r_env, max_dist
        self.lse = lse
        # [src][dest], lpTransElimSelfLoopIDD: 35 finite entries at most, -inf where the reference has no member
        self.T = [[self.lp_trans_elim_self_loop_idd(s, d) for d in range(12)] for s in range(N_STATES)]
        self.cells = {}
        self.lp_end = NEG_INF
        self._match = {}
        if fill:
            self.fill()

    @classmethod
    def from_profiles(cls, model, l_seq, r_seq, l_pm, r_pm, **kw):
        """the constructor's initialiser list (src/sampler.cpp:1185-1201) from a RateModel, the children's PosWeightMatrices
        and the two ProbModels (oracle.historian_oracle classes)"""
        def log_sub(pm):
            return [[[safe_log(v) for v in row] for row in m] for m in pm.sub_mat]

        def log_ins(pm):
            return [[safe_log(v) for v in iv] for iv in pm.ins_vec]

        def log_w(pm):
            return [safe_log(w) for w in pm.cpt_weight]
        log_root = [[safe_log(float(v)) + math.log(model.cpt_weight[c]) for v in ip] for c, ip in enumerate(model.ins_prob)]
        return cls(pre_multiply(l_seq, log_sub(l_pm)), pre_multiply(r_seq, log_sub(r_pm)), log_root,
                   calc_ins_probs(l_seq, log_ins(l_pm), log_w(l_pm)), calc_ins_probs(r_seq, log_ins(r_pm), log_w(r_pm)),
                   l_pm, r_pm, model.ins_ext_prob, **kw)

    # ---- transition scores (src/sampler.h:290-315, src/sampler.cpp:1451-1574) ----
    def idd_self_loop_prob(self):
        return self.root_ext_prob * self.l_pm.del_ext * self.r_pm.del_ext

    def idd_stay(self):
        return safe_log(self.idd_self_loop_prob())

    def idd_exit(self):
        return math.log(1 / (1 - self.idd_self_loop_prob()))

    def lp_trans(self, src, dest):
        """SiblingMatrix::lpTrans (src/sampler.cpp:1459-1566)"""
        L, R, log = self.l_pm, self.r_pm, safe_log
        root_ext, root_no_ext = log(self.root_ext_prob), log(1 - self.root_ext_prob)
        l_ins, l_del, l_ins_ext, l_del_ext = log(L.ins), log(L.dele), log(L.ins_ext), log(L.del_ext)
        l_no_ins, l_no_del, l_no_ins_ext, l_no_del_ext = log(1 - L.ins), log(1 - L.dele), log(1 - L.ins_ext), log(1 - L.del_ext)
        r_ins, r_del, r_ins_ext, r_del_ext = log(R.ins), log(R.dele), log(R.ins_ext), log(R.del_ext)
        r_no_ins, r_no_del, r_no_ins_ext, r_no_del_ext = log(1 - R.ins), log(1 - R.dele), log(1 - R.ins_ext), log(1 - R.del_ext)
        if src == IMM:
            if dest == WWW: return l_no_ins + r_no_ins
            if dest == IMI: return r_ins
            if dest == IIW: return l_ins + r_no_ins
        elif src == IMD:
            if dest == WWX: return l_no_ins
            if dest == IIX: return l_ins
        elif src == IDM:
            if dest == WXW: return r_no_ins
            if dest == IDI: return r_ins
        elif src == IDD:
            if dest == IDD: return self.idd_stay()
            if dest == IMM: return root_ext + l_no_del_ext + r_no_del_ext
            if dest == IMD: return root_ext + l_no_del_ext + r_del_ext
            if dest == IDM: return root_ext + l_del_ext + r_no_del_ext
            if dest == EEE: return root_no_ext + l_no_del_ext + r_no_del_ext
        elif src == WWW:
            if dest == IMM: return root_ext + l_no_del + r_no_del
            if dest == IMD: return root_ext + l_no_del + r_del
            if dest == IDM: return root_ext + l_del + r_no_del
            if dest == IDD: return root_ext + l_del + r_del
            if dest == EEE: return 0.
        elif src == WWX:
            if dest == IMM: return root_ext + l_no_del + r_no_del_ext
            if dest == IMD: return root_ext + l_no_del + r_del_ext
            if dest == IDM: return root_ext + l_del + r_no_del_ext
            if dest == IDD: return root_ext + l_del + r_del_ext
            if dest == EEE: return r_no_del_ext
        elif src == WXW:
            if dest == IMM: return root_ext + l_no_del_ext + r_no_del
            if dest == IMD: return root_ext + l_no_del_ext + r_del
            if dest == IDM: return root_ext + l_del_ext + r_no_del
            if dest == IDD: return root_ext + l_del_ext + r_del
            if dest == EEE: return l_no_del_ext
        elif src == IMI:
            if dest == WWW: return l_no_ins + r_no_ins_ext
            if dest == IMI: return r_ins_ext
            if dest == IIW: return l_ins + r_no_ins_ext
        elif src == IIW:
            if dest == WWW: return l_no_ins_ext
            if dest == IIW: return l_ins_ext
        elif src == IDI:
            if dest == WXW: return r_no_ins_ext
            if dest == IDI: return r_ins_ext
        elif src == IIX:
            if dest == WWX: return l_no_ins_ext
            if dest == IIX: return l_ins_ext
        return NEG_INF

    def lp_trans_elim_self_loop_idd(self, src, dest):
        """src/sampler.cpp:1451-1457"""
        if src == IDD:
            return NEG_INF if dest == IDD else self.lp_trans(src, dest) + self.idd_exit()
        return self.lp_trans(src, dest)

    def lp_trans_elim_wait(self, src, dest):
        """src/sampler.cpp:1568-1574"""
        t = self.lp_trans
        return self.lse(t(src, dest), t(src, WWW) + t(WWW, dest), t(src, WWX) + t(WWX, dest), t(src, WXW) + t(WXW, dest))

    # ---- lattice ----
    def in_envelope(self, i, j):
        """SparseDPMatrix::inEnvelope (src/sampler.h:146-149) with GuideAlignmentEnvelope::inRange (src/alignpath.h:56-61)"""
        if i == 0 or j == 0 or i == self.x_size - 1 or j == self.y_size - 1 or self.max_dist < 0:
            return True
        return abs(self.l_env[i] - self.r_env[j]) <= self.max_dist

    def cell(self, i, j, s):
        """SparseDPMatrix::cell (src/sampler.h:127-137): state EEE is lpEnd at the last cell"""
        if s == EEE:
            return self.lp_end if (i == self.x_size - 1 and j == self.y_size - 1) else NEG_INF
        return self.cells.get((i, j), EMPTY)[s]

    def log_match(self, i, j):
        """SiblingMatrix::logMatch (src/sampler.h:317-322): over the components, the three-vector logInnerProduct
        (src/logsumexp.h:139-144)"""
        got = self._match.get((i, j))
        if got is None:
            lse, got = self.lse, NEG_INF
            for root, ls, rs in zip(self.log_root, self.l_sub[i - 1], self.r_sub[j - 1]):
                lip = NEG_INF
                for a, b, c in zip(root, ls, rs):
                    lip = lse(lip, a + b + c)
                got = lse(got, lip)
            self._match[(i, j)] = got
        return got

    def fill(self):
        """src/sampler.cpp:1253-1333.  Inside a cell: the left block, the right block, the diagonal block - each only if its
        source cell is inside the envelope - then IDD from the wait states of the same cell"""
        T, lse, cells, env = self.T, self.lse, self.cells, self.in_envelope
        imm_www, imm_imi, imm_iiw = T[IMM][WWW], T[IMM][IMI], T[IMM][IIW]
        imd_wwx, imd_iix, idm_wxw, idm_idi = T[IMD][WWX], T[IMD][IIX], T[IDM][WXW], T[IDM][IDI]
        idd_imm, idd_imd, idd_idm = T[IDD][IMM], T[IDD][IMD], T[IDD][IDM]
        www_imm, www_imd, www_idm, www_idd = T[WWW][IMM], T[WWW][IMD], T[WWW][IDM], T[WWW][IDD]
        wwx_imm, wwx_imd, wwx_idm, wwx_idd = T[WWX][IMM], T[WWX][IMD], T[WWX][IDM], T[WWX][IDD]
        wxw_imm, wxw_imd, wxw_idm, wxw_idd = T[WXW][IMM], T[WXW][IMD], T[WXW][IDM], T[WXW][IDD]
        imi_www, imi_imi, imi_iiw = T[IMI][WWW], T[IMI][IMI], T[IMI][IIW]
        iiw_www, iiw_iiw, idi_wxw, idi_idi, iix_wwx, iix_iix = T[IIW][WWW], T[IIW][IIW], T[IDI][WXW], T[IDI][IDI], T[IIX][WWX], T[IIX][IIX]
        for i in range(self.x_size):
            for j in range(self.y_size):
                if not env(i, j):
                    continue
                d = [NEG_INF] * N_STATES
                if i == 0 and j == 0:
                    d[SSS] = 0.                      # lpStart() = 0
                    d[WWW] = imm_www
                if i > 0 and env(i - 1, j):
                    s = cells.get((i - 1, j), EMPTY)
                    e = self.l_emit[i - 1]
                    d[IIW] = e + lse(s[IMM] + imm_iiw, s[IMI] + imi_iiw, s[IIW] + iiw_iiw)
                    d[IIX] = e + lse(s[IMD] + imd_iix, s[IIX] + iix_iix)
                    d[IMD] = e + lse(s[WWW] + www_imd, s[WWX] + wwx_imd, s[WXW] + wxw_imd, s[IDD] + idd_imd)
                    d[WWW] = d[IIW] + iiw_www
                    d[WWX] = lse(d[IIX] + iix_wwx, d[IMD] + imd_wwx)
                if j > 0 and env(i, j - 1):
                    s = cells.get((i, j - 1), EMPTY)
                    e = self.r_emit[j - 1]
                    d[IMI] = e + lse(s[IMM] + imm_imi, s[IMI] + imi_imi)
                    d[IDI] = e + lse(s[IDM] + idm_idi, s[IDI] + idi_idi)
                    d[IDM] = e + lse(s[WWW] + www_idm, s[WWX] + wwx_idm, s[WXW] + wxw_idm, s[IDD] + idd_idm)
                    d[WWW] = lse(d[WWW], d[IMI] + imi_www)
                    d[WXW] = lse(d[IDI] + idi_wxw, d[IDM] + idm_wxw)
                if i > 0 and j > 0 and env(i - 1, j - 1):
                    s = cells.get((i - 1, j - 1), EMPTY)
                    d[IMM] = self.log_match(i, j) + lse(s[WWW] + www_imm, s[WWX] + wwx_imm, s[WXW] + wxw_imm, s[IDD] + idd_imm)
                    d[WWW] = lse(d[WWW], d[IMM] + imm_www)
                d[IDD] = lse(d[WWW] + www_idd, d[WWX] + wwx_idd, d[WXW] + wxw_idd)
                cells[(i, j)] = d
        e = cells.get((self.x_size - 1, self.y_size - 1), EMPTY)
        self.lp_end = lse(e[IDD] + T[IDD][EEE], e[WWW] + T[WWW][EEE], e[WWX] + T[WWX][EEE], e[WXW] + T[WXW][EEE])

    def lp_emit(self, i, j, state):
        """SiblingMatrix::lpEmit (src/sampler.cpp:1414-1422)"""
        if state == IMM:
            return self.log_match(i, j) if i > 0 and j > 0 else NEG_INF
        if state in (IDM, IMI, IDI):
            return self.r_emit[j - 1] if j > 0 else NEG_INF
        if state in (IMD, IIW, IIX):
            return self.l_emit[i - 1] if i > 0 else NEG_INF
        return 0.

    # ---- walks ----
    def sample(self, source):
        """SiblingMatrix::sample (src/sampler.cpp:1343-1386): (left, right, parent) rows of booleans, first column first.
        source.uniform() is random_double (a uniform in [0, 1)), source.geometric(p) a draw of
        std::geometric_distribution<int>(p) - failures before the first success of probability p."""
        i, j, state = self.x_size - 1, self.y_size - 1, EEE
        lp, rp, pp = [], [], []
        while i > 0 or j > 0:
            l, r, p = get_column(i, j, state)
            if l or r or p:
                lp.append(l), rp.append(r), pp.append(p)
            if state == IDD:        # IDD self-loops are added outside the main traceback step
                for _ in range(source.geometric(self.idd_self_loop_prob())):
                    lp.append(l), rp.append(r), pp.append(p)
            si, sj = (i - 1 if l else i), (j - 1 if r else j)
            e = self.lp_emit(i, j, state)
            src = self.cells.get((si, sj), EMPTY)
            w = [src[s] + self.T[s][state] + e for s in range(N_STATES)]       # keys in state order: one cell, map order
            top = max(w)
            assert top > NEG_INF, "traceback state has zero probability at cell (%d,%d,%d)" % (i, j, state)
            # random_key_log (src/util.h:220-236)
            norm = 0.
            for v in w:
                norm += math.exp(v - top)
            variate = source.uniform() * norm
            for s, v in enumerate(w):
                variate -= math.exp(v - top)
                if variate <= 0:
                    break
            else:
                raise AssertionError("random_key_log failed")
            i, j, state = si, sj, s
        return lp[::-1], rp[::-1], pp[::-1]

    def log_post_prob(self, path):
        """SiblingMatrix::logPostProb (src/sampler.cpp:1388-1412) of (left, right, parent) rows"""
        lrow, rrow, prow = path
        lp, i, j, state = 0., 0, 0, SSS
        for dl, dr, dp in zip(lrow, rrow, prow):
            if dl:
                i += 1
            if dr:
                j += 1
            prev, state = state, get_state(state, dl, dr, dp)
            if i >= self.x_size or j >= self.y_size or not self.in_envelope(i, j):
                return NEG_INF
            lp += self.lp_trans_elim_wait(prev, state) + self.lp_emit(i, j, state)
            lp = min(lp, self.cell(i, j, state))         # "mitigate precision errors"
        lp += self.lp_trans_elim_wait(state, EEE)
        lp = min(lp, self.lp_end)
        return lp - self.lp_end

    def parent_seq(self, path):
        """SiblingMatrix::parentSeq (src/sampler.cpp:1576-1608): the parent's profile [pos][cpt][tok], every position normalised"""
        lrow, rrow, prow = path
        pwm, lpos, rpos = [], 0, 0
        for dl, dr, dp in zip(lrow, rrow, prow):
            if not dp:
                # (the reference advances its child positions only inside parent columns: src/sampler.cpp:1582-1596)
                continue
            prof = [[0.] * len(root) for root in self.log_root]
            if dl:
                for c, row in enumerate(prof):
                    for a in range(len(row)):
                        row[a] += self.l_sub[lpos][c][a]
                lpos += 1
            if dr:
                for c, row in enumerate(prof):
                    for a in range(len(row)):
                        row[a] += self.r_sub[rpos][c][a]
                rpos += 1
            norm = NEG_INF
            for row in prof:
                for v in row:
                    norm = self.lse(norm, v)
            pwm.append([[v - norm for v in row] for row in prof])
        return pwm


class ListSource:
    """uniforms and geometric draws from a random.Random (tests) - the walk consumes them in the reference's order"""

    def __init__(self, rng):
        self.rng = rng

    def uniform(self):
        return self.rng.random()

    def geometric(self, p):
        # failures before the first success of probability p
        n = 0
        while self.rng.random() >= p:
            n += 1
        return n


class MTSource:
    """draws as std::mt19937 gives them to the reference: random_double (src/util.h:138-142) is one 32-bit word over 2^32;
    std::geometric_distribution<int>(p) as libstdc++ draws it - floor(log(1 - u) / log(1 - p)) over one canonical uniform
    (two words)"""

    def __init__(self, mt):
        self.mt = mt

    def uniform(self):
        return self.mt.next_u32() / 4294967296.0

    def geometric(self, p):
        u = self.mt.canonical()
        return int(math.floor(math.log(1. - u) / math.log(1. - p))) if 0. < p < 1. else 0


def random_case(seed, nx, ny, C=1, A=4, band=None, one_hot=False, sorted_env=True):
    """constructor arguments of a random sibling pair: profiles (or leaf-like one-hot columns) of nx and ny positions through
    random substitution matrices, random indel parameters; band: maxDistance with random envelope coordinates"""
    import random
    rng = random.Random(seed)

    def pwm(n):
        if one_hot:
            rows = []
            for _ in range(n):
                k = rng.randrange(A)
                rows.append([[0. if a == k else NEG_INF for a in range(A)] for _ in range(C)])
            return rows
        return [[[math.log(rng.uniform(.01, 1.)) for _ in range(A)] for _ in range(C)] for _ in range(n)]

    def log_sub():
        out = []
        for _ in range(C):
            m = [[rng.uniform(.05, 1.) + (3. if i == j else 0.) for j in range(A)] for i in range(A)]
            out.append([[math.log(v / sum(row)) for v in row] for row in m])
        return out
    l_seq, r_seq = pwm(nx), pwm(ny)
    l_log_sub, r_log_sub = log_sub(), log_sub()
    w = [rng.uniform(.2, 1.) for _ in range(C)]
    log_w = [math.log(v / sum(w)) for v in w]
    root = []
    for c in range(C):
        v = [rng.uniform(.1, 1.) for _ in range(A)]
        root.append([math.log(x / sum(v)) for x in v])
    log_root = [[root[c][a] + log_w[c] for a in range(A)] for c in range(C)]
    ins_ext, del_ext = rng.uniform(.3, .9), rng.uniform(.3, .9)
    l_pm = Indel(rng.uniform(.01, .3), rng.uniform(.01, .3), ins_ext, del_ext)
    r_pm = Indel(rng.uniform(.01, .3), rng.uniform(.01, .3), ins_ext, del_ext)
    l_env = r_env = None
    md = -1
    if band is not None:
        if sorted_env:       # as a guide alignment gives them: non-decreasing match counts along either sequence
            l_env, r_env = [0], [0]
            for _ in range(nx):
                l_env.append(l_env[-1] + (rng.random() < .9))
            for _ in range(ny):
                r_env.append(r_env[-1] + (rng.random() < .9))
        else:
            l_env = [0] + [rng.randint(0, max(nx, ny)) for _ in range(nx)]
            r_env = [0] + [rng.randint(0, max(nx, ny)) for _ in range(ny)]
        md = band
    return dict(l_sub=pre_multiply(l_seq, l_log_sub), r_sub=pre_multiply(r_seq, r_log_sub), log_root=log_root,
                l_emit=calc_ins_probs(l_seq, root, log_w), r_emit=calc_ins_probs(r_seq, root, log_w), l_pm=l_pm, r_pm=r_pm,
                ins_ext_prob=ins_ext, l_env=l_env, r_env=r_env, max_dist=md)
