"""Guide-alignment Viterbi at its edges: the cases shared by tests/test_oracle_quickalign_edges.py (which pins the yardstick and
the case set on the CPU) and tests/test_gpu_quickalign_edges.py (k_quickalign against the C oracle, bit for bit).

Every pair of tests/test_gpu_quickalign.py is a random protein pair under real-valued log scores, where no two cells ever tie.
Here the scores are small integers (ties of the end cell in most pairs, so that the reference's column-major scan order decides),
the shapes sit on the kernel's seams (64-row strips, the 16-column publish lag, the first lagged publish at 80 columns, 7000
columns of LDS tables), the envelopes are degenerate, and the batches are large enough for the narrow launches.

A case is (name, x_tok, y_tok, alph, submat, scores[11], diagonals or None): the job tuple of capi.QuickBatch behind a name."""
import functools
import os

import numpy as np

from historian_amd import capi
from oracle import c_oracle
from oracle import historian_oracle as ho
from oracle import quickalign_oracle as q

NEG_INF = float("-inf")
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
SCORE_NAMES = capi.QuickBatch.SCORE_NAMES
# 31 letters for the Python restatement, which takes text; '*' is outside every alphabet (token -1)
TEXT = "abcdefghijklmnopqrstuvwxyz01234"

# ---- score sets (zeros are +0.0: v_max_f64 and std::max part on the sign of zero) --------------------------------------------
# match +2 / mismatch -1 on four letters; opening a gap from a match or closing an insert into a delete -3, extending -1,
# every other transition and the three end-gap constants 0
_INTEGER = dict(m2m=0.0, m2i=-3.0, m2d=-3.0, i2i=-1.0, i2m=0.0, i2d=-3.0, d2d=-1.0, d2m=0.0, gap_open=0.0, gap_extend=0.0,
                no_gap=0.0)
_SETS = {
    "integer": _INTEGER,
    "no_gaps": dict(_INTEGER, m2i=NEG_INF, m2d=NEG_INF, i2d=NEG_INF),
    # end gaps that cost: the unsigned wrap of len - i - 2 at i = len - 1 (4294967295 extensions) shows on integer values
    "costly_ends": dict(_INTEGER, gap_open=-5.0, gap_extend=-1.0, no_gap=0.0),
}
SCORE_SETS = ("amino", "integer", "no_gaps", "costly_ends")


@functools.lru_cache(None)
def _amino():
    model = ho.RateModel.from_file(os.path.join(G, "testamino.json"))
    model.sub_rate = [m.tolist() for m in model.sub_rate]
    sc = q.QuickAlignScores(model, 1.0)
    return len(model.alphabet), np.array(sc.submat, dtype=np.float64), [getattr(sc, n) for n in SCORE_NAMES]


def score_set(name):
    """-> (alphabet size, submat, scores[11])"""
    if name == "amino":
        return _amino()
    return 4, match_mismatch(4), [_SETS[name][n] for n in SCORE_NAMES]


def match_mismatch(alph):
    return np.where(np.eye(alph, dtype=bool), 2.0, -1.0)


def random_submat(rng, alph):
    """symmetric, integer-valued, in -4 .. 4 with a positive diagonal"""
    m = rng.integers(-4, 5, size=(alph, alph))
    m = np.triu(m) + np.triu(m, 1).T
    m[np.arange(alph), np.arange(alph)] = rng.integers(1, 5, size=alph)
    return m.astype(np.float64)


# ---- sequences -------------------------------------------------------------------------------------------------------------------
def random_tokens(rng, alph, n):
    return rng.integers(0, alph, size=n).astype(np.int32)


def related_pair(rng, alph, lx, ly, sub=.15):
    """y: the first ly tokens of x with a fraction `sub` redrawn, padded with random tokens (the pairs of test_gpu_quickalign.py)"""
    x = random_tokens(rng, alph, lx)
    y = random_tokens(rng, alph, ly)
    n = min(lx, ly)
    keep = rng.random(n) > sub
    y[:n] = np.where(keep, x[:n], y[:n])
    return x, y


def case(name, x, y, set_name, diagonals=None, alph=None, submat=None):
    a, sm, sv = score_set(set_name)
    if alph is not None:
        a, sm = alph, submat
    d = None if diagonals is None else [int(v) for v in diagonals]
    return (name, np.ascontiguousarray(x, dtype=np.int32), np.ascontiguousarray(y, dtype=np.int32), a, sm, sv, d)


def transposed(c, name):
    n, x, y, a, sm, sv, d = c
    return (name, y, x, a, sm.T.copy(), sv, None if d is None else [-v for v in d])


def cut(c, rows, cols):
    """the leading rows x cols corner of a full-envelope case"""
    n, x, y, a, sm, sv, d = c
    assert d is None
    return ("%s[:%d,:%d]" % (n, rows, cols), x[:rows].copy(), y[:cols].copy(), a, sm, sv, None)


# ---- the oracle, once per case -----------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(c):
    """c_oracle.quickalign of the case: dict(cells [(xlen+1),(ylen+1),3], score, x_end, y_end); computed once per name and never
    written to (the arrays are read-only)"""
    name, x, y, a, sm, sv, d = c
    r = _ORACLE.get(name)
    if r is None:
        r = c_oracle.quickalign(x, y, a, sm, c_oracle.QAScores(*sv), d)
        r["cells"].setflags(write=False)
        _ORACLE[name] = r
    return r


def end_gaps(c):
    """endGapScore(i, j) for 1 <= i <= xlen, 1 <= j <= ylen, as the reference adds it: (x part) + (y part), SeqIdx unsigned"""
    name, x, y, a, sm, sv, d = c
    s = dict(zip(SCORE_NAMES, sv))

    def part(n):
        k = np.arange(1, n + 1, dtype=np.int64)
        wrapped = ((n - k - 2) & 0xFFFFFFFF).astype(np.float64)
        return np.where(k == n, s["no_gap"], s["gap_open"] + wrapped * s["gap_extend"])
    return part(len(x))[:, None] + part(len(y))[None, :]


def maximal_cells(c):
    """(i, j) of every cell whose mat + endGap equals the oracle's score, in (i, j) order; none when the score is -inf"""
    r = oracle(c)
    if r["score"] == NEG_INF:
        return []
    hit = (r["cells"][1:, 1:, 0] + end_gaps(c)) == r["score"]
    return [(int(i) + 1, int(j) + 1) for i, j in np.argwhere(hit)]


# ---- ties of the end cell ----------------------------------------------------------------------------------------------------------
TIE_SIZES = ((130, 70), (70, 130), (200, 200), (129, 65))
TIE_CLASSES = ("several_maxima", "row_major_differs", "winner_below_strip_0", "several_in_column", "several_in_row")
TIE_PER_CLASS = 8
TIE_SEARCH = 1600


def tie_classes(c):
    """the classes (of TIE_CLASSES) the pair belongs to"""
    r = oracle(c)
    cells = maximal_cells(c)
    win = (r["x_end"], r["y_end"])
    out = set()
    if len(cells) > 1:
        out.add("several_maxima")
        if cells[0] != win:                                    # the first maximal cell of a row-major scan
            out.add("row_major_differs")
        if win[0] > 64:
            out.add("winner_below_strip_0")
        if sum(1 for i, j in cells if j == win[1]) > 1:
            out.add("several_in_column")
        if sum(1 for i, j in cells if i == win[0]) > 1:
            out.add("several_in_row")
    return out


@functools.lru_cache(None)
def random_tie_cases():
    """Seeded random 4-letter pairs of TIE_SIZES under `integer`: the first TIE_PER_CLASS of every class among TIE_SEARCH pairs.
    -> (cases, {class: [names]})"""
    members = {k: [] for k in TIE_CLASSES}
    kept = []
    for n in range(TIE_SEARCH):
        lx, ly = TIE_SIZES[n % len(TIE_SIZES)]
        rng = np.random.default_rng(7000 + n)
        x, y = related_pair(rng, 4, lx, ly, sub=.25) if (n // 4) % 2 else (random_tokens(rng, 4, lx), random_tokens(rng, 4, ly))
        c = case("tie_%03d_%dx%d" % (n, lx, ly), x, y, "integer")
        wanted = [k for k in tie_classes(c) if len(members[k]) < TIE_PER_CLASS]
        if wanted:
            kept.append(c)
            for k in wanted:
                members[k].append(c[0])
        else:
            _ORACLE.pop(c[0], None)
        if all(len(v) >= TIE_PER_CLASS for v in members.values()):
            break
    return tuple(kept), members


TANDEM_UNITS = ((0, 1, 2, 3, 3, 1, 0), (2, 2, 0, 3, 1, 0, 1))


@functools.lru_cache(None)
def repeat_tie_cases():
    """A 7-mer x 30 against the same 7-mer x 3 (28 tied cells in one column: every copy of the short one ends a perfect match),
    a homopolymer pair without gap transitions (mat = 2 min(i, j): 61 tied cells in the last column), and their transposes
    (the ties then lie in one row, and the lane's own `first j` decides)"""
    out = []
    for n, unit in enumerate(TANDEM_UNITS):
        c = case("tandem_%d_210x21" % n, np.tile(unit, 30), np.tile(unit, 3), "integer")
        out += [c, transposed(c, "tandem_%d_21x210" % n)]
    c = case("homopolymer_130x70", np.zeros(130), np.zeros(70), "no_gaps")
    out += [c, transposed(c, "homopolymer_70x130")]
    return tuple(out)


def tie_cases():
    return random_tie_cases()[0] + repeat_tie_cases()


# ---- shapes round the strips and the publish logic ---------------------------------------------------------------------------------
GRID_ROWS = (1, 2, 63, 64, 65, 128, 129)
GRID_COLS = (1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 128, 129)


@functools.lru_cache(None)
def shape_grid_cases():
    """Every rows x columns pairing (91), `amino` and `integer` by turns, and 1089 x 17: 18 strips on the 16 waves of the default
    launch (two waves take a second strip) at one column over the lag"""
    out = []
    shapes = [(r, cc) for r in GRID_ROWS for cc in GRID_COLS] + [(1089, 17)]
    for n, (lx, ly) in enumerate(shapes):
        set_name = "integer" if n % 2 else "amino"
        x, y = related_pair(np.random.default_rng(7500 + n), score_set(set_name)[0], lx, ly)
        out.append(case("grid_%dx%d_%s" % (lx, ly, set_name), x, y, set_name))
    return tuple(out)


# ---- alphabets and tokens outside them -----------------------------------------------------------------------------------------------
ALPHABETS = (1, 4, 20, 31)
FOREIGN_X = (0, 63, 64, 65, 129)       # position 0, the rows either side of the strip seam, the last position
FOREIGN_Y = (0, 63, 64, 69)


@functools.lru_cache(None)
def alphabet_cases():
    """130 x 70 pairs under the integer transitions with a random symmetric integer substitution matrix: alphabets of 1 (a
    homopolymer: ties everywhere), 4, 20 and 31 (the kernel's limit) letters, clean and with tokens of -1"""
    out = []
    for a in ALPHABETS:
        rng = np.random.default_rng(7700 + a)
        sm = random_submat(rng, a)
        x, y = related_pair(rng, a, 130, 70)
        out.append(case("alph%d_clean" % a, x, y, "integer", alph=a, submat=sm))
        xf, yf = x.copy(), y.copy()
        xf[list(FOREIGN_X)] = -1
        yf[list(FOREIGN_Y)] = -1
        out.append(case("alph%d_foreign_all" % a, xf, yf, "integer", alph=a, submat=sm))
        if a == 4:
            for p in FOREIGN_X:
                xf = x.copy()
                xf[p] = -1
                out.append(case("alph4_foreign_x%d" % p, xf, y, "integer", alph=a, submat=sm))
            for p in FOREIGN_Y:
                yf = y.copy()
                yf[p] = -1
                out.append(case("alph4_foreign_y%d" % p, x, yf, "integer", alph=a, submat=sm))
        if a in (4, 20):
            out.append(case("alph%d_foreign_whole_x" % a, np.full(130, -1), y, "integer", alph=a, submat=sm))
            out.append(case("alph%d_foreign_whole_y" % a, x, np.full(70, -1), "integer", alph=a, submat=sm))
    return tuple(out)


# ---- degenerate envelopes ----------------------------------------------------------------------------------------------------------
ENVELOPE_PAIRS = ((130, 90, "integer"), (70, 140, "amino"))
NO_CELL = ("no_cell_x", "no_cell_y", "empty")
ONE_CELL = ("corner_x", "corner_y")


def envelopes(lx, ly):
    """name -> diagonals d = i - j (legal: -ly .. lx; those with a cell: 1 - ly .. lx - 1)"""
    every = list(range(1 - ly, lx))
    return {
        "no_cell_x": [lx], "no_cell_y": [-ly], "empty": [],
        "corner_x": [lx - 1], "corner_y": [1 - ly],            # the cells (lx, 1) and (1, ly)
        "main": [0],
        "alternate": every[::2],                               # no two neighbouring diagonals: every ins and del is -inf
        "all_but_main": [d for d in every if d != 0],
        "two_bands": [-31, -30, -29, 29, 30, 31],
        "band5_rows_63_64": [3, 4, 5, 6, 7],                   # crosses the strip seam at columns 56 .. 61
    }


@functools.lru_cache(None)
def envelope_cases():
    """Both pairs under every envelope above, and each pair once with the full envelope (None): in a batch with the others it
    runs the kernel that tests membership, with a null bitmap"""
    out = []
    for n, (lx, ly, set_name) in enumerate(ENVELOPE_PAIRS):
        x, y = related_pair(np.random.default_rng(7800 + n), score_set(set_name)[0], lx, ly)
        for name, d in envelopes(lx, ly).items():
            out.append(case("env_%dx%d_%s" % (lx, ly, name), x, y, set_name, d))
        out.append(case("env_%dx%d_full" % (lx, ly), x, y, set_name))
    return tuple(out)


# ---- column tables at the LDS limit --------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def column_table_batches():
    """7000 columns is the last size whose per-column constants live in LDS, 7001 the first that moves them to global memory;
    `max_cols` is per batch, so the 70 x 30 pair beside the 7001-column one takes the global tables as well.  Each batch once
    with full envelopes (the kernel without the membership test) and once with a band of 9 diagonals."""
    out = []
    for cols, set_name in ((7000, "integer"), (7001, "amino")):
        a = score_set(set_name)[0]
        x, y = related_pair(np.random.default_rng(7900 + cols), a, 65, cols)
        xs, ys = related_pair(np.random.default_rng(7950 + cols), a, 70, 30)
        band = list(range(-3004, -2995))                       # rows 1 .. 65 at columns 2997 .. 3069
        full = [case("cols%d_full" % cols, x, y, set_name)]
        banded = [case("cols%d_band9" % cols, x, y, set_name, band)]
        if cols == 7001:
            full.append(case("cols7001_short_full", xs, ys, set_name))
            banded.append(case("cols7001_short_band9", xs, ys, set_name, list(range(-4, 5))))
        out += [tuple(full), tuple(banded)]
    return tuple(out)


# ---- batches large enough for the narrow launches -------------------------------------------------------------------------------------
LARGE_BATCHES = (128, 384)     # launch_quickalign: from 128 pairs at most 8 waves a pair, from 384 at most 4
LARGE_ROWS = (5, 70, 300, 641)   # 641 rows: 11 strips, several rounds on 8 and on 4 waves


@functools.lru_cache(None)
def large_batch(n_pairs):
    out = []
    for k in range(n_pairs):
        lx, ly = LARGE_ROWS[k % len(LARGE_ROWS)], 20 + k % 70
        x, y = related_pair(np.random.default_rng(8000 + k), 4, lx, ly)
        out.append(case("large_%03d_%dx%d" % (k, lx, ly), x, y, "integer"))      # (the 128 are the first third of the 384)
    return tuple(out)


# ---- every score set on the same pairs -------------------------------------------------------------------------------------------------
SCORE_SHAPES = ((65, 63), (129, 81), (63, 65), (81, 129))


@functools.lru_cache(None)
def score_set_cases(set_name):
    out = []
    a = score_set(set_name)[0]
    for n, (lx, ly) in enumerate(SCORE_SHAPES):
        x, y = related_pair(np.random.default_rng(8500 + n), a, lx, ly)
        out.append(case("scores_%s_%dx%d_full" % (set_name, lx, ly), x, y, set_name))
        out.append(case("scores_%s_%dx%d_band9" % (set_name, lx, ly), x, y, set_name, range(-4, 5)))
    return tuple(out)


# ---- the Python restatement on a case -------------------------------------------------------------------------------------------------
class _Alphabet:
    def __init__(self, alph):
        self.alphabet = TEXT[:alph]


class _Scores:
    def __init__(self, sm, sv):
        self.submat = [list(map(float, row)) for row in sm]
        for n, v in zip(SCORE_NAMES, sv):
            setattr(self, n, v)


def as_text(tok, alph):
    return "".join("*" if t < 0 else TEXT[t] for t in tok)


def python_matrix(c, fill=True):
    """oracle.quickalign_oracle.QuickAlignMatrix of the case (the second restatement of the reference's fill, with its traceback)"""
    name, x, y, a, sm, sv, d = c
    env = q.DiagonalEnvelope(as_text(x, a), as_text(y, a))
    if d is None:
        env.init_full()
    else:
        env.diagonals = sorted(d)
    return q.QuickAlignMatrix(env, _Alphabet(a), 1.0, scores=_Scores(sm, sv), fill=fill)


def python_cells(mx):
    out = np.full((mx.x_len + 1, mx.y_len + 1, 3), NEG_INF)
    for (i, j), v in mx.cells.items():
        out[i, j] = v
    return out


def align_path_over(c, cells, score, x_end, y_end):
    """the reference's traceback (alignPath) over a given matrix"""
    mx = python_matrix(c, fill=False)
    mx.cells = {(i, j): list(cells[i, j]) for i in range(1, mx.x_len + 1) for j in range(1, mx.y_len + 1)}
    mx.end = mx.result = float(score)
    mx.x_end, mx.y_end = int(x_end), int(y_end)
    return mx.align_path()
