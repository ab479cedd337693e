"""TEST INFRASTRUCTURE ONLY: ancestral sequence prediction restated on top of the sum-product oracle.

  max_post_state              SumProduct::maxPostState (reference src/sumprod.cpp:259-262)
  predict                     AlignColSumProduct::appendAncestralReconstructedColumn / appendAncestralPostProbColumn
                              (src/sumprod.cpp:401-426) driven as Reconstructor::predictAncestors drives them
                              (src/recon.cpp:1072-1085)
  compare_rows / compare_pp   what the device's prediction must agree with, and where a near tie of the oracle's own
                              posteriors leaves the choice to rounding

oracle/sumprod_oracle.SumProduct.log_node_post_prob is the yardstick; nothing here computes a posterior of its own."""
import math

from oracle import sumprod_oracle as so

WILD = "*"                      # Alignment::isWildcard: this character only (a leaf's 'x' is a wildcard to SumProduct, not here)
NEAR_TIE = 1e-6                 # a top-two gap of the oracle's log posteriors below this leaves the choice to rounding


def max_post_state(lpp):
    """index of the first maximum (std::max_element)"""
    best = 0
    for k, lp in enumerate(lpp):
        if lp > lpp[best]:
            best = k
    return best


def top_two_gap(lpp):
    s = sorted(lpp, reverse=True)
    return s[0] - s[1]


class Prediction:
    """rows: the predicted rows; pp: {row: {col: {char: prob}}}; lp: {(row, col): [A] log posteriors} of every '*' cell"""

    def __init__(self, rows, pp, lp):
        self.rows, self.pp, self.lp = rows, pp, lp

    def min_gap(self):
        return min(top_two_gap(v) for v in self.lp.values())

    def near_ties(self):
        return [k for k, v in self.lp.items() if top_two_gap(v) < NEAR_TIE]

    def threshold_margin(self, min_prob):
        """the smallest distance of a finite log posterior from log(min_prob)"""
        t = math.log(min_prob)
        return min(abs(x - t) for v in self.lp.values() for x in v if x > -math.inf)


def predict(model, tree, rows, min_prob=.01, max_prob=1., sp=None):
    """rows: [N] gapped strings in tree-node order -> Prediction"""
    sp = sp or so.SumProduct(model, tree)
    alph = model.alphabet
    lp_min = math.log(min_prob) if min_prob else -math.inf
    lp_max = math.log(max_prob)
    out = [[] for _ in rows]
    pp, lps = {}, {}
    for col, seq in enumerate(so.columns_of(tree, dict(enumerate(rows)))):
        sp.init_column(seq)
        sp.fill_up()
        sp.fill_down()
        for row, text in enumerate(rows):
            g = text[col]
            if g != WILD:
                out[row].append(g)
                continue
            lp = sp.log_node_post_prob(row)
            lps[(row, col)] = lp
            out[row].append(alph[max_post_state(lp)])
            for tok, x in enumerate(lp):
                if lp_min <= x <= lp_max:
                    pp.setdefault(row, {}).setdefault(col, {})[alph[tok]] = math.exp(x)
    return Prediction(["".join(r) for r in out], pp, lps)


def compare_rows(want, got_rows, input_rows, alphabet, tie_rtol=1e-9):
    """The predicted rows against the oracle's.  At a cell whose oracle top-two gap is below NEAR_TIE the pick must be a
    residue whose oracle posterior is within tie_rtol (relative) of the best; every other cell must be equal.
    -> the number of cells that took the exception."""
    assert len(got_rows) == len(want.rows)
    excused = 0
    for row, (w, g, src) in enumerate(zip(want.rows, got_rows, input_rows)):
        assert len(w) == len(g), "row %d" % row
        for col, (cw, cg) in enumerate(zip(w, g)):
            if cw == cg:
                continue
            assert src[col] == WILD, "row %d column %d: %r changed to %r" % (row, col, src[col], cg)
            lp = want.lp[(row, col)]
            assert top_two_gap(lp) < NEAR_TIE, "row %d column %d: %r, oracle %r (gap %g)" % (row, col, cg, cw, top_two_gap(lp))
            k = alphabet.find(cg)
            assert k >= 0 and abs(math.exp(lp[k]) - math.exp(max(lp))) <= tie_rtol * math.exp(max(lp)), (row, col, cg, cw)
            excused += 1
    return excused


def compare_pp(want, got_pp, rtol=1e-8):
    """same keys, values within rtol relative"""
    assert sorted(got_pp) == sorted(want.pp)
    for row in want.pp:
        assert sorted(got_pp[row]) == sorted(want.pp[row]), "row %d" % row
        for col in want.pp[row]:
            w, g = want.pp[row][col], got_pp[row][col]
            assert sorted(g) == sorted(w), "row %d column %d: %r, oracle %r" % (row, col, g, w)
            for ch in w:
                assert abs(g[ch] - w[ch]) <= rtol * w[ch], (row, col, ch, g[ch], w[ch])
