"""tests/ancestors_ref.py (ancestral sequence prediction on top of the sum-product oracle) against what the reference
holds for it: the root posteriors of t/testsumprod's fixture, which pins the oracle's log_node_post_prob byte for byte,
and the contract of appendAncestralReconstructedColumn - only '*' changes."""
import math
import re

from oracle import sumprod_oracle as so
from tests import ancestors_ref as AR
from tests.test_oracle_sumprod import G, load


def test_root_posteriors_are_the_testsumprod_fixtures():
    model, tree, gapped = load("testnj.jukescantor.json", "testaligncount.fa", "testaligncount.nh")
    rows = [gapped[n] for n in range(tree.nodes())]
    root = tree.nodes() - 1
    assert all(ch == "*" for ch in rows[root])
    pred = AR.predict(model, tree, rows, min_prob=0.)
    with open(G + "testsumprod.out") as f:
        text = f.read()
    want = [dict(re.findall(r"^P\( %s = (\S) \) = (\S+)$" % tree.name[root], block, re.M)) for block in text.split("Column #")[1:]]
    assert len(want) == len(rows[root]) and all(len(w) == len(model.alphabet) for w in want)
    for col, w in enumerate(want):
        assert {ch: so._g(p) for ch, p in pred.pp[root][col].items()} == w
        best = max(model.alphabet, key=lambda ch: pred.pp[root][col][ch])
        assert pred.rows[root][col] == best


def test_only_wildcards_change():
    for files in (("testcount.jukescantor.json", "testcount.historian.fa", "testcount.nh"),
                  ("testrates.mix2.json", "testcount.mix2.fa", "testcount.mix2.nh")):
        model, tree, gapped = load(*files)
        rows = [gapped[n] for n in range(tree.nodes())]
        pred = AR.predict(model, tree, rows)
        n_wild = sum(r.count("*") for r in rows)
        assert n_wild > 0 and len(pred.lp) == n_wild
        for src, out in zip(rows, pred.rows):
            assert len(src) == len(out)
            for a, b in zip(src, out):
                assert (a == b) if a != "*" else (b in model.alphabet)
        # the PP map holds exactly the '*' cells' residues at or above the threshold, and a cell's posteriors add up to 1
        for (row, col), lp in pred.lp.items():
            assert set(pred.pp[row][col]) == {model.alphabet[k] for k, x in enumerate(lp) if x >= math.log(.01)}
            assert abs(sum(math.exp(x) for x in lp) - 1.) < 1e-3        # (table log_sum_exp: ~1e-5 per addition)
        assert set(pred.pp) == {row for row, _ in pred.lp}


def test_first_maximum_wins():
    assert AR.max_post_state([-1., -.5, -.5, -2.]) == 1
    assert AR.max_post_state([-math.inf] * 4) == 0
    assert AR.top_two_gap([-1., -.5, -.5]) == 0.
