"""`historian recon -ancseq -ancprob` end to end: bin/hxrecon reconstructs a family on the device and then predicts its
ancestral sequences (Reconstructor::predictAncestors: one hx_sumprod_ancestors call over the reconstruction's columns).

The reconstruction is what the device made of the family, so the expectation is restated from the printed `row` lines with
tests/ancestors_ref.py over the oracle's ProbModel matrices.  `anc` rows must be the oracle's except where the oracle's own
top-two gap is below 1e-6 (there: a residue whose oracle posterior is within 1e-9 relative of the best); at most 2 % of the
wildcard cells may need that.  `pp` values (hex field) within 1e-8 relative, same keys.  Without the two job keys the
output is byte for byte what is left when the `anc` and `pp` lines are taken out."""
import math
import os
import subprocess

import pytest

from historian_amd import capi, counts
from oracle import c_oracle
from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from tests import ancestors_ref as AR
from tests import recon_helpers as R
from tests import test_oracle_testhist as TH
from tests.test_gpu_sumprod import _fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
HXRECON = os.path.join(ROOT, "historian_amd", "bin", "hxrecon")


def _run(job):
    out = subprocess.run([HXRECON, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ), timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    return out.stdout.decode()


@pytest.mark.parametrize("name", ["testcount.historian.fa", "PF16593.testspan.testnj.historian.fa band 40"])
def test_hxrecon_predicts_the_ancestors_of_its_reconstruction(tmp_path, name):
    case = TH.CASES[name]
    tree, seqs, guide = TH.load_case(case)
    kw = case["kw"]
    opts = dict(band=kw["max_distance_from_guide"], maxstates=0, seed=5489)
    if "min_post_prob" in kw:
        opts["posterior"] = kw["min_post_prob"]
    else:
        opts["samples"] = kw["profile_samples"]
    files = (G + case["model"], tree, seqs, guide, str(tmp_path / "seqs.fa"), str(tmp_path / "guide.fa"))
    plain, keyed = str(tmp_path / "plain.txt"), str(tmp_path / "keyed.txt")
    R.write_job(plain, *files, **opts)
    R.write_job(keyed, *files, ancseq="", ancprob=".01", **opts)
    text = _run(keyed)
    lines = text.splitlines(keepends=True)
    assert "".join(l for l in lines if not l.startswith(("anc ", "pp "))) == _run(plain)
    rows_by_node = R.parse_hxrecon("".join(l for l in lines if l.startswith("row ")))["rows"]
    n = tree.nodes()
    assert sorted(rows_by_node) == list(range(n))
    rows = [rows_by_node[k] for k in range(n)]
    anc, got_pp = {}, {}
    for l in lines:
        f = l.split()
        if f[0] == "anc":
            assert f[2] == tree.name[int(f[1])]
            anc[int(f[1])] = f[3] if len(f) > 3 else ""
        elif f[0] == "pp":
            got_pp.setdefault(int(f[1]), {}).setdefault(int(f[2]) - 1, {})[f[3]] = float.fromhex(f[4])
            assert f[5] == "%.6f" % float.fromhex(f[4])
    assert sorted(anc) == list(range(n))
    omodel = ho.RateModel.from_file(G + case["model"])
    otree = so.Tree(tree.parent, tree.branch_length, tree.name)
    want = AR.predict(omodel, otree, rows, min_prob=.01)
    cells = len(want.lp)
    assert cells == sum(r.count("*") for r in rows) > 0
    excused = AR.compare_rows(want, [anc[k] for k in range(n)], rows, omodel.alphabet, tie_rtol=1e-9)
    print("%d wildcard cells, %d of them near ties of the oracle, %d took the exception; nearest posterior to log .01: %.3g"
          % (cells, len(want.near_ties()), excused, want.threshold_margin(.01)))
    assert excused <= .02 * cells
    AR.compare_pp(want, got_pp, rtol=1e-8)
    # `pp` lines come in row, column, character order
    keys = [(int(f[1]), int(f[2]), f[3]) for f in (l.split() for l in lines) if f[0] == "pp"]
    assert keys == sorted(keys)


def test_predict_ancestors_changes_wildcards_only():
    """The Python bookkeeping of counts.predict_ancestors only - '*' cells and nothing else replaced, leaf rows untouched,
    the PP map thresholded - against AncestorPredictor.run, the same device call.  No independent check of the numbers:
    those are compared with the oracle in tests/test_gpu_ancestors.py."""
    capi.init(0, c_oracle.table())
    try:
        _, model, tree, gapped = _fixture("testcount.jukescantor.json", "testcount.historian.fa", "testcount.nh")
        rows = [gapped[k] for k in range(tree.nodes())]
        out, pp = counts.predict_ancestors(model, tree.parent, tree.branch_length, rows, min_prob=.01)
        res = counts.AncestorPredictor(model, tree.parent, tree.branch_length).run(counts.tokenize_columns(model.alphabet, rows), want_post=True)
        plain, none = counts.predict_ancestors(model, tree.parent, tree.branch_length, rows)
    finally:
        capi.shutdown()
    assert none is None and plain == out
    want_keys = {}
    for r, (src, dst) in enumerate(zip(rows, out)):
        assert len(src) == len(dst)
        if "*" not in src:
            assert src == dst                                    # a leaf's row comes back untouched
        for col, (a, b) in enumerate(zip(src, dst)):
            if a != "*":
                assert a == b
                continue
            assert b == model.alphabet[res["best"][col, r]]
            ks = {model.alphabet[k] for k, lp in enumerate(res["node_post"][col, r]) if lp >= math.log(.01)}
            if ks:
                want_keys[(r, col)] = ks
    assert sum(r.count("*") for r in rows) == 12
    assert {(r, col): set(v) for r, by_col in pp.items() for col, v in by_col.items()} == want_keys
    for r, by_col in pp.items():
        for col, v in by_col.items():
            for ch, p in v.items():
                assert p == math.exp(res["node_post"][col, r][model.alphabet.index(ch)])
