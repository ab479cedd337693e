"""Indel counts carried through profiles on the device (hx_batch_event_counts: BackwardMatrix::getCounts with the carried
x/y.getTrans(..)->counts terms, reference src/forward.cpp:579-584, 1183-1214) against tests/indel_carry_ref.py, which path
enumeration pins (tests/test_oracle_indel_carry.py); per-transition posteriors; run-to-run identity."""
import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import helpers as H
from tests import indel_carry_ref as R

pytestmark = pytest.mark.gpu
M = "tests/golden/models/"
G = "tests/golden/reference_data/"
COUNT = ho.DPMatrix.CountIndelEvents | ho.DPMatrix.CollapseChains
TIMES = (.1, .2, .15, .3)


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def _times(tm):
    return [tm[k] for k in ("l_t", "r_t", "l_ins_wait", "l_del_wait", "r_ins_wait", "r_del_wait")]


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1., abs(b))


def _on_device(imgs, root, flags):
    b = capi.Batch([imgs], capi.HX_KEEP_BACKWARD | flags)
    b.forward()
    b.backward()
    got = b.event_counts(0, _times(root.tm), R.carried_table(root.x), R.carried_table(root.y))
    b.close()
    return got


def _compare(got, want, tol, what):
    counts, x_post, y_post = got
    counts_w, x_w, y_w = want
    for k in R.KEYS:
        assert _close(counts[k], counts_w[k], tol), (what, k, counts[k], counts_w[k])
    assert np.max(np.abs(x_post - np.array(x_w))) <= tol, what
    assert np.max(np.abs(y_post - np.array(y_w))) <= tol, what


@pytest.mark.parametrize("flags", [0, capi.HX_LSE_FAST])
def test_without_tables_it_is_the_plain_indel_count(flags):
    cases = [H.leaf_case(701, 40, 36), H.leaf_case(702, 90, 100, band=6), H.leaf_case(703, 150, 140, alphabet="arndcqeghilkmfpstwyv", jc=False),
             H.leaf_case(704, 70, 3), H.leaf_case(705, 200, 210, band=10)]
    b = capi.Batch([H.job_images(f) for f in cases], capi.HX_KEEP_BACKWARD | flags)
    b.forward()
    b.backward()
    tm = [.2, .3, .09, .08, .14, .13]
    for k in range(len(cases)):
        plain = b.indel_counts(k, tm)
        got, x_post, y_post = b.event_counts(k, tm)
        for key in R.KEYS:
            assert _close(got[key], plain[key], 1e-12), (k, key, got[key], plain[key])
        # a leaf is one chain: the path takes each of its transitions but the one into END with probability 1 (to the accuracy
        # of the fills' table log-sum-exp: Forward x Backward of a cell is lpEnd to ~1e-5 per residue)
        assert np.allclose(x_post[:-1], 1., atol=5e-3) and np.allclose(y_post[:-1], 1., atol=5e-3)
        assert x_post[-1] == 0. and y_post[-1] == 0.
    with pytest.raises(capi.HxError):
        b.event_counts(len(cases), tm)
    b.close()


ENUMERATED = [("jc.json", ["acg", "ag", "ct"]), ("jc.json", ["acg", "ag", "ct", "g"]), ("jc.json", ["acg", "t", "tca", "gg"]),
              ("wag.json", ["arn", "an", "dr", "r"])]


@pytest.mark.parametrize("model_file,seqs", ENUMERATED)
def test_enumerated_cases(model_file, seqs):
    # the exact policy fills the oracle's cells bit for bit: only exp() and the order of the sums differ
    model = ho.RateModel.from_file(M + model_file)
    for strategy in (ho.DPMatrix.CountIndelEvents, COUNT):
        root = R.root_pair(model, seqs, TIMES, strategy)
        imgs = H.job_images(root)
        root.fill()
        _compare(_on_device(imgs, root, 0), R.get_indel_counts(ho.BackwardMatrix(root), root.tm), 1e-12, seqs)


def _family(k):
    """(name, model, sequences, times): the reference's testcount tree ((seq2, seq3), seq1), PF16593 and gp120 subsets"""
    if k == 0:
        tc = dict(R.read_fasta(G + "testcount.fa"))
        return "testcount", ho.RateModel.from_file(G + "testcount.jukescantor.json"), [tc["seq2"], tc["seq3"], tc["seq1"]], (1., 1., 1., .001)
    if k == 1:
        return "PF16593", ho.RateModel.from_file(M + "wag.json"), [s[:24] for _, s in R.read_fasta(G + "PF16593.fa")[:4]], TIMES
    return "gp120", ho.RateModel.from_file(M + "wag.json"), [s[:30] for _, s in R.read_fasta(G + "gp120.fa")[:4]], TIMES


@pytest.mark.parametrize("family", [0, 1, 2])
@pytest.mark.parametrize("kind", ["sampled", "posterior"])
@pytest.mark.parametrize("band", [None, 4])
def test_internal_node_pairs(family, kind, band):
    name, model, seqs, times = _family(family)
    root = R.root_pair(model, seqs, times, COUNT, kind=kind, seed=3 + family, band=band)
    imgs = H.job_images(root)
    root.fill()
    want = R.get_indel_counts(ho.BackwardMatrix(root), root.tm)
    assert any(sum(c) > 0 for c in R.carried_table(root.x))
    # in-slots beyond the inline ones of the state records (the CSR path and its slot -> transition map): testcount's x profile
    wide = [st.in_[k] for st in root.x.state[:-1] for k in range(3, len(st.in_))]
    for flags, tol in ((0, 1e-9), (capi.HX_LSE_FAST, 1e-6), (capi.HX_LSE_TRUNC, 1e-6)):
        got = _on_device(imgs, root, flags)
        _compare(got, want, tol, (name, kind, band, flags))
        if family == 0:
            assert wide and max(got[1][t] for t in wide) > 0, (kind, band)     # (x_post of in-slots 3, 4, ...)


def test_two_runs_are_bit_identical():
    name, model, seqs, times = _family(2)
    root = R.root_pair(model, seqs, times, COUNT, kind="posterior", seed=5)
    imgs = H.job_images(root)
    runs = []
    for _ in range(2):
        b = capi.Batch([imgs, H.job_images(H.leaf_case(706, 300, 280))], capi.HX_KEEP_BACKWARD | capi.HX_LSE_FAST)
        b.forward()
        b.backward()
        for _ in range(2):
            c, xp, yp = b.event_counts(0, _times(root.tm), R.carried_table(root.x), R.carried_table(root.y))
            runs.append(np.concatenate([[c[k] for k in R.KEYS], xp, yp]))
        b.close()
    for r in runs[1:]:
        H.assert_same_bits(r, runs[0], "event counts of two runs")
