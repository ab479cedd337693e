"""The tree-height chain of tests/test_gpu_treesampler.py (5 leaves x 70 columns, the 4 x 20 mixture, 200 steps, one seed)
twice on the device: DeviceEvaluator in lengths mode - the rates given once, exp(R t) of the changed branches computed by
k_branch_expm - and DeviceEvaluator(sub_prob=the oracle's sub_prob_matrix_ss), which builds the same matrices on the host and
uploads them.  The matrices have the same bits, so the chains are the same chain: moves, nodes, decisions, variates, and
logAcceptProb EQUAL as floats; the resident state at the end has the bytes of a history created on the final tree."""
import random

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from historian_amd import treesampler as ts
from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import tree_ref
from tests.test_gpu_treesampler import SEED, STEPS, chain_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def _sampler(mode, length=None):
    js, parent, first_length, rows = chain_input()
    model, omodel = hostmodel.RateModel(js), ho.RateModel(js)
    length = first_length if length is None else length
    tokens = counts.tokenize_columns(model.alphabet, rows)
    if mode == "lengths":
        ev = ts.DeviceEvaluator(model, parent, length, tokens)
    else:
        # tree_ref._sub_prob: sub_prob_matrix_ss's operations in numpy, the same bits (checked below at one length) in a
        # hundredth of the time - the chain asks for some 4 000 matrices
        ev = ts.DeviceEvaluator(model, parent, length, tokens, sub_prob=lambda t: [tree_ref._sub_prob(sr, t) for sr in omodel.sub_rate])
        for sr in omodel.sub_rate:
            assert np.asarray(ho.sub_prob_matrix_ss(sr.tolist(), length[0])).tobytes() == tree_ref._sub_prob(sr, length[0]).tobytes()
    assert ev.mode == mode
    return ts.TreeSampler(model, parent, length, rows, ev), ev


def test_the_lengths_chain_is_the_matrices_chain():
    lengths, lev = _sampler("lengths")
    mats, mev = _sampler("matrices")
    assert lengths.parts == mats.parts
    lengths.run(STEPS, random.Random(SEED))
    mats.run(STEPS, random.Random(SEED))
    assert len(lengths.steps) == STEPS
    for k, (a, b) in enumerate(zip(lengths.steps, mats.steps)):
        assert a == b, (k, a, b)                      # (move type, node, logAcceptProb, accepted, u): floats compared with ==
    assert lengths.length == mats.length and lengths.moves_accepted == mats.moves_accepted and lengths.log_likelihood == mats.log_likelihood
    assert min(lengths.moves_accepted[3:]) > 5 and min(p - a for p, a in zip(lengths.moves_proposed[3:], lengths.moves_accepted[3:])) > 5
    # the resident state of both against a history created on the final tree
    fresh, fev = _sampler("lengths", lengths.length)
    want = fev.history.log_like(0)
    for ev in (lev, mev):
        got = ev.history.log_like(0)
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()
    for r in range(len(lengths.length) - 1):
        assert lev.history.branch_matrix(r).tobytes() == fev.history.branch_matrix(r).tobytes() == mev.history.branch_matrix(r).tobytes(), r
    assert lengths.parts[3] == want[0] and lengths.log_likelihood == fresh.log_likelihood
    for ev in (lev, mev, fev):
        ev.close()


def test_an_explicit_mode_overrides_the_default():
    js, parent, length, rows = chain_input()
    model = hostmodel.RateModel(js)
    tokens = counts.tokenize_columns(model.alphabet, rows)
    ev = ts.DeviceEvaluator(model, parent, length, tokens, mode="matrices")             # model.sub_prob: scipy's expm
    assert ev.mode == "matrices"
    lv = ts.DeviceEvaluator(model, parent, length, tokens, sub_prob=model.sub_prob, mode="lengths")
    assert lv.mode == "lengths"
    assert abs(ev.lp_sub() - lv.lp_sub()) <= 1e-9 * abs(lv.lp_sub()) and lv.lp_sub() == _sampler("lengths")[1].lp_sub()
    with pytest.raises(ValueError):
        ts.DeviceEvaluator(model, parent, length, tokens, mode="other")
    ev.close()
    lv.close()
