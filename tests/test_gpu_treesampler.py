"""A tree-height chain on the device against the same chain on the CPU: historian_amd/treesampler.py with the resident
history (capi.History) and with the oracle's evaluator (tests/history_ref.py), from the same seeded generator.

5 leaves x 70 columns, the 4 x 20 protein mixture, 200 steps.  Both evaluators take the oracle's exp(R t).  The chains
must make the same moves and the same decisions; logAcceptProb within 1e-9 absolute.  The seed is chosen so that no
acceptance of the CPU chain is decided within 1e-6 of its threshold (asserted): a decision cannot differ by rounding."""
import functools
import json
import math
import random

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from historian_amd import treesampler as ts
from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import history_ref as HR
from tests.test_gpu_ancestors import PROT4, _recon_columns

pytestmark = pytest.mark.gpu
SEED, STEPS = 2, 200


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


@functools.lru_cache(maxsize=None)
def chain_input():
    with open(PROT4) as f:
        js = json.load(f)
    rng = np.random.default_rng(41)
    parent, length = HR.ultrametric_tree(rng, 5)
    rows = _recon_columns(rng, parent, js["alphabet"], 70)
    return js, parent, length, rows


@functools.lru_cache(maxsize=None)
def cpu_chain():
    """the CPU chain, run once and left unchanged"""
    js, parent, length, rows = chain_input()
    sampler = ts.TreeSampler(hostmodel.RateModel(js), parent, length, rows, HR.OracleEvaluator(ho.RateModel(js), parent, length, rows))
    first = sampler.parts
    sampler.run(STEPS, random.Random(SEED))
    return sampler, first


def _device_sampler(length=None):
    js, parent, first_length, rows = chain_input()
    model = hostmodel.RateModel(js)
    length = first_length if length is None else length
    ev = ts.DeviceEvaluator(model, parent, length, counts.tokenize_columns(model.alphabet, rows), sub_prob=HR.oracle_sub_prob(ho.RateModel(js)))
    return ts.TreeSampler(model, parent, length, rows, ev), ev


def test_the_device_chain_makes_the_cpu_chains_moves_and_the_books_are_kept():
    cpu, cpu_first = cpu_chain()
    # the oracle alone: every drawn acceptance is decided well away from its threshold
    margins = [abs(lap - math.log(u)) for _, _, lap, _, u in cpu.steps if u is not None and u > 0]
    print("CPU chain: %d of %d acceptances drawn, nearest to its threshold %.3g; %s" % (len(margins), STEPS, min(margins), cpu.move_stats().replace("\n", "; ")))
    assert len(margins) > 20 and min(margins) >= 1e-6
    assert min(cpu.moves_accepted[3:]) > 5 and min(p - a for p, a in zip(cpu.moves_proposed[3:], cpu.moves_accepted[3:])) > 5
    dev, ev = _device_sampler()
    for a, b in zip(dev.parts[:3], cpu_first[:3]):
        assert a == b                                  # tree, root, indels: the same host code on the same counts
    assert abs(dev.parts[3] - cpu_first[3]) <= 1e-9
    dev.run(STEPS, random.Random(SEED))
    worst = 0.
    for k, (d, c) in enumerate(zip(dev.steps, cpu.steps)):
        assert d[:2] == c[:2] and d[3] == c[3] and d[4] == c[4], (k, d, c)
        assert abs(d[2] - c[2]) <= 1e-9, (k, d, c)
        worst = max(worst, abs(d[2] - c[2]))
    print("device chain: largest difference of a logAcceptProb %.3g" % worst)
    assert dev.length == cpu.length and dev.moves_accepted == cpu.moves_accepted
    # bookkeeping: the resident history's current state has the bytes of a history created on the final tree
    fresh, fresh_ev = _device_sampler(dev.length)
    got, want = ev.history.log_like(0), fresh_ev.history.log_like(0)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()
    assert dev.parts[3] == got[0] and dev.log_likelihood == fresh.log_likelihood
    ev.close()
    fresh_ev.close()
