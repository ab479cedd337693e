"""`hxtest condpwm`: the C++ mirror's TreeAlignFuncs::getConditionalPWMs (csrc/host/hx_host_sampler.cpp over
hx_history_excluded_profiles) and what BranchAlignMove does next with its result (src/sampler.cpp:590-594): an unbanded
Sampler::BranchMatrix, a sample, its logPostProb.  On the 5-leaf x 70-column fixture of tests/test_gpu_treesampler.py, for
a leaf branch and an internal branch.

The profiles: the bounds of tests/test_gpu_condpwm.py against the restatement (tests/condpwm_ref.py).  lpEnd: 1e-9
relative against oracle/branch_oracle.py fed the restated profiles through preMultiply and calcInsProbs - the project's
bound for sums of such terms."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import branch_oracle as bo
from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from tests import condpwm_ref as CR
from tests.test_gpu_condpwm import compare
from tests.test_gpu_treemoves_mirror import _newick, _postorder
from tests.test_gpu_treesampler import PROT4, chain_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HXTEST = os.path.join(ROOT, "historian_amd", "bin", "hxtest")


@functools.lru_cache(maxsize=None)
def _files(tmp):
    js, parent, length, rows = chain_input()
    with open(os.path.join(tmp, "rows.fa"), "w") as f:
        for r, row in enumerate(rows):
            f.write(">n%d\n%s\n" % (r, row))
    with open(os.path.join(tmp, "tree.nh"), "w") as f:
        f.write(_newick(parent, length) + "\n")
    return os.path.join(tmp, "rows.fa"), os.path.join(tmp, "tree.nh")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _files(str(tmp_path_factory.mktemp("condpwm")))


def _branches():
    """a leaf branch and an internal branch, as our node numbers"""
    _, parent, _, _ = chain_input()
    internal = set(p for p in parent if p >= 0)
    return 0, next(r for r in range(len(parent) - 1) if r in internal)


@pytest.mark.parametrize("which", ["leaf", "internal"])
@pytest.mark.parametrize("normalize", [0, 1])
def test_profiles_branch_matrix_and_sample(files, which, normalize):
    js, parent, length, rows = chain_input()
    node = _branches()[which == "internal"]
    assert (node in set(parent)) == (which == "internal")
    p = parent[node]
    mirror = _postorder(parent).index(node)                  # the Newick reader numbers the nodes in post-order
    out = subprocess.run([HXTEST, "condpwm", files[0], files[1], PROT4, str(mirror), str(normalize)], capture_output=True, text=True, check=True).stdout
    lines = [l.split() for l in out.splitlines()]
    model = ho.RateModel(js)
    tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
    sp = so.SumProduct(model, tree)
    (want_p, want_n), (norm_p, norm_n), _, _ = CR.conditional_pwms_and_norms(sp, rows, [(p, node), (node, p)])
    assert [int(v) for v in lines[0][1:]] == [want_p.shape[0], want_n.shape[0]] and lines[0][0] == "lengths"

    def rows_of(tag, want):
        got = [[float.fromhex(v) for v in l[2:]] for l in lines if l[0] == tag]
        assert [int(l[1]) for l in lines if l[0] == tag] == list(range(want.shape[0]))
        return np.asarray(got).reshape(want.shape)
    got_p, got_n = rows_of("parent", want_p), rows_of("node", want_n)
    compare(got_p, want_p, norm_p, bool(normalize), "mirror, parent of %s branch" % which)
    compare(got_n, want_n, norm_n, bool(normalize), "mirror, node of %s branch" % which)
    # what BranchAlignMove builds from them, on the restated profiles
    if normalize:
        want_p, want_n = want_p - norm_p[:, None, None], want_n - norm_n[:, None, None]
    pm = ho.ProbModel(model, max(1e-9, length[node]))
    with np.errstate(divide="ignore"):
        log_sub = [np.log(np.asarray(m, dtype=float)).tolist() for m in pm.sub_mat]
        log_ins = [np.log(np.asarray(q, dtype=float)).tolist() for q in model.ins_prob]
    log_w = [math.log(w) for w in model.cpt_weight]
    y = want_n.tolist()
    matrix = bo.BranchMatrix(want_p.tolist(), bo.pre_multiply(y, log_sub), bo.calc_ins_probs(y, log_ins, log_w),
                             bo.trans_scores(pm.ins, pm.dele, pm.ins_ext, pm.del_ext), viterbi=False)
    lp_end = float.fromhex(next(l for l in lines if l[0] == "lpEnd")[1])
    print("%s branch, normalize %d: lpEnd mirror %.17g oracle %.17g, relative %.3g" % (which, normalize, lp_end, matrix.lp_end,
                                                                                      abs(lp_end - matrix.lp_end) / abs(matrix.lp_end)))
    assert math.isfinite(matrix.lp_end) and abs(lp_end - matrix.lp_end) <= 1e-9 * abs(matrix.lp_end)
    # the sampled path: a row per sequence, as many steps in each as it has positions, a finite logPostProb
    at = next(k for k, l in enumerate(lines) if l[0] == "lpEnd")
    path = [out.splitlines()[at + 1], out.splitlines()[at + 2]]
    assert len(path[0]) == len(path[1]) and set(path[0] + path[1]) <= set("*-")
    assert path[0].count("*") == want_p.shape[0] and path[1].count("*") == want_n.shape[0]
    lpp = float.fromhex(next(l for l in lines if l[0] == "logPostProb")[1])
    assert math.isfinite(lpp) and lpp <= 1e-9


def test_a_prune_and_regraft_map_is_not_built(files):
    """The mirror's Abort is std::terminate: the child ends with SIGABRT.  It holds no device when it does:
    getConditionalPWMs checks the map (neighboursOnly) before residentHistory creates a history, and hxtest initialises
    nothing before that call.  Whoever reorders that turns this into an abort of a process that holds the GPU - keep the
    check first."""
    node = _postorder(chain_input()[1]).index(_branches()[1])
    out = subprocess.run([HXTEST, "condpwm", files[0], files[1], PROT4, "prune:%d" % node, "1"], capture_output=True, text=True)
    assert out.returncode != 0 and "Prune" in out.stderr and "moves are not built" in out.stderr, (out.returncode, out.stderr)
    assert "lpEnd" not in out.stdout
