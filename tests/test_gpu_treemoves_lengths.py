"""`hxtest treemoves` on the fixture of tests/test_gpu_treemoves_mirror.py, twice: as built (the mirror hands the history its
rate matrices once and branch lengths per move; exp(R t) on the device) and with HX_HISTORY_HOST_EXPM=1 (getSubProbMatrix on
the host, the matrices uploaded per move).  k_branch_expm has getSubProbMatrix's bits, so the two outputs - the four parts,
every step's logAcceptProb and proposed tree in hex floats, the final tree, the move counts - are identical text."""
import os
import subprocess

import pytest

from tests.test_gpu_treemoves_mirror import ROOT, STEPS, _newick
from tests.test_gpu_treesampler import PROT4, chain_input

pytestmark = pytest.mark.gpu


def _run(tmp_path, host_expm):
    env = dict(os.environ)
    env.pop("HX_HISTORY_HOST_EXPM", None)
    if host_expm:
        env["HX_HISTORY_HOST_EXPM"] = "1"
    return subprocess.run([os.path.join(ROOT, "historian_amd", "bin", "hxtest"), "treemoves", str(tmp_path / "rows.fa"), str(tmp_path / "tree.nh"),
                           PROT4, str(STEPS), "11"], capture_output=True, text=True, check=True, env=env).stdout


def test_the_mirrors_chain_is_the_same_text_with_the_exponentials_on_either_side(tmp_path):
    _, parent, length, rows = chain_input()
    with open(tmp_path / "rows.fa", "w") as f:
        for r, row in enumerate(rows):
            f.write(">n%d\n%s\n" % (r, row))
    with open(tmp_path / "tree.nh", "w") as f:
        f.write(_newick(parent, length) + "\n")
    device, host = _run(tmp_path, False), _run(tmp_path, True)
    lines = device.splitlines()
    assert sum(l.startswith("step") for l in lines) == STEPS and any(l.startswith("final") for l in lines)
    assert device == host
