"""`hxtest condpwm ... device`: the C++ mirror's BranchMatrixBase built from a resident history
(hx_history_branch_batch_create: the profiles, preMultiply and calcInsProbs stay on the device, yEmit alone is read back)
against `hxtest condpwm ...` without the argument, which downloads the profiles and runs preMultiply and calcInsProbs on
the host.  The same fixture and branches as tests/test_gpu_condpwm_mirror.py; the output is equal byte for byte: the
profiles printed, lpEnd, the seeded sample and its logPostProb."""
import subprocess

import pytest

from tests.test_gpu_condpwm_mirror import HXTEST, _branches, _files
from tests.test_gpu_treemoves_mirror import _postorder
from tests.test_gpu_treesampler import PROT4, chain_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _files(str(tmp_path_factory.mktemp("handoff")))


@pytest.mark.parametrize("which", ["leaf", "internal"])
@pytest.mark.parametrize("normalize", [1, 0])
def test_the_device_built_matrix_prints_the_same_lines(files, which, normalize):
    parent = chain_input()[1]
    node = _branches()[which == "internal"]
    mirror = _postorder(parent).index(node)                  # the Newick reader numbers the nodes in post-order
    args = [HXTEST, "condpwm", files[0], files[1], PROT4, str(mirror), str(normalize)]
    host = subprocess.run(args, capture_output=True, check=True).stdout
    device = subprocess.run(args + ["device"], capture_output=True, check=True).stdout
    assert b"lpEnd" in host and b"logPostProb" in host and host.count(b"\n") > 10
    assert device == host
