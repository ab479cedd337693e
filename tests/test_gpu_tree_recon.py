"""From a guide alignment to the reconstruction without a tree given: the reference's `testhist` case 5 (reference
Makefile:309, `historian recon ... -guide data/PF16593.testspan.fa -model data/testamino.json -nj`) through `hxrecon` with
`buildtree nj`, and the mirror's `testnj` / `testupgma` mains with the distance matrix from the device."""
import os
import subprocess

import pytest

from tests import recon_helpers as R
from tests import test_oracle_testhist as TH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
BIN = os.path.join(ROOT, "historian_amd", "bin") + os.sep


def device_env():
    return {k: v for k, v in os.environ.items() if k != "HX_HOST_DISTANCES"}


@pytest.mark.parametrize("distances", ["device", "host"])
def test_hxrecon_estimates_the_tree_of_testhist_case_5(tmp_path, distances):
    # the tree file of case 4 is the fixture of `testnj` on the same guide, so the expected output is case 4's; here the job
    # holds no tree, and the nodes must come out numbered as the reference's Newick reader numbers them
    case = TH.CASES["PF16593.testspan.testnj.historian.fa band 40"]
    tree, seqs, guide = TH.load_case(case)
    seqs_fa = tmp_path / "seqs.fa"
    seqs_fa.write_text("".join(">%s\n%s\n" % s for s in seqs.values()))
    job = tmp_path / "job.txt"
    job.write_text("model %s\nseqs %s\nguide %s\nband 40\nsamples 100\nmaxstates 0\nseed 5489\nbuildtree nj\n"
                   % (G + case["model"], seqs_fa, G + case["guide"]))
    env = dict(device_env(), HX_HOST_DISTANCES="1") if distances == "host" else device_env()
    out = subprocess.run([BIN + "hxrecon", str(job)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    got = R.parse_hxrecon(out.stdout.decode())
    assert R.fasta_rows(tree, got["rows"]) == open(G + "PF16593.testspan.testnj.historian.fa").read()


@pytest.mark.parametrize("main, model, fasta, want", [
    ("testnj", "testnj.jukescantor.json", "testnj.fa", "testnj.out.nh"),
    ("testnj", "testamino.json", "PF16593.testspan.fa", "PF16593.testspan.testnj.nh"),
    ("testupgma", "testnj.jukescantor.json", "testnj.fa", "testupgma.out.nh"),
    ("testupgma", "testamino.json", "PF16593.testspan.fa", "PF16593.testspan.testupgma.nh")])
def test_the_mirrors_mains_with_device_distances(main, model, fasta, want):
    out = subprocess.run([BIN + main, G + model, G + fasta], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=device_env(), timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout.decode() == open(G + want).read()


def test_the_mirrors_device_distances_are_tree_refs():
    # RateModel::distanceMatrix's own plumbing (tokens, rate layout, the expected rate) on the 6 pairs of testnj.fa, none of
    # which tree_ref flags as a near tie: bit for bit from the mirror's expected rate
    from oracle import historian_oracle as ho
    from oracle.ref_mains import read_fasta
    from tests import tree_ref as T
    out = subprocess.run([BIN + "hxtest", "distances", G + "testnj.fa", G + "testnj.jukescantor.json"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=device_env(), timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = [l.split() for l in out.stdout.decode().splitlines()]
    rate = float.fromhex(lines[0][1])
    model = ho.RateModel.from_file(G + "testnj.jukescantor.json")
    rows = [s for _, s in read_fasta(G + "testnj.fa")]
    assert len(lines) == 7
    for f in lines[1:]:
        info = {}
        want = T.ml_distance(model, rows[int(f[1])], rows[int(f[2])], esr=rate, info=info)
        assert info["min_gap"] >= 1e-9 and f[3] == want.hex()
