"""The C++ host mirror's tree estimation (historian_amd/csrc/host/hx_host_tree.cpp) on its host path, HX_HOST_DISTANCES=1:
`bin/testnj` and `bin/testupgma` print the reference's four Newick fixtures byte for byte (reference Makefile:270-276), and
RateModel::mlDistance equals tests/tree_ref.py bit for bit.  No GPU is touched."""
import os
import subprocess

import pytest

from oracle import historian_oracle as ho
from tests import tree_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
BIN = os.path.join(ROOT, "historian_amd", "bin") + os.sep
ENV = dict(os.environ, HX_HOST_DISTANCES="1")


def run(*args):
    out = subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    return out.stdout.decode()


@pytest.mark.parametrize("main, model, fasta, want", [
    ("testnj", "testnj.jukescantor.json", "testnj.fa", "testnj.out.nh"),
    ("testnj", "testamino.json", "PF16593.testspan.fa", "PF16593.testspan.testnj.nh"),
    ("testupgma", "testnj.jukescantor.json", "testnj.fa", "testupgma.out.nh"),
    ("testupgma", "testamino.json", "PF16593.testspan.fa", "PF16593.testspan.testupgma.nh")])
def test_the_mirrors_mains_print_the_references_trees(main, model, fasta, want):
    assert run(BIN + main, G + model, G + fasta) == open(G + want).read()


def mirror_distances(fasta, model, *more):
    rate, dist = None, {}
    for line in run(BIN + "hxtest", "distances", fasta, model, *more).splitlines():
        f = line.split()
        if f[0] == "rate":
            rate = float.fromhex(f[1])
        elif f[0] == "d":
            dist[(int(f[1]), int(f[2]))] = float.fromhex(f[3])
    return rate, dist


@pytest.mark.parametrize("model_file, fasta, iterations, pairs", [
    ("testnj.jukescantor.json", "testnj.fa", 100, None),
    ("testnj.jukescantor.json", "testnj.fa", 0, None),
    ("testnj.jukescantor.json", "testnj.fa", 3, None),
    ("testamino.json", "PF16593.testspan.fa", 100, 60),        # rows 0 x 1..42 and 1 x 2..19: a second's worth of the 903 pairs
    ("testamino.json", "PF16593.testspan.fa", 0, None)])
def test_the_mirrors_distances_are_tree_refs_bit_for_bit(model_file, fasta, iterations, pairs):
    from oracle.ref_mains import read_fasta
    model = ho.RateModel.from_file(G + model_file)
    rows = [s for _, s in read_fasta(G + fasta)]
    rate, got = mirror_distances(G + fasta, G + model_file, str(iterations), *([str(pairs)] if pairs else []))
    # the equilibrium distribution is a least-squares solve, by Householder QR in the mirror and by LAPACK here: the two
    # expected rates agree to rounding, and the search is compared from the mirror's
    assert abs(rate - T.expected_sub_rate(model)) <= 1e-13 * rate
    assert len(got) == (pairs or len(rows) * (len(rows) - 1) // 2)
    for (i, j), d in got.items():
        assert d.hex() == T.ml_distance(model, rows[i], rows[j], iterations, esr=rate).hex(), (i, j)


def test_an_alphabet_of_more_than_32_symbols_takes_the_host_path(tmp_path):
    # 34 symbols, uniform rates: the device refuses it (HX_ERR_RANGE), RateModel::distanceMatrix must not ask it -
    # no HX_HOST_DISTANCES here, and no GPU either
    alphabet = "abcdefghijklmnopqrstuvwxyz01234567"
    js = dict(alphabet=alphabet, insrate=.01, delrate=.01, insextprob=.5, delextprob=.5,
              subrate={a: {b: 1. / 33 for b in alphabet if b != a} for a in alphabet})
    import json
    (tmp_path / "m.json").write_text(json.dumps(js))
    rows = ["abcdefghij0123", "abcdefghji0124", "abcdxfghij0723"]
    (tmp_path / "a.fa").write_text("".join(">s%d\n%s\n" % (k, r) for k, r in enumerate(rows)))
    env = {k: v for k, v in os.environ.items() if k != "HX_HOST_DISTANCES"}
    out = subprocess.run([BIN + "hxtest", "distances", str(tmp_path / "a.fa"), str(tmp_path / "m.json")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=env, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = [l.split() for l in out.stdout.decode().splitlines()]
    rate = float.fromhex(lines[0][1])
    model = ho.RateModel(js)
    for f in lines[1:]:
        assert f[3] == T.ml_distance(model, rows[int(f[1])], rows[int(f[2])], esr=rate).hex()
