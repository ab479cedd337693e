"""The C++ mirror Sampler::SiblingMatrix (hx_host_sibling.cpp: scores and profiles prepared on the host from a real model and
real sequences, the fill on the device, the walks on the copy read back) through `hxtest sibling`, against tests/sibling_ref.py:
lpEnd bit for bit, the printed sampled alignment's logPostProb against the restatement's log_post_prob of that same alignment,
rows spelling the sequences, parent profile rows normalised and equal to the restatement's, fillBatch of two envelopes equal
to two single fills.  The restatement is pinned by enumeration (tests/test_oracle_sibling.py), not by a reference fixture."""
import math
import os
import subprocess

import pytest

from oracle import historian_oracle as ho
from oracle.ref_mains import read_fasta
from tests import sibling_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "historian_amd", "bin") + os.sep
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
LG = os.path.join(ROOT, "tests", "golden", "models", "lg.json")
NEG = float("-inf")


def run(args):
    return subprocess.run([BIN + "hxtest", "sibling"] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          check=True, timeout=300).stdout.decode()


def restated(xs, ys, tl, tr, band):
    model = ho.RateModel.from_file(LG)

    def prob_model(t):
        t = max(1e-9, t)
        return ho.ProbModel(model, t, [ho.sub_prob_matrix_ss(m.tolist(), t) for m in model.sub_rate])

    def pwm(seq):
        # TreeAlignFuncs::leafPWM of the mirror: a symbol outside the alphabet is every residue
        rows = []
        for ch in seq:
            k = model.alphabet.find(ch.lower())
            rows.append([[0. if k < 0 or a == k else NEG for a in range(len(model.alphabet))] for _ in range(model.components())])
        return rows
    kw = {}
    if band is not None:
        m = min(len(xs), len(ys))       # the ungapped diagonal as guide: match count at a position's column
        kw = dict(l_env=[min(i, m) for i in range(len(xs) + 1)], r_env=[min(j, m) for j in range(len(ys) + 1)], max_dist=band)
    return sr.SiblingMatrix.from_profiles(model, pwm(xs), pwm(ys), prob_model(tl), prob_model(tr), **kw)


def check(fasta, xs, ys, tl, tr, band):
    out = run([fasta, LG, tl, tr] + ([] if band is None else [band])).splitlines()
    want = restated(xs, ys, tl, tr, band)
    assert out[0].split()[0] == "lpEnd" and float.fromhex(out[0].split()[1]) == want.lp_end
    rows = out[1:4]
    assert len(set(map(len, rows))) == 1
    assert rows[0].replace("-", "") == xs and rows[1].replace("-", "") == ys and set(rows[2]) <= set("*-")
    path = tuple([c != "-" for c in row] for row in rows)
    assert all(any(col) for col in zip(*path))
    got_lp = float.fromhex(out[4].split()[1])
    want_lp = want.log_post_prob(path)
    print("logPostProb of the printed alignment: mirror %.17g restatement %.17g" % (got_lp, want_lp))
    assert NEG < want_lp <= 0. and abs(got_lp - want_lp) <= 1e-12 * max(1., abs(want_lp))
    parent = want.parent_seq(path)
    shown = [line for line in out if line.startswith("parent ")]
    assert len(shown) == min(3, len(parent)) and shown
    for pos, line in enumerate(shown):
        vals = [float.fromhex(v) for v in line.split()[2:]]
        assert abs(math.log(sum(math.exp(v) for v in vals))) <= 1e-3        # normalised with the table operator
        assert vals == [v for row in parent[pos] for v in row]
    # fillBatch: envelopes (none, band or 10) in one device batch against two single fills
    last = out[-1].split()
    assert last[:2] == ["fillBatch", "lpEnd"] and last[4] == "single" and last[-1] == "0"
    assert last[2] == last[5] and last[3] == last[6]
    banded = want if band is not None else restated(xs, ys, tl, tr, 10)
    plain = want if band is None else restated(xs, ys, tl, tr, None)
    assert float.fromhex(last[2]) == plain.lp_end and float.fromhex(last[3]) == banded.lp_end


@pytest.mark.parametrize("band", [None, 3])
def test_sibling_matrix_of_the_mirror_on_the_pf16593_pair(band):
    (_, xs), (_, ys) = read_fasta(G + "PF16593.pair.fa")
    check(G + "PF16593.pair.fa", xs, ys, 0.7, 0.4, band)


def test_sibling_matrix_of_the_mirror_on_a_gp120_pair_of_several_strips(tmp_path):
    # two sequences of the reference's gp120 set, about 500 residues each: eight strips, dealt to eight wavefronts
    seqs = read_fasta(G + "gp120.fa")[:2]
    (_, xs), (_, ys) = [(n, s.replace("-", "")) for n, s in seqs]
    pair = tmp_path / "gp120.pair.fa"
    pair.write_text("".join(">%s\n%s\n" % (n, s.replace("-", "")) for n, s in seqs))
    check(str(pair), xs, ys, 0.3, 0.5, 20)
