"""The C++ mirror's walks through device-resident matrices (hx_host_branch.cpp, hx_host_sibling.cpp: Refiner::BranchMatrix::best,
Sampler::BranchMatrix::sample / logPostProb, Sampler::SiblingMatrix::sample / sampleBatch / logPostProb) through `hxtest walks`,
against the restatements (tests/sibling_ref.py, tests/walks_ref.py, oracle/branch_oracle.py): the printed alignments are the
restatements' walks from the same std::mt19937 seeds, the generator stands where the restatement's stands, logPostProb is the
restatement's; the output equals that of the host walks (HX_HOST_WALKS=1) line for line, and no dense matrix is read."""
import os
import subprocess

import pytest

from oracle import branch_oracle as bo
from oracle import historian_oracle as ho
from oracle.ref_mains import read_fasta
from tests import walks_ref as wr
from tests.test_gpu_sibling_mirror import BIN, G, LG, NEG, restated

pytestmark = pytest.mark.gpu

MARGIN = 1e-12          # tests/test_oracle_walks.py: below this a walk could hang on the last bits of exp()


def run(args, host_walks):
    env = dict(os.environ)
    env.pop("HX_HOST_WALKS", None)
    if host_walks:
        env["HX_HOST_WALKS"] = "1"
    return subprocess.run([BIN + "hxtest", "walks"] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          check=True, timeout=300, env=env).stdout.decode().splitlines()


def envelope(xs, ys, band):
    if band is None:
        return None, None, -1
    m = min(len(xs), len(ys))           # the ungapped diagonal as guide: match count at a position's column
    return [min(i, m) for i in range(len(xs) + 1)], [min(j, m) for j in range(len(ys) + 1)], band


def restated_branch(xs, ys, t, band, viterbi):
    model = ho.RateModel.from_file(LG)
    t = max(1e-9, t)
    pm = ho.ProbModel(model, t, [ho.sub_prob_matrix_ss(m.tolist(), t) for m in model.sub_rate])
    lpm = ho.LogProbModel(pm)

    def pwm(seq):
        rows = []
        for ch in seq:
            k = model.alphabet.find(ch.lower())
            rows.append([[0. if k < 0 or a == k else NEG for a in range(len(model.alphabet))] for _ in range(model.components())])
        return rows
    log_sub = [[[ho.safe_log(v) for v in row] for row in m] for m in pm.sub_mat]
    y = pwm(ys)
    xe, ye, md = envelope(xs, ys, band)
    return bo.BranchMatrix(pwm(xs), bo.pre_multiply(y, log_sub), bo.calc_ins_probs(y, lpm.log_ins_prob, lpm.log_cpt_weight),
                           bo.trans_scores(pm.ins, pm.dele, pm.ins_ext, pm.del_ext), xe, ye, md, viterbi=viterbi)


def gapped(seqs, rows):
    out = []
    for r, row in enumerate(rows):
        it = iter(seqs[r]) if r < 2 else None
        out.append("".join(("-" if not b else (next(it) if it else "*")) for b in row))
    return out


def close(got, want):
    return NEG < want <= 0. and abs(got - want) <= 1e-12 * max(1., abs(want))      # as tests/test_gpu_sibling_mirror.py


def check(fasta, xs, ys, tl, tr, band):
    args = [fasta, LG, tl, tr] + ([] if band is None else [band])
    out, host = run(args, False), run(args, True)
    assert out[-1] == "dense matrix reads: 0"
    assert host[-1].startswith("dense matrix reads: ") and int(host[-1].split()[-1]) > 0
    assert out[:-1] == host[:-1]
    n_words = 6 * (len(xs) + len(ys)) + 16
    # the sibling matrix: sample from std::mt19937(20)
    sib = restated(xs, ys, tl, tr, band)
    words = wr.mt_words(20, n_words)
    w = wr.sibling_walk(sib, wr.WordSource(words))
    assert w.margin >= MARGIN
    assert float.fromhex(out[0].split()[2]) == sib.lp_end
    assert out[1:4] == gapped((xs, ys), w.rows)
    assert out[4].split()[:2] == ["sibling", "logPostProb"] and close(float.fromhex(out[4].split()[2]), sib.log_post_prob(w.rows))
    assert out[5] == "sibling next word %d" % words[w.words_used]
    # the branch matrix, left sequence as parent: sample from std::mt19937(21), best() of the Viterbi matrix
    fwd, vit = restated_branch(xs, ys, tl, band, False), restated_branch(xs, ys, tl, band, True)
    words = wr.mt_words(21, n_words)
    w = wr.branch_walk(fwd, wr.WordSource(words))
    assert w.margin >= MARGIN
    assert float.fromhex(out[6].split()[2]) == fwd.lp_end
    assert out[7:9] == gapped((xs, ys), w.rows)
    assert out[9].split()[:2] == ["branch", "logPostProb"] and close(float.fromhex(out[9].split()[2]), wr.branch_log_post_prob(fwd, w.rows))
    assert out[10] == "branch next word %d" % words[w.words_used]
    assert float.fromhex(out[11].split()[2]) == vit.lp_end
    assert out[12:14] == gapped((xs, ys), vit.best())
    # sampleBatch over a fillBatch of two envelopes (none, band or 10): the banded one's alignment from std::mt19937(31)
    assert out[14] == "sampleBatch equals single samples: yes"
    banded = sib if band is not None else restated(xs, ys, tl, tr, 10)
    w = wr.sibling_walk(banded, wr.WordSource(wr.mt_words(31, n_words)))
    assert w.margin >= MARGIN
    assert out[15:18] == gapped((xs, ys), w.rows)


@pytest.mark.parametrize("band", [None, 3])
def test_walks_of_the_mirror_on_the_pf16593_pair(band):
    (_, xs), (_, ys) = read_fasta(G + "PF16593.pair.fa")
    check(G + "PF16593.pair.fa", xs, ys, 0.7, 0.4, band)


def test_walks_of_the_mirror_on_a_gp120_pair_of_several_strips(tmp_path):
    seqs = read_fasta(G + "gp120.fa")[:2]
    (_, xs), (_, ys) = [(n, s.replace("-", "")) for n, s in seqs]
    pair = tmp_path / "gp120.pair.fa"
    pair.write_text("".join(">%s\n%s\n" % (n, s.replace("-", "")) for n, s in seqs))
    check(str(pair), xs, ys, 0.3, 0.5, 20)
