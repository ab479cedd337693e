"""`historian count` / `fit -fixsubrates` on unaligned sequences through the C++ mirror (hxrecon `count indel`, `fit`):
profiles that carry indel counts, the root's getCounts on the device (hx_batch_event_counts), and the EM loop over the indel
rates - against tests/indel_carry_ref.py's restatement of the same loop (fills by the plain-C oracle, which the exact policy
reproduces bit for bit)."""
import os
import subprocess

import pytest

from oracle import historian_oracle as ho
from tests import indel_carry_ref as R
from tests import recon_helpers as RH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HXRECON = os.path.join(ROOT, "historian_amd", "bin", "hxrecon")
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
MODEL = G + "testcount.jukescantor.json"


def _model():
    m = ho.RateModel.from_file(MODEL)
    m.sub_rate = [x.tolist() for x in m.sub_rate]
    return m


def _testcount():
    tree = RH.parse_newick(open(G + "testcount.nh").read())
    ung = dict(R.read_fasta(G + "testcount.fa"))
    return tree, {n: (tree.name[n], ung[tree.name[n]]) for n in range(tree.nodes()) if tree.is_leaf(n)}


def _families():
    return [_testcount(), RH.balanced_family(4, 16, "ACGT", seed=3, branch=.1)]


def _run(tmp_path, families, **opts):
    jobs = []
    for k, (tree, seqs) in enumerate(families):
        job = str(tmp_path / ("job%d.txt" % k))
        RH.write_job(job, MODEL, tree, seqs, {}, str(tmp_path / ("s%d.fa" % k)), str(tmp_path / ("g%d.fa" % k)), **opts)
        jobs.append(job)
    out = subprocess.run([HXRECON] + jobs, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, HX_FILL_MODE="exact"))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout.decode()


def _values(text, tag):
    """{key: value} of the lines "<tag> <key> <hex> <%.9g>", one dict per occurrence of the tag's first key"""
    blocks = []
    for line in text.splitlines():
        f = line.split()
        if f and f[0] == tag:
            if f[1] == "ins":
                blocks.append({})
            blocks[-1][f[1]] = float.fromhex(f[2])
    return blocks


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1., abs(b))


def test_count_indel_on_testcount(tmp_path):
    tree, seqs = _testcount()
    text = _run(tmp_path, [(tree, seqs)], count="indel")
    got = _values(text, "indelCounts")
    assert len(got) == 1
    want = R.reconstruct_counts(_model(), tree, seqs)
    for k in R.KEYS + ("lp",):
        assert _close(got[0][k], want[k], 1e-9), (k, got[0][k], want[k])
    assert not any(line.startswith("row ") for line in text.splitlines())      # no root traceback in count mode


def test_count_indel_on_two_families(tmp_path):
    fams = _families()
    text = _run(tmp_path, fams, count="indel")
    got, total = _values(text, "indelCounts"), _values(text, "indelCountsTotal")
    assert len(got) == 2 and len(total) == 1
    model = _model()
    want = [R.reconstruct_counts(model, t, s) for t, s in fams]
    for k in R.KEYS + ("lp",):
        for g, w in zip(got, want):
            assert _close(g[k], w[k], 1e-9), (k, g[k], w[k])
        assert _close(total[0][k], want[0][k] + want[1][k], 1e-9), k


@pytest.mark.parametrize("which", ["testcount", "two families"])
def test_fit_matches_the_restated_em_loop(tmp_path, which):
    fams = _families()[:1] if which == "testcount" else _families()
    text = _run(tmp_path, fams, fit="6 0.001")
    em = [float.fromhex(line.split()[2]) for line in text.splitlines() if line.startswith("em ")]
    rates = {line.split()[0]: float.fromhex(line.split()[1]) for line in text.splitlines()
             if line.split()[0] in ("insRate", "delRate", "insExtProb", "delExtProb")}
    model = _model()
    want = R.fit(model, fams, 6, .001)
    assert len(em) == len(want), (em, want)
    for a, b in zip(em, want):
        assert _close(a, b, 1e-8), (a, b)
    for k, v in (("insRate", model.ins_rate), ("delRate", model.del_rate), ("insExtProb", model.ins_ext_prob),
                 ("delExtProb", model.del_ext_prob)):
        assert _close(rates[k], v, 1e-8), (k, rates[k], v)


def test_a_job_without_the_new_keys_prints_what_it_printed_before(tmp_path):
    # the reconstruction keys only: the same lines as ever (lpFinalFwd, lpFinalTrace, band, row), the oracle's reconstruction
    tree, seqs = _testcount()
    text = _run(tmp_path, [(tree, seqs)])
    assert {line.split()[0] for line in text.splitlines()} <= {"lpFinalFwd", "lpFinalTrace", "band", "row"}
    res, rows = RH.oracle_reconstruct(MODEL, tree, seqs, {})
    got = RH.parse_hxrecon(text)
    assert _close(got["lpFinalFwd"], res["lp_final_fwd"], 1e-12) and _close(got["lpFinalTrace"], res["lp_final_trace"], 1e-12)
    assert got["rows"] == rows
