"""The yardstick and the case set of tests/test_gpu_quickalign_edges.py, pinned on the CPU: the cases keep what they are there
for (ties of the end cell in every class, envelopes without a cell and with one), and the two restatements of the reference's
fill (oracle/oracle_quickalign.c, oracle/quickalign_oracle.py) agree bit for bit on the small ones, ties included."""
import numpy as np
import pytest

from tests import helpers as H
from tests import quickalign_edge_cases as E


def test_every_tie_class_holds_its_pairs():
    cases, members = E.random_tie_cases()
    by_name = {c[0]: c for c in cases}
    assert set(members) == set(E.TIE_CLASSES)
    for k in E.TIE_CLASSES:
        assert len(members[k]) >= 8, (k, members[k])
        for name in members[k]:
            assert k in E.tie_classes(by_name[name]), (k, name)
    # counted again over everything kept, straight from the definition
    count = dict.fromkeys(E.TIE_CLASSES, 0)
    for c in cases:
        r = E.oracle(c)
        mx = r["cells"][1:, 1:, 0]                                   # (end gaps are 0 under `integer`)
        hit = np.argwhere(mx == r["score"]) + 1
        win = (r["x_end"], r["y_end"])
        count["several_maxima"] += len(hit) > 1
        count["row_major_differs"] += len(hit) > 1 and tuple(hit[0]) != win
        count["winner_below_strip_0"] += len(hit) > 1 and (win[0] - 1) // 64 > 0
        count["several_in_column"] += int((hit[:, 1] == win[1]).sum()) > 1
        count["several_in_row"] += int((hit[:, 0] == win[0]).sum()) > 1
    assert all(v >= 8 for v in count.values()), count


def test_repeat_pairs_tie_as_described():
    for c in E.repeat_tie_cases():
        cells = E.maximal_cells(c)
        r = E.oracle(c)
        if c[0].startswith("tandem"):
            assert len(cells) == 28 and r["score"] == 42.0          # 21 matches; every further copy of the 7-mer ends one
        else:
            assert len(cells) == 61 and r["score"] == 140.0         # 2 min(i, j) at j = 70, i = 70 .. 130
        long_x = len(c[1]) > len(c[2])
        assert len({(j if long_x else i) for i, j in cells}) == 1     # all in one column (in one row once transposed)


@pytest.mark.parametrize("c", E.tie_cases(), ids=lambda c: c[0])
def test_the_winner_is_the_first_maximum_by_column_then_row(c):
    r = E.oracle(c)
    cells = E.maximal_cells(c)
    assert len(cells) > 1
    assert min(cells, key=lambda ij: (ij[1], ij[0])) == (r["x_end"], r["y_end"])


def test_envelopes_without_a_cell_and_with_one():
    for c in E.envelope_cases():
        kind = c[0].split("_", 2)[2]
        r = E.oracle(c)
        finite = int(np.isfinite(r["cells"][:, :, 0]).sum())
        if kind in E.NO_CELL:
            assert r["score"] == E.NEG_INF and (r["x_end"], r["y_end"]) == (0, 0) and finite == 0, c[0]
            assert not np.isfinite(r["cells"]).any()
        elif kind in E.ONE_CELL:
            assert finite == 1 and np.isfinite(r["score"]), c[0]
            assert (r["x_end"], r["y_end"]) == ((len(c[1]), 1) if kind == "corner_x" else (1, len(c[2])))
        elif kind == "alternate":
            assert not np.isfinite(r["cells"][:, :, 1:]).any() and finite > 0, c[0]      # no ins or del without a neighbour
        else:
            assert finite > 1, c[0]


def small_cases():
    out = [c for c in E.shape_grid_cases() if len(c[1]) <= 17 and len(c[2]) <= 17]
    out += [E.cut(c, 40, 40) for c in E.random_tie_cases()[0]]
    out += [E.cut(c, 40, 40) for c in E.repeat_tie_cases()]
    out += list(E.envelope_cases())
    out += [c for c in E.alphabet_cases() if c[0].endswith("foreign_all")]
    for s in E.SCORE_SETS:
        out += [c for c in E.score_set_cases(s) if len(c[1]) <= 65]
    return out


@pytest.mark.parametrize("c", small_cases(), ids=lambda c: c[0])
def test_the_two_restatements_agree(c):
    want = E.oracle(c)
    mx = E.python_matrix(c)
    H.assert_same_bits(E.python_cells(mx), want["cells"], c[0])
    H.assert_same_bits([mx.end], [want["score"]], c[0] + " score")
    assert (mx.x_end, mx.y_end) == (want["x_end"], want["y_end"])


def test_the_cut_tie_pairs_still_tie():
    # (so that the comparison of the two restatements above decides end cells by the scan order as well)
    tied = sum(len(E.maximal_cells(E.cut(c, 40, 40))) > 1 for c in E.tie_cases())
    assert tied >= 8, tied


def test_case_names_are_unique_and_the_sets_complete():
    groups = [E.tie_cases(), E.shape_grid_cases(), E.alphabet_cases(), E.envelope_cases(), E.large_batch(384)]
    groups += list(E.column_table_batches()) + [E.score_set_cases(s) for s in E.SCORE_SETS]
    names = [c[0] for g in groups for c in g]
    assert len(names) == len(set(names))
    assert len(E.shape_grid_cases()) == 92
    assert {(len(c[1]), len(c[2])) for c in E.shape_grid_cases()} == {(r, cc) for r in E.GRID_ROWS for cc in E.GRID_COLS} | {(1089, 17)}
    assert sorted({c[3] for c in E.alphabet_cases()}) == [1, 4, 20, 31]
    for c in (c for g in groups for c in g):
        for v in list(c[5]) + list(np.ravel(c[4])):
            assert not (v == 0 and np.signbit(v)), c[0]             # zeros are +0.0 (hx_quick.hip, dmax)
        assert np.isfinite(c[5][9])                                  # gap_extend: 0 * -inf would be NaN
