"""Host side of the acquisition search under linear input constraints: `cell_boxes` against the brute force of
tests/domain_constraints_ref.py and against the oracle's walk, every refusal of `LinearConstraints`, and the repair step as
tests/domain_constraints_ref.py restates it — sound on every problem, complete where the constraints' supports are disjoint.
The GPU tests hold the kernel to that restatement bit for bit.  No GPU.

In every random case the restatement's mask must hold at least 10 % feasible and at least 10 % infeasible rows: `mixed` fails
the test otherwise, so no case passes because its constraint binds nowhere or everywhere."""
import numpy as np
import pytest

import domain_constraints_ref as cr
import domain_ref as dr
from bark_amd.optimizer import LinearConstraints, cell_boxes, domain as dom, split_table
from oracle import oracle as orc
from test_domain_cpu import HAND_BOUNDS, HAND_FT, hand_forest

CAT, INT, CONT = cr.CAT, cr.INT, cr.CONT


def mixed(mask):
    share = float(np.mean(mask))
    assert 0.1 <= share <= 0.9, f"{share:.3f} of the rows are feasible: the case does not test both outcomes"
    return mask


@pytest.fixture(scope="module")
def P5():
    model, data, bounds, ft = cr.mixed5()
    F = model[0]
    F.setflags(write=False)
    boxes = cr.brute_boxes(F, bounds, ft)
    table = split_table(F, bounds, ft)
    return F, bounds, ft, boxes, table


def run(boxes, ft, bounds, A, b, eq, rows, passes=4):
    """The restatement on (A, b, eq) -> (repaired, mask, csr + b + tol + eq)."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    eq = np.zeros(len(b), dtype=bool) if eq is None else np.asarray(eq, dtype=bool)
    con = (*cr.csr(A), np.asarray(b, dtype=np.float64), cr.tolerances(A, b, bounds), eq)
    out, mask = cr.repair(*boxes, ft, *con, rows, passes)
    return out, mask, con


def check_sound(boxes, ft, con, rows, out, mask):
    """Feasible rows: every constraint within tol, every coordinate in the cell it started in, untouched columns as they were."""
    off, lo, hi = boxes
    row_ptr, col, coef, b, tol, eq = con
    touched = sorted(set(int(c) for c in col))
    rest = [f for f in range(rows.shape[1]) if f not in touched]
    assert np.array_equal(out[:, rest], rows[:, rest])
    for i in np.flatnonzero(mask):
        for k in range(len(b)):
            r = sum(float(coef[e]) * float(out[i, col[e]]) for e in range(row_ptr[k], row_ptr[k + 1])) - b[k]
            assert (abs(r) <= tol[k]) if eq[k] else (r <= tol[k]), (i, k, r)
        for f in touched:
            c = cr.find_cell(off, hi, f, rows[i, f])
            assert c is not None and lo[c] <= out[i, f] <= hi[c], (i, f)


# ---- cell boxes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hand", "mixed5"])
def test_cell_boxes_invariants(case, P5):
    F, bounds, ft = (hand_forest(), HAND_BOUNDS, HAND_FT) if case == "hand" else P5[:3]
    boxes, table = cell_boxes(F, bounds, ft), split_table(F, bounds, ft)
    want = cr.brute_boxes(F, bounds, ft)
    for got, ref in zip(boxes, want):
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
    assert np.array_equal(boxes.cell_off, table.cell_off)
    assert (boxes.cell_lo <= table.cell_rep).all() and (table.cell_rep <= boxes.cell_hi).all()
    for f in range(len(ft)):
        lo, hi = boxes.cell_lo[boxes.cell_off[f]:boxes.cell_off[f + 1]], boxes.cell_hi[boxes.cell_off[f]:boxes.cell_off[f + 1]]
        if ft[f] == CAT:
            assert np.array_equal(lo, hi)
            continue
        # the cells tile the feature's range: no gap, no overlap
        assert lo[0] == (int(bounds[f, 0]) if ft[f] == INT else bounds[f, 0]) and hi[-1] == bounds[f, 1]
        assert (lo <= hi).all()
        assert np.array_equal(lo[1:], hi[:-1] + 1 if ft[f] == INT else np.nextafter(hi[:-1], np.inf))
    # both ends of every cell walk every tree as the representative does
    d = len(ft)
    base = table.cell_rep[table.cell_off[:-1]]
    for end in (boxes.cell_lo, boxes.cell_hi):
        rep_rows, end_rows = np.tile(base, (len(end), 1)), np.tile(base, (len(end), 1))
        for f in range(d):
            s = slice(int(table.cell_off[f]), int(table.cell_off[f + 1]))
            rep_rows[s, f], end_rows[s, f] = table.cell_rep[s], end[s]
        for forest in np.asarray(F).reshape((-1,) + np.asarray(F).shape[-2:]):
            assert np.array_equal(orc.pass_through_forest(forest, end_rows, ft), orc.pass_through_forest(forest, rep_rows, ft))


def test_one_point_feature_is_one_degenerate_cell(P5):
    F, bounds, ft, boxes, table = P5
    off, lo, hi = boxes
    assert off[5] - off[4] == 1 and lo[off[4]] == hi[off[4]] == 0.5


# ---- LinearConstraints ----------------------------------------------------------------------------------------------------------
def test_linear_constraints_compile():
    bounds = np.array([[0.0, 1.0], [-3.0, 2.0], [0.0, 10.0], [0.0, 11.0]])
    ft = np.array([CONT, CONT, INT, CAT])
    A = [[1.0, 2.0, 0.0, 0.0], [0.0, -1.0, 3.0, 0.0], [1.0, 1.0, 0.0, 0.0]]
    c = LinearConstraints(A, [1.0, -2.0, 0.5], [False, False, True]).compiled(bounds, ft)
    row_ptr, col, coef = cr.csr(A)
    assert np.array_equal(c.row_ptr, row_ptr) and np.array_equal(c.col, col) and np.array_equal(c.coef, coef)
    assert c.row_ptr.dtype == c.col.dtype == np.int64 and c.coef.dtype == c.b.dtype == c.tol.dtype == np.float64
    assert c.equality.dtype == np.uint8 and c.equality.tolist() == [0, 0, 1]
    assert np.allclose(c.tol, cr.tolerances(A, [1.0, -2.0, 0.5], bounds), rtol=1e-15, atol=0)
    assert np.allclose(c.tol, 1e-12 * np.array([1 + 1 + 6, 2 + 3 + 30, 0.5 + 1 + 3]), rtol=1e-15, atol=0)
    assert LinearConstraints([1.0, 1.0, 0.0, 0.0], [1.0]).A.shape == (1, 4)  # one row may come as a vector
    assert LinearConstraints(A, [1.0, -2.0, 0.5], tol=1e-9).compiled(bounds, ft).tol[0] == 1e-9 * 8


def test_linear_constraints_refusals():
    bounds = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 10.0], [0.0, 11.0]])
    ft = np.array([CONT, CONT, INT, CAT])
    with pytest.raises(ValueError, match="1 to 16"):
        LinearConstraints(np.ones((17, 4)), np.ones(17))
    with pytest.raises(ValueError, match="1 to 16"):
        LinearConstraints(np.ones((0, 4)), np.ones(0))
    with pytest.raises(ValueError, match="at most 64"):
        LinearConstraints(np.ones((2, 65)), np.ones(2))
    wide = np.zeros((2, 80))
    wide[0, :40], wide[1, 30:70] = 1.0, 1.0  # 70 distinct features over the two rows
    with pytest.raises(ValueError, match="at most 64"):
        LinearConstraints(wide, np.ones(2))
    wide[1, 64:] = 0.0
    LinearConstraints(wide, np.ones(2))      # exactly 64
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            LinearConstraints([[1.0, bad, 0.0, 0.0]], [1.0])
        with pytest.raises(ValueError, match="finite"):
            LinearConstraints([[1.0, 1.0, 0.0, 0.0]], [bad])
    with pytest.raises(ValueError, match="no non-zero"):
        LinearConstraints([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], [1.0, 1.0])
    with pytest.raises(ValueError, match=r"\(K, d\)"):
        LinearConstraints([[1.0, 1.0, 0.0, 0.0]], [1.0, 2.0])
    with pytest.raises(ValueError, match="categorical"):
        LinearConstraints([[1.0, 0.0, 0.0, 1.0]], [1.0]).compiled(bounds, ft)
    with pytest.raises(ValueError, match="integer"):
        LinearConstraints([[1.0, 0.0, 1.0, 0.0]], [1.0], [True]).compiled(bounds, ft)
    LinearConstraints([[1.0, 0.0, 1.0, 0.0]], [1.0], [False]).compiled(bounds, ft)  # an inequality may carry an integer
    with pytest.raises(ValueError, match="features"):
        LinearConstraints([[1.0, 1.0, 0.0]], [1.0]).compiled(bounds, ft)


# ---- the repair step ----------------------------------------------------------------------------------------------------------
RANDOM_CASES = {
    # name: (A, b, equality); d = 5, features (continuous [0, 1], continuous [-1, 2], integer [0, 10], categorical, {0.5})
    "budget": ([[1.0, 1.0, 0.0, 0.0, 0.0]], [0.9], None),
    "budget_with_integer": ([[1.0, 0.5, 0.2, 0.0, 0.0]], [1.6], None),
    "ordering": ([[1.0, -1.0, 0.0, 0.0, 0.0]], [0.0], None),
    "disjoint": ([[2.0, 0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.25, 0.0, 0.0]], [1.9, 2.2], None),
    "overlap": ([[1.0, 1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, -0.1, 0.0, 0.0], [0.0, -1.0, 0.3, 0.0, 0.0]], [1.2, -0.6, 1.5], None),
    "equality": ([[1.0, 0.25, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0]], [0.6, 8.0], [True, False]),
}


@pytest.mark.parametrize("name", sorted(RANDOM_CASES))
@pytest.mark.parametrize("passes", [1, 4])
def test_restatement_is_sound(P5, name, passes):
    F, bounds, ft, boxes, table = P5
    A, b, eq = RANDOM_CASES[name]
    rows = cr.uniform_rows(bounds, ft, 300, seed=11)
    out, mask, con = run(boxes, ft, bounds, A, b, eq, rows, passes)
    mixed(mask)
    check_sound(boxes, ft, con, rows, out, mask)
    for forest in F:  # the property the search rests on: the walk does not see the move
        assert np.array_equal(orc.pass_through_forest(forest, out[mask], ft), orc.pass_through_forest(forest, rows[mask], ft))


@pytest.mark.parametrize("name", ["budget", "budget_with_integer", "ordering", "disjoint", "equality"])
def test_restatement_is_complete_for_disjoint_supports(P5, name):
    """Every cell of the grid: feasible exactly where the closed box test admits the cell."""
    F, bounds, ft, boxes, table = P5
    A, b, eq = RANDOM_CASES[name]
    grid = dr.grid_product(*table)
    assert 2000 <= len(grid) <= 5000
    grid = grid[::3]
    out, mask, con = run(boxes, ft, bounds, A, b, eq, grid)
    row_ptr, col, coef, bb, tol, e = con
    for k in range(len(bb)):  # pairwise disjoint supports
        for j in range(k):
            assert not set(col[row_ptr[k]:row_ptr[k + 1]]) & set(col[row_ptr[j]:row_ptr[j + 1]])
    want = np.array([cr.box_admits(*boxes, row_ptr, col, coef, bb, e, x) for x in grid])
    assert np.array_equal(mixed(mask), want)
    check_sound(boxes, ft, con, grid, out, mask)


def test_equality_on_two_continuous_features():
    """x0 + x1 = 1 on [0, 1]^2 cut at thresholds that are no binary fractions."""
    from test_domain_cpu import chain_tree

    F = np.stack([chain_tree([(0, 0.3), (0, 0.55), (0, 0.8)]), chain_tree([(1, 0.15), (1, 0.6), (1, 0.35)])])[None]
    bounds, ft = np.array([[0.0, 1.0], [0.0, 1.0]]), np.array([CONT, CONT])
    boxes, table = cr.brute_boxes(F, bounds, ft), split_table(F, bounds, ft)
    assert np.array_equal(np.diff(table.cell_off), [4, 4])
    grid = dr.grid_product(*table)
    out, mask, con = run(boxes, ft, bounds, [[1.0, 1.0]], [1.0], [True], grid)
    mixed(mask)
    check_sound(boxes, ft, con, grid, out, mask)
    assert (np.abs(out[mask].sum(axis=1) - 1.0) <= 3e-12).all()
    want = np.array([cr.box_admits(*boxes, *con[:4], con[5], x) for x in grid])
    assert np.array_equal(mask, want)
    # a feasible row is not moved
    again, mask2, _ = run(boxes, ft, bounds, [[1.0, 1.0]], [1.0], [True], out[mask])
    assert mask2.all() and np.array_equal(again, out[mask])


def test_open_lower_edge_is_never_reached(P5):
    """A constraint that pushes x0 and x1 down as far as they go: the rows stop one step above the threshold that closes the
    cell below, and still walk the trees as before."""
    F, bounds, ft, boxes, table = P5
    off, lo, hi = boxes
    rows = cr.uniform_rows(bounds, ft, 300, seed=12)
    out, mask, con = run(boxes, ft, bounds, [[1.0, 1.0, 0.0, 0.0, 0.0]], [0.3], None, rows)
    mixed(mask)
    pinned = 0
    for f in (0, 1):
        thresholds = hi[off[f]:off[f + 1] - 1]  # the lower ends "a" of the feature's second, third, ... cell
        assert not np.isin(out[:, f], thresholds).any()
        pinned += int(np.isin(out[:, f], np.nextafter(thresholds, np.inf)).sum())
    assert pinned > 20  # the case does reach the edges
    inside = np.array([cr.box_admits(*boxes, *con[:4], con[5], x) is not None for x in rows])
    for forest in F:
        assert np.array_equal(orc.pass_through_forest(forest, out[inside], ft), orc.pass_through_forest(forest, rows[inside], ft))


def test_one_point_feature_is_never_moved(P5):
    F, bounds, ft, boxes, table = P5
    rows = cr.uniform_rows(bounds, ft, 200, seed=13)
    out, mask, _ = run(boxes, ft, bounds, [[0.0, 0.0, 0.0, 0.0, 1.0]], [0.4], None, rows)
    assert not mask.any() and np.array_equal(out, rows)
    out, mask, _ = run(boxes, ft, bounds, [[0.0, 0.0, 0.0, 0.0, 1.0]], [0.5], None, rows)
    assert mask.all() and np.array_equal(out, rows)
    out, mask, con = run(boxes, ft, bounds, [[1.0, 0.0, 0.0, 0.0, 1.0]], [0.9], None, rows)  # leaves x0 <= 0.4
    mixed(mask)
    assert (out[:, 4] == 0.5).all() and (out[mask, 0] <= 0.4 + 1e-12).all()
    check_sound(boxes, ft, con, rows, out, mask)


def test_rows_outside_every_cell_and_nan_rows_are_left_alone(P5):
    F, bounds, ft, boxes, table = P5
    rows = cr.uniform_rows(bounds, ft, 40, seed=14)
    rows[0, 0], rows[1, 0], rows[2, 1], rows[3, 2] = 1.5, -0.25, np.nan, 11.0
    rows[4, 3] = np.nan  # no coefficient on the categorical feature: not read
    out, mask, _ = run(boxes, ft, bounds, [[1.0, 1.0, 0.2, 0.0, 0.0]], [5.0], None, rows)
    assert not mask[:4].any() and mask[4:].all()
    assert out[:4].tobytes() == rows[:4].tobytes() and np.isnan(out[4, 3])


def test_search_loop_with_a_repair_callable():
    """`local_search` on the CPU with torch tensors: incumbents from feasible rows only, infeasible neighbours never win."""
    import torch

    off, rep = np.array([0, 4, 7]), np.array([0.0, 1.0, 2.0, 3.0, 0.0, 1.0, 2.0])
    acq = lambda rows: (rows[:, 0] - 3.0) ** 2 + (rows[:, 1] - 2.0) ** 2  # noqa: E731  the minimum (3, 2) is infeasible
    feasible = lambda rows: rows.sum(dim=1) <= 3.0                         # noqa: E731
    cand = torch.tensor(dr.grid_product(off, rep))
    seen = []

    def repair(rows):
        seen.append(rows.shape[0])
        return rows, feasible(rows)

    args = (acq, lambda first, n: cand[first:first + n], lambda x: torch.tensor(dr.neighbours(off, rep, x.numpy())), len(cand), 5, 2, 8)
    x, info = dom.local_search(*args, repair=repair)
    assert x.sum() <= 3.0 and info["value"] == 2.0 and sorted(x.tolist()) in ([1.0, 2.0], )
    assert sum(seen[:3]) == len(cand)
    x0, info0 = dom.local_search(*args)
    assert x0.tolist() == [3.0, 2.0] and info0["value"] == 0.0
    with pytest.raises(ValueError, match="no feasible cell"):
        dom.local_search(*args, repair=lambda rows: (rows, torch.zeros(rows.shape[0], dtype=torch.bool)))
