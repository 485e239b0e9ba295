"""The acquisition search under linear input constraints on the device — `optimizer.domain_repair`,
`propose_from_domain(constraints=...)`, csrc/domain.hip bark_domain_repair_hip — against the host restatement of
tests/domain_constraints_ref.py (which tests/test_domain_constraints_cpu.py shows sound, and complete for disjoint supports).

The repair is table look-ups, compares and multiplies, adds and divides that are rounded one by one: rows and mask are compared
bit for bit.  A repaired row stays in its cell, so its leaves and its acquisition value are compared bit for bit as well.  The
kernel has two instances, chosen by d alone (d <= 24 keeps the touched columns in LDS, wider rows work in place); the cell table
is read from global memory whatever its size, the 72 KB table below is there for the binary search's depth."""
import numpy as np
import pytest

import domain_constraints_ref as cr
from bark_amd import _lib

pytestmark = pytest.mark.gpu

CAT, INT, CONT = cr.CAT, cr.INT, cr.CONT
SEED = 0x5EED0456
_CACHE = {}

BUDGET = ([[1.0, 0.5, 0.2, 0.0, 0.0]], [1.6], None)
OVERLAP = ([[1.0, 1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, -0.1, 0.0, 0.0], [0.0, -1.0, 0.3, 0.0, 0.0]], [1.2, -0.6, 1.5], None)
EQUALITY = ([[1.0, 0.25, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0]], [0.6, 8.0], [True, False])


@pytest.fixture(scope="module")
def G():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd import optimizer

    return optimizer


def shared(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def mixed(mask):
    share = float(np.mean(mask))
    assert 0.1 <= share <= 0.9, f"{share:.3f} of the rows are feasible: the case does not test both outcomes"
    return mask


def problem5(G):
    def make():
        model, data, bounds, ft = cr.mixed5()
        boxes, table = G.cell_boxes(model[0], bounds, ft), G.split_table(model[0], bounds, ft)
        for got, want in zip(boxes, cr.brute_boxes(model[0], bounds, ft)):
            assert np.array_equal(got, want)
        assert 2000 <= G.domain_plan(table)["grid"] <= 5000
        return model, data, bounds, ft, boxes, table
    return shared("mixed5", make)


def problem70(G):
    def make():
        F, bounds, ft = cr.wide70()
        return F, bounds, ft, G.cell_boxes(F, bounds, ft)
    return shared("wide70", make)


def compiled(G, boxes, ft, case):
    """(LinearConstraints, its compiled form against the ends of the boxes, as `domain_repair` compiles it)."""
    A, b, eq = case
    con = G.LinearConstraints(A, b, eq)
    off, lo, hi = boxes
    return con, con.compiled(np.stack((lo[off[:-1]], hi[off[1:] - 1]), axis=1), ft)


def want_repair(boxes, ft, c, rows, passes):
    return cr.repair(*boxes, ft, c.row_ptr, c.col, c.coef, c.b, c.tol, c.equality.astype(bool), rows, passes)


def same_as_restatement(G, boxes, ft, case, rows, passes=4, want=None):
    """The kernel on `rows` against the restatement: identical bits, rows and mask.  -> (rows, mask) of the restatement."""
    con, c = compiled(G, boxes, ft, case)
    want_rows, want_ok = want_repair(boxes, ft, c, rows, passes) if want is None else want
    got_rows, got_ok = G.domain_repair(boxes, ft, con, np.array(rows), passes)
    got_rows, got_ok = got_rows.cpu().numpy(), got_ok.cpu().numpy()
    assert got_rows.dtype == np.float64 and got_ok.dtype == np.bool_ and got_rows.shape == rows.shape
    assert np.array_equal(got_ok, want_ok), np.flatnonzero(got_ok != want_ok)[:5]
    assert got_rows.tobytes() == want_rows.tobytes(), np.argwhere(got_rows != want_rows)[:5]
    return want_rows, want_ok


def rows5(G, n=1025):
    """Uniform rows of the d = 5 domain with four that lie outside every cell or hold a NaN in a touched column."""
    def make():
        bounds, ft = problem5(G)[2:4]
        rows = cr.uniform_rows(bounds, ft, 1025, seed=21)
        rows[3, 0], rows[100, 1], rows[256, 2], rows[1024, 0] = 1.5, np.nan, -1.0, np.nan
        rows[7, 3] = np.nan  # no coefficient there: neither read nor written
        rows.setflags(write=False)
        return rows
    return shared("rows5", make)[:n]


# ---- the kernel against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_repair_bit_for_bit_one_constraint(G, n, passes):
    model, data, bounds, ft, boxes, table = problem5(G)
    rows = rows5(G)
    whole = shared(("budget", passes), lambda: want_repair(boxes, ft, compiled(G, boxes, ft, BUDGET)[1], rows, passes))
    mixed(whole[1])
    assert not whole[1][[3, 100, 256, 1024]].any() and whole[0][[3, 100, 256, 1024]].tobytes() == rows[[3, 100, 256, 1024]].tobytes()
    same_as_restatement(G, boxes, ft, BUDGET, rows[:n], passes, (whole[0][:n], whole[1][:n]))  # a row does not depend on its neighbours


@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("name,case", [("overlap", OVERLAP), ("equality", EQUALITY)])
def test_repair_bit_for_bit_overlapping_and_equality_rows(G, name, case, passes):
    model, data, bounds, ft, boxes, table = problem5(G)
    want_rows, want_ok = same_as_restatement(G, boxes, ft, case, rows5(G, 600), passes)
    mixed(want_ok)
    assert np.isnan(want_rows[7, 3])


def sixteen_rows(d, touched, seed, shift):
    """K = 16 rows over the features `touched`: every row a random half of them, all of them used by some row."""
    rng = np.random.default_rng(seed)
    A = np.zeros((16, d))
    for k in range(16):
        pick = rng.permutation(touched)[:max(1, len(touched) // 2)]
        A[k, pick] = rng.uniform(0.25, 1.0, len(pick)) * rng.choice([-1.0, 1.0], len(pick))
    A[np.arange(len(touched)) % 16, touched] = np.where(A[np.arange(len(touched)) % 16, touched] == 0, 0.5,
                                                        A[np.arange(len(touched)) % 16, touched])
    return A, np.full(16, shift), None


def test_repair_sixteen_constraints(G):
    model, data, bounds, ft, boxes, table = problem5(G)
    case = sixteen_rows(5, [0, 1, 2, 4], seed=31, shift=1.0)
    assert np.count_nonzero(np.any(np.asarray(case[0]) != 0, axis=0)) == 4
    _, ok = same_as_restatement(G, boxes, ft, case, rows5(G, 300))
    mixed(ok)


@pytest.mark.parametrize("n", [1, 257])
def test_repair_one_touched_feature_of_seventy(G, n):
    """d = 70: the instance that works in the rows' own memory.  One coefficient: 69 columns are neither read nor written."""
    F, bounds, ft, boxes = problem70(G)
    rows = cr.uniform_rows(bounds, ft, 257, seed=22)
    rows[:, 40] = np.nan  # untouched
    rows[5, 17] = np.nan  # touched
    A = np.zeros((1, 70))
    A[0, 17] = -2.0       # x17 >= -0.05: two of its three cells end below that
    want_rows, ok = same_as_restatement(G, boxes, ft, (A, [0.1], None), rows[:n])
    if n > 1:
        mixed(ok)
        assert not ok[5] and np.isnan(want_rows[:, 40]).all()


def test_repair_sixty_four_touched_features(G):
    F, bounds, ft, boxes = problem70(G)
    rows = cr.uniform_rows(bounds, ft, 257, seed=23)
    touched = np.arange(3, 67)
    A = np.zeros((2, 70))  # two disjoint rows of 32 features
    A[0, touched[:32]], A[1, touched[32:]] = 1.0, np.linspace(-1.0, 1.0, 32) + 1.0 / 64
    want_rows, ok = same_as_restatement(G, boxes, ft, (A, [-26.0, -10.0], None), rows)
    mixed(ok)
    rest = np.setdiff1d(np.arange(70), touched)
    assert want_rows[:, rest].tobytes() == rows[:, rest].tobytes()
    # K = 16 rows of 32 coefficients over the same 64 features: 512 stored coefficients
    _, ok = same_as_restatement(G, boxes, ft, sixteen_rows(70, touched, seed=32, shift=2.0), rows[:96])
    mixed(ok)


def test_repair_with_a_table_past_64_kib(G):
    """9004 cells, 72 KB per array: thirteen steps of the binary search, the table read from global memory."""
    rng = np.random.default_rng(9)
    cells = [5000, 4001, 3]
    off = np.concatenate(([0], np.cumsum(cells))).astype(np.int64)
    hi = np.concatenate([np.sort(rng.uniform(0.0, 1.0, c - 1)).tolist() + [1.0] for c in cells])
    lo = np.concatenate([[0.0] + np.nextafter(hi[off[f]:off[f + 1] - 1], np.inf).tolist() for f in range(3)])
    boxes, ft = G.CellBoxes(off, lo, hi), np.full(3, CONT, dtype=np.int64)
    rows = rng.uniform(size=(300, 3))
    _, ok = same_as_restatement(G, boxes, ft, ([[1.0, 1.0, 0.0]], [0.999], None), rows)
    mixed(ok)


def test_caller_rows_are_not_modified_and_empty_input(G):
    import torch

    model, data, bounds, ft, boxes, table = problem5(G)
    con = G.LinearConstraints(*BUDGET)
    rows = torch.as_tensor(np.array(rows5(G, 64)), device="cuda")
    before = rows.clone()
    out, ok = G.domain_repair(boxes, ft, con, rows)
    assert out.data_ptr() != rows.data_ptr() and torch.equal(rows.nan_to_num(7.0), before.nan_to_num(7.0))
    out, ok = G.domain_repair(boxes, ft, con, rows[:0])
    assert out.shape == (0, 5) and ok.shape == (0,) and ok.dtype == torch.bool
    with pytest.raises(ValueError, match="passes"):
        G.domain_repair(boxes, ft, con, rows, passes=65)
    with pytest.raises(ValueError, match="categorical"):
        G.domain_repair(boxes, ft, G.LinearConstraints([[1.0, 0.0, 0.0, 1.0, 0.0]], [1.0]), rows)


# ---- what the repair preserves ------------------------------------------------------------------------------------------------
def test_cell_and_value_are_preserved(G):
    from bark_amd import forest as bf

    model, data, bounds, ft, boxes, table = problem5(G)
    rows = np.array(rows5(G, 600))
    rows[7, 3] = 1.0  # the scan reads every column
    out, ok = G.domain_repair(boxes, ft, G.LinearConstraints(*OVERLAP), rows)
    out, ok = out.cpu().numpy(), ok.cpu().numpy()
    mixed(ok)
    assert (out[ok] != rows[ok]).any(axis=1).mean() > 0.1  # rows did move
    for forest in model[0]:
        assert np.array_equal(bf.pass_through_forest(forest, out[ok], ft), bf.pass_through_forest(forest, rows[ok], ft))
    for kind in ("lcb_mean", "ei"):
        before = np.asarray(G.acquisition_scan(model, data, rows[ok], ft, kind=kind, return_values=True)[2])
        after = np.asarray(G.acquisition_scan(model, data, out[ok], ft, kind=kind, return_values=True)[2])
        assert before.dtype == np.float64 and np.isfinite(before).all() and before.tobytes() == after.tobytes()


# ---- the searches -----------------------------------------------------------------------------------------------------------------
def grid5(G):
    """(grid rows, unconstrained values of every row) of the d = 5 problem."""
    def make():
        model, data, bounds, ft, boxes, table = problem5(G)
        rows = G.domain_candidates(table, bounds, ft, G.domain_plan(table)["grid"], "grid", 0).cpu().numpy()
        return rows, np.asarray(G.acquisition_scan(model, data, rows, ft, return_values=True)[2])
    return shared("grid5", make)


def brute_force(G, case):
    """-> (x, grid index, value, feasible count): the restatement's repair and mask on the whole grid, the unconstrained values."""
    model, data, bounds, ft, boxes, table = problem5(G)
    rows, values = grid5(G)
    fixed, ok = want_repair(boxes, ft, compiled(G, boxes, ft, case)[1], rows, 4)
    at = int(np.flatnonzero(ok)[np.argmin(values[ok])])  # the first of equal minima
    return fixed[at], at, values[at], int(ok.sum())


def excluding_the_minimiser(G):
    """One constraint on x0 that cuts the unconstrained minimiser's cell off, by 1e-6: far more than tol, which would admit
    the cell's own edge."""
    model, data, bounds, ft, boxes, table = problem5(G)
    rows, values = grid5(G)
    off, lo, hi = boxes
    c = cr.find_cell(off, hi, 0, rows[int(np.argmin(values)), 0])
    if c > off[0]:
        return [[1.0, 0.0, 0.0, 0.0, 0.0]], [float(hi[c - 1]) - 1e-6], None  # x0 below the threshold under the cell
    return [[-1.0, 0.0, 0.0, 0.0, 0.0]], [-float(lo[c + 1]) - 1e-6], None   # x0 above the cell's upper end


@pytest.mark.parametrize("name", ["budget", "overlap", "excluding"])
def test_exhaustive_route_equals_the_brute_force(G, name):
    model, data, bounds, ft, boxes, table = problem5(G)
    case = {"budget": BUDGET, "overlap": OVERLAP}.get(name) or excluding_the_minimiser(G)
    x, at, value, count = brute_force(G, case)
    rows, values = grid5(G)
    free_x, free = G.propose_from_domain(model, data, bounds, ft, return_info=True)
    assert free["index"] == int(np.argmin(values)) and "feasible" not in free
    con = G.LinearConstraints(*case)
    for round_size in (500, 4096):
        got, info = G.propose_from_domain(model, data, bounds, ft, constraints=con, round_size=round_size, return_info=True)
        assert info["exhaustive"] and info["index"] == at and info["value"] == value
        assert got.dtype == np.float64 and got.tobytes() == x.tobytes()
        assert info["rows"] == len(rows) and info["feasible"] == count and 0 < count < len(rows)
        assert (np.asarray(case[0]) @ got <= np.asarray(case[1]) + 1e-9).all()
    if name == "excluding":
        assert at != free["index"] and value >= free["value"] and not np.array_equal(got, free_x)
    reuse = G.propose_from_domain(model, data, bounds, ft, constraints=con, reuse_fit=True, return_info=True)
    assert reuse[0].tobytes() == x.tobytes() and reuse[1]["value"] == value and reuse[1]["fits"] == 1


def test_nothing_feasible_is_a_value_error(G):
    model, data, bounds, ft, boxes, table = problem5(G)
    con = G.LinearConstraints([[1.0, 1.0, 0.0, 0.0, 0.0]], [-2.0])
    with pytest.raises(ValueError, match="no feasible cell"):
        G.propose_from_domain(model, data, bounds, ft, constraints=con)
    with pytest.raises(ValueError, match="no feasible cell"):
        G.propose_from_domain(model, data, bounds, ft, constraints=con, exhaustive_limit=0, n_candidates=200, starts=2)


def test_search_route(G):
    from bark_amd.tree_kernels import fit_posterior

    model, data, bounds, ft, boxes, table = problem5(G)
    A, b, _ = OVERLAP
    con = G.LinearConstraints(A, b)
    tol = compiled(G, boxes, ft, OVERLAP)[1].tol
    kw = dict(constraints=con, exhaustive_limit=0, n_candidates=300, starts=2, seed=SEED, return_info=True)
    x, info = G.propose_from_domain(model, data, bounds, ft, round_size=100, **kw)
    assert not info["exhaustive"] and info["index"] == -1 and info["sweeps"] >= 1
    assert (np.asarray(A) @ x - np.asarray(b) <= tol).all()
    assert info["value"] == float(G.acquisition_scan(model, data, x[None], ft, return_values=True)[2][0])
    assert info["start_values"].shape == (2,) and np.isfinite(info["start_values"]).all()
    assert info["value"] <= info["start_values"].min() and (info["final_values"] <= info["start_values"]).all()
    J = len(table.cell_rep)
    assert info["rows"] == 300 + info["sweeps"] * 2 * J and 0 < info["feasible"] < info["rows"]
    assert info["value"] >= brute_force(G, OVERLAP)[2]  # the restatement's minimum over the feasible cells
    others = [G.propose_from_domain(model, data, bounds, ft, round_size=4096, **kw),
              G.propose_from_domain(model, data, bounds, ft, round_size=100, reuse_fit=True, **kw),
              G.propose_from_domain(None, None, bounds, ft, round_size=100, posterior=fit_posterior(model, data, ft), **kw)]
    for other_x, other in others:
        assert other_x.tobytes() == x.tobytes() and other["value"] == info["value"]
        assert np.array_equal(other["final_values"], info["final_values"]) and other["feasible"] == info["feasible"]
    assert others[1][1]["fits"] == 1 and others[2][1]["fits"] == 0


def test_without_constraints_nothing_changes(G):
    model, data, bounds, ft, boxes, table = problem5(G)
    rows, values = grid5(G)
    keys = {"value", "exhaustive", "grid", "index", "sweeps", "scans", "fits", "start_values", "final_values"}
    x, info = G.propose_from_domain(model, data, bounds, ft, constraints=None, return_info=True)
    assert set(info) == keys and info["index"] == int(np.argmin(values)) and info["value"] == values.min()
    assert x.tobytes() == rows[info["index"]].tobytes() and info["scans"] == 1
    kw = dict(exhaustive_limit=0, n_candidates=300, starts=2, seed=SEED, return_info=True)
    x, info = G.propose_from_domain(model, data, bounds, ft, **kw)
    again, same = G.propose_from_domain(model, data, bounds, ft, constraints=None, passes=9, **kw)
    assert set(info) == keys and x.tobytes() == again.tobytes() and info["value"] == same["value"]
    at = np.flatnonzero((rows == x).all(axis=1))  # an unrepaired row is a row of representatives
    assert len(at) == 1 and values[at[0]] == info["value"]


# ---- the entry point's refusals -------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing(G):
    import torch

    model, data, bounds, ft, boxes, table = problem5(G)
    c = compiled(G, boxes, ft, BUDGET)[1]
    dev = {k: _lib.to_device(np.ascontiguousarray(v)) for k, v in dict(
        off=boxes.cell_off, lo=boxes.cell_lo, hi=boxes.cell_hi, ft=ft, row_ptr=c.row_ptr, col=c.col, coef=c.coef, b=c.b, tol=c.tol,
        eq=c.equality).items()}
    rows = torch.as_tensor(np.array(rows5(G, 64)), device="cuda")
    before = rows.clone()
    ok = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    total = len(boxes.cell_lo)

    def call(**over):
        a = dict(dev, total=total, d=5, K=1, passes=4, rows=rows, n=64, out=ok)
        a.update(over)
        return _lib.lib().bark_domain_repair_hip(
            _lib.ptr(a["off"]), _lib.ptr(a["lo"]), _lib.ptr(a["hi"]), a["total"], _lib.ptr(a["ft"]), a["d"], _lib.ptr(a["row_ptr"]),
            _lib.ptr(a["col"]), _lib.ptr(a["coef"]), _lib.ptr(a["b"]), _lib.ptr(a["tol"]), _lib.ptr(a["eq"]), a["K"], a["passes"],
            _lib.ptr(a["rows"]), a["n"], _lib.ptr(a["out"]), _lib.stream_ptr())

    refused = [dict(K=0), dict(K=17), dict(d=0), dict(d=4097), dict(total=4), dict(total=2 ** 20 + 1), dict(n=-1), dict(n=2 ** 32 + 1),
               dict(passes=0), dict(passes=65)]
    refused += [{name: None} for name in ("off", "lo", "hi", "ft", "row_ptr", "col", "coef", "b", "tol", "eq", "rows", "out")]
    for over in refused:
        assert call(**over) == _lib.BARK_ERR_ARG, over
        assert _lib.lib().bark_last_error()
    assert call(n=0, rows=None, out=None) == _lib.BARK_OK
    torch.cuda.synchronize()
    assert (ok == 7).all() and torch.equal(rows.nan_to_num(7.0), before.nan_to_num(7.0))
    assert call() == _lib.BARK_OK
    assert np.array_equal(ok.cpu().numpy().astype(bool), want_repair(boxes, ft, c, before.cpu().numpy(), 4)[1])


def test_constraint_arrays_the_kernel_cannot_address_mark_every_row_infeasible(G):
    """The CSR arrays are device memory: what the entry point cannot see, the kernel refuses without reading or writing past an
    array — a row_ptr that does not rise from 0, a column outside the row, a 65th touched feature."""
    import torch

    F, bounds, ft, boxes = problem70(G)
    rows = torch.as_tensor(cr.uniform_rows(bounds, ft, 300, seed=24), device="cuda")
    before = rows.clone()
    table = [_lib.to_device(np.ascontiguousarray(a)) for a in boxes]
    ftd = _lib.to_device(ft)

    def call(row_ptr, col):
        row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
        K = len(row_ptr) - 1
        args = [_lib.to_device(a) for a in (row_ptr, col, np.ones(len(col)), np.full(K, 100.0), np.zeros(K), np.zeros(K, dtype=np.uint8))]
        ok = torch.full((300,), 7, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().bark_domain_repair_hip(*(_lib.ptr(t) for t in table), len(boxes.cell_lo), _lib.ptr(ftd), 70,
                                                     *(_lib.ptr(t) for t in args), K, 4, _lib.ptr(rows), 300, _lib.ptr(ok),
                                                     _lib.stream_ptr()))
        return ok.cpu().numpy()

    assert (call([0, 3], [1, 2, 3]) == 1).all()  # the arrays as they should be: x1 + x2 + x3 <= 100 holds everywhere
    for row_ptr, col in (([1, 3], [1, 2, 3]), ([0, 3, 2], [1, 2, 3]), ([0, 3], [1, 2, 70]), ([0, 3], [-1, 2, 3]),
                         ([0, 65], list(range(65)))):
        assert (call(row_ptr, col) == 0).all(), (row_ptr, col)
    assert torch.equal(rows, before)
