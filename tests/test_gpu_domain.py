"""Acquisition search over the whole domain on the device — bark_amd.optimizer.domain, csrc/domain.hip — against the host
restatement of tests/domain_ref.py (which tests/test_domain_cpu.py holds to the oracle's walk).

The generators are integer arithmetic, table look-ups and one multiply-add without contraction per element: every row is
compared bit for bit.  The searches go through `acquisition_scan`, whose value for a row does not depend on the rows around
it, so "exact" below means equal doubles, not a tolerance."""
import numpy as np
import pytest

import domain_ref as dr
from bark_amd import synthetic

pytestmark = pytest.mark.gpu

CAT, INT, CONT = dr.CAT, dr.INT, dr.CONT
SEED = 0x5EED0123
_CACHE = {}


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


def generator_case(d):
    """(table, bounds, ft) with d features cycling through continuous, integer and categorical."""
    def make():
        kinds = [CONT, INT, CAT]
        ft = np.array([kinds[f % 3] for f in range(d)], dtype=np.int64)
        bounds = np.array([[(-1.5, 2.25), (-3.0, 12.0), (0.0, float(0b1011010))][f % 3] for f in range(d)])
        F = synthetic.sample_prior_forests(3, 6, bounds, ft, seed=40 + d)
        from bark_amd.optimizer import split_table

        table = split_table(F, bounds, ft)
        assert np.array_equal(table.cell_off, dr.brute_table(F, bounds, ft)[0])
        return table, bounds, ft
    return shared(("gen", d), make)


def same_rows(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("mode", ["uniform", "cells", "grid"])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_generator_rows_bit_for_bit(G, mode, n):
    table, bounds, ft = generator_case(5)
    grid = G.domain_plan(table)["grid"]
    n = min(n, grid)
    want = shared(("rows", mode, 1000), lambda: dr.candidates(*table, bounds, ft, min(1000, grid), mode, SEED, 3))
    same_rows(G.domain_candidates(table, bounds, ft, n, mode, SEED, round=3), want[:n])


@pytest.mark.parametrize("mode", ["uniform", "cells", "grid"])
def test_rows_do_not_depend_on_first(G, mode):
    table, bounds, ft = generator_case(5)
    n = min(1000, G.domain_plan(table)["grid"])
    whole = G.domain_candidates(table, bounds, ft, n, mode, SEED, round=3)
    import torch

    parts = torch.cat([G.domain_candidates(table, bounds, ft, 300, mode, SEED, round=3),
                       G.domain_candidates(table, bounds, ft, n - 300, mode, SEED, round=3, first=300)])
    assert torch.equal(whole, parts)
    assert G.domain_candidates(table, bounds, ft, 0, mode, SEED).shape == (0, 5)


def test_grid_is_the_cartesian_product_in_itertools_order(G):
    table, bounds, ft = generator_case(2)
    same_rows(G.domain_candidates(table, None, None, G.domain_plan(table)["grid"], "grid", 0), dr.grid_product(*table))


@pytest.mark.parametrize("mode", ["uniform", "cells"])
def test_row_index_past_32_bits(G, mode):
    table, bounds, ft = generator_case(5)
    first = 2 ** 32 - 5
    want = dr.candidates(*table, bounds, ft, 10, mode, SEED, 0, first)
    same_rows(G.domain_candidates(table, bounds, ft, 10, mode, SEED, first=first), want)
    low = dr.candidates(*table, bounds, ft, 5, mode, SEED, 0, 0)  # what a truncated high word would repeat
    assert not np.array_equal(want[5:], low)


@pytest.mark.parametrize("mode", ["uniform", "cells", "grid"])
@pytest.mark.parametrize("d", [1, 2, 7])
def test_one_feature_and_a_half_used_last_block(G, mode, d):
    table, bounds, ft = generator_case(d)
    n = min(300, G.domain_plan(table)["grid"])
    same_rows(G.domain_candidates(table, bounds, ft, n, mode, SEED, round=1), dr.candidates(*table, bounds, ft, n, mode, SEED, 1))


@pytest.mark.parametrize("mode", ["uniform", "cells"])
def test_round_and_high_seed_word_address_the_stream(G, mode):
    import torch

    table, bounds, ft = generator_case(5)
    base = G.domain_candidates(table, bounds, ft, 200, mode, SEED)
    other_round = G.domain_candidates(table, bounds, ft, 200, mode, SEED, round=1)
    assert not torch.equal(base, other_round)
    same_rows(other_round, dr.candidates(*table, bounds, ft, 200, mode, SEED, 1))
    high = SEED + (0xABCD << 32)
    got = G.domain_candidates(table, bounds, ft, 200, mode, high)
    assert not torch.equal(base, got)
    same_rows(got, dr.candidates(*table, bounds, ft, 200, mode, high))


def test_table_beyond_the_lds_copy(G):
    """A table of more than 64 KiB is read from global memory: the other kernel instance, the same rows."""
    rng = np.random.default_rng(9)
    cells = [5000, 4001, 3]
    off = np.concatenate(([0], np.cumsum(cells))).astype(np.int64)
    table = G.CellTable(off, rng.uniform(size=int(off[-1])))
    bounds, ft = np.tile([[0.0, 1.0]], (3, 1)), np.full(3, CONT)
    for mode, first in (("cells", 0), ("grid", 5000 * 4001 * 3 - 700)):
        same_rows(G.domain_candidates(table, bounds, ft, 700, mode, SEED, first=first),
                  dr.candidates(off, table.cell_rep, bounds, ft, 700, mode, SEED, 0, first))
    x = rng.uniform(size=(2, 3))
    same_rows(G.domain_neighbours(table, x), dr.neighbours(off, table.cell_rep, x))


@pytest.mark.parametrize("K", [1, 3])
def test_neighbours_bit_for_bit(G, K):
    table, bounds, ft = generator_case(5)
    x = dr.candidates(*table, bounds, ft, K, "uniform", SEED + 1)
    same_rows(G.domain_neighbours(table, x), dr.neighbours(*table, x))
    import torch

    assert torch.equal(G.domain_neighbours(table, torch.as_tensor(x, device="cuda")), G.domain_neighbours(table, x))


def test_neighbours_refuse_more_rows_than_the_scan_takes(G):
    table, bounds, ft = generator_case(5)
    J = len(table.cell_rep)
    import torch

    x = torch.zeros((1, 5), dtype=torch.float64, device="cuda").expand(2 ** 24 // J + 1, 5)  # a view: 40 bytes
    with pytest.raises(ValueError, match="2\\^24"):
        G.domain_neighbours(table, x)
    with pytest.raises(ValueError, match="unknown mode"):
        G.domain_candidates(table, bounds, ft, 4, "sobol", 0)
    with pytest.raises(ValueError, match="round"):
        G.domain_candidates(table, bounds, ft, 4, "cells", 0, round=-1)


# ---- the searches ---------------------------------------------------------------------------------------------------------------
def small_problem():
    """N = 16, d = 3 (continuous, integer, 4 categories), 3 forests of 4 trees: a grid of a few hundred cells."""
    def make():
        X, y, bounds, ft = synthetic.mixed_problem(16, seed=12, d_cont=1, n_int=1, n_cat=1, cats=4)
        F = synthetic.sample_prior_forests(3, 4, bounds, ft, seed=77)
        model = (F, np.array([0.1, 0.05, 0.2]), np.array([1.0, 0.8, 1.2]))
        return model, (X, y), bounds, ft
    return shared("small", make)


def large_problem():
    """N = 24, d = 5, 4 forests of 8 trees: searched, never enumerated."""
    def make():
        X, y, bounds, ft = synthetic.mixed_problem(24, seed=13, d_cont=3, n_int=1, n_cat=1, cats=4)
        F = synthetic.sample_prior_forests(4, 8, bounds, ft, seed=78)
        model = (F, np.array([0.1, 0.05, 0.2, 0.15]), np.array([1.0, 0.8, 1.2, 0.9]))
        return model, (X, y), bounds, ft
    return shared("large", make)


def grid_scan(G, kind):
    """(rows, values, minimum, index) of one scan over the materialised grid of the small problem."""
    def make():
        model, data, bounds, ft = small_problem()
        table = G.split_table(model[0], bounds, ft)
        grid = G.domain_plan(table)["grid"]
        assert 100 <= grid <= 2000, grid
        rows = G.domain_candidates(table, bounds, ft, grid, "grid", 0)
        value, index, acq = G.acquisition_scan(model, data, rows, ft, kind=kind, return_values=True)
        return rows.cpu().numpy(), acq.cpu().numpy(), float(value), int(index)
    return shared(("grid", kind), make)


@pytest.mark.parametrize("kind", ["lcb_mean", "lcb_mixture", "ei"])
def test_exhaustive_is_exact(G, kind):
    model, data, bounds, ft = small_problem()
    rows, acq, value, index = grid_scan(G, kind)
    assert value == acq.min() and index == int(np.argmin(acq))
    for round_size in (97, 4096):
        x, info = G.propose_from_domain(model, data, bounds, ft, kind=kind, round_size=round_size, return_info=True)
        assert info["exhaustive"] and info["grid"] == len(rows) and info["scans"] == -(-len(rows) // round_size)
        assert info["value"] == value and info["index"] == index  # bit for bit, the same row
        assert x.dtype == np.float64 and np.array_equal(x, rows[index])
    # the reference's own criterion (tests/optimization/test_optimality.py): no worse than random candidates.  Exact: every
    # point lies in a cell, and a cell's value is that of its representative.
    table = G.split_table(model[0], bounds, ft)
    cand = G.domain_candidates(table, bounds, ft, 10 ** 4, "uniform", SEED)
    random_best, _ = G.acquisition_scan(model, data, cand, ft, kind=kind)
    assert info["value"] <= float(random_best)


def test_search_never_goes_below_the_exhaustive_minimum(G):
    model, data, bounds, ft = small_problem()
    rows, acq, value, index = grid_scan(G, "lcb_mean")
    x, info = G.propose_from_domain(model, data, bounds, ft, exhaustive_limit=0, n_candidates=2000, starts=8, seed=SEED,
                                    return_info=True)
    assert not info["exhaustive"] and info["value"] >= value
    at = np.flatnonzero((rows == x).all(axis=1))
    assert len(at) == 1 and acq[at[0]] == info["value"]  # the row returned is the row scored


def test_search_ends_in_a_local_minimum_and_is_reproducible(G):
    model, data, bounds, ft = large_problem()
    kw = dict(exhaustive_limit=0, n_candidates=5000, starts=4, seed=SEED, return_info=True)
    x, info = G.propose_from_domain(model, data, bounds, ft, round_size=1000, **kw)
    assert not info["exhaustive"] and info["grid"] > 5000 and 1 <= info["sweeps"] < 32
    assert info["scans"] == 5 + info["sweeps"]
    assert info["start_values"].shape == info["final_values"].shape == (4,)
    assert (info["final_values"] <= info["start_values"]).all() and info["value"] == info["final_values"].min()
    assert (np.diff(info["start_values"]) >= 0).all()
    table = G.split_table(model[0], bounds, ft)
    _, _, near = G.acquisition_scan(model, data, G.domain_neighbours(table, x[None]), ft, return_values=True)
    assert float(near.min()) == info["value"]  # nothing strictly lower, and x's own cell is among its neighbours
    for other in (G.propose_from_domain(model, data, bounds, ft, round_size=4096, **kw),
                  G.propose_from_domain(model, data, bounds, ft, round_size=1000, **kw)):
        assert np.array_equal(other[0], x) and other[1]["value"] == info["value"]
        assert np.array_equal(other[1]["final_values"], info["final_values"])
    uniform = G.propose_from_domain(model, data, bounds, ft, round_size=4096, mode="uniform", **kw)[1]
    assert (uniform["final_values"] <= uniform["start_values"]).all()


def test_pending_is_passed_through(G):
    model, data, bounds, ft = small_problem()
    first = G.propose_from_domain(model, data, bounds, ft)
    second, info = G.propose_from_domain(model, data, bounds, ft, pending=first[None], return_info=True)
    assert not np.array_equal(first, second)
    table = G.split_table(model[0], bounds, ft)
    rows = G.domain_candidates(table, bounds, ft, info["grid"], "grid", 0)
    value, index = G.acquisition_scan(model, data, rows, ft, pending=first[None])
    assert info["value"] == float(value) and info["index"] == int(index)
