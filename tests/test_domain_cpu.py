"""Host side of the acquisition search over the whole domain (bark_amd/optimizer/domain.py): the cell table against the brute
force of tests/domain_ref.py, the property that makes one representative per cell enough (every point of a cell reaches the
leaves its representative reaches, checked with the oracle's walk), the plan, the refusals, and the search loop.  No GPU."""
import numpy as np
import pytest

import domain_ref as dr
from bark_amd import _lib, forest as bf, synthetic
from bark_amd.optimizer import domain as dom
from oracle import oracle as orc

CAT, INT, CONT = dr.CAT, dr.INT, dr.CONT


def chain_tree(splits, L=32):
    """A right-leaning chain: node 2i splits on splits[i] with leaf 2i + 1 on its left; the last right child is a leaf."""
    t = np.zeros(L, dtype=bf.NODE_RECORD_DTYPE)
    n = len(splits)
    for i, (f, thr) in enumerate(splits):
        t[2 * i] = (0, f, thr, 2 * i + 1, 2 * i + 2, 0xFFFFFFFF if i == 0 else 2 * i - 2, i, 1)
        t[2 * i + 1] = (1, 0, 0, 0, 0, 2 * i, i + 1, 1)
    t[2 * n] = (1, 0, 0, 0, 0, max(2 * n - 2, 0), n, 1)
    return t


# hand-made: f0 continuous [0, 1], f1 integer [0, 10], f2 integer [3, 3], f3 categorical {0, 1, 3}
HAND_BOUNDS = np.array([[0.0, 1.0], [0.0, 10.0], [3.0, 3.0], [0.0, 11.0]])
HAND_FT = np.array([CONT, INT, INT, CAT], dtype=np.int64)


def hand_forest():
    trees = [
        # thresholds equal to lo and to hi, one outside the bounds, a duplicated one
        chain_tree([(0, 0.25), (0, 0.0), (0, 0.75), (0, 1.0), (0, 1.5), (0, 0.75), (0, -0.5)]),
        # a non-integer threshold on an integer feature, floor(t) == hi (no boundary), t == lo (a boundary), duplicates by floor
        chain_tree([(1, 4.5), (1, 4.0), (1, 10.0), (1, 0.0), (1, 7.0), (1, 10.5), (1, -1.0)]),
        # the one-point integer feature and a categorical split
        chain_tree([(2, 3.0), (3, 2.0), (2, 2.0), (0, 0.5)]),
    ]
    # a pruned split: node 2 split f0 at 0.6 and was pruned back to a leaf, so its children are inactive
    pruned = chain_tree([(0, 0.4), (0, 0.6)])
    pruned[2]["is_leaf"] = 1
    pruned[3]["active"] = pruned[4]["active"] = 0
    assert pruned[2]["feature_idx"] == 0 and float(pruned[2]["threshold"]) == np.float32(0.6)  # stale fields of the leaf stay
    trees.append(pruned)
    # an inactive record that still looks like an internal node
    stale = chain_tree([(0, 0.1)])
    stale[10] = (0, 0, 0.9, 0, 0, 0, 0, 0)
    trees.append(stale)
    return np.stack(trees)


@pytest.fixture(scope="module")
def prior():
    X, y, bounds, ft = synthetic.mixed_problem(16, seed=3)
    F = synthetic.sample_prior_forests(4, 8, bounds, ft, seed=21)
    F.setflags(write=False)
    return F, bounds, ft


def same_table(got, want):
    assert got.cell_off.dtype == np.int64 and got.cell_rep.dtype == np.float64
    assert np.array_equal(got.cell_off, want[0]) and got.cell_rep.tobytes() == want[1].tobytes()


def test_split_table_equals_brute_force(prior):
    F, bounds, ft = prior
    same_table(dom.split_table(F, bounds, ft), dr.brute_table(F, bounds, ft))
    same_table(dom.split_table(F[1, 2], bounds, ft), dr.brute_table(F[1, 2], bounds, ft))  # any leading shape
    H = hand_forest()
    table = dom.split_table(H, HAND_BOUNDS, HAND_FT)
    same_table(table, dr.brute_table(H, HAND_BOUNDS, HAND_FT))
    # by hand: f0 boundaries 0.1, 0.25, 0.4, 0.75 (0.0, 1.0, 1.5, -0.5, the pruned 0.6 and the stale 0.9 are not)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    edges = [0.0, f32(0.1), 0.25, f32(0.4), 0.5, 0.75, 1.0]
    assert np.array_equal(table.cell_rep[:6], [0.5 * (a + b) for a, b in zip(edges[:-1], edges[1:])])
    # f1: floors 4, 4, 10 (== hi: none), 0, 7, 10, -1 -> boundaries 0, 4, 7 -> cells [0,0] [1,4] [5,7] [8,10]
    assert table.cell_rep[6:10].tolist() == [0.0, 2.0, 6.0, 9.0]
    assert table.cell_rep[10:].tolist() == [3.0, 0.0, 1.0, 3.0] and table.cell_off.tolist() == [0, 6, 10, 11, 14]


def test_representative_that_would_round_onto_the_lower_end_takes_the_upper():
    # a cell whose ends are neighbouring doubles: thresholds are float32, so the upper bound supplies the second end
    t = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    tree = chain_tree([(0, t)])[None]
    b = np.array([[0.0, np.nextafter(t, 2.0)]])
    assert 0.5 * (t + b[0, 1]) == t  # the midpoint rounds onto the lower end, which belongs to the cell below
    table = dom.split_table(tree, b, np.array([CONT]))
    same_table(table, dr.brute_table(tree, b, np.array([CONT])))
    assert table.cell_rep.tolist() == [0.5 * t, b[0, 1]]


def leaves_of(F3, points, ft):
    """(B, n, m) leaf indices by the oracle's walk."""
    return np.stack([orc.pass_through_forest(F3[b], points, ft) for b in range(F3.shape[0])])


@pytest.mark.parametrize("which", ["prior", "hand"])
def test_every_point_of_a_cell_reaches_the_leaves_of_its_representative(prior, which):
    if which == "prior":
        F, bounds, ft = prior
    else:
        F, bounds, ft = hand_forest()[None], HAND_BOUNDS, HAND_FT
    off, rep = dom.split_table(F, bounds, ft)
    ranges = dr.cell_ranges(F, bounds, ft)
    bases = dr.candidates(off, rep, bounds, ft, 12, "cells", seed=5)
    J, d = len(rep), len(ft)
    owner = np.repeat(np.arange(d), np.diff(off))
    at_rep = dr.neighbours(off, rep, bases)
    for end in (0, 1):
        other = at_rep.copy().reshape(len(bases), J, d)
        for j in range(J):
            a, b = ranges[j]
            assert a <= rep[j] <= b
            other[:, j, owner[j]] = (a, b)[end]
        assert np.array_equal(leaves_of(F, at_rep, ft), leaves_of(F, other.reshape(-1, d), ft))


def test_neighbouring_cells_are_told_apart_by_the_split_between_them(prior):
    """Every boundary comes from a split; a point of that node's subspace goes left with the cell below it and right with
    the cell above, so the two representatives differ in that tree — and no boundary is there without such a split."""
    F, bounds, ft = prior
    off, rep = dom.split_table(F, bounds, ft)
    ranges = dr.cell_ranges(F, bounds, ft)
    seen = set()
    for b in range(F.shape[0]):
        for t in range(F.shape[1]):
            tree = F[b, t]
            for i in np.flatnonzero((tree["active"] == 1) & (tree["is_leaf"] == 0)):
                f, thr = int(tree[i]["feature_idx"]), float(tree[i]["threshold"])
                if ft[f] == CAT:
                    continue
                sub = synthetic._subspace(tree, int(i), bounds, ft)
                probe = np.empty(len(ft))
                for g in range(len(ft)):
                    if ft[g] == CAT:
                        probe[g] = (int(sub[g, 1]) & -int(sub[g, 1])).bit_length() - 1
                    elif ft[g] == INT:
                        probe[g] = sub[g, 1]
                    else:
                        probe[g] = sub[g, 1]
                upper = np.floor(thr) if ft[f] == INT else thr
                below = [j for j in range(off[f], off[f + 1] - 1) if ranges[j][1] == upper]
                assert len(below) == 1, (b, t, i)
                j = below[0]
                two = np.stack([probe, probe])
                two[0, f], two[1, f] = rep[j], rep[j + 1]
                got = orc.pass_through_forest(F[b], two, ft)
                assert got[0, t] != got[1, t]
                seen.add(j)
    cont_or_int = [j for f in range(len(ft)) if ft[f] != CAT for j in range(off[f], off[f + 1] - 1)]
    assert seen == set(cont_or_int)


def test_domain_plan_and_refusals(prior):
    F, bounds, ft = prior
    table = dom.split_table(F, bounds, ft)
    plan = dom.domain_plan(table)
    want = [len(np.unique(F[(F["active"] == 1) & (F["is_leaf"] == 0) & (F["feature_idx"] == f)]["threshold"])) + 1 for f in range(10)]
    assert plan["cells"].tolist() == want + [5, 5]
    assert plan["neighbours"] == sum(want) + 10 == len(table.cell_rep)
    grid = 1
    for c in want + [5, 5]:
        grid *= c
    assert isinstance(plan["grid"], int) and plan["grid"] == grid
    big = dom.domain_plan(dom.CellTable(np.arange(0, 4096 * 256 + 1, 256), np.zeros(2 ** 20)))
    assert big["grid"] == 256 ** 4096 and big["neighbours"] == 2 ** 20  # far past 64 bits: a Python int

    zero = bounds.copy()
    zero[10, 1] = 0.0
    with pytest.raises(ValueError, match="zero mask"):
        dom.split_table(F, zero, ft)
    stump = chain_tree([(0, 0.5)])
    wide = np.tile([[0.0, 1.0]], (4097, 1))
    with pytest.raises(ValueError, match="4096 features"):
        dom.split_table(stump, wide, np.full(4097, CONT))
    assert dom.domain_plan(dom.split_table(stump, wide[:4096], np.full(4096, CONT)))["neighbours"] == 4097
    many = np.zeros(2 ** 20, dtype=bf.NODE_RECORD_DTYPE)
    many["active"] = 1
    many["threshold"] = (np.arange(1, 2 ** 20 + 1) / 2.0 ** 21).astype(np.float32)  # distinct, inside (0, 1)
    with pytest.raises(ValueError, match="2\\^20 cells"):
        dom.split_table(many, [[0.0, 1.0]], [CONT])
    assert dom.domain_plan(dom.split_table(many[1:], [[0.0, 1.0]], [CONT]))["grid"] == 2 ** 20
    with pytest.raises(ValueError, match="reads feature"):
        dom.split_table(chain_tree([(3, 0.5)]), [[0.0, 1.0]], [CONT])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    assert {"bark_domain_candidates_hip", "bark_domain_neighbours_hip"} <= set(_lib.SIGNATURES)
    off, rep, out = np.array([0, 2, 5], dtype=np.int64), np.zeros(5), np.zeros(10)  # host arrays: nothing may touch them
    b, ft = np.zeros((2, 2)), np.full(2, CONT, dtype=np.int64)
    p = _lib.ptr

    def cand(o, r, total, d, mode, n, first=0, round_=0, bounds=b):
        return lib.bark_domain_candidates_hip(p(o), p(r), total, p(bounds), p(ft), d, mode, 7, round_, first, n, p(out), None)

    for args, msg in [((off, rep, 5, 2, 3, 1), b"unknown mode"), ((off, rep, 5, 2, -1, 1), b"unknown mode"),
                      ((off, rep, 5, 2, 1, -1), b"n = -1"), ((off, rep, 5, 0, 1, 1), b"d = 0"), ((off, rep, 5, 4097, 1, 1), b"d = 4097"),
                      ((None, rep, 5, 2, 1, 1), b"null cell table"), ((off, None, 5, 2, 2, 1), b"null cell table"),
                      ((off, rep, 2 ** 20 + 1, 2, 1, 1), b"cells"), ((off, rep, 1, 2, 2, 1), b"cells"),
                      ((off, rep, 5, 2, 1, 1, -1), b"first"), ((off, rep, 5, 2, 1, 1, 0, 2 ** 32), b"round"),
                      ((None, None, 0, 2, 0, 1, 0, 0, None), b"bounds")]:
        assert cand(*args) == _lib.BARK_ERR_ARG and msg in lib.bark_last_error(), args
    assert cand(off, rep, 5, 2, 1, 0) == 0 and cand(None, None, 0, 2, 0, 0) == 0  # n == 0: a successful no-op
    assert lib.bark_last_error() == b""

    def near(o, r, total, d, K, x=out):
        return lib.bark_domain_neighbours_hip(p(o), p(r), total, d, p(x), K, p(out), None)

    assert near(off, rep, 5, 2, 0) == 0
    for args, msg in [((None, rep, 5, 2, 1), b"null cell table"), ((off, rep, 5, 0, 1), b"d = 0"), ((off, rep, 5, 2, -1), b"negative"),
                      ((off, rep, 5, 2, 2 ** 24 // 5 + 1), b"2^24"), ((off, rep, 2 ** 20, 2, 17), b"2^24"),
                      ((off, rep, 5, 2, 1, None), b"null argument")]:
        assert near(*args) == _lib.BARK_ERR_ARG and msg in lib.bark_last_error(), args
    assert near(off, rep, 2 ** 20, 2, 0) == 0


# ---- the search loop, on a synthetic piecewise-constant acquisition ----------------------------------------------------------------
class Synthetic:
    """acq(x) = sum_f w_f[cell_f(x)] + A[cell_0(x), cell_1(x)], rounded to one decimal so that ties are common."""

    def __init__(self, cells, seed):
        rng = np.random.default_rng(seed)
        self.off = np.concatenate(([0], np.cumsum(cells))).astype(np.int64)
        self.rep = np.concatenate([np.sort(rng.uniform(size=c)) for c in cells])
        self.w = [np.round(rng.normal(size=c), 1) for c in cells]
        self.A = np.round(rng.normal(size=(cells[0], cells[1])), 1)
        self.calls = 0

    def cell(self, rows, f):
        mine = self.rep[self.off[f]:self.off[f + 1]]
        at = np.searchsorted(mine, rows[:, f])
        assert np.array_equal(mine[at], rows[:, f])  # only representatives are ever scored
        return at

    def __call__(self, rows):
        self.calls += 1
        idx = [self.cell(rows, f) for f in range(len(self.w))]
        return np.round(sum(w[i] for w, i in zip(self.w, idx)) + self.A[idx[0], idx[1]], 1)

    def rows(self, seed):
        return lambda first, n: dr.candidates(self.off, self.rep, None, None, n, "cells", seed, 0, first)


@pytest.mark.parametrize("cells,n_candidates,starts", [((7, 5, 9, 4, 6), 400, 4), ((3, 2, 2), 300, 16), ((40, 30, 20, 10), 64, 3)])
def test_reference_search_ends_in_a_local_minimum(cells, n_candidates, starts):
    acq = Synthetic(cells, seed=sum(cells))
    x, info = dr.search(acq, acq.rows(11), acq.off, acq.rep, n_candidates, 128, starts, 32)
    assert info["sweeps"] < 32  # it stopped because nothing moved
    near = acq(dr.neighbours(acq.off, acq.rep, x[None]))
    assert info["value"] == acq(x[None])[0] == near.min()  # the own-cell moves are among the neighbours
    assert (info["final_values"] <= info["start_values"]).all() and info["value"] == info["final_values"].min()
    grid = dr.grid_product(acq.off, acq.rep)
    assert info["value"] >= acq(grid).min()
    if len(grid) <= starts:  # fewer distinct rows than starts: every cell is an incumbent, so the global minimum is found
        assert len(info["start_values"]) == len(grid) and info["value"] == acq(grid).min()
    # the rounds only bound the memory
    x2, info2 = dr.search(acq, acq.rows(11), acq.off, acq.rep, n_candidates, 37, starts, 32)
    assert np.array_equal(x, x2) and np.array_equal(info["final_values"], info2["final_values"])


@pytest.mark.parametrize("cells,n_candidates,starts,round_size", [((7, 5, 9, 4, 6), 400, 4, 128), ((3, 2, 2), 300, 8, 37),
                                                                  ((40, 30, 20, 10), 64, 3, 64), ((6, 6), 50, 5, 7)])
def test_product_search_loop_equals_the_reference_loop(cells, n_candidates, starts, round_size):
    """`local_search` is torch plumbing that runs on any device: on host tensors, with the reference's generators and the
    synthetic acquisition, it must take the reference loop's every decision (ties included)."""
    import torch

    acq = Synthetic(cells, seed=sum(cells))
    want_x, want = dr.search(acq, acq.rows(3), acq.off, acq.rep, n_candidates, round_size, starts, 32)
    calls = acq.calls
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    got_x, got = dom.local_search(lambda rows: t(acq(rows.numpy())), lambda first, n: t(acq.rows(3)(first, n)),
                                  lambda x: t(dr.neighbours(acq.off, acq.rep, x.numpy())), n_candidates, round_size, starts, 32)
    assert np.array_equal(got_x, want_x) and got["value"] == want["value"] and got["sweeps"] == want["sweeps"]
    assert np.array_equal(got["start_values"], want["start_values"]) and np.array_equal(got["final_values"], want["final_values"])
    assert got["scans"] == acq.calls - calls == -(-n_candidates // round_size) + got["sweeps"]
