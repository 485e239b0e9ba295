"""The host side of tests/test_gpu_sweep_info.py (tests/info_ref.py), without a GPU: the placed pivot against a plain unblocked
elimination, the margin condition of every placed pivot, and the assignment of bad matrices to every row of sweep_ref.CASES —
every class the row's N allows, a healthy matrix in every chunk, the caps per call — and the leaf-space positions.
(Every row's calls are printed: run with -s to see them.)"""
import numpy as np
import pytest

import info_ref as ir
import sweep_ref as sr

NAMES = list(sr.CASES)
SMALL_N = 900  # up to here every placed pivot is compared with the unblocked elimination; beyond, two per row


class _Plans(dict):
    def __missing__(self, name):
        inp = sr.make_inputs(sr.CASES[name])
        self[name] = inp, ir.plan_row(inp)
        return self[name]


PLANS = _Plans()


def test_class_positions():
    cp = ir.class_positions
    assert cp(1) == {"p1": [1]}
    assert list(cp(100)) == ["p1", "group", "p17", "pN", "noise"] and cp(100)["pN"] == [100]
    assert list(cp(128)) == ["p1", "group", "p17", "p128", "noise"]  # pivot N is p128
    assert list(cp(129)) == ["p1", "group", "p17", "p128", "p129", "noise"]  # pivot N and the last block's first are p129
    assert list(cp(200)) == ["p1", "group", "p17", "p128", "p129", "pN", "noise"]
    full = cp(700)
    assert list(full) == list(ir.CLASSES)
    assert full["last_first"] == [641] and full["pN"] == [700] and all(257 <= p <= 384 for p in full["middle"])
    assert cp(769)["last_first"] == [769] and "pN" not in cp(769)  # the last block step has one pivot
    assert set(cp(2100)["middle"]) == set(range(8 * 128 + 1, 9 * 128 + 1)) and cp(2100)["last_first"] == [2049]
    assert all(5 <= p <= 16 for p in full["group"]) and full["group"][0] == 10
    assert cp(7)["group"][0] == 7


def test_elimination_and_closed_form_on_a_small_matrix():
    rng = np.random.default_rng(5)
    Z = rng.integers(0, 4, size=(40, 12))
    K = (Z[:, None, :] == Z[None, :, :]).mean(axis=2)
    scale, s2 = 1.3, 1e-6 + 0.07
    dA, q = ir._running_q(ir._a_matrix(K, scale, s2))
    assert np.allclose(dA, ir.eliminate(ir._a_matrix(K, scale, s2))[0], rtol=1e-12)
    for p in (1, 2, 5, 16, 17, 39, 40):
        shift, piv = ir.place_pivot(K, scale, s2, p)
        K_s = ir._form(K, shift, scale, s2)
        got, bad = ir.eliminate(K_s)
        assert bad == [p] and ir.first_bad_pivot(K_s) == p
        assert np.allclose(got, piv, rtol=1e-9, atol=1e-12) and np.allclose(piv, ir.predicted_pivots(dA, q, p), rtol=1e-8, atol=1e-11)
        assert np.isclose(piv[-1], -dA[p - 1], rtol=1e-9)
    assert ir.first_bad_pivot(ir._a_matrix(K, scale, s2)) == 0
    # replace=True goes on behind a bad pivot with 1.0 in its place
    piv, bad = ir.eliminate(np.array([[-2.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, -1.0]]), replace=True)
    assert bad == [1, 3] and np.allclose(piv, [-2.0, 2.0, -1.0])


@pytest.mark.parametrize("name", NAMES)
def test_row_assignment(name):
    inp, plan = PLANS[name]
    case = inp.case
    print(name, [[(h.b, h.cls, h.p) for h in c.bad] for c in plan.calls])
    assert plan.classes == ir.class_positions(case.N) and not plan.unassigned
    used = [h.cls for c in plan.calls for h in c.bad]
    assert sorted(used) == sorted(plan.classes)  # every class the row's N allows, once
    if name == "one_n1":
        assert used == ["p1"]
    cap = 6 if case.N > 1500 else 9
    first = middle = last = adjacent = False
    for c in plan.calls:
        assert 1 <= len(c.bad) <= cap
        bad = {h.b for h in c.bad}
        assert len(bad) == len(c.bad)
        for c0, n in ir.chunks_of(case):
            inside = {b - c0 for b in bad if c0 <= b < c0 + n}
            assert len(inside) < n, (name, c0)  # a healthy matrix in every chunk
            first |= 0 in inside
            last |= n - 1 in inside
            middle |= n // 2 in inside
            adjacent |= any(b + 1 in inside for b in inside)
        # the call's vectors: the row's own values except at the bad matrices
        keep = np.array([b not in bad for b in range(case.B)])
        assert np.array_equal(c.noise[keep], inp.noise[keep]) and np.array_equal(c.shift[keep], inp.shift[keep])
        assert not c.info[keep].any() and np.array_equal(c.healthy, np.flatnonzero(keep))
        for h in c.bad:
            assert (c.noise[h.b], c.shift[h.b], c.info[h.b]) == (h.noise, h.shift, h.p)
            assert h.p in plan.classes[h.cls] and 1 <= h.p <= case.N
            assert ir.margin_ok(h.pivots) and len(h.pivots) == (1 if h.cls == "noise" else h.p)
            assert (h.noise == ir.BAD_NOISE) == (h.cls == "noise") and (h.cls == "noise" or h.noise == inp.noise[h.b])
    n_max = max(n for _, n in ir.chunks_of(case))
    n_bad = sum(len(c.bad) for c in plan.calls)
    if n_bad >= 4 and n_max >= 4:  # the first, the middle and the last matrix of a chunk, and two adjacent ones
        assert first and middle and last and adjacent, (name, first, middle, last, adjacent)


@pytest.mark.parametrize("name", NAMES)
def test_placed_pivots_against_the_unblocked_elimination(name):
    """Every placed pivot of the rows up to N = 900, two of every larger row: the unblocked elimination of the K_s that the
    kernel is given stops at the same pivot, with the same pivots.  The matrix with the negative diagonal fails at pivot 1 and,
    with 1.0 in the place of every bad pivot, again in a later block step (a later 16 x 16 sub-block where N <= 128)."""
    inp, plan = PLANS[name]
    case = inp.case
    hits = [h for c in plan.calls for h in c.bad]
    placed = [h for h in hits if h.cls != "noise"]
    if case.N > SMALL_N:
        placed = sorted(placed, key=lambda h: h.p)[1:3]  # (p = 1 needs no elimination)
        assert len(placed) == 2
    for h in placed:
        K_s = ir.bad_matrix(inp, h)[:h.p, :h.p]  # the elimination up to pivot p reads nothing else
        piv, bad = ir.eliminate(K_s)
        assert bad == [h.p], (name, h.cls, h.p, bad)
        assert np.allclose(piv, h.pivots, rtol=1e-7, atol=1e-10), (name, h.cls, float(np.abs(piv - h.pivots).max()))
    for h in hits:
        if h.cls == "noise":
            K_s = ir.bad_matrix(inp, h)
            n = case.N if case.N <= SMALL_N else 2 * ir.NB  # two block steps of the larger rows
            piv, bad = ir.eliminate(K_s[:n, :n], replace=True)
            assert bad[0] == 1 and piv[0] == h.pivots[0] < ir.FAIL_MAX
            unit = ir.NB if case.N > ir.NB else ir.SB
            assert any((b - 1) // unit > 0 for b in bad[1:]), (name, bad[:8])


def test_leafspace_positions():
    """A negative scale puts the first non-positive pivot of M = I + c Z'Z in the first 128 leaves, in the second block and past
    256 leaves, with the margin condition met; the unblocked elimination of M agrees."""
    import leafspace_ref as lr

    seen = set()
    for plan in ir.leaf_plans():
        inp = plan.inp
        lr.check_shape(inp)
        assert not plan.missing and 5 <= inp.case.B <= 8
        bad = sorted(plan.placed)
        assert bad[0] == 0 and bad[-1] == inp.case.B - 1 and any(b + 1 in plan.placed for b in bad) and len(plan.healthy) >= 2
        for b, (rng, k, c, piv) in plan.placed.items():
            lo, hi = ir.LEAF_RANGES[rng]
            assert lo < k <= (hi or inp.R) and plan.info[b] == k and ir.margin_ok(piv) and c < 0
            assert np.isclose(plan.scale[b], c * inp.m * (1e-6 + inp.noise[b])) and plan.scale[b] < 0
            M = np.eye(inp.R) + c * (inp.Z[b].T @ inp.Z[b])
            got, where = ir.eliminate(M)
            assert where == [k] and np.allclose(got, piv, rtol=1e-9, atol=1e-12)
            seen.add("past256" if rng == "inner" else rng)
        keep = plan.healthy
        assert np.array_equal(plan.scale[keep], inp.scale[keep]) and (plan.scale[keep] > 0).all()
    assert seen == {"first", "second", "past256"}
