"""Sample paths across every cut of their host drivers (bark_leaf_posterior_paths_hip, bark_path_scan_hip, and the Python
slicing of LeafPosterior.sample_paths / LeafPaths).  tests/test_gpu_paths.py holds the kernels to their tile edges with at
most 4 forests, 385 leaves and 18 paths, where every loop of the drivers takes one turn.  Here each loop takes a second one:

  forests per leaf walk    16 (PS_MAX_WALK), fewer when the codes of a slab pass 64 MiB       19 forests / R = 2048
  resident factors         256 MiB / 8 R^2                                                       9 forests at R = 2048
  paths per LDS round      48 KiB / 8 R, 3 at R = 2048 with the unit's largest dynamic LDS     17 paths at R = 2048
  paths per C call         4096, sliced in Python                                               4100 paths
  pivots                   a later panel, a later residency chunk, the last pivot of all        R = 65 and R = 2048

The references are those of tests/test_gpu_paths.py: numpy's Cholesky of the state read back (rtol 1e-9, atol 1e-8) for the
weights, the host loop in tree order (bit for bit) for the scans.  Where a cut lies is read off the library's byte queries
(paths_ref.resident_factors, paths_ref.scan_walk) and every test asserts that its path list crosses it."""
import ctypes
import time

import numpy as np
import pytest

from bark_amd import _lib as L
from bark_amd import synthetic
from bark_amd.fitting import _philox
from bark_amd.tree_kernels import path_list

import paths_ref
from leafspace_ref import build_forest
from test_gpu_paths import ATOL, DEEP, KW, RTOL, Fixture, host

pytestmark = pytest.mark.gpu

FULL, MAX, MIN = L.SAMPLE_FULL, L.SAMPLE_MAX, L.SAMPLE_MIN


# ---- the two C entry points themselves, on a sorted path list ----
def c_paths(post, pf, pd, seed=0, eps=None):
    """bark_leaf_posterior_paths_hip -> (W (P, R), info_out (B,)), numpy."""
    import torch

    lib = L.lib()
    pf, pd = np.ascontiguousarray(pf, dtype=np.int32), np.ascontiguousarray(pd, dtype=np.int32)
    P = int(pf.shape[0])
    W = torch.empty((P, post.R), dtype=torch.float64, device="cuda")
    info = torch.full((post.B,), -77, dtype=torch.int32, device="cuda")
    eps_d = None if eps is None else torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float64)).cuda()
    ws = L.workspace(int(lib.bark_leaf_posterior_paths_workspace_bytes(post.R, post.m, post.B, P, eps is None)))
    rc = lib.bark_leaf_posterior_paths_hip(L.ctx(), post.packed.info_ref, L.ptr(post.noise), L.ptr(post.scale), L.ptr(post.state),
                                           post.nbytes, L.ptr(pf), L.ptr(pd), P, L.ptr(eps_d), ctypes.c_uint64(seed), L.ptr(W),
                                           L.ptr(info), L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.bark_last_error()
    return host(W), host(info)


def c_scan(post, pf, W_sorted, cand, reduce=FULL):
    """bark_path_scan_hip -> (f (P, C) or (values (P,), indices (P,)), info_out (B,)), numpy."""
    import torch

    lib = L.lib()
    pf = np.ascontiguousarray(pf, dtype=np.int32)
    P, C = int(pf.shape[0]), int(cand.shape[0])
    Wd = torch.from_numpy(np.ascontiguousarray(W_sorted)).cuda()
    cd = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.float64)).cuda()
    full = reduce == FULL
    f = torch.empty((P, C), dtype=torch.float64, device="cuda") if full else None
    red = None if full else torch.empty(P, dtype=torch.float64, device="cuda")
    idx = None if full else torch.empty(P, dtype=torch.int64, device="cuda")
    info = torch.full((post.B,), -77, dtype=torch.int32, device="cuda")
    ws = L.workspace(int(lib.bark_path_scan_workspace_bytes(post.R, post.m, P, C, reduce)))
    rc = lib.bark_path_scan_hip(L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(pf), L.ptr(Wd), P, L.ptr(cd), C,
                                reduce, L.ptr(f), L.ptr(red), L.ptr(idx), L.ptr(info), L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.bark_last_error()
    return (host(f) if full else (host(red), host(idx))), host(info)


def check_scan(paths, cand, want):
    """evaluate and both directions of minimise against the host loop's values `want`, bit for bit."""
    np.testing.assert_array_equal(paths.evaluate(cand), want)
    for maximise in (False, True):
        v, i = paths.minimise(cand, maximise=maximise)
        wv, wi = paths_ref.first_argmin(want, maximise)
        np.testing.assert_array_equal(v, wv)
        np.testing.assert_array_equal(i, wi)


# ------------------------------------------------------------------ A. many forests, small R ----
NA, BA, MA, SEED_A = 24, 19, 3, 0x5EED0000A


class Many:
    """19 prior forests of 3 trees, N = 24, 300 candidates, and the call that names every forest in order: one path each,
    17 of forest 17.  The other tests of this section compare their subsets with this call bit for bit."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.X, self.y, self.bounds, self.ft = synthetic.mixed_problem(NA, seed=35, **KW)
        self.F = synthetic.sample_prior_forests(BA, MA, self.bounds, self.ft, seed=36)
        self.noise, self.scale = 0.05 + 0.01 * np.arange(BA), 0.7 + 0.05 * np.arange(BA)  # distinct: a wrong b shows in W
        self.post = fit_posterior((self.F, self.noise, self.scale), (self.X, self.y), self.ft)
        self.R = self.post.R
        self.Minv, self.w, _ = paths_ref.read_state(self.post.state.cpu().numpy(), BA, self.R)
        self.cand = synthetic.mixed_problem(300, seed=36, **KW)[0]
        self.cand[[7, 150, 299]] = self.cand[21]  # duplicated rows: ties
        self.cols = paths_ref.leaf_columns(self.F, self.ft, self.cand)[0]
        self.walk = paths_ref.scan_walk(L.lib(), self.R, MA, 300)
        self.forest = np.array(list(range(17)) + [17] * 17 + [18])  # sorted: the caller's order is the device's
        self.paths = self.post.sample_paths(forests=self.forest, seed=SEED_A)
        self.draw = self.paths.draw
        self.W, self.f = host(self.paths.W), self.paths.evaluate(self.cand)
        self.low, self.high = self.paths.minimise(self.cand), self.paths.minimise(self.cand, maximise=True)
        self.row = {(int(b), int(s)): p for p, (b, s) in enumerate(zip(self.forest, self.draw))}

    def same_bits_as_the_full_call(self, forests):
        """A call for `forests` (caller's order) gives, per (forest, draw), the rows of the call that names all 19."""
        paths = self.post.sample_paths(forests=forests, seed=SEED_A)
        at = [self.row[(int(b), int(s))] for b, s in zip(paths.forest, paths.draw)]
        assert np.array_equal(host(paths.W), self.W[at])
        assert np.array_equal(paths.evaluate(self.cand), self.f[at])
        for maximise, (wv, wi) in ((False, self.low), (True, self.high)):
            v, i = paths.minimise(self.cand, maximise=maximise)
            assert np.array_equal(v, wv[at]) and np.array_equal(i, wi[at])


@pytest.fixture(scope="module")
def many():
    return Many()


def test_nineteen_forests_take_two_leaf_walks(many):
    """Cut: 16 forests per leaf walk (scan_walk = PS_MAX_WALK).  The runs 0..18 are consecutive, so only `n < walk` ends the
    first chunk: walks of forests 0..15 and 16..18, the second with b_lo = 16, an offset of 16 forests into `packed`, sub.B = 3
    and run table entries from r0 = 16 on; forest 17's 17 paths take two LDS rounds in the second chunk.  run_of searches 19
    runs in the weights, the normals and the status kernel."""
    assert many.walk == 16 and paths_ref.walk_chunks(many.forest, many.walk) == [(0, 16), (16, 3)]
    assert many.draw.tolist() == [0] * 17 + list(range(17)) + [0]
    eps = _philox.path_normals(SEED_A, many.forest, many.draw, many.R)
    want = paths_ref.weights(many.Minv, many.w, many.noise, many.scale, MA, many.forest, eps)
    np.testing.assert_allclose(many.W, want, rtol=RTOL, atol=ATOL)
    f = paths_ref.evaluate(many.W, many.forest, many.cols)
    np.testing.assert_array_equal(many.f, f)
    assert np.array_equal(f[:, 7], f[:, 21]) and np.array_equal(f[:, 299], f[:, 21])
    for maximise, (v, i) in ((False, many.low), (True, many.high)):
        wv, wi = paths_ref.first_argmin(f, maximise)
        np.testing.assert_array_equal(v, wv)
        np.testing.assert_array_equal(i, wi)


def test_normals_of_the_forests_past_sixteen(many):
    """Cut: none of the normals' own, but their counter takes b = run_b[run_of(p)] and no test had a forest above 3 or more
    than 3 runs.  With M^-1 = I, w = 0 and scale = m the weights are the normals (test_gpu_paths.test_normals)."""
    import torch

    R = many.R
    unit = many.post._copy()
    unit.state[:8 * BA * R * R].view(torch.float64).copy_(torch.eye(R, dtype=torch.float64).repeat(BA, 1).reshape(-1))
    at = paths_ref.align256(8 * BA * R * R)
    unit.state[at:at + 8 * BA * R].zero_()
    unit.scale = torch.full((BA,), float(MA), dtype=torch.float64, device="cuda")
    assert (many.forest >= 16).sum() == 19
    W = host(unit.sample_paths(forests=many.forest, seed=SEED_A).W)
    want = _philox.path_normals(SEED_A, many.forest, many.draw, R)
    assert (np.abs(want) < 9).all()
    np.testing.assert_allclose(W, want, rtol=0, atol=1e-12)
    late = [16, 18, 17, 17]  # alone and out of order: (16, 0) (18, 0) (17, 0) (17, 1)
    W = host(unit.sample_paths(forests=late, seed=SEED_A).W)
    np.testing.assert_allclose(W, _philox.path_normals(SEED_A, late, [0, 0, 0, 1], R), rtol=0, atol=1e-12)


def test_a_hole_in_the_list_and_a_callers_order(many):
    """Cut: the leaf walk's other end, `run_b[r0 + n] == run_b[r0] + n`.  Without forest 7 the walks are 0..6 and 8..18 (7 and
    11 forests, b_lo = 8, run index and forest index apart by one from there on).  The same list shuffled goes through
    `order`.  Both give the bits of the call that names all 19, per (forest, draw)."""
    hole = np.array(list(range(7)) + list(range(8, 19)) + [17])
    assert paths_ref.walk_chunks(np.sort(hole), many.walk) == [(0, 7), (8, 11)]
    many.same_bits_as_the_full_call(hole)
    shuffled = np.random.default_rng(5).permutation(hole)
    assert not np.array_equal(shuffled, np.sort(shuffled))
    many.same_bits_as_the_full_call(shuffled)


@pytest.mark.parametrize("forests", [[16, 17, 17, 18], [17, 18, 17], [18]])
def test_only_forests_past_sixteen(many, forests):
    """Cut: none is crossed, but the first walk starts at b_lo >= 16: the offset b_lo * m * stride * 16 into `packed` and
    the codes' (b - b_lo) with a first chunk that does not begin at forest 0."""
    chunks = paths_ref.walk_chunks(np.sort(forests), many.walk)
    assert len(chunks) == 1 and chunks[0][0] == min(forests) >= 16
    many.same_bits_as_the_full_call(np.array(forests))


def expected_info(sorted_forest, hit, walk, B):
    """info_out of bark_path_scan_hip when the walks of the forests `hit` (B,) bool set the fault flag."""
    info = np.zeros(B, dtype=np.int32)
    for b_lo, n in paths_ref.walk_chunks(sorted_forest, walk):
        if hit[b_lo:b_lo + n].any():
            info[b_lo:b_lo + n] = -1
    return info


def test_an_invalid_category_is_reported_by_the_walk_that_met_it(many):
    """Cut: 16 forests per leaf walk, and path_fault_take_kernel once per walk.

    What sets the flag, read in common.h (walk_tree): a tree's walk writes *fault = 1 when it COMES TO a categorical split
    whose feature value truncates to a negative or non-finite number, and goes right; a tree that never tests the feature on
    the row's way down sets nothing.  traverse.hip (walk_one_hot -> launch_walk<2>) runs one such walk per (forest of the
    chunk, candidate), all on the context's one flag.  paths.hip: after the slabs of a chunk, path_fault_take_kernel writes
    -1 to info_out of every run of THAT chunk if the flag is up, notes it in `seen` and takes the flag down, so the next
    chunk starts clean; forests outside the reporting chunks keep the 0 paths_info_kernel gave all B of them;
    path_fault_restore_kernel puts the flag back up at the end, for bark_ctx_status; path_status_kernel turns the FULL rows
    of reported forests into NaN.  paths_ref.meets_invalid_categorical restates the first part on the host.

    The row is chosen so that some forest of 0..15 meets the value and none of 16..18 does: the first walk reports for all
    of its 16 forests, also those that never saw the value, the second must not inherit the flag.  A second list of single
    forests far apart has a clean walk before and after the reporting one."""
    from bark_amd.fitting.mll import _clear_fault

    cat = int(np.flatnonzero(many.ft == 0)[0])
    hits = np.array([[paths_ref.meets_invalid_categorical(many.F[b], many.ft, np.r_[x[:cat], -1.0, x[cat + 1:]]) for b in range(BA)]
                     for x in many.cand])
    rows = np.flatnonzero(hits[:, :16].any(axis=1) & ~hits[:, 16:].any(axis=1))
    assert rows.size and not hits[rows[0], :16].all()
    bad = many.cand.copy()
    bad[rows[0], cat] = -1.0
    hit = hits[rows[0]]
    _clear_fault()
    a = int(np.flatnonzero(~hit)[0])
    h = int([b for b in np.flatnonzero(hit) if a + 1 < b < 17][0])
    apart = np.array([a, h, 18])  # a clean walk, the reporting one, a clean walk: single forests, no two adjacent
    assert paths_ref.walk_chunks(apart, many.walk) == [(a, 1), (h, 1), (18, 1)]
    for pf in (many.forest, apart):
        want = expected_info(pf, hit, many.walk, BA)
        named = np.unique(pf)
        assert (want[named] == -1).any() and (want[named] == 0).any() and not want[np.setdiff1d(np.arange(BA), named)].any()
        at = [many.row[(int(b), int(s))] for b, s in zip(pf, path_list(pf, BA)[1])]
        f, info = c_scan(many.post, pf, many.W[at], bad)
        assert info.tolist() == want.tolist()
        with pytest.raises(ValueError, match="categorical"):  # the flag is up again after the call (and read-and-reset here)
            L.check_categorical_fault()
        reported = want[pf] != 0
        assert np.isnan(f[reported]).all()
        # a forest of a clean walk never tested the feature on this row: its values are those at the valid row
        assert np.array_equal(f[~reported], many.f[at][~reported])
        (v, i), info = c_scan(many.post, pf, many.W[at], bad, MIN)
        assert info.tolist() == want.tolist()
        assert np.isnan(v[reported]).all() and (i[reported] == -1).all()
        assert np.array_equal(v[~reported], many.low[0][at][~reported]) and np.array_equal(i[~reported], many.low[1][at][~reported])
        _clear_fault()
        f, info = c_scan(many.post, pf, many.W[at], many.cand)
        assert not info.any() and np.array_equal(f, many.f[at])
        L.check_categorical_fault()  # nothing left behind


# ------------------------------------------------------------------ B. more than 4096 paths ----
COUNTS = (1500, 2598, 2)  # sorted: forest 1 holds paths 1500 .. 4097, so the cut at 4096 falls inside its run


@pytest.fixture(scope="module")
def small():
    return Fixture()


@pytest.mark.parametrize("given", [False, True], ids=["seeded", "eps"])
def test_4100_paths_in_two_calls(small, given):
    """Cut: 4096 paths per C call, in LeafPosterior.sample_paths and LeafPaths._scan.  4100 paths in a shuffled order whose
    sorted list has forest 1 on both sides of the cut: the second call factorises forest 1 again, numbers its draws from
    2596, and takes rows 4096.. of W, of the draw numbers and (given=True) of the caller's eps after `order`."""
    fx, S = small, 0xC0FFEE
    forests = np.random.default_rng(8).permutation(np.repeat(np.arange(3), COUNTS))
    forest, draw, order = path_list(forests, 3)
    srt = forest[order]
    assert paths_ref.call_splits(srt) == [(0, 4096), (4096, 4)] and srt[4095] == srt[4096] == 1
    assert draw[order][4096:].tolist() == [2596, 2597, 0, 1]
    eps = np.random.default_rng(9).standard_normal((4100, fx.R)) if given else None
    paths = fx.post.sample_paths(forests=forests, seed=S, eps=eps)
    assert paths.forest.tolist() == forest.tolist() and paths.draw.tolist() == draw.tolist()
    W = host(paths.W)
    normals = eps if given else _philox.path_normals(S, forest, draw, fx.R)
    np.testing.assert_allclose(W, fx.ref_weights(forest, normals), rtol=RTOL, atol=ATOL)
    # a path is a function of (seed, forest, draw) and the state (or of its eps row): the same one asked for alone
    at = [0, 1499, 1500, 1501, 4094, 4095, 4096, 4097, 4098, 4099] + np.random.default_rng(10).integers(0, 4100, 4).tolist()
    for j in order[at]:
        alone, info = c_paths(fx.post, [forest[j]], [draw[j]], seed=S, eps=eps[j:j + 1] if given else None)
        assert not info.any() and np.array_equal(alone[0], W[j]), (j, forest[j], draw[j])
    cand = fx.cand[:64].copy()
    cand[[3, 63]] = cand[40]
    cols = paths_ref.leaf_columns(fx.F, fx.ft, cand)[0]
    check_scan(paths, cand, paths_ref.evaluate(W, forest, cols))


# ------------------------------------------------------------------ C. the leaf limit ----
NC, BC, MC, RC = 40, 9, 64, 2048


class Limit:
    """9 forests of 64 complete trees of depth 5: m = 64 and R = 2048, both at the documented limit; one path of each of
    forests 0..7 and 17 of forest 8, from the caller's normals."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        t0 = time.perf_counter()
        self.X, self.y, self.bounds, self.ft = synthetic.mixed_problem(NC, seed=71)
        rng = np.random.default_rng(72)
        self.F = np.stack([build_forest((("full", MC, 5),), rng, self.bounds, self.ft) for _ in range(BC)])
        self.noise, self.scale = np.linspace(0.05, 0.3, BC), np.linspace(0.8, 1.4, BC)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.post = fit_posterior((self.F, self.noise, self.scale), (self.X, self.y), self.ft)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert self.post.R == RC and self.post.m == MC
        self.forest = np.array(list(range(8)) + [8] * 17)  # sorted
        self.draw = path_list(self.forest, BC)[1]
        self.eps = rng.standard_normal((25, RC))
        self.paths = self.post.sample_paths(forests=self.forest, eps=self.eps)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        self.W = host(self.paths.W)
        print(f"\nleaf-limit fixture: forests {t1 - t0:.2f} s, fit_posterior {t2 - t1:.2f} s, sample_paths (9 factors) {t3 - t2:.2f} s")


@pytest.fixture(scope="module")
def limit():
    return Limit()


def test_a_ninth_factor_at_2048_leaves(limit):
    """Cut: 8 resident factors at R = 2048 (256 MiB / 8 R^2).  Nine forests occur, so the factor / weights loop takes a second
    turn with r0 = 8: forest 8 is factorised alone into slot 0, its 17 paths start at p_lo = run_p0[8] = 8 and read rows
    (r - r0) R + a of that slot.

    The reference at this size, on the host alone (a state-like M^-1 built in numpy from the leaf membership of forests
    made like these, N = 40): the float64 weights of paths_ref.weights differ from its longdouble restatement by at most
    1.3e-16, 1.3e-8 of the tolerance, so numpy's own error is not what the tolerance is spent on."""
    lib = L.lib()
    resident = paths_ref.resident_factors(lib, RC, MC)
    runs = np.unique(limit.forest)
    assert resident == 8 and len(runs) == 9 > resident and np.searchsorted(limit.forest, runs[resident]) == 8
    assert np.isfinite(limit.W).all()
    Minv, w, info = paths_ref.read_state(limit.post.state.cpu().numpy(), BC, RC)
    assert not info.any()
    want = paths_ref.weights(Minv, w, limit.noise, limit.scale, MC, limit.forest, limit.eps)
    np.testing.assert_allclose(limit.W, want, rtol=RTOL, atol=ATOL)


def test_fewer_than_nine_forests_per_walk_at_2048_leaves(limit):
    """Cuts: the leaf walk cut by bytes (64 MiB of codes: 64 words per candidate at R = 2048), and 3 paths per LDS round
    (48 KiB / 8 R) with the launch's dynamic LDS at the unit's registered maximum, 82 944 bytes at m = 64.  The candidate
    count is the smallest whose padded slab leaves room for fewer than 9 forests, less 37 so that the last workgroup is
    ragged; forest 8 is then walked on its own (b_lo = 8) and its 17 paths take six LDS rounds.  The candidates are drawn
    from 300 distinct rows: ties everywhere, the lowest index wins."""
    lib = L.lib()
    C = paths_ref.smallest_candidates_below(lib, RC, MC, BC) - 37
    walk = paths_ref.scan_walk(lib, RC, MC, C)
    assert walk <= 8 and C < 65536 and len(paths_ref.walk_chunks(limit.forest, walk)) == 2
    assert paths_ref.walk_chunks(limit.forest, walk)[-1] == (8, 1) and (limit.forest == 8).sum() == 17 > 5 * 3
    rows = synthetic.mixed_problem(300, seed=73)[0]
    pick = np.random.default_rng(74).integers(0, 300, size=C)
    cols = paths_ref.leaf_columns(limit.F, limit.ft, rows)[0]
    want = paths_ref.evaluate(limit.W, limit.forest, cols)[:, pick]  # the host loop is per candidate: rows may be gathered after it
    check_scan(limit.paths, rows[pick], want)


def test_pivots_in_a_later_panel_and_a_later_residency_chunk(limit):
    """Cut: 8 resident factors, and the exits of paths_factor_kernel past its first panel.  Forest 8 (second residency
    chunk, block 0 of a launch with r0 = 8) has diagonal entry (40, 40) negated: `bad` is latched at c = 8 of the second
    panel, the break out of the i0 loop and then out of the j0 loop.  Forest 2 has (2047, 2047) negated: the last pivot of
    the last panel.  The C entry reports 41 and 2048; the paths of the two are NaN, all others keep their bits."""
    import torch

    broken = limit.post._copy()
    Mv = broken.state[:8 * BC * RC * RC].view(torch.float64).view(BC, RC, RC)
    assert float(Mv[8, 40, 40]) > 0 and float(Mv[2, 2047, 2047]) > 0
    Mv[8, 40, 40] = -Mv[8, 40, 40]
    Mv[2, 2047, 2047] = -Mv[2, 2047, 2047]
    assert paths_ref.resident_factors(L.lib(), RC, MC) == 8
    W, info = c_paths(broken, limit.forest, limit.draw, eps=limit.eps)
    assert info.tolist() == [0, 0, 2048, 0, 0, 0, 0, 0, 41]
    failed = np.isin(limit.forest, [2, 8])
    assert np.isnan(W[failed]).all() and np.array_equal(W[~failed], limit.W[~failed])


def test_pivots_of_the_second_and_third_panel():
    """Cut: the 32-column panels of paths_factor_kernel at R = 65 (DEEP of tests/test_gpu_paths.py): pivot 33 is the first of
    the second panel (`bad` latched at c = 0 with j0 = 32), pivot 65 the lone row of the third.  Forest 1 is left whole
    between them and keeps the bits of the call on the whole state."""
    import torch

    from bark_amd.tree_kernels import fit_posterior

    R = 65
    X, y, bounds, ft = synthetic.mixed_problem(40, seed=100 + R)
    rng = np.random.default_rng(R)
    F = np.stack([build_forest(DEEP[R], rng, bounds, ft) for _ in range(3)])
    post = fit_posterior((F, np.array([0.05, 0.1, 0.2]), np.array([0.9, 1.0, 1.2])), (X, y), ft)
    assert post.R == R
    pf, pd = [0, 1, 1, 2], [0, 0, 1, 0]
    good, info = c_paths(post, pf, pd, seed=6)
    assert not info.any() and np.isfinite(good).all()
    Mv = post.state[:8 * 3 * R * R].view(torch.float64).view(3, R, R)
    Mv[0, 32, 32] = -Mv[0, 32, 32]
    Mv[2, 64, 64] = -Mv[2, 64, 64]
    W, info = c_paths(post, pf, pd, seed=6)
    assert info.tolist() == [33, 0, 65]
    assert np.isnan(W[[0, 3]]).all() and np.array_equal(W[1:3], good[1:3])
