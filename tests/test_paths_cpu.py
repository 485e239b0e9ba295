"""Host side of the sample paths (include/bark_hip.h, "Sample paths from a fitted posterior"): the Philox restatement of the
normals, the path list, the plan and workspace queries with every refused shape, and the reference's own identity.  No GPU."""
import ctypes

import numpy as np
import pytest

from bark_amd import _lib, synthetic
from bark_amd.fitting import _philox
from bark_amd.tree_kernels import path_list, paths_plan

import paths_ref
from leafspace_ref import LeafRef, leaf_matrix, host_pack, leaf_bit_table


def test_philox_known_answers_and_the_normals_addressing():
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        assert tuple(int(v) for v in _philox.philox4x32(key, ctr)) == want
    seed, R = 0x1234567890ABCDEF, 7
    z = _philox.path_normals(seed, [2, 0, 2], [0, 0, 1], R)
    assert z.shape == (3, R) and np.isfinite(z).all() and (np.abs(z) < 9).all()
    # entry a of path (b, s) from the words of counter (b, s, a // 2, 0) under the key (low, high ^ "path"), by hand
    key = (seed & 0xFFFFFFFF, (seed >> 32) ^ 0x70617468)
    for p, (b, s) in enumerate([(2, 0), (0, 0), (2, 1)]):
        for a in range(R):
            w = [int(v) for v in _philox.philox4x32(key, (b, s, a // 2, 0))]
            u1, u2 = ((w[0] | w[1] << 32) >> 11) * 2.0 ** -53, ((w[2] | w[3] << 32) >> 11) * 2.0 ** -53
            r, th = np.sqrt(-2.0 * np.log(1.0 - u1)), 6.283185307179586 * u2
            assert z[p, a] == (r * np.cos(th) if a % 2 == 0 else r * np.sin(th))
    # a row is a function of (seed, b, s): not of the other rows, their order or R's parity
    assert np.array_equal(_philox.path_normals(seed, [2], [1], R)[0], z[2])
    assert np.array_equal(_philox.path_normals(seed, [2], [1], R + 1)[0, :R], z[2])
    assert not np.array_equal(_philox.path_normals(seed + 1, [2], [1], R)[0], z[2])
    assert not np.array_equal(z[0], z[2]) and not np.array_equal(z[0], z[1])
    big = _philox.path_normals(5, np.zeros(64, dtype=int), np.arange(64), 512)  # 32768 normals: mean and variance
    assert abs(big.mean()) < 0.03 and abs(big.var() - 1.0) < 0.03


def test_path_list_draw_numbers_and_order():
    forest, draw, order = path_list(None, 3, 2)
    assert forest.tolist() == [0, 0, 1, 1, 2, 2] and draw.tolist() == [0, 1, 0, 1, 0, 1] and order.tolist() == list(range(6))
    forest, draw, order = path_list([2, 0, 2, 1, 2, 0], 3)
    assert forest.dtype == np.int32 and draw.dtype == np.int32 and order.dtype == np.int64
    assert draw.tolist() == [0, 0, 1, 0, 2, 1]  # the count of earlier entries naming the same forest
    assert forest[order].tolist() == [0, 0, 1, 2, 2, 2] and order.tolist() == [1, 5, 3, 0, 2, 4]  # stable
    # the caller's order comes back: row j of the device's result is path order[j]
    result = np.stack([forest[order], draw[order]], axis=1)
    back = np.empty_like(result)
    back[order] = result
    assert back[:, 0].tolist() == forest.tolist() and back[:, 1].tolist() == draw.tolist()
    assert path_list([1], 3)[1].tolist() == [0]
    for bad in ([], [3], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            path_list(bad, 3)
    with pytest.raises(ValueError):
        path_list(None, 3, 0)


def test_plan_and_workspace_queries_and_refusals():
    lib = _lib.lib()
    assert paths_plan(1, 1) == {"route": "blocked", "max_leaves": 2048} == paths_plan(2048, 64)
    for R, m in ((0, 5), (2049, 5), (8192, 5), (100, 0), (100, 65)):
        with pytest.raises(ValueError, match="at most 64 trees and 2048 leaves"):
            paths_plan(R, m)
        route, limit = ctypes.c_int(-1), ctypes.c_int64(-1)
        assert lib.bark_leaf_posterior_paths_plan(R, m, ctypes.byref(route), ctypes.byref(limit)) == _lib.BARK_ERR_ARG
        assert (route.value, limit.value) == (1, 2048)  # the answer is given either way, the shape is refused
        assert lib.bark_leaf_posterior_paths_workspace_bytes(R, m, 3, 6, 1) == 0
        assert lib.bark_path_scan_workspace_bytes(R, m, 6, 100, 2) == 0
    assert lib.bark_leaf_posterior_paths_plan(100, 5, None, None) == 0
    a = lambda n: (n + 255) & ~255  # noqa: E731
    R, m, B = 100, 5, 3
    # run table (3 P + 1 ints), min(P, B) factors, the normals when the call draws them
    assert lib.bark_leaf_posterior_paths_workspace_bytes(R, m, B, 6, 0) == a(4 * 19) + a(8 * 3 * R * R)
    assert lib.bark_leaf_posterior_paths_workspace_bytes(R, m, B, 6, 1) == a(4 * 19) + a(8 * 3 * R * R) + a(8 * 6 * R)
    assert lib.bark_leaf_posterior_paths_workspace_bytes(R, m, B, 2, 0) == a(4 * 7) + a(8 * 2 * R * R)
    # R = 2048: 256 MiB hold 8 factors however many forests occur
    assert lib.bark_leaf_posterior_paths_workspace_bytes(2048, m, 64, 4096, 0) == a(4 * (3 * 4096 + 1)) + 8 * (8 * 2048 * 2048)
    for B_, P in ((0, 6), (3, 0), (3, 4097), (3, -1)):
        assert lib.bark_leaf_posterior_paths_workspace_bytes(R, m, B_, P, 0) == 0
    # scan: run table (2 P + 1 ints), a flag, the codes of one slab for min(16, 64 MiB / codes) forests, the partials
    W = 4
    for C, cpad in ((1, 128), (65535, 65536), (65536, 65536), (65537, 65536)):
        codes = a(4 * 16 * W * cpad)
        assert lib.bark_path_scan_workspace_bytes(R, m, 6, C, 0) == a(4 * 13) + 256 + codes
        nblk = -(-C // 256)
        for reduce in (1, 2):
            assert lib.bark_path_scan_workspace_bytes(R, m, 6, C, reduce) == a(4 * 13) + 256 + codes + 2 * a(8 * nblk * 6)
    assert lib.bark_path_scan_workspace_bytes(2048, m, 1, 65536, 0) == 256 + 256 + 4 * 4 * 64 * 65536  # 4 forests per walk
    for P, C in ((0, 10), (4097, 10), (6, 0), (6, (1 << 24) + 1)):
        assert lib.bark_path_scan_workspace_bytes(R, m, P, C, 0) == 0
    assert lib.bark_path_scan_workspace_bytes(R, m, 4096, 1 << 24, 0) > 0
    assert lib.bark_last_error() == b"" or b"at most" in lib.bark_last_error()
    assert {"bark_leaf_posterior_paths_hip", "bark_path_scan_hip", "bark_leaf_posterior_paths_plan"} <= set(_lib.SIGNATURES)


def test_the_cuts_of_the_host_drivers_lie_where_the_gpu_tests_cross_them():
    """tests/test_gpu_paths_chunks.py picks its shapes to cross these three; read off the byte queries as it reads them."""
    lib = _lib.lib()
    # resident factors: floor(256 MiB / 8 R^2)
    assert paths_ref.resident_factors(lib, 2048, 64) == 8 and paths_ref.resident_factors(lib, 2048) == 8
    assert paths_ref.resident_factors(lib, 1449) == 15 and paths_ref.resident_factors(lib, 1448) == 16
    assert paths_ref.resident_factors(lib, 2047) == 8 and paths_ref.resident_factors(lib, 1931) == 8 and paths_ref.resident_factors(lib, 1930) == 9
    # forests per leaf walk: 16 while their codes of one slab fit 64 MiB
    for R, m, C in ((11, 3, 300), (11, 3, 1), (65, 33, 300), (385, 4, 65537), (2048, 64, 128), (2048, 64, 16384)):
        assert paths_ref.scan_walk(lib, R, m, C) == 16, (R, C)
    assert paths_ref.scan_walk(lib, 2048, 64, 16385) == 15 and paths_ref.scan_walk(lib, 2048, 64, 65536) == 4
    # the leaf-limit fixture: 9 forests of 2048 leaves are first cut at 64 MiB / (64 words x 4 bytes x 9) = 29 127.1 candidates
    C = paths_ref.smallest_candidates_below(lib, 2048, 64, 9)
    assert C == 29184 and paths_ref.scan_walk(lib, 2048, 64, C - 37) == 8 and paths_ref.scan_walk(lib, 2048, 64, C - 128) == 9
    # the leaf walks of a sorted list: cut at a missing forest and after `walk` consecutive ones
    full = list(range(17)) + [17] * 17 + [18]
    assert paths_ref.walk_chunks(full, 16) == [(0, 16), (16, 3)] and paths_ref.walk_chunks(full, 8) == [(0, 8), (8, 8), (16, 3)]
    assert paths_ref.walk_chunks(list(range(7)) + list(range(8, 19)), 16) == [(0, 7), (8, 11)]
    assert paths_ref.walk_chunks([17, 17, 18], 16) == [(17, 2)] and paths_ref.walk_chunks([3], 1) == [(3, 1)]
    assert paths_ref.walk_chunks(list(range(8)) + [8] * 17, 8) == [(0, 8), (8, 1)]
    assert paths_ref.call_splits(np.zeros(4096)) == [(0, 4096)] and paths_ref.call_splits(np.zeros(4100)) == [(0, 4096), (4096, 4)]
    assert paths_ref.MAX_PATHS == 4096
    from bark_amd.tree_kernels import posterior

    assert posterior.MAX_PATHS_PER_CALL == paths_ref.MAX_PATHS
    assert lib.bark_path_scan_workspace_bytes(11, 3, 4096, 64, 0) > 0 == lib.bark_path_scan_workspace_bytes(11, 3, 4097, 64, 0)


def test_path_list_across_the_split_at_4096():
    """The 4100-entry list of the GPU test: the draw number counts the earlier entries of the same forest in the caller's
    order whichever side of the split at 4096 they fall on, and `order` is the stable sort."""
    counts = (1500, 2598, 2)
    forests = np.random.default_rng(8).permutation(np.repeat(np.arange(3), counts))
    forest, draw, order = path_list(forests, 3)
    assert forest.tolist() == forests.tolist() and len(order) == 4100
    seen = [0, 0, 0]
    for i, b in enumerate(forests):  # by hand
        assert draw[i] == seen[b]
        seen[b] += 1
    assert tuple(seen) == counts
    srt = forest[order]
    assert (np.diff(srt) >= 0).all() and np.array_equal(order, np.argsort(forests, kind="stable"))
    for b in range(3):  # stable: inside a forest's run the caller's positions rise, so the draws are 0, 1, 2, ...
        run = order[srt == b]
        assert (np.diff(run) > 0).all() and draw[run].tolist() == list(range(counts[b]))
    # forest 1 straddles the split: the second call starts with its draws 2596 and 2597
    assert srt[4095] == srt[4096] == 1 and draw[order][4094:].tolist() == [2594, 2595, 2596, 2597, 0, 1]
    assert paths_ref.call_splits(srt) == [(0, 4096), (4096, 4)]


def test_the_walk_that_sets_the_fault_flag():
    """paths_ref.meets_invalid_categorical against the oracle's walk, which refuses the same rows as a whole."""
    from oracle import oracle as orc

    kw = dict(d_cont=2, n_int=1, n_cat=1)
    X, y, bounds, ft = synthetic.mixed_problem(24, seed=35, **kw)
    F = synthetic.sample_prior_forests(19, 3, bounds, ft, seed=36)
    cand = synthetic.mixed_problem(40, seed=36, **kw)[0]
    cat = int(np.flatnonzero(ft == 0)[0])
    met = 0
    for x in cand:
        assert not any(paths_ref.meets_invalid_categorical(F[b], ft, x) for b in range(19))
        for value in (-1.0, np.nan, np.inf, -0.5):
            bad = x.copy()
            bad[cat] = value
            for b in (0, 5, 17):
                meets = paths_ref.meets_invalid_categorical(F[b], ft, bad)
                if value == -0.5:  # truncates to -0.0: category 0, valid
                    assert not meets
                if value == -1.0:
                    met += meets
                    try:
                        leaves = orc.pass_through_forest(F[b], bad[None], ft)
                        refused = False
                    except ValueError:
                        refused = True
                    assert refused == meets
                    if not meets:  # the feature was never tested on the way down: the leaves are those of the valid row
                        assert np.array_equal(leaves, orc.pass_through_forest(F[b], x[None], ft))
    assert 0 < met < 3 * len(cand)


def test_reference_identity_on_the_test_inputs():
    """G G' = M^-1 for the restatement's factor, in float64 and in longdouble, on the shape of the GPU tests (B = 3, m = 5,
    N = 40, d = 4 with one categorical and one integer feature)."""
    kw = dict(d_cont=2, n_int=1, n_cat=1)
    X, y, bounds, ft = synthetic.mixed_problem(40, seed=31, **kw)
    F = synthetic.sample_prior_forests(3, 5, bounds, ft, seed=41)
    info, packed = host_pack(F, ft)
    R = int(info.max_bits)
    bits = leaf_bit_table(packed, F.shape[2], int(info.max_depth))
    noise, scale = np.array([0.05, 0.1, 0.2]), np.array([0.8, 1.0, 1.3])
    for b in range(3):
        ref = LeafRef(leaf_matrix(F[b], bits[b], X, ft, R), y, noise[b], scale[b], 5)
        Minv = np.linalg.inv(ref.L @ ref.L.T)
        Minv = 0.5 * (Minv + Minv.T)
        G = paths_ref.factor(Minv)
        assert np.array_equal(G, np.tril(G)) and (np.diag(G) > 0).all()
        np.testing.assert_allclose(G @ G.T, Minv, rtol=1e-13, atol=1e-14)
        Gl = paths_ref.factor(Minv, np.longdouble)
        np.testing.assert_allclose(G, Gl.astype(np.float64), rtol=1e-11, atol=1e-13)
        eps = np.random.default_rng(b).standard_normal((2, R))
        W = paths_ref.weights(Minv[None], ref.w[None], noise[b:b + 1], scale[b:b + 1], 5, [0, 0], eps)
        mean = scale[b] / (5 * (1e-6 + noise[b])) * ref.w
        np.testing.assert_allclose(W - mean, np.sqrt(scale[b] / 5) * eps @ G.T, rtol=1e-12, atol=1e-13)
    cols, R2 = paths_ref.leaf_columns(F, ft, X)
    assert R2 == R and cols.shape == (3, 40, 5) and (np.diff(cols, axis=2) > 0).all()  # tree order is column order
    Wt = np.arange(2 * R, dtype=np.float64).reshape(2, R)
    f = paths_ref.evaluate(Wt, [1, 2], cols)
    assert np.array_equal(f[0], cols[1].sum(axis=1)) and np.array_equal(f[1], cols[2].sum(axis=1) + 5 * R)
    v, i = paths_ref.first_argmin(np.array([[3.0, 1.0, 1.0], [2.0, 2.0, 0.5]]))
    assert v.tolist() == [1.0, 0.5] and i.tolist() == [1, 2]
