"""What the sampler's device paths share (csrc/sampler_step.h), checked on the host: the Metropolis decision through the test hook
bark_debug_metropolis, and the step table of the two one-launch sweeps through the exported builders — its words, and the status
and text of every refusal of a step's pack.  The texts are the ones the builders had before they shared their checks.  No GPU."""
import ctypes
import itertools
import math

import numpy as np
import pytest

INF, NAN = math.inf, math.nan
USE_OTHER = "; use bark_tree_sweep_chains_hip (the multi-launch sweep) for this shape"


@pytest.fixture(scope="module")
def L():
    from bark_amd import _lib

    _lib.lib()
    return _lib


@pytest.fixture(autouse=True)
def leave_no_error_behind(L):
    """The refusals provoked here set the thread's last-error message; a successful query clears it for whatever test runs next."""
    yield
    v = ctypes.c_int(0)
    assert L.lib().bark_tree_sweep_resident_query(128, 6, 4, 0, ctypes.byref(v), None, None) == L.BARK_OK
    assert L.lib().bark_last_error() == b""


def reference_rule(log_u, log_q_prior, delta):
    """bark_sampler.py:259 — Python's own min, arguments in this order: min(nan, 0) is nan, and nothing is <= nan."""
    return int(log_u <= min(log_q_prior + delta, 0))


def test_metropolis_rule_over_the_special_values(L):
    decide = L.lib().bark_debug_metropolis
    log_us = (-INF, -1.0, -0.0, 0.0, 5e-324, 1.0, INF, NAN)
    others = (-INF, -1.0, 0.0, 1.0, INF, NAN)
    seen = set()
    for log_u, log_q, delta in itertools.product(log_us, others, others):
        want = reference_rule(log_u, log_q, delta)
        assert decide(log_u, log_q, delta) == want, (log_u, log_q, delta)
        seen.add(want)
    assert seen == {0, 1}
    # what the GPU test of the five paths relies on, for any finite delta
    for delta in (-3.5, 0.0, 2.25):
        assert [decide(math.log(0.5), NAN, delta), decide(0.0, INF, delta), decide(5e-324, INF, delta), decide(-1.0, -INF, delta)] == [0, 1, 0, 0]


def test_metropolis_rule_on_the_boundary(L):
    decide = L.lib().bark_debug_metropolis
    for log_q, delta in ((-0.5, -0.25), (-3.0, 1.5), (0.25, -0.25), (1e-300, -1e-300), (-1.0, 1.0), (0.5, 0.25), (-0.1, 0.3)):
        log_u = log_q + delta  # exactly log_alpha, as the library forms it
        want = 1 if log_u <= 0.0 else 0
        assert decide(log_u, log_q, delta) == want == reference_rule(log_u, log_q, delta), (log_q, delta)
        above, below = float(np.nextafter(log_u, INF)), float(np.nextafter(log_u, -INF))
        assert decide(above, log_q, delta) == 0 and decide(below, log_q, delta) == (1 if below <= 0.0 else 0)


# ---- the step table: 3 steps, 2 chains -------------------------------------------------------------------------------------
STEPS, NC = 3, 2
OFFSETS = np.array([0, 256, 2304], dtype=np.int64)
PACKS = [(5, 2, 6), (31, 8, 16), (1, 0, 2)]  # per step: packed nodes per tree, max depth, max_bits
R_OLD = np.array([[3, 1], [15, 8], [1, 1]], dtype=np.int64)
TREE_INDEX = np.array([0, 1, 0], dtype=np.int64)
R_NEW = np.array([[4, 2], [3, 4], [1, 1]], dtype=np.int64)
NLEAVES = np.array([[2, 3], [1, 4]], dtype=np.int32)  # (chains, trees)
M_TREES, LCAP, RCAP = 2, 4, 8


def _infos(L, trees, **patch):
    """The packs of the three steps, `trees` trees per chain in each; patch: field=(step, value)."""
    infos = (L.PackInfo * STEPS)()
    for t, (stride, depth, bits) in enumerate(PACKS):
        infos[t].B, infos[t].m, infos[t].L, infos[t].stride = NC, trees, 100, stride
        infos[t].max_leaves, infos[t].max_depth, infos[t].packed_bytes, infos[t].max_bits = bits, depth, NC * trees * stride * 16, bits
    for field, (t, value) in patch.items():
        setattr(infos[t], field, value)
    return infos


def _resident(L, infos=None, offsets=OFFSETS, r_old=R_OLD, nc=NC):
    infos = _infos(L, 2) if infos is None else infos
    table = np.full(STEPS * (4 + 65), -7, dtype=np.int64)
    rc = L.lib().bark_tree_sweep_resident_table(L.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), L.ptr(r_old), STEPS, nc, L.ptr(table))
    return rc, table, L.lib().bark_last_error().decode()


def _leafchain(L, infos=None, offsets=OFFSETS, r_new=R_NEW, nc=NC):
    infos = _infos(L, 1) if infos is None else infos
    table = np.full(STEPS * (4 + 65), -7, dtype=np.int64)
    rc = L.lib().bark_leafchain_sweep_table(L.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), L.ptr(TREE_INDEX), L.ptr(r_new), L.ptr(NLEAVES),
                                            STEPS, nc, M_TREES, LCAP, RCAP, L.ptr(table))
    return rc, table, L.lib().bark_last_error().decode()


def test_both_builders_write_the_same_layout(L):
    lib = L.lib()
    words = STEPS * (4 + NC)
    assert lib.bark_tree_sweep_resident_table_bytes(STEPS, NC) == lib.bark_leafchain_sweep_table_bytes(STEPS, NC) == 8 * words
    for build, word3, column in ((_resident, [bits for _, _, bits in PACKS], R_OLD), (_leafchain, TREE_INDEX.tolist(), R_NEW)):
        rc, table, msg = build(L)
        assert rc == L.BARK_OK and msg == ""
        want = [[int(OFFSETS[t]), PACKS[t][0], PACKS[t][1], word3[t]] for t in range(STEPS)]
        assert table[:4 * STEPS].reshape(STEPS, 4).tolist() == want
        assert np.array_equal(table[4 * STEPS:words].reshape(STEPS, NC), column)
        assert (table[words:] == -7).all()  # nothing past the table


def _col(a, t, b, value):
    out = a.copy()
    out[t, b] = value
    return out


def _off(t, value):
    out = OFFSETS.copy()
    out[t] = value
    return out


def test_resident_builder_refusals_keep_their_texts(L):
    pack = "pack one [old, new] pair per chain (B = chains, m = 2)"
    cases = [
        (dict(infos=_infos(L, 2, B=(1, 3))), f"step 1: {pack}"),
        (dict(infos=_infos(L, 2, m=(2, 1))), f"step 2: {pack}"),
        (dict(infos=_infos(L, 2, stride=(0, 0))), "step 0: bad offset, stride or depth"),
        (dict(infos=_infos(L, 2, stride=(0, 65))), "one-launch sweep, step 0: 65 packed nodes in a tree, at most 64 fit LDS" + USE_OTHER),
        (dict(offsets=_off(1, 264)), "step 1: bad offset, stride or depth"),
        (dict(offsets=_off(2, -16)), "step 2: bad offset, stride or depth"),
        (dict(infos=_infos(L, 2, max_depth=(1, -1))), "step 1: bad offset, stride or depth"),
        (dict(infos=_infos(L, 2, max_depth=(1, (1 << 24) + 1))), "step 1: bad offset, stride or depth"),
        (dict(r_old=_col(R_OLD, 0, 1, 0)), "step 0 chain 1: r_old = 0 is not inside (0, 6)"),
        (dict(r_old=_col(R_OLD, 1, 0, 16)), "step 1 chain 0: r_old = 16 is not inside (0, 16)"),
        (dict(nc=0), "one-launch sweep: 0 chains are outside 1..64" + USE_OTHER),
        (dict(nc=65), "one-launch sweep: 65 chains are outside 1..64" + USE_OTHER),
    ]
    for kwargs, text in cases:
        rc, table, msg = _resident(L, **kwargs)
        assert rc == L.BARK_ERR_ARG and msg == text, (text, msg)
        assert (table == -7).all()  # a refusal writes nothing
    assert _resident(L, infos=_infos(L, 2, stride=(0, 64), max_depth=(1, 1 << 24)))[0] == L.BARK_OK  # the edges themselves pass


def test_leafchain_builder_refusals_keep_their_texts(L):
    pack = "pack one new tree per chain (B = chains, m = 1)"
    cases = [
        (dict(infos=_infos(L, 1, B=(1, 3))), f"step 1: {pack}"),
        (dict(infos=_infos(L, 1, m=(2, 2))), f"step 2: {pack}"),
        (dict(infos=_infos(L, 1, stride=(0, 0))), "leaf-space chains, step 0: 0 packed nodes in a tree, at most 64"),
        (dict(infos=_infos(L, 1, stride=(0, 65))), "leaf-space chains, step 0: 65 packed nodes in a tree, at most 64"),
        (dict(offsets=_off(1, 264)), "step 1: bad offset or depth"),
        (dict(offsets=_off(2, -16)), "step 2: bad offset or depth"),
        (dict(infos=_infos(L, 1, max_depth=(1, -1))), "step 1: bad offset or depth"),
        (dict(infos=_infos(L, 1, max_depth=(1, (1 << 24) + 1))), "step 1: bad offset or depth"),
        (dict(r_new=_col(R_NEW, 0, 1, 0)), "leaf-space chains, step 0 chain 1: a new tree of 0 leaves, at most 4 fit"),
        (dict(r_new=_col(R_NEW, 1, 0, 5)), "leaf-space chains, step 1 chain 0: a new tree of 5 leaves, at most 4 fit"),
        (dict(nc=0), "leaf-space chains: 0 chains are outside 1..64"),
        (dict(nc=65), "leaf-space chains: 65 chains are outside 1..64"),
    ]
    for kwargs, text in cases:
        rc, table, msg = _leafchain(L, **kwargs)
        assert rc == L.BARK_ERR_ARG and msg == text, (text, msg)
        assert (table == -7).all()
    assert _leafchain(L, infos=_infos(L, 1, stride=(0, 64), max_depth=(1, 1 << 24)))[0] == L.BARK_OK


def test_leafchain_plan_reports_the_shared_chain_limit(L):
    from bark_amd.fitting import leafchain_plan

    assert leafchain_plan(128, 64, 4, 8)["max_chains"] == 64
    assert L.lib().bark_tree_swap_chains_workspace_bytes(128, 4, 64, None) > 0 and L.lib().bark_tree_swap_chains_workspace_bytes(128, 4, 65, None) == 0
