"""bark_leaf_codes_hip, bark_leaf_indices_hip, bark_gram_from_leaves_hip and bark_onehot_match_hip called through the C ABI, bit for
bit against the host reference of tests/frontend_ref.py (pinned by tests/test_frontend_reference_cpu.py) over every launch variant:
each row of frontend_ref.CASES asserts through bark_frontend_variant_query which kernel it reaches.

Canary rule: every output buffer is filled with a fixed non-zero pattern before each call and compared WHOLE afterwards — the
written block against the reference, every other element (row tails, gaps between batches, the element in front of an offset base,
the words behind the last plane) against the pattern.  Nothing here has a tolerance."""
import ctypes

import numpy as np
import pytest

import frontend_ref as fr
from bark_amd import _lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64  # canary elements behind every output


def _signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


def canary(n, dtype):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if dtype == "u32":
        return torch.full((n,), _signed(fr.CANARY32, 32), dtype=torch.int32, device=_lib.torch_device())
    return torch.full((n,), _signed(fr.CANARY64, 64), dtype=torch.int64, device=_lib.torch_device())


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint64)


def device(a):
    import torch

    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(_lib.torch_device())


def fault_flag():
    """bark_ctx_status: the categorical-fault flag of this thread's context, read and cleared"""
    flag = ctypes.c_int32(-1)
    _lib.check(_lib.lib().bark_ctx_status(_lib.ctx(), _lib.stream_ptr(), ctypes.byref(flag)))
    return flag.value


def run_codes(info, packed_d, X_d, expect_rc=0):
    """-> (rc, device buffer incl. guard, (B, W, npad))"""
    lib = _lib.lib()
    N, d = X_d.shape
    B, W, npad = int(info.B), int(lib.bark_leaf_words(ctypes.byref(info))), int(lib.bark_leaf_npad(N))
    buf = canary(B * W * npad + GUARD, "u32")
    rc = lib.bark_leaf_codes_hip(_lib.ctx(), _lib.ptr(packed_d), ctypes.byref(info), _lib.ptr(X_d), N, d, _lib.ptr(buf), _lib.stream_ptr())
    assert rc == expect_rc, (rc, lib.bark_last_error())
    return buf, (B, W, npad)


def run_indices(info, packed_d, X_d, expect_rc=0):
    lib = _lib.lib()
    N, d = X_d.shape
    B, m = int(info.B), int(info.m)
    buf = canary(B * N * m + GUARD, "u32")
    rc = lib.bark_leaf_indices_hip(_lib.ctx(), _lib.ptr(packed_d), ctypes.byref(info), _lib.ptr(X_d), N, d, _lib.ptr(buf), _lib.stream_ptr())
    assert rc == expect_rc, (rc, lib.bark_last_error())
    return buf, (B, N, m)


def split(buf, shape):
    """host copy of a canaried buffer -> (the output block, True if everything behind it still is the canary)"""
    h = host(buf)
    n = int(np.prod(shape))
    pattern = fr.CANARY32 if h.dtype == np.uint32 else fr.CANARY64
    return h[:n].reshape(shape), bool((h[n:] == pattern).all())


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "%d cells differ, first at %s: got %#x want %#x" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def check_codes(inp, X, info=None, packed=None):
    """bark_leaf_codes_hip for the call's forests (or `info`/`packed`) against the reference, padding and guard included; -> device codes"""
    info = info or inp.info
    packed = inp.packed if packed is None else packed
    which = inp.which if info is inp.info else np.arange(int(info.B))
    buf, shape = run_codes(info, device(packed), device(X))
    got, intact = split(buf, shape)
    want = fr.codes_of(inp, X)[which]
    assert got.shape == want.shape
    assert np.array_equal(got, want), first_difference(got, want)
    assert intact, "written behind B * W * npad"
    return buf, got


@pytest.mark.parametrize("name", fr.WALK_CASES)
def test_leaf_codes_and_indices(name):
    inp = fr.make_inputs(name)
    case = inp.case
    fr.check_shape(name, inp)
    fault_flag()
    _, got = check_codes(inp, inp.X1)
    n = inp.distinct.shape[0]
    if case.B > n:  # the same planes from another walk variant: the distinct forests alone, a grid of a few workgroups
        few = fr.distinct_info(inp)
        assert fr.walk_variant_name(fr.query(few, case.N, case.N, case.d)) != fr.walk_variant_name(fr.query(inp.info, case.N, case.N, case.d))
        _, small = check_codes(inp, inp.X1, few, inp.packed[:n])
        assert np.array_equal(got, small[inp.which])
    buf, shape = run_indices(inp.info, device(inp.packed), device(inp.X1))
    idx, intact = split(buf, shape)
    want = np.stack([orc.pass_through_forest(F, inp.X1, inp.ft) for F in inp.distinct])[inp.which]
    assert np.array_equal(idx, want), first_difference(idx, want)
    assert intact, "written behind B * N * m"
    assert fault_flag() == 0  # NaN and inf sit on non-categorical features only


@pytest.mark.parametrize("name", [n for n in fr.WALK_CASES if fr.CASES[n].mixed and fr.CASES[n].d >= 4])
def test_categorical_fault_in_the_last_block(name):
    """One invalid category (NaN, -1, inf in turn) at the last point — in the last, partly live block — raises the context's
    fault flag exactly when the reference raises for that point; the clean input leaves it at 0; reading clears it."""
    inp = fr.make_inputs(name)
    case = inp.case
    run = run_indices if case.indices else run_codes
    packed_d = device(inp.packed)
    fault_flag()
    seen = 0
    for bad in (np.nan, -1.0, np.inf):
        X = inp.X1.copy()
        X[case.N - 1, inp.ft == fr.CAT] = bad
        expected = 0
        for F in inp.distinct:
            try:
                orc.pass_through_forest(F, X[case.N - 1:], inp.ft)
            except ValueError:
                expected = 1
        run(inp.info, packed_d, device(X))
        assert fault_flag() == expected, (name, bad)
        assert fault_flag() == 0  # cleared by the read
        run(inp.info, packed_d, device(inp.X1))
        assert fault_flag() == 0, (name, "clean input")
        seen += expected
    assert seen == 3 or case.m < 8, name  # (a single prior tree may not split on a category at all)


def gram_reference(counts, case, M, par, b):
    p = {k: (None if v is None else float(v[b])) for k, v in par.items()}
    return fr.gram_from_counts(counts[:, :M], case.m, **p)


@pytest.mark.parametrize("name", fr.GRAM_CASES)
def test_gram_block_and_canary(name):
    inp = fr.make_inputs(name)
    case = inp.case
    fr.check_shape(name, inp)
    lib = _lib.lib()
    B, N = case.B, case.N
    fault_flag()
    codes1, _ = check_codes(inp, inp.X1)
    codes2 = {case.M: codes1 if case.same else check_codes(inp, inp.X2)[0]}
    assert fault_flag() == 0
    null = {"shift": None, "scale": None, "noise": None}
    for combo in (fr.PARAM_COMBOS if case.params else [()]):
        if combo:
            par, counts = fr.gram_params(inp, combo)
        else:
            par, counts = null, [fr.agree_from_indices(orc.pass_through_forest(inp.distinct[w], inp.X1, inp.ft),
                                                       orc.pass_through_forest(inp.distinct[w], inp.X2, inp.ft)) for w in inp.which]
        par_d = {k: (None if v is None else device(v)) for k, v in par.items()}
        for ld, bs, off, M in fr.gram_layouts(case):
            if M not in codes2:  # the planes of x2 are npad(M) apart: codes of the first M points, walked again
                codes2[M] = check_codes(inp, inp.X2[:M])[0]
            total = off + (B - 1) * bs + N * ld
            buf = canary(total + GUARD, "f64")
            assert buf.data_ptr() % 16 == 0
            v = fr.query(inp.info, N, M, case.d, ld, bs, 8 * off)
            rc = lib.bark_gram_from_leaves_hip(_lib.ptr(codes1), N, _lib.ptr(codes2[M]), M, ctypes.byref(inp.info), _lib.ptr(par_d["shift"]),
                                               _lib.ptr(par_d["scale"]), _lib.ptr(par_d["noise"]), ctypes.c_void_p(buf.data_ptr() + 8 * off),
                                               ld, bs, _lib.stream_ptr())
            assert rc == 0, lib.bark_last_error()
            got = host(buf)
            want = np.full(total + GUARD, fr.CANARY64, dtype=np.uint64)
            cell = np.full(total + GUARD, -1, dtype=np.int64)
            for b in range(B):
                ref = gram_reference(counts[b], case, M, par, b)
                pos = off + b * bs + np.arange(N)[:, None] * ld + np.arange(M)[None, :]
                want[pos] = ref.view(np.uint64)
                cell[pos] = (b * N + np.arange(N)[:, None]) * M + np.arange(M)[None, :]
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                where = [("b=%d i=%d j=%d" % (c // (N * M), c // M % N, c % M)) if c >= 0 else "outside the block, element %d" % e
                         for e, c in zip(bad[:8], cell[bad[:8]])]
                raise AssertionError("%s %s combo=%s ld=%d batch_stride=%d offset=%d M=%d: %d elements differ: %s (got %#x want %#x)" % (
                    name, fr.gram_variant_name(v), combo, ld, bs, off, M, len(bad), where, got[bad[0]], want[bad[0]]))


def test_refusals_launch_nothing():
    """BARK_ERR_ARG with a message, and the canary intact: a code of 113 words, ld < M, more than 65535 forests."""
    lib = _lib.lib()
    rng = np.random.default_rng(113)
    ft = fr.feature_types(4, True)
    F = fr.make_forests("bits113", 1, 8, ft, rng)
    info, packed = fr.pack(F, ft)
    assert fr.query(info, 40, 40, 4).words == 113
    X = fr.points(40, ft, rng)
    buf, shape = run_codes(info, device(packed), device(X), expect_rc=_lib.BARK_ERR_ARG)
    assert b"113" in lib.bark_last_error() and (host(buf) == fr.CANARY32).all()

    F = fr.make_forests("prior", 2, 9, ft, rng)
    info, packed = fr.pack(F, ft)
    packed_d, X_d = device(packed), device(X)
    codes, shape = run_codes(info, packed_d, X_d)
    out = canary(2 * 40 * 40 + GUARD, "f64")
    null = ctypes.c_void_p(0)
    rc = lib.bark_gram_from_leaves_hip(_lib.ptr(codes), 40, _lib.ptr(codes), 40, ctypes.byref(info), null, null, null, _lib.ptr(out), 39, 1600, _lib.stream_ptr())
    assert rc == _lib.BARK_ERR_ARG and b"ld=39" in lib.bark_last_error() and (host(out) == fr.CANARY64).all()

    many = _lib.PackInfo.from_buffer_copy(info)  # a hand-written info: nothing behind the two packed forests is ever read
    many.B = 65536
    many.packed_bytes = many.B * many.m * many.stride * 16
    small = canary(4096, "u32")
    for fn in (lib.bark_leaf_codes_hip, lib.bark_leaf_indices_hip):
        rc = fn(_lib.ctx(), _lib.ptr(packed_d), ctypes.byref(many), _lib.ptr(X_d), 40, 4, _lib.ptr(small), _lib.stream_ptr())
        assert rc == _lib.BARK_ERR_ARG and b"65535" in lib.bark_last_error() and (host(small) == fr.CANARY32).all()
    rc = lib.bark_gram_from_leaves_hip(_lib.ptr(codes), 40, _lib.ptr(codes), 40, ctypes.byref(many), null, null, null, _lib.ptr(out), 40, 1600, _lib.stream_ptr())
    assert rc == _lib.BARK_ERR_ARG and b"65535" in lib.bark_last_error() and (host(out) == fr.CANARY64).all()
    assert fault_flag() == 0


@pytest.mark.parametrize("N,m,t,value,gap,col0", [(300, 7, 3, 1.0, 0, 0), (257, 5, 4, 0.75, 3, 2), (1, 1, 0, -2.5, 1, 1), (37, 9, 0, 1.5, 5, 0)])
def test_onehot_match_strided(N, m, t, value, gap, col0):
    """bark_onehot_match_hip against np.equal: a column of the (N, m) index output (ldl = m), an output of row stride ldo > r at
    a column offset, a value other than 1, N * r no multiple of 256; the canary everywhere outside the written columns."""
    lib = _lib.lib()
    rng = np.random.default_rng(N + m)
    ft = fr.feature_types(8, True)
    F = fr.make_forests("prior", 1, m, ft, rng)
    info, packed = fr.pack(F, ft)
    X = fr.points(N, ft, rng, F)
    buf, shape = run_indices(info, device(packed), device(X))
    idx = split(buf, shape)[0][0]
    assert np.array_equal(idx, orc.pass_through_forest(F[0], X, ft))
    ids = np.unique(idx[:, t])
    r = len(ids)
    ldo = col0 + r + gap
    assert (N * r) % 256 or N * r == 0
    out = canary(N * ldo + GUARD, "f64")
    rc = lib.bark_onehot_match_hip(ctypes.c_void_p(buf.data_ptr() + 4 * t), N, m, _lib.ptr(device(ids)), r, value,
                                   ctypes.c_void_p(out.data_ptr() + 8 * col0), ldo, _lib.stream_ptr())
    assert rc == 0, lib.bark_last_error()
    want = np.full(N * ldo + GUARD, fr.CANARY64, dtype=np.uint64)
    block = np.where(np.equal(idx[:, t][:, None], ids[None, :]), value, 0.0)
    want[(np.arange(N)[:, None] * ldo + col0 + np.arange(r)[None, :])] = block.view(np.uint64)
    got = host(out)
    assert np.array_equal(got, want), first_difference(got, want)
