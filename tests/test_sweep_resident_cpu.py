"""The host side of the one-launch tree sweep (csrc/sweep_resident.hip): the shape query behind bark_amd.fitting.sweep_plan, the
step-table builder, and the condition that makes tests/test_gpu_sweep_resident.py's mask comparisons exact — every proposal of
every GPU case is decided with a margin of at least 1e-6, in float64 and in np.longdouble alike.  No GPU."""
import ctypes

import numpy as np
import pytest

import lowrank_ref as lr
import sweep_resident_ref as sr


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


def test_sweep_plan_variants_and_limits(L):
    from bark_amd.fitting import sweep_plan

    p = sweep_plan(128, 6, 4)
    assert p["variant"] == 1 and p["threads"] in (512, 1024) and 0 < p["lds_bytes"] <= 160 * 1024 and p["reason"] == ""
    assert sweep_plan(129, 6, 4)["variant"] == 2
    p = sweep_plan(512, 6, 4)
    assert p["variant"] == 2 and 0 < p["lds_bytes"] <= 160 * 1024
    for kwargs in (dict(N=513, r_max=6, d=4), dict(N=128, r_max=17, d=4), dict(N=128, r_max=6, d=4, nc=65), dict(N=0, r_max=6, d=4),
                   dict(N=128, r_max=1, d=4)):
        p = sweep_plan(**kwargs)
        assert p["variant"] == 0 and p["lds_bytes"] == 0 and p["reason"], kwargs
    assert sweep_plan(128, 6, 4, max_nodes_bytes=2048)["variant"] == 1
    p = sweep_plan(128, 6, 4, max_nodes_bytes=2080)  # 65 packed nodes per tree: the pair does not fit its 2 KiB of LDS
    assert p["variant"] == 0 and "bark_tree_sweep_chains_hip" in p["reason"]
    # X rows that push K_inv out of LDS: the other variant, not an overflow — and every answer fits the CU's 160 KiB
    d_lds = max(d for d in range(1, 200) if sweep_plan(128, 6, d)["variant"] == 1)
    p = sweep_plan(128, 6, d_lds + 2)
    assert p["variant"] == 2 and p["lds_bytes"] <= 160 * 1024
    for N in (1, 3, 64, 127, 128, 129, 256, 511, 512):
        d_max = sweep_plan(N, 16, 1)["d_max"]
        assert d_max >= 4
        assert sweep_plan(N, 16, d_max)["variant"] in (1, 2) and sweep_plan(N, 16, d_max)["lds_bytes"] <= 160 * 1024
        p = sweep_plan(N, 16, d_max + 1)
        assert p["variant"] == 0 and "bark_tree_sweep_chains_hip" in p["reason"]


def _infos(L, specs):
    infos = (L.PackInfo * len(specs))()
    for t, (B, m, stride, depth, bits) in enumerate(specs):
        infos[t].B, infos[t].m, infos[t].L, infos[t].stride = B, m, 100, stride
        infos[t].max_leaves, infos[t].max_depth, infos[t].packed_bytes, infos[t].max_bits = bits, depth, B * m * stride * 16, bits
    return infos


def test_table_builder(L):
    lib = L.lib()
    steps, nc = 3, 2
    infos = _infos(L, [(2, 2, 5, 2, 6), (2, 2, 31, 8, 16), (2, 2, 1, 0, 2)])
    offsets = np.array([0, 256, 2304], dtype=np.int64)
    r_old = np.array([[3, 1], [15, 8], [1, 1]], dtype=np.int64)
    nbytes = int(lib.bark_tree_sweep_resident_table_bytes(steps, nc))
    assert nbytes == 8 * (4 * steps + steps * nc)
    buf = np.full(nbytes + 16, 0x5A, dtype=np.uint8)

    def build(offsets=offsets, infos=infos, r_old=r_old, nc=nc):
        return lib.bark_tree_sweep_resident_table(L.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), L.ptr(r_old), steps, nc,
                                                  ctypes.c_void_p(buf.ctypes.data + 8))

    assert build() == L.BARK_OK
    assert (buf[:8] == 0x5A).all() and (buf[-8:] == 0x5A).all()
    words = np.frombuffer(buf[8:-8].tobytes(), dtype=np.int64)
    head, tail = words[:4 * steps].reshape(steps, 4), words[4 * steps:].reshape(steps, nc)
    assert np.array_equal(head, [[0, 5, 2, 6], [256, 31, 8, 16], [2304, 1, 0, 2]]) and np.array_equal(tail, r_old)
    for bad in ([[0, 1], [15, 8], [1, 1]], [[6, 1], [15, 8], [1, 1]], [[3, 1], [16, 8], [1, 1]]):  # r_old outside (0, r)
        assert build(r_old=np.array(bad, dtype=np.int64)) == L.BARK_ERR_ARG and b"r_old" in lib.bark_last_error()
    assert build(infos=_infos(L, [(2, 3, 5, 2, 6), (2, 2, 31, 8, 16), (2, 2, 1, 0, 2)])) == L.BARK_ERR_ARG  # m != 2
    assert build(infos=_infos(L, [(2, 2, 5, 2, 6), (3, 2, 31, 8, 16), (2, 2, 1, 0, 2)])) == L.BARK_ERR_ARG  # B != nc
    assert build(infos=_infos(L, [(2, 2, 5, 2, 6), (2, 2, 33, 8, 17), (2, 2, 1, 0, 2)])) == L.BARK_ERR_ARG  # 17 leaves
    assert b"bark_tree_sweep_chains_hip" in lib.bark_last_error()
    assert build(offsets=np.array([0, 250, 2304], dtype=np.int64)) == L.BARK_ERR_ARG  # not 16-byte aligned
    assert build(infos=_infos(L, [(2, 2, 64, 2, 6), (2, 2, 31, 8, 16), (2, 2, 1, 0, 2)])) == L.BARK_OK  # 64 packed nodes per tree fit
    assert build(infos=_infos(L, [(2, 2, 65, 2, 6), (2, 2, 31, 8, 16), (2, 2, 1, 0, 2)])) == L.BARK_ERR_ARG  # 65 do not
    assert b"bark_tree_sweep_chains_hip" in lib.bark_last_error()
    assert lib.bark_tree_sweep_resident_table_bytes(3, 65) == 0 and lib.bark_tree_sweep_resident_table_bytes(0, 2) == 0
    assert lib.bark_tree_sweep_resident_workspace_bytes(128, 16, 64) > 0 and lib.bark_tree_sweep_resident_workspace_bytes(513, 16, 1) == 0


def _check_margin(name, inp):
    lo, hi = sr.host_sweep(inp), sr.host_sweep(inp, np.longdouble)
    assert np.array_equal(lo.mask, hi.mask), name
    assert (lo.mask >= 0).all()
    smallest = min(lo.margin.min(), hi.margin.min())
    print(name, "smallest decision margin", smallest)
    assert smallest >= sr.MARGIN, (name, smallest)
    ordinary = np.isfinite(inp.log_q) & np.isfinite(inp.log_u)
    assert 0 < lo.mask[ordinary].sum() < ordinary.sum(), name  # both branches among the ordinary proposals
    assert np.allclose(lo.quad, hi.quad, rtol=1e-9, atol=1e-9) and np.allclose(lo.logdet, hi.logdet, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_decision_margin_of_every_gpu_case(name):
    case, inp = sr.CASES[name], sr.make_inputs(name)
    assert inp.cur.shape[:2] == (case.nc, case.steps) and inp.X.shape == (case.N, lr.CHAIN_D)
    r = [sum(pair) for row in case.leaves for pair in row]
    assert 2 <= min(r) and max(r) <= 16
    _check_margin(name, inp)


@pytest.mark.parametrize("N", [128, 130])
def test_decision_margin_of_the_nan_cases(N):
    inp = sr.nan_inputs(N)
    _check_margin(f"nan/N{N}", inp)
    tr = sr.host_sweep(inp)
    assert tr.mask[0, 1] == 0 and tr.mask[1, 2] == 0  # the NaN log_u and the NaN log_q_prior reject


def _gauss_jordan(den):
    """small_kernel's elimination in float64: den^-1 as the kernels compute it (symmetric only to cond(den) * eps)."""
    r = den.shape[0]
    a = np.concatenate([den, np.eye(r)], axis=1)
    for col in range(r):
        p = col + int(np.argmax(np.abs(a[col:, col])))
        if p != col:
            a[[col, p]] = a[[p, col]]
        a[col] = a[col] / a[col, col]
        others = np.arange(r) != col
        a[others] = a[others] - np.outer(a[others, col], a[col])
    return a[:, r:]


def test_mirrored_rewrite_needs_the_symmetrised_inverse():
    """The rewrite of sweep_resident.hip restated in numpy on the n512 case (three accepted 16-leaf steps in a row, cond(den) up to
    1e5): mirroring the upper triangle of Y S Y' with S = (inv + inv') / 2 stays as close to np.longdouble as the multi-launch
    path's K - (Y inv) Y', inside the issue's matrix bar.  (Mirrored with the inverse as computed the two triangles hold Y inv Y' and
    Y inv' Y', and the next near-singular system amplifies the difference: printed, not asserted — it is rounding noise.)  A
    restatement of the algorithm, not of the kernel: tests/test_gpu_sweep_resident.py holds the kernel to the same bar."""
    from oracle import oracle as orc

    inp = sr.make_inputs("n512")
    N, steps, y = 512, 3, inp.y.reshape(-1)
    worst = {}
    for b in range(2):
        K = inp.scale[b] * orc.forest_gram_matrix(inp.cur[b], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[b]) * np.eye(N)
        K0 = np.linalg.inv(K)
        K0 = 0.5 * (K0 + K0.T)
        s = np.sqrt(inp.scale[b] / steps)
        runs = {"longdouble": K0.astype(np.longdouble), "launches": K0, "as computed": K0, "symmetrised": K0}
        for t in range(steps):  # every proposal applied: the accept rule is not what is looked at here
            U_old = s * orc.get_leaf_vectors(inp.cur[b, t], inp.X, inp.ft)
            U = np.concatenate([U_old, s * orc.get_leaf_vectors(inp.prop[b, t], inp.X, inp.ft)], axis=1)
            r = U.shape[1]
            C = np.diag(np.where(np.arange(r) < U_old.shape[1], -1.0, 1.0))
            runs["longdouble"] = lr.swap(runs["longdouble"], U, U_old.shape[1], y, np.longdouble)[2]
            for kind in ("launches", "as computed", "symmetrised"):
                Ki = runs[kind]
                Y = Ki @ U
                inv = _gauss_jordan(C + U.T @ Y)
                if kind == "launches":
                    runs[kind] = Ki - (Y @ inv) @ Y.T
                    continue
                D = Y @ (Y @ (0.5 * (inv + inv.T) if kind == "symmetrised" else inv.T)).T
                runs[kind] = Ki - (np.triu(D) + np.triu(D, 1).T)
        want = np.asarray(runs["longdouble"], dtype=np.float64)
        for kind in ("launches", "as computed", "symmetrised"):
            worst[kind] = max(worst.get(kind, 0.0), lr.used(runs[kind], want, lr.MAT_RTOL, lr.MAT_ATOL))
        worst["symmetrised vs launches"] = max(worst.get("symmetrised vs launches", 0.0),
                                               lr.used(runs["symmetrised"], runs["launches"], lr.MAT_RTOL, lr.MAT_ATOL))
    print("fraction of the matrix bar used against np.longdouble:", {k: "%.2g" % v for k, v in worst.items()})
    assert worst["launches"] <= 1.0 and worst["symmetrised"] <= 1.0 and worst["symmetrised vs launches"] <= 1.0  # the issue's bar
