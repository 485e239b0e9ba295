"""The low-rank updates of csrc/lowrank.hip — bark_lowrank_update_hip, bark_lowrank_swap_eval_hip / _apply_hip, the chain
entry points behind ChainBatch and the Metropolis decision of a device-side sweep — against the host reference of
tests/lowrank_ref.py (pinned to the oracle, to np.longdouble and to the dispatch by tests/test_lowrank_reference_cpu.py).

Every row of lowrank_ref.UPDATE_CASES sits on an edge of a kernel (rows per workgroup, column chunks, tiles, rank bins,
segment lengths of the column form) and runs with a K_inv that is NOT symmetric — so the right factor U'K_inv, the column
form's output blocks and the `symmetric` flag all show in the result — and with its symmetrised form where the call
promises symmetry.  Per call: the result against the reference; the K_out-only, logabsdet-only and in-place forms and a
second call bit for bit against the first; NaN guard bands around K_out and a byte pattern around a workspace of exactly
bark_lowrank_workspace_bytes(N, r).  PIVOT_CASES need the row swap of small_kernel or report an exactly singular system at a
known column; CHAIN_CASES run one to 64 chains, pairs of unequal leaf counts and both sides of the 8 / 9 and 16 / 17 leaf
switches through ChainBatch against the host and against single chains.

The bars are the project's (lowrank_ref.MAT_*, SCALAR_*, BATCH_*); the fraction of each that a case uses is printed (-s).

Not tested: a sweep in which one chain's proposal is exactly singular (the -1 latch of decide_kernel).  With trees that
partition the points, C + U'K_inv U is singular only if the swapped kernel matrix is, and scale K + (1e-6 + noise) I never is;
no honest input reaches the latch through ChainBatch.  The flag itself is tested through the raw entry points below."""
import ctypes

import numpy as np
import pytest

import lowrank_ref as lr

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
PAD = 32 * 1024  # bytes of pattern on either side of the workspace: more than a whole 128-column block of partials (16 KiB at r = 16)


@pytest.fixture(scope="module")
def G():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bark_amd.fitting as fit
    from bark_amd import _lib

    class NS:
        pass

    ns = NS()
    ns.torch, ns.lib, ns.L, ns.fit = torch, _lib.lib(), _lib, fit
    return ns


class Guarded:
    """An (N, N) output between two bands of NaN."""

    def __init__(self, G, N, fill=None):
        self.G, self.N, self.band = G, N, max(2 * N, 256)
        self.buf = G.torch.full((2 * self.band + N * N,), float("nan"), dtype=G.torch.float64, device="cuda")
        self.mat = self.buf[self.band:self.band + N * N].view(N, N)
        if fill is not None:
            self.mat.copy_(fill)

    def clean(self):
        t = self.G.torch
        return bool(t.isnan(self.buf[:self.band]).all()) and bool(t.isnan(self.buf[self.band + self.N * self.N:]).all()) \
            and not bool(t.isnan(self.mat).any())


class Workspace:
    """Exactly bark_lowrank_workspace_bytes(N, r) bytes inside a buffer filled with a byte pattern."""

    def __init__(self, G, N, r):
        self.G, self.N, self.r = G, N, r
        self.bytes = int(G.lib.bark_lowrank_workspace_bytes(N, r))
        assert self.bytes > 0
        self.buf = G.torch.full((2 * PAD + self.bytes,), PATTERN, dtype=G.torch.uint8, device="cuda")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + PAD)

    def intact(self):
        return bool((self.buf[:PAD] == PATTERN).all()) and bool((self.buf[PAD + self.bytes:] == PATTERN).all())

    def status(self):
        flag = ctypes.c_int32(-7)
        self.G.L.check(self.G.lib.bark_lowrank_status_hip(self.ptr, self.N, self.r, ctypes.byref(flag), self.G.L.stream_ptr()))
        return flag.value


def scalar_slot(G, n=1):
    """n doubles between NaN neighbours: -> (whole tensor, pointer to the first of the n)."""
    t = G.torch.full((n + 2,), float("nan"), dtype=G.torch.float64, device="cuda")
    return t, ctypes.c_void_p(t.data_ptr() + 8)


def run_update(G, K, U, sub, sym, ws, K_out=None, want_logdet=True, in_place=False):
    """One bark_lowrank_update_hip -> (Guarded or None, logabsdet tensor or None)."""
    N, r = U.shape
    out = None
    if in_place:
        out = Guarded(G, N, fill=K)
        K_ptr = out_ptr = G.L.ptr(out.mat)
    else:
        out = Guarded(G, N) if K_out else None
        K_ptr, out_ptr = G.L.ptr(K), G.L.ptr(out.mat if out else None)
    slot, slot_ptr = scalar_slot(G) if want_logdet else (None, ctypes.c_void_p(0))
    G.L.check(G.lib.bark_lowrank_update_hip(K_ptr, N, G.L.ptr(U), r, int(sub), int(sym), out_ptr, slot_ptr, ws.ptr, ws.bytes,
                                            G.L.stream_ptr()))
    G.torch.cuda.synchronize()
    assert ws.intact(), "written outside the workspace"
    if out is not None:
        assert out.clean(), "K_out: written outside, or a NaN inside"
    if slot is not None:
        assert bool(G.torch.isnan(slot[[0, 2]]).all()) and not bool(G.torch.isnan(slot[1]))
    return out, slot


def run_swap(G, Ks, U, r_old, y, ws):
    """eval, apply out of place, apply in place -> (scalars (2,), K_out Guarded, in-place Guarded)."""
    N, r = U.shape
    slot, slot_ptr = scalar_slot(G, 2)
    G.L.check(G.lib.bark_lowrank_swap_eval_hip(G.L.ptr(Ks), N, G.L.ptr(U), r_old, r - r_old, G.L.ptr(y), slot_ptr, ws.ptr, ws.bytes,
                                               G.L.stream_ptr()))
    out, inplace = Guarded(G, N), Guarded(G, N, fill=Ks)
    G.L.check(G.lib.bark_lowrank_swap_apply_hip(G.L.ptr(Ks), N, r, ws.ptr, G.L.ptr(out.mat), G.L.stream_ptr()))
    G.L.check(G.lib.bark_lowrank_swap_apply_hip(G.L.ptr(inplace.mat), N, r, ws.ptr, G.L.ptr(inplace.mat), G.L.stream_ptr()))
    G.torch.cuda.synchronize()
    assert ws.intact() and out.clean() and inplace.clean()
    assert bool(G.torch.isnan(slot[[0, 3]]).all())
    return slot[1:3], out, inplace


def report(name, worst):
    print(name, "fraction of each bar used:", {k: "%.2g" % v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


def note(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), value)


# ------------------------------------------------------------------------------ update cases ----
@pytest.mark.parametrize("name", list(lr.UPDATE_CASES))
def test_update_and_swap_on_every_edge(G, name):
    torch, dev = G.torch, G.L.to_device
    case, inp = lr.UPDATE_CASES[name], lr.make_inputs(name)
    N, r = case.N, case.r
    U, y = dev(inp.U), dev(inp.y)
    ws = Workspace(G, N, r)
    worst = {}
    for sym in (0, 1):
        K_host = inp.Ks if sym else inp.K
        K = dev(K_host)
        for sub in (0, 1):
            tag = (name, sub, sym)
            want, want_lad = lr.update(K_host, inp.U, sub)
            full, lad = run_update(G, K, U, sub, sym, ws, K_out=True)
            assert ws.status() == 0, tag
            note(worst, "K_out", lr.used(full.mat.cpu().numpy(), want, lr.MAT_RTOL, lr.MAT_ATOL))
            note(worst, "logabsdet", lr.used(float(lad[1]), want_lad, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
            # the forms with one output, K_out == K_inv, and the same call again: the same bits
            only_K, _ = run_update(G, K, U, sub, sym, ws, K_out=True, want_logdet=False)
            assert torch.equal(only_K.mat, full.mat), tag
            del only_K
            _, only_lad = run_update(G, K, U, sub, sym, ws, K_out=False)
            assert torch.equal(only_lad[1], lad[1]), tag
            aliased, alias_lad = run_update(G, K, U, sub, sym, ws, in_place=True)
            assert torch.equal(aliased.mat, full.mat) and torch.equal(alias_lad[1], lad[1]), tag
            del aliased
            again, again_lad = run_update(G, K, U, sub, sym, ws, K_out=True)
            assert torch.equal(again.mat, full.mat) and torch.equal(again_lad[1], lad[1]), tag
            del again, full
            assert torch.equal(K, dev(K_host)), tag  # the input is read only
    Ks = dev(inp.Ks)
    for r_old in lr.swap_splits(case):
        want_q, want_d, want = lr.swap(inp.Ks, inp.U, r_old, inp.y)
        scalars, out, inplace = run_swap(G, Ks, U, r_old, y, ws)
        assert ws.status() == 0, (name, r_old)
        got_q, got_d = (float(v) for v in scalars.cpu().numpy())
        note(worst, "dquad", lr.used(got_q, want_q, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
        note(worst, "dlogdet", lr.used(got_d, want_d, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
        note(worst, "swap K_out", lr.used(out.mat.cpu().numpy(), want, lr.MAT_RTOL, lr.MAT_ATOL))
        assert torch.equal(inplace.mat, out.mat), (name, r_old)
        scalars2, out2, _ = run_swap(G, Ks, U, r_old, y, ws)
        assert torch.equal(scalars2, scalars) and torch.equal(out2.mat, out.mat), (name, r_old)
        del out, out2, inplace
    report(name, worst)


# ------------------------------------------------------------------------------- pivot cases ----
@pytest.mark.parametrize("N", lr.PIVOT_N)
@pytest.mark.parametrize("name", list(lr.PIVOT_CASES))
def test_pivot_cases(G, name, N):
    """K = I, subtract.  symmetric = 1 takes the column form at N = 130 and the row form at N = 129; symmetric = 0 the row
    form at both.  The singular systems are ordinary data the library is documented to report."""
    dev = G.L.to_device
    case = lr.PIVOT_CASES[name]
    r = case.r
    U_host = lr.pivot_U(name, N)
    K, U = dev(np.eye(N)), dev(U_host)
    y_host = np.random.default_rng(N).standard_normal(N)
    y = dev(y_host)
    ws = Workspace(G, N, r)

    def update(U_dev, sym):
        slot, slot_ptr = scalar_slot(G)
        out = Guarded(G, N)
        G.L.check(G.lib.bark_lowrank_update_hip(G.L.ptr(K), N, G.L.ptr(U_dev), r, 1, sym, G.L.ptr(out.mat), slot_ptr, ws.ptr, ws.bytes,
                                                G.L.stream_ptr()))
        return out, slot

    def swap_eval(U_dev):
        slot, slot_ptr = scalar_slot(G, 2)
        G.L.check(G.lib.bark_lowrank_swap_eval_hip(G.L.ptr(K), N, G.L.ptr(U_dev), r, 0, G.L.ptr(y), slot_ptr, ws.ptr, ws.bytes,
                                                   G.L.stream_ptr()))
        return slot

    if not case.singular:
        worst = {}
        want, want_lad = lr.update(np.eye(N), U_host, True)
        for sym in (1, 0):
            out, slot = update(U, sym)
            assert ws.status() == 0 and ws.intact() and out.clean(), (name, sym)
            note(worst, "K_out", lr.used(out.mat.cpu().numpy(), want, lr.MAT_RTOL, lr.MAT_ATOL))
            note(worst, "logabsdet", lr.used(float(slot[1]), want_lad, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
        want_q, want_d, _ = lr.swap(np.eye(N), U_host, r, y_host)  # r_old = r: C = -I, the same system
        slot = swap_eval(U)
        assert ws.status() == 0
        note(worst, "dquad", lr.used(float(slot[1]), want_q, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
        note(worst, "dlogdet", lr.used(float(slot[2]), want_d, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
        report(f"{name}/N{N}", worst)
        return
    regular_host = lr.pivot_U("swap_col3", N)  # the same r: the same workspace layout
    assert lr.PIVOT_CASES["swap_col3"].r == r
    regular = dev(regular_host)
    want, want_lad = lr.update(np.eye(N), regular_host, True)
    for sym in (1, 0):
        update(U, sym)
        assert ws.status() == case.singular, (name, sym)
        out, slot = update(regular, sym)  # the flag does not outlive the call that set it
        assert ws.status() == 0 and ws.intact() and out.clean(), (name, sym)
        assert lr.used(out.mat.cpu().numpy(), want, lr.MAT_RTOL, lr.MAT_ATOL) <= 1.0
        assert lr.used(float(slot[1]), want_lad, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    swap_eval(U)
    assert ws.status() == case.singular, name
    slot = swap_eval(regular)
    assert ws.status() == 0 and ws.intact(), name
    want_q, want_d, _ = lr.swap(np.eye(N), regular_host, r, y_host)
    assert lr.used(float(slot[1]), want_q, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    assert lr.used(float(slot[2]), want_d, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    update(U, 1)
    assert ws.status() == case.singular  # update after swap_eval, and
    swap_eval(regular)
    assert ws.status() == 0  # swap_eval clears what update left


# ------------------------------------------------------------------------------- chain cases ----
@pytest.mark.parametrize("name", list(lr.CHAIN_CASES))
def test_chain_batch_against_host_and_single_chains(G, name):
    torch, fit = G.torch, G.fit
    case, inp = lr.CHAIN_CASES[name], lr.make_chain_inputs(name)
    nc, m = len(case.leaves), inp.forests.shape[1]
    X, y, ft = inp.X, inp.y, inp.ft
    old = inp.forests[:, 0]
    batch = fit.ChainBatch.from_forests(inp.forests, inp.noise, inp.scale, X, y, ft)
    got = batch.propose_trees(old, inp.new, X, ft, inp.scale, m)
    assert got.shape == (nc,) and np.isfinite(got).all()
    mask = np.arange(nc) % 3 != 1 if nc > 1 else np.array([True])  # chains 0 and 63 accept, 1 and 31 reject
    picked = sorted({0, 1, nc // 2 - 1, nc - 1} & set(range(nc))) if nc > 8 else list(range(nc))
    worst, refs = {}, {}
    for b in picked:
        want, _, K_new = lr.chain_reference(inp, b)
        refs[b] = K_new
        note(worst, "new_mll", lr.used(got[b], want, lr.SCALAR_RTOL, lr.SCALAR_ATOL))
    if nc == lr.MAX_CHAINS:
        assert {0, 31, 63} <= set(picked)
    singles = [fit.ChainState.from_forest(inp.forests[b], inp.noise[b], inp.scale[b], X, y, ft) for b in range(nc)]
    want1 = np.array([singles[b].propose_tree(old[b], inp.new[b], X, ft, inp.scale[b], m) for b in range(nc)])
    note(worst, "batch vs single", lr.used(got, want1, lr.BATCH_RTOL, lr.BATCH_ATOL))
    before = batch.K_inv.clone()
    batch.accept(mask)
    for b in range(nc):
        if mask[b]:
            singles[b].accept()
            assert torch.equal(batch.K_inv[b], singles[b].K_inv), (name, b)  # accepted: the single chain's bits
            if b in refs:  # and the swapped inverse, at the bar the chain tests hold a resident inverse to
                note(worst, "K_inv after accept (rtol 1e-7, atol 1e-8)", lr.used(batch.K_inv[b].cpu().numpy(), refs[b], 1e-7, 1e-8))
        else:
            assert torch.equal(batch.K_inv[b], before[b]), (name, b)  # rejected: untouched
    note(worst, "mll after accept", lr.used(batch.mll, [s.mll for s in singles], lr.BATCH_RTOL, lr.BATCH_ATOL))
    report(name, worst)


# ----------------------------------------------------------------------------- decision rule ----
@pytest.mark.parametrize("N", [130, 129])
def test_device_decision_rejects_nan(G, N):
    """ChainBatch.sweep_trees, 3 chains x 4 steps, against the host rule (lowrank_ref.metropolis) driven through
    propose_trees / accept: N = 130 decides inside small_kernel, N = 129 in decide_kernel.  One log_u and one log_q_prior are
    NaN: bark_sampler.py:259 compares against Python's min(log_alpha, 0), which is NaN then — both are rejections."""
    torch, fit = G.torch, G.fit
    from bark_amd import synthetic

    nc, steps = 3, 4
    X, y, _, ft = synthetic.unit_cube_problem(N, lr.CHAIN_D, seed=N)
    cur = np.stack([np.stack([lr.caterpillar_tree(2 + (b + t) % 4, (b + t) % lr.CHAIN_D) for t in range(steps)]) for b in range(nc)])
    prop = np.stack([np.stack([lr.caterpillar_tree(1 + (2 * b + t) % 5, (b + 2 * t + 1) % lr.CHAIN_D) for t in range(steps)])
                     for b in range(nc)])
    assert lr.chain_path(N, 5 + 5) == ("grid<16>" if N == 130 else "streams")
    noise, scale = np.array([0.1, 0.07, 0.2]), np.array([1.0, 0.8, 1.2])
    rng = np.random.default_rng(11)
    log_q = rng.normal(0.0, 0.5, size=(nc, steps))
    log_u = np.log(rng.uniform(size=(nc, steps)))
    log_u[0, 1] = np.nan
    log_q[1, 2] = np.nan
    host = fit.ChainBatch.from_forests(cur, noise, scale, X, y, ft)
    want_mask = np.zeros((nc, steps), dtype=bool)
    for t in range(steps):
        before = host.mll.copy()
        vals = host.propose_trees(cur[:, t], prop[:, t], X, ft, scale, steps)
        want_mask[:, t] = [lr.metropolis(2.0 * (vals[b] - before[b]), 0.0, log_q[b, t], log_u[b, t]) == 1 for b in range(nc)]
        host.accept(want_mask[:, t])
    assert not want_mask[0, 1] and not want_mask[1, 2]
    finite = np.isfinite(log_q) & np.isfinite(log_u)
    assert 0 < want_mask[finite].sum() < finite.sum()  # both branches of the rule among the ordinary proposals
    dev = fit.ChainBatch.from_forests(cur, noise, scale, X, y, ft)
    mask = dev.sweep_trees(cur, prop, log_q, log_u, X, ft, scale, steps)
    assert not mask[0, 1], "a NaN log_u was accepted"
    assert not mask[1, 2], "a NaN log_q_prior was accepted"
    assert np.array_equal(mask, want_mask), (mask, want_mask)
    assert np.array_equal(dev.last_accept, want_mask.astype(np.int32))  # 0 / 1: nothing singular
    worst = {"quad": lr.used(dev.quad, host.quad, lr.BATCH_RTOL, lr.BATCH_ATOL),
             "logdet": lr.used(dev.logdet, host.logdet, lr.BATCH_RTOL, lr.BATCH_ATOL)}
    assert torch.equal(dev.K_inv, host.K_inv)  # K_inv and the running state moved for the accepted proposals only
    report(f"decision/N{N}", worst)
