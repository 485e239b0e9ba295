"""The acquisition scan's target kinds (bark_acquisition_scan_targets_hip: expected improvement, probability of improvement,
min-value entropy search) against the host reference of tests/acq_targets_ref.py, over the case table of acq_ref.CASES.

Bars: values within the posterior bar of DESIGN.md section 2 pushed through the formula by the reference itself
(acq_targets_ref.propagated_bar; nothing here is tuned from the device's output), indices equal
(tests/test_acquisition_targets_cpu.py establishes on the host that every case's minimum is separated by 1e-6 and that
float64 agrees with mpmath).  The summation order is part of the contract, so chunking, a repeated call and the two kernel
variants are compared bit for bit."""
import numpy as np
import pytest

import acq_pending_ref as apr
import acq_ref as ar
import acq_targets_ref as tr

pytestmark = pytest.mark.gpu
CASE_KINDS = [(name, kind) for kind in tr.KINDS for name in tr.CASES[kind]]


@pytest.fixture(scope="module")
def scan():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd.optimizer import acquisition_scan

    return acquisition_scan


def run(scan, name, kind, targets=None, **kw):
    inp = ar.make_inputs(name)
    kw.setdefault("chunk", inp.case.chunk)
    targets = tr.targets_of(name) if targets is None else targets
    return scan(inp.model, inp.data, inp.cand, inp.ft, kind=kind, targets=targets, return_values=True, **kw)


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name,kind", CASE_KINDS)
def test_case_against_reference(scan, name, kind):
    want, bar = tr.reference(name, kind)
    at = int(np.argmin(want))
    value, index, acq = run(scan, name, kind)
    assert acq.shape == (ar.CASES[name].C,) and acq.dtype == np.float64
    used = tr.bar_used(acq, want, bar)
    print(f"{name} {kind}: fraction of the propagated bar used {used:.3g}")
    assert used <= 1.0
    assert index == at
    assert value == acq[at]


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("name", ["prior_n257_chunks", "prior_n64", "m64_r256"])
def test_chunking_and_repeats_are_bit_identical(scan, name, kind):
    base = run(scan, name, kind)
    for other in (run(scan, name, kind), run(scan, name, kind, chunk=1), run(scan, name, kind, chunk=ar.CASES[name].B)):
        assert same(other, base)


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("name", ["prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit", "m64_r128"])
def test_lds_and_global_variants_are_bit_identical(scan, name, kind):
    a = run(scan, name, kind, variant="lds")
    assert same(a, run(scan, name, kind, variant="global"))
    assert np.array_equal(a[2], run(scan, name, kind)[2])  # auto


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("name", ["prior_n64", "m2_r65"])
def test_one_target_against_the_same_target_five_times(scan, name, kind):
    """Not bit for bit: g + g + g + g + g rounds at 3 g and at 5 g and the quotient by 5 rounds once more, so (5 g) / 5 is g
    up to 2 eps per forest; the B = 3 forests' running sums then round apart by at most eps / 2 each per call.  Together at
    most (2 + B) eps = 5 eps of mean_b |mean_s g| (a sum of forests of either sign may cancel, so not of the value); 8 eps
    asked."""
    t1 = tr.targets_of(name, 1)
    a = run(scan, name, kind, targets=t1)
    b = run(scan, name, kind, targets=np.repeat(t1, 5, axis=1))
    mu, var = ar.posterior(name)
    g = tr.utility(mu, np.sqrt(var), t1, kind)  # (B, C): one target per forest
    scale = np.abs(g).mean(axis=0)
    err = float((np.abs(a[2] - b[2]) / scale).max() / np.finfo(np.float64).eps)
    print(f"{name} {kind}: S = 1 against the target five times, largest difference {err:.3g} eps of mean_b |g|")
    assert err <= 8.0 and a[1] == b[1]
    # a scalar and a (B,) vector are the (B, 1) matrix
    if name == "m2_r65":
        assert same(a, run(scan, name, kind, targets=t1[:, 0]))
        flat = np.full_like(t1, t1[0, 0])
        assert same(run(scan, name, kind, targets=flat), run(scan, name, kind, targets=float(t1[0, 0])))


def test_incumbent_is_the_default_target(scan):
    inp = ar.make_inputs("m2_r65")
    for kind in ("ei", "pi"):
        a = scan(inp.model, inp.data, inp.cand, inp.ft, kind=kind, return_values=True)
        assert same(a, run(scan, "m2_r65", kind, targets=float(inp.y.min())))


def test_candidate_slabs_ei(scan):
    """C = 65 537: two slabs of candidates under each of two chunks of forests; the values only (tests/acq_ref.py says why
    no minimum of this case is separated), and each slab equal to a scan of that slab alone"""
    case = ar.SLAB_CASE
    inp = ar.make_inputs(case)
    t = tr.targets_of(case, 5)
    want, bar = tr.reference(case, "ei", 5)
    kw = dict(kind="ei", targets=t, return_values=True, chunk=case.chunk)
    value, index, acq = scan(inp.model, inp.data, inp.cand, inp.ft, **kw)
    used = tr.bar_used(acq, want, bar)
    print(f"{case.name} ei: fraction of the propagated bar used {used:.3g}")
    assert used <= 1.0
    slab = 1 << 16
    assert np.array_equal(acq[slab:], scan(inp.model, inp.data, inp.cand[slab:], inp.ft, **kw)[2])
    assert index == int(np.argmin(acq)) and value == acq[index]


def test_pending_and_skip_ei(scan):
    """two pending points and one skipped candidate: the dense reference of tests/acq_pending_ref.py (training inputs
    augmented by the pending points) pushed through the EI formula; the skipped candidate, which would win, does not"""
    t, skip, want, bar, at = tr.pending_reference()
    inp = ar.make_inputs(apr.CASES[tr.PENDING_CASE].base)
    pend = apr.pending_of(tr.PENDING_CASE)
    kw = dict(kind="ei", targets=t, return_values=True, pending=pend)
    value, index, acq = scan(inp.model, inp.data, inp.cand, inp.ft, skip=list(skip), **kw)
    used = tr.bar_used(acq, want, bar)
    print(f"{tr.PENDING_CASE} ei: fraction of the propagated bar used {used:.3g}")
    assert used <= 1.0
    assert index == at and index not in skip and value == acq[at]
    free = scan(inp.model, inp.data, inp.cand, inp.ft, **kw)
    assert free[1] == skip[0] and np.array_equal(free[2], acq)  # a skipped candidate keeps its value
    plain = scan(inp.model, inp.data, inp.cand, inp.ft, kind="ei", targets=t, return_values=True)
    assert not np.array_equal(plain[2], acq)  # the conditioning is not a no-op


def test_greedy_ei_batch(scan):
    from bark_amd.optimizer import propose_batch_from_candidates

    t, picks, vecs, bars = tr.greedy_ei()
    case = apr.CASES[tr.GREEDY_CASE]
    inp = ar.make_inputs(case.base)
    rows, idx = propose_batch_from_candidates(inp.model, inp.data, inp.cand, inp.ft, q=tr.GREEDY_Q, kind="ei", targets=t,
                                              pending=apr.pending_of(tr.GREEDY_CASE))
    assert len(set(idx.tolist())) == tr.GREEDY_Q
    assert np.array_equal(idx, picks) and np.array_equal(rows, inp.cand[picks])


def test_propose_mes_end_to_end(scan):
    """f* on the device from a seeded generator, the scan against them, the row: equal to the arg-min of the host MES
    formula on the f* that generate_fstar_samples returns for the same seed (the gap is checked here, on those values)"""
    import torch

    from bark_amd.optimizer import propose_mes_from_candidates
    from bark_amd.optimizer.thompson_sampling import generate_fstar_samples

    name, S, seed = "prior_n64", 16, 1234
    inp = ar.make_inputs(name)
    fstar = generate_fstar_samples(inp.model, inp.data, inp.ft, num_samples=S, generator=seed)
    assert fstar.shape == (inp.case.B, S)
    mu, var = ar.posterior(name)
    want, bar = tr.acquisition(mu, var, fstar, "mes"), tr.propagated_bar(mu, var, fstar, "mes")
    at, gap = apr.gap_of(want)
    assert gap >= apr.MARGIN and float(bar.max()) < (np.delete(want, at).min() - want[at]) / 2
    row = propose_mes_from_candidates(inp.model, inp.data, inp.cand, inp.ft, num_samples=S, generator=seed)
    assert np.array_equal(row, inp.cand[at])
    value, index, acq = run(scan, name, "mes", targets=fstar)
    used = tr.bar_used(acq, want, bar)
    print(f"{name} mes against {S} f* draws: fraction of the propagated bar used {used:.3g}")
    assert used <= 1.0 and index == at
    cand = torch.from_numpy(inp.cand).cuda()
    trow = propose_mes_from_candidates(inp.model, (torch.from_numpy(inp.X).cuda(), inp.y), cand, inp.ft, num_samples=S,
                                       generator=seed)
    assert trow.is_cuda and np.array_equal(trow.cpu().numpy(), inp.cand[at])


def test_torch_inputs_stay_on_the_device(scan):
    import torch

    from bark_amd.optimizer import propose_batch_from_candidates, propose_from_candidates

    name = "prior_n64"
    inp = ar.make_inputs(name)
    t = tr.targets_of(name)
    value, index, acq = run(scan, name, "ei")
    cand, td = torch.from_numpy(inp.cand).cuda(), torch.from_numpy(np.array(t)).cuda()
    data = (torch.from_numpy(inp.X).cuda(), inp.y)
    tv, ti, tacq = scan(inp.model, data, cand, inp.ft, kind="ei", targets=td, return_values=True)
    assert tv.is_cuda and ti.is_cuda and tacq.is_cuda and ti.dtype == torch.int64
    assert tv.item() == value and ti.item() == index and np.array_equal(tacq.cpu().numpy(), acq)
    row = propose_from_candidates(inp.model, inp.data, cand, inp.ft, kind="ei", targets=td)
    assert row.is_cuda and np.array_equal(row.cpu().numpy(), inp.cand[index])
    assert np.array_equal(propose_from_candidates(inp.model, inp.data, inp.cand, inp.ft, kind="ei", targets=t), inp.cand[index])
    rows, picks = propose_batch_from_candidates(inp.model, data, cand, inp.ft, q=2, kind="ei", targets=td)
    assert rows.is_cuda and picks.is_cuda and picks[0].item() == index and picks[1].item() != index


class Raw:
    """the C entry on the inputs of a case: device buffers, the workspace and the call"""

    def __init__(self, name):
        import torch

        from bark_amd import _lib
        from bark_amd.forest import _feat_types, _points, packed_forest

        self.lib, self._lib, self.torch = _lib.lib(), _lib, torch
        inp = ar.make_inputs(name)
        ft = _feat_types(inp.ft)
        self.pf = packed_forest(inp.F, ft)
        self.Xd, _ = _points(inp.X, ft.shape[0])
        self.cd, _ = _points(inp.cand, ft.shape[0])
        self.yd = _lib.to_device(inp.y.reshape(-1))
        self.nd, self.sd = _lib.to_device(inp.noise), _lib.to_device(inp.scale)
        self.N, self.d = self.Xd.shape
        self.C, self.B = self.cd.shape[0], inp.case.B
        R = int(self.pf.info.max_bits)
        self.ws = _lib.workspace(int(self.lib.bark_acquisition_scan_targets_workspace_bytes(self.N, R, self.pf.m, self.B, self.C, 0)))

    def head(self):
        p = self._lib.ptr
        return (self._lib.ctx(), p(self.pf.packed), self.pf.info_ref, p(self.Xd), self.N, self.d, p(self.yd), p(self.nd),
                p(self.sd), p(self.cd), self.C, None, 0, None, 0)

    def tail(self, info):
        return (info, self._lib.ptr(self.ws), self.ws.numel(), self.B, self._lib.stream_ptr())

    def targets(self, targets, S, kind, acq, best, idx, info, kappa=1.96):
        return self.lib.bark_acquisition_scan_targets_hip(*self.head(), targets, S, kappa, kind, 0, acq, best, idx, *self.tail(info))

    def pending(self, kind, acq, best, idx, info, kappa=1.96):
        return self.lib.bark_acquisition_scan_pending_hip(*self.head(), kappa, kind, 0, acq, best, idx, *self.tail(info))


def test_c_entry_refuses_before_any_launch():
    """kinds 2 - 4 with NULL targets, S = 0 and S = 1025, an unknown kind and a NaN kappa return BARK_ERR_ARG with the outputs
    untouched; the entry points without targets still refuse the target kinds"""
    import torch

    from bark_amd import _lib

    raw = Raw("m2_r65")
    t = _lib.to_device(np.array(tr.targets_of("m2_r65")))
    S = int(t.shape[1])
    wide = torch.zeros((raw.B, 1025), dtype=torch.float64, device="cuda")
    best = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    info = torch.full((raw.B,), 7, dtype=torch.int32, device="cuda")
    outs = (None, _lib.ptr(best), _lib.ptr(idx), _lib.ptr(info))
    for kind in (_lib.ACQ_EI, _lib.ACQ_PI, _lib.ACQ_MES):
        assert raw.targets(None, S, kind, *outs) == _lib.BARK_ERR_ARG
        assert raw.targets(_lib.ptr(t), 0, kind, *outs) == _lib.BARK_ERR_ARG
        assert raw.targets(_lib.ptr(t), -1, kind, *outs) == _lib.BARK_ERR_ARG
        assert raw.targets(_lib.ptr(wide), 1025, kind, *outs) == _lib.BARK_ERR_ARG
        assert raw.targets(_lib.ptr(t), S, kind, *outs, kappa=float("nan")) == _lib.BARK_ERR_ARG
        assert raw.pending(kind, *outs) == _lib.BARK_ERR_ARG
    assert raw.targets(_lib.ptr(t), S, 5, *outs) == _lib.BARK_ERR_ARG
    assert raw.targets(_lib.ptr(t), S, -1, *outs) == _lib.BARK_ERR_ARG
    torch.cuda.synchronize()
    assert best.item() == 7.0 and idx.item() == 7 and (info == 7).all()
    assert raw.targets(_lib.ptr(t), S, _lib.ACQ_EI, *outs) == _lib.BARK_OK
    torch.cuda.synchronize()
    assert idx.item() == int(np.argmin(tr.reference("m2_r65", "ei")[0])) and not info.any()


@pytest.mark.parametrize("kind", [0, 1])
def test_confidence_bounds_through_the_new_entry(kind):
    """kinds 0 / 1 with NULL targets: bark_acquisition_scan_pending_hip, bit for bit"""
    import torch

    from bark_amd import _lib

    raw = Raw("prior_n64")

    def outputs():
        return (torch.zeros(raw.C, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
                torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(raw.B, dtype=torch.int32, device="cuda"))

    a, b = outputs(), outputs()
    assert raw.targets(None, 0, kind, *(_lib.ptr(v) for v in a)) == _lib.BARK_OK
    assert raw.pending(kind, *(_lib.ptr(v) for v in b)) == _lib.BARK_OK
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert np.array_equal(a[0].cpu().numpy(), _scan_values("prior_n64", kind))


def _scan_values(name, kind):
    from bark_amd.optimizer import acquisition_scan

    inp = ar.make_inputs(name)
    return acquisition_scan(inp.model, inp.data, inp.cand, inp.ft, kind=ar.KINDS[kind], return_values=True)[2]


@pytest.mark.parametrize("kind", tr.KINDS)
def test_guard_bands_around_output_and_targets(scan, kind):
    """acq_out and targets inside NaN-filled buffers: C values written, nothing in front of or behind them, and no NaN read
    from around the targets"""
    import torch

    from bark_amd import _lib

    name = "prior_n64"
    raw = Raw(name)
    _, _, acq = run(scan, name, kind)
    t = np.array(tr.targets_of(name))
    C, B, G = raw.C, raw.B, 64
    tbuf = torch.full((t.size + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
    tbuf[G:G + t.size] = torch.from_numpy(t.reshape(-1)).cuda()
    before = tbuf.clone()
    buf = torch.full((C + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
    scal = torch.full((2 * G + 1,), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.full((2 * G + 1,), -77, dtype=torch.int64, device="cuda")
    info = torch.full((B + 2 * G,), -77, dtype=torch.int32, device="cuda")
    rc = raw.targets(tbuf.data_ptr() + 8 * G, t.shape[1], tr_kind(kind), buf.data_ptr() + 8 * G, scal.data_ptr() + 8 * G,
                     idx.data_ptr() + 8 * G, info.data_ptr() + 4 * G)
    assert rc == _lib.BARK_OK
    torch.cuda.synchronize()
    assert torch.equal(tbuf.view(torch.int64), before.view(torch.int64))  # the targets are read only
    buf, scal, idx, info = buf.cpu().numpy(), scal.cpu().numpy(), idx.cpu().numpy(), info.cpu().numpy()
    assert np.isnan(buf[:G]).all() and np.isnan(buf[-G:]).all() and np.array_equal(buf[G:-G], acq)
    assert np.isnan(scal[:G]).all() and np.isnan(scal[G + 1:]).all() and scal[G] == acq.min()
    assert (idx[:G] == -77).all() and (idx[G + 1:] == -77).all() and idx[G] == int(np.argmin(acq))
    assert (info[:G] == -77).all() and (info[-G:] == -77).all() and not info[G:-G].any()


def tr_kind(kind):
    from bark_amd import _lib

    return {"ei": _lib.ACQ_EI, "pi": _lib.ACQ_PI, "mes": _lib.ACQ_MES}[kind]


@pytest.mark.parametrize("kind", tr.KINDS)
def test_nan_target_does_not_win(scan, kind):
    """one NaN among the targets of one forest: every candidate's mean runs over it, so every value is NaN and none wins"""
    name = "prior_n64"
    t = np.array(tr.targets_of(name))
    t[1, 2] = np.nan
    value, index, acq = run(scan, name, kind, targets=t)
    assert np.isnan(acq).all() and np.isnan(value) and index == -1
    good = run(scan, name, kind)  # nothing is left behind
    assert good[1] == int(np.argmin(tr.reference(name, kind)[0]))
