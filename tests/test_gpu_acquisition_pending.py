"""Acquisition scan conditioned on pending points (bark_acquisition_scan_pending_hip, acq_condition_kernel) and the greedy
batch built on it, against the host reference of tests/acq_pending_ref.py: the oracle's dense `forest_predict` on the
training inputs augmented by the pending points.

Bars: values to the posterior bar of DESIGN.md section 2 (rtol 1e-9, atol 1e-8); indices equal
(tests/test_acquisition_pending_cpu.py establishes on the host that every winner, at every greedy pick, is separated by a
relative gap of 1e-6); chunking, the kernel variant, a repeated call and P = 0 against the existing entry point bit for
bit; the two orders of a pair of pending points to the value bar only, as documented."""
import numpy as np
import pytest

import acq_pending_ref as pr
import acq_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scan():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd.optimizer import acquisition_scan

    return acquisition_scan


def run(scan, name, kind="lcb_mean", pending="case", **kw):
    case = pr.CASES[name]
    inp = ar.make_inputs(case.base)
    if isinstance(pending, str):
        pending = pr.pending_of(name)
    return scan(inp.model, inp.data, inp.cand, inp.ft, kappa=case.base.kappa, kind=kind, return_values=True, pending=pending, **kw)


def bar_used(got, want):
    return float((np.abs(got - want) / (pr.ATOL + pr.RTOL * np.abs(want))).max())


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("name", pr.CONDITIONING + pr.AWKWARD)
def test_conditioning_against_the_dense_reference(scan, name, kind):
    want, at = pr.conditioned(name)[kind]
    value, index, acq = run(scan, name, kind)
    assert acq.shape == (300,) and acq.dtype == np.float64
    used = bar_used(acq, want)
    print(f"{name} {kind}: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    assert index == at and value == acq[at]


@pytest.mark.parametrize("kind", pr.KINDS)
def test_conditioning_changes_the_values(scan, kind):
    """the pending points matter at these shapes: without them the vector misses the conditioned reference"""
    want, _ = pr.conditioned("p64")[kind]
    assert bar_used(run(scan, "p64", kind, pending=None)[2], want) > 1e3


@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("name", ["n257_prior_p5", "p64"])
def test_chunks_variants_and_repeats_are_bit_identical(scan, name, kind):
    base = run(scan, name, kind)
    for kw in (dict(), dict(chunk=1), dict(chunk=2), dict(chunk=3), dict(variant="lds"), dict(variant="global"),
               dict(variant="global", chunk=2)):
        assert same(run(scan, name, kind, **kw), base), kw


@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("name", ["n20_m1_p1", "n257_prior_p5"])
def test_no_pending_points_is_the_existing_entry_point(scan, name, kind):
    """P = 0 (and an empty skip list) through bark_acquisition_scan_pending_hip against bark_acquisition_scan_hip"""
    inp = ar.make_inputs(pr.CASES[name].base)
    old = scan(inp.model, inp.data, inp.cand, inp.ft, kind=kind, return_values=True)
    assert same(run(scan, name, kind, pending=np.empty((0, inp.X.shape[1]))), old)
    assert same(run(scan, name, kind, pending=None, skip=[]), old)


@pytest.mark.parametrize("kind", pr.KINDS)
def test_order_of_pending_points(scan, kind):
    ab, ba = run(scan, "pair_ab", kind), run(scan, "pair_ba", kind)
    used = bar_used(ab[2], ba[2])
    print(f"pair {kind}: fraction of the bar between the two orders {used:.3g}, bit-identical: {np.array_equal(ab[2], ba[2])}")
    assert used <= 1.0 and ab[1] == ba[1]
    assert bar_used(ab[2], pr.conditioned("pair_ab")[kind][0]) <= 1.0


@pytest.mark.parametrize("kind", pr.KINDS)
def test_candidate_slabs(scan, kind):
    """C = 70 000: two slabs of candidates under two chunks of forests, the conditioned matrix shared by both"""
    case = pr.SLAB
    inp = ar.make_inputs(case.base)
    pend = pr.pending_of(case)
    value, index, acq = scan(inp.model, inp.data, inp.cand, inp.ft, kappa=case.base.kappa, kind=kind, return_values=True,
                             pending=pend, chunk=case.base.chunk)
    assert acq.shape == (case.base.C,)
    assert index == int(np.argmin(acq)) and value == acq[index]
    rows = np.unique(np.append(np.arange(0, case.base.C, pr.SLAB_STRIDE), index))
    mu, var = pr.dense(inp, pend, inp.cand[rows])
    used = bar_used(acq[rows], ar.acquisition(mu, var, case.base.kappa, kind))
    print(f"{case.name} {kind}: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    mu, var, _ = pr.leafspace(inp, pend)  # the whole vector: ties between candidates that share their leaves, lowest index
    assert index == pr.gap_of(ar.acquisition(mu, var, case.base.kappa, kind))[0]


@pytest.mark.parametrize("kind", pr.KINDS)
def test_skip(scan, kind):
    name = "n64_m13_p2"
    want, at = pr.conditioned(name)[kind]
    base = run(scan, name, kind)
    assert base[1] == at
    second = pr.gap_of(want, [at])[0]
    for skip in ([at], np.array([at, at]), [299, at, 0]):
        value, index, acq = run(scan, name, kind, skip=skip)
        assert np.array_equal(acq, base[2])
        runner = pr.gap_of(want, list(skip))[0]
        assert index == runner and value == acq[runner]
    assert run(scan, name, kind, skip=[at])[1] == second
    # without pending points too
    inp = ar.make_inputs(pr.CASES[name].base)
    v0, i0, a0 = scan(inp.model, inp.data, inp.cand, inp.ft, kind=kind, return_values=True)
    v1, i1, a1 = scan(inp.model, inp.data, inp.cand, inp.ft, kind=kind, return_values=True, skip=[i0])
    assert np.array_equal(a0, a1) and i1 == pr.gap_of(a0, [i0])[0] and v1 == a0[i1]


def test_every_candidate_skipped(scan):
    inp = ar.make_inputs(pr.CASES["n64_m13_p2"].base)
    pend = pr.pending_of("n64_m13_p2")
    full = scan(inp.model, inp.data, inp.cand[:64], inp.ft, return_values=True, pending=pend)
    value, index, acq = scan(inp.model, inp.data, inp.cand[:64], inp.ft, return_values=True, pending=pend, skip=np.arange(64))
    assert np.isnan(value) and index == -1 and np.array_equal(acq, full[2])
    with pytest.raises(ValueError, match="at most 64"):
        scan(inp.model, inp.data, inp.cand, inp.ft, skip=np.arange(65))
    for bad in ([300], [-1]):
        with pytest.raises(ValueError, match="skip indices"):
            scan(inp.model, inp.data, inp.cand, inp.ft, skip=bad)
    with pytest.raises(ValueError, match="at most 64 pending"):
        scan(inp.model, inp.data, inp.cand, inp.ft, pending=np.concatenate([pr.pending_of("p64"), pend[:1]]))


@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("name", pr.GREEDY)
def test_greedy_batch(scan, name, kind):
    from bark_amd.optimizer import propose_batch_from_candidates

    case = pr.CASES[name]
    inp = ar.make_inputs(case.base)
    picks, vecs, pends = pr.greedy(name, kind)
    rows, idx = propose_batch_from_candidates(inp.model, inp.data, inp.cand, inp.ft, case.q, kappa=case.base.kappa, kind=kind,
                                              pending=pr.pending_of(name))
    assert idx.dtype == np.int64 and np.array_equal(idx, picks), (idx, picks)
    assert len(set(idx.tolist())) == case.q
    assert np.array_equal(rows, inp.cand[picks])
    value, index, acq = scan(inp.model, inp.data, inp.cand, inp.ft, kappa=case.base.kappa, kind=kind, return_values=True,
                             pending=pends[-1], skip=picks[:-1])
    used = bar_used(acq, vecs[-1])
    print(f"{name} {kind}: fraction of the bar used at the last pick {used:.3g}")
    assert used <= 1.0 and index == picks[-1]


def test_torch_inputs_stay_on_the_device(scan):
    import torch

    from bark_amd.optimizer import propose_batch_from_candidates

    name = "greedy_q4_n64"
    case = pr.CASES[name]
    inp = ar.make_inputs(case.base)
    picks, _, pends = pr.greedy(name, "lcb_mean")
    cand = torch.from_numpy(inp.cand).cuda()
    pend = torch.from_numpy(pr.pending_of(name)).cuda()
    rows, idx = propose_batch_from_candidates(inp.model, inp.data, cand, inp.ft, case.q, pending=pend)
    assert rows.is_cuda and idx.is_cuda and idx.dtype == torch.int64 and rows.shape == (case.q, inp.cand.shape[1])
    assert np.array_equal(idx.cpu().numpy(), picks) and np.array_equal(rows.cpu().numpy(), inp.cand[picks])
    host = scan(inp.model, inp.data, inp.cand, inp.ft, return_values=True, pending=pends[-1], skip=picks[:-1])
    tv, ti, tacq = scan(inp.model, inp.data, cand, inp.ft, return_values=True, pending=torch.from_numpy(pends[-1]).cuda(),
                        skip=idx[:-1])
    assert tv.is_cuda and ti.is_cuda and tacq.is_cuda
    assert tv.item() == host[0] and ti.item() == host[1] and np.array_equal(tacq.cpu().numpy(), host[2])
    # without pending points of the caller's
    rows2, idx2 = propose_batch_from_candidates(inp.model, inp.data, cand, inp.ft, 2)
    assert idx2[0].item() == scan(inp.model, inp.data, inp.cand, inp.ft)[1] and idx2[0].item() != idx2[1].item()


def test_invalid_categorical_value_in_a_pending_point(scan):
    name = "n257_prior_p5"
    inp = ar.make_inputs(pr.CASES[name].base)
    cat = int(np.flatnonzero(np.asarray(inp.ft) == 0)[0])
    pend = pr.pending_of(name).copy()
    pend[3, cat] = -1.0
    with pytest.raises(ValueError, match="categorical"):
        scan(inp.model, inp.data, inp.cand, inp.ft, pending=pend, chunk=2)
    assert run(scan, name, chunk=2)[1] == pr.conditioned(name)["lcb_mean"][1]  # the flag is cleared


class Raw:
    """the C entry on the inputs of a case, outputs inside guard bands"""

    G = 64

    def __init__(self, name):
        import torch

        from bark_amd import _lib
        from bark_amd.forest import _feat_types, _points, packed_forest

        self.torch, self.L, self.lib = torch, _lib, _lib.lib()
        case = pr.CASES[name]
        inp = ar.make_inputs(case.base)
        ft = _feat_types(inp.ft)
        self.pf = packed_forest(inp.F, ft)
        self.Xd, _ = _points(inp.X, ft.shape[0])
        self.cd, _ = _points(inp.cand, ft.shape[0])
        self.pd, _ = _points(np.concatenate([pr.pending_of(name)] * 40)[:65], ft.shape[0])  # 65 rows: one past the limit
        self.yd = _lib.to_device(inp.y.reshape(-1))
        self.nd, self.sd = _lib.to_device(inp.noise), _lib.to_device(inp.scale)
        self.N, self.d = self.Xd.shape
        self.C, self.B, self.kappa = self.cd.shape[0], case.base.B, case.base.kappa
        self.R = int(self.pf.info.max_bits)
        G = self.G
        self.buf = torch.full((self.C + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
        self.scal = torch.full((2 * G + 1,), float("nan"), dtype=torch.float64, device="cuda")
        self.idx = torch.full((2 * G + 1,), -77, dtype=torch.int64, device="cuda")
        self.info = torch.full((self.B + 2 * G,), -77, dtype=torch.int32, device="cuda")
        self.skip = torch.zeros(65, dtype=torch.int64, device="cuda")
        self.ws = _lib.workspace(int(self.lib.bark_acquisition_scan_pending_workspace_bytes(self.N, self.R, self.pf.m, self.B, self.C, 64)))

    def call(self, P, n_skip=0):
        L, G = self.L, self.G
        return self.lib.bark_acquisition_scan_pending_hip(
            L.ctx(), L.ptr(self.pf.packed), self.pf.info_ref, L.ptr(self.Xd), self.N, self.d, L.ptr(self.yd), L.ptr(self.nd),
            L.ptr(self.sd), L.ptr(self.cd), self.C, L.ptr(self.pd), P, L.ptr(self.skip), n_skip, self.kappa, 0, 0,
            self.buf.data_ptr() + 8 * G, self.scal.data_ptr() + 8 * G, self.idx.data_ptr() + 8 * G,
            self.info.data_ptr() + 4 * G, L.ptr(self.ws), self.ws.numel(), self.B, L.stream_ptr())

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool(self.buf.isnan().all() and self.scal.isnan().all() and (self.idx == -77).all() and (self.info == -77).all())


def test_c_entry_refuses_and_writes_inside_its_outputs_only(scan):
    """P = 65, a negative P and n_skip = 65 return BARK_ERR_ARG before any launch: the NaN-filled outputs stay as they were.
    A good call writes C values, one scalar, one index and B status words, and nothing in front of or behind them."""
    name = "n64_m13_p2"
    raw = Raw(name)
    for P, n_skip in ((65, 0), (-1, 0), (2, 65), (2, -1)):
        assert raw.call(P, n_skip) == raw.L.BARK_ERR_ARG, (P, n_skip)
        assert b"at most 64 pending" in raw.lib.bark_last_error()
    assert raw.untouched()
    _, _, acq = run(scan, name)
    assert raw.call(2) == raw.L.BARK_OK
    raw.torch.cuda.synchronize()
    G = raw.G
    buf, scal, idx, info = raw.buf.cpu().numpy(), raw.scal.cpu().numpy(), raw.idx.cpu().numpy(), raw.info.cpu().numpy()
    assert np.isnan(buf[:G]).all() and np.isnan(buf[-G:]).all() and np.array_equal(buf[G:-G], acq)
    assert np.isnan(scal[:G]).all() and np.isnan(scal[G + 1:]).all() and scal[G] == acq.min()
    assert (idx[:G] == -77).all() and (idx[G + 1:] == -77).all() and idx[G] == int(np.argmin(acq))
    assert (info[:G] == -77).all() and (info[-G:] == -77).all() and not info[G:-G].any()


def test_call_is_capturable(scan):
    """the call only enqueues (no allocation, no host synchronisation): captured once, replayed twice, the eager bits"""
    name = "n64_m13_p2"
    raw = Raw(name)
    torch = raw.torch
    _, _, acq = run(scan, name)
    assert raw.call(2) == raw.L.BARK_OK  # eager first: the one-off set-up of the library is not part of a capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = raw.call(2)
    assert rc == raw.L.BARK_OK
    for _ in range(2):
        raw.buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(raw.buf.cpu().numpy()[raw.G:-raw.G], acq)
        assert raw.idx[raw.G].item() == int(np.argmin(acq)) and not raw.info[raw.G:-raw.G].any()
