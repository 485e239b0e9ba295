"""The fitted leaf-space posterior (tree_kernels.fit_posterior / LeafPosterior; bark_leaf_posterior_fit_hip,
bark_acquisition_scan_fitted_hip, bark_leaf_posterior_condition_hip) against the project's own stateless path, which has its
reference tests (tests/test_gpu_acquisition*.py).  The claim is identity of bits, not a tolerance: the state holds what the
stateless scan computes before it looks at a candidate, and the same kernels consume it in the same order.  Fit and
stateless call use the same `chunk`.

Shapes: N = 48, d = 4 (two continuous features, one integer, one categorical), B = 5 prior forests of m = 8 trees,
noise 0.1, chunk = 2 (chunks of 2, 2 and 1 forests), C = 700 candidates (two full tiles of 256 and a ragged one), both scan
variants.  The forests are prior-sized, so "global" runs the global scan at the largest R the fixture gives."""
import ctypes

import numpy as np
import pytest

from bark_amd import synthetic

pytestmark = pytest.mark.gpu

N, B, M, C, CHUNK = 48, 5, 8, 700, 2
KINDS = ("lcb_mean", "lcb_mixture", "ei", "pi", "mes")
VARIANTS = ("lds", "global")


class Fixture:
    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        kw = dict(d_cont=2, n_int=1, n_cat=1)
        self.X, self.y, self.bounds, self.ft = synthetic.mixed_problem(N, seed=11, **kw)
        self.cand = synthetic.mixed_problem(C, seed=12, **kw)[0]
        self.pend = synthetic.mixed_problem(3, seed=13, **kw)[0]
        F = synthetic.sample_prior_forests(B, M, self.bounds, self.ft, seed=21)
        self.model = (F, np.full(B, 0.1), np.linspace(0.8, 1.3, B))
        self.data = (self.X, self.y)
        rng = np.random.default_rng(5)
        self.targets = float(self.y.min()) + rng.uniform(-0.5, 0.5, size=(B, 3))  # explicit (B, S = 3) targets
        self.post = fit_posterior(self.model, self.data, self.ft, chunk=CHUNK)

    def stateless(self, cand=None, **kw):
        from bark_amd.optimizer import acquisition_scan

        return acquisition_scan(self.model, self.data, self.cand if cand is None else cand, self.ft, chunk=CHUNK,
                                return_values=True, **kw)

    def fitted(self, cand=None, post=None, **kw):
        return (post or self.post).scan(self.cand if cand is None else cand, return_values=True, **kw)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2].shape == b[2].shape and np.array_equal(a[2], b[2])


def target_cases(fx, kind):
    if kind in ("lcb_mean", "lcb_mixture"):
        return [None]
    return [fx.targets] if kind == "mes" else [None, fx.targets]


def test_object(fx):
    import torch

    p = fx.post
    assert (p.B, p.m, p.d, p.N, p.chunk) == (B, M, 4, N, CHUNK) and p.R == int(p.packed.info.max_bits)
    assert p.nbytes == p.state.numel() and p.state.data_ptr() % 256 == 0
    assert p.info.dtype == torch.int32 and p.info.is_cuda and p.info.shape == (B,) and not p.info.any()
    assert p.train_y_min == float(fx.y.min())
    assert np.array_equal(p.feat_types, fx.ft) and p.noise.is_cuda and p.scale.is_cuda


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_scan_from_the_state_is_the_stateless_scan(fx, kind, variant):
    for targets in target_cases(fx, kind):
        want = fx.stateless(kind=kind, variant=variant, targets=targets)
        got = fx.fitted(kind=kind, variant=variant, targets=targets)
        assert got[2].shape == (C,) and np.isfinite(want[2]).all()
        assert same(got, want), (kind, variant, targets is None)
        # through the keyword of the stateless function, model and data left out
        from bark_amd.optimizer import acquisition_scan

        assert same(acquisition_scan(None, None, fx.cand, None, kind=kind, variant=variant, targets=targets, return_values=True,
                                     posterior=fx.post), want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_pending_and_skip_leave_the_state_alone(fx, kind, variant):
    targets = target_cases(fx, kind)[-1]
    before = fx.fitted(kind=kind, variant=variant, targets=targets)
    state = fx.post.state.clone()
    skip = [int(before[1]), 3]
    want = fx.stateless(kind=kind, variant=variant, targets=targets, pending=fx.pend, skip=skip)
    got = fx.fitted(kind=kind, variant=variant, targets=targets, pending=fx.pend, skip=skip)
    assert same(got, want) and got[1] not in skip
    assert not np.array_equal(got[2], before[2])  # the pending points matter at this shape
    assert bool((fx.post.state == state).all())
    assert same(fx.fitted(kind=kind, variant=variant, targets=targets), before)


@pytest.mark.parametrize("variant", VARIANTS)
def test_condition(fx, variant):
    want = fx.stateless(variant=variant, pending=fx.pend)
    new = fx.post.condition(fx.pend)
    assert new is not fx.post and new.state.data_ptr() != fx.post.state.data_ptr() and new.packed is fx.post.packed
    assert same(fx.fitted(post=new, variant=variant), want)
    assert same(fx.fitted(variant=variant, pending=fx.pend), want)  # out of place inside the scan: the same bits
    twice = fx.post.condition(fx.pend[:2])
    assert twice.condition_(fx.pend[2:]) is twice
    assert bool((twice.state == new.state).all())
    assert same(fx.fitted(post=twice, variant=variant), want)
    # the original is as it was
    assert same(fx.fitted(variant=variant), fx.stateless(variant=variant))
    # a pending point on top of a conditioned state
    assert same(fx.fitted(post=fx.post.condition(fx.pend[:2]), variant=variant, pending=fx.pend[2:]), want)


@pytest.mark.parametrize("kind", ["lcb_mean", "ei"])
def test_greedy_batch(fx, kind):
    from bark_amd.optimizer import propose_batch_from_candidates

    state = fx.post.state.clone()
    want_rows, want_idx = propose_batch_from_candidates(fx.model, fx.data, fx.cand, fx.ft, 4, kind=kind, pending=fx.pend[:1],
                                                        chunk=CHUNK)
    rows, idx = propose_batch_from_candidates(None, None, fx.cand, None, 4, kind=kind, pending=fx.pend[:1], posterior=fx.post)
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx) and len(set(idx.tolist())) == 4
    assert np.array_equal(rows, want_rows)
    assert bool((fx.post.state == state).all())


def test_greedy_batch_on_the_device(fx):
    import torch

    from bark_amd.optimizer import propose_batch_from_candidates

    want_rows, want_idx = propose_batch_from_candidates(fx.model, fx.data, fx.cand, fx.ft, 3, chunk=CHUNK)
    rows, idx = propose_batch_from_candidates(None, None, torch.from_numpy(fx.cand).cuda(), None, 3, posterior=fx.post)
    assert rows.is_cuda and idx.is_cuda and idx.dtype == torch.int64
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(rows.cpu().numpy(), want_rows)
    value, index, acq = fx.post.scan(torch.from_numpy(fx.cand).cuda(), return_values=True)
    assert value.is_cuda and index.is_cuda and acq.is_cuda
    host = fx.fitted()
    assert value.item() == host[0] and index.item() == host[1] and np.array_equal(acq.cpu().numpy(), host[2])


def domain_call(fx, **kw):
    from bark_amd.optimizer import propose_from_domain

    return propose_from_domain(fx.model, fx.data, fx.bounds, fx.ft, return_info=True, chunk=CHUNK, **kw)


def test_domain_enumeration_reuses_the_fit(fx):
    from bark_amd.optimizer import domain_plan, split_table

    grid = domain_plan(split_table(fx.model[0], fx.bounds, fx.ft))["grid"]
    assert 1 < grid <= 2 ** 22  # small enough to be enumerated
    for kw in (dict(), dict(pending=fx.pend, kind="lcb_mixture", round_size=1000)):
        x0, i0 = domain_call(fx, **kw)
        x1, i1 = domain_call(fx, reuse_fit=True, **kw)
        assert i0["exhaustive"] and i1["exhaustive"] and i0["fits"] == i0["scans"] == i1["scans"] and i1["fits"] == 1
        assert np.array_equal(x0, x1) and i0["value"] == i1["value"] and i0["index"] == i1["index"]
    x2, i2 = domain_call(fx, posterior=fx.post)
    x0, i0 = domain_call(fx)
    assert i2["fits"] == 0 and np.array_equal(x0, x2) and i0["value"] == i2["value"]


def test_domain_search_reuses_the_fit(fx):
    kw = dict(exhaustive_limit=1, n_candidates=2048, starts=3, seed=4)
    x0, i0 = domain_call(fx, **kw)
    x1, i1 = domain_call(fx, reuse_fit=True, **kw)
    assert not i0["exhaustive"] and not i1["exhaustive"] and i0["scans"] == i1["scans"] >= 2
    assert i0["fits"] == i0["scans"] and i1["fits"] == 1
    assert np.array_equal(x0, x1) and i0["value"] == i1["value"]
    assert np.array_equal(i0["start_values"], i1["start_values"]) and np.array_equal(i0["final_values"], i1["final_values"])


def test_a_second_candidate_set_of_one(fx):
    for kind in ("lcb_mean", "lcb_mixture"):
        want = fx.stateless(cand=fx.cand[5:6], kind=kind)
        got = fx.fitted(cand=fx.cand[5:6], kind=kind)
        assert got[2].shape == (1,) and got[1] == 0 and same(got, want)
    full = fx.fitted()
    assert fx.fitted(cand=fx.cand[5:6])[0] == full[2][5]


def test_scan_chunk_does_not_matter(fx):
    base = fx.fitted(pending=fx.pend)
    for chunk in (1, 3, 5):
        assert same(fx.fitted(pending=fx.pend, chunk=chunk), base)


def test_python_refusals(fx):
    from bark_amd.optimizer import acquisition_scan

    with pytest.raises(ValueError, match="at most 64 pending"):
        fx.post.scan(fx.cand, pending=np.repeat(fx.pend, 22, axis=0)[:65])
    with pytest.raises(ValueError, match="at most 64 pending"):
        fx.post.condition(np.repeat(fx.pend, 22, axis=0)[:65])
    with pytest.raises(ValueError, match="features"):
        fx.post.scan(fx.cand[:, :3])
    with pytest.raises(ValueError, match="unknown kind"):
        fx.post.scan(fx.cand, kind="ucb")
    with pytest.raises(ValueError, match="unknown variant"):
        fx.post.scan(fx.cand, variant="fast")
    with pytest.raises(ValueError, match="needs targets"):
        fx.post.scan(fx.cand, kind="mes")
    with pytest.raises(TypeError, match="LeafPosterior"):
        acquisition_scan(None, None, fx.cand, None, posterior=object())
    bad = fx.cand.copy()
    bad[699, 3] = -1.0  # the categorical column
    with pytest.raises(ValueError, match="categorical"):
        fx.post.scan(bad)
    assert same(fx.fitted(), fx.stateless())  # the flag is cleared and the state is intact
    pend = fx.pend.copy()
    pend[1, 3] = np.nan
    with pytest.raises(ValueError, match="categorical"):
        fx.post.scan(fx.cand, pending=pend)
    assert not fx.post.info.any() and same(fx.fitted(), fx.stateless())
    broken = fx.post.condition(fx.pend[:1])
    with pytest.raises(ValueError, match="categorical"):
        broken.condition_(pend)
    assert (broken.info == -1).all() and not fx.post.info.any()


def test_c_entries_refuse_before_any_launch(fx):
    """a state buffer one byte short, P = 65, an unknown kind and a target kind without targets return BARK_ERR_ARG with the
    NaN-filled outputs untouched"""
    import torch

    from bark_amd import _lib as L

    lib, p = L.lib(), fx.post
    cd, pd = L.to_device(fx.cand), L.to_device(np.repeat(fx.pend, 22, axis=0)[:65].copy())
    best = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    info = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    need = int(lib.bark_acquisition_scan_fitted_workspace_bytes(p.R, p.m, B, C, 64, 0))
    assert need > 0
    ws = L.workspace(need)

    def scan(state_bytes=p.nbytes, P=0, kind=0, targets=None, S=0):
        return lib.bark_acquisition_scan_fitted_hip(
            L.ctx(), L.ptr(p.packed.packed), p.packed.info_ref, p.d, L.ptr(p.noise), L.ptr(p.scale), L.ptr(p.state), state_bytes,
            L.ptr(cd), C, L.ptr(pd), P, None, 0, L.ptr(targets), S, 1.96, kind, 0, None, L.ptr(best), L.ptr(idx), L.ptr(info),
            L.ptr(ws), ws.numel(), B, L.stream_ptr())

    for kw, message in ((dict(state_bytes=p.nbytes - 1), b"state buffer too small"), (dict(P=65), b"at most 64 pending"),
                        (dict(kind=5), b"unknown kind"), (dict(kind=4), b"needs targets")):
        assert scan(**kw) == L.BARK_ERR_ARG, kw
        assert message in lib.bark_last_error(), (kw, lib.bark_last_error())
    fit_ws = int(lib.bark_leaf_posterior_fit_workspace_bytes(N, p.R, p.m, B))
    ws = L.workspace(max(need, fit_ws))
    Xd, yd = L.to_device(fx.X), L.to_device(fx.y.reshape(-1))
    scratch = torch.empty(p.nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.bark_leaf_posterior_fit_hip(L.ctx(), L.ptr(p.packed.packed), p.packed.info_ref, L.ptr(Xd), N, p.d, L.ptr(yd), L.ptr(p.noise),
                                         L.ptr(p.scale), L.ptr(scratch), p.nbytes - 1, L.ptr(info), L.ptr(ws), ws.numel(), B,
                                         L.stream_ptr())
    assert rc == L.BARK_ERR_ARG and b"state buffer too small" in lib.bark_last_error()
    rc = lib.bark_leaf_posterior_condition_hip(L.ctx(), L.ptr(p.packed.packed), p.packed.info_ref, p.d, L.ptr(p.noise), L.ptr(p.scale),
                                               L.ptr(pd), 65, L.ptr(scratch), p.nbytes, L.ptr(info), L.ptr(ws), ws.numel(), B,
                                               L.stream_ptr())
    assert rc == L.BARK_ERR_ARG and b"at most 64 pending" in lib.bark_last_error()
    torch.cuda.synchronize()
    assert bool(best.isnan().all()) and idx.item() == -77 and bool((info == -77).all())
    assert ctypes.c_size_t(lib.bark_leaf_posterior_bytes(p.R, p.m, B)).value == p.nbytes
