"""Conditioning a fitted posterior on points with observed or fantasised values (LeafPosterior.observe / condition(values=) /
fantasise / log_predictive; bark_leaf_posterior_observe_hip, acq_observe_kernel) against tests/observe_ref.py, against a
refit on the augmented data, and bit for bit against the believer's M^-1.

Cases (observe_ref.NAMES): the PCase bases of acq_pending_ref at the smallest shapes at which the kernel can go wrong — R = 8
with one tree and one point, R = 100, R no multiple of 64, one point twice, leaves no training point reaches, 64 points —
one base of R = 1100 > 1024 leaves (every thread-strided loop takes a second trip) and one of B = 5 forests in chunks of 2
(a ragged last chunk).  The bar is the project's posterior bar (acq_ref.RTOL, ATOL = 1e-9, 1e-8) unless a test says
otherwise.  The host reference lives on the columns the points reach; `host_state` places it on the device's columns (a
column nobody reaches is an identity row of M^-1 and a zero of w)."""
import numpy as np
import pytest

import acq_pending_ref as pr
import acq_ref as ar
import observe_ref as ob
import paths_ref

pytestmark = pytest.mark.gpu

KINDS = ("lcb_mean", "lcb_mixture", "ei", "pi")
SEED, DRAW = 11, 2


class Fixture:
    def __init__(self, name):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.name, self.case = name, ob.case_of(name)
        self.inp = ar.make_inputs(self.case.base)
        self.chunk = self.case.base.chunk
        self.pts, self.vals = ob.points_of(name), ob.values_of(name)
        self.B, self.P = self.inp.F.shape[0], len(self.pts)
        self.post = fit_posterior(self.inp.model, self.inp.data, self.inp.ft, chunk=self.chunk)
        self.R = self.post.R
        every = np.concatenate([self.inp.X, self.inp.cand, self.pts])
        self.dev_cols = paths_ref.leaf_columns(self.inp.F, self.inp.ft, every)[0]  # (B, n, m)
        self.per_forest = self.vals[None, :] + 0.5 * np.arange(self.B)[:, None]
        self.targets = float(self.inp.y.min()) + np.random.default_rng(5).uniform(-0.5, 0.5, size=(self.B, 3))

    def state(self, post):
        return paths_ref.read_state(post.state.cpu().numpy(), self.B, self.R)

    def host_state(self, forests):
        """(M^-1 (B, R, R), w (B, R)) of observe_ref's forests on the device's columns"""
        Minv, w = np.stack([np.eye(self.R)] * self.B), np.zeros((self.B, self.R))
        for b, f in enumerate(forests):
            at = np.empty(f.Minv.shape[0], dtype=np.int64)
            at[np.concatenate(f.cols).ravel()] = self.dev_cols[b].ravel()
            assert len(set(at.tolist())) == at.size
            Minv[b][np.ix_(at, at)] = f.Minv
            w[b, at] = f.w
        return Minv, w

    def mu_sd(self, post, points):
        """the state's predictive mean and standard deviation at the first of `points`, per forest, as the device forms
        them: the values a fantasy returns with eps = 0 and with eps = 1"""
        mu = post.fantasise(points, eps=np.zeros((self.B, len(points))), chunk=self.chunk)[1][:, 0]
        return mu, post.fantasise(points, eps=np.ones((self.B, len(points))), chunk=self.chunk)[1][:, 0] - mu


_cache = {}


def fixture(name) -> Fixture:
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def close(got, want, what):
    used = float((np.abs(got - want) / (ob.ATOL + ob.RTOL * np.abs(want))).max())
    print(f"{what}: fraction of the bar used {used:.3g}")
    assert used <= 1.0, (what, used)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def c_observe(fx, post, points, values=None, *, stride=None, mode=0, eps=None, seed=0, draw=0, Bc=None, P=None, state_bytes=None,
              ws_bytes=None, null_points=False):
    """bark_leaf_posterior_observe_hip itself on post's state -> (rc, values_out (B, P), logpred (B,), info (B,)); the
    outputs start as -77"""
    import ctypes

    import torch

    from bark_amd import _lib as L

    lib = L.lib()
    pd = L.to_device(np.ascontiguousarray(points))
    P = len(points) if P is None else P
    vd = None if values is None else L.to_device(np.ascontiguousarray(values, dtype=np.float64))
    ed = None if eps is None else L.to_device(np.ascontiguousarray(eps, dtype=np.float64))
    if stride is None:
        stride = P if vd is not None and vd.ndim == 2 else 0
    out = torch.full((fx.B, max(len(points), 1)), -77.0, dtype=torch.float64, device="cuda")
    lp = torch.full((fx.B,), -77.0, dtype=torch.float64, device="cuda")
    info = torch.full((fx.B,), -77, dtype=torch.int32, device="cuda")
    Bc = fx.B if Bc is None else Bc
    ws = L.workspace(max(int(lib.bark_leaf_posterior_observe_workspace_bytes(post.R, post.m, Bc, min(max(P, 1), 64))), 256))
    rc = lib.bark_leaf_posterior_observe_hip(
        L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise), L.ptr(post.scale),
        L.ptr(None if null_points else pd), P, L.ptr(vd), stride, mode, L.ptr(ed), ctypes.c_uint64(seed), draw, L.ptr(post.state),
        post.nbytes if state_bytes is None else state_bytes, L.ptr(out), L.ptr(lp), L.ptr(info), L.ptr(ws),
        ws.numel() if ws_bytes is None else ws_bytes, Bc, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:, :len(points)], lp.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name", ob.NAMES)
def test_minv_has_the_bits_of_the_believer(name):
    fx = fixture(name)
    for vals in (fx.vals, fx.per_forest, ob.LIAR):
        seen = fx.post.condition(fx.pts, vals) if np.ndim(vals) != 1 else fx.post.observe(fx.pts, vals, chunk=fx.chunk)
        believer = fx.post.condition(fx.pts)
        (Ma, wa, ia), (Mb, wb, ib) = fx.state(seen), fx.state(believer)
        assert same_bits(Ma, Mb) and not ia.any() and not ib.any()
        assert same_bits(wb, fx.state(fx.post)[1]) and not np.array_equal(wa, wb)  # w moves with the values only
    assert seen.N == fx.post.N and seen.train_y_min == fx.post.train_y_min  # a fantasy is no datum


@pytest.mark.parametrize("name", ob.NAMES)
def test_state_against_the_host_reference(name):
    fx = fixture(name)
    for label, vals in (("(P,)", fx.vals), ("(B, P)", fx.per_forest)):
        want_M, want_w = fx.host_state(ob.sequential(fx.inp, fx.pts, vals)["forests"])
        got_M, got_w, info = fx.state(fx.post.condition(fx.pts, vals))
        assert not info.any()
        close(got_M, want_M, f"{name} {label} M^-1")
        close(got_w, want_w, f"{name} {label} w")


@pytest.mark.parametrize("name", ob.NAMES)
def test_scan_after_observe_against_a_refit(name):
    from bark_amd.tree_kernels import fit_posterior

    fx = fixture(name)
    seen = fx.post.observe(fx.pts, fx.vals, chunk=fx.chunk)
    assert seen is not fx.post and seen.N == fx.post.N + fx.P
    assert seen.train_y_min == min(fx.post.train_y_min, float(fx.vals.min()))
    data = (np.concatenate([fx.inp.X, fx.pts]), np.concatenate([fx.inp.y.reshape(-1), fx.vals]).reshape(-1, 1))
    refit = fit_posterior(fx.inp.model, data, fx.inp.ft, chunk=fx.chunk)
    for kind in KINDS:
        targets = fx.targets if kind in ("ei", "pi") else None
        _, i_got, got = seen.scan(fx.inp.cand, kind=kind, return_values=True, targets=targets)
        _, i_want, want = refit.scan(fx.inp.cand, kind=kind, return_values=True, targets=targets)
        close(got, want, f"{name} {kind}")
        if pr.gap_of(want)[1] >= ob.MARGIN:
            assert i_got == i_want, (name, kind)
    assert i_want == pr.gap_of(want)[0]


def test_slices_and_chunks_change_no_bit():
    fx = fixture("b5_chunk2_p3")
    pts, vals = (np.asarray(v, dtype=np.float64) for v in ar.problem(70, 500)[:2])
    vals = vals.reshape(-1)
    whole = fx.post.observe(pts, vals)
    parts = fx.post.observe(pts[:64], vals[:64]).observe_(pts[64:], vals[64:])
    assert whole.N == parts.N == fx.post.N + 70
    assert bool((whole.state == parts.state).all())
    for chunk in (1, 2, 3):
        assert bool((fx.post.observe(pts, vals.reshape(-1, 1), chunk=chunk).state == whole.state).all()), chunk
    drawn = [fx.post.fantasise(pts[:5], seed=SEED, draw=DRAW, chunk=chunk) for chunk in (None, 2)]
    assert same_bits(drawn[0][1], drawn[1][1]) and bool((drawn[0][0].state == drawn[1][0].state).all())


@pytest.mark.parametrize("name", ob.NAMES)
def test_log_predictive(name):
    import bark_amd.fitting as fit

    fx = fixture(name)
    before = fx.post.state.clone()
    got = fx.post.log_predictive(fx.pts, fx.vals, chunk=fx.chunk)
    assert got.shape == (fx.B,) and bool((fx.post.state == before).all())
    close(got, ob.sequential(fx.inp, fx.pts, fx.vals)["logpred"], f"{name} against the host reference")
    kw = dict(include_scale=True, include_2pi=False)
    Xa, ya = np.concatenate([fx.inp.X, fx.pts]), np.concatenate([fx.inp.y.reshape(-1), fx.vals]).reshape(-1, 1)
    F, noise, scale = fx.inp.model
    want = fit.batched_mll(F, noise, scale, Xa, ya, fx.inp.ft, **kw) - fit.batched_mll(F, noise, scale, fx.inp.X, fx.inp.y, fx.inp.ft, **kw)
    close(got, want, f"{name} against the difference of two MLLs")


@pytest.mark.parametrize("name", ob.NAMES)
def test_fantasies_from_given_normals(name):
    fx = fixture(name)
    eps = np.random.default_rng(17).standard_normal((fx.B, fx.P))
    new, values = fx.post.fantasise(fx.pts, eps=eps, chunk=fx.chunk)
    assert isinstance(values, np.ndarray) and values.shape == (fx.B, fx.P) and new is not fx.post
    ref = ob.sequential(fx.inp, fx.pts, eps=eps)
    close(values, ref["values"], f"{name} values")
    (M1, w1, _), (M2, w2, _) = fx.state(new), fx.state(fx.post.condition(fx.pts, values))
    assert same_bits(M1, M2)
    close(w1, w2, f"{name} w against condition(values=)")
    close(w1, fx.host_state(ref["forests"])[1], f"{name} w against the host reference")


@pytest.mark.parametrize("name", ob.NAMES)
def test_fantasies_from_philox(name):
    import torch

    from bark_amd.fitting import _philox

    fx = fixture(name)
    new, values = fx.post.fantasise(fx.pts, seed=SEED, draw=DRAW, chunk=fx.chunk)
    eps = _philox.fantasy_normals(SEED, np.arange(fx.B), DRAW, fx.P)
    close(values, ob.sequential(fx.inp, fx.pts, eps=eps)["values"], f"{name} values")
    again, values2 = fx.post.fantasise(fx.pts, seed=SEED, draw=DRAW, chunk=fx.chunk)
    assert same_bits(values, values2) and bool((new.state == again.state).all())
    assert not np.array_equal(values, fx.post.fantasise(fx.pts, seed=SEED, draw=DRAW + 1, chunk=fx.chunk)[1])
    assert not np.array_equal(values, fx.post.fantasise(fx.pts, seed=SEED + 1, draw=DRAW, chunk=fx.chunk)[1])
    on_device = fx.post.fantasise(torch.from_numpy(fx.pts).cuda(), seed=SEED, draw=DRAW, chunk=fx.chunk)[1]
    assert on_device.is_cuda and same_bits(on_device.cpu().numpy(), values)


def test_philox_normals_directly():
    """eps = (value - mu) / sqrt(v) of a two-point call on a fresh state, with mu and sqrt(v) taken from the device itself (the
    values that eps = 0 and eps = 1 return), so that only the normal is left: entry 0 (r cos th) from the fresh state, entry 1
    (r sin th) from the state after the first point, which a one-point call with the same (seed, draw) leaves bit for bit.
    Tolerance: the atol 1e-12 of tests/test_gpu_paths.py for path_normals, scaled by 1 / sqrt(v) where that exceeds 1 — the
    subtraction value - mu is exact to an ulp of the value, which the division by sqrt(v) magnifies."""
    from bark_amd.fitting import _philox

    fx = fixture("n64_m13_p2")
    pts = pr.pending_of("pair_ab")
    want = _philox.fantasy_normals(SEED, np.arange(fx.B), DRAW, 2)
    both = fx.post.fantasise(pts, seed=SEED, draw=DRAW)[1]
    first, one = fx.post.fantasise(pts[:1], seed=SEED, draw=DRAW)
    assert same_bits(one[:, 0], both[:, 0])
    for p, state in ((0, fx.post), (1, first)):
        mu, sd = fx.mu_sd(state, pts[p:p + 1])
        got = (both[:, p] - mu) / sd
        tol = 1e-12 * max(1.0, float((1.0 / sd).max()))
        print(f"entry {p}: max |eps - want| {np.abs(got - want[:, p]).max():.3g}, tolerance {tol:.3g}")
        np.testing.assert_allclose(got, want[:, p], rtol=0, atol=tol)


def test_failed_forest():
    """a forest whose status is non-zero (marked as tests/test_gpu_paths.py marks one; the categorical fault of
    tests/test_gpu_posterior_state.py marks every forest of the call, checked in test_python_refusals) is left alone, its rows
    of both outputs are NaN, and the others are what they are without it"""
    fx = fixture("b5_chunk2_p3")
    for Bc in (5, 2):
        good, marked = fx.post._copy(), fx.post._copy()
        marked.info[2] = 9
        rc0, v0, l0, i0 = c_observe(fx, good, fx.pts, mode=1, seed=SEED, draw=DRAW, Bc=Bc)
        rc1, v1, l1, i1 = c_observe(fx, marked, fx.pts, mode=1, seed=SEED, draw=DRAW, Bc=Bc)
        assert rc0 == rc1 == 0 and not i0.any() and i1.tolist() == [0, 0, 9, 0, 0]
        assert np.isnan(v1[2]).all() and np.isnan(l1[2])
        keep = [0, 1, 3, 4]
        assert same_bits(v1[keep], v0[keep]) and same_bits(l1[keep], l0[keep]) and np.isfinite(v0).all() and np.isfinite(l0).all()
        (M0, w0, _), (M1, w1, _), (Mf, wf, _) = fx.state(good), fx.state(marked), fx.state(fx.post)
        assert same_bits(M1[keep], M0[keep]) and same_bits(w1[keep], w0[keep])
        assert same_bits(M1[2], Mf[2]) and same_bits(w1[2], wf[2]) and not same_bits(M0[2], Mf[2])
    with pytest.raises(np.linalg.LinAlgError):
        marked.observe_(fx.pts, fx.vals)


@pytest.mark.parametrize("name", ob.GREEDY)
def test_greedy_batches(name):
    from bark_amd.fitting import _philox
    from bark_amd.optimizer import propose_batch_from_candidates

    fx = fixture(name)
    case, inp = fx.case, fx.inp
    before = fx.post.state.clone()
    normals = lambda b, draw, n: _philox.fantasy_normals(3, [b], [draw], n)[0]  # noqa: E731
    for kind in pr.KINDS:
        for kw, fantasy in ((dict(fantasy=0.0), 0.0), (dict(fantasy="sample", seed=3), "sample")):
            want, gap = ob.greedy(inp, fx.pts, case.q, kind, case.base.kappa, fantasy, normals)
            assert gap >= ob.MARGIN, (name, kind, fantasy, gap)
            rows, idx = propose_batch_from_candidates(None, None, inp.cand, None, case.q, kappa=case.base.kappa, kind=kind, pending=fx.pts,
                                                      posterior=fx.post, **kw)
            print(f"{name} {kind} fantasy={fantasy}: picks {idx.tolist()} host gap {gap:.3g}")
            assert idx.dtype == np.int64 and len(set(idx.tolist())) == case.q and np.array_equal(idx, want)
            assert np.array_equal(rows, inp.cand[want])
        today = propose_batch_from_candidates(inp.model, inp.data, inp.cand, inp.ft, case.q, kappa=case.base.kappa, kind=kind,
                                              pending=fx.pts, chunk=fx.chunk)
        mean = propose_batch_from_candidates(None, None, inp.cand, None, case.q, kappa=case.base.kappa, kind=kind, pending=fx.pts,
                                             posterior=fx.post, fantasy="mean")
        assert np.array_equal(mean[0], today[0]) and np.array_equal(mean[1], today[1])
    assert bool((fx.post.state == before).all())
    with pytest.raises(ValueError, match="fit_posterior"):
        propose_batch_from_candidates(inp.model, inp.data, inp.cand, inp.ft, 2, fantasy=0.0)


def test_python_refusals():
    fx = fixture("n64_m13_p2")
    before = fx.post.state.clone()
    many = np.repeat(fx.pts, 33, axis=0)[:65]
    with pytest.raises(ValueError, match="at most 64"):
        fx.post.condition_(many, 0.0)
    with pytest.raises(ValueError, match="between 1 and 64"):
        fx.post.fantasise(many)
    with pytest.raises(ValueError, match="finite"):
        fx.post.observe_(fx.pts, np.array([0.5, np.nan]))
    with pytest.raises(ValueError, match="finite"):
        fx.post.log_predictive(fx.pts, np.array([np.inf, 0.5]))
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((fx.B, fx.P))):
        with pytest.raises(ValueError, match="values must be"):
            fx.post.observe_(fx.pts, bad)
    for bad in (np.zeros(3), np.zeros((fx.B + 1, fx.P)), np.zeros((fx.P, 1))):
        with pytest.raises(ValueError, match="values must be"):
            fx.post.condition_(fx.pts, bad)
    with pytest.raises(ValueError, match="eps must be"):
        fx.post.fantasise(fx.pts, eps=np.zeros((fx.P, fx.B + 1)))
    for kw in (dict(seed=1.5), dict(draw="0"), dict(seed=True)):
        with pytest.raises(TypeError, match="must be an int"):
            fx.post.fantasise(fx.pts, **kw)
    with pytest.raises(ValueError, match="draw must lie"):
        fx.post.fantasise(fx.pts, draw=-1)
    assert bool((fx.post.state == before).all()) and fx.post.N == 64
    # an invalid categorical value marks the state failed, as condition_ does
    fx = fixture("n257_prior_p5")  # prior forests: they split on the categorical columns, the complete trees above do not
    bad = fx.pts.copy()
    bad[1, -1] = np.nan
    broken = fx.post._copy()
    with pytest.raises(ValueError, match="categorical"):
        broken.observe_(bad, fx.vals)
    assert (broken.info == -1).all() and not fx.post.info.any() and broken.N == 257


def test_c_entry_refuses_before_any_launch():
    from bark_amd import _lib as L

    fx = fixture("n64_m13_p2")
    post = fx.post._copy()
    before = post.state.clone()
    lib = L.lib()
    need = int(lib.bark_leaf_posterior_observe_workspace_bytes(post.R, post.m, fx.B, fx.P))
    many = np.repeat(fx.pts, 33, axis=0)[:65]
    for kw, message in ((dict(null_points=True), b"null argument"), (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                        (dict(stride=1), b"value_stride"), (dict(stride=fx.P + 1), b"value_stride"),
                        (dict(no_values=True), b"needs values"), (dict(state_bytes=post.nbytes - 1), b"state buffer too small"),
                        (dict(draw=-1), b"draw number"), (dict(many=True), b"at most 64")):
        vals = None if kw.pop("no_values", False) else fx.vals
        pts = many if kw.pop("many", False) else fx.pts
        rc, out, lp, info = c_observe(fx, post, pts, None if vals is None else np.resize(vals, len(pts)), **kw)
        assert rc == L.BARK_ERR_ARG and message in lib.bark_last_error(), (kw, lib.bark_last_error())
        assert (out == -77).all() and (lp == -77).all() and (info == -77).all()
    rc, out, lp, info = c_observe(fx, post, fx.pts, fx.vals, ws_bytes=need - 1)
    assert rc == L.BARK_ERR_WORKSPACE and (info == -77).all() and (out == -77).all()
    assert bool((post.state == before).all())
    # P = 0 launches nothing but the copy of the status
    rc, out, lp, info = c_observe(fx, post, fx.pts, fx.vals, P=0)
    assert rc == 0 and not info.any() and (out == -77).all() and (lp == -77).all() and bool((post.state == before).all())


def test_sample_paths_follow_the_data():
    """a path with eps = 0 is the posterior mean's leaf table c w: summed over a candidate's leaves it is c sum w of the NEW w"""
    fx = fixture("n64_m13_p2")
    seen = fx.post.observe(fx.pts, fx.vals)
    paths = seen.sample_paths(1, eps=np.zeros((fx.B, fx.R)))
    got = paths.evaluate(fx.inp.cand[:1])[:, 0]
    close(got, ob.sequential(fx.inp, fx.pts, fx.vals)["mu"][:, 0], "eps = 0 paths at candidate 0")
    assert not np.allclose(got, fx.post.sample_paths(1, eps=np.zeros((fx.B, fx.R))).evaluate(fx.inp.cand[:1])[:, 0], rtol=1e-6, atol=1e-6)
