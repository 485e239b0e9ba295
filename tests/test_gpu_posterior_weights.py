"""Importance weights of the forest samples of a fitted posterior (LeafPosterior.log_weights / reweight_ / observe_(reweight=) /
subset / resample / scan(weights=); bark_forest_weights_hip, bark_acquisition_scan_fitted_weighted_hip,
bark_leaf_posterior_gather_hip) against tests/weights_ref.py and, wherever the algebra is exact, bit for bit against the
unweighted scan of a subset.

Shapes, the smallest at which each piece can go wrong: B = 5 prior forests of m = 3 trees in chunks of 2 (a `first` chunk and a
ragged last one) on N = 24 points of the mixed cont / int / cat problem, C = 300 candidates (two scan tiles, the second
ragged).  Seed 41 gives forests of 5, 8, 8, 8 and 9 leaves — R = 9, odd, and a subset narrower than the state; seed 44 gives
R = 10, even.  One case of 4 complete trees of 32 leaves (R = 128) puts the scan's LDS image past 64 KiB."""
import numpy as np
import pytest

import acq_ref as ar
import observe_ref as ob
import paths_ref
import weights_ref as wr

pytestmark = pytest.mark.gpu

KINDS = ("lcb_mean", "lcb_mixture", "ei", "pi", "mes")
SUM_KINDS = ("lcb_mean", "ei", "pi", "mes")
VARIANTS = ("lds", "global")
CASES = {"odd": ar.Case("weights_r9", ("prior", 3), N=24, B=5, C=300, chunk=2, seed=41),
         "even": ar.Case("weights_r10", ("prior", 3), N=24, B=5, C=300, chunk=2, seed=44),
         "r128": ar.Case("weights_r128", ("full", 4, 5), N=24, B=2, C=300, seed=45)}
EPS = float(np.finfo(np.float64).eps)


class Fixture:
    def __init__(self, name):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.case = CASES[name]
        self.inp = ar.make_inputs(self.case)
        self.B, self.kappa = self.case.B, self.case.kappa
        self.post = fit_posterior(self.inp.model, self.inp.data, self.inp.ft, chunk=self.case.chunk)
        self.R = self.post.R
        self.pending = np.asarray(ar.problem(2, 777)[0], dtype=np.float64)
        self.skip = [5, 299]
        self.targets = float(self.inp.y.min()) + np.random.default_rng(5).uniform(-0.5, 0.5, size=(self.B, 3))
        self._one = {}

    def one(self, k):
        """subset([k]), made once"""
        if k not in self._one:
            self._one[k] = self.post.subset([k])
        return self._one[k]

    def scan_kw(self, kind, rows=None, extras=False):
        rows = slice(None) if rows is None else rows
        kw = dict(kind=kind, kappa=self.kappa, return_values=True)
        if kind in ("ei", "pi", "mes"):
            kw["targets"] = self.targets[rows]
        if extras:
            kw.update(pending=self.pending, skip=self.skip)
        return kw

    def state(self, post):
        return paths_ref.read_state(post.state.cpu().numpy(), post.B, post.R)


_cache = {}


def fixture(name) -> Fixture:
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_scan(got, want):
    return same_bits(got[0], want[0]) and got[1] == want[1] and same_bits(got[2], want[2])


def c_scan(post, cand, kind, variant, *, weighted, weights=None, targets=None, kappa=1.96, Bc=None):
    """one of the two C entry points on post's state -> (rc, best, index, values (C,), info (B,))"""
    import torch

    from bark_amd import _lib as L
    from bark_amd.optimizer.acquisition import KINDS as K, VARIANTS as V

    lib = L.lib()
    cd = L.to_device(np.ascontiguousarray(cand))
    C = int(cd.shape[0])
    td = None if targets is None else L.to_device(np.ascontiguousarray(targets))
    wd = None if weights is None else L.to_device(np.ascontiguousarray(weights, dtype=np.float64))
    acq = torch.full((C,), -77.0, dtype=torch.float64, device="cuda")
    best = torch.full((), -77.0, dtype=torch.float64, device="cuda")
    idx = torch.full((), -77, dtype=torch.int64, device="cuda")
    info = torch.full((post.B,), -77, dtype=torch.int32, device="cuda")
    Bc = post.B if Bc is None else Bc
    need = lib.bark_acquisition_scan_fitted_weighted_workspace_bytes if weighted else lib.bark_acquisition_scan_fitted_workspace_bytes
    ws = L.workspace(int(need(post.R, post.m, Bc, C, 0, V[variant])))
    front = (L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise), L.ptr(post.scale), L.ptr(post.state),
             post.nbytes, L.ptr(cd), C, L.ptr(None), 0, L.ptr(None), 0, L.ptr(td), 0 if td is None else int(td.shape[1]), float(kappa),
             K[kind], V[variant])
    back = (L.ptr(acq), L.ptr(best), L.ptr(idx), L.ptr(info), L.ptr(ws), ws.numel(), Bc, L.stream_ptr())
    if weighted:
        rc = lib.bark_acquisition_scan_fitted_weighted_hip(*front, L.ptr(wd), *back)
    else:
        rc = lib.bark_acquisition_scan_fitted_hip(*front, *back)
    torch.cuda.synchronize()
    return rc, float(best.item()), int(idx.item()), acq.cpu().numpy(), info.cpu().numpy()


EXTRAS = {"plain": {}, "pending": dict(pending=True), "skip": dict(skip=True), "pending_skip": dict(pending=True, skip=True)}


@pytest.mark.parametrize("extras", sorted(EXTRAS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_hot_weights_are_the_scan_of_that_forest(variant, extras):
    """1.0 t and 0.0 + t are exact, a skipped forest adds nothing and nothing is divided: bit for bit.  Pending points and
    skipped candidates alone and together; the target kinds with S = 3 targets per forest and, for "ei" and "pi", without
    any (the default target, the `train_y_min` that `subset` carries over)."""
    fx = fixture("odd")
    more = {}
    if EXTRAS[extras].get("pending"):
        more["pending"] = fx.pending
    if EXTRAS[extras].get("skip"):
        more["skip"] = fx.skip
    for kind in KINDS:
        for k in range(fx.B):
            got = fx.post.scan(fx.inp.cand, variant=variant, weights=np.eye(fx.B)[k], **fx.scan_kw(kind), **more)
            want = fx.one(k).scan(fx.inp.cand, variant=variant, **fx.scan_kw(kind, slice(k, k + 1)), **more)
            assert same_scan(got, want), (kind, k)
            assert np.isfinite(got[2]).all()
            if kind in ("ei", "pi"):
                kw = dict(kind=kind, return_values=True, variant=variant, **more)
                assert fx.one(k).train_y_min == fx.post.train_y_min
                default = fx.post.scan(fx.inp.cand, weights=np.eye(fx.B)[k], **kw)
                assert same_scan(default, fx.one(k).scan(fx.inp.cand, **kw)), (kind, k, "default target")
                assert not same_bits(default[2], got[2])


def test_general_weights():
    """sum kinds: sum_b w_b v_b in forest order, v_b the one-forest scans.  The device runs the same multiplies and adds in
    the same order; allowing for a fused multiply-add per term the bound is 2 B 2^-52 sum_b |w_b v_b| per candidate.
    lcb_mixture: the weighted moments in longdouble from the device's per-forest (mu, var), at the bar of the unweighted
    check (tests/test_gpu_acquisition.py:36-37 and :69: ar.ATOL + ar.RTOL |want|, used fraction <= 1)."""
    from bark_amd.tree_kernels import forest_predict

    fx = fixture("odd")
    raw = np.random.default_rng(3).uniform(0.1, 1.0, size=fx.B)
    raw[1] = 0.0
    w = raw / raw.sum()
    for kind in SUM_KINDS:
        per = np.stack([fx.one(b).scan(fx.inp.cand, **fx.scan_kw(kind, slice(b, b + 1)))[2] for b in range(fx.B)])
        want, mag = wr.combine(w, per)
        best, index, got = fx.post.scan(fx.inp.cand, weights=raw, **fx.scan_kw(kind))
        bound = 2 * fx.B * 2.0 ** -52 * mag
        print(f"{kind}: max |got - want| / bound {float((np.abs(got - want) / bound).max()):.3g}")
        assert (np.abs(got - want) <= bound).all(), kind
        assert index == int(np.argmin(got)) and best == got[index]
    mu, var = forest_predict(fx.inp.model, fx.inp.data, fx.inp.cand, fx.inp.ft)
    want = wr.mixture(w, mu, var, fx.kappa).astype(np.float64)
    got = fx.post.scan(fx.inp.cand, weights=raw, **fx.scan_kw("lcb_mixture"))[2]
    used = float((np.abs(got - want) / (ar.ATOL + ar.RTOL * np.abs(want))).max())
    print(f"lcb_mixture: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    equal = fx.post.scan(fx.inp.cand, weights=None, **fx.scan_kw("lcb_mixture"))[2]
    assert not np.allclose(got, equal, rtol=1e-6, atol=1e-6)  # the weights matter


def test_no_weights_keeps_its_bits():
    fx = fixture("odd")
    for kind in KINDS:
        tg = fx.targets if kind in ("ei", "pi", "mes") else None
        for variant in VARIANTS:
            old = c_scan(fx.post, fx.inp.cand, kind, variant, weighted=False, targets=tg, kappa=fx.kappa, Bc=2)
            new = c_scan(fx.post, fx.inp.cand, kind, variant, weighted=True, weights=None, targets=tg, kappa=fx.kappa, Bc=2)
            assert old[0] == new[0] == 0 and same_scan(old[1:4], new[1:4]) and not old[4].any() and not new[4].any(), (kind, variant)
        plain = fx.post.scan(fx.inp.cand, **fx.scan_kw(kind))
        assert fx.post.log_weights is None and same_scan(plain, old[1:4])
        assert same_scan(fx.post.scan(fx.inp.cand, weights=None, **fx.scan_kw(kind)), plain)
        # a state with weights, told to ignore them
        tilted = fx.post._copy()
        tilted.reweight_(np.linspace(0.0, -3.0, fx.B))
        assert same_scan(tilted.scan(fx.inp.cand, weights=None, **fx.scan_kw(kind)), plain)
        state = tilted.scan(fx.inp.cand, **fx.scan_kw(kind))
        assert not same_bits(state[2], plain[2])
    assert fx.post.log_weights is None


def test_chunks_change_no_bit():
    fx = fixture("odd")
    raw = np.array([0.3, 0.0, 0.2, 0.4, 0.1])
    for kind in KINDS:
        for extras in (False, True):
            runs = [fx.post.scan(fx.inp.cand, weights=raw, chunk=chunk, **fx.scan_kw(kind, None, extras)) for chunk in (1, 2, 5)]
            assert same_scan(runs[0], runs[1]) and same_scan(runs[0], runs[2]), (kind, extras)


def test_zero_weight_ignores_a_failed_forest():
    """the status word marked directly, as tests/test_gpu_paths.py and tests/test_gpu_posterior_observe.py mark one"""
    fx = fixture("odd")
    marked = fx.post._copy()
    marked.info[2] = 9
    keep = [0, 1, 3, 4]
    rest = fx.post.subset(keep)
    w = np.array([0.25, 0.25, 0.0, 0.25, 0.25])  # sums to 1 exactly: the host normalisation changes no bit
    for kind in KINDS:
        for variant in VARIANTS:
            got = marked.scan(fx.inp.cand, variant=variant, weights=w, **fx.scan_kw(kind))
            want = rest.scan(fx.inp.cand, variant=variant, weights=np.full(4, 0.25), **fx.scan_kw(kind, keep))
            assert same_scan(got, want) and np.isfinite(got[2]).all() and got[1] >= 0, (kind, variant)
        tg = fx.targets if kind in ("ei", "pi", "mes") else None
        rc, best, index, values, info = c_scan(marked, fx.inp.cand, kind, "lds", weighted=True, weights=w, targets=tg, kappa=fx.kappa)
        assert rc == 0 and info.tolist() == [0, 0, 9, 0, 0] and index == got[1] and same_bits(best, got[0])  # reported, not fatal
        live = np.array([0.2, 0.2, 0.2, 0.2, 0.2])
        rc, best, index, values, info = c_scan(marked, fx.inp.cand, kind, "lds", weighted=True, weights=live, targets=tg, kappa=fx.kappa)
        assert rc == 0 and np.isnan(best) and index == -1 and info.tolist() == [0, 0, 9, 0, 0]
        rc, best, index, values, info = c_scan(marked, fx.inp.cand, kind, "lds", weighted=False, targets=tg, kappa=fx.kappa)
        assert rc == 0 and np.isnan(best) and index == -1
    with pytest.raises(np.linalg.LinAlgError):
        marked.scan(fx.inp.cand, weights=live)
    with pytest.raises(np.linalg.LinAlgError):
        marked.scan(fx.inp.cand)


def test_lds_table_past_64_kib():
    """R = 128: tri + R = 8384 doubles, 67 072 bytes of image in front of the leaf lists — a weighted LDS instantiation whose
    limit was not raised fails to launch exactly here"""
    from bark_amd.optimizer import acquisition_plan

    fx = fixture("r128")
    assert fx.R == 128 and acquisition_plan(fx.R, 4, "lds")["lds_bytes"] > 64 * 1024
    targets = float(fx.inp.y.min()) + np.array([[0.1, -0.2, 0.3], [0.0, 0.2, -0.1]])
    for kind in KINDS:
        kw = dict(kind=kind, return_values=True, weights=[0.75, 0.25])
        if kind in ("ei", "pi", "mes"):
            kw["targets"] = targets
        assert same_scan(fx.post.scan(fx.inp.cand, variant="lds", **kw), fx.post.scan(fx.inp.cand, variant="global", **kw)), kind


@pytest.mark.parametrize("B", [5, 1000])
def test_weight_kernel_against_the_restatement(B):
    """exp and log of the device library against numpy's, a handful of operations each: 8 ulp of the largest weight for the
    weights, 8 ulp of each statistic's own size for the statistics"""
    import torch

    from bark_amd import _lib as L
    from bark_amd.tree_kernels import forest_weights

    rng = np.random.default_rng(B)
    inc = np.linspace(0.0, -800.0, B)[rng.permutation(B)]
    log_w = np.log(rng.dirichlet(np.ones(B)))
    info = np.zeros(B, dtype=np.int32)
    info[[1, B - 1]] = (4, -1)
    inc_d, lw_d, info_d = L.to_device(inc), L.to_device(log_w), L.to_device(info)
    for lw_h, lw in ((None, None), (log_w, lw_d)):
        got_l, got_w, got_s = forest_weights(lw, inc_d, info_d)
        want_l, want_w, want_s = wr.update(lw_h, inc, info)
        got_l, got_w = got_l.cpu().numpy(), got_w.cpu().numpy()
        top = float(want_w.max())
        print(f"B = {B}: max |w - want| / ulp(max w) {float(np.abs(got_w - want_w).max() / (EPS * top)):.3g}, "
              f"|stats - want| {np.abs(got_s - want_s)} of {want_s}")
        assert np.abs(got_w - want_w).max() <= 8 * EPS * top
        assert (np.abs(got_s - want_s) <= 8 * EPS * np.array([max(1.0, abs(want_s[0])), want_s[1], want_s[2]])).all()
        assert (got_w[[1, B - 1]] == 0).all() and np.isneginf(got_l[[1, B - 1]]).all()
        assert np.array_equal(np.isneginf(got_l), np.isneginf(want_l)) and (got_w == 0).sum() >= 2
        fine = np.isfinite(want_l)
        assert np.abs(got_l[fine] - want_l[fine]).max() <= 8 * EPS * max(1.0, float(np.abs(want_l[fine]).max()))
        again = forest_weights(lw, inc_d, info_d)
        assert same_bits(again[0].cpu().numpy(), got_l) and same_bits(again[1].cpu().numpy(), got_w) and same_bits(again[2], got_s)
    if B == 1000:
        assert (got_w[info == 0] == 0).any()  # some weights underflow to exactly 0, which is allowed
    dead = forest_weights(lw_d, inc_d, torch.ones_like(info_d))
    assert dead[2][0] == -np.inf and np.isnan(dead[2][1:]).all() and bool(torch.isnan(dead[0]).all()) and bool(torch.isnan(dead[1]).all())


def test_all_dead_keeps_state_and_weights():
    fx = fixture("odd")
    post = fx.post._copy()
    post.reweight_(np.linspace(0.0, -2.0, fx.B))
    before_w, before_s, before_z = post.log_weights.clone(), post.state.clone(), post.log_normaliser
    with pytest.raises(ValueError, match="no forest is left"):
        post.reweight_(np.full(fx.B, -np.inf))
    post.info[:] = 3
    with pytest.raises(ValueError, match="no forest is left"):
        post.reweight_(np.zeros(fx.B))
    post.info[:] = 0
    assert bool((post.log_weights == before_w).all()) and bool((post.state == before_s).all()) and post.log_normaliser == before_z
    # dead forests stay dead through observe_: with one live forest the update leaves it all the weight, exactly
    lone = fx.post._copy()
    lone.log_weights = post.log_weights.new_tensor([-np.inf, 0.0, -np.inf, -np.inf, -np.inf])
    x, y = np.asarray(ar.problem(3, 500)[0], dtype=np.float64), np.array([0.1, -0.3, 0.2])
    assert same_bits(lone.observe(x, y, reweight=True).weights.cpu().numpy(), np.eye(fx.B)[1])


def test_reweight_through_observe():
    """the same kernel, the same slices of 64 points and the same sums as log_predictive: bit for bit"""
    import bark_amd.fitting as fit
    from bark_amd import _lib as L
    from bark_amd.tree_kernels import forest_weights

    fx = fixture("odd")
    pts, vals = (np.asarray(v, dtype=np.float64) for v in ar.problem(73, 500)[:2])
    vals = vals.reshape(-1)
    post = fx.post._copy()
    log_w_h, X, y = None, fx.inp.X, np.asarray(fx.inp.y, dtype=np.float64).reshape(-1)
    for lo, hi in ((0, 3), (3, 73)):
        x, v = pts[lo:hi], vals[lo:hi]
        lp = post.log_predictive(x, v, chunk=2)
        want = forest_weights(post.log_weights, L.to_device(lp), post.info)
        plain = post.observe(x, v)
        assert post.observe_(x, v, reweight=True, chunk=2) is post
        assert same_bits(post.log_weights.cpu().numpy(), want[0].cpu().numpy()) and post.log_normaliser == float(want[2][0])
        assert same_bits(post.weights.cpu().numpy(), want[1].cpu().numpy())
        assert bool((post.state == plain.state).all()) and post.N == plain.N and post.train_y_min == plain.train_y_min
        ref_l, ref_w, ref_s = wr.update(log_w_h, lp)
        assert abs(post.log_normaliser - ref_s[0]) <= 8 * EPS * max(1.0, abs(ref_s[0]))
        assert abs(post.ess - ref_s[1]) <= 8 * EPS * ref_s[1] * fx.B
        # the dense oracle: log_w_new + log Z - log_w_old is the forest's MLL(data + new) - MLL(data), at log_predictive's bar
        Xa, ya = np.concatenate([X, x]), np.concatenate([y, v])
        F, noise, scale = fx.inp.model
        kw = dict(include_scale=True, include_2pi=False)
        diff = (fit.batched_mll(F, noise, scale, Xa, ya.reshape(-1, 1), fx.inp.ft, **kw)
                - fit.batched_mll(F, noise, scale, X, y.reshape(-1, 1), fx.inp.ft, **kw))
        got = post.log_weights.cpu().numpy() + post.log_normaliser - (0.0 if log_w_h is None else log_w_h)
        used = float((np.abs(got - diff) / (ob.ATOL + ob.RTOL * np.abs(diff))).max())
        print(f"points {lo}:{hi}: ess {post.ess:.3g}, fraction of the bar used against the dense MLLs {used:.3g}")
        assert used <= 1.0
        log_w_h, X, y = post.log_weights.cpu().numpy(), Xa, ya
    assert fx.post.log_weights is None
    assert fx.post.observe(pts[:3], vals[:3]).log_weights is None  # the default leaves the call as it was
    seen = fx.post.observe(pts[:3], vals[:3], reweight=True)
    assert seen.log_weights is not None and seen.condition(pts[3:5]).log_weights is seen.log_weights
    assert seen.fantasise(pts[3:5])[0].log_weights is seen.log_weights


@pytest.mark.parametrize("name", ["odd", "even", "r128"])
def test_gather_and_subset(name):
    fx = fixture(name)
    index = [3, 0, 3, 4] if fx.B == 5 else [1, 1, 0]
    assert fx.R % 2 == (1 if name == "odd" else 0)
    sub = fx.post.subset(index)
    assert sub.B == len(index) and sub.R == fx.R and sub.log_weights is None
    (M0, w0, i0), (M1, w1, i1) = fx.state(fx.post), fx.state(sub)
    assert same_bits(M1, M0[index]) and same_bits(w1, w0[index]) and np.array_equal(i1, i0[index])
    assert same_bits(sub.noise.cpu().numpy(), fx.inp.noise[index]) and same_bits(sub.scale.cpu().numpy(), fx.inp.scale[index])
    assert np.array_equal(sub.forest, fx.inp.F[index])
    marked = fx.post._copy()
    marked.info[index[0]] = 7
    assert fx.state(marked.subset(index))[2].tolist() == [7 if b == index[0] else 0 for b in index]
    whole = fx.post.subset(range(fx.B))
    for kind in ("lcb_mean", "lcb_mixture"):
        assert same_scan(whole.scan(fx.inp.cand, kind=kind, return_values=True), fx.post.scan(fx.inp.cand, kind=kind, return_values=True))


def test_gather_refusals():
    import torch

    from bark_amd import _lib as L

    fx = fixture("odd")
    lib, post = L.lib(), fx.post
    out = torch.empty(post.nbytes, dtype=torch.uint8, device="cuda")
    before = post.state.clone()
    good = L.to_device(np.array([0, 1], dtype=np.int64))
    stream = L.stream_ptr()
    for idx, n, dst, message in ((L.to_device(np.array([0, 5], dtype=np.int64)), 2, out, b"outside"),
                                 (L.to_device(np.array([-1], dtype=np.int64)), 1, out, b"outside"),
                                 (good, 2, post.state, b"overlap"), (good, 0, out, b"bad shape"), (None, 2, out, b"null argument")):
        rc = lib.bark_leaf_posterior_gather_hip(L.ptr(post.state), post.B, post.R, L.ptr(idx), n, L.ptr(dst), stream)
        assert rc == L.BARK_ERR_ARG and message in lib.bark_last_error(), (message, lib.bark_last_error())
    assert bool((post.state == before).all())


def test_resample():
    fx = fixture("odd")
    post = fx.post._copy()
    post.reweight_(np.array([-0.3, -np.inf, -1.5, 0.0, -0.7]))
    w = post.weights.cpu().numpy()
    assert w[1] == 0 and abs(post.ess - 1 / (w * w).sum()) <= 8 * EPS * fx.B
    index = wr.systematic(w, 7, 1)
    new = post.resample(n=7, seed=1)
    assert new.B == 7 and new.log_weights is None and 1 not in index.tolist() and new.ess == 7.0
    assert np.array_equal(new.forest, fx.inp.F[index]) and same_bits(new.noise.cpu().numpy(), fx.inp.noise[index])
    sub = post.subset(index)
    assert sub.log_weights is not None and abs(float(sub.weights.sum().item()) - 1.0) <= 8 * EPS
    for kind in ("lcb_mean", "lcb_mixture", "ei"):
        kw = dict(kind=kind, return_values=True)
        assert same_scan(new.scan(fx.inp.cand, **kw), sub.scan(fx.inp.cand, weights=None, **kw)), kind
    assert post.resample(seed=1).B == fx.B and post.log_weights is not None
    with pytest.raises(ValueError, match="weight 0"):
        post.subset([1, 1])


def test_consumers_follow_the_state_weights():
    import torch

    from bark_amd.optimizer import propose_batch_from_candidates, propose_from_candidates, propose_from_domain
    from bark_amd.optimizer.thompson_sampling import propose_thompson_from_candidates

    fx = fixture("odd")
    bounds = ar.problem(fx.case.N, 100 + fx.case.seed)[2]
    for k in (0, 4):
        hot = fx.post._copy()
        hot.log_weights = torch.log(torch.from_numpy(np.eye(fx.B)[k])).cuda()
        alone = fx.one(k)
        assert hot.ess == 1.0 and np.array_equal(hot.live_forest, fx.inp.F[k:k + 1])
        for kind in ("lcb_mean", "ei"):
            got = propose_batch_from_candidates(None, None, fx.inp.cand, None, 3, kind=kind, posterior=hot)
            want = propose_batch_from_candidates(None, None, fx.inp.cand, None, 3, kind=kind, posterior=alone)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (k, kind)
            got = propose_batch_from_candidates(None, None, fx.inp.cand, None, 3, kind=kind, posterior=hot, fantasy="sample", seed=2)
            assert got[1].shape == (3,) and len(set(got[1].tolist())) == 3
        assert np.array_equal(propose_from_candidates(None, None, fx.inp.cand, None, posterior=hot),
                              propose_from_candidates(None, None, fx.inp.cand, None, posterior=alone))
        got = propose_from_domain(None, None, bounds, fx.inp.ft, posterior=hot)
        want = propose_from_domain(None, None, bounds, fx.inp.ft, posterior=alone)
        assert np.array_equal(np.asarray(got), np.asarray(want)), k
        index, info = propose_thompson_from_candidates(None, None, fx.inp.cand, None, 6, seed=3, posterior=hot, return_info=True)
        assert info["forest"].tolist() == [k] * 6 and index.shape == (6,)
    index, info = propose_thompson_from_candidates(None, None, fx.inp.cand, None, 6, seed=3, posterior=fx.post, return_info=True)
    assert np.array_equal(info["forest"], np.random.default_rng(3).integers(0, fx.B, size=6))  # no weights: the uniform draw
