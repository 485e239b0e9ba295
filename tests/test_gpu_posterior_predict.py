"""Predictions from a fitted posterior on the device (LeafPosterior.predict / scores, predictive_scores(posterior=),
forest_predict(posterior=), propose_mes_from_candidates without model and data; bark_leaf_posterior_predict_hip) against
tests/predict_ref.py and, wherever the orders of the contract make it exact, bit for bit against the scan and the stateless
scores.  The cases are those of tests/acq_ref.py, fitted at the case's chunk; every state is fitted once and shared."""
import numpy as np
import pytest

import acq_ref as ar
import predict_ref as pr
import scores_ref as sr
import weights_ref as wr

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = ("prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit", "m13_past_lds", "m64_r256")
LDS_CASES = ("prior_n64", "prior_n257_chunks", "m13_lds_limit")
CHUNK_CASES = ("prior_n64", "prior_n257_chunks", ar.SLAB_CASE.name)
PROBS = [0.025, 0.5, 0.975]


class Fixture:
    def __init__(self, name):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.name, self.case, self.inp = name, sr.case_of(name), sr.inputs(name)
        self.B, self.x, self.y = self.case.B, self.inp.cand, sr.targets(name)
        self.post = fit_posterior(self.inp.model, self.inp.data, self.inp.ft, chunk=self.case.chunk)
        self._full = None

    @property
    def full(self):
        """predict with everything, equal weights, made once"""
        if self._full is None:
            self._full = self.post.predict(self.x, per_forest=True, quantiles=PROBS)
        return self._full


_cache = {}


def fixture(name) -> Fixture:
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_dict(a, b):
    return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)


def one_hot(B, b):
    w = np.zeros(B)
    w[b] = 1.0
    return w


def within(got, want, bar, what):
    used = float((np.abs(got - want) / bar).max())
    print(f"{what}: {used:.3g} of the bar")
    assert used <= 1.0, (what, used)


def ulps(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)) / np.spacing(np.abs(np.asarray(want, dtype=np.float64)))


# ---- moments and per-forest arrays against the reference ------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_moments_and_forest_arrays(name):
    fx = fixture(name)
    mu, var = pr.forest_moments(name)
    got = fx.full
    within(got["forest_mean"], mu, ar.ATOL + ar.RTOL * np.abs(mu), f"{name} forest_mean")
    within(got["forest_var"], var, ar.ATOL + ar.RTOL * np.abs(var), f"{name} forest_var")
    w = np.full(fx.B, 1.0 / fx.B)
    mean, v = (a.astype(np.float64) for a in pr.two_pass(w, mu, var))
    within(got["mean"], mean, ar.ATOL + ar.RTOL * np.abs(mean), f"{name} mean")
    within(got["var"], v, pr.var_bar(w, mu, var), f"{name} var")
    # the recurrence of the contract on the device's own per-forest arrays: the same bits
    mean_w, var_w = pr.west(w, got["forest_mean"], got["forest_var"])
    assert same_bits(got["mean"], mean_w) and same_bits(got["var"], var_w)


@pytest.mark.parametrize("name", ("prior_n64", "m2_r65"))
def test_observation_adds_the_noise(name):
    fx = fixture(name)
    got = fx.post.predict(fx.x, per_forest=True, observation=True)
    s2 = (1e-6 + fx.inp.noise)[:, None]
    assert same_bits(got["forest_mean"], fx.full["forest_mean"]) and same_bits(got["mean"], fx.full["mean"])
    assert same_bits(got["forest_var"], fx.full["forest_var"] + s2)
    mu, var = pr.forest_moments(name, observation=True)
    w = np.full(fx.B, 1.0 / fx.B)
    within(got["var"], pr.two_pass(w, mu, var)[1].astype(np.float64), pr.var_bar(w, mu, var), f"{name} observation var")


# ---- bit identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHUNK_CASES)
def test_chunks_give_the_same_bits(name):
    fx = fixture(name)
    w = pr.random_weights(fx.B)
    want = fx.post.predict(fx.x, per_forest=True, quantiles=PROBS, weights=w, chunk=fx.B)
    want_s = fx.post.scores(fx.x, fx.y, return_values=True, weights=w, chunk=fx.B)
    for chunk in (1, 2):
        assert same_dict(fx.post.predict(fx.x, per_forest=True, quantiles=PROBS, weights=w, chunk=chunk), want), chunk
        assert same_dict(fx.post.scores(fx.x, fx.y, return_values=True, weights=w, chunk=chunk), want_s), chunk
    # quantiles from the workspace slab (no per-forest output) are those read from forest_out
    assert same_bits(fx.post.predict(fx.x, quantiles=PROBS, weights=w, chunk=2)["quantiles"], want["quantiles"])


@pytest.mark.parametrize("name", LDS_CASES)
def test_variants_give_the_same_bits(name):
    fx = fixture(name)
    want_s = fx.post.scores(fx.x, fx.y, return_values=True, variant="auto")
    for variant in ("lds", "global"):
        assert same_dict(fx.post.predict(fx.x, per_forest=True, quantiles=PROBS, variant=variant), fx.full), variant
        assert same_dict(fx.post.scores(fx.x, fx.y, return_values=True, variant=variant), want_s), variant


def test_lds_variant_past_the_limit_raises():
    fx = fixture("m13_past_lds")
    with pytest.raises(ValueError, match="LDS variant"):
        fx.post.predict(fx.x, variant="lds")
    with pytest.raises(ValueError, match="LDS variant"):
        fx.post.scores(fx.x, fx.y, variant="lds")


@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks", "m2_r65", "m13_past_lds"))
def test_forest_mean_is_the_one_hot_scan(name):
    fx = fixture(name)
    for b in range(fx.B):
        _, _, values = fx.post.scan(fx.x, kappa=0.0, kind="lcb_mean", weights=one_hot(fx.B, b), return_values=True)
        assert same_bits(fx.full["forest_mean"][b], values), b


@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks", "m13_past_lds"))
def test_scores_are_the_stateless_scores(name):
    from bark_amd.tree_kernels import forest_predict, predictive_scores

    fx = fixture(name)
    want = predictive_scores(fx.inp.model, fx.inp.data, fx.x, fx.y, fx.inp.ft, return_values=True, chunk=fx.case.chunk)
    got = fx.post.scores(fx.x, fx.y, return_values=True)
    assert set(got) == set(sr.KEYS) and same_dict(got, want)
    assert same_dict(predictive_scores(None, None, fx.x, fx.y, None, return_values=True, posterior=fx.post), got)
    mu, var = forest_predict(None, None, fx.x, None, posterior=fx.post)
    assert same_bits(mu, fx.full["forest_mean"]) and same_bits(var, fx.full["forest_var"])


def test_torch_points_give_device_tensors():
    import torch

    fx = fixture("m2_r65")
    got = fx.post.predict(torch.from_numpy(fx.x).cuda(), per_forest=True, quantiles=PROBS)
    assert all(v.is_cuda for v in got.values()) and same_dict({k: v.cpu().numpy() for k, v in got.items()}, fx.full)
    many = fx.post.predict(fx.x, quantiles=np.linspace(0.02, 0.98, 19))["quantiles"]  # two calls: 16 + 3 probabilities
    assert many.shape == (19, fx.case.C) and (np.diff(many, axis=0) >= 0).all()


# ---- weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks"))
def test_one_hot_weights_are_that_forest(name):
    fx = fixture(name)
    for b in range(fx.B):
        got = fx.post.predict(fx.x, quantiles=PROBS, weights=one_hot(fx.B, b))
        mu, var = fx.full["forest_mean"][b], fx.full["forest_var"][b]
        assert same_bits(got["mean"], mu) and ulps(got["var"], var).max() <= 2
        for q, p in enumerate(PROBS):
            assert ulps(got["quantiles"][q], mu + pr.zscore(p) * np.sqrt(var)).max() <= 4, (b, p)


def c_predict(post, x, weights, *, per_forest=True):
    """the C entry point on post's state, nothing raised -> (rc, moments (2, C), forest (2, B, C), info (B,))"""
    import torch

    from bark_amd import _lib as L

    lib = L.lib()
    xd = L.to_device(np.ascontiguousarray(x))
    C, B = int(xd.shape[0]), post.B
    wd = None if weights is None else L.to_device(np.ascontiguousarray(weights, dtype=np.float64))
    mom = torch.full((2, C), -77.0, dtype=torch.float64, device="cuda")
    fo = torch.full((2, B, C), -77.0, dtype=torch.float64, device="cuda") if per_forest else None
    info = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    ws = L.workspace(int(lib.bark_leaf_posterior_predict_workspace_bytes(post.R, post.m, B, B, C, 0, int(per_forest), 0, 0)))
    rc = lib.bark_leaf_posterior_predict_hip(L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise),
                                             L.ptr(post.scale), L.ptr(post.state), post.nbytes, L.ptr(xd), C, L.ptr(wd), 0, L.ptr(None),
                                             L.ptr(None), L.ptr(None), 0, 0, L.ptr(mom), L.ptr(fo), L.ptr(None), L.ptr(None),
                                             L.ptr(None), L.ptr(None), L.ptr(info), L.ptr(ws), ws.numel(), B, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, mom.cpu().numpy(), None if fo is None else fo.cpu().numpy(), info.cpu().numpy()


def test_failed_forest_counts_only_with_weight():
    fx = fixture("prior_n257_chunks")
    marked = fx.post._copy()
    marked.info[2] = 9
    w = np.array([0.4, 0.1, 0.0, 0.3, 0.2])
    rc, mom, fo, info = c_predict(marked, fx.x, w)
    assert rc == 0 and info.tolist() == [0, 0, 9, 0, 0] and np.isfinite(mom).all()  # reported, not fatal
    assert same_dict(dict(zip(("mean", "var"), mom)), {k: fx.post.predict(fx.x, weights=w)[k] for k in ("mean", "var")})
    assert np.isnan(fo[:, 2]).all()
    got = marked.predict(fx.x, weights=w, quantiles=PROBS)  # the Python layer raises nothing either
    assert np.isfinite(got["quantiles"]).all()
    live = np.array([0.4, 0.1, 0.1, 0.2, 0.2])
    rc, mom, fo, info = c_predict(marked, fx.x, live)
    assert rc == 0 and info.tolist() == [0, 0, 9, 0, 0] and np.isnan(mom).all() and np.isnan(fo[:, 2]).all()
    keep = [0, 1, 3, 4]
    assert same_bits(fo[0][keep], fx.full["forest_mean"][keep]) and same_bits(fo[1][keep], fx.full["forest_var"][keep])
    rc, mom, _, _ = c_predict(marked, fx.x, None, per_forest=False)  # equal weights: every forest counts
    assert rc == 0 and np.isnan(mom).all()
    with pytest.raises(np.linalg.LinAlgError):
        marked.predict(fx.x, weights=live)
    with pytest.raises(np.linalg.LinAlgError):
        marked.scores(fx.x, fx.y, weights="equal")


@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks", "m13_lds_limit"))
def test_random_weights_against_the_reference(name):
    fx = fixture(name)
    w = pr.random_weights(fx.B)
    mu, var = pr.forest_moments(name)
    got = fx.post.predict(fx.x, weights=w)
    mean, v = (a.astype(np.float64) for a in pr.two_pass(w, mu, var))
    within(got["mean"], mean, ar.ATOL + ar.RTOL * np.abs(mean), f"{name} weighted mean")
    within(got["var"], v, pr.var_bar(w, mu, var), f"{name} weighted var")
    # weights_ref.mixture at kappa = 1 is mean - sd of the same mixture
    lcb = wr.mixture(w, mu, var, 1.0).astype(np.float64)
    sd_bar = pr.var_bar(w, mu, var) / (2 * np.sqrt(v))
    within(got["mean"] - np.sqrt(got["var"]), lcb, ar.ATOL + ar.RTOL * np.abs(mean) + sd_bar, f"{name} against weights_ref.mixture")


# ---- weighted scores -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("observation", (False, True))
@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks", "m13_lds_limit"))
def test_weighted_scores_against_the_reference(name, observation):
    fx = fixture(name)
    w = pr.random_weights(fx.B)
    A = sr.precheck(name)
    mu, var = pr.forest_moments(name, observation)
    want = pr.scores(w, mu, var, fx.y)
    got = fx.post.scores(fx.x, fx.y, weights=w, observation=observation, return_values=True)
    for k in sr.KEYS:
        within(got[k], want[k], A * (ar.ATOL + ar.RTOL * np.abs(want[k])), f"{name} {k} observation={observation}")
    if observation:  # the two calls differ by exactly the added s2_b
        plain = fx.post.predict(fx.x, per_forest=True)
        noisy = fx.post.predict(fx.x, per_forest=True, observation=True)
        assert same_bits(noisy["forest_var"], plain["forest_var"] + (1e-6 + fx.inp.noise)[:, None])
        again = pr.scores(w, noisy["forest_mean"], noisy["forest_var"], fx.y)
        for k in sr.KEYS:
            assert np.allclose(got[k], again[k], rtol=1e-12, atol=1e-12), k


# ---- quantiles ---------------------------------------------------------------------------------------------------------
ERFC_ULP = 8  # allowance for the device erfc's error, in units of 2^-53 of F


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks"))
def test_quantiles_solve_the_device_mixture(name, weighted):
    fx = fixture(name)
    B = fx.B
    w = pr.random_weights(B) if weighted else np.full(B, 1.0 / B)
    got = fx.post.predict(fx.x, per_forest=True, quantiles=PROBS, weights=w) if weighted else fx.full
    mu, var, t = got["forest_mean"], got["forest_var"], got["quantiles"]
    for q, p in enumerate(PROBS):
        resid = np.abs(pr.cdf(t[q], w, mu, var) - LD(p)).astype(np.float64)
        bar = (ERFC_ULP + B) * 2.0 ** -53 + 4 * np.spacing(np.abs(t[q])) * pr.pdf(t[q], w, mu, var).astype(np.float64)
        used = float((resid / bar).max())
        print(f"{name} p={p} weighted={weighted}: |F(t) - p| uses {used:.3g} of the bar, largest residual {resid.max():.3g}")
        assert used <= 1.0, (name, p, used)
    assert (np.diff(t, axis=0) >= 0).all()
    assert (t[1] >= mu.min(axis=0)).all() and (t[1] <= mu.max(axis=0)).all()
    # against the reference posterior's quantiles
    mu_r, var_r = pr.forest_moments(name)
    for q, p in enumerate(PROBS):
        want = pr.quantile(p, w, mu_r, var_r).astype(np.float64)
        within(t[q], want, (1 + abs(pr.zscore(p))) * (ar.ATOL + ar.RTOL * np.abs(want)), f"{name} quantile {p} against the reference")


def test_one_forest_one_point_quantile():
    fx = fixture("m1_r64")
    got = fx.full
    assert got["quantiles"].shape == (3, 1)
    for q, p in enumerate(PROBS):
        want = got["forest_mean"][0] + pr.zscore(p) * np.sqrt(got["forest_var"][0])
        assert same_bits(got["quantiles"][q], want), p


# ---- MES without model and data ----------------------------------------------------------------------------------------
def test_mes_from_the_state_alone():
    from bark_amd.optimizer import propose_mes_from_candidates

    fx = fixture("prior_n64")
    post = fx.post._copy()
    cand = fx.x[:300]

    def targets_of(p):
        values, _ = p.sample_paths(8, seed=3).minimise(cand)
        return values.reshape(p.B, 8)

    T = targets_of(post)
    row, info = propose_mes_from_candidates(None, None, cand, fx.inp.ft, posterior=post, num_samples=8, seed=3, return_info=True)
    value, index = post.scan(cand, kind="mes", targets=T)
    assert info["index"] == index and same_bits(info["value"], value) and same_bits(info["targets"].cpu().numpy(), T)
    assert np.array_equal(row, cand[index])
    assert np.array_equal(propose_mes_from_candidates(None, None, cand, None, posterior=post, num_samples=8, seed=3), row)
    # with model and data the draws are still generate_fstar_samples': the unchanged path, through the same scan
    import torch

    from bark_amd.optimizer import acquisition_scan
    from bark_amd.optimizer.thompson_sampling import generate_fstar_samples

    site_x = torch.as_tensor(fx.inp.X, device="cuda")
    fstar = generate_fstar_samples(fx.inp.model, (site_x, fx.inp.y), fx.inp.ft, num_samples=8, generator=5)
    _, idx = acquisition_scan(fx.inp.model, fx.inp.data, cand, fx.inp.ft, kind="mes", targets=fstar, posterior=post)
    old = propose_mes_from_candidates(fx.inp.model, fx.inp.data, cand, fx.inp.ft, num_samples=8, generator=5, posterior=post)
    assert np.array_equal(old, cand[idx])
    # the draws follow the state
    x_new, y_new = ar.problem(3, 4242)[:2]
    post.observe_(x_new, y_new)
    T2 = targets_of(post)
    assert not np.array_equal(T2, T)
    _, info2 = propose_mes_from_candidates(None, None, cand, None, posterior=post, num_samples=8, seed=3, return_info=True)
    assert same_bits(info2["targets"].cpu().numpy(), T2)
