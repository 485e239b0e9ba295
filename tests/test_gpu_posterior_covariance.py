"""The joint covariance from a fitted posterior on the device (LeafPosterior.covariance; bark_leaf_posterior_covariance_hip)
against tests/covariance_ref.py and, wherever the orders of the contract make it exact, bit for bit against itself and the
other readers of the state.  The cases are those of tests/acq_ref.py, fitted at the case's chunk; every state is fitted once
and shared, and no test modifies a shared state."""
from functools import lru_cache

import numpy as np
import pytest

import acq_ref as ar
import covariance_ref as cr
import predict_ref as pr

pytestmark = pytest.mark.gpu

TI, TJ = cr.TI, cr.TJ
TRUTH_CASES = ("m1_r64", "m2_r65", "m13_lds_limit", "m13_past_lds", "m64_r128", "prior_n257_chunks")
LDS_CASES = ("prior_n64", "m13_lds_limit", "m64_r128")


class Fixture:
    def __init__(self, name):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.name, self.case, self.inp = name, ar.CASES[name], ar.make_inputs(name)
        self.B = self.case.B
        self.i1, self.i2 = cr.CASE_POINTS[name]
        self.x1, self.x2 = self.inp.cand[self.i1], self.inp.cand[self.i2]
        self.post = fit_posterior(self.inp.model, self.inp.data, self.inp.ft, chunk=self.case.chunk)
        self._full = None

    @property
    def full(self):
        """(mixture, forest) of the general call at the case's points, equal weights, made once"""
        if self._full is None:
            self._full = self.post.covariance(self.x1, self.x2, per_forest=True)
        return self._full


@lru_cache(maxsize=None)
def fixture(name) -> Fixture:
    return Fixture(name)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def within(got, want, bar, what):
    used = float((np.abs(got - want) / bar).max())
    print(f"{what}: {used:.3g} of the bar")
    assert used <= 1.0, (what, used)


def close(a, b):
    return np.allclose(a, b, rtol=cr.ORDER_TOL, atol=cr.ORDER_TOL)


def one_hot(B, b):
    w = np.zeros(B)
    w[b] = 1.0
    return w


# ---- against the dense reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("name", TRUTH_CASES)
def test_against_the_dense_truth(name, weighted):
    fx = fixture(name)
    want = cr.truth(name, fx.i1, fx.i2)
    w = pr.random_weights(fx.B) if weighted else np.full(fx.B, 1.0 / fx.B)
    mix, forest = fx.post.covariance(fx.x1, fx.x2, per_forest=True, weights=w, chunk=fx.case.chunk) if weighted else fx.full
    assert forest.shape == want.shape and mix.shape == want.shape[1:]
    within(forest, want, cr.forest_bar(name), f"{name} per forest")
    mu1, mu2 = cr.mu_of(name, fx.i1), cr.mu_of(name, fx.i2)
    within(mix, cr.mixture(w, want, mu1, mu2).astype(np.float64), cr.mixture_bar(name, w, mu1, mu2), f"{name} mixture weighted={weighted}")
    # the header's forest-order sum on the device's own blocks and predict's own means: two orders of the same numbers at most
    p1 = fx.post.predict(fx.x1, per_forest=True, weights=w)
    p2 = fx.post.predict(fx.x2, per_forest=True, weights=w)
    assert close(mix, cr.mixture_order(w, forest, p1["forest_mean"], p1["mean"], p2["forest_mean"], p2["mean"]))


# ---- tile edges -------------------------------------------------------------------------------------------------------
EDGE_1, EDGE_2 = np.arange(0, 2 * TI + 3), np.arange(40, 40 + 2 * TJ + 3)


@lru_cache(maxsize=None)
def edge_reference():
    ref = cr.two_stage("prior_n64", EDGE_1, EDGE_2)
    ref.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def edge_whole():
    fx = fixture("prior_n64")
    return fx.post.covariance(fx.inp.cand[EDGE_1], fx.inp.cand[EDGE_2], per_forest=True)


@pytest.mark.parametrize("C2", (1, TJ - 1, TJ, TJ + 1, 2 * TJ + 3))
@pytest.mark.parametrize("C1", (1, TI - 1, TI, TI + 1, 2 * TI + 3))
def test_tile_edges(C1, C2):
    fx = fixture("prior_n64")
    mix, forest = fx.post.covariance(fx.inp.cand[EDGE_1[:C1]], fx.inp.cand[EDGE_2[:C2]], per_forest=True)
    assert forest.shape == (fx.B, C1, C2) and mix.shape == (C1, C2)
    within(forest, edge_reference()[:, :C1, :C2], cr.forest_bar("prior_n64"), f"edges {C1} x {C2}")
    # an entry does not know the shape of the call it was computed in
    whole_mix, whole = edge_whole()
    assert same_bits(forest, whole[:, :C1, :C2]) and same_bits(mix, whole_mix[:C1, :C2])


# ---- bit identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", (False, True))
@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks"))
def test_chunks_give_the_same_bits(name, symmetric):
    fx = fixture(name)
    w = pr.random_weights(fx.B)
    x2 = None if symmetric else fx.x2
    want = fx.post.covariance(fx.x1, x2, per_forest=True, weights=w, chunk=fx.B)
    for chunk in (1, 2):
        got = fx.post.covariance(fx.x1, x2, per_forest=True, weights=w, chunk=chunk)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), chunk
        # the mixture alone goes through the chunk's blocks in the workspace
        assert same_bits(fx.post.covariance(fx.x1, x2, weights=w, chunk=chunk), want[0]), chunk


@pytest.mark.parametrize("name", LDS_CASES)
def test_variants_give_the_same_bits(name):
    fx = fixture(name)
    want = fx.post.covariance(fx.x1, fx.x2, per_forest=True, variant="auto")
    sym = fx.post.covariance(fx.x1, per_forest=True, observation=True)
    for variant in ("lds", "global"):
        got = fx.post.covariance(fx.x1, fx.x2, per_forest=True, variant=variant)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), variant
        got = fx.post.covariance(fx.x1, per_forest=True, observation=True, variant=variant)
        assert same_bits(got[0], sym[0]) and same_bits(got[1], sym[1]), variant


def test_lds_variant_past_the_limit_raises():
    fx = fixture("m13_past_lds")
    with pytest.raises(ValueError, match="LDS variant"):
        fx.post.covariance(fx.x1, fx.x2, variant="lds")
    assert same_bits(fx.post.covariance(fx.x1, fx.x2, variant="global"), fx.full[0])


# ---- the symmetric call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, C", [("prior_n64", 2 * TJ + 3), ("prior_n64", TI + 1), ("prior_n64", TJ), ("m2_r65", 5), ("m1_r64", 1),
                                     ("m13_past_lds", TJ + 1)])
def test_symmetric_call(name, C):
    fx = fixture(name)
    x = fx.inp.cand[:C]
    w = pr.random_weights(fx.B)
    mix, forest = fx.post.covariance(x, per_forest=True, weights=w)
    assert forest.shape == (fx.B, C, C)
    assert same_bits(mix, mix.T) and same_bits(forest, forest.transpose(0, 2, 1))
    gmix, gforest = fx.post.covariance(x, x, per_forest=True, weights=w)
    assert same_bits(np.tril(forest), np.tril(gforest)) and same_bits(np.tril(mix), np.tril(gmix))
    assert close(gforest, gforest.transpose(0, 2, 1))  # the other triangle: the other order of the same sums
    p = fx.post.predict(x, per_forest=True, weights=w)
    assert close(np.diagonal(forest, axis1=1, axis2=2), p["forest_var"]) and close(np.diagonal(mix), p["var"])
    # observation noise: exactly s2_b on the per-forest diagonal, nothing off it
    omix, oforest = fx.post.covariance(x, per_forest=True, weights=w, observation=True)
    want = forest.copy()
    k = np.arange(C)
    want[:, k, k] = forest[:, k, k] + (1e-6 + fx.inp.noise)[:, None]
    assert same_bits(oforest, want)
    po = fx.post.predict(x, weights=w, observation=True)
    off = ~np.eye(C, dtype=bool)
    assert close(np.diagonal(omix), po["var"]) and same_bits(omix[off], mix[off])
    with pytest.raises(ValueError, match="share no noise"):
        fx.post.covariance(x, x, observation=True)


# ---- weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks"))
def test_one_hot_weights_are_that_forest(name):
    fx = fixture(name)
    sym = fx.post.covariance(fx.x1, per_forest=True)[1]
    for b in range(fx.B):
        mix, forest = fx.post.covariance(fx.x1, fx.x2, per_forest=True, weights=one_hot(fx.B, b))
        assert same_bits(mix, fx.full[1][b]) and same_bits(forest[b], fx.full[1][b]), b
        assert np.isnan(np.delete(forest, b, axis=0)).all()
        assert same_bits(fx.post.covariance(fx.x1, weights=one_hot(fx.B, b)), sym[b]), b


def c_covariance(post, x1, x2, weights, *, forest=True, mixture=True):
    """the C entry point on post's state, nothing raised -> (rc, mixture (C1, C2), forest (B, C1, C2), info (B,))"""
    import torch

    from bark_amd import _lib as L

    lib = L.lib()
    x1d = L.to_device(np.ascontiguousarray(x1))
    x2d = None if x2 is None else L.to_device(np.ascontiguousarray(x2))
    C1, B = int(x1d.shape[0]), post.B
    C2 = C1 if x2d is None else int(x2d.shape[0])
    wd = None if weights is None else L.to_device(np.ascontiguousarray(weights, dtype=np.float64))
    mix = torch.full((C1, C2), -77.0, dtype=torch.float64, device="cuda") if mixture else None
    fo = torch.full((B, C1, C2), -77.0, dtype=torch.float64, device="cuda") if forest else None
    info = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    need = int(lib.bark_leaf_posterior_covariance_workspace_bytes(post.R, post.m, B, B, C1, C2, int(x2d is None), 1, 1, 0))
    ws = L.workspace(need)
    rc = lib.bark_leaf_posterior_covariance_hip(L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise),
                                                L.ptr(post.scale), L.ptr(post.state), post.nbytes, L.ptr(x1d), C1, L.ptr(x2d), C2,
                                                L.ptr(wd), 0, 0, L.ptr(fo), L.ptr(mix), L.ptr(info), L.ptr(ws), ws.numel(), B,
                                                L.stream_ptr())
    torch.cuda.synchronize()
    return rc, None if mix is None else mix.cpu().numpy(), None if fo is None else fo.cpu().numpy(), info.cpu().numpy()


def test_zero_weight_and_failed_forests():
    fx = fixture("prior_n257_chunks")
    full = fx.full[1]
    w = np.array([0.4, 0.1, 0.0, 0.3, 0.2])
    mix, forest = fx.post.covariance(fx.x1, fx.x2, per_forest=True, weights=w)
    keep = [0, 1, 3, 4]
    assert np.isnan(forest[2]).all() and same_bits(forest[keep], full[keep])
    # the forest of weight 0 does not enter: the four others alone give the same mixture
    p1, p2 = fx.post.predict(fx.x1, per_forest=True, weights=w), fx.post.predict(fx.x2, per_forest=True, weights=w)
    assert close(mix, cr.mixture_order(w, full, p1["forest_mean"], p1["mean"], p2["forest_mean"], p2["mean"]))
    # a failed forest poisons the mixture only when it has weight
    marked = fx.post._copy()
    marked.info[2] = 9
    rc, cmix, cforest, info = c_covariance(marked, fx.x1, fx.x2, w)
    assert rc == 0 and info.tolist() == [0, 0, 9, 0, 0]  # reported, not fatal
    assert same_bits(cmix, mix) and np.isnan(cforest[2]).all() and same_bits(cforest[keep], full[keep])
    assert same_bits(marked.covariance(fx.x1, fx.x2, weights=w), mix)  # the Python layer raises nothing either
    live = np.array([0.4, 0.1, 0.1, 0.2, 0.2])
    rc, cmix, cforest, info = c_covariance(marked, fx.x1, fx.x2, live)
    assert rc == 0 and info.tolist() == [0, 0, 9, 0, 0] and np.isnan(cmix).all() and np.isnan(cforest[2]).all()
    assert same_bits(cforest[keep], full[keep])
    rc, cmix, _, _ = c_covariance(marked, fx.x1, None, None, forest=False)  # equal weights: every forest counts
    assert rc == 0 and np.isnan(cmix).all()
    with pytest.raises(np.linalg.LinAlgError):
        marked.covariance(fx.x1, fx.x2, weights=live)


# ---- the state as observe_ and condition leave it -----------------------------------------------------------------------
def test_after_observe_it_is_the_refit():
    from bark_amd.tree_kernels import fit_posterior

    name = "prior_n64"
    fx = fixture(name)
    x_new, y_new = ar.problem(3, 4242)[:2]
    moved = fx.post._copy().observe_(x_new, y_new)
    X = np.vstack([fx.inp.X, x_new])
    y = np.concatenate([fx.inp.y, np.asarray(y_new).reshape((-1,) + fx.inp.y.shape[1:])])
    refit = fit_posterior(fx.inp.model, (X, y), fx.inp.ft)
    w = pr.random_weights(fx.B)
    for x2 in (fx.x2, None):
        got_mix, got = moved.covariance(fx.x1, x2, per_forest=True, weights=w)
        want_mix, want = refit.covariance(fx.x1, x2, per_forest=True, weights=w)
        if x2 is not None:
            assert not close(got, fx.full[1])  # the three points moved it
        within(got, want, cr.forest_bar(name), f"observe_ against the refit, per forest, symmetric={x2 is None}")
        mu1 = refit.predict(fx.x1, per_forest=True)["forest_mean"]
        mu2 = mu1 if x2 is None else refit.predict(x2, per_forest=True)["forest_mean"]
        within(got_mix, want_mix, cr.mixture_bar(name, w, mu1, mu2), f"observe_ against the refit, mixture, symmetric={x2 is None}")


def test_condition_is_the_rank_one_downdate():
    name = "prior_n64"
    fx = fixture(name)
    for p in (fx.inp.cand[500:501], fx.x1[3:4]):
        cond = fx.post.condition(p)
        after = cond.covariance(fx.x1, fx.x2, per_forest=True)[1]
        before = fx.full[1]
        c1p = fx.post.covariance(fx.x1, p, per_forest=True)[1]   # (B, C1, 1)
        cp2 = fx.post.covariance(p, fx.x2, per_forest=True)[1]   # (B, 1, C2)
        var_p = fx.post.covariance(p, per_forest=True)[1][:, 0, 0]
        s2 = 1e-6 + fx.inp.noise
        want = before - c1p * cp2 / (var_p + s2)[:, None, None]
        assert np.abs(c1p * cp2).max() > 1e-3  # the identity has something to subtract
        within(after, want, cr.forest_bar(name), "condition against the rank-one identity")


# ---- conventions and refusals ----------------------------------------------------------------------------------------------
def test_torch_points_give_device_tensors():
    import torch

    fx = fixture("m2_r65")
    mix, forest = fx.post.covariance(torch.from_numpy(fx.x1).cuda(), torch.from_numpy(fx.x2).cuda(), per_forest=True)
    assert mix.is_cuda and forest.is_cuda
    assert same_bits(mix.cpu().numpy(), fx.full[0]) and same_bits(forest.cpu().numpy(), fx.full[1])
    only = fx.post.covariance(torch.from_numpy(fx.x1).cuda())
    assert only.is_cuda and tuple(only.shape) == (len(fx.x1), len(fx.x1))
    assert isinstance(fx.post.covariance(fx.x1), np.ndarray)


def test_refusals():
    from bark_amd import _lib as L

    fx = fixture("m2_r65")
    d = fx.x1.shape[1]
    with pytest.raises(ValueError):
        fx.post.covariance(fx.x1[:0])
    with pytest.raises(ValueError):
        fx.post.covariance(fx.x1, fx.x1[:0])
    with pytest.raises(ValueError, match="at most 65536 points"):
        fx.post.covariance(np.zeros((65537, d)))
    with pytest.raises(ValueError, match="at most 65536 points"):
        fx.post.covariance(fx.x1, np.zeros((65537, d)))
    rc, _, _, _ = c_covariance(fx.post, fx.x1, fx.x2, None, forest=False, mixture=False)
    assert rc == L.BARK_ERR_ARG and b"or both must be given" in L.lib().bark_last_error()
    # and the state is still what it was
    assert same_bits(fx.post.covariance(fx.x1, fx.x2), fx.full[0])
