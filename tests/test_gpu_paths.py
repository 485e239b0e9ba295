"""Sample paths from a fitted posterior and Thompson proposals (LeafPosterior.sample_paths, LeafPaths, optimizer's
propose_thompson_*; bark_leaf_posterior_paths_hip, bark_path_scan_hip) against tests/paths_ref.py, which starts from the state
read back from the device.

Shapes: B = 3 prior forests of m = 5 trees, N = 40, d = 4 (two continuous features, one integer, one categorical), noise >= 0.05.
The deep-tree cases put R just below, at and just above every tile edge of the new kernels:
  32   the factorisation's tile (paths_factor_kernel: 32 x 32 tiles, one panel / two panels)
  64   the lanes of a wave in paths_weights_kernel (one stride / two), and two / three panels of the factorisation
  256  the project's earlier edge (eight panels), and the candidates per scan workgroup
  384  the scan stages 16 paths of a forest per LDS round up to R = 384, 15 from 385 on; a forest of 17 paths takes two rounds
and the candidate counts 65 535, 65 536 and 65 537 straddle the scan's slab."""
import numpy as np
import pytest

from bark_amd import synthetic
from bark_amd.fitting import _philox

import paths_ref
from leafspace_ref import build_forest

pytestmark = pytest.mark.gpu

N, B, M = 40, 3, 5
KW = dict(d_cont=2, n_int=1, n_cat=1)
RTOL, ATOL = 1e-9, 1e-8  # the project's fp64 tolerance


class Fixture:
    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.X, self.y, self.bounds, self.ft = synthetic.mixed_problem(N, seed=31, **KW)
        self.F = synthetic.sample_prior_forests(B, M, self.bounds, self.ft, seed=41)
        self.noise, self.scale = np.array([0.05, 0.1, 0.2]), np.array([0.8, 1.0, 1.3])
        self.model, self.data = (self.F, self.noise, self.scale), (self.X, self.y)
        self.post = fit_posterior(self.model, self.data, self.ft)
        self.R = self.post.R
        self.Minv, self.w, _ = paths_ref.read_state(self.post.state.cpu().numpy(), B, self.R)
        self.cand = synthetic.mixed_problem(700, seed=32, **KW)[0]
        self.cols = paths_ref.leaf_columns(self.F, self.ft, self.cand)[0]
        self.pend = synthetic.mixed_problem(3, seed=33, **KW)[0]

    def ref_weights(self, forest, eps, Minv=None):
        return paths_ref.weights(self.Minv if Minv is None else Minv, self.w, self.noise, self.scale, M, forest, eps)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def host(t):
    return t.cpu().numpy()


def test_weights(fx):
    forest = np.array([2, 0, 1, 2, 2, 0])
    eps = np.random.default_rng(1).standard_normal((6, fx.R))
    paths = fx.post.sample_paths(forests=forest, eps=eps)
    assert paths.P == 6 and paths.forest.tolist() == forest.tolist() and paths.draw.tolist() == [0, 0, 0, 1, 2, 1]
    W = host(paths.W)
    assert W.shape == (6, fx.R) and paths.W.is_cuda
    np.testing.assert_allclose(W, fx.ref_weights(forest, eps), rtol=RTOL, atol=ATOL)
    # all forests, b-major
    eps = np.random.default_rng(2).standard_normal((2 * B, fx.R))
    paths = fx.post.sample_paths(2, eps=eps)
    assert paths.forest.tolist() == [0, 0, 1, 1, 2, 2] and paths.draw.tolist() == [0, 1] * 3
    np.testing.assert_allclose(host(paths.W), fx.ref_weights(paths.forest, eps), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("conditioned", [False, True])
def test_the_factor_reconstructs_the_state(fx, conditioned):
    post = fx.post.condition(fx.pend) if conditioned else fx.post
    Minv, w, info = paths_ref.read_state(post.state.cpu().numpy(), B, fx.R)
    assert not info.any() and (not conditioned or not np.array_equal(Minv, fx.Minv))
    b, R = 1, fx.R
    W = host(post.sample_paths(forests=[b] * R, eps=np.eye(R)).W)
    c = fx.scale[b] / (M * (1e-6 + fx.noise[b]))
    D = W - c * w[b]  # row p: sqrt(scale / m) times column p of G
    assert np.array_equal(np.triu(D.T, 1), np.zeros((R, R)))  # G is lower triangular, exactly
    np.testing.assert_allclose(D.T @ D * (M / fx.scale[b]), Minv[b], rtol=RTOL, atol=ATOL)


def test_scan_bits(fx):
    import torch

    forest = np.array([2, 1, 2])  # omits forest 0, names forest 2 twice
    paths = fx.post.sample_paths(forests=forest, seed=3)
    W = host(paths.W)
    cand = fx.cand.copy()
    cand[[5, 300, 699]] = cand[17]  # duplicated rows: ties
    cols = paths_ref.leaf_columns(fx.F, fx.ft, cand)[0]
    want = paths_ref.evaluate(W, forest, cols)
    got = paths.evaluate(cand)
    assert isinstance(got, np.ndarray) and got.shape == (3, 700)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(got[:, 5], got[:, 17]) and np.array_equal(got[:, 699], got[:, 17])
    for maximise in (False, True):
        v, i = paths.minimise(cand, maximise=maximise)
        wv, wi = paths_ref.first_argmin(want, maximise)
        assert i.dtype == np.int64
        np.testing.assert_array_equal(v, wv)
        np.testing.assert_array_equal(i, wi)
    # a tie at the extreme itself: every candidate is the same row
    same = np.repeat(cand[17:18], 300, axis=0)
    v, i = paths.minimise(same)
    assert i.tolist() == [0, 0, 0] and np.array_equal(v, want[:, 17])
    v, i = paths.minimise(same, maximise=True)
    assert i.tolist() == [0, 0, 0]
    # torch in, device tensors out; C = 1; P = 1
    td = torch.from_numpy(cand).cuda()
    f = paths.evaluate(td)
    v, i = paths.minimise(td)
    assert f.is_cuda and v.is_cuda and i.is_cuda and np.array_equal(host(f), want)
    one = paths.evaluate(cand[9:10])
    assert one.shape == (3, 1) and np.array_equal(one[:, 0], want[:, 9])
    v, i = paths.minimise(cand[9:10])
    assert i.tolist() == [0, 0, 0] and np.array_equal(v, want[:, 9])
    single = fx.post.sample_paths(forests=[1], seed=3)
    assert np.array_equal(single.evaluate(cand)[0], want[1])  # (1, 0) again, alone
    sub = paths.subset([2, 0])
    assert np.array_equal(sub.evaluate(cand), want[[2, 0]]) and sub.forest.tolist() == [2, 2]


@pytest.mark.parametrize("C", [65535, 65536, 65537])
def test_scan_slab_edge(fx, C):
    rng = np.random.default_rng(C)
    pick = rng.integers(0, 700, size=C)  # rows of the 700 whose leaf columns are known
    cand = fx.cand[pick]
    forest = np.array([1, 2, 2])
    paths = fx.post.sample_paths(forests=forest, seed=4)
    want = paths_ref.evaluate(host(paths.W), forest, fx.cols[:, pick])
    np.testing.assert_array_equal(paths.evaluate(cand), want)
    for maximise in (False, True):
        v, i = paths.minimise(cand, maximise=maximise)
        wv, wi = paths_ref.first_argmin(want, maximise)
        np.testing.assert_array_equal(v, wv)
        np.testing.assert_array_equal(i, wi)  # 700 distinct rows among C: ties everywhere, the lowest index wins


def test_addressing(fx):
    full = fx.post.sample_paths(2, seed=11)
    again = fx.post.sample_paths(2, seed=11)
    Wf = host(full.W)
    assert np.array_equal(Wf, host(again.W)) and np.isfinite(Wf).all()
    assert np.array_equal(host(fx.post.sample_paths(forests=[2], seed=11).W)[0], Wf[4])  # (2, 0) of the b-major call
    mixed = fx.post.sample_paths(forests=[2, 0, 1, 2, 0], seed=11)  # (2,0) (0,0) (1,0) (2,1) (0,1)
    assert np.array_equal(host(mixed.W), Wf[[4, 0, 2, 5, 1]])
    other = fx.post.sample_paths(forests=[1, 1, 2], seed=11)
    assert np.array_equal(host(other.W), Wf[[2, 3, 4]])
    assert not np.array_equal(host(fx.post.sample_paths(forests=[2], seed=12).W)[0], Wf[4])  # another seed
    assert not np.array_equal(Wf[4], Wf[5]) and not np.array_equal(Wf[4, :8], Wf[2, :8])  # another draw, another forest
    assert not np.array_equal(host(fx.post.sample_paths(forests=[2], seed=11 + (1 << 32)).W)[0], Wf[4])  # the high word counts


def test_normals(fx):
    """With M^-1 = I, w = 0 and scale = m the weights are the normals themselves: G = I, c w = 0, sqrt(scale / m) = 1."""
    import torch

    R = fx.R
    unit = fx.post._copy()
    state = unit.state
    state[:8 * B * R * R].view(torch.float64).copy_(torch.eye(R, dtype=torch.float64).repeat(B, 1).reshape(-1))
    at = paths_ref.align256(8 * B * R * R)
    state[at:at + 8 * B * R].zero_()
    unit.scale = torch.full((B,), float(M), dtype=torch.float64, device="cuda")
    forest, draw = [2, 0, 2, 1], [0, 0, 1, 0]
    W = host(unit.sample_paths(forests=forest, seed=0xABCDEF0123456789).W)
    want = _philox.path_normals(0xABCDEF0123456789, forest, draw, R)
    assert (np.abs(want) < 9).all()
    np.testing.assert_allclose(W, want, rtol=0, atol=1e-12)
    # and on the fitted state: the seeded weights are the weights of the restated normals
    W = host(fx.post.sample_paths(forests=forest, seed=77).W)
    np.testing.assert_allclose(W, fx.ref_weights(np.array(forest), _philox.path_normals(77, forest, draw, R)), rtol=RTOL, atol=ATOL)


def test_status(fx):
    import torch

    forest = np.array([0, 1, 1, 2])
    good = fx.post.sample_paths(forests=forest, seed=5)
    Wg, fg = host(good.W), good.evaluate(fx.cand)
    # a state that is not positive definite: pivot 3 of forest 1 (1-based) is negated
    broken = fx.post._copy()
    Mv = broken.state[:8 * B * fx.R * fx.R].view(torch.float64).view(B, fx.R, fx.R)
    Mv[1, 2, 2] = -Mv[1, 2, 2]
    paths = broken.sample_paths(forests=forest, seed=5)
    W = host(paths.W)
    assert np.isnan(W[1:3]).all() and np.array_equal(W[[0, 3]], Wg[[0, 3]])
    f = paths.evaluate(fx.cand)
    assert np.isnan(f[1:3]).all() and np.array_equal(f[[0, 3]], fg[[0, 3]])
    v, i = paths.minimise(fx.cand)
    assert np.isnan(v[1:3]).all() and i[1:3].tolist() == [-1, -1]
    wv, wi = paths_ref.first_argmin(fg[[0, 3]])
    assert np.array_equal(v[[0, 3]], wv) and np.array_equal(i[[0, 3]], wi)
    # the C entry reports the pivot
    from bark_amd import _lib as L

    lib = L.lib()
    info = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    Wd = torch.empty((2, fx.R), dtype=torch.float64, device="cuda")
    pf, pd = np.array([1, 2], dtype=np.int32), np.zeros(2, dtype=np.int32)

    def call(post, P=2, state_bytes=None, pf=pf, pd=pd):
        ws = L.workspace(int(lib.bark_leaf_posterior_paths_workspace_bytes(fx.R, M, B, 2, 1)))
        return lib.bark_leaf_posterior_paths_hip(L.ctx(), post.packed.info_ref, L.ptr(post.noise), L.ptr(post.scale), L.ptr(post.state),
                                                 post.nbytes if state_bytes is None else state_bytes, L.ptr(pf), L.ptr(pd), P, None, 5,
                                                 L.ptr(Wd), L.ptr(info), L.ptr(ws), ws.numel(), L.stream_ptr())

    assert call(broken) == 0
    assert host(info).tolist() == [0, 3, 0] and np.isnan(host(Wd)[0]).all() and np.array_equal(host(Wd)[1], Wg[3])
    # a status already in the state
    marked = fx.post._copy()
    marked.info[2] = 9
    assert call(marked) == 0
    assert host(info).tolist() == [0, 0, 9] and np.isnan(host(Wd)[1]).all() and np.array_equal(host(Wd)[0], Wg[1])
    # refusals, before any launch: the outputs keep their fill
    info.fill_(-77)
    Wd.fill_(7.0)
    for kw, message in ((dict(P=0), b"paths per call"), (dict(P=4097), b"paths per call"), (dict(state_bytes=fx.post.nbytes - 1), b"too small"),
                        (dict(pf=np.array([2, 1], dtype=np.int32)), b"non-decreasing"), (dict(pf=np.array([1, 3], dtype=np.int32)), b"non-decreasing"),
                        (dict(pd=np.array([0, -1], dtype=np.int32)), b"negative draw")):
        assert call(fx.post, **kw) == L.BARK_ERR_ARG and message in lib.bark_last_error(), (kw, lib.bark_last_error())
    torch.cuda.synchronize()
    assert bool((info == -77).all()) and bool((Wd == 7.0).all())
    # an invalid categorical value in a candidate: the error of LeafPosterior.scan, and the flag is cleared
    bad = fx.cand.copy()
    bad[699, 3] = -1.0
    with pytest.raises(ValueError, match="categorical"):
        good.minimise(bad)
    with pytest.raises(ValueError, match="categorical"):
        good.evaluate(bad)
    assert np.array_equal(good.evaluate(fx.cand), fg)
    with pytest.raises(ValueError, match="features"):
        good.evaluate(fx.cand[:, :3])
    with pytest.raises(ValueError, match="eps must be"):
        fx.post.sample_paths(forests=[0], eps=np.zeros((2, fx.R)))


# R = full trees' leaves + null trees: (pieces, R); all with at most 64 trees
DEEP = {31: (("full", 1, 4), ("null", 15)), 32: (("full", 1, 4), ("null", 16)), 33: (("full", 1, 4), ("null", 17)),
        63: (("full", 1, 5), ("null", 31)), 64: (("full", 1, 5), ("null", 32)), 65: (("full", 1, 5), ("null", 33)),
        255: (("full", 1, 7), ("full", 1, 6), ("full", 1, 5), ("null", 31)), 256: (("full", 2, 7),), 257: (("full", 2, 7), ("null", 1)),
        384: (("full", 3, 7),), 385: (("full", 3, 7), ("null", 1))}


@pytest.mark.parametrize("R", sorted(DEEP))
def test_deep_trees_at_the_tile_edges(R):
    from bark_amd.tree_kernels import fit_posterior

    X, y, bounds, ft = synthetic.mixed_problem(N, seed=100 + R)
    cand = synthetic.mixed_problem(300, seed=200 + R)[0]
    rng = np.random.default_rng(R)
    F = np.stack([build_forest(DEEP[R], rng, bounds, ft) for _ in range(2)])
    m = F.shape[1]
    noise, scale = np.array([0.05, 0.2]), np.array([0.9, 1.2])
    post = fit_posterior((F, noise, scale), (X, y), ft)
    assert post.R == R
    Minv, w, _ = paths_ref.read_state(post.state.cpu().numpy(), 2, R)
    forest = np.array([1] * 17 + [0])  # 17 paths of one forest: two LDS rounds of the scan
    eps = rng.standard_normal((18, R))
    paths = post.sample_paths(forests=forest, eps=eps)
    W = host(paths.W)
    want = paths_ref.weights(Minv, w, noise, scale, m, forest, eps)
    np.testing.assert_allclose(W, want, rtol=RTOL, atol=ATOL)
    cols = paths_ref.leaf_columns(F, ft, cand)[0]
    f = paths_ref.evaluate(W, forest, cols)
    np.testing.assert_array_equal(paths.evaluate(cand), f)
    v, i = paths.minimise(cand)
    wv, wi = paths_ref.first_argmin(f)
    np.testing.assert_array_equal(v, wv)
    np.testing.assert_array_equal(i, wi)


class Domain:
    def __init__(self):
        from bark_amd.tree_kernels import fit_posterior

        kw = dict(d_cont=1, n_int=1, n_cat=1)
        self.X, self.y, self.bounds, self.ft = synthetic.mixed_problem(N, seed=51, **kw)
        self.F = synthetic.sample_prior_forests(4, 5, self.bounds, self.ft, seed=61)
        self.model = (self.F, np.array([0.05, 0.1, 0.1, 0.2]), np.array([0.8, 1.0, 1.1, 1.3]))
        self.data = (self.X, self.y)
        self.post = fit_posterior(self.model, self.data, self.ft)

    def path_values(self, info, rows, seed):
        """The values of the draws' paths at `rows`, by the host loop: (q, n)."""
        forests = np.array([d["forest"] for d in info])
        W = host(self.post.sample_paths(forests=forests, seed=seed).W)
        assert [d["draw"] for d in info] == self.post.sample_paths(forests=forests, seed=seed).draw.tolist()
        return paths_ref.evaluate(W, forests, paths_ref.leaf_columns(self.F, self.ft, rows)[0])


@pytest.fixture(scope="module")
def dom():
    return Domain()


def test_domain_exhaustive(dom):
    from bark_amd.optimizer import domain_candidates, domain_plan, propose_thompson_from_domain, split_table, thompson_forests

    q, seed = 6, 9
    X, info = propose_thompson_from_domain(dom.model, dom.data, dom.bounds, dom.ft, q, seed=seed, return_info=True)
    assert X.shape == (q, 3) and [d["forest"] for d in info] == thompson_forests(4, q, seed).tolist()
    for i, d in enumerate(info):
        table = split_table(dom.F[d["forest"]:d["forest"] + 1], dom.bounds, dom.ft)
        grid = domain_plan(table)["grid"]
        assert d["exhaustive"] and d["grid"] == grid and d["sweeps"] == 0 and 1 < grid < 100000
    # brute force: every draw's path over its forest's whole grid, first minimum in grid order
    for fb in sorted({d["forest"] for d in info}):
        table = split_table(dom.F[fb:fb + 1], dom.bounds, dom.ft)
        rows = host(domain_candidates(table, dom.bounds, dom.ft, domain_plan(table)["grid"], "grid", 0))
        f = dom.path_values(info, rows, seed)
        for i, d in enumerate(info):
            if d["forest"] == fb:
                at = int(np.argmin(f[i]))
                assert d["index"] == at and d["value"] == f[i, at] and np.array_equal(X[i], rows[at])
    for round_size in (7, 64):
        X2, info2 = propose_thompson_from_domain(None, None, dom.bounds, dom.ft, q, seed=seed, posterior=dom.post, round_size=round_size,
                                                 return_info=True)
        assert np.array_equal(X2, X) and [d["value"] for d in info2] == [d["value"] for d in info]
    assert np.array_equal(propose_thompson_from_domain(dom.model, dom.data, dom.bounds, dom.ft, q, seed=seed), X)


def test_domain_search(dom):
    from bark_amd.optimizer import domain_neighbours, propose_thompson_from_domain, split_table

    q, seed = 6, 9
    kw = dict(exhaustive_limit=1, n_candidates=512, starts=3, seed=seed, posterior=dom.post, return_info=True)
    X, info = propose_thompson_from_domain(None, None, dom.bounds, dom.ft, q, **kw)
    at_x = dom.path_values(info, X, seed)
    for i, d in enumerate(info):
        assert not d["exhaustive"] and d["index"] == -1 and d["sweeps"] >= 1
        assert d["value"] == at_x[i, i] and (d["value"] <= d["start_values"]).all()
        table = split_table(dom.F[d["forest"]:d["forest"] + 1], dom.bounds, dom.ft)
        near = host(domain_neighbours(table, X[i:i + 1]))
        assert (d["value"] <= dom.path_values(info, near, seed)[i]).all()
    X2, _ = propose_thompson_from_domain(None, None, dom.bounds, dom.ft, q, round_size=100, **kw)
    assert np.array_equal(X2, X)


def test_candidates(fx):
    import torch

    from bark_amd.optimizer import propose_thompson_from_candidates, thompson_forests

    q, seed = 7, 21
    idx, info = propose_thompson_from_candidates(fx.model, fx.data, fx.cand, fx.ft, q, seed=seed, return_info=True)
    idx2, info2 = propose_thompson_from_candidates(None, None, fx.cand, None, q, seed=seed, posterior=fx.post, return_info=True)
    assert idx.dtype == np.int64 and idx.shape == (q,) and np.array_equal(idx, idx2)
    assert set(info) == set(info2) == {"forest", "draw", "value", "unique"}
    for k in info:
        assert np.array_equal(info[k], info2[k]), k
    assert info["forest"].tolist() == thompson_forests(B, q, seed).tolist() and info["unique"] == len(set(idx.tolist()))
    W = host(fx.post.sample_paths(forests=info["forest"], seed=seed).W)
    f = paths_ref.evaluate(W, info["forest"], fx.cols)
    wv, wi = paths_ref.first_argmin(f)
    assert np.array_equal(idx, wi) and np.array_equal(info["value"], wv)
    assert np.array_equal(propose_thompson_from_candidates(fx.model, fx.data, fx.cand, fx.ft, q, seed=seed), idx)
    on_device = propose_thompson_from_candidates(None, None, torch.from_numpy(fx.cand).cuda(), None, q, seed=seed, posterior=fx.post)
    assert on_device.is_cuda and np.array_equal(host(on_device), idx)
    # a conditioned posterior gives other paths: the pending points count
    cond = fx.post.condition(fx.pend)
    assert not np.array_equal(host(cond.sample_paths(forests=info["forest"], seed=seed).W), W)
