"""The noise/scale half of the sampler step for a batch of chains, decided on the device
(`ChainBatch.step_noise_scale`, `bark_noise_scale_step_chains_hip`; bark_sampler.py:266-282): both branches bit for bit
against the leaf-space inverse export, the Metropolis rule against the host model of tests/noise_scale_ref.py, an R x R
sweep of two block rows, the flags that must leave a chain untouched, the reference's recorded steps end to end and the
argument checks of the C entry point."""
import ctypes

import numpy as np
import pytest

import leafspace_ref as lr
import noise_scale_ref as nsr

pytestmark = pytest.mark.gpu

MLL_TOL = dict(rtol=1e-9, atol=1e-8)  # against the oracle (test_gpu_parity.py)
ROUTE_TOL = dict(rtol=1e-12, atol=1e-10)  # against the same arithmetic by another entry point (test_gpu_context.py)


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bark_amd.fitting as fit
    import bark_amd.forest as bf
    from bark_amd import _lib, synthetic
    from oracle import oracle as orc

    class NS:
        pass

    ns = NS()
    ns.torch, ns.fit, ns.bf, ns.lib, ns.syn, ns.orc = torch, fit, bf, _lib, synthetic, orc
    return ns


def abi_step(env, cb, forests, new_noise, new_scale, log_q, log_u, X, ft, *, nc=None, info_B=None, accept="alloc", short=0):
    """One bark_noise_scale_step_chains_hip call on the batch's own K_inv -> (rc, accept_out, state) as numpy; the
    keyword arguments bend one argument each for the argument checks."""
    torch, L = env.torch, env.lib
    lib = L.lib()
    pf = env.bf.packed_forest(np.ascontiguousarray(forests), np.ascontiguousarray(ft, dtype=np.int64))
    info = L.PackInfo.from_buffer_copy(pf.info)
    if info_B is not None:
        info.B = info_B
    Xd = L.to_device(np.ascontiguousarray(X, dtype=np.float64))
    dev = [L.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in (new_noise, new_scale, log_q, log_u)]
    state = L.to_device(np.ascontiguousarray(np.stack([cb.quad, cb.logdet], axis=1)))
    acc = torch.full((cb.nc,), 7, dtype=torch.int32, device="cuda") if accept == "alloc" else accept
    nbytes = int(lib.bark_noise_scale_step_chains_workspace_bytes(cb.N, int(pf.info.max_bits), pf.m, cb.nc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    rc = lib.bark_noise_scale_step_chains_hip(L.ctx(), L.ptr(cb.K_inv), cb.N, cb.nc if nc is None else nc, L.ptr(pf.packed),
                                              ctypes.byref(info), L.ptr(Xd), Xd.shape[1], L.ptr(cb.y), *(L.ptr(v) for v in dev),
                                              L.ptr(state), L.ptr(acc), L.ptr(ws), nbytes - short, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, (None if acc is None else acc.cpu().numpy()), state.cpu().numpy()


@pytest.mark.parametrize("N", [129, 130])
def test_accept_and_reject_bit_for_bit(env, N):
    """Two full 64-wide output tiles and an edge tile of 1 or 2; log_q_prior forces accept / reject / accept.  Accepted
    chains hold exactly what the leaf-space inverse export gives at the proposed values (same sweep shape, same
    arithmetic); the rejected chain keeps every bit."""
    fit, syn = env.fit, env.syn
    nc, m = 3, 8
    X, y, bounds, ft = syn.mixed_problem(N, seed=21)
    F = syn.sample_prior_forests(nc, m, bounds, ft, seed=210)
    noise, scale = np.array([0.1, 0.07, 0.2]), np.array([1.0, 0.8, 1.2])
    nn, nsc = np.array([0.105, 0.068, 0.19]), np.array([1.02, 0.82, 1.15])  # |new_mll - cur_mll| < 30: +50 / -1e3 decide
    cb = fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, quad0, logdet0 = cb.K_inv.clone(), cb.quad.copy(), cb.logdet.copy()
    mask = cb.step_noise_scale(F, nn, nsc, [50.0, -1e3, 50.0], np.full(nc, np.log(0.5)), X, ft)
    assert mask.dtype == bool and mask.tolist() == [True, False, True]
    assert env.torch.equal(cb.K_inv[1], before[1])
    assert cb.quad[1] == quad0[1] and cb.logdet[1] == logdet0[1]
    K_ref, Ky_ref, logdet_ref = fit.batched_kernel_inverse(F, nn, nsc, X, y, ft, no_null=False, method="leafspace", chunk=3,
                                                           return_device=True)
    mll_ref = 0.5 * (-(Ky_ref.cpu().numpy() @ y.reshape(-1)) - logdet_ref.cpu().numpy())
    want = env.orc.batched_mll(F, nn, nsc, X, y, ft, include_scale=True, include_2pi=False)
    for b in (0, 2):
        assert env.torch.equal(cb.K_inv[b], K_ref[b])
        print(f"N={N} chain {b}: mll {cb.mll[b]!r} route {mll_ref[b]!r} oracle {want[b]!r}")
        assert np.isclose(cb.mll[b], mll_ref[b], **ROUTE_TOL)
        assert np.isclose(cb.mll[b], want[b], **MLL_TOL)


RULE_SEED = 3  # checked on the CPU: the model alone accepts and rejects, no decision closer than 1e-6 (asserted below)


def test_metropolis_rule_matches_the_model(env):
    """N = 64: one output tile.  Random proposal ratios and uniform draws; the device's flags are the model's."""
    fit, syn = env.fit, env.syn
    nc, m, N = 4, 8, 64
    X, y, bounds, ft = syn.mixed_problem(N, seed=22)
    F = syn.sample_prior_forests(nc, m, bounds, ft, seed=220)
    noise, scale = np.array([0.1, 0.07, 0.2, 0.15]), np.array([1.0, 0.8, 1.2, 0.9])
    rng = np.random.default_rng(RULE_SEED)
    nn, nsc = noise * np.exp(rng.normal(0.0, 0.1, nc)), scale * np.exp(rng.normal(0.0, 0.1, nc))
    log_q, log_u = rng.normal(0.0, 0.5, nc), np.log(rng.uniform(size=nc))
    yv = y.reshape(-1)
    state = np.empty((nc, 2))
    for b in range(nc):
        Ks = nsr.kernel_matrix(F[b], noise[b], scale[b], X, ft)
        state[b] = yv @ np.linalg.inv(Ks) @ yv, np.linalg.slogdet(Ks)[1]
    want, state2, K_want = nsr.step(F, noise, scale, nn, nsc, log_q, log_u, X, y, ft, state)
    new_mll = [nsr.proposal_mll(F[b], nn[b], nsc[b], X, yv, ft) for b in range(nc)]
    margin = np.abs(nsr.log_alpha(log_q, new_mll, state) - log_u)
    print("model flags", want, "margins", margin)
    assert (want == 1).any() and (want == 0).any() and set(want.tolist()) <= {0, 1}
    assert margin.min() >= 1e-6
    cb = fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    mask = cb.step_noise_scale(F, nn, nsc, log_q, log_u, X, ft)
    assert np.array_equal(mask, want == 1)
    assert np.allclose(cb.mll, 0.5 * (-state2[:, 0] - state2[:, 1]), **MLL_TOL)
    K = cb.K_inv.cpu().numpy()
    assert np.allclose(K, K_want, rtol=1e-8, atol=1e-9)  # K_inv: test_kernel_inverse_for_acquisition_builder's bound


def test_two_block_rows_of_the_leaf_system(env):
    """128 < R <= 256: the R x R sweep has two block rows (and R > N leaves columns of Z empty).  K_inv against
    np.linalg.inv of the oracle's kernel matrix at rtol 1e-9; entries far below the matrix's largest are held to the same
    1e-9 of that largest entry, which is how the error of an explicit inverse is bounded (norm-wise, cond(K_s) ~ 1e3)."""
    fit, syn = env.fit, env.syn
    nc, N = 2, 70
    X, y, bounds, ft = syn.mixed_problem(N, seed=23)
    rng = np.random.default_rng(23)
    pieces = (("full", 1, 7), ("full", 2, 4), ("null", 1))
    F = np.stack([lr.build_forest(pieces, rng, bounds, ft) for _ in range(nc)])
    info, _ = lr.host_pack(F, ft)
    assert 128 < info.max_bits <= 256 and -(-int(info.max_bits) // lr.NB) == 2
    noise, scale = np.array([0.1, 0.2]), np.array([1.0, 1.2])
    nn, nsc = np.array([0.11, 0.19]), np.array([0.95, 1.25])  # |new_mll - cur_mll| < 5: +50 accepts
    cb = fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    mask = cb.step_noise_scale(F, nn, nsc, [50.0, 50.0], np.full(nc, np.log(0.5)), X, ft)
    assert mask.tolist() == [True, True]
    K = cb.K_inv.cpu().numpy()
    for b in range(nc):
        want = np.linalg.inv(nsr.kernel_matrix(F[b], nn[b], nsc[b], X, ft))
        err = np.abs(K[b] - want)
        print(f"chain {b}: max |dK_inv| {err.max():.3e} of max |K_inv| {np.abs(want).max():.3e}")
        assert np.allclose(K[b], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    want = env.orc.batched_mll(F, nn, nsc, X, y, ft, include_scale=True, include_2pi=False)
    assert np.allclose(cb.mll, want, **MLL_TOL)


@pytest.fixture(scope="module")
def small(env):
    """Four chains on 64 points, shared by the flag and argument tests (none of which may change it on failure paths)."""
    syn = env.syn
    nc, m, N = 4, 8, 64
    X, y, bounds, ft = syn.mixed_problem(N, seed=24)
    F = syn.sample_prior_forests(nc, m, bounds, ft, seed=240)
    noise, scale = np.array([0.1, 0.07, 0.2, 0.15]), np.array([1.0, 0.8, 1.2, 0.9])
    return F, noise, scale, X, y, ft


def test_nan_draws_and_nonpositive_noise_reject_without_writing(env, small):
    """NaN log_u, NaN log_q_prior and new_noise = -1 (1e-6 + noise <= 0: the MLL is NaN) are rejections, flag 0, beside a
    chain that accepts."""
    F, noise, scale, X, y, ft = small
    cb = env.fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, st0 = cb.K_inv.clone(), np.stack([cb.quad, cb.logdet], axis=1)
    lu = np.array([np.nan, np.log(0.5), np.log(0.5), np.log(0.5)])
    lq = np.array([50.0, np.nan, 50.0, 50.0])
    nn = np.array([0.105, 0.072, -1.0, 0.155])
    rc, acc, st = abi_step(env, cb, F, nn, scale, lq, lu, X, ft)
    assert rc == 0 and acc.tolist() == [0, 0, 0, 1]
    assert env.torch.equal(cb.K_inv[:3], before[:3]) and not env.torch.equal(cb.K_inv[3], before[3])
    assert np.array_equal(st[:3], st0[:3]) and not np.array_equal(st[3], st0[3])


def test_negative_scale_flags_its_chain_only(env, small):
    F, noise, scale, X, y, ft = small
    F, noise, scale = F[:3], noise[:3], scale[:3]
    nn, nsc = np.array([0.12, 0.1, 0.18]), np.array([0.9, -5.0, 1.1])
    lq, lu = np.full(3, 50.0), np.full(3, np.log(0.5))
    cb = env.fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, st0 = cb.K_inv.clone(), np.stack([cb.quad, cb.logdet], axis=1)
    rc, acc, st = abi_step(env, cb, F, nn, nsc, lq, lu, X, ft)
    assert rc == 0 and acc.tolist() == [1, -1, 1]
    assert env.torch.equal(cb.K_inv[1], before[1]) and np.array_equal(st[1], st0[1])
    # the method: the other chains are updated (state taken before raising), then LinAlgError
    cb = env.fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, quad0, logdet0 = cb.K_inv.clone(), cb.quad.copy(), cb.logdet.copy()
    with pytest.raises(np.linalg.LinAlgError):
        cb.step_noise_scale(F, nn, nsc, lq, lu, X, ft)
    assert env.torch.equal(cb.K_inv[1], before[1]) and cb.quad[1] == quad0[1] and cb.logdet[1] == logdet0[1]
    assert not env.torch.equal(cb.K_inv[0], before[0]) and not env.torch.equal(cb.K_inv[2], before[2])
    want = env.orc.batched_mll(F, nn, nsc, X, y, ft, include_scale=True, include_2pi=False)
    assert np.allclose(cb.mll[[0, 2]], want[[0, 2]], **MLL_TOL)


def test_invalid_category_flags_every_chain_and_raises(env, small):
    """A categorical split evaluated at -1 (forest.py:38 raises in `1 << int(x)`): -2 for every chain, nothing written,
    and the error `propose_trees` raises."""
    F, noise, scale, X, y, ft = small
    F = F[:3].copy()
    noise, scale = noise[:3], scale[:3]
    cat = int(np.flatnonzero(ft == 0)[0])
    F[1, 0] = env.bf.create_empty_forest(1, F.shape[2])[0]
    F[1, 0, 0] = (0, cat, float(0b0101), 1, 2, 0xFFFFFFFF, 0, 1)  # root: categorical split, every point evaluates it
    F[1, 0, 1] = (1, 0, 0, 0, 0, 0, 1, 1)
    F[1, 0, 2] = (1, 0, 0, 0, 0, 0, 1, 1)
    cb = env.fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, st0 = cb.K_inv.clone(), np.stack([cb.quad, cb.logdet], axis=1)
    bad = X.copy()
    bad[5, cat] = -1.0
    lq, lu = np.full(3, 50.0), np.full(3, np.log(0.5))
    rc, acc, st = abi_step(env, cb, F, noise, scale, lq, lu, bad, ft)
    assert rc == 0 and acc.tolist() == [-2, -2, -2]
    assert env.torch.equal(cb.K_inv, before) and np.array_equal(st, st0)
    with pytest.raises(ValueError):
        env.lib.check_categorical_fault()  # reads and clears the context's flag
    with pytest.raises((ValueError, OverflowError)):
        cb.step_noise_scale(F, noise, scale, lq, lu, bad, ft)
    assert env.torch.equal(cb.K_inv, before)
    assert np.array_equal(cb.quad, st0[:, 0]) and np.array_equal(cb.logdet, st0[:, 1])
    assert cb.step_noise_scale(F, noise, scale, lq, lu, X, ft).all()  # the flag does not leak into the next call


def test_g11_reference_steps_through_the_batch_alone(env):
    """tests/golden/g11_sampler_steps.npz: both chains through sweep_trees + step_noise_scale for every recorded step; the
    batch is built once and never rebuilt."""
    from conftest import load_golden

    fit, orc = env.fit, env.orc
    g = load_golden("g11_sampler_steps")
    X, y, ft = g["X"], g["y"], g["feat_types"]
    chains, steps, m = g["accept"].shape
    forests = orc.nodes_from_raw(g["start_forest"]).copy()
    noise, scale = g["start_noise"].copy(), g["start_scale"].copy()
    cb = fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
    assert np.allclose(cb.mll, g["start_mll"], **MLL_TOL)
    for s in range(steps):
        old, new = orc.nodes_from_raw(g["old"][:, s]), orc.nodes_from_raw(g["new"][:, s])
        mask = cb.sweep_trees(old, new, g["log_q"][:, s], np.log(g["u"][:, s]), X, ft, scale, m)
        assert np.array_equal(mask, g["accept"][:, s])
        forests[mask] = new[mask]
        assert np.allclose(cb.mll, g["cur_mll"][:, s, -1], **MLL_TOL)
        acc = cb.step_noise_scale(forests, g["ns_prop"][:, s, 0], g["ns_prop"][:, s, 1], g["ns_log_q"][:, s],
                                  np.log(g["ns_u"][:, s]), X, ft)
        assert np.array_equal(acc, g["ns_accept"][:, s])
        noise = np.where(acc, g["ns_prop"][:, s, 0], noise)
        scale = np.where(acc, g["ns_prop"][:, s, 1], scale)
        print(f"step {s}: mll {cb.mll!r} recorded {g['mll_after'][:, s]!r}")
        assert np.allclose(cb.mll, g["mll_after"][:, s], **MLL_TOL)
        assert np.array_equal(forests, orc.nodes_from_raw(g["forest_after"][:, s]))


def test_argument_checks_launch_nothing(env, small):
    """nc outside 1..64, info->B != nc, a null accept_out and a workspace one byte short: a status, a message, and
    neither K_inv, the state nor accept_out touched."""
    F, noise, scale, X, y, ft = small
    L, lib = env.lib, env.lib.lib()
    cb = env.fit.ChainBatch.from_forests(F, noise, scale, X, y, ft)
    before, st0 = cb.K_inv.clone(), np.stack([cb.quad, cb.logdet], axis=1)
    lq, lu = np.full(4, 50.0), np.full(4, np.log(0.5))
    cases = [(dict(nc=0), L.BARK_ERR_ARG), (dict(nc=65), L.BARK_ERR_ARG), (dict(info_B=3), L.BARK_ERR_ARG),
             (dict(accept=None), L.BARK_ERR_ARG), (dict(short=1), L.BARK_ERR_WORKSPACE)]
    for kw, status in cases:
        rc, acc, st = abi_step(env, cb, F, noise, scale, lq, lu, X, ft, **kw)
        assert rc == status, (kw, rc)
        assert lib.bark_last_error() != b"", kw
        assert acc is None or (acc == 7).all(), kw
        assert np.array_equal(st, st0) and env.torch.equal(cb.K_inv, before), kw
    rc, acc, _ = abi_step(env, cb, F, noise, scale, lq, lu, X, ft)  # the same call, unbent, runs
    assert rc == 0 and acc.tolist() == [1, 1, 1, 1] and lib.bark_last_error() == b""
