"""No GPU: the host model of the batched noise/scale step (tests/noise_scale_ref.py) against the reference's own recorded
sampler steps, and the host-side workspace function of `bark_noise_scale_step_chains_hip`."""
import numpy as np
import pytest

from bark_amd import _lib
from oracle import oracle as orc

import noise_scale_ref as nsr
from conftest import load_golden

TOL = dict(rtol=1e-9, atol=1e-8)  # the project's MLL tolerance


def test_model_reproduces_the_recorded_noise_scale_decisions():
    """tests/golden/g11_sampler_steps.npz: every ns_accept, ns_new_mll and mll_after of the reference's
    `_step_bark_sampler` (bark_sampler.py:266-282), both chains stepped as a batch."""
    g = load_golden("g11_sampler_steps")
    X, y, ft = g["X"], g["y"], g["feat_types"]
    yv = y.reshape(-1)
    chains, steps = g["ns_accept"].shape
    noise, scale = g["start_noise"].copy(), g["start_scale"].copy()
    for s in range(steps):
        forests = orc.nodes_from_raw(g["forest_after"][:, s])  # the noise/scale half leaves the forest alone
        state = np.empty((chains, 2))
        for c in range(chains):  # the chain's state after the tree sweep of this step
            Ks = nsr.kernel_matrix(forests[c], noise[c], scale[c], X, ft)
            state[c] = yv @ np.linalg.inv(Ks) @ yv, np.linalg.slogdet(Ks)[1]
        assert np.allclose(0.5 * (-state[:, 0] - state[:, 1]), g["cur_mll"][:, s, -1], **TOL)
        nn, nsc = g["ns_prop"][:, s, 0], g["ns_prop"][:, s, 1]
        new_mll = [nsr.proposal_mll(forests[c], nn[c], nsc[c], X, yv, ft) for c in range(chains)]
        assert np.allclose(new_mll, g["ns_new_mll"][:, s], **TOL)
        acc, state2, K_inv = nsr.step(forests, noise, scale, nn, nsc, g["ns_log_q"][:, s], np.log(g["ns_u"][:, s]), X, y, ft,
                                      state)
        assert np.array_equal(acc, g["ns_accept"][:, s].astype(np.int32)), (s, acc)
        assert np.allclose(0.5 * (-state2[:, 0] - state2[:, 1]), g["mll_after"][:, s], **TOL)
        assert np.array_equal(state2[acc == 0], state[acc == 0])  # rejected chains keep their state, bit for bit
        noise, scale = np.where(acc > 0, nn, noise), np.where(acc > 0, nsc, scale)
        assert np.array_equal(noise, g["noise_after"][:, s]) and np.array_equal(scale, g["scale_after"][:, s])
        for c in range(chains):  # K_inv' belongs to the (noise, scale) the chain ends the step with
            Ks = nsr.kernel_matrix(forests[c], noise[c], scale[c], X, ft)
            assert np.allclose(K_inv[c] @ Ks, np.eye(X.shape[0]), atol=1e-9)


def test_model_flags():
    """NaN draws and a non-positive noise variance reject; a negative scale is flagged -1 for its chain only."""
    g = load_golden("g11_sampler_steps")
    X, y, ft = g["X"], g["y"], g["feat_types"]
    forests = orc.nodes_from_raw(g["start_forest"])
    forests = np.concatenate([forests, forests[:1]])
    noise, scale = np.array([0.1, 0.1, 0.1]), np.array([1.0, 1.0, 1.0])
    state = np.empty((3, 2))
    for c in range(3):
        Ks = nsr.kernel_matrix(forests[c], noise[c], scale[c], X, ft)
        state[c] = y.reshape(-1) @ np.linalg.inv(Ks) @ y.reshape(-1), np.linalg.slogdet(Ks)[1]
    big, lu = np.full(3, 50.0), np.full(3, np.log(0.5))
    run = lambda nn, ns, lq, u: nsr.step(forests, noise, scale, nn, ns, lq, u, X, y, ft, state)[0]  # noqa: E731
    assert run(noise, scale, big, lu).tolist() == [1, 1, 1]
    assert run(noise, scale, big, np.array([np.nan, lu[1], lu[2]])).tolist() == [0, 1, 1]
    assert run(noise, scale, np.array([50.0, np.nan, 50.0]), lu).tolist() == [1, 0, 1]
    assert run(np.array([0.1, 0.1, -1.0]), scale, big, lu).tolist() == [1, 1, 0]
    assert run(noise, np.array([1.0, -5.0, 1.0]), big, lu).tolist() == [1, -1, 1]


@pytest.mark.parametrize("N,R,m,nc", [(64, 20, 8, 1), (130, 257, 8, 3), (4096, 150, 50, 64)])
def test_workspace_covers_the_leafspace_inverse(N, R, m, nc):
    """bark_noise_scale_step_chains_workspace_bytes is a pure host function: the leaf-space inverse layout of one chunk of
    nc forests plus the step's own slots."""
    lib = _lib.lib()
    need = int(lib.bark_noise_scale_step_chains_workspace_bytes(N, R, m, nc))
    assert need >= int(lib.bark_kernel_inverse_leafspace_workspace_bytes(N, R, m, nc)) > 0
    assert need % 256 == 0
    assert int(lib.bark_noise_scale_step_chains_workspace_bytes(N, R, m, 0)) == 0
