"""Float64 host model of the noise/scale half of the sampler step for a batch of chains (bark_sampler.py:266-282), numpy
and the oracle only: what `ChainBatch.step_noise_scale` / `bark_noise_scale_step_chains_hip` must decide and leave behind.

Per chain b, with K_s(noise, scale) = scale K_b + (1e-6 + noise) I and state[b] = (y'K^-1 y, log|K|) of the chain:

    new_mll   = oracle.batched_mll at (new_noise[b], new_scale[b])      (inv + slogdet, scale included, no 2 pi)
    cur_mll   = 0.5 (-state[b, 0] - state[b, 1])
    accept[b] =  1  iff log_u[b] <= log_q[b] + (new_mll - cur_mll) and log_u[b] <= 0     (a NaN compares false)
                 0  otherwise, and whenever 1e-6 + new_noise[b] is not positive (log of it is NaN)
                -1  K_s at the proposed values is not positive definite although 1e-6 + new_noise[b] > 0 (the device meets a
                    non-positive pivot of I + c Z'Z, which has the sign pattern of K_s / s2)
                -2  for every chain, when a walk meets an invalid categorical value (the oracle raises ValueError)

Accepted chains get state' = (y'K_s^-1 y, -2 new_mll - y'K_s^-1 y) and K_inv' = inv(K_s) at the proposed values; every other
chain keeps its state, and its K_inv' is inv(K_s) at its current (noise, scale)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc


def kernel_matrix(forest, noise, scale, X, ft):
    K = orc.forest_gram_matrix(forest, X, X, ft)
    return scale * K + (1e-6 + noise) * np.eye(K.shape[0])


def proposal_mll(forest, noise, scale, X, y, ft):
    """MLL of one forest in the sampler's convention (bark_sampler.py:267-272)."""
    return orc.batched_mll(np.asarray(forest)[None], [noise], [scale], X, y, ft, include_scale=True, include_2pi=False)[0]


def log_alpha(log_q, new_mll, state):
    state = np.asarray(state, dtype=np.float64).reshape(-1, 2)
    cur_mll = 0.5 * (-state[:, 0] - state[:, 1])
    return np.asarray(log_q, dtype=np.float64) + (np.asarray(new_mll, dtype=np.float64) - cur_mll)


def decide(log_q, log_u, new_mll, state):
    """The Metropolis rule alone -> (chains,) bool."""
    log_u = np.asarray(log_u, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (log_u <= log_alpha(log_q, new_mll, state)) & (log_u <= 0.0)


def step(forests, noise, scale, new_noise, new_scale, log_q, log_u, X, y, ft, state):
    """-> (accept (chains,) int32, state' (chains, 2), K_inv' (chains, N, N))."""
    forests = np.asarray(forests)
    nc = forests.shape[0]
    X = np.asarray(X, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    vec = lambda v: np.asarray(v, dtype=np.float64).reshape(-1)  # noqa: E731
    noise, scale, new_noise, new_scale, log_q, log_u = (vec(v) for v in (noise, scale, new_noise, new_scale, log_q, log_u))
    state = np.array(state, dtype=np.float64).reshape(nc, 2)
    accept = np.zeros(nc, dtype=np.int32)
    K_inv = np.empty((nc, X.shape[0], X.shape[0]))
    try:
        for b in range(nc):
            orc.pass_through_forest(forests[b], X, ft)
    except ValueError:
        accept[:] = -2
        return accept, state, None
    for b in range(nc):
        K_inv[b] = np.linalg.inv(kernel_matrix(forests[b], noise[b], scale[b], X, ft))
        if not (1e-6 + new_noise[b] > 0.0):
            continue
        Ks = kernel_matrix(forests[b], new_noise[b], new_scale[b], X, ft)
        try:
            np.linalg.cholesky(Ks)
        except np.linalg.LinAlgError:
            accept[b] = -1
            continue
        new_mll = proposal_mll(forests[b], new_noise[b], new_scale[b], X, yv, ft)
        if decide(log_q[b : b + 1], log_u[b : b + 1], [new_mll], state[b])[0]:
            accept[b] = 1
            K_inv[b] = np.linalg.inv(Ks)
            quad = float(yv @ K_inv[b] @ yv)
            state[b] = quad, -2.0 * new_mll - quad
    return accept, state, K_inv
