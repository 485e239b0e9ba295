"""Noise / scale proposals of the sampler (reference: src/bark/fitting/noise_scale_proposals.py, `get_noise_scale_proposal`).

The reference draws and scores in one function.  Here the two are apart: `draw_normals` gives one standard normal per chain and
parameter from the sampler's Philox stream, `propose` moves (noise, scale) by them, and `log_q_prior` is the pure ratio the
Metropolis step adds to the likelihood difference.  A handful of scalars per step: host numpy.  The formulas, step sizes and
log-densities are the reference's, the sign handling of `get_noise_proposal_softplus` included."""

from __future__ import annotations

import math

import numpy as np

from . import _philox

PROPOSAL_STEP_SIZE = np.array([1.0, 0.00000001])  # noise_scale_proposals.py:11 (the value in force)


def half_normal_logpdf(x, scale):  # noise_scale_proposals.py:15-18; scale is std ** 2
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_normal = -0.5 * (x ** 2) / scale - 0.5 * np.log(scale)
    return np.where(x >= 0, log_normal, -np.inf)


def gamma_logpdf(x, shape, rate):  # noise_scale_proposals.py:22-28
    return (shape - 1) * np.log(x) - rate * x - math.lgamma(shape) + shape * np.log(rate)


def inverse_gamma_logpdf(x, shape, rate):  # noise_scale_proposals.py:32-39
    scale = 1 / rate
    return -(shape + 1) * np.log(x) - scale / x - math.lgamma(shape) + shape * np.log(scale)


def draw_normals(seed: int, step: int, nc: int, chain_offset: int = 0):
    """-> (z (chains, 2): the normals of the noise and of the scale move, log_u (chains,): log of the accept uniform of
    bark_sampler.py:276) of step `step`.  Stream (seed, sweep = step, chain, tree = 0xFFFFFFFF): draws 0, 1 -> z[:, 0] and
    draws 2, 3 -> z[:, 1] by Box-Muller, sqrt(-2 log(1 - a)) cos(2 pi b); draw 4 -> the uniform."""
    u = _philox.uniforms(seed, chain_offset + np.arange(nc), _philox.NOISE_SCALE_TREE, step, 5)
    z = np.sqrt(-2.0 * np.log1p(-u[:, [0, 2]])) * np.cos(2.0 * np.pi * u[:, [1, 3]])
    with np.errstate(divide="ignore"):
        return z, np.log(u[:, 4])


def _check(params):
    if not params.use_softplus_transform and not params.sample_scale:
        raise NotImplementedError("You must sample the scale parameter in the log space")  # noise_scale_proposals.py:78-81


def propose(noise, scale, params, z):
    """The moves of noise_scale_proposals.py:43-67 by the normals z (chains, 2) -> (new_noise, new_scale)."""
    _check(params)
    noise, scale = np.asarray(noise, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if params.use_softplus_transform:
            def move(cur, step, u):  # propose_positive_transition_softplus
                return np.log(np.exp(np.log(np.exp(cur) - 1) + step * u) + 1)
        else:
            def move(cur, step, u):  # propose_positive_transition
                return np.exp(np.log(cur + 1e-30) + step * u)
        new_noise = move(noise, PROPOSAL_STEP_SIZE[0], z[:, 0])
        new_scale = move(scale, PROPOSAL_STEP_SIZE[1], z[:, 1]) if params.sample_scale else scale.copy()
    return new_noise, new_scale


def log_q_prior(noise, scale, new_noise, new_scale, params):
    """log q ratio + log prior ratio of the move (noise, scale) -> (new_noise, new_scale), per chain: the three branches of
    noise_scale_proposals.py:71-156 (log space; softplus with the scale; softplus, noise alone)."""
    _check(params)
    noise, scale, new_noise, new_scale = (np.asarray(v, dtype=np.float64) for v in (noise, scale, new_noise, new_scale))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if not params.use_softplus_transform:
            log_q = -np.log(noise) - np.log(scale) + np.log(new_noise) + np.log(new_scale)
        elif params.sample_scale:
            noise_step_var, scale_step_var = PROPOSAL_STEP_SIZE ** 2
            log_q = (
                (np.log(np.exp(noise) - 1) - np.log(np.exp(new_noise) - 1)) ** 2 / noise_step_var
                + np.log(1 - np.exp(-noise))
                - np.log(1 - np.exp(-new_noise))
                + (np.log(np.exp(scale) - 1) - np.log(np.exp(new_scale) - 1)) ** 2 / scale_step_var
                + np.log(1 - np.exp(-scale))
                - np.log(1 - np.exp(-new_scale))
            )
        else:
            noise_step_var = PROPOSAL_STEP_SIZE[0] ** 2
            log_q = (
                (np.log(np.exp(noise) - 1) - np.log(np.exp(new_noise) - 1)) ** 2 / noise_step_var
                + np.log(1 - np.exp(-noise))
                - np.log(1 - np.exp(-new_noise))
            )
            log_q = log_q * -1
            log_prior = inverse_gamma_logpdf(new_noise, params.gamma_prior_shape, params.gamma_prior_rate) - inverse_gamma_logpdf(
                noise, params.gamma_prior_shape, params.gamma_prior_rate)
            return log_q + log_prior
        log_prior = (half_normal_logpdf(new_noise, 1.0) + half_normal_logpdf(new_scale, 5.0) - half_normal_logpdf(noise, 1.0)
                     - half_normal_logpdf(scale, 5.0))
        return log_q + log_prior


def get_noise_scale_proposal(noise, scale, params, z):
    """`get_noise_scale_proposal` of the reference with its normals passed in: -> ((new_noise, new_scale), log_q_prior)."""
    new_noise, new_scale = propose(noise, scale, params, z)
    return (new_noise, new_scale), log_q_prior(noise, scale, new_noise, new_scale, params)
