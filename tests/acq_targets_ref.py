"""Host reference of the acquisition scan's target kinds (numpy and the standard library only, no GPU): expected
improvement, probability of improvement and min-value entropy search, shared by tests/test_acquisition_targets_cpu.py and
tests/test_gpu_acquisition_targets.py.

Written from the formulas of include/bark_hip.h, not from the kernel, in float64 on (mu, var) of `acq_ref.posterior`
(the oracle's dense LU route).  With sd = sqrt(max(var, 0)), Phi(z) = erfc(-z / sqrt 2) / 2, phi(z) = exp(-z^2 / 2) / sqrt(2 pi):
    ei:   z = (t - mu) / sd,  g = (t - mu) Phi(z) + sd phi(z)                 (sd == 0: max(t - mu, 0))
    pi:   g = Phi(z)                                                          (sd == 0: t > mu)
    mes:  gam = (t - mu) / (sd + 1e-7), inner = sqrt(2 pi e) sd Phi(gam) (1e-10 where <= 0),
          g = log(sd sqrt(2 pi e)) - (log(inner) - gam phi(gam) / (2 Phi(gam) + 1e-10))
    acq[x] = -mean_b mean_s g(mu_b(x), sd_b(x), t[b][s])
(mes is the reference's information_based_fidelity.py:39-87 at the target fidelity, with its guards).

Targets.  With the incumbent min(y) as the one target the utilities of some cases are about 1e-14 with gaps to match,
which no index test survives, so the targets come from the reference's own posterior: t[b][s] is a low quantile of mu_b
over the case's candidates, S = 1 (level 0.25) or S = 5 (levels 0.05 ... 0.5), which keeps z of order one for a good
share of the candidates.

Bar.  The device posterior is held to rtol 1e-9 / atol 1e-8 and the utilities amplify that, so the
bar of a case and kind is that posterior bar pushed through the formula: the acquisition at the four corners
mu +- (1e-9 |mu| + 1e-8), var +- (1e-9 |var| + 1e-8), and per candidate the largest change against the centre.

`precheck` establishes per case and kind that every var is at least VAR_FLOOR, that the best value is MARGIN below the
runner-up (the device index has to be equal, not close), and that float64 agrees with a 50-digit mpmath evaluation of
the same formulas within 1 % of the bar on at most 2000 (candidate, forest, target) triples, the arg-min's and the
runner-up's among them."""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

import acq_pending_ref as apr
import acq_ref as ar

KINDS = ("ei", "pi", "mes")
RTOL, ATOL = ar.RTOL, ar.ATOL
MARGIN, VAR_FLOOR = ar.MARGIN, ar.VAR_FLOOR
AGREE = 0.01  # float64 against mpmath: this fraction of the bar
MP_DIGITS = 50
MP_TRIPLES = 2000
LEVELS = {1: np.array([0.25]), 5: np.linspace(0.05, 0.5, 5)}
# S per case: 1 and 5 alternate over the case table, the chunked case and the tree-limit cases get one of each
S_OF = {"prior_n64": 5, "prior_n257_chunks": 5, "m1_r64": 1, "m2_r65": 5, "m13_lds_limit": 1, "m13_past_lds": 5,
        "m64_r128": 1, "m64_r256": 5}
MIN_SURVIVORS = 6
# the cases the GPU tests run per kind: those that pass `precheck` (tests/test_acquisition_targets_cpu.py holds the two equal)
CASES = {kind: tuple(ar.CASES) for kind in KINDS}
PENDING_CASE = "n64_m13_p2"  # of acq_pending_ref: two pending points
GREEDY_CASE, GREEDY_Q = "greedy_q4_n64", 3  # its forests, data, candidates and pending points; three picks
SQRT_2PI_E = math.sqrt(2.0 * math.pi * math.e)

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def Phi(z):
    return 0.5 * _erfc(-np.asarray(z, dtype=np.float64) / math.sqrt(2.0))


def phi(z):
    z = np.asarray(z, dtype=np.float64)
    return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def utility(mu, sd, t, kind):
    """g of the header, element-wise over broadcastable float64 arrays"""
    mu, sd, t = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(sd, dtype=np.float64),
                                    np.asarray(t, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "mes":
            gam = (t - mu) / (sd + 1e-7)
            cdf, pdf = Phi(gam), phi(gam)
            inner = SQRT_2PI_E * sd * cdf
            inner = np.where(inner <= 0, 1e-10, inner)
            return np.log(sd * SQRT_2PI_E) - (np.log(inner) - gam * pdf / (2.0 * cdf + 1e-10))
        z = (t - mu) / sd
        if kind == "ei":
            return np.where(sd > 0, (t - mu) * Phi(z) + sd * phi(z), np.maximum(t - mu, 0.0))
        if kind == "pi":
            return np.where(sd > 0, Phi(z), (t > mu).astype(np.float64))
    raise ValueError(kind)


def acquisition(mu, var, targets, kind):
    """mu, var (B, C), targets (B, S) -> (C,): the negated mean over forests of the mean over targets"""
    mu, var, targets = (np.asarray(v, dtype=np.float64) for v in (mu, var, targets))
    sd = np.sqrt(np.maximum(var, 0.0))
    g = utility(mu[:, :, None], sd[:, :, None], targets[:, None, :], kind)  # (B, C, S)
    return -np.mean(np.mean(g, axis=2), axis=0)


def propagated_bar(mu, var, targets, kind):
    """(C,): the posterior bar pushed through the formula (the four corners; see the module docstring)"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    centre = acquisition(mu, var, targets, kind)
    dmu, dvar = RTOL * np.abs(mu) + ATOL, RTOL * np.abs(var) + ATOL
    bar = np.zeros_like(centre)
    for sm in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            bar = np.maximum(bar, np.abs(acquisition(mu + sm * dmu, var + sv * dvar, targets, kind) - centre))
    return bar


def quantile_targets(mu, S):
    """(B, S): row b the LEVELS[S] quantiles of mu_b over the candidates"""
    out = np.quantile(np.asarray(mu, dtype=np.float64), LEVELS[S], axis=1).T.copy()
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def targets_of(name, S=None):
    """of a case of acq_ref.CASES by name (S: S_OF[name]), or of an acq_ref.Case with S given"""
    mu, _ = ar.posterior(name)
    return quantile_targets(mu, S_OF[name] if S is None else S)


@lru_cache(maxsize=None)
def reference(name, kind, S=None):
    """-> (values (C,), bar (C,)) of a case"""
    mu, var = ar.posterior(name)
    t = targets_of(name, S)
    v, bar = acquisition(mu, var, t, kind), propagated_bar(mu, var, t, kind)
    v.setflags(write=False)
    bar.setflags(write=False)
    return v, bar


def bar_used(got, want, bar):
    """largest fraction of the propagated bar used; the caller asserts <= 1"""
    return float((np.abs(np.asarray(got) - want) / bar).max())


def _mp_utility(mp, mu, sd, t, kind):
    mu, sd, t = mp.mpf(float(mu)), mp.mpf(float(sd)), mp.mpf(float(t))
    Phi_ = lambda z: mp.erfc(-z / mp.sqrt(2)) / 2  # noqa: E731
    phi_ = lambda z: mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)  # noqa: E731
    E = mp.sqrt(2 * mp.pi * mp.e)
    if kind == "mes":
        gam = (t - mu) / (sd + mp.mpf(1e-7))
        cdf, pdf = Phi_(gam), phi_(gam)
        inner = E * sd * cdf
        if inner <= 0:
            inner = mp.mpf(1e-10)
        return mp.log(sd * E) - (mp.log(inner) - gam * pdf / (2 * cdf + mp.mpf(1e-10)))
    z = (t - mu) / sd
    return (t - mu) * Phi_(z) + sd * phi_(z) if kind == "ei" else Phi_(z)


def check_against_mpmath(mu, var, targets, kind, must=()):
    """float64 against mpmath on at most MP_TRIPLES triples (all of the candidates in `must` first, the rest drawn with a
    fixed seed); -> the largest fraction of the bar used.  sd is formed in float64 (it is the formulas' input)."""
    import mpmath as mp

    mp.mp.dps = MP_DIGITS
    mu, var, targets = (np.asarray(v, dtype=np.float64) for v in (mu, var, targets))
    B, C = mu.shape
    S = targets.shape[1]
    sd = np.sqrt(np.maximum(var, 0.0))
    bar = propagated_bar(mu, var, targets, kind)
    triples = [(c, b, s) for c in must for b in range(B) for s in range(S)]
    rng = np.random.default_rng(12345)
    left = MP_TRIPLES - len(triples)
    total = C * B * S
    for flat in (rng.choice(total, size=min(left, total), replace=False) if left > 0 else ()):
        triples.append((int(flat) // (B * S), (int(flat) // S) % B, int(flat) % S))
    worst = 0.0
    for c, b, s in triples:
        g64 = float(utility(mu[b, c], sd[b, c], targets[b, s], kind))
        gmp = _mp_utility(mp, mu[b, c], sd[b, c], targets[b, s], kind)
        worst = max(worst, float(abs(mp.mpf(g64) - gmp)) / float(bar[c]))
    # the whole value of the candidates that decide the index
    for c in must:
        total_mp = -sum(sum(_mp_utility(mp, mu[b, c], sd[b, c], targets[b, s], kind) for s in range(S)) / S for b in range(B)) / B
        worst = max(worst, float(abs(mp.mpf(float(acquisition(mu[:, c:c + 1], var[:, c:c + 1], targets, kind)[0])) - total_mp))
                    / float(bar[c]))
    return worst


@lru_cache(maxsize=None)
def precheck(name, kind):
    """-> (values float64 (C,), bar (C,), arg-min); raises AssertionError where a case is unfit for an exact index test"""
    mu, var = ar.posterior(name)
    assert var.min() >= VAR_FLOOR, (name, float(var.min()))
    v, bar = reference(name, kind)
    assert np.isfinite(v).all() and np.isfinite(bar).all() and (bar > 0).all(), (name, kind)
    i = int(np.argmin(v))
    must = [i]
    if v.size > 1:
        rest = np.delete(v, i)
        gap = float(rest.min() - v[i])
        assert gap >= MARGIN, (name, kind, gap)
        assert float(bar.max()) < gap / 2, (name, kind, float(bar.max()), gap)  # within the bar the index cannot move
        j = int(np.argmin(rest))
        must.append(j + (j >= i))
    used = check_against_mpmath(mu, var, targets_of(name), kind, must)
    assert used <= AGREE, (name, kind, used)
    return v, bar, i


@lru_cache(maxsize=None)
def survivors(kind):
    """names of acq_ref.CASES that pass `precheck` for the kind (the single-candidate case always counts)"""
    out = []
    for name in ar.CASES:
        try:
            precheck(name, kind)
        except AssertionError:
            continue
        out.append(name)
    return tuple(out)


@lru_cache(maxsize=None)
def pending_reference():
    """EI conditioned on the pending points of PENDING_CASE, from acq_pending_ref's dense route (the training inputs
    augmented by the pending points) -> (targets (B, 5), skip, values (C,), bar (C,), arg-min outside skip).  The one skipped
    candidate is the winner of the unrestricted scan."""
    case = apr.CASES[PENDING_CASE]
    mu, var = apr.dense(ar.make_inputs(case.base), apr.pending_of(PENDING_CASE))
    t = quantile_targets(mu, 5)
    v, bar = acquisition(mu, var, t, "ei"), propagated_bar(mu, var, t, "ei")
    skip = (int(np.argmin(v)),)
    return t, skip, v, bar, apr.gap_of(v, skip)[0]


@lru_cache(maxsize=None)
def greedy_ei():
    """the loop of `propose_batch_from_candidates(kind="ei", q=GREEDY_Q)` over the dense route
    -> (targets (B, 5), picks (q,), the acquisition vector of every pick [(C,)], its bar [(C,)])"""
    case = apr.CASES[GREEDY_CASE]
    inp = ar.make_inputs(case.base)
    pend = apr.pending_of(GREEDY_CASE)
    t = quantile_targets(apr.dense(inp, None)[0], 5)  # the believer's conditioning leaves the means where they are
    picks, vecs, bars = [], [], []
    for _ in range(GREEDY_Q):
        cur = np.concatenate([pend, inp.cand[picks]], axis=0) if picks else pend
        mu, var = apr.dense(inp, cur)
        vecs.append(acquisition(mu, var, t, "ei"))
        bars.append(propagated_bar(mu, var, t, "ei"))
        picks.append(apr.gap_of(vecs[-1], picks)[0])
    return t, np.asarray(picks), vecs, bars
