"""Device time of the fidelity information gain (LeafPosterior.information_gain, bark_fidelity_gain_fitted_hip) at m = 50 prior
trees beside the reference's formulation in torch on the device: per forest the (G, C, S) arrays of _entropy_low_fidelity
(information_based_fidelity.py:90-167), candidates in blocks so that the arrays fit, then the mean over the forests.
hipEvent medians of 5 after 2 warm-ups on device-resident points and targets, one process per row.

  gain ms     the library call from the fitted state (walks, moments, quadrature, sums)
  ns/eval     gain ms / (B C S (n_a + G)): per grid-point-and-target evaluation, as if every pair were separated
  torch ms    the quadrature alone: its five moments per (forest, pair) come from the dense route on the host and are not
              timed, so the comparison favours torch
  max_diff    largest |library - torch| over the gains.  The two differ by design where a forest does not separate a pair: the
              library takes the closed form there, torch integrates with s^2 = 0 as the reference does
Usage: PYTHONPATH=$PWD python tools/time_fidelity_gain.py [--rows S,B,N,C ...]"""
import argparse
import json
import math
import subprocess
import sys

ROWS = [(100, 64, 512, 1), (100, 64, 512, 256), (100, 64, 512, 4096)]
M_TREES = 50
WARMUP, REPS = 2, 5
GRID = (-10.0, 10.0, 100, 0.25, 250)
BLOCK = 1 << 25  # elements of a (G, c, S) array


def torch_route(torch, mom, targets):
    """mom: five (B, C) device tensors, targets (B, S) -> gains (C,)"""
    lo, hi, n_a, pad, G = GRID
    Phi = lambda z: 0.5 * torch.erfc(-z / math.sqrt(2))  # noqa: E731
    phi = lambda z: torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)  # noqa: E731
    B, C = mom[0].shape
    S = targets.shape[1]
    step = max(1, BLOCK // (G * S))
    total = torch.zeros(C, dtype=torch.float64, device=targets.device)
    fk = torch.linspace(lo, hi, n_a, dtype=torch.float64, device=targets.device).reshape(-1, 1, 1)
    unit = torch.linspace(0.0, 1.0, G, dtype=torch.float64, device=targets.device).reshape(-1, 1, 1)
    for b in range(B):
        t = targets[b].reshape(1, 1, S)
        for c0 in range(0, C, step):
            mu_m, var_m, mu_0, var_0, cov = (v[b, c0:c0 + step].reshape(1, -1, 1) for v in mom)
            sd_m, sd_0 = var_m.clamp_min(0).sqrt(), var_0.clamp_min(0).sqrt()
            ssd = (var_0 - cov ** 2 / (var_m + 1e-9)).clamp_min(0).sqrt() + 1e-9
            Z = 1.0 / (Phi((t - mu_0) / (sd_0 + 1e-9)) * sd_m + 1e-10)

            def Psi(f):
                u = mu_0 + cov * (f - mu_m) / (var_m + 1e-9)
                return Phi((t - u) / ssd) * phi((f - mu_m) / (sd_m + 1e-9))

            live = Psi(fk).abs().sum(dim=-1, keepdim=True) > 1e-8
            fmin = torch.where(live, fk, math.inf).amin(dim=0, keepdim=True) - pad
            fmax = torch.where(live, fk, -math.inf).amax(dim=0, keepdim=True) + pad
            z = Z * Psi(fmin + unit * (fmax - fmin))
            yv = torch.special.xlogy(z, z)
            h = (fmax - fmin) / (G - 1)
            integral = (h * (yv.sum(dim=0, keepdim=True) - 0.5 * (yv[:1] + yv[-1:]))).mean(dim=-1)
            total[c0:c0 + step] += (torch.log(sd_m * math.sqrt(2 * math.pi * math.e)).reshape(-1) + integral.reshape(-1))
    return total / B


def host_moments(np, bf, model, data, query, target, ft):
    """the dense route: mu_m, var_m, mu_0, var_0, cov, each (B, C)"""
    F, noise, scale = model
    X, y = data
    C = query.shape[0]
    P = np.concatenate([query, target])
    s = scale[:, None, None]
    K_inv = np.linalg.inv(s * bf.batched_forest_gram_matrix(F, X, X, ft) + (1e-6 + noise[:, None, None]) * np.eye(X.shape[0]))
    K_pX = s * bf.batched_forest_gram_matrix(F, P, X, ft)
    mu = (K_pX @ K_inv @ y.reshape(-1, 1))[:, :, 0]
    i = np.arange(C)
    K_pp = s * bf.batched_forest_gram_matrix(F, P, P, ft)
    half = K_pX @ K_inv
    var = K_pp[:, np.arange(2 * C), np.arange(2 * C)] - np.einsum("bpn,bpn->bp", half, K_pX)
    cov = K_pp[:, i, C + i] - np.einsum("bpn,bpn->bp", half[:, :C], K_pX[:, C:])
    return mu[:, :C], var[:, :C], mu[:, C:], var[:, C:], cov


def one(S, B, N, C):
    import numpy as np
    import torch

    import bark_amd.forest as bf
    import bark_amd.synthetic as syn
    from bark_amd.optimizer import fstar_at_fidelity, with_fidelity
    from bark_amd.tree_kernels import fit_posterior

    def measure(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out)), res

    # the last categorical column of the mixed problem is the fidelity; level 0 is the target
    X, y, bounds, ft = syn.mixed_problem(N, seed=1)
    x, _, _, _ = syn.mixed_problem(C, seed=2)
    j = X.shape[1] - 1
    F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B))
    post = fit_posterior(model, (X, y), ft)
    x[:, j] = 1.0 + (np.arange(C) % 2)
    query, target = x, with_fidelity(x, j, 0)
    targets = fstar_at_fidelity(post, X, fidelity_feature=j, target=0, num_samples=S, seed=4)
    qd, td = (torch.as_tensor(v, device="cuda") for v in (query, target))
    row = {"S": S, "B": B, "N": N, "C": C, "m": M_TREES, "R": post.R}
    gain_ms, gain = measure(lambda: post.information_gain(qd, td, targets))
    row.update(gain_ms=round(gain_ms, 3), ns_per_eval=round(gain_ms * 1e6 / (B * C * S * (GRID[2] + GRID[4])), 5))
    mom = [torch.as_tensor(np.ascontiguousarray(v), device="cuda") for v in host_moments(np, bf, model, (X, y), query, target, ft)]
    try:
        torch_ms, ref = measure(lambda: torch_route(torch, mom, targets))
        row.update(torch_ms=round(torch_ms, 3), speedup=round(torch_ms / gain_ms, 2), max_diff=float((ref - gain).abs().max().item()))
    except (ValueError, MemoryError, RuntimeError) as exc:
        row["torch_error"] = f"{type(exc).__name__}: {exc}"[:200]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=None, help="S,B,N,C")
    ap.add_argument("--one", default=None, help="S,B,N,C: measure this row in this process")
    args = ap.parse_args()
    if args.one:
        one(*(int(v) for v in args.one.split(",")))
        return
    rows_in = [tuple(r.split(",")) for r in args.rows] if args.rows else ROWS
    rows = []
    for r in rows_in:  # a fresh process per row; this one never opens the device
        spec = ",".join(map(str, r))
        try:
            p = subprocess.run([sys.executable, __file__, "--one", spec], capture_output=True, text=True, timeout=400)
        except subprocess.TimeoutExpired:
            print(f"row {spec}: no result after 400 s", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode or not line:
            print(f"row {spec}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            break  # nothing more is started on the device after a failure
        print(line[-1], flush=True)
        rows.append(json.loads(line[-1]))
    print("| S | B | N | C | R | gain ms | ns / eval | torch ms | speed-up | max diff |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['S']} | {r['B']} | {r['N']} | {r['C']} | {r['R']} | {r['gain_ms']} | {r['ns_per_eval']} "
              f"| {r.get('torch_ms', r.get('torch_error', '-'))} | {r.get('speedup', '-')} | {r.get('max_diff', '-')} |")


if __name__ == "__main__":
    main()
