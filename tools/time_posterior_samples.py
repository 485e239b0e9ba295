"""Device time of tree_kernels.posterior_samples (leaf-space joint draws) at m = 50 trees, FULL and MAX, beside a numpy
restatement of the same algebra on the host.  Warmed medians of hipEvent pairs around the call on device-resident points
and eps (forests on the host as always, so the time includes the forest upload of the call).

  sweep   the same call with C = 1, S = 1: leaf walk, I + c Z'Z, the R x R sweep with the identity right-hand side, w
  draws   full call - sweep: candidate walk + weights (V'E', MFMA) + gather (+ reduction)
The split of `draws` into the weights and gather kernels comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/time_posterior_samples.py): sample_weights_kernel, sample_gather_kernel.

numpy: M = I + c Z'Z, Cholesky, w, W = c w + sqrt(scale/m) U^-1 E', f = Z_C W per forest (leaf columns from the device
leaf walk, not timed), on the host BLAS threads; timed on up to 8 forests and scaled to B.
Usage: PYTHONPATH=$PWD python tools/time_posterior_samples.py [--reps K] [--shapes B,N,C,S ...] [--no-numpy]"""
import argparse
import json
import os
import time

import numpy as np
import torch

import bark_amd.forest as bf
import bark_amd.synthetic as syn
import bark_amd.tree_kernels as tk

SHAPES = [(1, 128, 1000, 64), (16, 512, 10000, 64), (256, 512, 10000, 16), (256, 4096, 10000, 16)]
M_TREES = 50


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def numpy_draws(F, noise, scale, X, y, cand, ft, S, nb):
    """Host restatement for the first nb forests -> seconds per forest (the leaf walks are not timed)."""
    rng = np.random.default_rng(0)
    N, L = X.shape[0], F.shape[-1]
    total = 0.0
    for b in range(nb):
        leaves = np.concatenate([bf.pass_through_forest(F[b], X, ft), bf.pass_through_forest(F[b], cand, ft)])
        t0 = time.perf_counter()
        uniq, col = np.unique(leaves.astype(np.int64) + np.arange(M_TREES) * L, return_inverse=True)
        col = col.reshape(leaves.shape)
        R = len(uniq)
        Z = np.zeros((N, R))
        Zc = np.zeros((cand.shape[0], R))
        np.put_along_axis(Z, col[:N], 1.0, axis=1)
        np.put_along_axis(Zc, col[N:], 1.0, axis=1)
        s2 = 1e-6 + noise[b]
        c = scale[b] / (M_TREES * s2)
        M = np.eye(R) + c * (Z.T @ Z)
        Lc = np.linalg.cholesky(M)  # M = L L' = U'U with U = L'
        w = np.linalg.solve(M, Z.T @ y.reshape(-1))
        G = np.linalg.solve(Lc.T, rng.standard_normal((S, R)).T)  # U^-1 E'
        W = c * w[:, None] + np.sqrt(scale[b] / M_TREES) * G
        _ = Zc @ W
        total += time.perf_counter() - t0
    return total / nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes] if args.shapes else SHAPES
    rows = []
    for (B, N, C, S) in shapes:
        X, y, bounds, ft = syn.mixed_problem(N, seed=1)
        cand, _, _, _ = syn.mixed_problem(C, seed=2)
        F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=3)
        noise, scale = np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B)
        model = (F, noise, scale)
        R = tk.posterior_sample_dim(F, ft)
        Xd, yd, cd = (torch.as_tensor(v, device="cuda") for v in (X, y, cand))
        eps = torch.randn((B, S, R), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
        eps1 = eps[:, :1].contiguous()
        sweep = device_ms(lambda: tk.posterior_samples(model, (Xd, yd), cd[:1], ft, 1, eps=eps1), args.reps)
        row = {"B": B, "N": N, "C": C, "S": S, "m": M_TREES, "R": R, "sweep_ms": round(sweep, 3)}
        for red in (None, "max"):
            t = device_ms(lambda: tk.posterior_samples(model, (Xd, yd), cd, ft, S, eps=eps, reduce=red), args.reps)
            key = "full" if red is None else "max"
            row[f"{key}_ms"] = round(t, 3)
            row[f"{key}_draws_ms"] = round(t - sweep, 3)
        if not args.no_numpy:
            nb = min(B, 8)
            per = numpy_draws(F, noise, scale, X, y, cand, ft, S, nb)
            row["numpy_ms"] = round(per * B * 1e3, 1)
            row["numpy_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eps, eps1
        torch.cuda.empty_cache()
    print("| B | N | C | S | R | sweep ms | FULL ms | FULL - sweep | MAX ms | MAX - sweep | numpy ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['B']} | {r['N']} | {r['C']} | {r['S']} | {r['R']} | {r['sweep_ms']} | {r['full_ms']} | {r['full_draws_ms']} "
              f"| {r['max_ms']} | {r['max_draws_ms']} | {r.get('numpy_ms', '-')} |")


if __name__ == "__main__":
    main()
