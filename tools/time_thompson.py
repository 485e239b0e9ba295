"""Time of Thompson sampling through sample paths, beside `posterior_samples(reduce="min")` for the same B, S and C.

At B = 64 forests of m = 50 prior trees, N = 512 and C = 2^18 candidates, for S = 1 and S = 16 paths per forest:
  paths    fit_posterior -> sample_paths(S, seed) -> minimise(candidates), and its three parts alone
  samples  tree_kernels.posterior_samples(..., S, eps, reduce="min"): the route that exists without the path object
Device-resident points, candidates and eps; forests on the host as always (both routes upload them).  Wall-clock around a
device synchronisation, the median of `--reps` runs after `--warmup` runs.
Usage: PYTHONPATH=$PWD python tools/time_thompson.py [--reps 5] [--warmup 2] [--shape B,N,C] [--draws 1 16]"""
import argparse
import json
import time

import numpy as np
import torch

import bark_amd.synthetic as syn
import bark_amd.tree_kernels as tk

M_TREES = 50


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default="64,512,262144")
    ap.add_argument("--draws", type=int, nargs="*", default=[1, 16])
    args = ap.parse_args()
    B, N, C = (int(v) for v in args.shape.split(","))
    X, y, bounds, ft = syn.mixed_problem(N, seed=1)
    cand = syn.mixed_problem(C, seed=2)[0]
    F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B))
    Xd, yd, cd = (torch.as_tensor(v, device="cuda") for v in (X, y, cand))
    R = tk.posterior_sample_dim(F, ft)
    for S in args.draws:
        eps = torch.randn((B, S, R), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
        post = tk.fit_posterior(model, (Xd, yd), ft)
        paths = post.sample_paths(S, seed=1)
        row = {"B": B, "N": N, "C": C, "S": S, "m": M_TREES, "R": R,
               "paths_ms": wall_ms(lambda: tk.fit_posterior(model, (Xd, yd), ft).sample_paths(S, seed=1).minimise(cd), args.reps, args.warmup),
               "fit_ms": wall_ms(lambda: tk.fit_posterior(model, (Xd, yd), ft), args.reps, args.warmup),
               "sample_paths_ms": wall_ms(lambda: post.sample_paths(S, seed=1), args.reps, args.warmup),
               "minimise_ms": wall_ms(lambda: paths.minimise(cd), args.reps, args.warmup),
               "samples_ms": wall_ms(lambda: tk.posterior_samples(model, (Xd, yd), cd, ft, S, eps=eps, reduce="min"), args.reps,
                                     args.warmup)}
        print(json.dumps(row), flush=True)
        del eps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
