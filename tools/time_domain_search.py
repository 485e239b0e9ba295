"""What optimizer.propose_from_domain reaches, and how long it takes, beside what a user did before it existed: torch.rand
candidates in the box, as many as the search scores, through acquisition_scan ("Search over the domain").

  exhaustive   a small problem whose cell grid is enumerated: the exact minimiser
  search       B = 64, m = 50, N = 512, d = 10: multi-start local search from `cells` candidates
  random       the same problem, C uniform candidates in the box in one scan, C = the rows the search scored
  search, budget   the same problem under one linear constraint (the six continuous features sum to at most 2.5): the search
               with constraints=, the repair kernel alone on 2^18 rows, and uniform candidates filtered by hand, as many as
               the search repaired (at most 2^21)
  fit / scan / batch   on the search problem: tree_kernels.fit_posterior alone, one LeafPosterior.scan of 2^18 candidates beside
               the stateless acquisition_scan, and a greedy batch of q = 8 over them with and without posterior=

The exhaustive and search rows are printed twice, with the column reuse_fit false and true (propose_from_domain(reuse_fit=...)):
the same x and value, one fit instead of one per scan.

The value reached is the result; wall time (host clock around the call, which ends in a read-back) is context.  Median of 5
after 2 warm-ups.  Usage: PYTHONPATH=$PWD python tools/time_domain_search.py"""
import json
import time

import numpy as np

WARMUP, REPS = 2, 5


def measure(fn):
    import torch

    for _ in range(WARMUP):
        out = fn()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def main():
    import torch

    import bark_amd.synthetic as syn
    from bark_amd.optimizer import acquisition_scan, domain_plan, propose_batch_from_candidates, propose_from_domain, split_table
    from bark_amd.tree_kernels import fit_posterior

    # exhaustive: d = 4 mixed, 8 forests of 10 trees
    X, y, bounds, ft = syn.mixed_problem(64, seed=1, d_cont=2, n_int=1, n_cat=1, cats=5)
    F = syn.sample_prior_forests(8, 10, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, 8), np.linspace(0.7, 1.4, 8))
    plan = domain_plan(split_table(F, bounds, ft))
    for reuse in (False, True):
        ms, (x, info) = measure(lambda: propose_from_domain(model, (X, y), bounds, ft, return_info=True, reuse_fit=reuse))
        print(json.dumps({"route": "exhaustive", "reuse_fit": reuse, "B": 8, "m": 10, "N": 64, "d": 4, "grid": plan["grid"],
                          "value": info["value"], "scans": info["scans"], "fits": info["fits"], "ms": round(ms, 2)}), flush=True)

    # search: B = 64, m = 50, N = 512, d = 10
    B, m, N = 64, 50, 512
    X, y, bounds, ft = syn.mixed_problem(N, seed=1, d_cont=6)
    F = syn.sample_prior_forests(B, m, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B))
    data = (torch.as_tensor(X, device="cuda"), torch.as_tensor(y, device="cuda"))
    plan = domain_plan(split_table(F, bounds, ft))
    for reuse in (False, True):
        ms, (x, info) = measure(lambda: propose_from_domain(model, data, bounds, ft, seed=5, return_info=True, reuse_fit=reuse))
        scored = 2 ** 18 + info["sweeps"] * 8 * plan["neighbours"]
        print(json.dumps({"route": "search", "reuse_fit": reuse, "B": B, "m": m, "N": N, "d": 10, "grid": float(plan["grid"]),
                          "cells": plan["neighbours"], "value": info["value"], "best_start": float(info["start_values"][0]),
                          "sweeps": info["sweeps"], "scans": info["scans"], "fits": info["fits"], "rows_scored": scored,
                          "ms": round(ms, 2)}), flush=True)

    lo = torch.as_tensor(bounds[:, 0], device="cuda")
    hi = torch.as_tensor(np.where(ft == syn.CAT, 5.0, bounds[:, 1] + (ft == syn.INT)), device="cuda")  # integers, categories: floor
    discrete = torch.as_tensor(ft != syn.CONT, device="cuda")

    def random_route(C):
        gen = torch.Generator(device="cuda").manual_seed(5)
        cand = lo + torch.rand((C, 10), dtype=torch.float64, device="cuda", generator=gen) * (hi - lo)
        cand = torch.where(discrete, cand.floor(), cand)
        value, _ = acquisition_scan(model, data, cand, ft)
        return float(value)

    for C in (2 ** 18, min(scored, 2 ** 24)):
        ms, value = measure(lambda: random_route(C))
        print(json.dumps({"route": "random", "C": C, "value": value, "ms": round(ms, 2)}), flush=True)

    # the search under one budget inequality over the continuous features: sum of the six <= 2.5
    from bark_amd.optimizer import LinearConstraints, cell_boxes, domain_candidates, domain_repair

    budget = LinearConstraints((ft == syn.CONT).astype(np.float64)[None], [2.5])
    ms, (x, info) = measure(lambda: propose_from_domain(model, data, bounds, ft, seed=5, return_info=True, constraints=budget))
    print(json.dumps({"route": "search, budget", "value": info["value"], "best_start": float(info["start_values"][0]),
                      "sweeps": info["sweeps"], "scans": info["scans"], "rows_repaired": info["rows"], "feasible": info["feasible"],
                      "budget_at_x": float(x[ft == syn.CONT].sum()), "ms": round(ms, 2)}), flush=True)
    boxes, table = cell_boxes(F, bounds, ft), split_table(F, bounds, ft)
    cells = domain_candidates(table, bounds, ft, 2 ** 18, "cells", 5)
    ms, (_, ok) = measure(lambda: domain_repair(boxes, ft, budget, cells))  # with the copy that spares the caller's rows
    print(json.dumps({"route": "repair", "rows": 2 ** 18, "touched": 6, "feasible": int(ok.sum()), "ms": round(ms, 3)}), flush=True)
    cont = torch.as_tensor(ft == syn.CONT, device="cuda")

    def filtered_route(C):
        gen = torch.Generator(device="cuda").manual_seed(5)
        cand = lo + torch.rand((6 * C, 10), dtype=torch.float64, device="cuda", generator=gen) * (hi - lo)
        cand = torch.where(discrete, cand.floor(), cand)
        cand = cand[cand[:, cont].sum(dim=1) <= 2.5][:C]  # what a user did by hand: keep the uniform candidates that comply
        value, _ = acquisition_scan(model, data, cand, ft)
        return float(value), int(cand.shape[0])

    ms, (value, kept) = measure(lambda: filtered_route(min(info["rows"], 2 ** 21)))
    print(json.dumps({"route": "random, filtered by hand", "C": kept, "value": value, "ms": round(ms, 2)}), flush=True)

    # the fitted state on the search problem: the fit alone, one scan from it, a greedy batch with and without it
    gen = torch.Generator(device="cuda").manual_seed(6)
    cand = lo + torch.rand((2 ** 18, 10), dtype=torch.float64, device="cuda", generator=gen) * (hi - lo)
    cand = torch.where(discrete, cand.floor(), cand)
    ms, post = measure(lambda: fit_posterior(model, data, ft))
    print(json.dumps({"route": "fit", "B": B, "m": m, "N": N, "R": post.R, "state_bytes": post.nbytes, "ms": round(ms, 2)}), flush=True)
    ms_state, got = measure(lambda: post.scan(cand))
    ms_none, want = measure(lambda: acquisition_scan(model, data, cand, ft))
    print(json.dumps({"route": "scan", "C": 2 ** 18, "from_state_ms": round(ms_state, 2), "stateless_ms": round(ms_none, 2),
                      "same_bits": bool(got[0] == want[0] and got[1] == want[1])}), flush=True)
    ms_state, got = measure(lambda: propose_batch_from_candidates(None, None, cand, None, 8, posterior=post))
    ms_none, want = measure(lambda: propose_batch_from_candidates(model, data, cand, ft, 8))
    print(json.dumps({"route": "batch", "q": 8, "C": 2 ** 18, "from_state_ms": round(ms_state, 2), "stateless_ms": round(ms_none, 2),
                      "same_picks": bool((got[1] == want[1]).all())}), flush=True)


if __name__ == "__main__":
    main()
