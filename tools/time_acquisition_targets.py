"""Device time of the acquisition scan's target kinds at m = 50 prior trees beside the lcb_mean scan of the same build and
beside the route a user had before them: forest_predict(method="leafspace") (two (B, C) arrays) + the formula in torch
(one pass over the (B, C) arrays per target, so no (B, C, S) array is ever formed), the mean over forests and the arg-min.
hipEvent medians of 5 after 2 warm-ups on device-resident points and targets, one process per row.

  scan ms     the call (leaf-space sweep of every chunk included)
  lcb ms      acquisition_scan(kind="lcb_mean") on the same inputs: the cost of everything but the utility
  ns/triple   (scan - lcb) / (B C S): what one (candidate, forest, target) evaluation adds
  torch ms    the route above; same_index / value_diff compare its result with the scan's
Usage: PYTHONPATH=$PWD python tools/time_acquisition_targets.py [--rows kind,S,B,N,C ...]"""
import argparse
import json
import math
import subprocess
import sys

ROWS = [("ei", 1, 64, 512, 10**6), ("pi", 1, 64, 512, 10**6), ("mes", 100, 64, 512, 10**6)]
M_TREES = 50
WARMUP, REPS = 2, 5


def torch_route(tk, torch, model, data, cand, ft, kind, targets):
    mu, var = tk.forest_predict(model, data, cand, ft, method="leafspace")
    sd = var.clamp_min(0).sqrt()
    E = math.sqrt(2 * math.pi * math.e)
    total = torch.zeros_like(mu)
    for s in range(targets.shape[1]):
        t = targets[:, s:s + 1]
        if kind == "mes":
            gam = (t - mu) / (sd + 1e-7)
            cdf = 0.5 * torch.erfc(-gam / math.sqrt(2))
            pdf = torch.exp(-0.5 * gam * gam) / math.sqrt(2 * math.pi)
            inner = E * sd * cdf
            inner = inner.masked_fill(inner <= 0, 1e-10)
            total += torch.log(sd * E) - (torch.log(inner) - gam * pdf / (2 * cdf + 1e-10))
        else:
            z = (t - mu) / sd
            cdf = 0.5 * torch.erfc(-z / math.sqrt(2))
            total += cdf if kind == "pi" else (t - mu) * cdf + sd * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    acq = -(total / targets.shape[1]).mean(dim=0)
    return acq.min(), acq.argmin()


def one(kind, S, B, N, C):
    import numpy as np
    import torch

    import bark_amd.synthetic as syn
    import bark_amd.tree_kernels as tk
    from bark_amd import _lib
    from bark_amd.optimizer import acquisition_plan, acquisition_scan

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

    X, y, bounds, ft = syn.mixed_problem(N, seed=1)
    cand, _, _, _ = syn.mixed_problem(C, seed=2)
    F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B))
    R = tk.posterior_sample_dim(F, ft)
    Xd, yd, cd = (torch.as_tensor(v, device="cuda") for v in (X, y, cand))
    # targets below the bulk of the data, S per forest: an incumbent-like spread, not tuned to the model
    lo, mid = float(np.quantile(y, 0.02)), float(np.quantile(y, 0.3))
    targets = torch.linspace(lo, mid, B * S, dtype=torch.float64, device="cuda").reshape(S, B).T.contiguous()
    row = {"kind": kind, "S": S, "B": B, "N": N, "C": C, "m": M_TREES, "R": R, "variant": acquisition_plan(R, M_TREES)["variant"]}

    scan_ms, (best, idx) = measure(lambda: acquisition_scan(model, (Xd, yd), cd, ft, kind=kind, targets=targets))
    lcb_ms, _ = measure(lambda: acquisition_scan(model, (Xd, yd), cd, ft, kind="lcb_mean"))
    row.update(scan_ms=round(scan_ms, 3), lcb_ms=round(lcb_ms, 3),
               ns_per_triple=round((scan_ms - lcb_ms) * 1e6 / (B * C * S), 5))
    _lib.release_workspace()
    torch.cuda.empty_cache()
    try:
        torch_ms, (pbest, pidx) = measure(lambda: torch_route(tk, torch, model, (Xd, yd), cd, ft, kind, targets))
        row.update(torch_ms=round(torch_ms, 3), speedup=round(torch_ms / scan_ms, 2), same_index=bool(pidx.item() == idx.item()),
                   value_diff=float(abs(pbest.item() - best.item())))
    except (ValueError, MemoryError, RuntimeError) as exc:  # the (B, C) arrays over the budget
        row["torch_error"] = f"{type(exc).__name__}: {exc}"[:200]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=None, help="kind,S,B,N,C")
    ap.add_argument("--one", default=None, help="kind,S,B,N,C: measure this row in this process")
    args = ap.parse_args()
    if args.one:
        k, *rest = args.one.split(",")
        one(k, *(int(v) for v in rest))
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
    print("| kind | S | B | N | C | R | variant | scan ms | lcb_mean ms | ns / triple | torch ms | speed-up |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['kind']} | {r['S']} | {r['B']} | {r['N']} | {r['C']} | {r['R']} | {r['variant']} | {r['scan_ms']} | {r['lcb_ms']} "
              f"| {r['ns_per_triple']} | {r.get('torch_ms', r.get('torch_error', '-'))} | {r.get('speedup', '-')} |")


if __name__ == "__main__":
    main()
