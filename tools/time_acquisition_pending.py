"""Device time of optimizer.acquisition_scan with pending points, and of a greedy batch, at B = 64 forests of m = 50 prior
trees, N = 256, C = 10^5 (lcb_mean): the scan with P = 0, 8 and 64 pending points, and
propose_batch_from_candidates(q = 8) beside 8 unconditioned scans.  hipEvent medians of 5 after 2 warm-ups on
device-resident points, one process.  Conditioning is expected to add O(P R^2) per forest and to vanish beside the scan.
Usage: PYTHONPATH=$PWD python tools/time_acquisition_pending.py [--B 64 --N 256 --C 100000]"""
import argparse
import json

M_TREES, WARMUP, REPS = 50, 2, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--C", type=int, default=10**5)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bark_amd.synthetic as syn
    import bark_amd.tree_kernels as tk
    from bark_amd.optimizer import acquisition_scan, propose_batch_from_candidates

    def measure(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return round(float(np.median(out)), 3), round(float(min(out)), 3), round(float(max(out)), 3)

    X, y, bounds, ft = syn.mixed_problem(args.N, seed=1)
    cand, _, _, _ = syn.mixed_problem(args.C, seed=2)
    pend, _, _, _ = syn.mixed_problem(64, seed=4)
    F = syn.sample_prior_forests(args.B, M_TREES, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, args.B), np.linspace(0.7, 1.4, args.B))
    Xd, yd, cd, pd = (torch.as_tensor(v, device="cuda") for v in (X, y, cand, pend))
    row = {"B": args.B, "N": args.N, "C": args.C, "m": M_TREES, "R": tk.posterior_sample_dim(F, ft), "ms": "median, min, max"}
    row["scan_existing_entry"] = measure(lambda: acquisition_scan(model, (Xd, yd), cd, ft))
    for P in (0, 8, 64):
        row[f"scan_P{P}"] = measure(lambda: acquisition_scan(model, (Xd, yd), cd, ft, pending=pd[:P]))
    row["batch_q8"] = measure(lambda: propose_batch_from_candidates(model, (Xd, yd), cd, ft, 8))
    row["eight_unconditioned_scans"] = measure(lambda: [acquisition_scan(model, (Xd, yd), cd, ft) for _ in range(8)])
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
