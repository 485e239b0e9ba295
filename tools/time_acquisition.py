"""Device time of optimizer.acquisition_scan at m = 50 prior trees beside the route it replaces:
forest_predict(method="leafspace") (two (B, C) arrays) + the reduction over the forests and the arg-min in torch.
hipEvent medians of 5 after 2 warm-ups on device-resident points, one process per shape.

  scan      the call
  sweep     the same call with one candidate: leaf walk, I + c Z'Z, the R x R sweep with the identity right-hand side,
            w, M^-1 per chunk — what both routes share
  share     (scan - sweep) / scan: the candidate walk, acq_scan_kernel and the finish
  lds B/clk the table reads of acq_scan_kernel, B C m (m + 1) / 2 doubles, over (scan - sweep) on 256 CUs at 2.4 GHz,
            against the 256 B/clk/CU of ds_read_b64 (a lower bound of the kernel's own rate: the walk is in the time)
  extra MB  torch.cuda.max_memory_allocated over the call + the library's workspace: outputs, intermediates, scratch
Usage: PYTHONPATH=$PWD python tools/time_acquisition.py [--shapes B,N,C ...] [--kind lcb_mean] [--variant auto]"""
import argparse
import json
import subprocess
import sys

SHAPES = [(4, 64, 10**4), (20, 128, 10**5), (256, 512, 10**5), (256, 4096, 10**6)]
M_TREES = 50
WARMUP, REPS = 2, 5


def one(B, N, C, kind, variant):
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
        _lib.release_workspace()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        extra = torch.cuda.max_memory_allocated() - base + _lib.workspace_bytes()
        return float(np.median(out)), extra / 2**20, res

    X, y, bounds, ft = syn.mixed_problem(N, seed=1)
    cand, _, _, _ = syn.mixed_problem(C, seed=2)
    F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=3)
    model = (F, np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B))
    R = tk.posterior_sample_dim(F, ft)
    Xd, yd, cd = (torch.as_tensor(v, device="cuda") for v in (X, y, cand))
    row = {"B": B, "N": N, "C": C, "m": M_TREES, "R": R, "kind": kind, "variant": acquisition_plan(R, M_TREES, variant)["variant"]}

    scan_ms, scan_mb, (best, idx) = measure(lambda: acquisition_scan(model, (Xd, yd), cd, ft, kind=kind, variant=variant))
    sweep_ms, _, _ = measure(lambda: acquisition_scan(model, (Xd, yd), cd[:1], ft, kind=kind, variant=variant))
    row.update(scan_ms=round(scan_ms, 3), sweep_ms=round(sweep_ms, 3), share=round((scan_ms - sweep_ms) / scan_ms, 3),
               scan_extra_mb=round(scan_mb, 1))
    reads = B * C * M_TREES * (M_TREES + 1) / 2 * 8
    row["lds_bytes_per_clk_cu"] = round(reads / (max(scan_ms - sweep_ms, 1e-6) * 1e-3 * 2.4e9 * 256), 1)

    def parent():
        mu, var = tk.forest_predict(model, (Xd, yd), cd, ft, method="leafspace")
        if kind == "lcb_mean":
            acq = (mu - 1.96 * var.clamp_min(0).sqrt()).mean(dim=0)
        else:
            mu_y = mu.mean(dim=0)
            var_y = (var + mu**2).mean(dim=0) - mu_y**2
            acq = mu_y - 1.96 * var_y.clamp_min(0).sqrt()
        return acq.min(), acq.argmin()

    try:
        parent_ms, parent_mb, (pbest, pidx) = measure(parent)
        row.update(parent_ms=round(parent_ms, 3), parent_extra_mb=round(parent_mb, 1), speedup=round(parent_ms / scan_ms, 2),
                   same_index=bool(pidx.item() == idx.item()), value_diff=float(abs(pbest.item() - best.item())))
    except (ValueError, MemoryError, RuntimeError) as exc:  # the (B, C) outputs or its workspace over the budget
        row["parent_error"] = f"{type(exc).__name__}: {exc}"[:200]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--kind", default="lcb_mean")
    ap.add_argument("--variant", default="auto")
    ap.add_argument("--one", default=None, help="B,N,C: measure this shape in this process")
    args = ap.parse_args()
    if args.one:
        one(*(int(v) for v in args.one.split(",")), args.kind, args.variant)
        return
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes] if args.shapes else SHAPES
    rows = []
    for s in shapes:  # a fresh process per shape; this one never opens the device
        try:
            p = subprocess.run([sys.executable, __file__, "--one", ",".join(map(str, s)), "--kind", args.kind, "--variant", args.variant],
                               capture_output=True, text=True, timeout=400)
        except subprocess.TimeoutExpired:
            print(f"shape {s}: no result after 400 s", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode or not line:
            print(f"shape {s}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            break  # nothing more is started on the device after a failure
        print(line[-1], flush=True)
        rows.append(json.loads(line[-1]))
    print("| B | N | C | R | variant | scan ms | sweep ms | share | LDS B/clk/CU | parent ms | speed-up | scan MB | parent MB |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['B']} | {r['N']} | {r['C']} | {r['R']} | {r['variant']} | {r['scan_ms']} | {r['sweep_ms']} | {r['share']} "
              f"| {r['lds_bytes_per_clk_cu']} | {r.get('parent_ms', r.get('parent_error', '-'))} | {r.get('speedup', '-')} "
              f"| {r['scan_extra_mb']} | {r.get('parent_extra_mb', '-')} |")


if __name__ == "__main__":
    main()
