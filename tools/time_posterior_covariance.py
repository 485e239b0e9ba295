"""Device time of the joint covariance from a fitted posterior (LeafPosterior.covariance, bark_leaf_posterior_covariance_hip) at
m = 50 prior trees beside the same blocks composed in torch on the device: per forest Z1 M^-1 Z2' in fp64 with dense one-hot
matrices Z (C, R), one torch.matmul pair per forest, scaled by scale_b / m.  hipEvent medians of 5 after 2 warm-ups on
device-resident points, one process per row.

  blocks ms   the library call with per_forest=True: the walks, the (B, C1, C2) blocks, predict's means and the mixture
  mixture ms  the library call for the mixture alone (the blocks of a chunk pass through the workspace)
  torch ms    the B products alone.  The one-hot matrices and M^-1 are made before the clock starts and the mixture is not
              formed, so the comparison favours torch.  The columns of the state's M^-1 are numbered by the library's leaf
              codes, which no public call returns; the yardstick numbers the leaves itself (np.unique per tree) and inverts
              I + c Z'Z of the training points in torch — the same matrix up to that numbering, and the same products
  max_diff    largest |library - torch| over the blocks
Usage: PYTHONPATH=$PWD python tools/time_posterior_covariance.py [--rows B,N,C ...]"""
import argparse
import json
import subprocess
import sys

ROWS = [(64, 512, 256), (64, 512, 2048)]
M_TREES = 50
WARMUP, REPS = 2, 5


def one(B, N, C):
    import numpy as np
    import torch

    import bark_amd.synthetic as syn
    from bark_amd.forest import _leaf_indices, _points
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

    X, y, bounds, ft = syn.mixed_problem(N, seed=1)
    x1, _, _, _ = syn.mixed_problem(C, seed=2)
    x2, _, _, _ = syn.mixed_problem(C, seed=3)
    F = syn.sample_prior_forests(B, M_TREES, bounds, ft, seed=4)
    noise, scale = np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B)
    post = fit_posterior((F, noise, scale), (X, y), ft)
    x1d, x2d = (torch.as_tensor(v, device="cuda") for v in (x1, x2))
    row = {"B": B, "N": N, "C": C, "m": M_TREES, "R": post.R}
    blocks_ms, (_, blocks) = measure(lambda: post.covariance(x1d, x2d, per_forest=True))
    mixture_ms, _ = measure(lambda: post.covariance(x1d, x2d))
    row.update(blocks_ms=round(blocks_ms, 3), mixture_ms=round(mixture_ms, 3))

    # the yardstick's operands: leaf node indices of all points, columns numbered per tree in ascending node order
    ids = _leaf_indices(post.packed, _points(np.vstack([X, x1, x2]), post.d)[0]).cpu().numpy().astype(np.int64)  # (B, N + 2C, m)
    Z1, Z2, Minv = [], [], []
    for b in range(B):
        cols, off = [], 0
        for t in range(M_TREES):
            u, inv = np.unique(ids[b, :, t], return_inverse=True)
            cols.append(off + inv.reshape(-1))
            off += len(u)
        a = torch.as_tensor(np.stack(cols, axis=1), device="cuda")
        Z = torch.zeros((a.shape[0], post.R), dtype=torch.float64, device="cuda")
        Z.scatter_(1, a, 1.0)
        ZX = Z[:N]
        c = scale[b] / (M_TREES * (1e-6 + noise[b]))
        Minv.append(torch.linalg.inv(torch.eye(post.R, dtype=torch.float64, device="cuda") + c * (ZX.T @ ZX)))
        Z1.append(Z[N:N + C].contiguous())
        Z2.append(Z[N + C:].contiguous())
    Z1, Z2, Minv = torch.stack(Z1), torch.stack(Z2), torch.stack(Minv)
    sm = torch.as_tensor(scale / M_TREES, device="cuda").reshape(-1, 1, 1)
    try:
        torch_ms, ref = measure(lambda: sm * torch.matmul(torch.matmul(Z1, Minv), Z2.transpose(1, 2)))
        row.update(torch_ms=round(torch_ms, 3), speedup=round(torch_ms / blocks_ms, 2), max_diff=float((ref - blocks).abs().max().item()))
    except (ValueError, MemoryError, RuntimeError) as exc:
        row["torch_error"] = f"{type(exc).__name__}: {exc}"[:200]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=None, help="B,N,C")
    ap.add_argument("--one", default=None, help="B,N,C: measure this row in this process")
    args = ap.parse_args()
    if args.one:
        one(*(int(v) for v in args.one.split(",")))
        return
    rows_in = [tuple(r.split(",")) for r in args.rows] if args.rows else ROWS
    rows = []
    for r in rows_in:  # a fresh process per row; this one never opens the device
        spec = ",".join(map(str, r))
        try:
            p = subprocess.run([sys.executable, __file__, "--one", spec], capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            print(f"row {spec}: no result after 300 s", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode or not line:
            print(f"row {spec}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            break  # nothing more is started on the device after a failure
        print(line[-1], flush=True)
        rows.append(json.loads(line[-1]))
    print("| B | N | C1 = C2 | R | blocks ms | mixture ms | torch ms | speed-up | max diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['B']} | {r['N']} | {r['C']} | {r['R']} | {r['blocks_ms']} | {r['mixture_ms']} "
              f"| {r.get('torch_ms', r.get('torch_error', '-'))} | {r.get('speedup', '-')} | {r.get('max_diff', '-')} |")


if __name__ == "__main__":
    main()
