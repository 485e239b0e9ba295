"""What a prediction from a fitted posterior costs ("Predicting from the fitted state"), at B = 64 forests of
m = 50 trees, N = 512, d = 10 and 2^18 points, the shape of the other tables of that section:

  moments            bark_leaf_posterior_predict_hip, moments only
  moments_q2         ... plus Q = 2 quantiles (0.025, 0.975), mu_b / var_b through the workspace slab
  moments_scores     ... moments plus the predictive scores of targets
  scan_lcb_mixture   bark_acquisition_scan_fitted_hip, kind lcb_mixture with values: the same per-point sums
  replaced_route     forest_predict(method="leafspace") + mixture_of_gaussians_as_normal on device tensors: the route replaced
                     (a Python call, so it includes the refit and the marshalling, as a user pays them)

Each of the first four rows times the library call alone (ctypes, arguments prepared outside) between two events on the stream;
the last a Python call between the same events.  Median of 5 after 2 warm-ups, in one child process under its own timeout.  Not a
pass/fail criterion.
Usage: PYTHONPATH=$PWD python tools/time_posterior_predict.py"""
import argparse
import json
import statistics
import subprocess
import sys

import numpy as np

WARMUP, REPS = 2, 5
B, M, N, C = 64, 50, 512, 1 << 18
PROBS = (0.025, 0.975)


def measure(call):
    import torch

    times = []
    for rep in range(WARMUP + REPS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        rc = call()
        stop.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        if rep >= WARMUP:
            times.append(start.elapsed_time(stop))
    return round(float(np.median(times)), 4)


def child():
    import torch

    import bark_amd.synthetic as syn
    from bark_amd import _lib as L
    from bark_amd.tree_kernels import fit_posterior, forest_predict, mixture_of_gaussians_as_normal

    X, y, bounds, ft = syn.mixed_problem(N, seed=1, d_cont=6)
    F = syn.sample_prior_forests(B, M, bounds, ft, seed=3)
    noise, scale = np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B)
    pts, yp = syn.mixed_problem(C, seed=2, d_cont=6)[:2]
    post = fit_posterior((F, noise, scale), (X, y), ft)
    pts_d = L.to_device(np.ascontiguousarray(pts, dtype=np.float64))
    yp_d = L.to_device(np.ascontiguousarray(yp, dtype=np.float64).reshape(-1))
    lib, R = L.lib(), post.R
    dev = dict(dtype=torch.float64, device="cuda")
    mom, quant, values = torch.empty((2, C), **dev), torch.empty((2, C), **dev), torch.empty(C, **dev)
    rows, mix = torch.empty((B, 2), **dev), torch.empty(2, **dev)
    best, idx = torch.empty((), **dev), torch.empty((), dtype=torch.int64, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    p_h = np.asarray(PROBS, dtype=np.float64)
    z_h = np.asarray([statistics.NormalDist().inv_cdf(p) for p in PROBS], dtype=np.float64)
    front = (L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise), L.ptr(post.scale), L.ptr(post.state),
             post.nbytes, L.ptr(pts_d), C)

    def predict(Q, scores):
        ws = L.workspace(int(lib.bark_leaf_posterior_predict_workspace_bytes(R, M, B, B, C, Q, 0, int(scores), 0)))
        y_ = L.ptr(yp_d if scores else None)
        return lambda: lib.bark_leaf_posterior_predict_hip(
            *front, None, 0, y_, L.ptr(p_h if Q else None), L.ptr(z_h if Q else None), Q, 0, L.ptr(mom), None,
            L.ptr(quant if Q else None), L.ptr(rows if scores else None), L.ptr(mix if scores else None), None, L.ptr(info), L.ptr(ws),
            ws.numel(), B, L.stream_ptr())

    row = {"B": B, "m": M, "N": N, "C": C, "R": R}
    row["moments_ms"] = measure(predict(0, False))
    row["moments_q2_ms"] = measure(predict(2, False))
    row["moments_scores_ms"] = measure(predict(0, True))
    ws = L.workspace(int(lib.bark_acquisition_scan_fitted_workspace_bytes(R, M, B, C, 0, 0)))
    row["scan_lcb_mixture_ms"] = measure(lambda: lib.bark_acquisition_scan_fitted_hip(
        *front, None, 0, None, 0, None, 0, 1.96, L.ACQ_LCB_MIXTURE, 0, L.ptr(values), L.ptr(best), L.ptr(idx), L.ptr(info), L.ptr(ws),
        ws.numel(), B, L.stream_ptr()))

    def replaced():
        mu, var = forest_predict((F, noise, scale), (X, y), pts_d, ft, method="leafspace")
        mixture_of_gaussians_as_normal(mu, var)
        return 0

    row["replaced_route_ms"] = measure(replaced)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child()
    else:
        out = subprocess.run([sys.executable, __file__, "--child"], check=True, timeout=600, capture_output=True, text=True)
        print(out.stdout.strip().splitlines()[-1], flush=True)
