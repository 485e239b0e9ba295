"""What taking in P new observations costs through LeafPosterior.observe, beside what a user did before it existed: a refit
(fit_posterior) on the N + P points ("Conditioning on observed and fantasised values").

  observe   bark_leaf_posterior_observe_hip on a copy of the state fitted to the first N points: one launch pair per chunk
  refit     bark_leaf_posterior_fit_hip on all N + P points, into a fresh state

at B = 64 forests of m = 50 trees, d = 10, for N = 512 and 4096 and P = 1 and 16.  Each row times the library call alone
(ctypes, arguments prepared outside) between two events on the stream; the packing of the forests, the copy of the state and
every read-back are outside.  Median of 5 after 2 warm-ups, one process per shape.  Not a pass/fail criterion.
Usage: PYTHONPATH=$PWD python tools/time_observe.py"""
import json
import subprocess
import sys

import numpy as np

WARMUP, REPS = 2, 5
B, M = 64, 50
SHAPES = [(512, 1), (512, 16), (4096, 1), (4096, 16)]


def measure(prepare, call):
    import torch

    times = []
    for rep in range(WARMUP + REPS):
        args = prepare()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        rc = call(args)
        stop.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        if rep >= WARMUP:
            times.append(start.elapsed_time(stop))
    return float(np.median(times))


def child(N, P):
    import torch

    import bark_amd.synthetic as syn
    from bark_amd import _lib as L
    from bark_amd.fitting.mll import _leaf_inputs
    from bark_amd.tree_kernels import fit_posterior

    X, y, bounds, ft = syn.mixed_problem(N + P, seed=1, d_cont=6)
    F = syn.sample_prior_forests(B, M, bounds, ft, seed=3)
    noise, scale = np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B)
    post = fit_posterior((F, noise, scale), (X[:N], y[:N]), ft)
    lib, R = L.lib(), post.R
    pts, vals = L.to_device(X[N:]), L.to_device(np.asarray(y[N:], dtype=np.float64).reshape(-1))
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    head = lambda p: (L.ctx(), L.ptr(p.packed.packed), p.packed.info_ref)  # noqa: E731

    ws = L.workspace(int(lib.bark_leaf_posterior_observe_workspace_bytes(R, M, B, P)))
    ms_observe = measure(
        lambda: post._copy(),
        lambda c: lib.bark_leaf_posterior_observe_hip(*head(c), c.d, L.ptr(c.noise), L.ptr(c.scale), L.ptr(pts), P, L.ptr(vals), 0,
                                                      L.OBSERVE_VALUES, None, 0, 0, L.ptr(c.state), c.nbytes, None, None, L.ptr(info),
                                                      L.ptr(ws), ws.numel(), B, L.stream_ptr()))
    q = _leaf_inputs(F, noise, scale, X, y, ft)
    ws = L.workspace(int(lib.bark_leaf_posterior_fit_workspace_bytes(N + P, R, M, B)))
    ms_refit = measure(
        lambda: torch.empty(post.nbytes, dtype=torch.uint8, device="cuda"),
        lambda st: lib.bark_leaf_posterior_fit_hip(L.ctx(), L.ptr(q.pf.packed), q.pf.info_ref, L.ptr(q.Xd), N + P, q.d, L.ptr(q.yd),
                                                   L.ptr(q.noise_d), L.ptr(q.scale_d), L.ptr(st), post.nbytes, L.ptr(info), L.ptr(ws),
                                                   ws.numel(), B, L.stream_ptr()))
    assert q.R == R and not info.any()
    print(json.dumps({"B": B, "m": M, "N": N, "P": P, "R": R, "observe_ms": round(ms_observe, 3), "refit_ms": round(ms_refit, 3)}),
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3:
        child(int(sys.argv[1]), int(sys.argv[2]))
    else:
        for N, P in SHAPES:  # a fresh process per shape: no shape inherits another's allocator or clock state
            subprocess.run([sys.executable, __file__, str(N), str(P)], check=True, timeout=300)
