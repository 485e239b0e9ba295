"""What the importance weights of a fitted posterior cost ("Weighted forest samples"):

  scan      bark_acquisition_scan_fitted_hip (equal weights) beside bark_acquisition_scan_fitted_weighted_hip with all weights
            positive and with every other weight zero, kind lcb_mean, at B = 64 forests of m = 50 trees, N = 512, d = 10 and
            2^18 candidates, the shape of the other tables of that section
  kernels   bark_forest_weights_hip at B = 64 and 4096; bark_leaf_posterior_gather_hip of all 64 forests of that state
            beside torch indexing of the same three views

Each row times the library call alone (ctypes, arguments prepared outside) between two events on the stream.  Median of 5
after 2 warm-ups, one process per build and row group.  With --parent-lib the equal-weight scan is also timed on another build
of the library (the parent commit's libbarkhip.so), the two builds alternating for --rounds rounds in one session; the spread
of a build is the range of its medians over the rounds.  Not a pass/fail criterion.
Usage: PYTHONPATH=$PWD python tools/time_weighted_scan.py [--parent-lib PATH] [--rounds 3]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

WARMUP, REPS = 2, 5
B, M, N, C = 64, 50, 512, 1 << 18
NEW = ("bark_acquisition_scan_fitted_weighted_hip", "bark_acquisition_scan_fitted_weighted_workspace_bytes",
       "bark_forest_weights_hip", "bark_leaf_posterior_gather_hip")


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


def library():
    """the binding, without the entry points an older build of the library does not have -> (_lib, they are there)"""
    from bark_amd import _lib as L

    handle = ctypes.CDLL(L.LIB_PATH)
    have = all(hasattr(handle, name) for name in NEW)
    if not have:
        for name in NEW:
            L.SIGNATURES.pop(name, None)
    return L, have


def fitted(L):
    import bark_amd.synthetic as syn
    from bark_amd.tree_kernels import fit_posterior

    X, y, bounds, ft = syn.mixed_problem(N, seed=1, d_cont=6)
    F = syn.sample_prior_forests(B, M, bounds, ft, seed=3)
    noise, scale = np.linspace(0.05, 0.3, B), np.linspace(0.7, 1.4, B)
    cand = syn.mixed_problem(C, seed=2, d_cont=6)[0]
    return fit_posterior((F, noise, scale), (X, y), ft), L.to_device(np.ascontiguousarray(cand, dtype=np.float64))


def child_scan(build):
    """build: "this" or "parent", the role `run` gave the library of this process"""
    import torch

    L, have = library()
    post, cand = fitted(L)
    lib = L.lib()
    best = torch.empty((), dtype=torch.float64, device="cuda")
    idx = torch.empty((), dtype=torch.int64, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = L.workspace(int(lib.bark_acquisition_scan_fitted_workspace_bytes(post.R, M, B, C, 0, 0)))
    front = (L.ctx(), L.ptr(post.packed.packed), post.packed.info_ref, post.d, L.ptr(post.noise), L.ptr(post.scale), L.ptr(post.state),
             post.nbytes, L.ptr(cand), C, None, 0, None, 0, None, 0, 1.96, L.ACQ_LCB_MEAN, 0)
    back = (None, L.ptr(best), L.ptr(idx), L.ptr(info), L.ptr(ws), ws.numel(), B, L.stream_ptr())
    row = {"build": build, "B": B, "m": M, "N": N, "C": C, "R": post.R,
           "unweighted_ms": measure(lambda: lib.bark_acquisition_scan_fitted_hip(*front, *back))}
    if have:
        rng = np.random.default_rng(0)
        w = rng.uniform(0.5, 1.5, size=B)
        half = w.copy()
        half[1::2] = 0.0
        for name, v in (("weighted_ms", w), ("half_zero_ms", half)):
            wd = L.to_device(v / v.sum())
            row[name] = measure(lambda: lib.bark_acquisition_scan_fitted_weighted_hip(*front, L.ptr(wd), *back))
    print(json.dumps(row), flush=True)


def child_kernels():
    import torch

    L, have = library()
    assert have, "this build of the library has no weights"
    lib = L.lib()
    row = {}
    for b in (64, 4096):
        rng = np.random.default_rng(b)
        lw, inc = L.to_device(np.log(rng.dirichlet(np.ones(b)))), L.to_device(rng.uniform(-30.0, 0.0, size=b))
        out, w, stats = torch.empty_like(lw), torch.empty_like(lw), torch.empty(3, dtype=torch.float64, device="cuda")
        row[f"weights_B{b}_ms"] = measure(lambda: lib.bark_forest_weights_hip(L.ptr(lw), L.ptr(inc), None, b, L.ptr(out), L.ptr(w),
                                                                             L.ptr(stats), L.stream_ptr()))
    post, _ = fitted(L)
    R = post.R
    index = torch.from_numpy(np.random.default_rng(1).integers(0, B, size=B)).cuda()
    state = torch.empty_like(post.state)
    row["R"] = R
    row["gather_ms"] = measure(lambda: lib.bark_leaf_posterior_gather_hip(L.ptr(post.state), B, R, L.ptr(index), B, L.ptr(state),
                                                                         L.stream_ptr()))
    a, b2 = (8 * B * R * R + 255) & ~255, (8 * B * R + 255) & ~255
    Minv = post.state[:8 * B * R * R].view(torch.float64).view(B, R, R)
    wv = post.state[a:a + 8 * B * R].view(torch.float64).view(B, R)
    iv = post.state[a + b2:a + b2 + 4 * B].view(torch.int32)

    def by_torch():
        Minv[index], wv[index], iv[index]
        return 0

    row["torch_index_ms"] = measure(by_torch)
    print(json.dumps(row), flush=True)


def run(mode, lib_path=None):
    env = dict(os.environ)
    if lib_path:
        env["BARK_LIB_PATH"] = lib_path
    out = subprocess.run([sys.executable, __file__, "--child", mode, "--build", "parent" if lib_path else "this"], check=True,
                         timeout=600, env=env, capture_output=True, text=True)
    row = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--build", default="this")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        child_scan(a.build) if a.child == "scan" else child_kernels()
    else:  # a fresh process per build and round: no row inherits another's allocator or clock state
        rows = {"this": [], "parent": []}
        for _ in range(a.rounds):
            if a.parent_lib:
                rows["parent"].append(run("scan", a.parent_lib))
            rows["this"].append(run("scan"))
        run("kernels")
        for name, got in rows.items():
            if got:
                ms = [r["unweighted_ms"] for r in got]
                print(json.dumps({"build": name, "unweighted_ms_median": float(np.median(ms)), "spread_ms": round(max(ms) - min(ms), 4)}))
