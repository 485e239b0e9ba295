"""One step of run_bark_sampler(method="leafspace"), split into its parts: N = 512 and 4096, 50 trees, 1 / 8 / 64 chains, d = 8.
   python tools/time_sampler.py [reps]
Parts: the propose launch and the commit launch (hipEvents around the library call), the read-back of the proposals, the host
pack of the sweep (validation, leaf counts, packing, step table, upload), the sweep (enqueue to the end of its read-back), the
noise / scale half (host draw + step_noise_scale) — wall clock around host parts that end in a synchronisation.  Median of `reps`
steps after two warm-up steps.  As the comparison, the same proposals drawn on the host by tests/proposals_ref.py (plain
Python: what a user without the kernel would run), wall clock.  Every shape is a child process of its own under
`timeout -k 10 300`; the parent never opens the GPU and stops at the first child that fails."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

REGION_LIMIT_S = 300
m = 50
PARTS = ("propose", "readback", "host pack", "sweep", "commit", "noise/scale")
HEADER = f"{'N':>6} {'chains':>6} " + " ".join(f"{p + ' ms':>14}" for p in PARTS) + f" {'step ms':>10} {'host propose ms':>16} {'accepted':>8}"

if len(sys.argv) < 4:  # parent
    reps = sys.argv[1] if len(sys.argv) > 1 else "7"
    print(HEADER, flush=True)
    for N in (512, 4096):
        for nc in (1, 8, 64):
            rc = subprocess.run(["timeout", "-k", "10", str(REGION_LIMIT_S), sys.executable, os.path.abspath(__file__), reps, str(N),
                                 str(nc)]).returncode
            if rc:
                raise SystemExit(f"N = {N}, {nc} chains: the child ended with status {rc}; nothing more is started")
    raise SystemExit(0)

import torch

import proposals_ref as pr
from bark_amd import synthetic as syn
from bark_amd.fitting import BARKTrainParams, bark_sampler, noise_scale_proposals as nsp, tree_proposals as tp

reps, N, nc = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
X, y, bounds, ft = syn.unit_cube_problem(N, 8, seed=N)
forests = syn.sample_prior_forests(nc, m, bounds, ft, seed=100)
params = BARKTrainParams(num_chains=nc)
run = bark_sampler._Run((forests, np.full(nc, 0.1), np.ones(nc)), (X, y), bounds, params, ft, 1, "leafspace", None)
ref_params = pr.Params(params.alpha, params.beta, tuple(params.proposal_weights), run.max_leaves)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def step(times, host_times, accepted):
    """bark_sampler._Run.step with a clock around every part."""
    s = run.step_index
    (new_d, lq_d, lu_d, _), t = events(lambda: tp.propose_trees_device(run.nodes_d, run.bounds_d, run.ft_d, run.cparams, run.seed, s))
    times["propose"].append(t)
    (new, lq, lu), t = wall(lambda: (tp.records_from_device(new_d), lq_d.cpu().numpy(), lu_d.cpu().numpy()))
    times["readback"].append(t)
    _, t = wall(lambda: pr.propose_forests(run.forest.view(pr.NODE), bounds, ft, ref_params, run.seed, s))
    host_times.append(t)
    prepared, t = wall(lambda: run.batch._prepare_sweep(run.forest, new, lq, lu, X, ft, run.batch.scale, m, None))
    times["host pack"].append(t)
    enqueue, accept, tidx, r_new, ftc = prepared
    acc, t = wall(lambda: (enqueue(), run.batch._finish_sweep(accept, tidx, r_new, ftc))[1])
    times["sweep"].append(t)
    _, t = events(lambda: tp.commit_trees_device(run.nodes_d, new_d, run.batch.last_accept_device, run.tidx_d))
    times["commit"].append(t)
    run.forest[acc] = new[acc]
    accepted.append(int(acc.sum()))

    def noise_scale():
        z, ns_lu = nsp.draw_normals(run.seed, s, nc)
        (new_noise, new_scale), ns_lq = nsp.get_noise_scale_proposal(run.noise, run.scale, params, z)
        took = run.batch.step_noise_scale(new_noise, new_scale, ns_lq, ns_lu)
        run.noise, run.scale = np.where(took, new_noise, run.noise), np.where(took, new_scale, run.scale)

    _, t = wall(noise_scale)
    times["noise/scale"].append(t)
    run.step_index += 1


for _ in range(2):
    step({p: [] for p in PARTS}, [], [])
times, host_times, accepted = {p: [] for p in PARTS}, [], []
for _ in range(reps):
    step(times, host_times, accepted)
med = {p: float(np.median(v)) for p, v in times.items()}
print(f"{N:>6} {nc:>6} " + " ".join(f"{med[p]:>14.3f}" for p in PARTS) + f" {sum(med.values()):>10.3f} {float(np.median(host_times)):>16.3f} "
      f"{int(np.median(accepted)):>8}", flush=True)
