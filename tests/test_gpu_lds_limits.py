"""Every translation unit of libbarkhip.so raises the dynamic-LDS limit of its own kernels from its own launch path
(common.h: raise_lds_limits).  What can go wrong is a kernel missing from its unit's table, or a table raised after the launch
that needs it — and that shows only when the kernel is the first thing a process launches: in the rest of the suite an earlier
test has usually raised the limits already.  So every case here runs in a fresh child process whose one kernel-launching
library call is the entry point under test (packing, plan queries, the context and the workspace sizes are host code), and
compares with the host reference and the bars of that entry point's own tests.

The children run strictly one after another, each under its own time limit; the parent never touches the GPU.  A child that
exits non-zero fails its case, and no further child is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 180  # seconds: the import of torch, the host reference and one library call
LDS_DEFAULT = 64 * 1024  # dynamic LDS a kernel may use without a raised limit

_child_failed = []


def child(call: str):
    """`call` (an expression on this module, imported as t) in a fresh interpreter."""
    if _child_failed:
        pytest.fail(f"not started: the child of {_child_failed[0]} failed")
    code = f"import sys; sys.path[:0] = [{TESTS!r}, {ROOT!r}]; import test_gpu_lds_limits as t; t.{call}"
    flags = ["-s"] if sys.flags.no_user_site else []
    done = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(done.stdout, end="")
    if done.returncode != 0:
        _child_failed.append(call)
        pytest.fail(f"child {call} exited with {done.returncode}\n{done.stdout}\n{done.stderr}")


def used(got, want, rtol, atol):
    return float((np.abs(np.asarray(got) - want) / (atol + rtol * np.abs(want))).max())


def report(name, worst):
    print(name, "fraction of each bar used:", {k: "%.2g" % v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


# ---------------------------------------------------------------------------------------------- lowrank.hip ----
# skinny_kernel<RT, VEC>: 2 (128 KL + 2) r 8 bytes of LDS, past 64 KiB from r = 32 with KL = 1, so the bound RT = 32 at its
# top rank and RT = 64; VEC is N even.  symmetric = 0 with K_out: skinny_kernel forms K U (r > 16: no column form).
# r = 31 needs no raised limit: the control.
LOWRANK_SHAPES = [(64, 31), (64, 32), (65, 32), (64, 33), (65, 64)]


def child_lowrank(N, r):
    import lowrank_ref as lr
    import torch

    from bark_amd import _lib

    rng = np.random.default_rng([N, r])  # lowrank_ref.make_inputs' recipe at a shape of our own
    K = np.eye(N) + (0.25 / np.sqrt(N)) * rng.standard_normal((N, N))
    U = (0.6 / np.sqrt(N)) * rng.standard_normal((N, r))
    assert np.linalg.cond(np.eye(r) + U.T @ K @ U) <= lr.COND_MAX
    want, want_lad = lr.update(K, U, False)
    lib = _lib.lib()
    nbytes = int(lib.bark_lowrank_workspace_bytes(N, r))
    Kd, Ud = _lib.to_device(K), _lib.to_device(U)
    out = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda")
    lad = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.bark_lowrank_update_hip(_lib.ptr(Kd), N, _lib.ptr(Ud), r, 0, 0, _lib.ptr(out), _lib.ptr(lad), _lib.ptr(ws), nbytes,
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    report(f"lowrank N={N} r={r}", {"K_out": lr.used(out.cpu().numpy(), want, lr.MAT_RTOL, lr.MAT_ATOL),
                                    "logabsdet": lr.used(float(lad[0]), want_lad, lr.SCALAR_RTOL, lr.SCALAR_ATOL)})


@pytest.mark.parametrize("N,r", LOWRANK_SHAPES)
def test_lowrank_update_first_in_its_process(N, r):
    child(f"child_lowrank({N}, {r})")


# --------------------------------------------------------------------------------------- sweep_resident.hip ----
SR_LEAVES = (((2, 3), (3, 4)), ((3, 4), (2, 3)))  # two chains, two steps: (leaves of the old tree, of the new tree)


def smallest_resident_N(variant):
    """The smallest N at which the one-launch sweep takes `variant` with more than 64 KiB of LDS, from the plan query."""
    import lowrank_ref as lr

    from bark_amd.fitting import sweep_plan

    for N in range(1, 513):
        plan = sweep_plan(N, 16, lr.CHAIN_D, nc=2)
        if plan["variant"] == variant and plan["lds_bytes"] > LDS_DEFAULT:
            return N
    raise AssertionError(f"no N takes variant {variant} with more than 64 KiB")


def child_sweep_resident(N, variant):
    import ctypes

    import lowrank_ref as lr
    import sweep_resident_ref as sr
    import torch

    from bark_amd import _lib
    from bark_amd.fitting import _chains, sweep_plan
    from bark_amd.forest import _feat_types, _points
    from oracle import oracle as orc

    nc, steps = 2, 2
    assert sweep_plan(N, 16, lr.CHAIN_D, nc=nc)["variant"] == variant
    sr.CASES["lds_limits"] = sr.Case(N, nc, steps, SR_LEAVES, 0, "first launch of a process")
    inp = sr.make_inputs("lds_limits")
    want = sr.host_sweep(inp)
    assert want.margin.min() >= sr.MARGIN, want.margin  # a condition on the inputs: the masks must be identical
    y = inp.y.reshape(-1)
    K_inv, state = [], []
    for b in range(nc):  # host_sweep's starting state
        K = inp.scale[b] * orc.forest_gram_matrix(inp.cur[b], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[b]) * np.eye(N)
        Ki = np.linalg.inv(K)
        Ki = 0.5 * (Ki + Ki.T)
        K_inv.append(Ki)
        state.append([y @ Ki @ y, np.linalg.slogdet(K)[1]])
    lib = _lib.lib()
    ft = _feat_types(inp.ft)
    Xd, _ = _points(inp.X, ft.shape[0])
    infos, offsets, _, host = _chains.pack_steps_host([np.stack([inp.cur[:, t], inp.prop[:, t]], axis=1) for t in range(steps)], ft)
    r_old = np.ascontiguousarray(_chains.leaf_counts(inp.cur, ft).T)
    r_max = max(int(i.max_bits) for i in infos)
    packed, lq_d, lu_d, accept = _chains.upload_sweep(host, _chains.steps_major(inp.log_q, nc, steps),
                                                      _chains.steps_major(inp.log_u, nc, steps))
    table = np.empty(int(lib.bark_tree_sweep_resident_table_bytes(steps, nc)) // 8, dtype=np.int64)
    _lib.check(lib.bark_tree_sweep_resident_table(_lib.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), _lib.ptr(r_old), steps, nc,
                                                  _lib.ptr(table)))
    Kd, yd, state_d = _lib.to_device(np.stack(K_inv)), _lib.to_device(y), _lib.to_device(np.array(state))
    table_d, s_d = _lib.to_device(table), _lib.to_device(np.ascontiguousarray(np.sqrt(inp.scale / steps)))
    ws = torch.empty(int(lib.bark_tree_sweep_resident_workspace_bytes(N, r_max, nc)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.bark_tree_sweep_resident_hip(_lib.ctx(), _lib.ptr(Kd), N, nc, steps, _lib.ptr(packed), _lib.ptr(table_d),
                                                _lib.ptr(Xd), Xd.shape[1], _lib.ptr(s_d), _lib.ptr(yd), _lib.ptr(lq_d), _lib.ptr(lu_d),
                                                _lib.ptr(state_d), _lib.ptr(accept), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    acc, quad, logdet = _chains.read_decisions(accept, state_d)
    assert np.array_equal(acc.T, want.mask), (acc.T, want.mask)
    report(f"sweep_resident N={N} variant {variant}", {"quad": lr.used(quad, want.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
                                                       "logdet": lr.used(logdet, want.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL)})


@pytest.mark.parametrize("variant", [1, 2])
def test_sweep_resident_first_in_its_process(variant):
    child(f"child_sweep_resident({smallest_resident_N(variant)}, {variant})")


# ---------------------------------------------------------------------------------------------- acquire.hip ----
def child_acq_scan_lds():
    import acq_ref as ar

    from bark_amd.optimizer import acquisition_scan

    name = "m64_r128"
    inp = ar.make_inputs(name)
    want, at = ar.precheck(name)["lcb_mean"]
    value, index, acq = acquisition_scan(inp.model, inp.data, inp.cand, inp.ft, kappa=inp.case.kappa, kind="lcb_mean",
                                         return_values=True, variant="lds")
    report(f"acquisition scan {name} (LDS variant)", {"acq": used(acq, want, ar.RTOL, ar.ATOL)})
    assert index == at and value == acq[at]


def test_acquisition_scan_lds_variant_first_in_its_process():
    child("child_acq_scan_lds()")


# acq_condition_kernel: (R + 1) 8 + 264 bytes, past 64 KiB from R = 8159 of the 8192 leaves the leaf-space path admits.  63
# complete trees of depth 7 (8064 leaves) and one caterpillar tree of 95.
PENDING_R = 8159


def child_acq_scan_pending():
    import acq_pending_ref as pr
    import acq_ref as ar
    import lowrank_ref as lr

    from bark_amd import synthetic
    from bark_amd.optimizer import acquisition_scan
    from bark_amd.tree_kernels import posterior_sample_dim

    case = ar.Case("pend_r8159", ("leaves", 64, PENDING_R), N=64, B=1, C=64, seed=21)
    X, y, _, ft = ar.problem(case.N, 100 + case.seed)
    cand = ar.problem(case.C, 200 + case.seed)[0]
    pending = ar.problem(2, 300 + case.seed)[0][:1]
    rng = np.random.default_rng(case.seed)
    F = np.concatenate([synthetic.full_binary_forest(63, ar.D_CONT, 7, rng, node_limit=ar.NODE_LIMIT),
                        lr.caterpillar_tree(PENDING_R - 63 * 128, 0, node_limit=ar.NODE_LIMIT)[None]])[None]
    R = posterior_sample_dim(F, ft)
    assert R == PENDING_R and (R + 1) * 8 + 66 * 4 > LDS_DEFAULT >= R * 8 + 66 * 4
    inp = ar.Inputs(case, F, X, y, ft, cand, np.array([0.2]), np.array([1.1]))
    mu, var = pr.dense(inp, pending)
    want = ar.acquisition(mu, var, case.kappa, "lcb_mean")
    value, index, acq = acquisition_scan(inp.model, inp.data, cand, ft, kappa=case.kappa, kind="lcb_mean", return_values=True,
                                         pending=pending)
    report(f"pending-points scan R={R}", {"acq": used(acq, want, pr.RTOL, pr.ATOL)})
    assert index == int(np.argmin(acq)) and value == acq[index]


def test_acquisition_scan_pending_first_in_its_process():
    child("child_acq_scan_pending()")


# -------------------------------------------------------------------------------------------- leafspace.hip ----
def child_leafspace_inverse():
    import leafspace_ref as ls

    import bark_amd.fitting as fit

    case = min(ls.CASES.values(), key=lambda c: (c.shape[0], c.N * c.B))  # the smallest case of the table: null50
    inp = ls.make_inputs(case)
    K_inv, K_inv_y, logdet = fit.batched_kernel_inverse(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, no_null=False,
                                                        method="leafspace", chunk=case.bc)
    worst = {}
    for b in range(case.B):  # the bars of tests/test_gpu_leafspace.py::test_inverse
        ref = ls.reference(inp, b)
        Ki, Kiy = ref.inverse()
        worst["K_inv"] = max(worst.get("K_inv", 0.0), used(K_inv[b], Ki, 1e-8, 1e-9))
        worst["K_inv_y"] = max(worst.get("K_inv_y", 0.0), used(K_inv_y[b], Kiy, 1e-8, 1e-9))
        worst["logdet"] = max(worst.get("logdet", 0.0), used(logdet[b], ref.logdet(), 1e-10, 0.0))
    report(f"leaf-space inverse {case.name}", worst)


def test_leafspace_inverse_first_in_its_process():
    child("child_leafspace_inverse()")


# ------------------------------------------------------------------------------------------------- chol.hip ----
def child_mll(N):
    import bark_amd.fitting as fit
    from bark_amd import synthetic
    from oracle import oracle as orc

    X, y, bounds, ft = synthetic.mixed_problem(N, seed=N)
    F = synthetic.sample_prior_forests(1, 50, bounds, ft, seed=N)
    noise, scale = np.array([0.1]), np.array([1.2])
    got = fit.batched_mll(F, noise, scale, X, y, ft, include_scale=True, include_2pi=True)
    want = orc.batched_mll(F, noise, scale, X, y, ft, include_scale=True, include_2pi=True)
    report(f"bark_mll_batched_hip N={N} B=1", {"mll": used(got, want, 1e-9, 1e-8)})  # the MLL bar (tests/test_gpu_parity.py)


@pytest.mark.parametrize("N", [129, 300])  # one matrix of two block rows (two_block_kernel) and of three (diag / row / solve)
def test_mll_batched_first_in_its_process(N):
    child(f"child_mll({N})")
