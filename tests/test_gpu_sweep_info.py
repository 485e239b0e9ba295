"""info_out of bark_mll_batched_hip as a (B,) vector, and the isolation of a failing matrix from its neighbours, on every
schedule of the dense sweep (every row of sweep_ref.CASES: the one-launch kernels, fused plain with and without the ragged
split, pipelined, paired, split-K with and without look-ahead, candidates with cov_out, the identity right-hand side, a last
chunk on another schedule).

tests/info_ref.py places the first non-positive pivot of chosen matrices, through their `shift`, at the positions where the
index arithmetic changes — pivot 1, inside the first 16 x 16 sub-block, 17, 128, 129, a middle block step, the first and the
last pivot of the last block step — with a margin that no summation order can cross, plus one matrix with a negative diagonal
whose later pivots fail again (the first failure wins).  tests/test_sweep_info_reference_cpu.py checks that construction.

Per call: info_out equals the expected vector (the index for every bad matrix, 0 for every other one); every output of every
healthy matrix has the bits of the same call with the row's own healthy values (only a neighbour's data differs, and each
matrix's sums have a fixed order: any difference means a matrix read another matrix's state); the guard bands are intact and no
healthy output is NaN; the second route of the row reports the same vector.  What include/bark_hip.h says about a failed
matrix's own outputs is that they are unspecified: nothing is asserted about them.
(The wall time of every row is printed: run with -s to see it.)"""
import time

import numpy as np
import pytest

import info_ref as ir
import sweep_ref as sr

pytestmark = pytest.mark.gpu


def healthy_bits_equal(mixed, base, healthy):
    """{output: matrices whose bits differ} over the healthy matrices."""
    import torch

    idx = torch.as_tensor(healthy, device=mixed.mll.device, dtype=torch.int64)
    a, b = mixed.arrays(), base.arrays()
    assert a.keys() == b.keys()
    diff = {}
    for k in a:
        x, y = a[k][idx].view(torch.int64), b[k][idx].view(torch.int64)
        ne = (x != y).reshape(len(healthy), -1).any(dim=1)
        if bool(ne.any()):
            diff[k] = np.asarray(healthy)[ne.cpu().numpy()].tolist()
    return diff


def healthy_nans(out, healthy):
    import torch

    idx = torch.as_tensor(healthy, device=out.mll.device, dtype=torch.int64)
    return {k: int(torch.isnan(t[idx]).sum()) for k, t in out.arrays().items()}


def info_of(out, name):
    info = out.host("info")
    assert not (info == -3).any(), (name, "the device-side wait timed out again after the switch to event joins", info)
    return info


@pytest.mark.parametrize("name", list(sr.CASES))
def test_info_vector_and_isolation_on_every_schedule(name):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    t0 = time.perf_counter()
    case = sr.CASES[name]
    inp = sr.make_inputs(case)
    sr.check_cell(inp)
    plan = ir.plan_row(inp)
    assert plan.calls and not plan.unassigned, (name, plan.unassigned)
    t_host = time.perf_counter() - t0

    base = sr.run(inp)
    assert base.guards_intact(), name
    assert not info_of(base, name).any() and not any(base.nan_inside().values()), (name, base.host("info"))
    for k, call in enumerate(plan.calls):
        what = (name, k, [(h.b, h.cls, h.p) for h in call.bad])
        bad_inp = ir.with_call(inp, call)
        mixed = sr.run(bad_inp, shift=call.shift)
        info = info_of(mixed, name)
        assert np.array_equal(info, call.info), (what, info[call.info != info], call.info[call.info != info])
        healthy = call.healthy
        assert len(healthy) and mixed.guards_intact(), what
        assert not any(healthy_nans(mixed, healthy).values()), (what, healthy_nans(mixed, healthy))
        diff = healthy_bits_equal(mixed, base, healthy)
        assert not diff, (what, diff)
        if case.other is not None:  # the instrumented multi-launch sweep, or another chunk size: the same vector
            other = sr.run(bad_inp, shift=call.shift, timing=True) if case.other == "timing" else \
                sr.run(bad_inp, shift=call.shift, chunk=case.other)
            if case.other == "timing":
                assert other.timing.n_diag_launches >= -(-case.N // 128)
            assert np.array_equal(info_of(other, name), call.info), (what, "other route", other.host("info"))
            assert other.guards_intact(), what
            assert not any(healthy_nans(other, healthy).values()), what
            del other
        del mixed
    print("%s: %d calls, %d bad matrices, host %.1f s, total %.1f s" % (
        name, len(plan.calls), sum(len(c.bad) for c in plan.calls), t_host, time.perf_counter() - t0))


@pytest.mark.parametrize("name", ["two_n129", "splitk_n700_b20"])
def test_invalid_category_takes_precedence_over_a_bad_pivot(name):
    """A call that holds a matrix with a non-positive first pivot and also meets a NaN at a categorical split: every matrix
    reports -1 (one chunk per row here), none the pivot; bark_ctx_status then reads and clears the flag."""
    import dataclasses

    from bark_amd import _lib
    from oracle import oracle as orc

    case = sr.CASES[name]
    assert case.problem == "mixed" and case.bc == case.B
    inp = sr.make_inputs(case)
    d = sr.check_cell(inp)
    assert (d["schedule"] in ("one_block", "two_block", "multi_block")) == (name == "two_n129")
    b = case.B // 2
    hit = ir._try_class(inp, None, b, "noise", [1])
    assert hit is not None and hit.p == 1  # pivot 1 = scale (K[0, 0] - shift) + s2 with K[0, 0] = 1 whatever the walks give
    noise = inp.noise.copy()
    noise[b] = hit.noise
    pivot_only = sr.run(dataclasses.replace(inp, noise=noise))
    want = np.zeros(case.B, dtype=np.int32)
    want[b] = 1
    assert np.array_equal(pivot_only.host("info"), want), pivot_only.host("info")

    X = inp.X.copy()
    cat = np.flatnonzero(inp.ft == 0)
    assert len(cat)
    X[case.N // 2, cat] = np.nan
    with pytest.raises(ValueError):  # some walk of the batch evaluates a categorical split of that point
        orc.pass_through_forest(inp.F.reshape(-1, inp.F.shape[-1]), X, inp.ft)
    both = sr.run(dataclasses.replace(inp, noise=noise, X=X))
    with pytest.raises(ValueError):
        _lib.check_categorical_fault()  # bark_ctx_status reads the flag and clears it (before anything below can fail)
    _lib.check_categorical_fault()  # cleared: no later call sees it
    assert np.array_equal(both.host("info"), np.full(case.B, -1, dtype=np.int32)), both.host("info")
    assert both.guards_intact()
    clean = sr.run(inp)
    assert not clean.host("info").any()


# ------------------------------------------------------------------ the leaf-space entry points ----
_LEAF = []


def leaf_plan(which):
    if not _LEAF:
        _LEAF.extend(ir.leaf_plans())
    return _LEAF[which]


@pytest.mark.parametrize("entry", ["mll", "inverse", "draws"])
@pytest.mark.parametrize("which", [0, 1])
def test_leafspace_info_vector_and_isolation(which, entry):
    """bark_mll_leafspace_hip (with candidates), bark_kernel_inverse_leafspace_hip and bark_posterior_samples_hip: forests with
    a negative scale whose M = I + c Z'Z has its first non-positive pivot in the first 128 leaves, in the second block and past
    256 leaves, beside healthy forests, on the plain (3 block rows) and the split-K (5 block rows) layout of the R x R sweep."""
    import torch

    import leafspace_ref as lr

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    plan = leaf_plan(which)
    inp, B = plan.inp, plan.inp.case.B
    lr.check_shape(inp)
    assert not plan.missing

    def clean(out, info, rows):
        assert int(info[B]) == ir.LEAF_GUARD and all(bool(torch.isnan(t[B:]).all()) for t in out.values())
        assert not any(bool(torch.isnan(t[rows.to(t.device)]).any()) for t in out.values())

    everyone = torch.arange(B)
    base, base_info = ir.leaf_run(inp, entry, inp.scale)
    assert not base_info[:B].cpu().numpy().any()
    clean(base, base_info, everyone)
    mixed, info = ir.leaf_run(inp, entry, plan.scale)
    assert np.array_equal(info[:B].cpu().numpy(), plan.info), (info[:B].cpu().numpy(), plan.info)
    healthy = torch.as_tensor(plan.healthy)
    clean(mixed, info, healthy)
    for k in base:
        a, b = mixed[k][healthy.to(mixed[k].device)], base[k][healthy.to(base[k].device)]
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (entry, k)
