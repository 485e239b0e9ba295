"""Acquisition scan (bark_acquisition_scan_hip) against the host reference of tests/acq_ref.py (the oracle's dense
`forest_predict`, reduced with the reference's formulas), over the case table of acq_ref.CASES: N = 64 and 257, mixed
categorical / integer / continuous inputs, 1, 3 and 5 forests (three chunks), 1 ... 64 trees, candidate counts around the
scan's 256-candidate workgroups, leaf counts on both sides of a code-word edge and of the LDS limit.

Bars: values to the posterior bar of DESIGN.md section 2 (rtol 1e-9, atol 1e-8), indices equal (tests/test_acquisition_cpu.py
establishes on the host that every case's minimum is separated by 1e-6).  The summation order is part of the contract, so
chunking, a repeated call and the two kernel variants are compared bit for bit."""
import numpy as np
import pytest

import acq_ref as ar

from conftest import load_golden

pytestmark = pytest.mark.gpu
NAMES = list(ar.CASES)


@pytest.fixture(scope="module")
def scan():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd.optimizer import acquisition_scan

    return acquisition_scan


def run(scan, name, kind="lcb_mean", **kw):
    inp = ar.make_inputs(name)
    kw.setdefault("chunk", inp.case.chunk)
    return scan(inp.model, inp.data, inp.cand, inp.ft, kappa=inp.case.kappa, kind=kind, return_values=True, **kw)


def bar_used(got, want):
    return float((np.abs(got - want) / (ar.ATOL + ar.RTOL * np.abs(want))).max())


@pytest.fixture(scope="module")
def g6():
    from oracle import oracle as orc

    g = load_golden("g6_predict")
    forest = orc.nodes_from_raw(g["forest"]).reshape(-1, 50, 100)
    return g, (forest, g["noise"].reshape(-1), g["scale"].reshape(-1))


@pytest.mark.parametrize("kind", ar.KINDS)
def test_g6(scan, g6, kind):
    """the reference's own posterior: the values derived from the golden mu / var, minimum at candidate 26"""
    g, model = g6
    want = ar.acquisition(g["mu"], g["var"], 1.96, kind)
    value, index, acq = scan(model, (g["X"], g["y"]), g["cand"], g["feat_types"], kind=kind, return_values=True)
    used = bar_used(acq, want)
    print(f"g6 {kind}: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    assert index == 26 and value == acq[26]


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_case_against_reference(scan, name, kind):
    want, at = ar.precheck(name)[kind]
    value, index, acq = run(scan, name, kind)
    assert acq.shape == (ar.CASES[name].C,) and acq.dtype == np.float64
    used = bar_used(acq, want)
    print(f"{name} {kind}: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    assert index == at
    assert value == acq[at]


@pytest.mark.parametrize("name", ["m13_lds_limit", "m13_past_lds", "m64_r128", "m64_r256"])
def test_case_takes_the_variant_it_claims(name):
    from bark_amd.optimizer import acquisition_plan
    from bark_amd.tree_kernels import posterior_sample_dim

    inp = ar.make_inputs(name)
    want = "lds" if name in ("m13_lds_limit", "m64_r128") else "global"
    assert acquisition_plan(posterior_sample_dim(inp.F, inp.ft), inp.case.m)["variant"] == want


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("name", ["prior_n257_chunks", "prior_n64", "m64_r256"])
def test_chunking_and_repeats_are_bit_identical(scan, name, kind):
    base = run(scan, name, kind)
    for other in (run(scan, name, kind), run(scan, name, kind, chunk=1), run(scan, name, kind, chunk=ar.CASES[name].B)):
        assert other[0] == base[0] and other[1] == base[1] and np.array_equal(other[2], base[2])


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("name", ["prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit", "m64_r128"])
def test_lds_and_global_variants_are_bit_identical(scan, name, kind):
    a = run(scan, name, kind, variant="lds")
    b = run(scan, name, kind, variant="global")
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    c = run(scan, name, kind)  # auto
    assert np.array_equal(a[2], c[2])


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("name", ["prior_n64", "m1_r64", "m13_past_lds"])
def test_best_without_the_vector(scan, name, kind):
    inp = ar.make_inputs(name)
    value, index, acq = run(scan, name, kind)
    v2, i2 = scan(inp.model, inp.data, inp.cand, inp.ft, kappa=inp.case.kappa, kind=kind, chunk=inp.case.chunk)
    assert (v2, i2) == (value, index)
    assert index == int(np.argmin(acq)) and value == acq.min()


@pytest.mark.parametrize("kind", ar.KINDS)
def test_candidate_slabs(scan, kind):
    """C = 65 537: the scan walks the candidates in two slabs (65 536 and 1) under each of two chunks of forests.  A
    candidate's value does not depend on the other candidates, so each part equals a scan of that part alone, bit for bit."""
    inp = ar.make_inputs(ar.SLAB_CASE)
    C, slab = inp.case.C, 1 << 16
    kw = dict(kappa=inp.case.kappa, kind=kind, return_values=True, chunk=inp.case.chunk)
    value, index, acq = scan(inp.model, inp.data, inp.cand, inp.ft, **kw)
    assert acq.shape == (C,) and acq.dtype == np.float64
    used = bar_used(acq, ar.reference(ar.SLAB_CASE, kind))
    print(f"{inp.case.name} {kind}: fraction of the bar used {used:.3g}")
    assert used <= 1.0
    assert np.array_equal(acq[:slab], scan(inp.model, inp.data, inp.cand[:slab], inp.ft, **kw)[2])
    assert np.array_equal(acq[slab:], scan(inp.model, inp.data, inp.cand[slab:], inp.ft, **kw)[2])
    assert index == int(np.argmin(acq)) and value == acq[index]


def test_ties_go_to_the_lowest_index(scan):
    """exact duplicate rows: the winner of prior_n64 repeated in front of, inside and behind its own workgroup"""
    inp = ar.make_inputs("prior_n64")
    _, at = ar.precheck("prior_n64")["lcb_mean"]
    cand = inp.cand.copy()
    spots = [s for s in (3, ar.TILE + 5, 2 * ar.TILE, len(cand) - 1) if s != at]
    first = spots[0]
    for s in spots:
        cand[s] = inp.cand[at]
    value, index, acq = scan(inp.model, inp.data, cand, inp.ft, return_values=True)
    assert index == min(first, at)
    assert all(acq[s] == value for s in spots + [at])
    # and with the duplicates only behind the original
    cand = inp.cand.copy()
    later = [s for s in range(at + 1, len(cand), 97)]
    assert later
    for s in later:
        cand[s] = inp.cand[at]
    assert scan(inp.model, inp.data, cand, inp.ft)[1] == at


@pytest.mark.parametrize("name", ["prior_n64", "m13_past_lds"])
def test_agrees_with_the_leafspace_posterior(scan, name):
    """forest_predict(method="leafspace") reduced on the host: the same leaf-space quantities, summed in another order"""
    from bark_amd.tree_kernels import forest_predict

    inp = ar.make_inputs(name)
    mu, var = forest_predict(inp.model, inp.data, inp.cand, inp.ft, method="leafspace")
    for kind in ar.KINDS:
        want = ar.acquisition(mu, var, inp.case.kappa, kind)
        _, _, acq = run(scan, name, kind)
        err = float((np.abs(acq - want) / np.abs(want)).max())
        print(f"{name} {kind}: max relative difference to the leaf-space posterior {err:.3g}")
        assert np.allclose(acq, want, rtol=1e-12, atol=0.0)


def test_torch_inputs_stay_on_the_device(scan):
    import torch

    from bark_amd.optimizer import propose_from_candidates

    inp = ar.make_inputs("prior_n64")
    _, at = ar.precheck("prior_n64")["lcb_mean"]
    value, index, acq = run(scan, "prior_n64")
    cand = torch.from_numpy(inp.cand).cuda()
    tv, ti, tacq = scan(inp.model, (torch.from_numpy(inp.X).cuda(), inp.y), cand, inp.ft, return_values=True)
    assert tv.is_cuda and ti.is_cuda and tacq.is_cuda and ti.dtype == torch.int64
    assert tv.item() == value and ti.item() == index and np.array_equal(tacq.cpu().numpy(), acq)
    row = propose_from_candidates(inp.model, inp.data, cand, inp.ft)
    assert row.is_cuda and np.array_equal(row.cpu().numpy(), inp.cand[at])
    assert np.array_equal(propose_from_candidates(inp.model, inp.data, inp.cand, inp.ft), inp.cand[at])


def test_refusals(scan):
    from bark_amd import synthetic
    from bark_amd.optimizer import acquisition_plan
    from bark_amd.tree_kernels import posterior_sample_dim

    inp = ar.make_inputs("m13_past_lds")
    args = (inp.model, inp.data, inp.cand, inp.ft)
    assert acquisition_plan(posterior_sample_dim(inp.F, inp.ft), 13)["variant"] == "global"
    with pytest.raises(ValueError, match="LDS variant"):
        scan(*args, variant="lds")
    with pytest.raises(ValueError, match="unknown variant"):
        scan(*args, variant="fast")
    with pytest.raises(ValueError, match="unknown kind"):
        scan(*args, kind="ucb")
    with pytest.raises(ValueError, match="kappa"):
        scan(*args, kappa=float("nan"))
    with pytest.raises(ValueError, match="kappa"):
        scan(*args, kappa=float("inf"))
    with pytest.raises(ValueError, match="at least one candidate"):
        scan(inp.model, inp.data, inp.cand[:0], inp.ft)
    X, y, bounds, ft = ar.problem(64, 9)
    F65 = synthetic.full_binary_forest(65, ar.D_CONT, 1, np.random.default_rng(9), node_limit=ar.NODE_LIMIT)[None]
    with pytest.raises(ValueError, match="at most 64 trees"):
        scan((F65, [0.1], [1.0]), (X, y), X[:4], ft)
    value, index = scan(*args)  # nothing is left behind
    assert index == ar.precheck("m13_past_lds")["lcb_mean"][1] and np.isfinite(value)


def test_c_entry_refuses_before_any_launch():
    """the C entry itself: C = 0, unknown kind / variant, m = 65 and NaN kappa return BARK_ERR_ARG; the outputs stay untouched"""
    import ctypes

    import torch

    from bark_amd import _lib
    from bark_amd.forest import _feat_types, _points, packed_forest

    inp = ar.make_inputs("m2_r65")
    lib = _lib.lib()
    ft = _feat_types(inp.ft)
    pf = packed_forest(inp.F, ft)
    Xd, _ = _points(inp.X, ft.shape[0])
    cd, _ = _points(inp.cand, ft.shape[0])
    yd = _lib.to_device(inp.y.reshape(-1))
    nd, sd = _lib.to_device(inp.noise), _lib.to_device(inp.scale)
    N, d = Xd.shape
    C, B = cd.shape[0], inp.case.B
    R = int(pf.info.max_bits)
    ws = _lib.workspace(int(lib.bark_acquisition_scan_workspace_bytes(N, R, pf.m, B, C)))
    best = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    info = torch.full((B,), 7, dtype=torch.int32, device="cuda")

    def call(C=C, kappa=1.96, kind=0, variant=0, info_ref=pf.info_ref):
        return lib.bark_acquisition_scan_hip(_lib.ctx(), _lib.ptr(pf.packed), info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd),
                                             _lib.ptr(nd), _lib.ptr(sd), _lib.ptr(cd), C, kappa, kind, variant, None,
                                             _lib.ptr(best), _lib.ptr(idx), _lib.ptr(info), _lib.ptr(ws), ws.numel(), B,
                                             _lib.stream_ptr())

    wide = _lib.PackInfo.from_buffer_copy(pf.info)
    wide.m = 65
    for kw in (dict(C=0), dict(kind=2), dict(kind=-1), dict(variant=3), dict(kappa=float("nan")), dict(kappa=float("-inf")),
               dict(info_ref=ctypes.byref(wide))):
        assert call(**kw) == _lib.BARK_ERR_ARG, kw
    torch.cuda.synchronize()
    assert best.item() == 7.0 and idx.item() == 7 and (info == 7).all()
    assert call() == _lib.BARK_OK
    torch.cuda.synchronize()
    assert idx.item() == ar.precheck("m2_r65")["lcb_mean"][1] and not info.any()


def test_invalid_categorical_value_in_a_candidate(scan):
    inp = ar.make_inputs("prior_n257_chunks")
    cat = int(np.flatnonzero(np.asarray(inp.ft) == 0)[0])
    cand = inp.cand.copy()
    cand[:, cat] = -1.0
    with pytest.raises(ValueError, match="categorical"):
        scan(inp.model, inp.data, cand, inp.ft, chunk=2)
    value, index = scan(inp.model, inp.data, inp.cand, inp.ft, chunk=2)  # the flag is cleared
    assert index == ar.precheck("prior_n257_chunks")["lcb_mean"][1]


def test_guard_bands_around_the_output(scan):
    """acq_out inside a NaN-filled buffer: C values written, nothing in front of or behind them"""
    import torch

    from bark_amd import _lib
    from bark_amd.forest import _feat_types, _points, packed_forest

    name = "prior_n64"
    inp = ar.make_inputs(name)
    _, _, acq = run(scan, name)
    lib = _lib.lib()
    ft = _feat_types(inp.ft)
    pf = packed_forest(inp.F, ft)
    Xd, _ = _points(inp.X, ft.shape[0])
    cd, _ = _points(inp.cand, ft.shape[0])
    yd = _lib.to_device(inp.y.reshape(-1))
    nd, sd = _lib.to_device(inp.noise), _lib.to_device(inp.scale)
    N, d = Xd.shape
    C, B, G = cd.shape[0], inp.case.B, 64
    R = int(pf.info.max_bits)
    buf = torch.full((C + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
    scal = torch.full((2 * G + 1,), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.full((2 * G + 1,), -77, dtype=torch.int64, device="cuda")
    info = torch.full((B + 2 * G,), -77, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(int(lib.bark_acquisition_scan_workspace_bytes(N, R, pf.m, B, C)))
    rc = lib.bark_acquisition_scan_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd),
                                       _lib.ptr(nd), _lib.ptr(sd), _lib.ptr(cd), C, inp.case.kappa, 0, 0,
                                       buf.data_ptr() + 8 * G, scal.data_ptr() + 8 * G, idx.data_ptr() + 8 * G,
                                       info.data_ptr() + 4 * G, _lib.ptr(ws), ws.numel(), B, _lib.stream_ptr())
    assert rc == _lib.BARK_OK
    torch.cuda.synchronize()
    buf, scal, idx, info = buf.cpu().numpy(), scal.cpu().numpy(), idx.cpu().numpy(), info.cpu().numpy()
    assert np.isnan(buf[:G]).all() and np.isnan(buf[-G:]).all() and np.array_equal(buf[G:-G], acq)
    assert np.isnan(scal[:G]).all() and np.isnan(scal[G + 1:]).all() and scal[G] == acq.min()
    assert (idx[:G] == -77).all() and (idx[G + 1:] == -77).all() and idx[G] == int(np.argmin(acq))
    assert (info[:G] == -77).all() and (info[-G:] == -77).all() and not info[G:-G].any()
