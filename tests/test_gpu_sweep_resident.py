"""The one-launch tree sweep — ChainBatch.sweep_trees(method="resident"), csrc/sweep_resident.hip — on the device, against the
host loop (propose_trees / accept driven by lowrank_ref.metropolis), against the same sweep under method="launches" and
against the oracle's MLL of the final forests.  The cases (tests/sweep_resident_ref.py) sit on the edges of the kernel: fewer
points than threads, both variants on either side of N = 128 / 129, odd N, the 8 / 9 rank switch, 16 leaves, 64 chains with a
per-chain r_old, N = 512.  tests/test_sweep_resident_cpu.py holds every case to a decision margin of 1e-6, so the accept masks
must be identical, not close.  The bars are the project's (lowrank_ref.SCALAR_*, MAT_*); the fraction used is printed (-s).

Not tested: the -1 latch of a singular r x r system, which no valid forest reaches (det(C + G) = det K' / det K != 0)."""
import ctypes

import numpy as np
import pytest

import lowrank_ref as lr
import sweep_resident_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bark_amd.fitting as fit
    from bark_amd import _lib
    from oracle import oracle as orc

    class NS:
        pass

    ns = NS()
    ns.torch, ns.lib, ns.L, ns.fit, ns.orc = torch, _lib.lib(), _lib, fit, orc
    return ns


def report(name, worst):
    print(name, "fraction of each bar used:", {k: "%.2g" % v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


def batch(G, inp, chains=None):
    sel = slice(None) if chains is None else chains
    return G.fit.ChainBatch.from_forests(inp.cur[sel], inp.noise[sel], inp.scale[sel], inp.X, inp.y, inp.ft)


def sweep(cb, inp, method, chains=None):
    sel = slice(None) if chains is None else chains
    steps = inp.cur.shape[1]
    return cb.sweep_trees(inp.cur[sel], inp.prop[sel], inp.log_q[sel], inp.log_u[sel], inp.X, inp.ft, inp.scale[sel], steps, method=method)


def host_loop(G, inp):
    """propose_trees / accept with the decision on the host -> (mask, batch)."""
    nc, steps = inp.log_q.shape
    host = batch(G, inp)
    want = np.zeros((nc, steps), dtype=bool)
    for t in range(steps):
        before = host.mll.copy()
        vals = host.propose_trees(inp.cur[:, t], inp.prop[:, t], inp.X, inp.ft, inp.scale, steps)
        want[:, t] = [lr.metropolis(2.0 * (vals[b] - before[b]), 0.0, inp.log_q[b, t], inp.log_u[b, t]) == 1 for b in range(nc)]
        host.accept(want[:, t])
    return want, host


@pytest.mark.parametrize("name", list(sr.CASES))
def test_edge_table(G, name):
    torch = G.torch
    case, inp = sr.CASES[name], sr.make_inputs(name)
    plan = G.fit.sweep_plan(case.N, 16, lr.CHAIN_D, nc=case.nc)
    assert plan["variant"] == (1 if case.N <= 128 else 2)
    want, host = host_loop(G, inp)
    assert 0 < want.sum() < want.size
    launches = batch(G, inp)
    start = launches.K_inv.clone()
    assert torch.equal(start, start.mT), "the starting inverse is not exactly symmetric"
    mask_l = sweep(launches, inp, "launches")
    assert np.array_equal(mask_l, want)
    dev = batch(G, inp)
    assert torch.equal(dev.K_inv, start)
    mask = sweep(dev, inp, "resident")
    assert np.array_equal(mask, want), (mask, want)
    assert np.array_equal(dev.last_accept, want.astype(np.int32))
    worst = {}
    for key, other in (("host", host), ("launches", launches)):
        worst[f"quad vs {key}"] = lr.used(dev.quad, other.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL)
        worst[f"logdet vs {key}"] = lr.used(dev.logdet, other.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL)
    worst["K_inv vs launches"] = lr.used(dev.K_inv.cpu().numpy(), launches.K_inv.cpu().numpy(), lr.MAT_RTOL, lr.MAT_ATOL)
    assert torch.equal(dev.K_inv, dev.K_inv.mT), "K_inv is not exactly symmetric after the sweep"
    for b in range(case.nc):
        if not want[b].any():
            assert torch.equal(dev.K_inv[b], start[b]), (name, b)  # no accepted step: not a bit moved
    final = inp.cur.copy()
    final[want] = inp.prop[want]
    mll = G.orc.batched_mll(final, inp.noise, inp.scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False)
    worst["mll vs oracle (rtol 1e-9, atol 1e-8)"] = lr.used(dev.mll, mll, 1e-9, 1e-8)
    report(name, worst)


@pytest.mark.parametrize("N", [128, 130])
def test_nan_rule(G, N):
    inp = sr.nan_inputs(N)
    want, host = host_loop(G, inp)
    assert not want[0, 1] and not want[1, 2]
    finite = np.isfinite(inp.log_q) & np.isfinite(inp.log_u)
    assert 0 < want[finite].sum() < finite.sum()
    dev = batch(G, inp)
    mask = sweep(dev, inp, "resident")
    assert not mask[0, 1], "a NaN log_u was accepted"
    assert not mask[1, 2], "a NaN log_q_prior was accepted"
    assert np.array_equal(mask, want), (mask, want)
    report(f"nan/N{N}", {"quad": lr.used(dev.quad, host.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
                         "logdet": lr.used(dev.logdet, host.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL)})


def test_g11_replay(G):
    """Part (b) of test_gpu_context.test_g11_reference_sampler_steps_replayed_on_the_device with method="resident"."""
    from conftest import load_golden

    fit, orc = G.fit, G.orc
    g = load_golden("g11_sampler_steps")
    X, y, ft = g["X"], g["y"], g["feat_types"]
    chains, steps, m = g["accept"].shape
    tol = dict(rtol=1e-9, atol=1e-8)
    forests = orc.nodes_from_raw(g["start_forest"]).copy()
    noise, scale = g["start_noise"].copy(), g["start_scale"].copy()
    cb = fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
    for s in range(steps):
        old, new = orc.nodes_from_raw(g["old"][:, s]), orc.nodes_from_raw(g["new"][:, s])
        assert np.array_equal(old, forests)
        mask = cb.sweep_trees(old, new, g["log_q"][:, s], np.log(g["u"][:, s]), X, ft, scale, m, method="resident")
        assert np.array_equal(mask, g["accept"][:, s])
        forests[mask] = new[mask]
        assert np.allclose(cb.mll, g["cur_mll"][:, s, -1], **tol)
        acc = g["ns_accept"][:, s].astype(bool)
        noise = np.where(acc, g["ns_prop"][:, s, 0], noise)
        scale = np.where(acc, g["ns_prop"][:, s, 1], scale)
        if acc.any():
            cb = fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
        assert np.allclose(cb.mll, g["mll_after"][:, s], **tol)


def test_repeatable_and_chains_isolated(G):
    """The same sweep twice from the same start: the same bits.  The start is copied, not rebuilt: a batch's initial y'K^-1 y comes
    from bark_quadform_hip, whose workgroups add their shares atomically, so two builds may differ in its last bit."""
    torch = G.torch
    inp = sr.make_inputs("n129")
    a, b2 = batch(G, inp), batch(G, inp)
    assert torch.equal(a.K_inv, b2.K_inv)
    b2.quad, b2.logdet = a.quad.copy(), a.logdet.copy()
    ma, mb = sweep(a, inp, "resident"), sweep(b2, inp, "resident")
    assert np.array_equal(ma, mb) and torch.equal(a.K_inv, b2.K_inv)
    assert np.array_equal(a.quad, b2.quad) and np.array_equal(a.logdet, b2.logdet)
    for name, nc in (("n128", 4), ("n129", 3)):  # both variants: chain b of a batch == chain b alone
        inp = sr.make_inputs(name)
        chains = list(range(nc))
        full = batch(G, inp, chains)
        start_K, start_quad, start_logdet = full.K_inv.clone(), full.quad.copy(), full.logdet.copy()
        mfull = sweep(full, inp, "resident", chains)
        for b in chains:
            one = batch(G, inp, [b])
            one.K_inv.copy_(start_K[b:b + 1])  # the dense inverse agrees between batch sizes to rounding only
            one.quad, one.logdet = start_quad[b:b + 1].copy(), start_logdet[b:b + 1].copy()
            mone = sweep(one, inp, "resident", [b])
            assert np.array_equal(mone[0], mfull[b]) and torch.equal(one.K_inv[0], full.K_inv[b]), (name, b)
            assert one.quad[0] == full.quad[b] and one.logdet[0] == full.logdet[b], (name, b)


def raw_call(G, inp, K, state, accept, ws, nc=None):
    """bark_tree_sweep_resident_hip on caller-owned buffers (the packing of sweep_trees, restated)."""
    from bark_amd.forest import _feat_types, _points

    L, lib, torch = G.L, G.lib, G.torch
    nc_, steps = inp.log_q.shape
    nc = nc or nc_
    ft = _feat_types(inp.ft)
    Xd, _ = _points(inp.X, ft.shape[0])
    infos = (L.PackInfo * steps)()
    r_old = np.empty((steps, nc), dtype=np.int64)
    pairs, sizes = [], []
    info_one = L.PackInfo()
    for t in range(steps):
        pair = np.ascontiguousarray(np.stack([inp.cur[:nc, t], inp.prop[:nc, t]], axis=1))
        pairs.append(pair)
        L.check(lib.bark_forest_pack_info(L.ptr(pair), nc, 2, pair.shape[2], L.ptr(ft), ft.shape[0], ctypes.byref(infos[t])))
        sizes.append(int(infos[t].packed_bytes))
        for b in range(nc):
            L.check(lib.bark_forest_pack_info(L.ptr(np.ascontiguousarray(inp.cur[b, t])), 1, 1, pair.shape[2], L.ptr(ft), ft.shape[0],
                                              ctypes.byref(info_one)))
            r_old[t, b] = info_one.max_bits
    offsets = np.zeros(steps, dtype=np.int64)
    offsets[1:] = np.cumsum([(sz + 255) // 256 * 256 for sz in sizes[:-1]])
    host = torch.empty(int(offsets[-1]) + sizes[-1], dtype=torch.uint8)
    for t in range(steps):
        L.check(lib.bark_forest_pack(L.ptr(pairs[t]), L.ptr(ft), ft.shape[0], ctypes.byref(infos[t]),
                                     ctypes.c_void_p(host.data_ptr() + int(offsets[t]))))
    table = np.empty(int(lib.bark_tree_sweep_resident_table_bytes(steps, nc)) // 8, dtype=np.int64)
    L.check(lib.bark_tree_sweep_resident_table(L.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), L.ptr(r_old), steps, nc, L.ptr(table)))
    keep = [host.cuda(), L.to_device(table), L.to_device(np.sqrt(inp.scale[:nc] / steps)), L.to_device(inp.y.reshape(-1)),
            L.to_device(np.ascontiguousarray(inp.log_q[:nc].T)), L.to_device(np.ascontiguousarray(inp.log_u[:nc].T)), Xd]
    packed, table_d, s_d, y_d, lq, lu, _ = keep

    def call():
        return lib.bark_tree_sweep_resident_hip(L.ctx(), L.ptr(K), inp.X.shape[0], nc, steps, L.ptr(packed), L.ptr(table_d), L.ptr(Xd),
                                                Xd.shape[1], L.ptr(s_d), L.ptr(y_d), L.ptr(lq), L.ptr(lu), L.ptr(state), L.ptr(accept),
                                                ctypes.c_void_p(ws.data_ptr()), int(lib.bark_tree_sweep_resident_workspace_bytes(
                                                    inp.X.shape[0], 16, nc)), L.stream_ptr())
    return call, keep


def guarded(G, shape, dtype, fill):
    """A tensor of `shape` between two bands of NaN (float64) or of a pattern (other types)."""
    torch = G.torch
    n, band = int(np.prod(shape)), 512
    pat = float("nan") if dtype == torch.float64 else 0x5A
    buf = torch.full((n + 2 * band,), pat, dtype=dtype, device="cuda")
    view = buf[band:band + n].view(*shape)
    view.copy_(fill)
    intact = (lambda: bool(torch.isnan(buf[:band]).all() and torch.isnan(buf[band + n:]).all())) if dtype == torch.float64 \
        else (lambda: bool((buf[:band] == 0x5A).all() and (buf[band + n:] == 0x5A).all()))
    return view, intact


@pytest.mark.parametrize("name", ["n127", "n129"])
def test_guard_bands_and_one_launch(G, name):
    """NaN bands around K_inv, state, accept_out and the workspace stay intact.  The entry point enqueues one kernel and nothing
    else — no copy, no allocation, no synchronisation —, so it can be captured in a graph: the capture runs nothing, and one
    replay from the same start gives the eager call's bits."""
    torch = G.torch
    inp = sr.make_inputs(name)
    nc, steps = inp.log_q.shape
    ref = batch(G, inp)
    start = ref.K_inv.clone()
    state0 = torch.tensor(np.stack([ref.quad, ref.logdet], axis=1), device="cuda")
    want = sweep(ref, inp, "resident")
    K, K_ok = guarded(G, start.shape, torch.float64, start)
    state, st_ok = guarded(G, (nc, 2), torch.float64, state0)
    accept, ac_ok = guarded(G, (steps, nc), torch.int32, torch.zeros((steps, nc), dtype=torch.int32, device="cuda"))
    ws, ws_ok = guarded(G, (256,), torch.uint8, torch.zeros(256, dtype=torch.uint8, device="cuda"))
    call, keep = raw_call(G, inp, K, state, accept, ws)
    G.L.check(call())
    torch.cuda.synchronize()
    assert K_ok() and st_ok() and ac_ok() and ws_ok()
    assert torch.equal(K, ref.K_inv) and np.array_equal(accept.cpu().numpy().T > 0, want)
    assert np.array_equal(state.cpu().numpy()[:, 0], ref.quad) and np.array_equal(state.cpu().numpy()[:, 1], ref.logdet)
    # the same call captured and replayed once from the same start
    K.copy_(start)
    state.copy_(state0)
    accept.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.L.check(call())
    torch.cuda.synchronize()
    assert torch.equal(K, start), "capture must not run the kernel"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(K, ref.K_inv) and np.array_equal(accept.cpu().numpy().T > 0, want)
    assert K_ok() and st_ok() and ac_ok() and ws_ok()


def test_refusals(G):
    torch, fit = G.torch, G.fit
    inp = sr.make_inputs("n64")
    cb = batch(G, inp)
    before = cb.K_inv.clone()
    big = inp.prop.copy()
    big[0, 1] = lr.caterpillar_tree(15, 0)  # 2 + 15 = 17 leaves in one pair
    with pytest.raises(ValueError, match='method="launches"'):
        cb.sweep_trees(inp.cur, big, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, 4, method="resident")
    assert torch.equal(cb.K_inv, before)
    # a pair whose packed nodes do not fit their 2 KiB of LDS: 70 splits in a row whose two children are the same next node (walkable,
    # one leaf), 71 packed nodes where at most 64 fit
    from bark_amd.forest import NODE_RECORD_DTYPE

    deep = np.zeros(inp.prop.shape[2], dtype=NODE_RECORD_DTYPE)
    for k in range(70):
        deep[k] = (0, 0, 0.5, k + 1, k + 1, 0xFFFFFFFF if k == 0 else k - 1, k, 1)
    deep[70] = (1, 0, 0, 0, 0, 69, 70, 1)
    big = inp.prop.copy()
    big[1, 2] = deep
    with pytest.raises(ValueError, match='method="launches"'):
        cb.sweep_trees(inp.cur, big, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, 4, method="resident")
    assert torch.equal(cb.K_inv, before)
    mask = cb.sweep_trees(inp.cur, big, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, 4, method="launches")  # the other path takes it
    assert mask.shape == (2, 4)
    from bark_amd import synthetic

    X, y, _, ft = synthetic.unit_cube_problem(513, lr.CHAIN_D, seed=5)
    cur = np.stack([lr.caterpillar_tree(2, 0), lr.caterpillar_tree(3, 1)])[None]
    cb = fit.ChainBatch.from_forests(cur, [0.1], [1.0], X, y, ft)
    before = cb.K_inv.clone()
    with pytest.raises(ValueError, match='method="launches"'):
        cb.sweep_trees(cur, np.ascontiguousarray(cur[:, ::-1]), np.zeros((1, 2)), np.zeros((1, 2)), X, ft, [1.0], 2, method="resident")
    assert torch.equal(cb.K_inv, before)
    with pytest.raises(ValueError):
        cb.sweep_trees(cur, cur, np.zeros((1, 2)), np.zeros((1, 2)), X, ft, [1.0], 2, method="resident_lds")
    # 65 chains: the batch itself refuses them, and so does the entry point, before it looks at a pointer's target
    with pytest.raises(ValueError):
        fit.ChainBatch(np.zeros((65, 4, 4)), np.zeros(65), np.zeros(4))
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = G.lib.bark_tree_sweep_resident_hip(G.L.ctx(), G.L.ptr(one), 4, 65, 1, G.L.ptr(one), G.L.ptr(one), G.L.ptr(one), 1, G.L.ptr(one),
                                            G.L.ptr(one), G.L.ptr(one), G.L.ptr(one), G.L.ptr(one), G.L.ptr(one), G.L.ptr(one), 256,
                                            G.L.stream_ptr())
    assert rc == G.L.BARK_ERR_ARG and b"bark_tree_sweep_chains_hip" in G.lib.bark_last_error()
    assert not bool(one.any())


def test_categorical_fault(G):
    """One invalid categorical value that a walk reaches raises ValueError, as under method="launches" (mixed domain, N = 64)."""
    from bark_amd import synthetic

    X, y, bounds, ft = synthetic.mixed_problem(64, seed=3)
    cat = int(np.flatnonzero(np.asarray(ft) == 0)[0])
    forests = synthetic.sample_prior_forests(2, 3, bounds, ft, seed=3)
    prop = synthetic.sample_prior_forests(2, 3, bounds, ft, seed=4)
    from bark_amd.forest import NODE_RECORD_DTYPE

    tree = np.zeros(forests.shape[2], dtype=NODE_RECORD_DTYPE)  # one split on the categorical feature, two leaves
    tree[0] = (0, cat, 1.0, 1, 2, 0xFFFFFFFF, 0, 1)
    tree[1] = (1, 0, 0, 0, 0, 0, 1, 1)
    tree[2] = (1, 0, 0, 0, 0, 0, 1, 1)
    prop[1, 2] = tree
    noise, scale = np.array([0.1, 0.2]), np.array([1.0, 0.9])
    lq, lu = np.zeros((2, 3)), np.full((2, 3), -0.5)
    for method in ("launches", "resident"):
        cb = G.fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
        cb.sweep_trees(forests, prop, lq, lu, X, ft, scale, 3, method=method)  # valid values: fine
        bad = np.array(X, dtype=np.float64, copy=True)
        bad[17, cat] = -1.0
        cb = G.fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
        with pytest.raises(ValueError, match="categorical"):
            cb.sweep_trees(forests, prop, lq, lu, bad, ft, scale, 3, method=method)
