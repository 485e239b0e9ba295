"""Leaf-space sampler chains — bark_amd.fitting.LeafChainBatch, csrc/leafchain.hip — on the device, against the host reference
(tests/leafchain_ref.py), against ChainBatch.sweep_trees(method="launches") on the same inputs and against the oracle's MLL of
the final forests.  tests/test_leafchain_reference_cpu.py holds every case to a decision margin of 1e-6, so the accept masks
must be identical, not close.  Bars: the project's scalar bar (rtol 1e-9 / atol 1e-9) and matrix bar (rtol 1e-9 / atol 1e-11);
for case n4097 the matrix bar is 100 x the host reference's own float64-against-longdouble deviation.

The cases m64_cap1024, m64_tight and odd67 take the kernel to the corners of its limits (64 trees, 32 leaves per tree, 1024
slots): small inverses of 23 and 32 rows, steps 4 and 6 past one pass of the workgroup, a 63-node tree in LDS, capacities above
the 512 threads and off every multiple of 8, more than 512 active slots with gaps in `lc_build_inverse`, swaps of tree 63, and a
free stack that is pushed 31 deep and popped again, so that the bit-for-bit comparison of slot map and stack with the host
reference says something.  tests/test_leafchain_reference_cpu.py (test_table_contains_the_wide_edges) holds the table to
containing these steps, taken or refused as needed.  ChainBatch accepts every step of the table (r_old + r_new <= 64), so every
case is compared with the launches route too.  Chain isolation, the noise / scale step and the guard bands run on one small
case and on m64_cap1024.

Not tested: the -1 latch of a non-positive pivot in P_TT or S, which no valid forest reaches; N above 4097."""
import numpy as np
import pytest

import leafchain_ref as lc
import lowrank_ref as lr

pytestmark = pytest.mark.gpu

_REF = {}


def ref(name):
    if name not in _REF:
        inp = lc.make_inputs(name)
        _REF[name] = (inp, lc.leaf_sweep(inp))
    return _REF[name]


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


def batch(G, inp, chains=None, capacity=None):
    sel = slice(None) if chains is None else chains
    return G.fit.LeafChainBatch.from_forests(inp.forests[sel], inp.noise[sel], inp.scale[sel], inp.X, inp.y, inp.ft,
                                             capacity=inp.capacity if capacity is None else capacity, lcap=inp.lcap)


def sweep(cb, inp, chains=None):
    sel = slice(None) if chains is None else chains
    return cb.sweep_trees(inp.old[sel], inp.new[sel], inp.log_q[sel], inp.log_u[sel], inp.X, inp.ft, inp.scale[sel],
                          inp.forests.shape[1], tree_index=inp.tree_index)


def dense_launches(G, inp):
    """ChainBatch.sweep_trees(method="launches"), one step per call with the tree the chain really holds -> (mask, batch)."""
    nc, steps = inp.log_q.shape
    m = inp.forests.shape[1]
    cb = G.fit.ChainBatch.from_forests(inp.forests, inp.noise, inp.scale, inp.X, inp.y, inp.ft)
    cur = inp.forests.copy()
    mask = np.zeros((nc, steps), dtype=bool)
    for t in range(steps):
        k = int(inp.tree_index[t])
        mask[:, t] = cb.sweep_trees(cur[:, k][:, None], inp.new[:, t][:, None], inp.log_q[:, t:t + 1], inp.log_u[:, t:t + 1], inp.X,
                                    inp.ft, inp.scale, m, method="launches")[:, 0]
        cur[mask[:, t], k] = inp.new[mask[:, t], t]
    return mask, cb


def check_free_slots(dev, b, host=None):
    """The resident block itself (not the export): every slot no leaf holds is an identity row and column of P with a zero plane
    and v = 0, the free stack holds exactly those slots, and the slot map is the host reference's."""
    raw = dev.raw()
    P, v, planes, slots, nl, free = (raw[k][b] for k in ("P", "v", "planes", "slots", "nleaves", "free"))
    used = [int(slots[t, l]) for t in range(dev.m) for l in range(nl[t])]
    assert len(set(used)) == len(used) and all(0 <= s < dev.capacity for s in used)
    rest = sorted(set(range(dev.capacity)) - set(used))
    assert sorted(free.tolist()) == rest, "the free stack is not the complement of the slot map"
    eye = np.eye(dev.capacity)
    assert np.array_equal(P[rest], eye[rest]) and np.array_equal(P[:, rest], eye[:, rest]), "a free slot is not an identity row / column"
    assert not planes[rest].any() and not v[rest].any(), "a free slot keeps a plane or a v entry"
    assert (slots[np.arange(dev.lcap)[None, :] >= nl[:, None]] == -1).all()
    if host is not None:
        assert [list(slots[t, :nl[t]]) for t in range(dev.m)] == host.slots and free.tolist() == host.free


@pytest.mark.parametrize("name", list(lc.CASES))
def test_cases(G, name):
    case = lc.CASES[name]
    inp, want = ref(name)
    dev = batch(G, inp)
    # the state is smaller than an N x N inverse; the wide cases hold more slots than points (P alone is 8 capacity^2 bytes)
    assert dev.sweep_plan()["chain_bytes"] < 8 * case.N * case.N or case.N < 300 or inp.capacity >= case.N
    mask = sweep(dev, inp)
    assert np.array_equal(mask, want.mask == 1), (mask, want.mask)
    mask_l, launches = dense_launches(G, inp)
    assert np.array_equal(mask, mask_l)
    worst = {"quad vs host": lr.used(dev.quad, want.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
             "logdet vs host": lr.used(dev.logdet, want.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
             "quad vs launches": lr.used(dev.quad, launches.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
             "logdet vs launches": lr.used(dev.logdet, launches.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL)}
    mll = G.orc.batched_mll(want.final, inp.noise, inp.scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False)
    worst["mll vs oracle"] = lr.used(dev.mll, mll, lr.SCALAR_RTOL, lr.SCALAR_ATOL)
    out = dev.export()
    R = out["nleaves"].sum(axis=1)
    for b in range(case.nc):
        P, (Pw, vw, nlw) = out["P"][b], want.chains[b].export()
        assert np.array_equal(out["nleaves"][b], nlw) and np.array_equal(dev.nleaves[b], nlw)
        assert np.array_equal(P, P.T), "P is not exactly symmetric"
        assert np.array_equal(P[R[b]:], np.eye(inp.capacity)[R[b]:]), "rows past the leaves are not identity rows"
        check_free_slots(dev, b, want.chains[b])
        assert lr.used(out["v"][b], vw, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0, "v = Z'y"
        dense = lc.dense_P(want.final[b], inp.noise[b], inp.scale[b], inp.X, inp.ft, inp.capacity)
        if case.matrix:
            worst["P vs inv(M)"] = max(worst.get("P vs inv(M)", 0.0), lr.used(P, dense, lr.MAT_RTOL, lr.MAT_ATOL))
        else:
            worst["P vs host (100 x its own deviation)"] = max(worst.get("P vs host (100 x its own deviation)", 0.0),
                                                                float(np.abs(P - Pw).max()) / (100 * lc.N4097_P_DEVIATION))
    report(name, worst)


def test_g11_replay(G):
    """The reference sampler's recorded steps (tests/golden/g11_sampler_steps; the CPU file holds them to the pre-check) on the
    leaf-space state alone: tree sweeps and noise / scale proposals, no rebuild in between."""
    from conftest import load_golden

    g = load_golden("g11_sampler_steps")
    pre = lc.g11_replay()
    X, y, ft = g["X"], g["y"], g["feat_types"]
    chains, steps, m = g["accept"].shape
    tol = dict(rtol=1e-9, atol=1e-8)
    forests = G.orc.nodes_from_raw(g["start_forest"]).copy()
    cb = G.fit.LeafChainBatch.from_forests(forests, g["start_noise"], g["start_scale"], X, y, ft, capacity=pre.capacity, lcap=pre.lcap)
    assert np.allclose(cb.mll, g["start_mll"], **tol)
    for s in range(steps):
        old, new = G.orc.nodes_from_raw(g["old"][:, s]), G.orc.nodes_from_raw(g["new"][:, s])
        assert np.array_equal(old, forests)
        mask = cb.sweep_trees(old, new, g["log_q"][:, s], np.log(g["u"][:, s]), X, ft, cb.scale, m)
        assert np.array_equal(mask, g["accept"][:, s])
        forests[mask] = new[mask]
        assert np.allclose(cb.mll, g["cur_mll"][:, s, -1], **tol)
        took = cb.step_noise_scale(g["ns_prop"][:, s, 0], g["ns_prop"][:, s, 1], g["ns_log_q"][:, s], np.log(g["ns_u"][:, s]))
        assert np.array_equal(took, g["ns_accept"][:, s])
        assert np.allclose(cb.mll, g["mll_after"][:, s], **tol)
        assert np.allclose(cb.noise, g["noise_after"][:, s]) and np.allclose(cb.scale, g["scale_after"][:, s])
    for b in range(chains):
        check_free_slots(cb, b)


WIDE = ["n65", "m64_cap1024"]  # one small case and the full box: two chains each


@pytest.mark.parametrize("name", WIDE)
def test_repeatable_and_chains_isolated(G, name):
    torch = G.torch
    inp, want = ref(name)
    m = inp.forests.shape[1]
    a, b2 = batch(G, inp), batch(G, inp)
    assert torch.equal(a.state, b2.state) and np.array_equal(a.quad, b2.quad)
    ma, mb = sweep(a, inp), sweep(b2, inp)
    assert np.array_equal(ma, mb) and torch.equal(a.state, b2.state)
    assert np.array_equal(a.quad, b2.quad) and np.array_equal(a.logdet, b2.logdet)
    stride = a.sweep_plan()["chain_bytes"]
    for b in range(2):  # chain b of a batch == chain b alone, bit for bit
        one = batch(G, inp, [b])
        mone = sweep(one, inp, [b])
        assert np.array_equal(mone[0], ma[b]) and torch.equal(one.state, a.state[b * stride:(b + 1) * stride])
        assert one.quad[0] == a.quad[b] and one.logdet[0] == a.logdet[b]
    # a chain whose every proposal is rejected keeps its bits, whatever its neighbour does
    c = batch(G, inp)
    before = c.state.clone()
    lu = inp.log_u.copy()
    lu[1] = 1.0  # log_u > 0: never accepted
    m1 = c.sweep_trees(inp.old, inp.new, inp.log_q, lu, inp.X, inp.ft, inp.scale, m, tree_index=inp.tree_index)
    assert not m1[1].any() and np.array_equal(m1[0], ma[0])
    assert torch.equal(c.state[stride:], before[stride:]) and c.quad[1] == batch(G, inp).quad[1]


def test_nan_rule(G):
    inp, want = ref("n63")
    lq, lu = inp.log_q.copy(), inp.log_u.copy()
    lu[0, 0], lq[1, 0] = np.nan, np.nan
    dev = batch(G, inp)
    mask = dev.sweep_trees(inp.old, inp.new, lq, lu, inp.X, inp.ft, inp.scale, inp.forests.shape[1], tree_index=inp.tree_index)
    assert not mask[0, 0], "a NaN log_u was accepted"
    assert not mask[1, 0], "a NaN log_q_prior was accepted"
    chk = lc.leaf_sweep(inp._replace(log_q=lq, log_u=lu))
    assert chk.margin.min() >= lc.MARGIN and np.array_equal(mask, chk.mask == 1)


def test_refusals(G):
    torch = G.torch
    inp, _ = ref("n129")  # the worst case of this sweep needs 24 slots
    m = inp.forests.shape[1]
    with pytest.raises(ValueError, match="capacity"):
        sweep(batch(G, inp, capacity=23), inp)
    cb = batch(G, inp)
    before = cb.state.clone()
    big = inp.new.copy()
    big[1, 2] = lr.caterpillar_tree(9, 0)  # lcap + 1 leaves
    with pytest.raises(ValueError, match="leaves"):
        cb.sweep_trees(inp.old, big, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, m, tree_index=inp.tree_index)
    wrong = inp.old.copy()
    wrong[0, 0] = lr.caterpillar_tree(5, 0)  # not the tree the chain holds
    with pytest.raises(ValueError, match="old_trees"):
        cb.sweep_trees(wrong, inp.new, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, m, tree_index=inp.tree_index)
    with pytest.raises(ValueError):
        cb.sweep_trees(inp.old, inp.new, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, m, tree_index=[0, m, 1, 1])
    assert torch.equal(cb.state, before)
    with pytest.raises(ValueError):
        G.fit.LeafChainBatch.from_forests(np.repeat(inp.forests[:1], 65, axis=0), 0.1, 1.0, inp.X, inp.y, inp.ft)
    with pytest.raises(ValueError, match="lcap"):
        G.fit.LeafChainBatch.from_forests(inp.forests, inp.noise, inp.scale, inp.X, inp.y, inp.ft, lcap=7)
    with pytest.raises(ValueError, match="trees"):  # 65 trees
        G.fit.LeafChainBatch.from_forests(np.repeat(inp.forests[:, :1], 65, axis=1), inp.noise, inp.scale, inp.X, inp.y, inp.ft)
    tight = lc.make_inputs("m64_tight")  # its capacity is the sweep's worst case exactly: one slot less is refused before any launch
    cb = batch(G, tight, capacity=tight.capacity - 1)
    before = cb.state.clone()
    with pytest.raises(ValueError, match="capacity"):
        sweep(cb, tight)
    assert torch.equal(cb.state, before)
    one = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = G.L.ptr(one)
    rc = G.lib.bark_leafchain_sweep_hip(G.L.ctx(), p, 4, 1025, 2, 4, 1, 1, p, p, p, 1, p, p, p, p, p, p, 1 << 30, G.L.stream_ptr())
    assert rc == G.L.BARK_ERR_ARG and b"slots" in G.lib.bark_last_error() and not bool(one.any())


@pytest.mark.parametrize("name", WIDE)
def test_noise_scale_step(G, name):
    """Accepted, rejected and a negative scale (-1 -> LinAlgError, nothing written), against ChainBatch.step_noise_scale; at
    m64_cap1024 `lc_build_inverse` eliminates 576 active slots, more than the workgroup has threads.  The proposals' MLL
    differences, which only place log_u half a unit to either side of the decision, are the oracle's."""
    inp, want = ref(name)
    m = inp.forests.shape[1]
    dev = batch(G, inp)
    dense = G.fit.ChainBatch.from_forests(inp.forests, inp.noise, inp.scale, inp.X, inp.y, inp.ft)
    assert lr.used(dev.mll, dense.mll, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    nn, ns = inp.noise * np.array([1.3, 0.8]), inp.scale * np.array([0.9, 1.2])
    mll = lambda noise, scale: G.orc.batched_mll(inp.forests, noise, scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False)
    deltas = mll(nn, ns) - mll(inp.noise, inp.scale)
    lq = np.zeros(2)
    # chain 0 accepted; chain 1 rejected by the comparison itself where a non-positive log_u allows it
    lu = np.array([min(deltas[0], 0.0) - 0.5, deltas[1] + 0.5 if deltas[1] < -0.6 else 0.5])
    expect = np.array([True, bool(lu[1] <= deltas[1] and lu[1] <= 0.0)])
    assert expect[0] and not expect[1]
    before = dev.state.clone()
    stride = dev.sweep_plan()["chain_bytes"]
    mask = dev.step_noise_scale(nn, ns, lq, lu)
    mask_d = dense.step_noise_scale(inp.forests, nn, ns, lq, lu, inp.X, inp.ft)
    assert np.array_equal(mask, expect) and np.array_equal(mask_d, expect)
    assert G.torch.equal(dev.state[stride:], before[stride:]), "a rejected chain was written"
    report("noise/scale", {"quad": lr.used(dev.quad, dense.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL),
                           "logdet": lr.used(dev.logdet, dense.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL)})
    assert dev.noise[0] == nn[0] and dev.noise[1] == inp.noise[1]
    now = lc.dense_P(inp.forests[0], nn[0], ns[0], inp.X, inp.ft, inp.capacity)
    assert lr.used(dev.export()["P"][0], now, lr.MAT_RTOL, lr.MAT_ATOL) <= 1.0
    # the sweep goes on from the accepted values
    mask2 = dev.sweep_trees(inp.old, inp.new, inp.log_q, np.full_like(inp.log_u, 1.0), inp.X, inp.ft, dev.scale, m, tree_index=inp.tree_index)
    assert not mask2.any()
    before = dev.state.clone()
    quad = dev.quad.copy()
    with pytest.raises(np.linalg.LinAlgError):
        dev.step_noise_scale(nn, np.array([-1.0, 1.0]), lq, np.array([-50.0, 1.0]))
    assert G.torch.equal(dev.state, before) and np.array_equal(dev.quad, quad)
    m3 = dev.step_noise_scale(np.array([-1.0, 0.1]), ns, lq, np.array([-50.0, 1.0]))  # 1e-6 + noise <= 0: rejected, not an error
    assert not m3.any() and G.torch.equal(dev.state, before)


@pytest.mark.parametrize("name", WIDE)
def test_guard_bands_and_graph_capture(G, name):
    """The state block and the workspace sit between bands that stay intact, and the sweep — one enqueued kernel — is captured
    in a graph: the capture runs nothing, one replay gives the eager call's bits.  At m64_cap1024 the workspace matrices run at
    1024 x 32 and P and the scratch inverse at 1024 x 1024, the largest the layout allows."""
    torch = G.torch
    inp, want = ref(name)
    cb = batch(G, inp)
    start, mstate0 = cb.state.clone(), cb._mstate.clone()
    band = 4096

    def guarded(t):
        buf = torch.full((t.numel() + 2 * band,), 0x5A, dtype=torch.uint8, device="cuda")
        buf[band:band + t.numel()].copy_(t.view(torch.uint8).reshape(-1))
        return buf, (lambda: bool((buf[:band] == 0x5A).all() and (buf[band + t.numel():] == 0x5A).all()))

    sbuf, s_ok = guarded(start)
    wbuf, w_ok = guarded(cb._ws)
    cb.state, cb._ws = sbuf[band:band + start.numel()], wbuf[band:band + cb._ws.numel()]
    mask = sweep(cb, inp)
    assert np.array_equal(mask, want.mask == 1) and s_ok() and w_ok()
    final, mfinal = cb.state.clone(), cb._mstate.clone()
    cb.state.copy_(start)
    cb._mstate.copy_(mstate0)
    cb.nleaves = batch(G, inp).nleaves
    enqueue, accept, tidx, r_new, ft = cb._prepare_sweep(inp.old, inp.new, inp.log_q, inp.log_u, inp.X, inp.ft, inp.scale, inp.forests.shape[1],
                                                             inp.tree_index)
    accept.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    torch.cuda.synchronize()
    assert torch.equal(cb.state, start), "capture must not run the kernel"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cb.state, final) and torch.equal(cb._mstate, mfinal)
    assert np.array_equal(accept.cpu().numpy().T > 0, mask) and s_ok() and w_ok()
    # the noise / scale step (writes capacity^2 doubles of the workspace) and the export between the same bands
    cb.nleaves = np.stack([c_.export()[2] for c_ in want.chains])  # the replay ran behind the class's back
    cb._take_state()
    cb.step_noise_scale(inp.noise * 1.1, inp.scale * 0.9, np.zeros(2), np.array([-50.0, 1.0]))
    out = cb.export()
    torch.cuda.synchronize()
    assert s_ok() and w_ok() and np.array_equal(out["nleaves"], cb.nleaves)
