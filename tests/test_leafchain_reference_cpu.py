"""The host reference of the leaf-space sampler chains (tests/leafchain_ref.py) against the dense route, and the conditions its
case table must meet for tests/test_gpu_leafchain.py to ask for identical accept masks.  No GPU; the query and the table builder
are host code of the library."""
import ctypes

import numpy as np
import pytest

import leafchain_ref as lc
import lowrank_ref as lr

_CACHE = {}


def runs(name):
    if name not in _CACHE:
        inp = lc.make_inputs(name)
        _CACHE[name] = (inp, lc.leaf_sweep(inp), lc.leaf_sweep(inp, np.longdouble), lc.dense_sweep(inp))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case_conditions(name):
    """float64, longdouble and the dense route decide alike, with a margin of 1e-6; the float64 scalars stay within 1 % of the
    scalar bar of longdouble; cases marked `matrix` keep the exported P within 10 % of the matrix bar of longdouble and inside
    the bar of inv(M) of the final forest."""
    case = lc.CASES[name]
    inp, f64, ext, dense = runs(name)
    assert inp.noise.min() >= 1e-2
    assert np.array_equal(f64.mask, ext.mask) and np.array_equal(f64.mask, dense.mask)
    assert min(f64.margin.min(), ext.margin.min(), dense.margin.min()) >= lc.MARGIN
    assert 0 < f64.mask.sum() < f64.mask.size or name == "n3"
    assert lr.used(f64.quad, ext.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 0.01
    assert lr.used(f64.logdet, ext.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 0.01
    assert lr.used(f64.quad, dense.quad, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    assert lr.used(f64.logdet, dense.logdet, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 1.0
    dev = 0.0
    for b in range(case.nc):
        P, v, nl = f64.chains[b].export()
        Pe, ve, nle = ext.chains[b].export()
        assert np.array_equal(nl, nle) and np.array_equal(P, P.T)
        dev = max(dev, float(np.abs(P - Pe).max()))
        if case.matrix:
            assert lr.used(P, Pe, lr.MAT_RTOL, lr.MAT_ATOL) <= 0.1
            want = lc.dense_P(f64.final[b], inp.noise[b], inp.scale[b], inp.X, inp.ft, inp.capacity)
            assert lr.used(P, want, lr.MAT_RTOL, lr.MAT_ATOL) <= 1.0
    print(name, "max |P(float64) - P(longdouble)| = %.3g" % dev)
    if name == "n4097":  # the figure the device's matrix bar of this case is 100 x of
        assert dev <= lc.N4097_P_DEVIATION


def test_table_contains_the_wide_edges():
    """The edges the wide cases exist for are really in the table — conditions on the host reference's trajectory (taken steps,
    RefChain's free stack), not measurements: without them tests/test_gpu_leafchain.py would pass without having run them."""
    wide, tight, odd = (runs(name)[1] for name in ("m64_cap1024", "m64_tight", "odd67"))
    steps = lc.CASES["m64_cap1024"].steps
    every = [(steps[t], s) for chain in wide.log for t, s in enumerate(chain)]
    taken = [(step, s) for step, s in every if s.accepted]
    assert any(s.r_old == 32 and s.r_new == 32 for _, s in taken), "no accepted 32 -> 32 swap"
    assert any(s.r_new >= 23 and s.r_old <= 9 for _, s in taken), "no accepted swap from <= 9 to >= 23 leaves"
    assert any(step[0] == 63 for step, _ in taken), "no accepted swap of tree 63"
    assert any(step[1] == "dead" and s.r_new == 32 for step, s in taken), "no accepted 32-leaf proposal of unreached leaves"
    assert any(s.r_new == 32 and not s.accepted for _, s in every), "no rejected 32-leaf proposal"
    assert any(len(s.popped) >= 23 for _, s in taken) and any(len(s.pushed) == 31 for _, s in taken)
    # an accepted step computes q' afresh, so the returned scalars see only the last one: it must be a 32-leaf proposal somewhere
    assert any([s.r_new for s in chain if s.accepted][-1] == 32 for chain in wide.log), "no chain ends on an accepted 32-leaf swap"

    def pops_what_was_pushed(chain):
        for t, s in enumerate(chain):
            if s.accepted and (s.r_old, s.r_new) == (32, 1):
                assert len(s.pushed) == 31
                for later in chain[t + 1:]:
                    back = [x for x in later.popped if x in s.pushed]
                    if later.accepted and back:
                        # last pushed, first popped: not the ascending order the stack gives after init
                        assert back == [x for x in s.pushed[::-1] if x in back] and back != sorted(back)
                        return True
        return False

    assert any(pops_what_was_pushed(chain) for chain in wide.log), "no accepted 32 -> 1 swap whose slots a later swap pops"
    for traj in (wide, tight):
        assert all(len(a) > 512 for a in traj.init_active), [len(a) for a in traj.init_active]
    for a in odd.init_active:  # the unreached leaves of the initial forest sit between active slots
        assert len(set(range(int(a.max()))) - set(a.tolist())) > 0, "odd67: no empty-plane slot below an active one"
    # m64_tight: the capacity is the worst case of the sweep over the accept masks exactly, odd, above the workgroup's 512
    # threads, and one chain really uses all of it
    case = lc.CASES["m64_tight"]
    peak = [k if isinstance(k, int) else k[1] for k in case.init]
    for step in case.steps:
        peak[step[0]] = max(peak[step[0]], step[2])
    assert sum(peak) == case.capacity and case.capacity % 2 == 1 and case.capacity > 512
    assert any(s.free_after == 0 for chain in tight.log for s in chain), "m64_tight never runs the free stack empty"
    assert lc.CASES["m64_cap1024"].capacity == 1024 and lc.CASES["odd67"].capacity % 8 != 0


def test_tight_capacity_is_the_table_builders_bound(L):
    """The library's table builder takes m64_tight at its capacity and refuses it with one slot less."""
    case = lc.CASES["m64_tight"]
    nleaves = np.tile(np.array([k if isinstance(k, int) else k[1] for k in case.init]), (case.nc, 1))
    r_new = np.tile(np.array([s[2] for s in case.steps])[:, None], (1, case.nc))
    tidx = [s[0] for s in case.steps]
    assert build_table(L, tidx, r_new, nleaves, case.lcap, case.capacity, stride=63)[0] == 0
    rc, _, msg = build_table(L, tidx, r_new, nleaves, case.lcap, case.capacity - 1, stride=63)
    assert rc == L.BARK_ERR_ARG and "capacity" in msg


def test_g11_trajectory_passes_the_precheck():
    """The reference sampler's recorded steps (g11: N = 48, 2 chains, 3 steps of 8 trees + a noise / scale proposal) are a GPU
    case: float64 and longdouble take the recorded decisions with a margin far above 1e-6 and reproduce the recorded MLL."""
    from conftest import load_golden

    g = load_golden("g11_sampler_steps")
    f64, ext = lc.g11_replay(np.float64), lc.g11_replay(np.longdouble)
    for r in (f64, ext):
        assert np.array_equal(r.accept, g["accept"]) and np.array_equal(r.ns_accept, g["ns_accept"])
        assert min(r.tree_margin, r.ns_margin) >= lc.MARGIN
        assert np.allclose(r.mll, g["cur_mll"], rtol=1e-9, atol=1e-8) and np.allclose(r.mll_after, g["mll_after"], rtol=1e-9, atol=1e-8)
    assert g["start_noise"].min() >= 1e-2 and g["noise_after"].min() >= 1e-2
    assert lr.used(f64.mll, ext.mll, lr.SCALAR_RTOL, lr.SCALAR_ATOL) <= 0.01
    print("g11 margins: trees %.3g, noise/scale %.3g" % (f64.tree_margin, f64.ns_margin))


def test_unsymmetrised_rewrite_drifts():
    """Why the rewrite gives (i, j) and (j, i) one expression: kept as the formulas give it, P leaves the matrix bar at N = 64
    within a handful of accepted steps, while the symmetrised rewrite stays inside 10 % of it."""
    from bark_amd import synthetic

    X, y, _, ft = synthetic.unit_cube_problem(64, lc.D, seed=64)
    m, cap = 10, 96
    forest = np.stack([lr.caterpillar_tree(2 + t % 4, t % lc.D) for t in range(m)])
    worst = {}
    for symmetric in (True, False):
        ch = lc.RefChain(forest, 0.1, 1.0, X, y, ft, cap, np.float64, symmetric)
        ext = lc.RefChain(forest, 0.1, 1.0, X, y, ft, cap, np.longdouble, True)
        used = 0.0
        for k in range(12):  # every proposal is taken: twelve accepted steps
            new = lr.caterpillar_tree(2 + (3 * k + 1) % 5, (k + 1) % lc.D)
            for c in (ch, ext):
                c.propose(k % m, new)[1]()
            used = max(used, lr.used(ch.export()[0], ext.export()[0], lr.MAT_RTOL, lr.MAT_ATOL))
        worst[symmetric] = used
    print("fraction of the matrix bar used:", worst)
    assert worst[True] <= 0.1 and worst[False] > 1.0


# ------------------------------------------------------------------------- host code of the library ----
@pytest.fixture(scope="module")
def L():
    from bark_amd import _lib

    _lib.lib()
    return _lib


def test_query_limits(L):
    from bark_amd.fitting import leafchain_plan

    plan = leafchain_plan(4096, 256, 50, 32, nc=64, d=10)
    assert plan["reason"] == "" and plan["plane_words"] == 64 and plan["workgroups"] == 64 and plan["threads"] <= 512
    assert (plan["max_chains"], plan["max_trees"], plan["max_leaves"], plan["max_slots"]) == (64, 64, 32, 1024)
    assert plan["state_bytes"] == 64 * plan["chain_bytes"] and plan["chain_bytes"] < 1 << 20  # ~0.5 MB + planes, whatever N^2 is
    assert plan["chain_bytes"] >= 8 * 256 * 256 + 256 * 64 * 8
    assert L.lib().bark_leafchain_bytes(4096, 256, 50, 32, 64) == plan["state_bytes"]
    assert L.lib().bark_leafchain_workspace_bytes(4096, 256, 50, 32, 64) == plan["workspace_bytes"]
    big = leafchain_plan(16384, 256, 50, 32, nc=64)
    assert big["reason"] == "" and big["chain_bytes"] < 2 << 20
    for kw, word in ((dict(nc=65), "chains"), (dict(nc=0), "chains"), (dict(m=65), "trees"), (dict(lcap=33), "leaves"),
                     (dict(capacity=1025), "slots"), (dict(capacity=0), "slots"), (dict(N=0), "N =")):
        args = dict(N=128, capacity=64, m=4, lcap=8, nc=2)
        args.update(kw)
        plan = leafchain_plan(args["N"], args["capacity"], args["m"], args["lcap"], nc=args["nc"])
        assert word in plan["reason"] and plan["state_bytes"] == 0, (kw, plan)
        assert L.lib().bark_leafchain_bytes(args["N"], args["capacity"], args["m"], args["lcap"], args["nc"]) == 0
    assert leafchain_plan(128, 64, 4, 8)["reason"] == "" and L.lib().bark_last_error() == b""


def build_table(L, tree_index, r_new, nleaves, lcap, cap, stride=3, offsets=None):
    steps, nc = r_new.shape
    m = nleaves.shape[1]
    infos = (L.PackInfo * steps)()
    for t in range(steps):
        infos[t].B, infos[t].m, infos[t].L, infos[t].stride = nc, 1, 100, stride
        infos[t].max_leaves = infos[t].max_bits = int(r_new[t].max())
        infos[t].max_depth, infos[t].packed_bytes = 4, nc * stride * 16
    offsets = np.arange(steps, dtype=np.int64) * 256 if offsets is None else offsets
    table = np.full(int(L.lib().bark_leafchain_sweep_table_bytes(steps, nc)) // 8, -7, dtype=np.int64)
    rc = L.lib().bark_leafchain_sweep_table(L.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), L.ptr(np.ascontiguousarray(tree_index, dtype=np.int64)),
                                            L.ptr(np.ascontiguousarray(r_new, dtype=np.int64)), L.ptr(np.ascontiguousarray(nleaves, dtype=np.int32)),
                                            steps, nc, m, lcap, cap, L.ptr(table))
    return rc, table, L.lib().bark_last_error().decode()


def test_table_builder_validates(L):
    nleaves = np.array([[2, 3], [1, 4]])
    r_new = np.array([[4, 2], [3, 4], [1, 1]])
    rc, table, _ = build_table(L, [0, 1, 0], r_new, nleaves, 4, 8)
    assert rc == 0
    assert table[:12].reshape(3, 4).tolist() == [[0, 3, 4, 0], [256, 3, 4, 1], [512, 3, 4, 0]]
    assert np.array_equal(table[12:].reshape(3, 2), r_new)
    # the worst case of chain 0 is 4 + 3 = 7 slots, of chain 1 it is 2 + 4 = 6: capacity 7 is exact, 6 is one leaf short
    assert build_table(L, [0, 1, 0], r_new, nleaves, 4, 7)[0] == 0
    rc, _, msg = build_table(L, [0, 1, 0], r_new, nleaves, 4, 6)
    assert rc == L.BARK_ERR_ARG and "capacity" in msg
    rc, _, msg = build_table(L, [0, 1, 0], r_new, nleaves, 3, 8)  # r_new = lcap + 1
    assert rc == L.BARK_ERR_ARG and "leaves" in msg
    assert build_table(L, [0, 2, 0], r_new, nleaves, 4, 8)[0] == L.BARK_ERR_ARG  # tree index past m
    assert build_table(L, [0, -1, 0], r_new, nleaves, 4, 8)[0] == L.BARK_ERR_ARG
    assert build_table(L, [0, 1, 0], r_new, nleaves, 4, 8, stride=65)[0] == L.BARK_ERR_ARG  # more nodes than the walk's LDS holds
    assert build_table(L, [0, 1, 0], r_new, nleaves, 4, 8, offsets=np.array([0, 8, 512]))[0] == L.BARK_ERR_ARG
    assert build_table(L, [0, 1, 0], np.array([[4, 2], [3, 0], [1, 1]]), nleaves, 4, 8)[0] == L.BARK_ERR_ARG
    assert L.lib().bark_leafchain_sweep_table_bytes(3, 65) == 0
    assert build_table(L, [0, 1, 0], r_new, nleaves, 4, 8)[0] == 0  # and leave no message behind for whoever asks next
