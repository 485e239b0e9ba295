"""CPU tests of the tree proposals: the host restatement (tests/proposals_ref.py) against the reference's own functions
(tests/golden/g12_tree_proposals), the Philox stream against the published known answers, the statuses, the library's limit
checks (pure host), the noise / scale proposal of bark_amd.fitting.noise_scale_proposals, and the conditions under which the
edge cases of tests/test_gpu_proposals_edges.py mean something (restatement only).  No GPU."""
import ctypes
import types

import numpy as np
import pytest

import proposals_ref as pr
from bark_amd import _lib
from bark_amd.fitting import _philox, noise_scale_proposals as nsp, tree_proposals as tp
from conftest import load_golden

CHI2_999 = {2: 13.816, 3: 16.266}  # 99.9 % quantiles of the chi-squared law, by degrees of freedom
DIST_SEED = 2024                   # the distribution test's stream; the restatement passes at it (checked below)


@pytest.fixture(autouse=True)
def leave_no_error_behind():
    """The refusal tests end on a refused call; a query that succeeds clears the library's thread-local message again, which
    tests/test_host_cpu.py expects to find empty whatever ran before it."""
    yield
    assert tp.tree_proposals_plan(100, 4, 1, 1, 1)["reason"] == "" and _lib.lib().bark_last_error() == b""


@pytest.fixture(scope="module")
def g12():
    g = load_golden("g12_tree_proposals")
    g["trees"] = np.ascontiguousarray(g["trees"]).view(pr.NODE).reshape(g["trees"].shape[:-1])
    g["new_trees"] = np.ascontiguousarray(g["new_trees"]).view(pr.NODE).reshape(g["new_trees"].shape[:-1])
    return g


def test_apply_and_subspace_reproduce_the_reference(g12):
    params = pr.Params(max_leaves=100)
    kinds = set()
    for (k, kind, node, f), thr, want_q, want_p, want_new, want_sub in zip(g12["rows"], g12["thresholds"], g12["log_q"],
                                                                         g12["log_prior"], g12["new_trees"], g12["subspaces"]):
        tree = g12["trees"][k]
        assert np.array_equal(pr.subspace(tree, int(node), g12["bounds"], g12["feat_types"]), want_sub)
        got = pr.apply(tree, int(kind), int(node), int(f), float(thr), params)
        assert got.status == 0
        assert got.new_tree.tobytes() == want_new.tobytes(), (k, kind, node)
        for a, b in ((got.log_q, want_q), (got.log_prior, want_p)):
            assert abs(a - b) <= 1e-15 * abs(b), (k, kind, a, b)
        kinds.add(int(kind))
    assert kinds == {0, 1, 2} and len(g12["rows"]) > 100
    for tree, term, single in zip(g12["trees"], g12["terminal"], g12["singly_internal"]):
        assert pr.terminal(tree) == term[term >= 0].tolist() and pr.singly_internal(tree) == single[single >= 0].tolist()
    # some trees carry pruned records (inactive slots with stale fields)
    assert ((g12["trees"]["active"] == 0) & (g12["trees"]["depth"] > 0)).any()


def test_mask_spread_reproduces_the_reference(g12):
    for avail, draw, mask, upper in g12["masks"]:
        k = bin(int(avail)).count("1")
        if k < 2:
            assert mask == 0
            continue
        assert upper == (1 << k) - 1 and pr.spread_mask(int(avail), int(draw)) == mask
    # decide's draw covers exactly [1, 2^k - 2]: the reference's randint(1, 2^k - 1)
    tree = pr.root_tree(8)
    seen = {pr.decide([0.0, 0.0, 0.99, u, 0.5], tree, pr.MIXED_BOUNDS, pr.MIXED_FT, pr.Params()).threshold for u in np.linspace(0, 1 - 1e-12, 400)}
    assert seen == {float(v) for v in range(1, 31)}


def test_philox_known_answers():
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        assert pr.philox4x32(key, ctr) == want
        assert tuple(int(v) for v in _philox.philox4x32(key, ctr)) == want  # the product's host half (noise / scale draws)
    # the two host implementations address the stream alike
    u = _philox.uniforms(0x1234567890ABCDEF, [3, 4], [7, 0xFFFFFFFF], 9, 5)
    assert u[0].tolist() == pr.draws_of(0x1234567890ABCDEF, 9, 3, 7) and u[1].tolist() == pr.draws_of(0x1234567890ABCDEF, 9, 4, 0xFFFFFFFF)
    assert ((u >= 0) & (u < 1)).all()


def _split_root(feature, threshold, L=8):
    t = pr.root_tree(L)
    t[0] = (0, feature, threshold, 1, 2, 0xFFFFFFFF, 0, 1)
    t[1] = t[2] = (1, 0, 0, 0, 0, 0, 1, 1)
    return t


STATUS_CASES = {
    # name: (tree, draws (kind, node, feature, threshold, accept), params, status)
    "prune_of_a_root": (pr.root_tree(8), [0.3, 0.5, 0.5, 0.5, 0.5], pr.Params(), 1),
    "change_of_a_root": (pr.root_tree(8), [0.9, 0.5, 0.5, 0.5, 0.5], pr.Params(), 1),
    "one_category_left": (_split_root(3, 1.0), [0.1, 0.0, 0.99, 0.5, 0.5], pr.Params(), 2),     # left of {0}: one category remains
    "integer_interval_closed": (_split_root(2, 0.0), [0.1, 0.0, 0.6, 0.5, 0.5], pr.Params(), 2),  # left of x <= 0: [0, 0]
    "full_container": (pr.full_tree(7, 2, pr.MIXED_FT, pr.MIXED_BOUNDS, np.random.default_rng(0)), [0.1, 0.5, 0.1, 0.5, 0.5], pr.Params(), 3),
    "one_free_slot": (_split_root(0, 0.5, L=4), [0.1, 0.5, 0.1, 0.5, 0.5], pr.Params(), 3),
    "max_leaves": (_split_root(0, 0.5), [0.1, 0.5, 0.1, 0.5, 0.5], pr.Params(max_leaves=2), 4),
    "valid_grow": (_split_root(0, 0.5), [0.1, 0.5, 0.1, 0.5, 0.5], pr.Params(max_leaves=3), 0),
}


@pytest.mark.parametrize("name", sorted(STATUS_CASES))
def test_statuses(name, g12):
    tree, draws, params, status = STATUS_CASES[name]
    new, lq, lu, detail, _ = pr.propose(draws, tree, pr.MIXED_BOUNDS, pr.MIXED_FT, params)
    assert detail[3] == status
    if status:
        assert new.tobytes() == tree.tobytes() and lq == -np.inf
    else:
        assert np.isfinite(lq) and new.tobytes() != tree.tobytes()
    assert lu == np.log(draws[4])
    if name == "full_container":  # the reference raises OverflowError there (recorded in g12)
        assert g12["full_container_overflows"] == 1 and g12["full_container"].shape[0] == 7


def test_every_status_is_named():
    assert {c[3] for c in STATUS_CASES.values()} == {0, 1, 2, 3, 4}


def test_query_refuses_each_limit():
    ok = tp.tree_proposals_plan(100, 4, 32, 64, 50)
    assert ok["reason"] == "" and ok["workgroups"] == 800 and ok["threads"] == 256 and ok["nodes_bytes"] == 64 * 50 * 100 * 26
    assert (ok["max_slots"], ok["max_features"], ok["max_proposals"]) == (256, 1 << 20, 1 << 22)
    for args, word in (((0, 4, 1, 1, 1), "slots"), ((257, 4, 1, 1, 1), "slots"), ((100, 0, 1, 1, 1), "d ="),
                       ((100, (1 << 20) + 1, 1, 1, 1), "d ="), ((100, 4, 0, 1, 1), "max_leaves"), ((100, 4, 101, 1, 1), "max_leaves"),
                       ((100, 4, 1, 0, 1), "proposals"), ((100, 4, 1, 1, 0), "proposals"), ((100, 4, 1, 2048, 2049), "proposals")):
        plan = tp.tree_proposals_plan(*args)
        assert word in plan["reason"] and plan["nodes_bytes"] == 0 and plan["workgroups"] == 0, (args, plan)
    assert tp.tree_proposals_plan(256, 1 << 20, 256, 2048, 2048)["reason"] == ""
    assert _lib.lib().bark_tree_proposals_query(100, 4, 1, 1, 1, None) == _lib.BARK_ERR_ARG


def _call(params, sweep=0, nc=1, m=1, L=8, d=4):
    """bark_tree_proposals_hip without a context: the checks of the arguments of its own come first."""
    lib = _lib.lib()
    rc = lib.bark_tree_proposals_hip(None, None, nc, m, L, None, None, d, ctypes.byref(params) if params is not None else None, 1, sweep,
                                     None, None, None, None, None)
    return rc, lib.bark_last_error().decode()


def test_entry_point_refuses_bad_parameters_before_anything_else():
    good = types.SimpleNamespace(alpha=0.95, beta=2.0, proposal_weights=(0.25, 0.25, 0.5))
    rc, msg = _call(tp.proposal_params(good, 4))
    assert rc == _lib.BARK_ERR_ARG and "bark_ctx" in msg  # all parameters pass: the null context is what is refused
    bad = [(dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(beta=-1.0), "beta"),
           (dict(proposal_weights=(0.5, -0.1, 0.6)), "weight"), (dict(proposal_weights=(0.0, 0.0, 0.0)), "weights sum"),
           (dict(proposal_weights=(float("inf"), 0.0, 0.0)), "weight")]
    for change, word in bad:
        rc, msg = _call(tp.proposal_params(types.SimpleNamespace(**{**vars(good), **change}), 4))
        assert rc == _lib.BARK_ERR_ARG and word in msg, (change, msg)
    for kwargs, word in ((dict(sweep=-1), "sweep"), (dict(sweep=1 << 32), "sweep"), (dict(L=300), "slots"), (dict(nc=0), "proposals")):
        rc, msg = _call(tp.proposal_params(good, 4), **kwargs)
        assert rc == _lib.BARK_ERR_ARG and word in msg, (kwargs, msg)
    rc, msg = _call(tp.proposal_params(good, 4, chain_offset=(1 << 32) - 1), nc=2)
    assert rc == _lib.BARK_ERR_ARG and "offsets" in msg
    assert _call(None)[0] == _lib.BARK_ERR_ARG
    assert _lib.lib().bark_tree_proposals_commit_hip(None, None, None, None, 1, 1, 1, 8, None) == _lib.BARK_ERR_ARG
    assert _lib.lib().bark_tree_proposals_commit_hip(None, None, None, None, 0, 1, 1, 8, None) == _lib.BARK_ERR_ARG
    with pytest.raises(ValueError, match="2\\^24"):
        tp.check_bounds([[0.0, 1.0], [0.0, 2.0 ** 25]], [2, 1])
    with pytest.raises(ValueError, match="bounds must be"):
        tp.check_bounds([[0.0, 1.0]], [2, 1])


def _chi2(counts, probs):
    n = counts.sum()
    return float((((counts - n * probs) ** 2) / (n * probs)).sum())


def test_decide_distribution():
    """4 096 proposals from one 3-leaf tree: kinds against (0.25, 0.25, 0.5), grow nodes against uniform over the 3 leaves,
    features against uniform over d, each below the 99.9 % quantile of its chi-squared law."""
    tree = _split_root(0, 0.5, L=100)
    tree[3] = tree[4] = (1, 0, 0, 0, 0, 1, 2, 1)
    tree[1] = (0, 1, 0.5, 3, 4, 0, 1, 1)
    assert pr.terminal(tree) == [2, 3, 4] and pr.singly_internal(tree) == [1]
    params = pr.Params()
    dec = [pr.decide(pr.draws_of(DIST_SEED, 0, c, t), tree, pr.MIXED_BOUNDS, pr.MIXED_FT, params) for c in range(64) for t in range(64)]
    kinds = np.bincount([x.kind for x in dec], minlength=3)
    stat_kind = _chi2(kinds, np.array([0.25, 0.25, 0.5]))
    grows = [x for x in dec if x.kind == pr.GROW]
    nodes = np.array([sum(x.node == n for x in grows) for n in (2, 3, 4)])
    stat_node = _chi2(nodes, np.full(3, 1 / 3))
    feats = np.bincount([x.feature for x in dec if x.kind != pr.PRUNE], minlength=4)
    stat_feat = _chi2(feats, np.full(4, 0.25))
    print("chi2: kinds %.3f (2 dof), grow nodes %.3f (2 dof), features %.3f (3 dof)" % (stat_kind, stat_node, stat_feat))
    assert stat_kind < CHI2_999[2] and stat_node < CHI2_999[2] and stat_feat < CHI2_999[3]
    assert all(x.node == 1 for x in dec if x.kind != pr.GROW)


def test_noise_scale_log_q_prior_reproduces_the_reference(g12):
    branches = set()
    for branch, softplus, sample_scale, noise, scale, z0, z1, new_noise, new_scale, want in g12["noise_scale"]:
        p = types.SimpleNamespace(use_softplus_transform=bool(softplus), sample_scale=bool(sample_scale), gamma_prior_shape=2.5,
                                  gamma_prior_rate=9.0)
        got = float(nsp.log_q_prior(noise, scale, new_noise, new_scale, p))
        assert abs(got - want) <= 1e-15 * abs(want), (branch, got, want)
        (nn, ns), lqp = nsp.get_noise_scale_proposal([noise], [scale], p, [[z0, z1]])
        assert nn[0] == new_noise and ns[0] == new_scale and abs(float(lqp[0]) - want) <= 1e-15 * abs(want)
        branches.add(int(branch))
    assert branches == {0, 1, 2}
    with pytest.raises(NotImplementedError):
        nsp.log_q_prior(0.1, 1.0, 0.2, 1.0, types.SimpleNamespace(use_softplus_transform=False, sample_scale=False))


def test_noise_scale_draws():
    z, lu = nsp.draw_normals(5, 3, 4)
    z2, lu2 = nsp.draw_normals(5, 3, 2, chain_offset=2)
    assert np.array_equal(z[2:], z2) and np.array_equal(lu[2:], lu2)  # a chain's draws do not depend on the batch
    assert not np.array_equal(z, nsp.draw_normals(5, 4, 4)[0]) and not np.array_equal(z, nsp.draw_normals(6, 3, 4)[0])
    big, _ = nsp.draw_normals(1, 0, 4096)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1) < 0.05 and (lu <= 0).all()


def test_params_and_exports():
    import bark_amd.fitting as fit

    p = fit.BARKTrainParams()
    assert (p.warmup_steps, p.num_samples, p.steps_per_sample, p.use_softplus_transform, p.sample_scale) == (50, 5, 10, True, False)
    assert (p.gamma_prior_shape, p.gamma_prior_rate, p.alpha, p.beta, p.grow_prune_weight, p.change_weight) == (2.5, 9.0, 0.95, 2.0, 0.5, 1.0)
    assert (p.num_chains, p.verbose) == (1, False) and np.allclose(p.proposal_weights, [0.25, 0.25, 0.5])
    assert [e.value for e in fit.TreeProposalEnum] == [0, 1, 2] and [e.name for e in fit.TreeProposalEnum] == ["Grow", "Prune", "Change"]
    for name in ("run_bark_sampler", "propose_trees", "tree_proposals_plan", "noise_scale_proposals"):
        assert hasattr(fit, name)


# -------------------------------------------------------------------------------- edge cases ----
# The conditions that make tests/test_gpu_proposals_edges.py meaningful, asserted on the restatement's outputs alone: a badly
# chosen seed fails here, not silently on the device.
MOSTLY_REJECTED = ("idle_short", "tiny", "max_leaves_127", "ladders_stop")     # cases that are about a status other than 0


def _edge(name):
    forests, (new, lq, lu, detail, sa) = pr.edge_ref(name)
    c = pr.EDGE_CASES[name]
    return c, forests.reshape(-1, c.L), new.reshape(-1, c.L), detail.reshape(-1, 4), lq.reshape(-1)


def _words(nodes):
    return {int(n) // 64 for n in nodes if n >= 0}


def _interval(c, tree, d):
    return [float(v) for v in pr.subspace(tree, int(d[1]), c.bounds, c.ft)[int(d[2])]]


@pytest.mark.parametrize("name", sorted(pr.EDGE_CASES))
def test_edge_trees_are_trees_with_stale_slots_and_mostly_valid_proposals(name):
    c, trees, new, detail, lq = _edge(name)
    assert trees.shape[0] == c.nc * c.m <= 128
    for k, tree in enumerate(trees):
        if name == "guarded":
            assert pr.valid_tree(tree) == (k % c.m == c.m - 1)  # the last tree of every chain is a plain one
        elif name == "idle_pairs_odd":
            rest = tree.copy()
            rest["active"][pr.ORPHANS[k % c.m]] = 0
            assert not pr.valid_tree(tree) and pr.valid_tree(rest)
        else:
            assert pr.valid_tree(tree), (name, k)
        idle = tree[tree["active"] == 0]
        assert (idle["is_leaf"] <= 1).all() and all((idle[f] <= c.L).all() for f in ("left", "right", "parent"))
        if len(idle) >= 2:
            assert idle["depth"].any() and idle["feature_idx"].any()  # stale bits for the copy to keep
    # a rejected proposal copies the container unchanged; a grow or a prune changes it
    for tree, nt, d, q in zip(trees, new, detail, lq):
        assert (d[3] == 0) == np.isfinite(q)
        if d[3] != 0 or d[0] != pr.CHANGE:
            assert (nt.tobytes() == tree.tobytes()) == (d[3] != 0)
    share = float((detail[:, 3] != 0).mean())
    print(name, "statuses", np.bincount(detail[:, 3], minlength=5).tolist(), "share of status != 0: %.3f" % share)
    if not name.startswith(MOSTLY_REJECTED):
        assert share <= 0.5


def test_edge_cases_end_in_ragged_workgroups():
    assert sum((c.nc * c.m) % 4 != 0 for c in pr.EDGE_CASES.values()) >= 2  # four proposals per workgroup


def test_relabel_and_place():
    rng = np.random.default_rng(8)
    evolved = pr.evolved_forests(2, 3, 40, pr.MIXED_BOUNDS, pr.MIXED_FT, pr.Params(max_leaves=8), seed=3, sweeps=10).reshape(-1, 40)
    assert ((evolved["active"] == 0) & (evolved["depth"] > 0)).any()  # pruned records are there
    for tree in evolved:
        assert pr.valid_tree(tree)
        perm = np.concatenate([[0], 1 + rng.permutation(39)])
        moved = pr.relabel(tree, perm)
        assert pr.valid_tree(moved) and not pr.valid_tree(pr.relabel(tree, perm)[::-1])
        idle = np.flatnonzero(tree["active"] == 0)
        assert moved[perm[idle]].tobytes() == tree[idle].tobytes()                        # inactive records move unchanged
        assert pr.relabel(moved, np.argsort(perm)).tobytes() == tree.tobytes()
        assert sorted(pr.terminal(moved)) == sorted(perm[pr.terminal(tree)].tolist())
        assert sorted(pr.singly_internal(moved)) == sorted(perm[pr.singly_internal(tree)].tolist())
        n = int(tree["active"].sum())
        want = sorted(rng.choice(np.arange(1, 256), size=256 - n, replace=False).tolist())
        put = pr.place(tree, 256, want, rng)
        assert np.flatnonzero(put["active"] == 0).tolist() == want and pr.valid_tree(put)
        assert sorted(put["depth"][put["active"] == 1].tolist()) == sorted(tree["depth"][tree["active"] == 1].tolist())
    with pytest.raises(AssertionError):
        pr.place(pr.root_tree(8), 8, [1, 2, 3])  # 5 slots for one node
    # the cases' own inactive sets
    for name, sets in (("idle_pairs_255", pr.IDLE_PAIRS[255]), ("idle_pairs_256", pr.IDLE_PAIRS[256]), ("idle_short_one", [(200,)] * 3),
                       ("idle_short_none", [()] * 3), ("idle_pairs_odd", pr.IDLE_PAIRS_ODD)):
        c, trees, _, _, _ = _edge(name)
        for k, tree in enumerate(trees):
            assert np.flatnonzero(tree["active"] == 0).tolist() == list(sets[k % c.m]), (name, k)
    for name in pr.EDGE_CASES:
        if name.startswith("spread"):
            c, trees, _, _, _ = _edge(name)
            assert ((trees["active"] == 0).sum(axis=1) == (2 if c.L % 2 else 3)).all()
            assert len({t.tobytes() for t in trees}) == len(trees)


def test_caterpillar_has_one_singly_internal_node_where_asked():
    for L, depth, slot in ((65, 2, 64), (256, 60, 255), (70, 12, None), (3, 1, None)):
        t = pr.caterpillar(L, depth, 0, 0.5, [j % 2 for j in range(depth)], single_slot=slot)
        assert pr.valid_tree(t) and len(pr.terminal(t)) == depth + 1 and int(t["depth"].max()) == depth
        assert pr.singly_internal(t) == [2 * depth - 3 + (depth % 2) if slot is None and depth > 1 else (slot or 0)]


def test_spread256_reaches_every_word_with_every_kind():
    c, trees, new, detail, _ = _edge("spread256")
    ok = detail[detail[:, 3] == 0]
    assert set(ok[:, 0].tolist()) == {pr.GROW, pr.PRUNE, pr.CHANGE}
    assert _words(detail[detail[:, 0] == pr.GROW][:, 1]) == {0, 1, 2, 3} == _words(detail[detail[:, 0] != pr.GROW][:, 1])
    # grown children in different words, and singly internal nodes of the grown trees in word 3 (the recount's last ballot)
    grown = [(nt[d[1]]["left"] // 64, nt[d[1]]["right"] // 64) for nt, d in zip(new, detail) if d[0] == pr.GROW and d[3] == 0]
    assert any(a != b for a, b in grown)
    assert all(any(s >= 192 for s in pr.singly_internal(nt)) for nt, d in zip(new, detail) if d[0] == pr.GROW and d[3] == 0)


@pytest.mark.parametrize("L", [63, 64, 65, 128, 129, 192, 193, 255])
def test_spread_L_reaches_every_word_of_the_container(L):
    c, trees, new, detail, _ = _edge("spread_%d" % L)
    assert _words(detail[:, 1]) == set(range((L + 63) // 64))
    assert (trees["active"][:, L - 1] == 1).any()


def test_idle_pairs_are_taken_by_grows():
    for name, sets in (("idle_pairs_255", pr.IDLE_PAIRS[255]), ("idle_pairs_256", pr.IDLE_PAIRS[256]), ("idle_pairs_odd", pr.IDLE_PAIRS_ODD)):
        c, trees, new, detail, _ = _edge(name)
        taken = {}
        for k, (nt, d) in enumerate(zip(new, detail)):
            if d[0] == pr.GROW and d[3] == 0:
                assert (int(nt[d[1]]["left"]), int(nt[d[1]]["right"])) == tuple(sets[k % c.m][:2])
                taken[k % c.m] = taken.get(k % c.m, 0) + 1
        assert sorted(taken) == list(range(c.m)), (name, taken)
    pairs = [s[:2] for s in pr.IDLE_PAIRS[255] + pr.IDLE_PAIRS[256]] + pr.IDLE_PAIRS_ODD
    assert {(63, 64), (127, 128), (191, 192), (254, 255), (5, 255), (64, 65)} <= set(pairs)


def test_idle_short_grows_are_refused():
    for name in ("idle_short_one", "idle_short_none"):
        c, trees, new, detail, _ = _edge(name)
        grows = detail[detail[:, 0] == pr.GROW]
        assert len(grows) and set(grows[:, 3].tolist()) <= {2, 3} and (grows[:, 3] == 3).any()
        assert (detail[detail[:, 0] != pr.GROW][:, 3] != 3).all()


@pytest.mark.parametrize("L", [65, 129, 193, 256])
def test_last_slot_is_chosen(L):
    c, trees, new, detail, _ = _edge("last_single_%d" % L)
    other = detail[detail[:, 0] != pr.GROW]
    assert len(other) and (other[:, 1] == L - 1).all() and (other[:, 3] == 0).any()
    c, trees, new, detail, _ = _edge("last_leaf_%d" % L)
    grows = detail[(detail[:, 0] == pr.GROW) & (detail[:, 3] == 0)]
    assert (grows[:, 1] == L - 1).any() and (grows[:, 1] == L - 2).any()
    assert all(nt[L - 1]["left"] == 1 and nt[L - 1]["right"] == 2 for nt, d in zip(new, detail) if d[0] == pr.GROW and d[3] == 0 and d[1] == L - 1)


def test_tiny_containers():
    for L, want in ((1, {pr.GROW: {3}, pr.PRUNE: {1}, pr.CHANGE: {1}}), (2, {pr.GROW: {3}, pr.PRUNE: {1}, pr.CHANGE: {1}})):
        c, trees, new, detail, _ = _edge("tiny_%d" % L)
        assert {k: set(detail[detail[:, 0] == k][:, 3].tolist()) for k in want} == want
    c, trees, new, detail, _ = _edge("tiny_3")
    ok = [nt for nt, d in zip(new, detail) if d[0] == pr.GROW and d[3] == 0]
    assert ok and all(nt[0]["left"] == 1 and nt[0]["right"] == 2 and nt["active"].all() for nt in ok)
    assert {0, 1, 3} <= set(detail[:, 3].tolist())


def test_ladders_stop_and_open_where_they_should():
    causes = set()
    for name in ("ladders_stop", "ladders_stop_int", "ladders_stop_cat"):
        c, trees, new, detail, _ = _edge(name)
        for tree, d in zip(trees, detail):
            assert int(tree["depth"].max()) >= 12
            if d[3] == 2:
                lo, hi = _interval(c, tree, d)
                causes.add("lo == hi" if c.ft[d[2]] == pr.INT and lo == hi else "nbits < 2" if c.ft[d[2]] == pr.CAT and bin(int(hi)).count("1") < 2 else "?")
    assert causes == {"lo == hi", "nbits < 2"}
    seen = set()
    for name in ("ladders_open", "ladders_open_int", "ladders_open_cat", "ladders_open_cont"):
        c, trees, new, detail, _ = _edge(name)
        for tree, d in zip(trees, detail):
            if d[3] != 0 or d[0] == pr.PRUNE or d[1] == 0:
                continue
            lo, hi = _interval(c, tree, d)
            below = "left" if tree["left"][tree["parent"][d[1]]] == d[1] else "right"
            kind = int(c.ft[d[2]])
            full_lo, full_hi = c.bounds[d[2]]
            if kind == pr.CAT and hi != full_hi:
                seen.add("cat below " + below)
            elif kind != pr.CAT and lo > full_lo and hi < full_hi:
                seen.add(("int", "int", "cont")[kind] + " both")
    assert seen == {"cat below left", "cat below right", "int both", "cont both"}


def test_deep_prior_is_deep():
    c, trees, new, detail, _ = _edge("deep_prior")
    depth = np.array([t["depth"][d[1]] for t, d in zip(trees, detail) if d[3] == 0 and d[0] != pr.CHANGE])
    assert depth.max() >= 59 and ((trees["depth"] * trees["active"]).max(axis=1) == 60).all() and c.L == 256


def test_max_leaves_edge():
    _, trees, _, d127, _ = _edge("max_leaves_127")
    _, trees128, _, d128, _ = _edge("max_leaves_128")
    assert trees.tobytes() == trees128.tobytes() == _edge("spread256")[1].tobytes()
    grows = d127[:, 0] == pr.GROW
    assert grows.any() and set(d127[grows][:, 3].tolist()) <= {2, 4} and (d127[grows][:, 3] == 4).any()
    assert ((d128[:, 0] == pr.GROW) & (d128[:, 3] == 0)).any() and not (d128[:, 3] == 4).any()


def test_guarded_records_are_met():
    c, trees, new, detail, _ = _edge("guarded")
    L = c.L
    ends = set()
    for k, (tree, d) in enumerate(zip(trees, detail)):
        for f in ("left", "right"):
            assert (tree[f][tree["active"] == 1] <= L).all()
        assert (tree["parent"][np.flatnonzero(tree["active"])[1:]] <= L).all()
        outside = [i for i in np.flatnonzero(tree["active"] & (tree["is_leaf"] == 0)) if tree["left"][i] == L or tree["right"][i] == L]
        assert len(outside) == (1 if k % c.m < 2 else 0) and not set(outside) & set(pr.singly_internal(tree))
        if d[1] >= 0 and d[0] != pr.PRUNE:
            ends.add(pr.walk_end(tree, int(d[1])))
    assert ends == {"root", "outside", "cycle"}
