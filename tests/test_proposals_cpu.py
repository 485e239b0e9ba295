"""CPU tests of the tree proposals: the host restatement (tests/proposals_ref.py) against the reference's own functions
(tests/golden/g12_tree_proposals), the Philox stream against the published known answers, the statuses, the library's limit
checks (pure host) and the noise / scale proposal of bark_amd.fitting.noise_scale_proposals.  No GPU."""
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
