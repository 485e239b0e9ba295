"""Tree proposals on the device — bark_amd.fitting.tree_proposals, csrc/propose.hip — against the host restatement
(tests/proposals_ref.py, which tests/test_proposals_cpu.py holds to the reference's own functions).

Structure (new_nodes, detail) must match bit for bit.  The two logs may differ by 8 * 2^-52 * sum|terms|: log_q_prior is a sum of
at most five log / pow terms, each good to about an ulp in the device library and half an ulp in numpy, plus the roundings of
the sum; log_u is one log.  The largest multiple of 2^-52 * sum|terms| seen is printed (DESIGN.md section 9 records it).

Cases (proposals_ref.CASES): (nc, m, L, d) = (3, 5, 100, 4) mixed features with max_leaves in reach, (1, 1, 100, 1), (64, 64,
100, 4) — 4 096 waves, several rounds of the CUs — and (2, 3, 7, 4), containers that overflow."""
import numpy as np
import pytest

import proposals_ref as pr

pytestmark = pytest.mark.gpu

SEED, SWEEP = 0x5EED0123456789, 17
BAR = 8 * 2.0 ** -52
_REF = {}


def ref(name):
    """(forests, host proposals at (SEED, SWEEP)), computed once and shared."""
    if name not in _REF:
        c = pr.CASES[name]
        forests = c.forests()
        out = pr.propose_forests(forests, c.bounds, c.ft, c.params, SEED, SWEEP)
        for a in (forests,) + out:
            a.setflags(write=False)
        _REF[name] = (forests, out)
    return _REF[name]


@pytest.fixture(scope="module")
def G():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd.fitting import tree_proposals as tp

    class NS:
        pass

    ns = NS()
    ns.torch, ns.tp = torch, tp
    return ns


def device(G, name, forests=None, **kw):
    c = pr.CASES[name]
    forests = ref(name)[0] if forests is None else forests
    kw.setdefault("seed", SEED)
    kw.setdefault("sweep", SWEEP)
    if isinstance(forests, np.ndarray):
        forests = np.array(forests).view(G.tp.NODE_RECORD_DTYPE)  # a writable copy: the shared reference stays read-only
    return G.tp.propose_trees(forests, c.bounds, c.ft, c.params, max_leaves=c.params.max_leaves, **kw)


def compare(got, want):
    """Bit identity of the structure and the bar on the logs -> the largest multiple of 2^-52 * sum|terms| used."""
    new, lq, lu, detail = got
    wnew, wlq, wlu, wdetail, wsum = want
    assert np.array_equal(detail, wdetail)
    assert new.tobytes() == wnew.tobytes()
    fin = np.isfinite(wlq)
    assert np.array_equal(lq[~fin], wlq[~fin])  # -inf where the host says so
    worst = 0.0
    if fin.any():
        err = np.abs(lq[fin] - wlq[fin])
        assert (err <= BAR * wsum[fin]).all(), float((err / np.maximum(wsum[fin], 1e-300)).max() / 2.0 ** -52)
        nz = wsum[fin] > 0
        worst = float((err[nz] / wsum[fin][nz]).max() / 2.0 ** -52) if nz.any() else 0.0
        assert (err[~nz] == 0).all()  # a change: exactly 0
    ufin = np.isfinite(wlu)
    err_u = np.abs(lu[ufin] - wlu[ufin])
    assert (err_u <= BAR * np.abs(wlu[ufin])).all() and np.array_equal(lu[~ufin], wlu[~ufin])
    worst_u = float((err_u / np.maximum(np.abs(wlu[ufin]), 1e-300)).max() / 2.0 ** -52)
    return worst, worst_u


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_cases(G, name):
    forests, want = ref(name)
    got = device(G, name)
    worst = compare(got, want)
    status = np.bincount(want[3][..., 3].ravel(), minlength=5)
    print(name, "statuses", status.tolist(), "largest multiples of 2^-52 sum|terms|: log_q_prior %.3g, log_u %.3g" % worst)
    assert got[0].shape == forests.shape and got[1].shape == forests.shape[:2] and got[3].shape == forests.shape[:2] + (4,)
    if name == "overflow":
        assert status[3] > 0  # a full container: a rejected proposal, not an error
    if name == "mixed":
        assert status[4] > 0 or status[2] > 0
    if name == "wide":
        assert status[0] > 0 and status[1] > 0 and status[2] > 0 and set(want[3][..., 0].ravel()) == {0, 1, 2}


def test_grid_independence(G):
    """Chain 1 of the three-chain call = the one-chain call on that chain's forest at chain_offset 1; the same for one tree."""
    forests, _ = ref("mixed")
    whole = device(G, "mixed")
    one = device(G, "mixed", forests=forests[1:2], chain_offset=1)
    for a, b in zip(whole, one):
        assert a[1:2].tobytes() == b.tobytes()
    tree = device(G, "mixed", forests=forests[2:3, 3:4], chain_offset=2, tree_offset=3)
    for a, b in zip(whole, tree):
        assert a[2:3, 3:4].tobytes() == b.tobytes()
    other = device(G, "mixed", forests=forests[1:2])  # addressed as chain 0: another stream
    assert other[2].tobytes() != whole[2][1:2].tobytes()


def test_sweeps_and_seeds_differ_and_calls_repeat(G):
    a, b = device(G, "mixed"), device(G, "mixed")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c, d = device(G, "mixed", sweep=SWEEP + 1), device(G, "mixed", seed=SEED + 1)
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[2], d[2]) and not np.array_equal(c[2], d[2])
    assert not np.array_equal(a[3], c[3])
    # the host follows the address
    case = pr.CASES["mixed"]
    compare(c, pr.propose_forests(ref("mixed")[0], case.bounds, case.ft, case.params, SEED, SWEEP + 1))


def test_return_device_and_device_input(G):
    forests, want = ref("mixed")
    nodes_d = G.tp.records_to_device(np.array(forests).view(G.tp.NODE_RECORD_DTYPE))
    out = device(G, "mixed", forests=nodes_d, return_device=True)
    assert all(t.is_cuda for t in out) and out[0].dtype == G.torch.uint8 and out[0].shape == nodes_d.shape
    assert G.tp.records_from_device(out[0]).tobytes() == want[0].tobytes()
    assert G.tp.records_from_device(nodes_d).tobytes() == forests.tobytes()  # the input is not written


def test_commit_writes_exactly_the_accepted_trees(G):
    forests, want = ref("mixed")
    nc, m, L = forests.shape
    nodes_d = G.tp.records_to_device(np.array(forests).view(G.tp.NODE_RECORD_DTYPE))
    new_d = G.tp.records_to_device(np.array(want[0]).view(G.tp.NODE_RECORD_DTYPE))
    tree_index = np.array([0, 2, 2, 4, 1, 3, 1], dtype=np.int64)  # trees 2 and 1 twice
    rng = np.random.default_rng(3)
    accept = rng.choice(np.array([0, 1, -1], dtype=np.int32), size=(tree_index.shape[0], nc))
    accept[1, 0], accept[2, 0] = 0, 1    # a repeated tree taken by its second step only
    accept[4, 1], accept[6, 1] = -1, 0   # and one left alone by both
    assert {0, 1, -1} <= set(accept.ravel().tolist())
    G.tp.commit_trees_device(nodes_d, new_d, G.tp._lib.to_device(accept), G.tp._lib.to_device(tree_index))
    expect = forests.copy()
    for t, k in enumerate(tree_index):
        for c in range(nc):
            if accept[t, c] > 0:
                expect[c, k] = want[0][c, k]
    got = G.tp.records_from_device(nodes_d)
    assert got.tobytes() == expect.tobytes()
    assert expect.tobytes() != forests.tobytes() and expect.tobytes() != want[0].tobytes()
    assert G.tp.records_from_device(new_d).tobytes() == want[0].tobytes()


def test_refusals_come_before_any_launch(G):
    forests, _ = ref("overflow")
    case = pr.CASES["overflow"]
    rec = np.array(forests).view(G.tp.NODE_RECORD_DTYPE)
    with pytest.raises(ValueError, match="alpha"):
        G.tp.propose_trees(rec, case.bounds, case.ft, case.params._replace(alpha=1.0), seed=1, sweep=0)
    with pytest.raises(ValueError, match="weight"):
        G.tp.propose_trees(rec, case.bounds, case.ft, case.params._replace(proposal_weights=(0.0, 0.0, 0.0)), seed=1, sweep=0)
    with pytest.raises(ValueError, match="max_leaves"):
        G.tp.propose_trees(rec, case.bounds, case.ft, case.params, seed=1, sweep=0, max_leaves=8)
    with pytest.raises(ValueError, match="sweep"):
        G.tp.propose_trees(rec, case.bounds, case.ft, case.params, seed=1, sweep=-1)
    with pytest.raises(ValueError, match="slots"):
        G.tp.propose_trees(np.zeros((1, 1, 300), dtype=G.tp.NODE_RECORD_DTYPE), case.bounds, case.ft, case.params, seed=1, sweep=0)
    with pytest.raises(ValueError, match="bounds"):
        G.tp.propose_trees(rec, case.bounds[:3], case.ft, case.params, seed=1, sweep=0)
    nodes_d = G.tp.records_to_device(rec)
    with pytest.raises(ValueError, match="aliased"):
        G.tp.commit_trees_device(nodes_d, nodes_d, G.torch.zeros((1, 2), dtype=G.torch.int32, device="cuda"),
                                 G.torch.zeros(1, dtype=G.torch.int64, device="cuda"))
    G.torch.cuda.synchronize()  # nothing was launched that could have failed
    assert G.tp.records_from_device(nodes_d).tobytes() == forests.tobytes()
