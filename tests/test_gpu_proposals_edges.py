"""Tree proposals on the device in every ballot word and at the edges of the container — csrc/propose.hip works through four
64-bit ballot words over up to 256 slots, and the cases of tests/test_gpu_proposals.py keep every node in the first.

proposals_ref.EDGE_CASES against the host restatement: trees spread over containers of 63 .. 256 slots, inactive pairs that
straddle the words, the last slot, containers of 1 .. 3 slots, 12-level ladders on one feature, depth 60, max_leaves at its
edge, and the records the kernel guards against.  tests/test_proposals_cpu.py asserts, on the restatement alone, that these
cases reach what they are meant to reach.  Structure (new_nodes, detail) must match bit for bit, stale fields of inactive
slots and pruned nodes included; the logs are held to the bar of tests/test_gpu_proposals.py, 8 * 2^-52 * sum|terms|.  The
largest multiple of 2^-52 * sum|terms| seen is printed per case (DESIGN.md section 9 records the maximum).

Three checks need no restatement: an order-preserving embedding of compact trees into 256 slots draws the same proposals, the
commit kernel copies whole containers of 1, 7, 64 and 256 slots and nothing else, and one chain of the widest case alone
gives the bits of the whole call."""
import numpy as np
import pytest

import proposals_ref as pr
from test_gpu_proposals import BAR, G, compare  # noqa: F401  G is the module's fixture

pytestmark = pytest.mark.gpu

assert BAR == 8 * 2.0 ** -52


def device(G, name, forests=None, **kw):
    c = pr.EDGE_CASES[name]
    forests = pr.edge_ref(name)[0] if forests is None else forests
    kw.setdefault("seed", pr.EDGE_SEED)
    kw.setdefault("sweep", pr.edge_sweep(name))
    rec = np.array(forests).view(G.tp.NODE_RECORD_DTYPE)  # a writable copy: the shared reference stays read-only
    return G.tp.propose_trees(rec, c.bounds, c.ft, c.params, max_leaves=c.params.max_leaves, **kw)


@pytest.mark.parametrize("name", sorted(pr.EDGE_CASES))
def test_edge_cases(G, name):
    forests, want = pr.edge_ref(name)
    got = device(G, name)
    assert got[0].shape == forests.shape and got[1].shape == forests.shape[:2] and got[3].shape == forests.shape[:2] + (4,)
    status = np.bincount(want[3][..., 3].ravel(), minlength=5)
    # the figures first, the verdict after: a case over the bar still reports by how much
    fin = np.isfinite(want[1]) & (want[4] > 0) & np.isfinite(got[1])
    seen = float((np.abs(got[1][fin] - want[1][fin]) / want[4][fin]).max() / 2.0 ** -52) if fin.any() else 0.0
    ufin = np.isfinite(want[2]) & np.isfinite(got[2]) & (want[2] != 0)
    seen_u = float((np.abs(got[2][ufin] - want[2][ufin]) / np.abs(want[2][ufin])).max() / 2.0 ** -52) if ufin.any() else 0.0
    print(name, "statuses", status.tolist(), "largest multiples of 2^-52 sum|terms|: log_q_prior %.3g, log_u %.3g" % (seen, seen_u))
    compare(got, want)


def _spread_map(tree):
    """Strictly increasing, slot 0 fixed: the slots a tree has ever used (active, or inactive with a record left behind), spread
    evenly over 0..255 — at most 100 of them, so the step is at least 2.5; -1 for the others."""
    used = np.flatnonzero((tree["active"] != 0) | (tree.view(np.uint8).reshape(len(tree), -1) != 0).any(axis=1))
    assert used[0] == 0 and 4 <= len(used) <= 100
    dest = np.full(len(tree), -1, dtype=np.int64)
    dest[used] = np.round(np.linspace(0, 255, len(used))).astype(np.int64)
    assert (np.diff(dest[used]) > 0).all()
    return dest


def test_order_preserving_embedding(G):
    """The same 15 trees in 100 slots and, under a strictly increasing slot map, in 256: the kernel picks by ascending slot order,
    so it must draw the same proposal on both, the node at the mapped slot.  No restatement involved."""
    params = pr.Params(proposal_weights=(0.4, 0.3, 0.3), max_leaves=32)
    compact = pr.evolved_forests(3, 5, 100, pr.MIXED_BOUNDS, pr.MIXED_FT, params, seed=14, sweeps=14)
    dests = [[_spread_map(t) for t in row] for row in compact]
    rng = np.random.default_rng(15)
    wide = np.stack([np.stack([pr.stale_fill(pr.move(t, d, 256), rng) for t, d in zip(row, drow)]) for row, drow in zip(compact, dests)])
    assert {int(s) // 64 for t in wide.reshape(-1, 256) for s in np.flatnonzero(t["active"])} == {0, 1, 2, 3}
    assert all(pr.valid_tree(t) for row in wide for t in row)
    kinds, words = set(), set()
    for sweep in (17, 18, 19, 20):  # 60 proposals on either side
        a, b = (G.tp.propose_trees(np.array(f).view(G.tp.NODE_RECORD_DTYPE), pr.MIXED_BOUNDS, pr.MIXED_FT, params, max_leaves=32,
                                   seed=pr.EDGE_SEED, sweep=sweep) for f in (compact, wide))
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()      # log_q_prior, log_u
        assert np.array_equal(a[3][..., [0, 2, 3]], b[3][..., [0, 2, 3]])                  # kind, feature, status
        for c in range(3):
            for t in range(5):
                dest, (kind, node, _, status) = dests[c][t], a[3][c, t]
                assert b[3][c, t, 1] == (dest[node] if node >= 0 else -1)
                small, big = a[0][c, t].view(pr.NODE).copy(), b[0][c, t].view(pr.NODE)
                grown = []
                if status == 0:
                    kinds.add(int(kind)), words.add(int(dest[node]) // 64)
                if status == 0 and kind == pr.GROW:
                    small["active"][[small["left"][node], small["right"][node]]] = 0  # the children: by content, not by slot
                    grown = [int(big["left"][dest[node]]), int(big["right"][dest[node]])]
                    assert grown == np.flatnonzero(wide[c, t]["active"] == 0)[:2].tolist()
                    for g in grown:
                        assert big[g].tolist() == (1, 0, 0.0, 0, 0, dest[node], small["depth"][node] + 1, 1)
                want = pr.move(small, dest, 256)
                if grown:
                    want["left"][dest[node]], want["right"][dest[node]] = grown
                live = np.flatnonzero(big["active"])
                assert sorted(live.tolist()) == sorted(np.flatnonzero(want["active"]).tolist() + grown)
                keep = np.setdiff1d(live, grown)
                assert big[keep].tobytes() == want[keep].tobytes()
    assert kinds == {pr.GROW, pr.PRUNE, pr.CHANGE} and words == {0, 1, 2, 3}


@pytest.mark.parametrize("L", [1, 7, 64, 256])
def test_commit_copies_whole_containers(G, L):
    """13 L halfwords against the copy's stride of 64; 7 steps x 3 chains; tree_index -1 and m copy nothing."""
    nc, m = 3, 5
    rng = np.random.default_rng(L)
    before = rng.integers(0, 256, (nc, m, 26 * L), dtype=np.uint8)
    new = rng.integers(0, 256, (nc, m, 26 * L), dtype=np.uint8)
    new[before == new] ^= 0xFF  # every byte differs: a byte left behind shows
    tree_index = np.array([0, -1, 2, m, 4, 2, 1], dtype=np.int64)
    accept = rng.choice(np.array([0, 1, -1], dtype=np.int32), size=(len(tree_index), nc))
    accept[1], accept[3] = 1, 1          # the steps that name no tree are accepted by every chain
    accept[2, 0], accept[5, 0] = 0, 1    # a repeated tree taken by its second step only
    accept[0, 1], accept[4, 2], accept[6, 1] = 1, 1, -1
    nodes_d, new_d = G.tp._lib.to_device(before), G.tp._lib.to_device(new)
    G.tp.commit_trees_device(nodes_d, new_d, G.tp._lib.to_device(accept), G.tp._lib.to_device(tree_index))
    expect, taken = before.copy(), 0
    for t, k in enumerate(tree_index):
        for c in range(nc):
            if accept[t, c] > 0 and 0 <= k < m:
                expect[c, k] = new[c, k]
                taken += 1
    got = nodes_d.cpu().numpy()
    assert taken >= 3 and not (expect == new).all(axis=2).all()
    for c in range(nc):
        for k in range(m):
            assert got[c, k].tobytes() == expect[c, k].tobytes(), (c, k)
    assert new_d.cpu().numpy().tobytes() == new.tobytes()


def test_grid_independence_at_the_edges(G):
    """Chain 5 of the eight chains of spread256, alone at chain_offset 5, gives the bits of the whole call."""
    forests, _ = pr.edge_ref("spread256")
    whole = device(G, "spread256")
    one = device(G, "spread256", forests=forests[5:6], chain_offset=5)
    for a, b in zip(whole, one):
        assert a[5:6].tobytes() == b.tobytes()
    assert {int(n) // 64 for n in one[3][0, :, 1] if n >= 0} == {0, 1, 2, 3}
    other = device(G, "spread256", forests=forests[5:6])  # addressed as chain 0: another stream
    assert other[2].tobytes() != whole[2][5:6].tobytes()
