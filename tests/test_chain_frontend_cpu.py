"""The host-side steps the sampler's chain containers share (bark_amd/fitting/_chains.py): leaf counts, the packing of a
sweep's steps into one buffer, and the input checks with the message texts the three classes have always raised.  The library
loads and packs on the CPU; nothing here touches a GPU."""
import ctypes
import re

import numpy as np
import pytest

from bark_amd import _lib, synthetic
from bark_amd.fitting import _chains
from bark_amd.forest import NODE_RECORD_DTYPE

from leafspace_ref import host_pack

L = 100
FT = np.full(4, 2, dtype=np.int64)


def caterpillar(leaves, feature):
    """A tree of exactly `leaves` leaves (2 * leaves - 1 nodes): node 2k splits `feature`, left child a leaf, right the next split."""
    tree = np.zeros(L, dtype=NODE_RECORD_DTYPE)
    node, parent, depth = 0, 0xFFFFFFFF, 0
    for k in range(leaves - 1):
        left, right = 2 * k + 1, 2 * k + 2
        tree[node] = (0, feature, (k + 1) / leaves, left, right, parent, depth, 1)
        tree[left] = (1, 0, 0, 0, 0, node, depth + 1, 1)
        node, parent, depth = right, node, depth + 1
    tree[node] = (1, 0, 0, 0, 0, parent, depth, 1)
    return tree


def max_bits(tree, ft):
    info = _lib.PackInfo()
    _lib.check(_lib.lib().bark_forest_pack_info(_lib.ptr(np.ascontiguousarray(tree)), 1, 1, tree.shape[0], _lib.ptr(ft), ft.shape[0],
                                                ctypes.byref(info)))
    return int(info.max_bits)


def test_leaf_counts_are_the_packers_per_tree():
    X, y, bounds, ft = synthetic.mixed_problem(16, 3)
    F = synthetic.sample_prior_forests(3, 4, bounds, ft, seed=11)
    assert F.shape[:2] == (3, 4)
    got = _chains.leaf_counts(F, ft)
    assert got.shape == (3, 4) and got.dtype == np.int64
    for b in range(3):
        for t in range(4):
            assert got[b, t] == max_bits(F[b, t], ft)
    assert got.max() > 1  # not all stumps
    # a view in another order counts the same trees
    assert np.array_equal(_chains.leaf_counts(np.swapaxes(F, 0, 1), ft), got.T)
    # an active leaf record that no split points to is not a leaf of the tree
    stray = caterpillar(3, 0)
    stray[9] = (1, 0, 0, 0, 0, 0, 1, 1)
    one = _chains.leaf_counts(stray, FT)
    assert one.shape == () and int(one) == max_bits(stray, FT) == 3
    assert _chains.leaf_counts(np.stack([stray, caterpillar(17, 1)]), FT).tolist() == [3, 17]


# 3 chains; the old trees of the five steps have 1, 5, 17, 2 and 5 leaves, i.e. 1, 9, 33, 3 and 9 packed nodes of 16 bytes
STEP_LEAVES = (1, 5, 17, 2, 5)
NEW_LEAVES = (1, 3, 9, 2, 4)  # never more than the old tree: the old tree sets the step's stride
# k = 1: 48, 432, 1584, 144, 432 bytes -> rounded up to 256: 256, 512, 1792, 256;  k = 2: 96, 864, 3168, 288, 864 -> 256, 1024, 3328, 512
WANT = {1: ([48, 432, 1584, 144, 432], [0, 256, 768, 2560, 2816]), 2: ([96, 864, 3168, 288, 864], [0, 256, 1280, 4608, 5120])}


@pytest.mark.parametrize("k", [1, 2])
def test_pack_steps_host_offsets_and_bytes(k):
    old = [np.stack([caterpillar(n, b % 4) for b in range(3)]) for n in STEP_LEAVES]  # per step (chains, L)
    new = [np.stack([caterpillar(n, (b + 1) % 4) for b in range(3)]) for n in NEW_LEAVES]
    forests = [o[:, None] for o in old] if k == 1 else [np.stack([o, n], axis=1) for o, n in zip(old, new)]
    infos, offsets, sizes, host = _chains.pack_steps_host(forests, FT)
    want_sizes, want_offsets = WANT[k]
    assert sizes == want_sizes and [int(i.packed_bytes) for i in infos] == want_sizes
    if k == 1:  # two sizes pad differently (for k = 2 every size is 96 mod 256; they still round to different multiples)
        assert len({-s % 256 for s in sizes}) >= 2
    assert offsets.dtype == np.int64 and offsets.flags.c_contiguous and offsets.tolist() == want_offsets
    assert host.dtype == np.uint8 and host.shape == (want_offsets[-1] + want_sizes[-1],)
    for t, f in enumerate(forests):
        info, packed = host_pack(f, FT)
        assert (info.B, info.m, info.max_bits) == (3, k, infos[t].max_bits)
        assert np.array_equal(host[want_offsets[t]:want_offsets[t] + want_sizes[t]], packed.reshape(-1).view(np.uint8)), t


def test_steps_major_and_per_chain_vectors():
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    got = _chains.steps_major(a, 2, 3)
    assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, a.T)
    assert np.array_equal(_chains.steps_major(list(range(6)), 2, 3), a.T)  # anything of chains * steps values
    with pytest.raises(ValueError):
        _chains.steps_major(np.zeros(5), 2, 3)
    v = _chains.per_chain("log_u", np.arange(6.0)[::2], 3)
    assert v.dtype == np.float64 and v.flags.c_contiguous and v.tolist() == [0.0, 2.0, 4.0]
    assert _chains.per_chain("new_noise", [[1], [2], [3]], 3).shape == (3,)
    for name in ("new_noise", "new_scale", "log_q_prior", "log_u"):
        with pytest.raises(ValueError, match=f"^{name} has 2 entries for 3 chains$"):
            _chains.per_chain(name, [0.1, 0.2], 3)
    vecs = _chains.noise_scale_vectors([1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], 3)
    assert [x.tolist() for x in vecs] == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0], [10.0, 11.0, 12.0]]
    with pytest.raises(ValueError, match="^new_scale has 1 entries for 3 chains$"):  # the first bad one, in the entry points' order
        _chains.noise_scale_vectors([1, 2, 3], 4.0, [7, 8], [10, 11, 12], 3)


def test_broadcast_scale():
    s = _chains.broadcast_scale(2, 3)
    assert s.dtype == np.float64 and s.shape == (3,) and s.tolist() == [2.0, 2.0, 2.0]
    assert _chains.broadcast_scale(np.array([[1.0], [2.0], [3.0]], dtype=np.float32), 3).tolist() == [1.0, 2.0, 3.0]
    assert np.array_equal(np.sqrt(_chains.broadcast_scale([1.0, 4.0], 2) / 4), [0.5, 1.0])
    with pytest.raises(ValueError):
        _chains.broadcast_scale([1.0, 2.0], 3)


def test_check_step_trees():
    trees = np.stack([np.stack([caterpillar(2 + t, b) for t in range(4)]) for b in range(3)])  # (3, 4, L)
    view = trees[:, ::2]
    old, new = _chains.check_step_trees(view, view.copy(), 3)
    assert old.shape == new.shape == (3, 2, L) and old.dtype == NODE_RECORD_DTYPE
    assert old.flags.c_contiguous and new.flags.c_contiguous and np.array_equal(old, view)
    message = "^" + re.escape("trees must be (chains, steps, node_limit) records, got (3, 4, 100) and (3, 2, 100)") + "$"
    with pytest.raises(ValueError, match=message):
        _chains.check_step_trees(trees, view, 3)
    with pytest.raises(ValueError, match=re.escape("records, got (3, 4, 100) and (3, 4, 100)")):  # another batch's chains
        _chains.check_step_trees(trees, trees, 2)
    with pytest.raises(ValueError, match=re.escape("records, got (1, 3, 4, 100) and (1, 3, 4, 100)")):
        _chains.check_step_trees(trees[None], trees[None], 1)
    with pytest.raises(ValueError, match="nodes must have at least 3 dims"):
        _chains.check_step_trees(trees[0], trees[0], 3)
    with pytest.raises(TypeError, match="nodes must use NODE_RECORD_DTYPE"):
        _chains.check_step_trees(np.zeros((3, 4, L)), trees, 3)


class Owner:
    N = 4

    def __init__(self, X, Xd):
        self._X_seen = (X, Xd)


def test_points_cache_checks_rows_with_the_owners_noun():
    X, Xd = np.zeros((4, 2)), np.ones((4, 2))  # Xd stands for the device copy made when X was first seen
    owner = Owner(X, Xd)
    assert _chains.points_of(owner, X, FT[:2], "chains have") is Xd and owner._X_seen[0] is X
    short = Owner(X, np.ones((5, 2)))
    with pytest.raises(ValueError, match="^X has 5 rows, the chain has 4 points$"):
        _chains.points_of(short, X, FT[:2], "chain has")
    with pytest.raises(ValueError, match="^X has 5 rows, the chains have 4 points$"):
        _chains.points_of(short, X, FT[:2], "chains have")


def test_read_decisions_returns_host_copies():
    import torch

    accept = torch.tensor([[1, 0, -1], [0, 1, 1]], dtype=torch.int32)
    state = torch.tensor([[1.5, -2.0], [2.5, -3.0], [3.5, -4.0]], dtype=torch.float64)
    acc, quad, logdet = _chains.read_decisions(accept, state)
    assert acc.dtype == np.int32 and acc.tolist() == [[1, 0, -1], [0, 1, 1]]
    assert quad.tolist() == [1.5, 2.5, 3.5] and logdet.tolist() == [-2.0, -3.0, -4.0]
    state.zero_()  # the device goes on writing the state: the batch's mirrors must not alias it
    assert quad.tolist() == [1.5, 2.5, 3.5] and quad.flags.c_contiguous and logdet.flags.c_contiguous
