"""Philox4x32-10 in numpy integers: the host half of the sampler's random stream (csrc/philox.h holds the device half).
Private.  key = (seed low word, seed high word), counter = (chain, tree, sweep, block); words (0, 1) and (2, 3) of a block are
one 64-bit draw each, low word first, and a uniform double is (x >> 11) * 2^-53."""

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

NOISE_SCALE_TREE = 0xFFFFFFFF  # the counter's tree word of the noise/scale half of a step: no tree has this index


def philox4x32(key, counter) -> np.ndarray:
    """key (2,) and counter (..., 4) of 32-bit words -> (..., 4) uint32."""
    c = np.array(counter, dtype=np.uint64) & _LOW
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LOW, n2, p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(seed: int, chain, tree, sweep: int, n_draws: int) -> np.ndarray:
    """The first n_draws uniform doubles of the streams (seed, sweep, chain[i], tree[i]) -> (len(chain), n_draws)."""
    chain = np.asarray(chain, dtype=np.uint64).reshape(-1)
    tree = np.broadcast_to(np.asarray(tree, dtype=np.uint64).reshape(-1), chain.shape)
    blocks = (n_draws + 1) // 2
    ctr = np.empty((chain.shape[0], blocks, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = chain[:, None], tree[:, None], np.uint64(sweep)
    ctr[..., 3] = np.arange(blocks, dtype=np.uint64)[None, :]
    words = philox4x32((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), ctr).astype(np.uint64).reshape(chain.shape[0], blocks * 2, 2)
    x = words[..., 0] | (words[..., 1] << _S32)
    return ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)[:, :n_draws]


PATH_KEY = 0x70617468  # "path": csrc/paths.hip xors it into the key's high word


def _keyed_normals(key_xor: int, seed: int, forest, draw, R: int) -> np.ndarray:
    """Box-Muller normals (len(forest), R): key = (seed low word, seed high word ^ key_xor), counter = (forest, draw, a // 2, 0)
    for entry a; with u1, u2 the block's two uniforms, r = sqrt(-2 log(1 - u1)) and th = 6.283185307179586 u2, the even entry
    is r cos th and the odd one r sin th."""
    forest = np.asarray(forest, dtype=np.uint64).reshape(-1)
    draw = np.broadcast_to(np.asarray(draw, dtype=np.uint64).reshape(-1), forest.shape)
    half = (int(R) + 1) // 2
    ctr = np.zeros((forest.shape[0], half, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1] = forest[:, None], draw[:, None]
    ctr[..., 2] = np.arange(half, dtype=np.uint64)[None, :]
    seed = int(seed) & (2 ** 64 - 1)
    words = philox4x32((seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ key_xor), ctr).astype(np.uint64)
    u1 = ((words[..., 0] | (words[..., 1] << _S32)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u2 = ((words[..., 2] | (words[..., 3] << _S32)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r, th = np.sqrt(-2.0 * np.log(1.0 - u1)), 6.283185307179586 * u2
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(forest.shape[0], 2 * half)[:, :int(R)]


def path_normals(seed: int, forest, draw, R: int) -> np.ndarray:
    """The standard normals of the sample paths (forest[i], draw[i]) -> (len(forest), R), as csrc/paths.hip draws them when
    no eps is given: key = (seed low word, seed high word ^ PATH_KEY), counter = (forest, draw, a // 2, 0) for entry a; with
    u1, u2 the block's two uniforms, r = sqrt(-2 log(1 - u1)) and th = 6.283185307179586 u2, the even entry is r cos th and
    the odd one r sin th.  A row depends on (seed, forest, draw) only."""
    return _keyed_normals(PATH_KEY, seed, forest, draw, R)


FANTASY_KEY = 0x66616E74  # "fant": acq_observe_kernel (csrc/acquire.hip) xors it into the key's high word


def fantasy_normals(seed: int, forest, draw, P: int) -> np.ndarray:
    """The standard normals of the sampled fantasies (forest[i], draw[i]) at P points -> (len(forest), P), as
    csrc/acquire.hip draws them when no eps is given: `path_normals` with FANTASY_KEY in place of PATH_KEY, entry p for
    point p of the call.  A row depends on (seed, forest, draw) only."""
    return _keyed_normals(FANTASY_KEY, seed, forest, draw, P)
