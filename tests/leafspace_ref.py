"""Float64 host reference of the leaf-space quantities (numpy and the oracle only, no GPU), and the case table of
tests/test_gpu_leafspace.py.  tests/test_leafspace_reference_cpu.py pins this reference to the oracle's N-space route
at every shape of the table.

Z is the (N, R) one-hot leaf matrix in the packer's bit order: the oracle's walk gives each point's leaf (node index)
per tree, and the packed leaf record of that leaf holds its bit.  With s2 = 1e-6 + noise, c = scale / (m s2),
M = I + c Z'Z = U'U (U upper triangular), V = U^-T, v = Z'y and w = M^-1 v (include/bark_hip.h):

    mll      = -0.5 [ (y'y - c v'w) / s2 + N log s2 + log|M| ]      (scale included, no 2 pi: bark_sampler.py's convention)
    mu       = c Z_C w
    var      = (scale / m) diag(Z_C M^-1 Z_C')
    K_s^-1   = (I - c Z M^-1 Z') / s2,   K_s^-1 y = (y - c Z w) / s2,   log|K_s| = N log s2 + log|M|
    f[s]     = c Z_C w + sqrt(scale / m) Z_C V' eps[s]

M = L L' with L = U' lower triangular, so V = L^-1 and M^-1 = V'V: every quantity is one Cholesky factorisation and
triangular solves.  The factor with a positive diagonal is unique, so for a given eps the draws are unique too.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from bark_amd import _lib, synthetic
from bark_amd.forest import create_empty_forest
from oracle import oracle as orc

LEAF, CAT, FEAT = 0x80000000, 0x40000000, 0x3FFFFFFF
NB = 128  # block size of the R x R sweep (chol_tiles.h)


# ------------------------------------------------------------------ the packer's wire format ----
def host_pack(nodes3, ft):
    lib = _lib.lib()
    info = _lib.PackInfo()
    B, m, L = nodes3.shape
    nodes3 = np.ascontiguousarray(nodes3)
    ft = np.ascontiguousarray(ft, dtype=np.int64)
    _lib.check(lib.bark_forest_pack_info(_lib.ptr(nodes3), B, m, L, _lib.ptr(ft), ft.shape[0], ctypes.byref(info)))
    packed = np.zeros(info.packed_bytes // 4, dtype=np.uint32)
    _lib.check(lib.bark_forest_pack(_lib.ptr(nodes3), _lib.ptr(ft), ft.shape[0], ctypes.byref(info), _lib.ptr(packed)))
    return info, packed.reshape(B, m, info.stride, 4)


def walk_packed(packed_tree, x, max_depth):
    """numpy emulation of the device walk (traverse.hip) on the wire format."""
    n = packed_tree[0]
    for _ in range(max_depth):
        if n[0] & LEAF:
            break
        f = int(n[0] & FEAT)
        if n[0] & CAT:
            xt = np.trunc(x[f])
            left = bool((int(n[1]) >> int(xt)) & 1) if 0 <= xt < 32 else False
        else:
            left = x[f] <= float(np.uint32(n[1]).view(np.float32))
        n = packed_tree[int(n[2] if left else n[3])]
    assert n[0] & LEAF
    return int(n[1]), int(n[0] & 0xFF), int(n[2])


def leaf_bit_table(packed, node_limit, max_depth):
    """(B, m, node_limit) int64: the bit of (forest, tree, original leaf index), read from the packed leaf records that
    the walk can reach from the root (word 1: original index, word 2: bit; the records behind a tree's own are padding);
    -1 for nodes that are no reachable leaf."""
    B, m, stride = packed.shape[:3]
    leaf = (packed[..., 0] & LEAF) != 0
    reach = np.zeros((B, m, stride), dtype=bool)
    reach[:, :, 0] = True
    for _ in range(max_depth):  # split records pass the walk on to both children (words 2 and 3)
        b, t, r = np.nonzero(reach & ~leaf)
        reach[b, t, packed[b, t, r, 2].astype(np.int64)] = True
        reach[b, t, packed[b, t, r, 3].astype(np.int64)] = True
    table = np.full((B, m, node_limit), -1, dtype=np.int64)
    b, t, r = np.nonzero(reach & leaf)
    table[b, t, packed[b, t, r, 1].astype(np.int64)] = packed[b, t, r, 2]
    return table


def leaf_matrix(nodes2, bits, X, ft, R):
    """(N, R) one-hot leaf matrix of one forest: row x has a 1 in column bits[t, leaf_t(x)] for every tree t."""
    leaves = orc.pass_through_forest(nodes2, X, ft).astype(np.int64)  # (N, m) node indices
    cols = bits[np.arange(nodes2.shape[0])[None, :], leaves]
    assert (cols >= 0).all() and (cols < R).all()
    Z = np.zeros((X.shape[0], R))
    Z[np.arange(X.shape[0])[:, None], cols] = 1.0
    return Z


# ------------------------------------------------------------------ the reference arithmetic ----
def solve_lower(L, B, trans=False):
    """L x = B (trans: L' x = B) for lower-triangular L: blocked substitution, numpy only."""
    n, nb = L.shape[0], 256
    X = np.array(B, dtype=np.float64, copy=True)
    if not trans:
        for i0 in range(0, n, nb):
            i1 = min(n, i0 + nb)
            if i0:
                X[i0:i1] -= L[i0:i1, :i0] @ X[:i0]
            X[i0:i1] = np.linalg.solve(L[i0:i1, i0:i1], X[i0:i1])
    else:
        for i1 in range(n, 0, -nb):
            i0 = max(0, i1 - nb)
            if i1 < n:
                X[i0:i1] -= L[i1:, i0:i1].T @ X[i1:]
            X[i0:i1] = np.linalg.solve(L[i0:i1, i0:i1].T, X[i0:i1])
    return X


class LeafRef:
    """The leaf-space system of one forest: Z (N, R), y (N,), its noise and scale, m trees."""

    def __init__(self, Z, y, noise, scale, m):
        self.Z = Z
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.N, self.R = Z.shape
        self.m = m
        self.s2 = 1e-6 + float(noise)
        self.scale = float(scale)
        self.c = self.scale / (m * self.s2)
        M = Z.T @ Z
        M *= self.c
        M[np.diag_indices(self.R)] += 1.0
        self.L = np.linalg.cholesky(M)  # M = L L': U = L', V = L^-1
        del M
        self.v = Z.T @ self.y
        self.w = solve_lower(self.L, solve_lower(self.L, self.v), trans=True)
        self.logdet_M = 2.0 * np.log(np.diag(self.L)).sum()

    def mll(self):
        quad = (self.y @ self.y - self.c * (self.v @ self.w)) / self.s2
        return -0.5 * (quad + self.N * np.log(self.s2) + self.logdet_M)

    def logdet(self):
        return self.N * np.log(self.s2) + self.logdet_M

    def posterior(self, Zc):
        G = solve_lower(self.L, Zc.T)  # V Z_C'
        return self.c * (Zc @ self.w), self.scale / self.m * (G * G).sum(axis=0)

    def draw_cov(self, Zc):
        G = solve_lower(self.L, Zc.T)
        return self.scale / self.m * (G.T @ G)

    def inverse(self):
        G = solve_lower(self.L, self.Z.T)  # V Z'
        K_inv = (np.eye(self.N) - self.c * (G.T @ G)) / self.s2
        return K_inv, (self.y - self.c * (self.Z @ self.w)) / self.s2

    def draws(self, Zc, eps):
        """eps (S, R) -> f (S, C)."""
        mean = self.c * (Zc @ self.w)
        return mean[None, :] + np.sqrt(self.scale / self.m) * (Zc @ solve_lower(self.L, eps.T, trans=True)).T


# ------------------------------------------------------------------ the case table ----
NODE_LIMIT = 255  # a depth-7 complete tree
D_CONT = 8  # mixed_problem puts its 8 continuous columns first: the complete trees split on those


@dataclass(frozen=True)
class Case:
    """B forests; forest b is built from forests[b % len(forests)], a tuple of pieces concatenated along the tree axis:
    ("full", trees, depth) (complete trees, 2^depth leaves each), ("null", trees) (one leaf each) or ("prior", trees).
    shape: what the case claims to reach — (R, code words W, block rows, layout of the R x R sweep with identity columns
    at `bc` forests per chunk)."""

    name: str
    forests: tuple
    N: int
    B: int
    shape: tuple
    C: int  # candidates of the posterior and the draws
    S: int  # draws
    chunk: int | None = None  # forests per chunk (None: all B)
    seed: int = 0

    @property
    def bc(self):
        return min(self.chunk or self.B, self.B)


R513 = (("full", 4, 7), ("null", 1))
R1100 = (("full", 8, 7), ("full", 2, 5), ("null", 12))
CASES = {c.name: c for c in [
    Case("null50", ((("null", 50),),), N=63, B=2, shape=(50, 2, 1, "plain"), C=1, S=1, seed=1),
    Case("m1_r128", ((("full", 1, 7),),), N=300, B=2, shape=(128, 4, 1, "plain"), C=63, S=16, seed=2),
    Case("r129", ((("full", 1, 7), ("null", 1)),), N=63, B=2, shape=(129, 5, 2, "plain"), C=64, S=17, seed=3),
    Case("m64_r256", ((("full", 64, 2),),), N=300, B=2, shape=(256, 8, 2, "plain"), C=65, S=33, seed=4),
    Case("n1_r257", ((("full", 2, 7), ("null", 1)),), N=1, B=2, shape=(257, 9, 3, "plain"), C=300, S=32, seed=5),
    Case("r3xx_prior", ((("full", 10, 5), ("prior", 13)),), N=1000, B=2, shape=(355, 12, 3, "plain"), C=65, S=64, seed=6),
    Case("r513_splitk", (R513,), N=300, B=2, shape=(513, 17, 5, "splitk"), C=300, S=65, seed=7),
    Case("r513_plain", (R513,), N=63, B=60, shape=(513, 17, 5, "plain"), C=63, S=130, seed=8),
    Case("r1100_splitk", (R1100,), N=300, B=2, shape=(1100, 35, 9, "splitk"), C=300, S=17, seed=9),
    Case("r1100_pipelined", (R1100,), N=300, B=19, shape=(1100, 35, 9, "pipelined"), C=64, S=16, seed=10),
    Case("r2048_splitk", ((("full", 16, 7),),), N=1000, B=2, shape=(2048, 64, 16, "splitk"), C=65, S=33, seed=11),
    Case("r2048_pipelined", ((("full", 16, 7),),), N=300, B=6, shape=(2048, 64, 16, "pipelined"), C=1, S=64, seed=12),
    Case("r4096", ((("full", 32, 7),),), N=700, B=2, shape=(4096, 128, 32, "pipelined"), C=63, S=16, seed=13),
    Case("r8192", ((("full", 64, 7),),), N=300, B=1, shape=(8192, 256, 64, "pipelined"), C=300, S=65, seed=14),
    # one chunk, three leaf counts: bushy (360 leaves), prior and all null (50): the last two have padded leaf rows
    Case("mixed_chunk", ((("full", 10, 5), ("null", 40)), (("prior", 50),), (("null", 50),)), N=300, B=3,
         shape=(360, 12, 3, "plain"), C=300, S=130, seed=15),
    Case("prior_ragged", ((("prior", 50),),), N=300, B=5, shape=(132, 5, 2, "plain"), C=65, S=17, chunk=2, seed=16),
]}


# R > N: leaves no training point reaches (empty columns of Z) but candidates do
EMPTY_LEAF_CASES = ("n1_r257", "r513_plain", "r8192")


def limit_case(m):
    """The leaf-space inverse at m trees (half depth-1, half null: R = m + m // 2), N = 100; make_inputs(node_limit=3)."""
    return Case(f"m{m}", ((("full", m // 2, 1), ("null", m - m // 2)),), N=100, B=1, shape=(), C=1, S=1, seed=m)


def build_forest(pieces, rng, bounds, ft, node_limit=NODE_LIMIT):
    parts = []
    for p in pieces:
        if p[0] == "full":
            parts.append(synthetic.full_binary_forest(p[1], D_CONT, p[2], rng, node_limit=node_limit))
        elif p[0] == "null":
            parts.append(create_empty_forest(p[1], node_limit))
        else:
            parts.append(synthetic.sample_prior_forest(p[1], bounds, ft, rng, node_limit=node_limit))
    return np.concatenate(parts, axis=0)


def rr_layout(R, Bc):
    """The layout of the R x R sweep with R identity columns at Bc forests per chunk (make_layout / plan_chunk):
    split-K, pipelined or plain."""
    nrb = -(-R // NB)
    tiles = Bc * 2 * nrb
    if nrb >= 4 and (tiles < 600 if nrb < 8 else tiles * nrb < 3000):
        return "splitk"
    if nrb >= 8 and (Bc % 256 != 0 or nrb < 16):
        return "pipelined"
    return "plain"


@dataclass
class Inputs:
    case: Case
    F: np.ndarray  # (B, m, node_limit)
    X: np.ndarray
    y: np.ndarray
    ft: np.ndarray
    cand: np.ndarray
    noise: np.ndarray
    scale: np.ndarray
    eps: np.ndarray  # (B, S, R)
    info: object  # the packer's bark_pack_info
    Z: list  # per forest: (N, R)
    Zc: list  # per forest: (C, R)

    @property
    def m(self):
        return self.F.shape[1]

    @property
    def R(self):
        return int(self.info.max_bits)


def make_inputs(case: Case, node_limit=NODE_LIMIT):
    X, y, bounds, ft = synthetic.mixed_problem(case.N, seed=100 + case.seed)
    cand, _, _, _ = synthetic.mixed_problem(case.C, seed=200 + case.seed)
    rng = np.random.default_rng(case.seed)
    F = np.stack([build_forest(case.forests[b % len(case.forests)], rng, bounds, ft, node_limit) for b in range(case.B)])
    noise = np.linspace(0.1, 0.3, case.B)
    scale = np.linspace(0.8, 1.3, case.B)
    info, packed = host_pack(F, ft)
    R = int(info.max_bits)
    bits = leaf_bit_table(packed, F.shape[2], int(info.max_depth))
    Z = [leaf_matrix(F[b], bits[b], X, ft, R) for b in range(case.B)]
    Zc = [leaf_matrix(F[b], bits[b], cand, ft, R) for b in range(case.B)]
    eps = rng.standard_normal((case.B, case.S, R))
    return Inputs(case, F, X, y, ft, cand, noise, scale, eps, info, Z, Zc)


def reference(inp: Inputs, b: int) -> LeafRef:
    return LeafRef(inp.Z[b], inp.y, inp.noise[b], inp.scale[b], inp.m)


def check_shape(inp: Inputs):
    """The case reaches the R, code words, block rows and R x R layout it claims; the dense plan query (the same rule for
    N = C = R, identity columns and a chunk that is not a multiple of 256) agrees.  In EMPTY_LEAF_CASES (R > N) the
    training points leave leaves empty and candidates land in them."""
    from bark_amd.fitting import schedule_plan

    case = inp.case
    R, W, nrb, layout = case.shape
    assert inp.R == R, (case.name, inp.R)
    assert -(-R // 32) == W and -(-R // NB) == nrb, case.name
    assert rr_layout(R, case.bc) == layout, case.name
    assert case.bc % 256 != 0
    d = schedule_plan(R, case.bc, C=R, chunk=case.bc, m=inp.m, leaf_words=W)
    assert (d["nrb"], d["ncb"], d["splitk_layout"]) == (nrb, 2 * nrb, int(layout == "splitk")), (case.name, d)
    want = {"splitk": ("splitk", "splitk_lookahead"), "pipelined": ("pipelined",), "plain": ("plain",)}[layout]
    assert d["schedule"] in want and d["last_schedule"] in want, (case.name, d)
    if case.name in EMPTY_LEAF_CASES:
        assert R > case.N
        for Z, Zc in zip(inp.Z, inp.Zc):
            empty = Z.sum(axis=0) == 0
            assert (Zc[:, empty].sum(axis=1) > 0).any(), case.name
