"""Host reference and case table of the front end: the leaf walk (traverse.hip) and the Gram fill (gram.hip), every launch variant.

Both promise integer or bit-exact results, so nothing here has a tolerance.  Three pieces:

* the expected LEAF CODES of bark_leaf_codes_hip, `(B, W, npad)` uint32 in either encoding, padding included, built from the
  oracle's node indices (oracle.pass_through_forest) and a reader of the packed wire format that follows child links only — so the
  code reference does not depend on the packer's traversal order (tests/test_host_cpu.py owns that);
* the expected GRAM block from two index arrays in numpy float64, one rounding per documented step;
* a named table of shapes, `CASES`, each row naming the kernel variant it is there for, and `check_shape`, which asserts through
  bark_frontend_variant_query (the function the launchers themselves decide from) that the row reaches it.

tests/test_frontend_reference_cpu.py pins all of this without a device; tests/test_gpu_frontend.py runs the kernels against it."""
import ctypes
import dataclasses
from fractions import Fraction

import numpy as np

from bark_amd import _lib, synthetic as syn
from bark_amd.forest import NODE_RECORD_DTYPE
from oracle import oracle as orc

LEAF_FLAG = 0x80000000
CAT, INT, CONT = 0, 1, 2
CANARY32, CANARY64 = 0xA5C3F00D, 0xA5C3F00D5EEDBEEF  # what every output buffer holds before a call (a NaN pattern as a double)


# ---------------------------------------------------------------------------------------------------------------------------
# generators (beyond bark_amd.synthetic)
# ---------------------------------------------------------------------------------------------------------------------------
def feature_types(d, mixed):
    """continuous, integer and categorical features in turn (`mixed`), or all continuous"""
    return np.array([(CONT, CONT, INT, CAT)[f % 4] for f in range(d)] if mixed else [CONT] * d, dtype=np.int64)


def _threshold(kind, rng):
    if kind == CAT:
        return float(rng.integers(1, 31))  # a bitmask over the categories 0..4
    if kind == INT:
        return float(rng.integers(0, 10))
    return float(np.float32(rng.uniform(0.05, 0.95)))


def points(n, ft, rng, forests=None):
    """n points of the given feature types; with `forests`: some values exactly on thresholds the forests use and NaN, +-inf and
    -0.0 planted on the non-categorical features (tests/test_gpu_parity.py::test_fuzz_scrambled_containers_and_boundary_points)"""
    X = np.empty((n, len(ft)))
    for f, kind in enumerate(ft):
        X[:, f] = rng.integers(0, 5, n) if kind == CAT else rng.integers(0, 11, n) if kind == INT else rng.uniform(size=n)
    if forests is not None:
        thr = forests["threshold"][(forests["is_leaf"] == 0) & (forests["active"] == 1)].astype(np.float64)
        for f in np.flatnonzero(ft != CAT)[:12]:
            if thr.size:
                hit = rng.random(n) < 0.15
                X[hit, f] = rng.choice(thr, hit.sum())
            odd = rng.random(n) < 0.03
            X[odd, f] = rng.choice([np.inf, -np.inf, np.nan, -0.0, np.nextafter(0.5, 1)], odd.sum())
    return X


def comb_tree(k, L, feature, rng):
    """A tree with exactly k leaves and depth k - 1: a chain of splits on one continuous feature with increasing thresholds,
    each hanging a leaf on its left, so uniform points spread over all leaves and leaf j has dense id j."""
    assert 2 * k - 1 <= L
    tree = np.zeros(L, dtype=NODE_RECORD_DTYPE)
    thr = np.sort(rng.uniform(0.02, 0.98, k - 1)).astype(np.float32)
    node = 0
    for j in range(k - 1):
        left, right = 2 * j + 1, 2 * j + 2
        tree[node] = (0, feature, thr[j], left, right, 0xFFFFFFFF if j == 0 else node - 1, j, 1)
        tree[left] = (1, 0, 0, 0, 0, node, j + 1, 1)
        node = right
    tree[node] = (1, 0, 0, 0, 0, 0xFFFFFFFF if k == 1 else node - 1, k - 1, 1)
    return tree


def full_tree(depth, ft, rng, L):
    """A complete binary tree whose splits follow the feature types (category masks, integer and float32 thresholds)."""
    n = 2 ** (depth + 1) - 1
    assert n <= L
    tree = np.zeros(L, dtype=NODE_RECORD_DTYPE)
    for i in range(n):
        dep = (i + 1).bit_length() - 1
        parent = 0xFFFFFFFF if i == 0 else (i - 1) // 2
        if dep == depth:
            tree[i] = (1, 0, 0, 0, 0, parent, dep, 1)
        else:
            f = int(rng.integers(len(ft)))
            tree[i] = (0, f, _threshold(ft[f], rng), 2 * i + 1, 2 * i + 2, parent, dep, 1)
    return tree


def bushy_forest(m, depth, ft, rng, L=None):
    L = L or 2 ** (depth + 1) - 1
    return np.stack([full_tree(depth, ft, rng, L) for _ in range(m)])


def mixed_forest(pattern, ft, rng, L):
    """Trees by `pattern`: 1 = root only, 3 = three leaves, k >= 4 = a comb of k leaves (on the continuous features in turn).  With
    combs of 64 leaves and more between root-only trees, bit fields straddle word edges and whole words stay empty between two
    set bits of a point."""
    cont = np.flatnonzero(ft == CONT)
    trees = []
    for t, k in enumerate(pattern):
        if k == 3:
            tree = np.zeros(L, dtype=NODE_RECORD_DTYPE)
            cat = np.flatnonzero(ft == CAT)  # the root splits on a category where there is one, so every point meets one
            f, g = int(rng.choice(cat)) if len(cat) else int(rng.integers(len(ft))), int(rng.integers(len(ft)))
            tree[0] = (0, f, _threshold(ft[f], rng), 1, 2, 0xFFFFFFFF, 0, 1)
            tree[1] = (1, 0, 0, 0, 0, 0, 1, 1)
            tree[2] = (0, g, _threshold(ft[g], rng), 3, 4, 0, 1, 1)
            tree[3] = tree[4] = (1, 0, 0, 0, 0, 2, 2, 1)
        else:
            tree = comb_tree(k, L, int(cont[t % len(cont)]), rng)
        trees.append(tree)
    return np.stack(trees)


# ---------------------------------------------------------------------------------------------------------------------------
# wire format, variant query
# ---------------------------------------------------------------------------------------------------------------------------
def pack(F, ft):
    """(info, packed (B, m, stride, 4) uint32) of bark_forest_pack_info + bark_forest_pack, on the host"""
    F = np.ascontiguousarray(F)
    ft = np.ascontiguousarray(ft, dtype=np.int64)
    B, m, L = F.shape
    info = _lib.PackInfo()
    _lib.check(_lib.lib().bark_forest_pack_info(_lib.ptr(F), B, m, L, _lib.ptr(ft), len(ft), ctypes.byref(info)))
    packed = np.empty((B, m, int(info.stride), 4), dtype=np.uint32)
    assert packed.nbytes == info.packed_bytes
    _lib.check(_lib.lib().bark_forest_pack(_lib.ptr(F), _lib.ptr(ft), len(ft), ctypes.byref(info), _lib.ptr(packed)))
    return info, packed


def leaf_tables(packed, L):
    """Per forest and tree the map original node index -> dense leaf id and -> bit position, as (B, m, L) int64 arrays (-1: not a
    reachable leaf), read from the leaf records (w1 = original index, w0 & 0x7fffffff = dense id, w2 = bit position).  The records
    are found by following the child links w2 / w3 from slot 0, whatever order the packer numbered them in; the unused tail
    slots of a tree (self-looping leaves) are never reached."""
    B, m, stride, _ = packed.shape
    ids, bits = np.full((B, m, L), -1, dtype=np.int64), np.full((B, m, L), -1, dtype=np.int64)
    for b in range(B):
        for t in range(m):
            tree, stack, seen = packed[b, t], [0], set()
            while stack:
                k = stack.pop()
                if k in seen:
                    continue
                seen.add(k)
                w0, w1, w2, w3 = (int(v) for v in tree[k])
                if w0 & LEAF_FLAG:
                    ids[b, t, w1], bits[b, t, w1] = w0 & 0x7FFFFFFF, w2
                else:
                    stack += [w2, w3]
    return ids, bits


def query(info, N, M, d, ld=None, batch_stride=None, out_mod16=0):
    """bark_frontend_variant_query -> _lib.FrontendVariant"""
    ld = M if ld is None else ld
    v = _lib.FrontendVariant()
    _lib.check(_lib.lib().bark_frontend_variant_query(ctypes.byref(info), N, M, d, ld, N * ld if batch_stride is None else batch_stride,
                                                      out_mod16, ctypes.byref(v)))
    return v


def walk_variant_name(v):
    enc = "bits" if v.encoding == 1 else "bytes"
    if v.codes_grouped:
        return "grouped_%s_%s" % ("nodes_lds" if v.codes_nodes_lds else "nodes_global", enc)
    return "plain_%s_%s" % ("x_lds" if v.codes_x_lds else "x_global", enc)


def index_variant_name(v):
    return "plain_x_lds_indices" if v.indices_staged else "plain_x_global_indices"


def gram_variant_name(v):
    return "%s_%s_%s" % (_lib.GRAM_REPS[v.gram_rep], "wide" if v.gram_tile_cols > 64 else "narrow", "vec2" if v.gram_vec2 else "pairs")


WALK_VARIANTS = {"%s_%s" % (k, e) for k in ("grouped_nodes_lds", "grouped_nodes_global", "plain_x_lds", "plain_x_global") for e in ("bits", "bytes")} \
    | {"plain_x_lds_indices", "plain_x_global_indices"}
GRAM_VARIANTS = {"%s_%s_%s" % (r, t, v) for r in _lib.GRAM_REPS for t in ("wide", "narrow") for v in ("vec2", "pairs")}


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def reference_codes(F, X, ft, info=None, tables=None):
    """(B, W, npad) uint32: what bark_leaf_codes_hip writes for the forests F — the encoding the library picks from `info`, the
    point index fastest, and ZERO in every plane entry N <= i < npad."""
    lib = _lib.lib()
    if info is None:
        info, packed = pack(F, ft)
        tables = leaf_tables(packed, F.shape[2])
    ids, bits = tables
    B, m, _ = F.shape
    N, npad, W = X.shape[0], int(lib.bark_leaf_npad(X.shape[0])), int(lib.bark_leaf_words(ctypes.byref(info)))
    out = np.zeros((B, W, npad), dtype=np.uint32)
    trees = np.arange(m)
    for b in range(B):
        idx = orc.pass_through_forest(F[b], X, ft).astype(np.int64)  # (N, m) node indices
        if lib.bark_leaf_encoding(ctypes.byref(info)) == 1:  # one bit per tree
            pos = bits[b][trees[None, :], idx]
            assert (pos >= 0).all()
            for t in range(m):
                keep = (pos[:, t] >> 5) < W
                np.bitwise_or.at(out[b], (pos[keep, t] >> 5, np.flatnonzero(keep)), (1 << (pos[keep, t] & 31)).astype(np.uint32))
        else:  # 4 dense ids per dword
            dense = ids[b][trees[None, :], idx]
            assert (dense >= 0).all() and (dense < 256).all()
            for t in range(m):
                out[b, t >> 2, :N] |= (dense[:, t] << (8 * (t & 3))).astype(np.uint32)
    return out


_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def agree_from_codes(c1, c2, N, M, m, bits):
    """(N, M) number of agreeing trees from two code arrays (W, npad) of one forest, the way the Gram kernels count: popcount of
    a & b for the bit code; for the byte code m minus the bytes that differ (the unused byte lanes of the last word are equal)."""
    a, b = c1[:, :N, None], c2[:, None, :M]
    if bits:
        return _POP8[np.ascontiguousarray(a & b).view(np.uint8)].reshape(a.shape[0], N, M, 4).sum(axis=(0, 3))
    differ = np.ascontiguousarray(a ^ b).view(np.uint8).reshape(a.shape[0], N, M, 4) != 0
    return m - differ.sum(axis=(0, 3))


def agree_from_indices(idx1, idx2):
    return (idx1[:, None, :] == idx2[None, :, :]).sum(axis=2)


def gram_from_counts(count, m, shift=None, scale=None, noise=None):
    """The documented order (include/bark_hip.h), one float64 rounding per step: (1.0/m) * count, - shift, scale *, and
    + (1e-6 + noise) where i == j."""
    val = (1.0 / m) * count.astype(np.float64)
    if shift is not None:
        val = val - np.float64(shift)
    if scale is not None:
        val = np.float64(scale) * val
    if noise is not None:
        k = np.arange(min(val.shape))
        val[k, k] = val[k, k] + (1e-6 + np.float64(noise))
    return val


def _fl(x):
    return float(x)  # Fraction -> the nearest double


def gram_variants_exact(count, m, shift, scale, noise):
    """Per DISTINCT count on and off the diagonal, with exact rational arithmetic: the documented result and what three wrong
    kernels would give — shift and scale in the other order, `inv_m * count - shift` as one fused multiply-add, and
    `scale * val + jitter` as one.  -> dict name -> list of (count, on_diagonal, documented, wrong)"""
    inv_m = 1.0 / m
    out = {"swapped": [], "fma_shift": [], "fma_jitter": []}
    k = np.arange(min(count.shape))
    diag = set(int(c) for c in count[k, k]) if noise is not None else set()
    for c in sorted(set(int(c) for c in count.ravel())):
        for on_diag in ((False, True) if c in diag else (False,)):
            jit = (1e-6 + noise) if on_diag else None
            base = inv_m * c
            v = base - shift if shift is not None else base
            w = scale * v if scale is not None else v
            doc = w + jit if on_diag else w
            if shift is not None and scale is not None:
                alt = scale * base - shift
                out["swapped"].append((c, on_diag, doc, alt + jit if on_diag else alt))
            if shift is not None:
                f = _fl(Fraction(inv_m) * c - Fraction(shift))
                g = scale * f if scale is not None else f
                out["fma_shift"].append((c, on_diag, doc, g + jit if on_diag else g))
            if scale is not None and on_diag and v != 1.0:  # (x1 is x2 without a shift: the diagonal is scale * 1.0, exact in any evaluation)
                out["fma_jitter"].append((c, on_diag, doc, _fl(Fraction(scale) * Fraction(v) + Fraction(jit))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class WalkCase:
    variant: str      # WALK_VARIANTS name of the code walk (or of the index walk, `indices`)
    forest: str       # generator (make_forests)
    N: int
    B: int            # forests in the call: copies of at most 8 distinct ones
    d: int
    m: int
    mixed: bool = True      # continuous + integer + categorical features
    indices: bool = False   # the row is there for bark_leaf_indices_hip (MODE 0)
    flush: bool = False     # bit code whose fields straddle word edges and leave whole words empty between two set bits


@dataclasses.dataclass(frozen=True)
class GramCase:
    variant: str      # "<rep>_<tile>": the layouts of the row cover vec2 and shifted pairs
    forest: str
    N: int
    M: int
    m: int
    B: int = 2
    d: int = 4
    same: bool = False      # x1 is x2
    layouts: str = "basic"  # "basic": dense, aligned-even and 8-bytes-off; "sweep": every single cause of VEC2 = false
    params: bool = False    # shift / scale / noise: each alone, each pair, all three
    carry: bool = False     # byte ids whose xor has bit 7 and a lower bit set (the 7-bit compare would carry)


CASES = {
    # ---- code walks -------------------------------------------------------------------------------------------------------
    "walk_grouped_lds_bits": WalkCase("grouped_nodes_lds_bits", "prior", 300, 2, 12, 50),
    "walk_grouped_lds_bytes": WalkCase("grouped_nodes_lds_bytes", "bushy4", 300, 2, 8, 60),       # 60 x 31 nodes fit beside the rows
    "walk_grouped_global_bytes": WalkCase("grouped_nodes_global_bytes", "bushy4", 300, 2, 8, 64),  # 64 x 31 do not (61..63 such trees take the bit code)
    "walk_grouped_lds_bits_mixed": WalkCase("grouped_nodes_lds_bits", "mixed13", 300, 2, 8, 13, flush=True),      # 13 x 139 nodes fit
    "walk_grouped_global_bits": WalkCase("grouped_nodes_global_bits", "mixed14", 300, 2, 8, 14, flush=True),  # 14 x 139 do not
    "walk_plain_lds_bytes": WalkCase("plain_x_lds_bytes", "bushy4", 300, 1024, 8, 8),
    "walk_plain_lds_bits": WalkCase("plain_x_lds_bits", "mixed16", 300, 1024, 8, 16, flush=True),
    "walk_plain_lds_bytes_d31": WalkCase("plain_x_lds_bytes", "bushy4", 300, 1024, 31, 8),
    "walk_plain_global_bytes_d32": WalkCase("plain_x_global_bytes", "bushy4", 300, 1024, 32, 8),
    "walk_plain_lds_bits_d31": WalkCase("plain_x_lds_bits", "mixed16", 300, 1024, 31, 16, flush=True),
    "walk_plain_global_bits_d32": WalkCase("plain_x_global_bits", "mixed16", 300, 1024, 32, 16, flush=True),
    "walk_plain_global_bytes_d257": WalkCase("plain_x_global_bytes", "bushy4", 300, 2, 257, 8),
    "walk_plain_global_bits_d257": WalkCase("plain_x_global_bits", "mixed16", 300, 2, 257, 16, flush=True),
    # ---- index walks (MODE 0): the staging boundary d = 15 | 16, chunk edges of 32 trees, block edges of 256 points -------------
    "index_d15_m33_n257": WalkCase("plain_x_lds_indices", "prior", 257, 2, 15, 33, indices=True),
    "index_d16_m33_n257": WalkCase("plain_x_global_indices", "prior", 257, 2, 16, 33, indices=True),
    "index_d15_m1_n1": WalkCase("plain_x_lds_indices", "prior", 1, 2, 15, 1, indices=True),
    "index_d15_m31_n255": WalkCase("plain_x_lds_indices", "prior", 255, 2, 15, 31, indices=True),
    "index_d15_m32_n256": WalkCase("plain_x_lds_indices", "prior", 256, 2, 15, 32, indices=True),
    "index_d15_m64_n257": WalkCase("plain_x_lds_indices", "prior", 257, 2, 15, 64, indices=True),
    "index_d15_m65_n255": WalkCase("plain_x_lds_indices", "prior", 255, 2, 15, 65, indices=True),
    "index_d16_m65_n256": WalkCase("plain_x_global_indices", "prior", 256, 2, 16, 65, indices=True),
    "index_d16_m1_n1": WalkCase("plain_x_global_indices", "prior", 1, 2, 16, 1, indices=True),
    # ---- Gram: representations and tiles, tile-edge extents ---------------------------------------------------------------
    "gram_bytes7_comb128": GramCase("bytes7_wide", "comb128", 33, 65, 5, d=3),
    "gram_bytes8_comb129": GramCase("bytes8_wide", "comb129", 63, 127, 6, d=3, carry=True),
    "gram_bits_prior": GramCase("bits_wide", "prior", 65, 129, 50, d=8, layouts="sweep"),
    "gram_bits_w102": GramCase("bits_wide", "bits102", 31, 128, 8),
    "gram_bits_w103": GramCase("bits_narrow", "bits103", 64, 63, 9),
    "gram_bits_w112": GramCase("bits_narrow", "bits112", 65, 129, 7, layouts="sweep"),
    "gram_bytes7_m408": GramCase("bytes7_wide", "bushy4", 32, 64, 408),
    "gram_bytes7_m412": GramCase("bytes7_narrow", "bushy4", 63, 65, 412),
    "gram_bytes7_m409": GramCase("bytes7_narrow", "bushy5", 1, 2, 409),
    "gram_bytes7_m410": GramCase("bytes7_narrow", "bushy5", 33, 1, 410),
    "gram_bytes7_m411": GramCase("bytes7_narrow", "bushy5", 64, 127, 411),
    "gram_bytes8_m412": GramCase("bytes8_narrow", "bushy4+comb129", 65, 128, 412, carry=True),
    "gram_bytes7_m7": GramCase("bytes7_wide", "bushy4", 1, 1, 7),
    # ---- Gram: shift, scale, noise ---------------------------------------------------------------------------------------------
    "gram_params_m3_same": GramCase("bits_wide", "prior", 40, 40, 3, B=3, d=8, same=True, params=True),
    "gram_params_m3_rect": GramCase("bits_wide", "prior", 33, 70, 3, B=3, d=8, params=True),
    "gram_params_m7_same": GramCase("bits_wide", "prior", 40, 40, 7, B=3, d=8, same=True, params=True),
    "gram_params_m7_rect": GramCase("bits_wide", "prior", 70, 33, 7, B=3, d=8, params=True),
    "gram_params_m13_same": GramCase("bits_wide", "prior", 40, 40, 13, B=3, d=8, same=True, params=True),
    "gram_params_m13_rect": GramCase("bytes7_wide", "bushy5", 33, 70, 13, B=3, d=8, params=True),
}
WALK_CASES = [n for n, c in CASES.items() if isinstance(c, WalkCase)]
GRAM_CASES = [n for n, c in CASES.items() if isinstance(c, GramCase)]
PARAM_COMBOS = [("shift",), ("scale",), ("noise",), ("shift", "scale"), ("shift", "noise"), ("scale", "noise"), ("shift", "scale", "noise")]
MIXED_PATTERNS = {"mixed13": [70, 1, 1, 3, 65, 1, 1, 1, 3, 1, 66, 1, 3], "mixed14": [70, 1, 1, 3, 65, 1, 1, 1, 3, 1, 66, 1, 3, 1],
                  "mixed16": [70, 1, 1, 3, 65, 1, 1, 1, 3, 1, 66, 1, 3, 1, 1, 1]}
BITS_DEPTHS = {"bits102": [9] * 6 + [7, 6], "bits103": [9] * 6 + [7, 6, 5], "bits112": [9] * 7, "bits113": [9] * 7 + [0]}


def case_seed(name):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 100003


def make_forests(kind, n, m, ft, rng):
    """n distinct forests (n, m, L) of one generator"""
    d = len(ft)
    if kind == "prior":
        bounds = np.array([(0.0, 31.0) if k == CAT else (0.0, 10.0) if k == INT else (0.0, 1.0) for k in ft])
        return syn.sample_prior_forests(n, m, bounds, ft, seed=int(rng.integers(1 << 30)))
    if kind in ("bushy4", "bushy5"):  # complete trees of 16 / 32 leaves: the byte code (16 leaves: while m is a multiple of 4)
        return np.stack([bushy_forest(m, int(kind[5]), ft, rng) for _ in range(n)])
    if kind in MIXED_PATTERNS:
        assert len(MIXED_PATTERNS[kind]) == m
        return np.stack([mixed_forest(MIXED_PATTERNS[kind], ft, rng, 139) for _ in range(n)])
    if kind in ("comb128", "comb129"):
        k = int(kind[4:])
        return np.stack([np.stack([comb_tree(k, 2 * k - 1, t % d, rng) for t in range(m)]) for _ in range(n)])
    if kind == "bushy4+comb129":
        out = np.zeros((n, m, 257), dtype=NODE_RECORD_DTYPE)
        for b in range(n):
            out[b, :, :31] = bushy_forest(m, 4, ft, rng)
            out[b, m // 2] = comb_tree(129, 257, 0, rng)
        return out
    if kind in BITS_DEPTHS:
        assert len(BITS_DEPTHS[kind]) == m
        return np.stack([np.stack([full_tree(dep, ft, rng, 1023) for dep in BITS_DEPTHS[kind]]) for _ in range(n)])
    raise KeyError(kind)


@dataclasses.dataclass
class Inputs:
    case: object
    ft: np.ndarray
    distinct: np.ndarray   # (n <= 8, m, L) the distinct forests
    which: np.ndarray      # (B,) index into `distinct` of every forest of the call
    info: object           # PackInfo of the B forests of the call
    packed: np.ndarray     # (B, m, stride, 4) uint32
    tables: tuple          # leaf_tables of the distinct forests
    X1: np.ndarray
    X2: np.ndarray

    @property
    def forests(self):
        return self.distinct[self.which]


def make_inputs(name):
    case = CASES[name]
    rng = np.random.default_rng(case_seed(name))
    walk = isinstance(case, WalkCase)
    ft = feature_types(case.d, case.mixed if walk else case.forest in ("prior", "bushy4", "bushy5"))
    n = min(case.B, 8)
    distinct = make_forests(case.forest, n, case.m, ft, rng)
    which = np.arange(case.B) % n
    info, packed = pack(distinct[which], ft)
    dinfo, dpacked = (info, packed) if n == case.B else pack(distinct, ft)
    assert (dinfo.stride, dinfo.max_leaves, dinfo.max_bits) == (info.stride, info.max_leaves, info.max_bits)
    tables = leaf_tables(dpacked, distinct.shape[2])
    plant = distinct if walk or case.forest in ("prior", "bushy4", "bushy5") else None
    X1 = points(case.N, ft, rng, plant)
    X2 = X1 if walk or case.same else points(case.M, ft, rng, plant)
    return Inputs(case, ft, distinct, which, info, packed, tables, X1, X2)


def distinct_info(inp):
    """PackInfo with B = the number of distinct forests (same stride and widths as the call's: the packed layout is shared)"""
    info = _lib.PackInfo.from_buffer_copy(inp.info)
    info.B = inp.distinct.shape[0]
    info.packed_bytes = info.B * info.m * info.stride * 16
    return info


def codes_of(inp, X):
    """reference codes of the DISTINCT forests, (n, W, npad)"""
    return reference_codes(inp.distinct, X, inp.ft, distinct_info(inp), inp.tables)


def gram_layouts(case):
    """(ld, batch_stride, offset in elements) of every output layout the row runs"""
    N, M = case.N, case.M
    if case.layouts == "sweep":  # ld - M in 0..3, batch_stride - N * ld in 0..2, base aligned and 8 bytes off; M and M - 1 columns
        return [(Mv + a, N * (Mv + a) + g, off, Mv) for Mv in (M, M - 1) for a in range(4) for g in range(3) for off in (0, 1)]
    even = M + (M & 1)
    return [(M, N * M, 0, M), (even, N * even, 0, M), (even + 1, N * (even + 1) + 1, 1, M)]


def layout_causes(ld, bs, off):
    return tuple(c for c, bad in (("odd_ld", ld % 2), ("odd_batch_stride", bs % 2), ("base_off_8", off % 2)) if bad)


def visible(count, m, p):
    """every wrong evaluation that the combination admits (gram_variants_exact) changes at least one entry"""
    return all(any(doc != wrong for _, _, doc, wrong in rows) for rows in gram_variants_exact(count, m, p["shift"], p["scale"], p["noise"]).values() if rows)


def gram_params(inp, combo):
    """shift / scale / noise per forest for one combination (None where absent).  The values are drawn per forest from a seeded
    stream and the first draw is kept for which, on the REFERENCE's counts of that forest, the order of the steps and their separate
    roundings show in at least one entry (`visible`): with a handful of distinct counts most values hide one of them.
    -> dict of (B,) arrays, and the per-forest counts"""
    case = inp.case
    counts, out = [], {k: np.zeros(case.B) for k in ("shift", "scale", "noise")}
    for b in range(case.B):
        F = inp.distinct[inp.which[b]]
        count = agree_from_indices(orc.pass_through_forest(F, inp.X1, inp.ft), orc.pass_through_forest(F, inp.X2, inp.ft))
        counts.append(count)
        rng = np.random.default_rng([case.m, b, len(combo), sum(map(len, combo))])
        for _ in range(1000):
            draw = {"shift": rng.integers(1, case.m) / case.m if case.m > 1 and rng.random() < 0.5 else rng.uniform(0.05, 0.6),
                    "scale": rng.uniform(0.6, 1.9), "noise": rng.uniform(0.01, 0.3)}
            p = {k: (float(draw[k]) if k in combo else None) for k in draw}
            if visible(count, case.m, p):
                break
        else:
            raise AssertionError("no visible values for %s forest %d" % (combo, b))
        for k in out:
            out[k][b] = draw[k]
    return {k: (v if k in combo else None) for k, v in out.items()}, counts


def check_shape(name, inp=None):
    """Asserts, through the library's own variant query, that the row reaches the variant it is named for; returns the set of
    variant names (WALK_VARIANTS / GRAM_VARIANTS) it reaches."""
    case = CASES[name]
    inp = inp or make_inputs(name)
    assert inp.distinct.shape[0] <= 8 and inp.info.B == case.B and inp.info.m == case.m
    if isinstance(case, WalkCase):
        v = query(inp.info, case.N, case.N, case.d)
        got = index_variant_name(v) if case.indices else walk_variant_name(v)
        assert got == case.variant, (name, got, v.codes_workgroups)
        if case.N > 256:  # the last block is partly live, partly padding
            assert case.N % 256 and int(_lib.lib().bark_leaf_npad(case.N)) > case.N
        if case.mixed:
            assert {CAT, INT, CONT} <= set(inp.ft.tolist()) or case.d < 4
        if case.flush:
            _, bits = inp.tables
            lo, hi = np.where(bits >= 0, bits, 1 << 30).min(axis=2), bits.max(axis=2)  # (n, m) first and last bit of every tree's field
            assert ((lo >> 5) != (hi >> 5)).any(), name  # a field straddles a word edge
            codes = codes_of(inp, inp.X1)[:, :, :case.N]
            assert v.encoding == 1
            far = False
            for plane in codes.transpose(0, 2, 1).reshape(-1, codes.shape[1]):  # per point: words of consecutive set bits
                setw = np.flatnonzero(plane)
                far = far or bool((np.diff(setw) >= 2).any())
            assert far, name  # some point's consecutive set bits are at least two words apart: the flush loop runs twice
        return {index_variant_name(v), walk_variant_name(v)}
    reached = set()
    for ld, bs, off, M in gram_layouts(case):
        v = query(inp.info, case.N, M, case.d, ld, bs, 8 * (off % 2))
        assert gram_variant_name(v).startswith(case.variant + "_"), (name, gram_variant_name(v), v.words)
        assert bool(v.gram_vec2) == (not layout_causes(ld, bs, off)), (name, ld, bs, off)
        reached.add(gram_variant_name(v))
    assert reached == {case.variant + "_vec2", case.variant + "_pairs"}, (name, reached)
    if case.layouts == "sweep":
        single = {layout_causes(ld, bs, off) for ld, bs, off, M in gram_layouts(case)}
        assert {("odd_ld",), ("odd_batch_stride",), ("base_off_8",), ()} <= single
        # an odd M with ld = M, and an odd ld under an even M, each as the only cause
        assert any(M % 2 and ld == M and layout_causes(ld, bs, off) == ("odd_ld",) for ld, bs, off, M in gram_layouts(case))
        assert any(M % 2 == 0 and ld % 2 and layout_causes(ld, bs, off) == ("odd_ld",) for ld, bs, off, M in gram_layouts(case))
    if case.carry:
        ids, _ = inp.tables
        ok = False
        for b in range(inp.distinct.shape[0]):
            i1 = orc.pass_through_forest(inp.distinct[b], inp.X1, inp.ft).astype(np.int64)
            i2 = orc.pass_through_forest(inp.distinct[b], inp.X2, inp.ft).astype(np.int64)
            for t in range(case.m):
                x = ids[b, t][i1[:, t]][:, None] ^ ids[b, t][i2[:, t]][None, :]
                ok = ok or bool((((x & 0x80) != 0) & ((x & 0x7F) != 0)).any())
        assert ok, name  # two reached ids of one tree whose xor has bit 7 AND a lower bit set
    return reached


def design_table():
    """The variant table of DESIGN.md section 4 (front end), generated from the query."""
    rows = ["| case | shape | walk kernel | Gram kernel |", "|---|---|---|---|"]
    for name, case in CASES.items():
        inp = make_inputs(name)
        if isinstance(case, WalkCase):
            v = query(inp.info, case.N, case.N, case.d)
            rows.append("| `%s` | N = %d, B = %d, d = %d, m = %d, %s | `%s` | — |" % (
                name, case.N, case.B, case.d, case.m, case.forest, index_variant_name(v) if case.indices else walk_variant_name(v)))
        else:
            v = query(inp.info, case.N, case.M, case.d)
            rows.append("| `%s` | N = %d, M = %d, B = %d, m = %d, W = %d, %s | `%s` | `%s_%s` (+ `vec2` / `pairs` by layout) |" % (
                name, case.N, case.M, case.B, case.m, v.words, case.forest, walk_variant_name(v), *gram_variant_name(v).split("_")[:2]))
    return "\n".join(rows)
