"""numpy restatement of the sample paths (include/bark_hip.h, "Sample paths from a fitted posterior"); no GPU code here.

It starts from the state: M^-1 (B, R, R) and w (B, R) as `fit_posterior` left them on the device, read back as bytes.  For path
p of forest b:  W[p] = c_b w_b + sqrt(scale_b / m) G_b eps[p],  G_b = np.linalg.cholesky(M_b^-1),  c_b = scale_b / (m s2_b),
s2_b = 1e-6 + noise_b.  The path's value at x is the sum of W[p] over the leaf columns of x, tree by tree in the order
t = 0 .. m-1, in a Python loop: the leaf columns come from the oracle's walk and the packer's bit table (leafspace_ref)."""
import numpy as np

from leafspace_ref import host_pack, leaf_bit_table
from oracle import oracle as orc


def align256(n):
    return (n + 255) & ~255


def read_state(state_bytes: np.ndarray, B: int, R: int):
    """(M^-1 (B, R, R), w (B, R), info (B,)) from the bytes of a fitted state (bark_leaf_posterior_bytes' layout)."""
    raw = np.ascontiguousarray(state_bytes, dtype=np.uint8)
    a, b = align256(8 * B * R * R), align256(8 * B * R)
    Minv = raw[:8 * B * R * R].view(np.float64).reshape(B, R, R).copy()
    w = raw[a:a + 8 * B * R].view(np.float64).reshape(B, R).copy()
    info = raw[a + b:a + b + 4 * B].view(np.int32).copy()
    return Minv, w, info


def factor(Minv_b, dtype=np.float64):
    """Lower Cholesky factor; for longdouble an unblocked column sweep (numpy's LAPACK has no such type)."""
    if dtype == np.float64:
        return np.linalg.cholesky(Minv_b)
    A = Minv_b.astype(dtype)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def weights(Minv, w, noise, scale, m, forest, eps, dtype=np.float64):
    """W (P, R) of the paths `forest` (P,) with normals eps (P, R)."""
    forest = np.asarray(forest)
    W = np.empty(eps.shape, dtype=dtype)
    for b in np.unique(forest):
        G = factor(Minv[b], dtype)
        s2 = dtype(1e-6) + dtype(noise[b])
        c, root = dtype(scale[b]) / (dtype(m) * s2), np.sqrt(dtype(scale[b]) / dtype(m))
        for p in np.flatnonzero(forest == b):
            W[p] = c * w[b].astype(dtype) + root * (G @ eps[p].astype(dtype))
    return W


def leaf_columns(F, ft, X):
    """(B, n, m) int64: column of W that point x reads for tree t of forest b, and R."""
    info, packed = host_pack(F, ft)
    bits = leaf_bit_table(packed, F.shape[2], int(info.max_depth))
    m = F.shape[1]
    cols = np.stack([bits[b][np.arange(m)[None, :], orc.pass_through_forest(F[b], X, ft).astype(np.int64)] for b in range(F.shape[0])])
    assert (cols >= 0).all() and (cols < int(info.max_bits)).all()
    return cols, int(info.max_bits)


def evaluate(W, forest, cols):
    """f (P, n): the host loop, trees in the order t = 0 .. m-1 starting from 0.0."""
    P, n, m = W.shape[0], cols.shape[1], cols.shape[2]
    f = np.zeros((P, n))
    for p in range(P):
        c = cols[forest[p]]
        for t in range(m):
            f[p] = f[p] + W[p][c[:, t]]
    return f


def first_argmin(f, maximise=False):
    """(values, indices) per row, the lowest index among equals."""
    idx = np.argmax(f, axis=1) if maximise else np.argmin(f, axis=1)  # numpy returns the first occurrence
    return f[np.arange(f.shape[0]), idx], idx.astype(np.int64)


# ---- where the host drivers cut their work, read off the library's own byte queries (no GPU) ----
MAX_PATHS = 4096  # paths per C call


def resident_factors(lib, R, m=1):
    """Factors bark_leaf_posterior_paths_hip keeps in its workspace at a time, at most 4096: with 4096 forests and 4096
    paths the workspace is the run table (3 P + 1 ints) and min(4096, resident) matrices of R x R doubles, each area
    rounded up to 256 bytes."""
    total = int(lib.bark_leaf_posterior_paths_workspace_bytes(R, m, MAX_PATHS, MAX_PATHS, 0))
    area = total - align256(4 * (3 * MAX_PATHS + 1))
    k = area // (8 * R * R)
    assert total > 0 and align256(8 * k * R * R) == area, (R, total)
    return k


def scan_walk(lib, R, m, C):
    """Forests bark_path_scan_hip walks together over C candidates: a FULL scan of one path keeps the run table (3 ints),
    a flag and the one-hot codes of `walk` forests, ceil(R / 32) words for each candidate of a slab (at most 65 536,
    padded to 128)."""
    total = int(lib.bark_path_scan_workspace_bytes(R, m, 1, C, 0))
    words, cpad = -(-R // 32), -(-min(C, 65536) // 128) * 128
    walk, rest = divmod(total - 512, 4 * words * cpad)
    assert total > 0 and rest == 0, (R, C, total)
    return walk


def smallest_candidates_below(lib, R, m, forests):
    """The smallest candidate count, a multiple of 128 as the padded slab is, at which fewer than `forests` forests are
    walked together; every count from 127 below it up to a slab gives the same walk."""
    for C in range(128, 65536 + 1, 128):
        if scan_walk(lib, R, m, C) < forests:
            return C
    raise AssertionError(f"{forests} forests of {R} leaves are walked together at every candidate count")


def walk_chunks(sorted_forest, walk):
    """[(first forest, forests)] of the leaf walks bark_path_scan_hip makes for a sorted path list: the forests that occur,
    cut where the next one is not the successor of the last and after `walk` of them."""
    runs = np.unique(np.asarray(sorted_forest))
    chunks, r0 = [], 0
    while r0 < len(runs):
        n = 1
        while r0 + n < len(runs) and n < walk and runs[r0 + n] == runs[r0] + n:
            n += 1
        chunks.append((int(runs[r0]), n))
        r0 += n
    return chunks


def call_splits(sorted_forest):
    """[(first path, paths)] of the C calls Python makes for a sorted path list of any length."""
    P = len(sorted_forest)
    return [(p0, min(MAX_PATHS, P - p0)) for p0 in range(0, P, MAX_PATHS)]


def meets_invalid_categorical(F_b, ft, x):
    """Whether the device walk of row x through forest F_b (m, node_limit) sets the fault flag: some tree's path from
    the root comes to a categorical split whose feature value truncates to something negative or not finite
    (walk_tree in common.h; such a value goes right and the walk continues)."""
    for tree in F_b:
        node = tree[0]
        while not node["is_leaf"]:
            f = int(node["feature_idx"])
            if ft[f] == 0:
                xt = np.trunc(x[f])
                if not (xt >= 0.0 and xt < np.inf):
                    return True
                left = bool((int(node["threshold"]) >> int(xt)) & 1) if xt < 32 else False
            else:
                left = x[f] <= node["threshold"]
            node = tree[int(node["left"] if left else node["right"])]
    return False
