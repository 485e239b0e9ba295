"""Host restatement, in plain numpy and Python loops, of the acquisition search under linear input constraints: the cells' usable
closed intervals (bark_amd.optimizer.cell_boxes) by brute force, the repair step (csrc/domain.hip, bark_domain_repair_hip) one row
at a time with Python floats — a multiply and an add are two roundings, as on the device — and the closed-form box test that
says whether a cell holds a feasible point at all."""
import math

import numpy as np

CAT, INT, CONT = 0, 1, 2


# ---- cell boxes ---------------------------------------------------------------------------------------------------------------
def brute_boxes(forest, bounds, ft):
    """(cell_off, cell_lo, cell_hi) from a walk over every record, one feature at a time."""
    d = len(ft)
    thr = [[] for _ in range(d)]
    for node in np.asarray(forest).reshape(-1):
        if int(node["active"]) == 1 and int(node["is_leaf"]) == 0:
            thr[int(node["feature_idx"])].append(float(np.float64(node["threshold"])))
    off, los, his = [0], [], []
    for f in range(d):
        lo, hi = float(bounds[f][0]), float(bounds[f][1])
        if ft[f] == CAT:
            cats = [float(i) for i in range(64) if int(hi) >> i & 1]
            los += cats
            his += cats
        elif ft[f] == INT:
            ilo, ihi = int(lo), int(hi)
            cuts = sorted({int(math.floor(t)) for t in thr[f] if math.isfinite(t) and ilo <= math.floor(t) < ihi})
            los += [float(ilo)] + [float(c + 1) for c in cuts]
            his += [float(c) for c in cuts] + [float(ihi)]
        elif lo == hi:
            los.append(lo)
            his.append(lo)
        else:
            cuts = sorted({t for t in thr[f] if lo < t < hi})
            los += [lo] + [float(np.nextafter(t, np.inf)) for t in cuts]
            his += cuts + [hi]
        off.append(len(los))
    return np.array(off, dtype=np.int64), np.array(los, dtype=np.float64), np.array(his, dtype=np.float64)


# ---- constraints ----------------------------------------------------------------------------------------------------------------
def csr(A):
    """(row_ptr, col, coef) of the non-zeros of A (K, d), the columns of a row ascending."""
    A = np.asarray(A, dtype=np.float64)
    row_ptr, col, coef = [0], [], []
    for k in range(A.shape[0]):
        for f in range(A.shape[1]):
            if A[k, f] != 0:
                col.append(f)
                coef.append(float(A[k, f]))
        row_ptr.append(len(col))
    return np.array(row_ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(coef, dtype=np.float64)


def tolerances(A, b, bounds, tol=1e-12):
    """tol_k = tol (|b_k| + sum_f |A_kf| max(|lo_f|, |hi_f|)); a feature without a coefficient contributes nothing."""
    A = np.asarray(A, dtype=np.float64)
    out = []
    for k in range(A.shape[0]):
        s = abs(float(b[k]))
        for f in range(A.shape[1]):
            if A[k, f] != 0:
                s += abs(float(A[k, f])) * max(abs(float(bounds[f][0])), abs(float(bounds[f][1])))
        out.append(tol * s)
    return np.array(out, dtype=np.float64)


def residual(row_ptr, col, coef, b, x, k):
    s = 0.0
    for e in range(int(row_ptr[k]), int(row_ptr[k + 1])):
        p = float(coef[e]) * float(x[col[e]])  # rounded ...
        s = s + p                              # ... and rounded again: no fused multiply-add in Python
    return s - float(b[k])


def find_cell(off, hi, f, x):
    """First cell of feature f with x <= hi; None when there is none (x above the range, or NaN)."""
    if x != x:
        return None
    c = int(off[f]) + int(np.searchsorted(hi[int(off[f]):int(off[f + 1])], x, side="left"))  # hi ascends within a feature
    return c if c < int(off[f + 1]) else None


def repair(off, lo, hi, ft, row_ptr, col, coef, b, tol, eq, rows, passes=4):
    """-> (rows (n, d) repaired copy, feasible (n,) bool), the three steps of the entry point's contract."""
    rows = np.array(rows, dtype=np.float64)
    K = len(b)
    touched = sorted({int(c) for c in col})
    feasible = np.zeros(rows.shape[0], dtype=bool)
    for i in range(rows.shape[0]):
        x = [float(v) for v in rows[i]]
        cell = {}
        for f in touched:
            c = find_cell(off, hi, f, x[f])
            if c is None or x[f] < lo[c]:
                cell = None
                break
            cell[f] = c
        if cell is None:
            continue  # infeasible, unchanged
        for _ in range(passes):
            for k in range(K):
                r = residual(row_ptr, col, coef, b, x, k)
                for e in range(int(row_ptr[k]), int(row_ptr[k + 1])):
                    if (r == 0.0) if eq[k] else (r <= 0.0):
                        break
                    a, f = float(coef[e]), int(col[e])
                    if a == 0.0 or (eq[k] and ft[f] == INT):
                        continue
                    if ft[f] == INT:
                        w = x[f] - math.copysign(1.0, a) * math.ceil(r / abs(a))
                    else:
                        w = x[f] - r / a
                    w = min(max(w, float(lo[cell[f]])), float(hi[cell[f]]))
                    if w != x[f]:
                        x[f] = w
                        r = residual(row_ptr, col, coef, b, x, k)
        ok = True
        for k in range(K):
            r = residual(row_ptr, col, coef, b, x, k)
            ok = ok and (abs(r) <= tol[k] if eq[k] else r <= tol[k])
        for f in touched:
            rows[i, f] = x[f]
        feasible[i] = ok
    return rows, feasible


# ---- the closed box test ------------------------------------------------------------------------------------------------------
def box_admits(off, lo, hi, row_ptr, col, coef, b, eq, x):
    """Does the product cell that holds x contain a point with A x <= b (= b)?  Exact for one row, and for rows with pairwise
    disjoint supports: sum_f min(A_kf lo, A_kf hi) <= b_k, for equality min <= b_k <= max.  None when x lies in no cell."""
    for k in range(len(b)):
        low = high = 0.0
        for e in range(int(row_ptr[k]), int(row_ptr[k + 1])):
            f, a = int(col[e]), float(coef[e])
            c = find_cell(off, hi, f, float(x[f]))
            if c is None or x[f] < lo[c]:
                return None
            low += min(a * lo[c], a * hi[c])
            high += max(a * lo[c], a * hi[c])
        if low > b[k] or (eq[k] and high < b[k]):
            return False
    return True


# ---- the problems the CPU and the GPU tests share ---------------------------------------------------------------------------
def mixed5():
    """d = 5: two continuous features, an integer, three categories, a continuous feature with lo == hi; B = 2 prior forests of
    m = 4 trees, N = 24 points.  -> (model, (X, y), bounds, ft); the grid has 2079 cells."""
    from bark_amd import synthetic

    ft = np.array([CONT, CONT, INT, CAT, CONT], dtype=np.int64)
    bounds = np.array([[0.0, 1.0], [-1.0, 2.0], [0.0, 10.0], [0.0, float(0b1011)], [0.5, 0.5]])
    F = synthetic.sample_prior_forests(2, 4, bounds, ft, seed=0, beta=0.5)
    rng = np.random.default_rng(5)
    X = np.column_stack([rng.uniform(0, 1, 24), rng.uniform(-1, 2, 24), rng.integers(0, 11, 24), rng.choice([0, 1, 3], 24),
                         np.full(24, 0.5)]).astype(np.float64)
    y = rng.standard_normal(24)
    return (F, np.array([0.1, 0.05]), np.array([1.0, 0.8])), (X, y), bounds, ft


def wide70():
    """d = 70 continuous features in [-1, 1], B = 2 prior forests of m = 4 trees: most features carry no coefficient."""
    from bark_amd import synthetic

    ft = np.full(70, CONT, dtype=np.int64)
    bounds = np.tile([[-1.0, 1.0]], (70, 1))
    return synthetic.sample_prior_forests(2, 4, bounds, ft, seed=3, beta=0.5), bounds, ft


def uniform_rows(bounds, ft, n, seed):
    """n points of the domain, uniform over its values."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, len(ft)), dtype=np.float64)
    for f in range(len(ft)):
        lo, hi = float(bounds[f][0]), float(bounds[f][1])
        if ft[f] == CAT:
            out[:, f] = rng.choice([i for i in range(64) if int(hi) >> i & 1], n)
        elif ft[f] == INT:
            out[:, f] = rng.integers(int(lo), int(hi) + 1, n)
        else:
            out[:, f] = np.minimum(lo + rng.uniform(size=n) * (hi - lo), hi)
    return out
