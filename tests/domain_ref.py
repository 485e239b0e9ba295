"""Host restatement, in plain numpy and Python loops, of the acquisition search over the whole domain
(bark_amd/optimizer/domain.py, csrc/domain.hip): the cell table built by brute force, the three candidate lists with the
product's host Philox (bark_amd.fitting._philox) under the search's key and counter, the neighbour layout, and the search loop
over an arbitrary acq(rows) -> values callable."""
import itertools

import numpy as np

from bark_amd.fitting._philox import philox4x32

CAT, INT, CONT = 0, 1, 2
KEY_XOR = 0x646F6D61
MODES = {"uniform": 0, "cells": 1, "grid": 2}


# ---- cell table -------------------------------------------------------------------------------------------------------------
def brute_table(forest, bounds, ft):
    """(cell_off, cell_rep) from a walk over every record, one feature at a time."""
    d = len(ft)
    thr = [[] for _ in range(d)]
    for node in np.asarray(forest).reshape(-1):
        if int(node["active"]) == 1 and int(node["is_leaf"]) == 0:
            thr[int(node["feature_idx"])].append(float(np.float64(node["threshold"])))
    off, rep = [0], []
    for f in range(d):
        lo, hi = float(bounds[f][0]), float(bounds[f][1])
        if ft[f] == CAT:
            mask = int(hi)
            if mask == 0:
                raise ValueError("zero mask")
            cells = [float(i) for i in range(64) if mask >> i & 1]
        elif ft[f] == INT:
            ilo, ihi = int(lo), int(hi)
            cuts = sorted({int(np.floor(t)) for t in thr[f] if np.isfinite(t) and ilo <= np.floor(t) < ihi})
            starts = [ilo] + [c + 1 for c in cuts]
            ends = cuts + [ihi]
            cells = [float((a + b) // 2) for a, b in zip(starts, ends)]
        elif lo == hi:
            cells = [lo]
        else:
            cuts = sorted({t for t in thr[f] if lo < t < hi})
            edges = [lo] + cuts + [hi]
            cells = []
            for a, b in zip(edges[:-1], edges[1:]):
                mid = 0.5 * (a + b)
                cells.append(mid if mid > a else b)
        rep += cells
        off.append(len(rep))
    return np.array(off, dtype=np.int64), np.array(rep, dtype=np.float64)


def cell_ranges(forest, bounds, ft):
    """Per table slot the closed range (first, last) of the cell's points that the tests probe: continuous (rep, upper end),
    integer (a, b), categorical (c, c)."""
    off, rep = brute_table(forest, bounds, ft)
    out = []
    for f in range(len(ft)):
        cells = rep[off[f]:off[f + 1]]
        lo, hi = float(bounds[f][0]), float(bounds[f][1])
        if ft[f] == CAT:
            out += [(c, c) for c in cells]
        elif ft[f] == INT:
            thr = sorted({int(np.floor(float(n["threshold"]))) for n in np.asarray(forest).reshape(-1)
                          if int(n["active"]) == 1 and int(n["is_leaf"]) == 0 and int(n["feature_idx"]) == f
                          and np.isfinite(n["threshold"]) and int(lo) <= np.floor(float(n["threshold"])) < int(hi)})
            out += list(zip([float(int(lo))] + [float(c + 1) for c in thr], [float(c) for c in thr] + [float(int(hi))]))
        else:
            thr = sorted({float(n["threshold"]) for n in np.asarray(forest).reshape(-1)
                          if int(n["active"]) == 1 and int(n["is_leaf"]) == 0 and int(n["feature_idx"]) == f
                          and lo < float(n["threshold"]) < hi})
            out += list(zip(cells, thr + [hi]))
    return out


# ---- candidate lists ----------------------------------------------------------------------------------------------------------
def uniforms(seed, round_, index, d):
    """(len(index), d) uniform doubles: row i's draw f is word pair f % 2 of block f // 2 under counter (i low, i high, round, block)."""
    index = np.asarray(index, dtype=np.uint64)
    blocks = (d + 1) // 2
    ctr = np.empty((index.shape[0], blocks, 4), dtype=np.uint64)
    ctr[..., 0] = (index & np.uint64(0xFFFFFFFF))[:, None]
    ctr[..., 1] = (index >> np.uint64(32))[:, None]
    ctr[..., 2] = np.uint64(round_)
    ctr[..., 3] = np.arange(blocks, dtype=np.uint64)[None, :]
    key = (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ KEY_XOR)
    words = philox4x32(key, ctr).astype(np.uint64).reshape(index.shape[0], blocks * 2, 2)
    x = words[..., 0] | (words[..., 1] << np.uint64(32))
    return ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)[:, :d]


def pick(u, n):
    return min(int(u * float(n)), n - 1)


def candidates(off, rep, bounds, ft, n, mode, seed, round_=0, first=0):
    d = len(off) - 1
    index = [first + i for i in range(n)]
    out = np.empty((n, d), dtype=np.float64)
    if mode == "grid":
        cells = [int(off[f + 1] - off[f]) for f in range(d)]
        for r, g in enumerate(index):
            for f in range(d - 1, -1, -1):
                g, digit = divmod(g, cells[f])
                out[r, f] = rep[off[f] + digit]
        return out
    u = uniforms(seed, round_, index, d)
    for r in range(n):
        for f in range(d):
            if mode == "cells":
                out[r, f] = rep[off[f] + pick(u[r, f], int(off[f + 1] - off[f]))]
                continue
            lo, hi = float(bounds[f][0]), float(bounds[f][1])
            if ft[f] == CAT:
                bits = [i for i in range(64) if int(hi) >> i & 1]
                out[r, f] = bits[pick(u[r, f], len(bits))]
            elif ft[f] == INT:
                out[r, f] = int(lo) + pick(u[r, f], int(hi) - int(lo) + 1)
            else:
                out[r, f] = min(lo + u[r, f] * (hi - lo), hi)
    return out


def grid_product(off, rep):
    """The whole grid by itertools.product, feature d - 1 fastest."""
    return np.array(list(itertools.product(*[rep[off[f]:off[f + 1]] for f in range(len(off) - 1)])), dtype=np.float64)


# ---- neighbours ---------------------------------------------------------------------------------------------------------------
def neighbours(off, rep, x):
    x = np.asarray(x, dtype=np.float64)
    K, d = x.shape
    J = len(rep)
    out = np.repeat(x, J, axis=0).reshape(K, J, d)
    for f in range(d):
        for j in range(int(off[f]), int(off[f + 1])):
            out[:, j, f] = rep[j]
    return out.reshape(K * J, d)


# ---- search loop ----------------------------------------------------------------------------------------------------------------
def search(acq, make_rows, off, rep, n_candidates, round_size, starts, max_sweeps):
    """make_rows(first, n) -> rows.  -> (x, info): the loop of `propose_from_domain` beyond its exhaustive branch."""
    best = {}  # row bytes -> (value, lowest index, row)
    for first in range(0, n_candidates, round_size):
        rows = make_rows(first, min(round_size, n_candidates - first))
        values = acq(rows)
        for i, (row, v) in enumerate(zip(rows, values)):
            best.setdefault(row.tobytes(), (float(v), first + i, row.copy()))
    ranked = sorted(best.values(), key=lambda t: (t[0], t[1]))[:starts]
    x = np.stack([t[2] for t in ranked])
    value = np.array([t[0] for t in ranked])
    start_values = value.copy()
    K, J = x.shape[0], len(rep)
    sweeps = 0
    for _ in range(max_sweeps):
        near = neighbours(off, rep, x)
        vals = np.asarray(acq(near)).reshape(K, J)
        sweeps += 1
        moved = False
        for k in range(K):
            j = int(np.argmin(vals[k]))  # the first of equal minima
            if vals[k, j] < value[k]:
                x[k], value[k], moved = near[k * J + j], vals[k, j], True
        if not moved:
            break
    k = int(np.argmin(value))
    return x[k].copy(), {"value": float(value[k]), "sweeps": sweeps, "start_values": start_values, "final_values": value}
