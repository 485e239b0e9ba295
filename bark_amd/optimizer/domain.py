"""Acquisition search over the whole domain: what the reference's `propose` does with a Gurobi model over the tree structure
(src/bark/optimizer/opt_core.py, opt_model.py, proposals.py), without a solver and without a candidate array from the caller.

A tree kernel's posterior is piecewise constant.  For every feature, the thresholds of all trees of all forest samples cut its
range into cells, and the acquisition takes one value on each product cell: the leaf codes of two points of a cell agree, so the
scan's value agrees bit for bit.  `split_table` lists one representative per cell (host, numpy).  The candidates are generated
on the device from that table (csrc/domain.hip) and scored by `acquisition_scan`:

* a cell grid of at most `exhaustive_limit` cells is enumerated, which gives the exact global minimiser — what the solver
  returns up to its MIP gap, at the cell's centre as `_get_leaf_center` does;
* a larger grid is searched from the best of `n_candidates` random candidates by coordinate-wise local search over the moves
  "one coordinate to another cell", all neighbours of all incumbents scored in one scan per sweep.

By default every scan rebuilds the leaf-space systems of the B forests.  `propose_from_domain(reuse_fit=True)` fits them once
(`tree_kernels.fit_posterior`) and runs every scan of the enumeration or the search from that state; `posterior=` takes a
state fitted by the caller (DESIGN.md section 8 has the measured difference).

Linear input constraints (`constraints.LinearConstraints`, `propose_from_domain(constraints=...)`) add one device step between
"write rows" and "scan rows": `domain_repair` moves every row inside its own cell (`cell_boxes`) to a point that satisfies them,
which leaves its acquisition value as it was bit for bit, or marks the row infeasible."""

from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np

from .. import _lib
from .constraints import LinearConstraints
from ..fitting.tree_proposals import check_bounds
from ..forest import FeatureTypeEnum, _as_nodes, _is_torch

MAX_FEATURES, MAX_CELLS = 4096, 1 << 20  # limits of the cell table (include/bark_hip.h)
MAX_NEIGHBOURS = 1 << 24                 # rows of one neighbour launch: the scan's candidate limit
MODES = {"uniform": _lib.DOMAIN_UNIFORM, "cells": _lib.DOMAIN_CELLS, "grid": _lib.DOMAIN_GRID}
CAT, INT = FeatureTypeEnum.Cat.value, FeatureTypeEnum.Int.value


class CellTable(NamedTuple):
    """Feature f owns cell_rep[cell_off[f]:cell_off[f + 1]], its cells in ascending order."""
    cell_off: np.ndarray  # (d + 1,) int64
    cell_rep: np.ndarray  # (total,) float64


def _feature_cells(kind: int, lo: float, hi: float, thresholds: np.ndarray) -> np.ndarray:
    """The representatives of one feature.  The walk sends x left where x <= float64(float32 threshold)
    (csrc/traverse.hip), a categorical x where its bit of the mask is set."""
    if kind == CAT:
        mask = int(hi)
        if mask <= 0:
            raise ValueError("a categorical feature has no category (zero mask)")
        return np.array([i for i in range(mask.bit_length()) if mask >> i & 1], dtype=np.float64)
    if kind == INT:
        ilo, ihi = int(lo), int(hi)
        t = thresholds[(thresholds >= ilo) & (thresholds < ihi + 1)]  # NaN and +-inf drop out here
        cuts = np.unique(np.floor(t).astype(np.int64))
        cuts = cuts[(cuts >= ilo) & (cuts < ihi)]
        a = np.concatenate(([ilo], cuts + 1))
        b = np.concatenate((cuts, [ihi]))
        return ((a + b) // 2).astype(np.float64)
    cuts = np.unique(thresholds[(thresholds > lo) & (thresholds < hi)])
    if lo == hi:
        return np.array([lo], dtype=np.float64)
    a = np.concatenate(([lo], cuts))
    b = np.concatenate((cuts, [hi]))
    mid = 0.5 * (a + b)
    return np.where(mid > a, mid, b)


def split_table(forest, bounds, feat_types) -> CellTable:
    """The cell table of forest records of any leading shape (…, node_limit) inside `bounds` (d, 2) / `feat_types` (d,), as
    `fitting.tree_proposals.check_bounds` accepts them.  Only nodes with active == 1 and is_leaf == 0 are read.

    continuous: boundaries are the distinct float64(threshold) with lo < t < hi; cells (lo, t1], (t1, t2], …, (tT, hi] (the first
    also holds lo); the representative is 0.5 (a + b), or b where that does not exceed a; lo == hi is one cell {lo}.
    integer: boundaries are the distinct floor(t) with lo <= floor(t) < hi; cells [lo, b1], [b1 + 1, b2], …, [bT + 1, hi]; the
    representative is (a + b) // 2.  categorical: one cell per set bit of the mask, in bit order; a zero mask is a ValueError.
    ValueError past 4096 features or 2^20 cells."""
    b, ft = check_bounds(bounds, feat_types)
    d = int(ft.shape[0])
    if d < 1 or d > MAX_FEATURES:
        raise ValueError(f"the cell table takes 1 to {MAX_FEATURES} features (got {d})")
    nodes = _as_nodes(forest, 1).reshape(-1)
    split = nodes[(nodes["active"] == 1) & (nodes["is_leaf"] == 0)]
    feature = split["feature_idx"].astype(np.int64)
    if feature.size and feature.max() >= d:
        raise ValueError(f"a split reads feature {int(feature.max())} of {d}")
    thr = split["threshold"].astype(np.float64)
    reps = [_feature_cells(int(ft[f]), float(b[f, 0]), float(b[f, 1]), thr[feature == f]) for f in range(d)]
    off = np.zeros(d + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in reps])
    if off[-1] > MAX_CELLS:
        raise ValueError(f"the cell table holds at most 2^20 cells over all features (got {int(off[-1])})")
    return CellTable(off, np.ascontiguousarray(np.concatenate(reps), dtype=np.float64))


class CellBoxes(NamedTuple):
    """Feature f owns the slots cell_off[f]:cell_off[f + 1], as in `CellTable`: cell j is the closed interval [cell_lo[j], cell_hi[j]]."""
    cell_off: np.ndarray  # (d + 1,) int64
    cell_lo: np.ndarray   # (total,) float64
    cell_hi: np.ndarray   # (total,) float64


def _feature_boxes(kind: int, lo: float, hi: float, thresholds: np.ndarray):
    """(cell_lo, cell_hi) of one feature, the cells of `_feature_cells` in its order."""
    if kind == CAT:
        cats = _feature_cells(kind, lo, hi, thresholds)
        return cats, cats
    if kind == INT:
        ilo, ihi = int(lo), int(hi)
        t = thresholds[(thresholds >= ilo) & (thresholds < ihi + 1)]
        cuts = np.unique(np.floor(t).astype(np.int64))
        cuts = cuts[(cuts >= ilo) & (cuts < ihi)]
        return np.concatenate(([ilo], cuts + 1)).astype(np.float64), np.concatenate((cuts, [ihi])).astype(np.float64)
    if lo == hi:
        return np.array([lo], dtype=np.float64), np.array([lo], dtype=np.float64)
    cuts = np.unique(thresholds[(thresholds > lo) & (thresholds < hi)])
    return np.concatenate(([lo], np.nextafter(cuts, np.inf))), np.concatenate((cuts, [hi]))


def cell_boxes(forest, bounds, feat_types) -> CellBoxes:
    """The usable closed interval of every cell of `split_table(forest, bounds, feat_types)`, same offsets, same order: every
    point of [cell_lo, cell_hi] walks every tree as the cell's representative does.

    continuous cell (a, b]: hi = b; lo = a for the feature's first cell (which holds the domain's lower bound), otherwise
    nextafter(a, +inf), which still goes right at the threshold a (x <= thr goes left).  integer cell: its integer ends.
    categorical cell: lo = hi = the category.  lo == hi: one degenerate cell."""
    b, ft = check_bounds(bounds, feat_types)
    d = int(ft.shape[0])
    if d < 1 or d > MAX_FEATURES:
        raise ValueError(f"the cell table takes 1 to {MAX_FEATURES} features (got {d})")
    nodes = _as_nodes(forest, 1).reshape(-1)
    split = nodes[(nodes["active"] == 1) & (nodes["is_leaf"] == 0)]
    feature = split["feature_idx"].astype(np.int64)
    if feature.size and feature.max() >= d:
        raise ValueError(f"a split reads feature {int(feature.max())} of {d}")
    thr = split["threshold"].astype(np.float64)
    boxes = [_feature_boxes(int(ft[f]), float(b[f, 0]), float(b[f, 1]), thr[feature == f]) for f in range(d)]
    off = np.zeros(d + 1, dtype=np.int64)
    off[1:] = np.cumsum([lo.shape[0] for lo, _ in boxes])
    if off[-1] > MAX_CELLS:
        raise ValueError(f"the cell table holds at most 2^20 cells over all features (got {int(off[-1])})")
    return CellBoxes(off, np.ascontiguousarray(np.concatenate([lo for lo, _ in boxes]), dtype=np.float64),
                     np.ascontiguousarray(np.concatenate([hi for _, hi in boxes]), dtype=np.float64))


def domain_plan(table: CellTable) -> dict:
    """{"cells": cells per feature (d,) int64, "grid": their product (a Python int: it can pass 2^64), "neighbours": rows of
    `domain_neighbours` per point = the table's total}.  Host only."""
    cells = np.diff(np.asarray(table.cell_off, dtype=np.int64))
    return {"cells": cells, "grid": math.prod(int(c) for c in cells), "neighbours": int(cells.sum())}


class _DeviceTable:
    """The table, the bounds and the feature types on the device: uploaded once per search."""

    def __init__(self, table: CellTable, bounds=None, feat_types=None):
        off = np.ascontiguousarray(table.cell_off, dtype=np.int64)
        rep = np.ascontiguousarray(table.cell_rep, dtype=np.float64)
        if off.ndim != 1 or off.shape[0] < 2 or rep.ndim != 1 or off[0] != 0 or off[-1] != rep.shape[0] or (np.diff(off) < 1).any():
            raise ValueError("not a cell table: cell_off must rise from 0 to len(cell_rep), one cell or more per feature")
        self.d, self.total = int(off.shape[0]) - 1, int(rep.shape[0])
        if self.d > MAX_FEATURES or self.total > MAX_CELLS:
            raise ValueError(f"the cell table takes at most {MAX_FEATURES} features and 2^20 cells")
        self.off, self.rep = _lib.to_device(off), _lib.to_device(rep)
        self.bounds = self.ft = None
        if bounds is not None:
            b, ft = check_bounds(bounds, feat_types)
            if ft.shape[0] != self.d:
                raise ValueError(f"bounds have {ft.shape[0]} features, the table {self.d}")
            self.bounds, self.ft = _lib.to_device(b), _lib.to_device(ft)

    def candidates(self, n: int, mode: str, seed: int, round: int, first: int):
        import torch

        if mode not in MODES:
            raise ValueError(f"unknown mode {mode!r} (use 'uniform', 'cells' or 'grid')")
        if mode == "uniform" and self.bounds is None:
            raise ValueError("mode 'uniform' needs bounds and feat_types")
        n = int(n)
        out = torch.empty((max(n, 0), self.d), dtype=torch.float64, device=self.rep.device)
        _lib.check(_lib.lib().bark_domain_candidates_hip(
            _lib.ptr(self.off), _lib.ptr(self.rep), self.total, _lib.ptr(self.bounds), _lib.ptr(self.ft), self.d, MODES[mode],
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(round), int(first), n, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def neighbours(self, x):
        import torch

        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"x must be (K, {self.d}), got {tuple(x.shape)}")
        K = int(x.shape[0])
        if K * self.total > MAX_NEIGHBOURS:  # before the output is allocated; the entry point refuses it too
            raise ValueError(f"{K} points x {self.total} cells exceed the scan's 2^24 candidates")
        x = x.to(torch.float64).contiguous()
        out = torch.empty((K * self.total, self.d), dtype=torch.float64, device=self.rep.device)
        _lib.check(_lib.lib().bark_domain_neighbours_hip(_lib.ptr(self.off), _lib.ptr(self.rep), self.total, self.d, _lib.ptr(x), K,
                                                         _lib.ptr(out), _lib.stream_ptr()))
        return out


class _DeviceBoxes:
    """The cell boxes, the feature types and the compiled constraints on the device: uploaded once per search."""

    def __init__(self, boxes: CellBoxes, feat_types, constraints: LinearConstraints, passes: int = 4):
        off = np.ascontiguousarray(boxes.cell_off, dtype=np.int64)
        lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (boxes.cell_lo, boxes.cell_hi))
        if (off.ndim != 1 or off.shape[0] < 2 or lo.ndim != 1 or lo.shape != hi.shape or off[0] != 0 or off[-1] != lo.shape[0]
                or (np.diff(off) < 1).any()):
            raise ValueError("not cell boxes: cell_off must rise from 0 to len(cell_lo) == len(cell_hi), one cell or more per feature")
        self.d, self.total = int(off.shape[0]) - 1, int(lo.shape[0])
        if self.d > MAX_FEATURES or self.total > MAX_CELLS:
            raise ValueError(f"the cell table takes at most {MAX_FEATURES} features and 2^20 cells")
        if not isinstance(constraints, LinearConstraints):
            raise ValueError("constraints must be a LinearConstraints")
        self.passes = int(passes)
        if self.passes < 1 or self.passes > 64:
            raise ValueError(f"passes must lie in [1, 64], got {passes}")
        ft = np.ascontiguousarray(feat_types, dtype=np.int64).reshape(-1)
        ends = np.stack((lo[off[:-1]], hi[off[1:] - 1]), axis=1)  # the feature's range: its first cell's lo, its last cell's hi
        self.compiled = c = constraints.compiled(ends, ft)
        self.K = int(c.b.shape[0])
        self.off, self.lo, self.hi, self.ft = (_lib.to_device(a) for a in (off, lo, hi, ft))
        self.row_ptr, self.col, self.coef, self.b, self.tol, self.eq = (_lib.to_device(a) for a in c)

    def repair(self, rows):
        """rows (n, d) float64 device tensor, contiguous, repaired IN PLACE -> (rows, feasible (n,) bool)."""
        import torch

        if rows.ndim != 2 or rows.shape[1] != self.d or rows.dtype != torch.float64 or not rows.is_contiguous():
            raise ValueError(f"rows must be a contiguous (n, {self.d}) float64 tensor, got {tuple(rows.shape)} {rows.dtype}")
        n = int(rows.shape[0])
        ok = torch.empty(n, dtype=torch.uint8, device=rows.device)
        _lib.check(_lib.lib().bark_domain_repair_hip(
            _lib.ptr(self.off), _lib.ptr(self.lo), _lib.ptr(self.hi), self.total, _lib.ptr(self.ft), self.d, _lib.ptr(self.row_ptr),
            _lib.ptr(self.col), _lib.ptr(self.coef), _lib.ptr(self.b), _lib.ptr(self.tol), _lib.ptr(self.eq), self.K, self.passes,
            _lib.ptr(rows), n, _lib.ptr(ok), _lib.stream_ptr()))
        return rows, ok.bool()


def domain_repair(boxes: CellBoxes, feat_types, constraints: LinearConstraints, rows, passes: int = 4):
    """rows (n, d), numpy or torch -> (repaired rows (n, d) float64, feasible (n,) bool), device tensors; the caller's rows are
    not modified (bark_domain_repair_hip).  Every row is moved inside its own cell of `boxes` — only along features with a
    non-zero coefficient, the others are neither read nor written — until every constraint holds: up to `passes` rounds over
    the constraints in order, each violated one shifting its coordinates in feature order, clamped to the cell.

    A row marked feasible satisfies every constraint within tol_k and lies in its original cell, so its acquisition value is
    unchanged bit for bit.  When the rows of A have pairwise disjoint supports, every cell that passes the closed box test is
    marked feasible; with overlapping supports the repair is a heuristic that can miss feasible cells.  A row outside every
    cell, or with a NaN in a touched column, is infeasible and unchanged; other infeasible rows hold what the passes left."""
    import torch

    dev = _DeviceBoxes(boxes, feat_types, constraints, passes)
    xd = rows.to(_lib.torch_device()) if _is_torch(rows) else _lib.to_device(np.asarray(rows, dtype=np.float64))
    return dev.repair(xd.to(torch.float64).contiguous().clone())


def domain_candidates(table: CellTable, bounds, feat_types, n: int, mode: str, seed: int, round: int = 0, first: int = 0):
    """Rows first … first + n - 1 of the candidate list `mode` as an (n, d) float64 device tensor (bark_domain_candidates_hip):
    "uniform" draws in the box (integers and categories uniform over their values), "cells" one cell per feature uniformly —
    over cells, not volume, so the small cells near the data are represented — and "grid" enumerates the product of the cells
    in itertools.product order (no draws; keep first + n within `domain_plan(table)["grid"]`).  A row depends on (seed, round,
    row index) only.  bounds / feat_types may be None unless mode is "uniform"."""
    return _DeviceTable(table, bounds, feat_types).candidates(n, mode, seed, round, first)


def domain_neighbours(table: CellTable, x):
    """x (K, d), numpy or torch -> (K * total, d) float64 device tensor: row k * total + j is x[k] with the feature that owns
    table slot j moved to cell_rep[j] (bark_domain_neighbours_hip).  Moves inside the point's own cell are kept.  ValueError
    past 2^24 rows."""
    xd = x.to(_lib.torch_device()) if _is_torch(x) else _lib.to_device(np.asarray(x, dtype=np.float64))
    return _DeviceTable(table).neighbours(xd)


def _by_value_then_index(values, index):
    """Order of ascending (value, index); NaN values last."""
    import torch

    first = torch.argsort(index, stable=True)
    return first[torch.argsort(values[first], stable=True)]


def _best_distinct(rows, values, index, k: int):
    """The k best distinct rows by (value, lowest index of the row): -> rows, values, index, ordered."""
    import torch

    uniq, inverse = torch.unique(rows, dim=0, return_inverse=True)
    n = int(uniq.shape[0])
    lowest = torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=rows.device)
    lowest.scatter_reduce_(0, inverse, index, "amin")
    is_first = index == lowest[inverse]  # one occurrence per distinct row: the indices are distinct
    at = torch.empty(n, dtype=torch.int64, device=rows.device)
    at[inverse[is_first]] = torch.arange(rows.shape[0], device=rows.device)[is_first]
    order = _by_value_then_index(values[at], lowest)[:k]
    return uniq[order], values[at][order], lowest[order]


def _first_argmin(values):
    """(min, first index of it) along the last dim, the tie rule spelled out; a NaN in a row gives NaN and the last index."""
    import torch

    low = values.amin(-1)
    n = values.shape[-1]
    where = torch.where(values == low.unsqueeze(-1), torch.arange(n, device=values.device), n).amin(-1)
    return low, where.clamp(max=n - 1)


def local_search(acq, candidates, neighbours, n_candidates: int, round_size: int, starts: int, max_sweeps: int, repair=None):
    """The search loop on torch tensors of any device, over three callables: acq(rows (n, d)) -> values (n,),
    candidates(first, n) -> rows, neighbours(x (K, d)) -> (K J, d) in the layout of `domain_neighbours`.
    -> (x (d,), info as `propose_from_domain` documents it, without "grid" and "exhaustive").

    repair(rows) -> (rows, feasible (n,) bool), when given, runs on every candidate and neighbour array before it is scored:
    incumbents come from feasible rows only, an infeasible neighbour counts +inf.  ValueError("no feasible cell") when no
    candidate is feasible."""
    import torch

    top = None
    scans = 0
    for first in range(0, n_candidates, round_size):
        n = min(round_size, n_candidates - first)
        rows = candidates(first, n)
        feasible = None
        if repair is not None:
            rows, feasible = repair(rows)
        values = acq(rows)
        scans += 1
        index = torch.arange(first, first + n, dtype=torch.int64, device=rows.device)
        if feasible is not None:
            rows, values, index = rows[feasible], values[feasible], index[feasible]
            if rows.shape[0] == 0:
                continue
        if top is not None:
            rows, values, index = torch.cat((top[0], rows)), torch.cat((top[1], values)), torch.cat((top[2], index))
        top = _best_distinct(rows, values, index, starts)
    if top is None:
        raise ValueError("no feasible cell")
    x, value = top[0].clone(), top[1].clone()
    start_values = value.clone()
    K, d = x.shape
    sweeps = 0
    for _ in range(max_sweeps):
        near = neighbours(x)
        if repair is None:
            near_values = acq(near)
        else:
            near, feasible = repair(near)
            near_values = torch.where(feasible, acq(near), math.inf)
        low, j = _first_argmin(near_values.reshape(K, -1))
        scans += 1
        sweeps += 1
        moved = low < value  # strictly lower; a NaN never moves a point
        x = torch.where(moved.unsqueeze(1), near.reshape(K, -1, d)[torch.arange(K, device=x.device), j], x)
        value = torch.where(moved, low, value)
        if not bool(moved.any()):
            break
    _, best = _first_argmin(value)
    info = {"value": float(value[best]), "sweeps": sweeps, "scans": scans, "index": -1,
            "start_values": start_values.cpu().numpy(), "final_values": value.cpu().numpy()}
    return x[best].cpu().numpy(), info


def propose_from_domain(model, data, bounds, feat_types, kappa: float = 1.96, kind: str = "lcb_mean", n_candidates: int = 2 ** 18,
                        round_size: int = 2 ** 18, starts: int = 8, max_sweeps: int = 32, exhaustive_limit: int = 2 ** 22,
                        mode: str = "cells", seed: int = 0, pending=None, targets=None, chunk=None, variant: str = "auto",
                        return_info: bool = False, posterior=None, reuse_fit: bool = False, constraints=None, passes: int = 4):
    """-> x (d,) numpy float64: the point of the domain `bounds` / `feat_types` that minimises the acquisition, the reference's
    `propose` without its solver.  model, data, kind, kappa, pending and targets mean what they mean to `acquisition_scan`,
    through which every evaluation goes.  With return_info: (x, info).

    The cell grid of the model's forests (`split_table`, `domain_plan`) is enumerated when it has at most `exhaustive_limit`
    cells, in rounds of `round_size` rows: x is then the exact global minimiser, the first in grid order among equals.
    Otherwise `n_candidates` rows of `mode` ("cells" or "uniform", drawn with `seed`) are scanned, the `starts` best distinct
    rows (by value, then row index) become incumbents, and up to `max_sweeps` sweeps move every incumbent to its best
    neighbour (`domain_neighbours`; ties: the lowest slot) while that is strictly lower; x is the best incumbent (ties: the
    better start).  The result does not depend on `round_size`, and a seed gives the same x every time.

    reuse_fit=True fits the leaf-space posterior once (`tree_kernels.fit_posterior(model, data, feat_types, chunk)`), conditions
    it once on `pending`, and runs every scan from that state: the same x and the same value, bit for bit, without a
    factorisation per scan.  posterior: a `LeafPosterior` of the caller's to start from instead (it is not modified); `model`
    and `data` may then be None.  The default fits per scan, as before.

    info: "value" (the acquisition at x), "exhaustive", "grid" (cells of the grid, a Python int), "index" (x's row of the grid,
    -1 after a search), "sweeps", "scans" (calls of `acquisition_scan`), "fits" (factorisations of the B leaf-space systems:
    the number of scans by default, 1 with reuse_fit, 0 with `posterior`), "start_values" and "final_values" (one per
    incumbent, `starts` of them unless the candidates hold fewer distinct rows; empty when exhaustive).

    constraints: a `LinearConstraints` over the features (continuous and integer ones; DESIGN.md section 8 has the algorithm and
    its limits).  Every array of rows — a round of the grid, the candidates, the neighbours — is then repaired on the device
    before it is scored (`domain_repair`, `passes` rounds): moved inside its own cell, which does not change its value, to a
    point that satisfies them, or marked infeasible.  The enumeration scans the feasible rows of a round only and maps the
    winner back to its grid index (ties: the lowest); the search takes its incumbents from feasible candidates and counts an
    infeasible neighbour +inf.  x is the repaired row: it satisfies the constraints itself.  Exact over the cells when the
    constraints' supports are pairwise disjoint; with overlapping supports feasible cells can be missed, an infeasible x is
    never returned.  ValueError("no feasible cell") when nothing is feasible.  info then also holds "rows" (rows repaired) and
    "feasible" (those that passed).  With constraints=None nothing of this runs.

    ValueError when starts times the table's total exceeds the scan's 2^24 candidates, and for what `acquisition_scan` and
    `split_table` refuse.  No CPU fallback."""
    import torch

    from .acquisition import _fitted, acquisition_scan

    n_candidates, round_size, starts, max_sweeps = int(n_candidates), int(round_size), int(starts), int(max_sweeps)
    if round_size < 1 or round_size > MAX_NEIGHBOURS:
        raise ValueError(f"round_size must lie in [1, 2^24] (the scan's candidate limit), got {round_size}")
    if n_candidates < 1 or starts < 1 or max_sweeps < 0:
        raise ValueError("n_candidates and starts must be positive, max_sweeps non-negative")
    if mode not in ("cells", "uniform"):
        raise ValueError(f"unknown mode {mode!r} (use 'cells' or 'uniform')")
    b, ft = check_bounds(bounds, feat_types)
    if posterior is not None:
        posterior = _fitted(posterior, ft)
    table = split_table(model[0] if posterior is None else posterior.live_forest, b, ft)  # weight-0 forests cut no cell
    plan = domain_plan(table)
    dev = _DeviceTable(table, b, ft)
    repair, counts = None, None
    if constraints is not None:
        forest = model[0] if posterior is None else posterior.live_forest
        boxes = _DeviceBoxes(cell_boxes(forest, b, ft), ft, constraints, passes)
        counts = torch.zeros(2, dtype=torch.int64, device=dev.rep.device)  # rows repaired, rows feasible

        def repair(rows):
            rows, feasible = boxes.repair(rows)
            counts[0] += rows.shape[0]
            counts[1] += feasible.sum()
            return rows, feasible
    scan = dict(kappa=kappa, kind=kind, chunk=chunk, variant=variant, pending=pending, targets=targets)
    fits = None  # one per scan
    if posterior is not None or reuse_fit:
        from ..tree_kernels.posterior import fit_posterior

        fits = 0 if posterior is not None else 1
        if posterior is None:
            posterior = fit_posterior(model, data, ft, chunk=chunk)
        if pending is not None and len(pending):
            posterior = posterior.condition(pending)  # once per search; the caller's state stays as it is
        scan.update(pending=None, posterior=posterior)

    if plan["grid"] <= exhaustive_limit:
        grid = plan["grid"]
        best = torch.full((), math.inf, dtype=torch.float64, device=dev.rep.device)
        best_i = torch.full((), -1, dtype=torch.int64, device=dev.rep.device)
        best_row = torch.full((dev.d,), math.nan, dtype=torch.float64, device=dev.rep.device)
        scans = 0
        for first in range(0, grid, round_size):
            rows = dev.candidates(min(round_size, grid - first), "grid", 0, 0, first)
            if repair is not None:
                rows, feasible = repair(rows)
                kept = torch.nonzero(feasible).squeeze(1)  # ascending: the compacted rows stay in grid order
                if kept.shape[0] == 0:
                    continue
                rows = rows[kept]
            value, index = acquisition_scan(model, data, rows, ft, **scan)
            scans += 1
            better = value < best  # rounds run in grid order: equal values keep the lower index; (NaN, -1) never wins
            best_row = torch.where(better, rows[index.clamp(min=0)], best_row)
            best_i = torch.where(better, (index if repair is None else kept[index.clamp(min=0)]) + first, best_i)
            best = torch.where(better, value, best)
        x, at = best_row.cpu().numpy(), int(best_i)
        if counts is not None and int(counts[1]) == 0:
            raise ValueError("no feasible cell")
        if at < 0:
            raise RuntimeError("the acquisition is NaN on every cell of the grid")
        info = {"value": float(best), "exhaustive": True, "grid": grid, "index": at, "sweeps": 0, "scans": scans,
                "fits": scans if fits is None else fits, "start_values": np.empty(0), "final_values": np.empty(0)}
        if counts is not None:
            info["rows"], info["feasible"] = (int(c) for c in counts.cpu())
        return (x, info) if return_info else x

    if starts * plan["neighbours"] > MAX_NEIGHBOURS:
        raise ValueError(f"{starts} starts x {plan['neighbours']} cells exceed the scan's 2^24 candidates: use fewer starts")
    x, info = local_search(
        lambda rows: acquisition_scan(model, data, rows, ft, return_values=True, **scan)[2],
        lambda first, n: dev.candidates(n, mode, seed, 0, first), dev.neighbours, n_candidates, round_size, starts, max_sweeps,
        repair)
    info.update(exhaustive=False, grid=plan["grid"], fits=info["scans"] if fits is None else fits)
    if counts is not None:
        info["rows"], info["feasible"] = (int(c) for c in counts.cpu())
    return (x, info) if return_info else x
