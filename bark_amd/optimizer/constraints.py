"""Linear input constraints of a domain, as the reference's `propose` takes them from its BoFire domain (opt_core.py:90-99,
bofire_mixed/constraints.py:122-133): mixture sums, budgets, "a <= b" orderings.  Host only, numpy; `domain.py` passes what
`compiled` returns to the repair step on the device (csrc/domain.hip, bark_domain_repair_hip)."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ..forest import FeatureTypeEnum

MAX_CONSTRAINTS, MAX_TOUCHED = 16, 64  # limits of the repair step (include/bark_hip.h)


class CompiledConstraints(NamedTuple):
    """A in CSR with the columns of a row ascending, and what goes with it row by row."""
    row_ptr: np.ndarray   # (K + 1,) int64
    col: np.ndarray       # (nnz,) int64
    coef: np.ndarray      # (nnz,) float64
    b: np.ndarray         # (K,) float64
    tol: np.ndarray       # (K,) float64: tol (|b_k| + sum_f |A_kf| max(|lo_f|, |hi_f|))
    equality: np.ndarray  # (K,) uint8


class LinearConstraints:
    """Row k of A (K, d) means sum_f A[k, f] x_f <= b[k], or = b[k] where equality[k].  1 <= K <= 16 rows, at most 64 distinct
    features with a non-zero coefficient over all rows, every entry finite, no all-zero row: ValueError otherwise.  `tol` scales
    the slack of the final feasibility test (`compiled`)."""

    def __init__(self, A, b, equality=None, tol: float = 1e-12):
        self.A = np.atleast_2d(np.array(A, dtype=np.float64))
        self.b = np.array(b, dtype=np.float64).reshape(-1)
        K = self.A.shape[0]
        self.equality = np.zeros(K, dtype=bool) if equality is None else np.array(equality, dtype=bool).reshape(-1)
        self.tol = float(tol)
        if self.A.ndim != 2 or self.b.shape != (K,) or self.equality.shape != (K,):
            raise ValueError(f"A must be (K, d) with b and equality (K,), got {self.A.shape}, {self.b.shape}, {self.equality.shape}")
        if K < 1 or K > MAX_CONSTRAINTS:
            raise ValueError(f"1 to {MAX_CONSTRAINTS} constraints are taken (got {K})")
        if not (np.isfinite(self.A).all() and np.isfinite(self.b).all() and np.isfinite(self.tol) and self.tol >= 0):
            raise ValueError("A, b and tol must be finite (tol non-negative)")
        if not (self.A != 0).any(axis=1).all():
            raise ValueError(f"constraint {int(np.flatnonzero(~(self.A != 0).any(axis=1))[0])} has no non-zero coefficient")
        touched = int((self.A != 0).any(axis=0).sum())
        if touched > MAX_TOUCHED:
            raise ValueError(f"at most {MAX_TOUCHED} features may carry a non-zero coefficient (got {touched})")

    def compiled(self, bounds, feat_types) -> CompiledConstraints:
        """Checked against the domain: bounds (d, 2) — the ends of a categorical feature are not read — and feat_types (d,).
        ValueError for another d, a non-zero coefficient on a categorical feature, and an equality row with a non-zero
        coefficient on an integer feature."""
        bounds = np.asarray(bounds, dtype=np.float64)
        ft = np.asarray(feat_types, dtype=np.int64).reshape(-1)
        K, d = self.A.shape
        if ft.shape[0] != d or bounds.shape != (d, 2):
            raise ValueError(f"the constraints have {d} features, the domain {ft.shape[0]}")
        used = self.A != 0
        if used[:, ft == FeatureTypeEnum.Cat.value].any():
            raise ValueError("a constraint has a non-zero coefficient on a categorical feature")
        if used[self.equality][:, ft == FeatureTypeEnum.Int.value].any():
            raise ValueError("an equality constraint has a non-zero coefficient on an integer feature")
        reach = np.where(used.any(axis=0), np.abs(bounds).max(axis=1), 0.0)
        row, col = np.nonzero(used)  # row-major: ascending columns within a row
        row_ptr = np.zeros(K + 1, dtype=np.int64)
        row_ptr[1:] = np.cumsum(used.sum(axis=1))
        tol = self.tol * (np.abs(self.b) + np.abs(self.A) @ reach)
        return CompiledConstraints(row_ptr, col.astype(np.int64), np.ascontiguousarray(self.A[row, col]), self.b.copy(), tol,
                                   self.equality.astype(np.uint8))
