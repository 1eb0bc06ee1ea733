"""Extended-precision restatement of the density filter, W_ij = (r - d_ij) / sum_k (r - d_ik) over d_ij <= r, for the tests of
the device build at its edges (tests/test_gpu_filter_edges.py).  Brute force over all pairs in ``np.longdouble`` (64-bit
significand on x86-64), from the float64 coordinates as given: it shares no arithmetic, no grid and no ordering with the
kernels.  ``tests/elasticity_ref.filter_matrix`` (float64, scipy) stays the reference of the older tests."""
from typing import List, NamedTuple, Set, Tuple

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


class FilterRef(NamedTuple):
    n: int
    cols: List[np.ndarray]          # per row: the columns with d <= r, ascending (int64)
    weights: List[np.ndarray]       # per row: W_ij in longdouble, in the order of cols
    ties: Set[Tuple[int, int]]      # (i, j) with |d_ij - r| <= 8 eps r: float64 arithmetic may put them on either side

    def dense(self) -> np.ndarray:
        W = np.zeros((self.n, self.n), LD)
        for i in range(self.n):
            W[i, self.cols[i]] = self.weights[i]
        return W


def filter_matrix_ld(coords, radius, chunk=256) -> FilterRef:
    x = np.asarray(coords, dtype=np.float64).astype(LD)
    n = x.shape[0]
    r = LD(radius)
    tol = LD(8.0 * EPS) * r
    cols, weights, ties = [], [], set()
    for s in range(0, n, chunk):
        diff = x[s:s + chunk, None, :] - x[None, :, :]
        D = np.sqrt((diff * diff).sum(axis=2))
        for k in range(D.shape[0]):
            j = np.nonzero(D[k] <= r)[0]
            w = r - D[k, j]
            cols.append(j.astype(np.int64))
            weights.append(w / w.sum())
            for t in np.nonzero(np.abs(D[k] - r) <= tol)[0]:
                ties.add((s + k, int(t)))
    return FilterRef(n, cols, weights, ties)
