"""Float64 restatement of the Helmholtz (PDE) density filter (csrc/pde_filter.hip; include/femo_hip.h states it), written from
the formulas alone with SciPy sparse assembly:

  A = rt^2 L + M,  rt = r / (2 sqrt 3),  L_vw = sum_c |T_c| grad phi_v . grad phi_w,
  M lumped: M_vv = sum_{c around v} |T_c| / (d+1);  consistent: |T_c| (1 + delta_ab) / ((d+1)(d+2)) per cell,
  T[v,c] = |T_c| / (d+1),  V = diag |T_c|,  W = V^-1 T^T A^-1 T,  W^T = V W V^-1.

W and W^T come through ``splu``; ``pcg`` is the device's Jacobi-preconditioned CG step by step with its stopping test
sqrt(r^T D^-1 r) <= rtol sqrt(b^T D^-1 b) on the recurrence residual (femo_solve_cg, FEMO_PC_JACOBI).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

MASSES = ("lumped", "consistent")


def grads_and_volumes(x, conn):
    """Gradients of the barycentric coordinates (n_cell, d+1, d) and |T_c| (n_cell)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    p = x[conn]
    E = p[:, 1:, :] - p[:, :1, :]
    g = np.zeros((len(conn), d + 1, d))
    g[:, 1:, :] = np.transpose(np.linalg.inv(E), (0, 2, 1))
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    vol = np.abs(np.linalg.det(E)) / (2.0 if d == 2 else 6.0)
    return g, vol


def _scatter(conn, local, n):
    k = conn.shape[1]
    rows = np.repeat(conn, k, axis=1).ravel()
    cols = np.tile(conn, (1, k)).ravel()
    return sp.coo_matrix((local.ravel(), (rows, cols)), shape=(n, n)).tocsr()


def stiffness(x, conn):
    g, vol = grads_and_volumes(x, conn)
    return _scatter(conn, vol[:, None, None] * np.einsum("eak,ebk->eab", g, g), len(x))


def mass(x, conn, kind="lumped"):
    _, vol = grads_and_volumes(x, conn)
    d = np.asarray(x).shape[1]
    if kind == "lumped":
        local = vol[:, None, None] / (d + 1) * np.eye(d + 1)[None]
    elif kind == "consistent":
        local = vol[:, None, None] / ((d + 1) * (d + 2)) * (np.ones((d + 1, d + 1)) + np.eye(d + 1))[None]
    else:
        raise ValueError(kind)
    return _scatter(conn, local, len(x))


def transfer(x, conn):
    """T (n_vert x n_cell), T[v,c] = |T_c| / (d+1), and the cell volumes."""
    _, vol = grads_and_volumes(x, conn)
    k = conn.shape[1]
    rows = conn.ravel()
    cols = np.repeat(np.arange(len(conn)), k)
    return sp.coo_matrix((np.repeat(vol / k, k), (rows, cols)), shape=(len(x), len(conn))).tocsr(), vol


def operator(x, conn, radius, kind="lumped"):
    rt = radius / (2.0 * np.sqrt(3.0))
    return (rt * rt * stiffness(x, conn) + mass(x, conn, kind)).tocsr()


class Filter:
    """W and W^T of a mesh through a sparse LU of A."""

    def __init__(self, x, conn, radius, kind="lumped"):
        self.x, self.conn = np.asarray(x, dtype=np.float64), np.asarray(conn)
        self.A = operator(self.x, self.conn, radius, kind)
        self.T, self.vol = transfer(self.x, self.conn)
        self.lu = spla.splu(self.A.tocsc())

    def load(self, v, transpose=False):
        v = np.asarray(v, dtype=np.float64)
        return self.T @ (v / self.vol if transpose else v)

    def nodal(self, v, transpose=False):
        return self.lu.solve(self.load(v, transpose))

    def mean(self, p, transpose=False):
        y = (self.T.T @ p) / self.vol
        return y * self.vol if transpose else y

    def apply(self, v, transpose=False):
        return self.mean(self.nodal(v, transpose), transpose)

    def dense(self):
        n = len(self.conn)
        return np.stack([self.apply(e) for e in np.eye(n)], axis=1)


def pcg(A, b, rtol=1e-13, x0=None, max_it=10000):
    """Jacobi-preconditioned CG, the device's recurrence and stopping test.  Returns dict(x, iterations, converged)."""
    A = sp.csr_matrix(A)
    dinv = 1.0 / A.diagonal()
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x if x0 is not None else b.copy()
    tol2 = rtol * rtol * float(b @ (dinv * b))
    z = dinv * r
    gamma = float(r @ z)
    if not gamma > tol2:
        return dict(x=x, iterations=0, converged=1)
    p = z.copy()
    for it in range(1, max_it + 1):
        q = A @ p
        alpha = gamma / float(p @ q)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        gnew = float(r @ z)
        if not gnew > tol2:
            return dict(x=x, iterations=it, converged=1)
        p = z + (gnew / gamma) * p
        gamma = gnew
    return dict(x=x, iterations=max_it, converged=0)


def h_of(mesh_name):
    """The mesh size the radii of the tests are multiples of."""
    return {"rect8x4": 0.25, "square9j": 1.0 / 9, "cube4j": 0.25, "rect24x12": 1.0 / 12, "cube6j": 1.0 / 6, "fan40": 1.0,
            "rect48x24": 1.0 / 24}[mesh_name]
