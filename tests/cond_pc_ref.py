"""NumPy / SciPy restatement of the lattice preconditioner of the penalised heat conduction solves (csrc/conduction.hip:
k_cond_pc_diag, csrc/bpx.hip: pc_prepare), written from the definition alone:

    M^-1 = D^-1 + sum_l P_l C_l P_l^T
    C_l[I] = keep_l[I] theta / G_l[I]      (0 where G_l[I] == 0),   theta = 0.6
    G_l[I] = (Pt_l^T A Pt_l)_II = sum_c k(rho_c) |T_c| | sum_{a in c} w_aI free_a grad lambda_a |^2

  A      the operator that is solved: K_theta(rho) with identity rows / columns on the pinned vertices, the plain K_theta
         without a Dirichlet set (tests/thermal_ref.py supplies K_theta)
  Pt_l   multilinear interpolation from lattice l straight to the vertices with exact fp64 weights w_aI (no packed
         fractions, no single-precision 1/s), zero rows on pinned vertices (free_a)
  P_l, the lattice plan, the packed coordinates, the single-precision scaling and keep_l are those of
         oracle/bpx_oracle.py: `WeightedBPX` subclasses `bpx_oracle.BPX` and replaces coef[l], nothing else

G_l is formed two ways: by the sparse triple product (`galerkin_diagonal`) and cell by cell from the closed form
(`cell_diagonal`, the way the device forms it), so that the two derivations check each other.  The weights come from the
closed form: it gives an exact zero where no free vertex reaches a node, which the triple product does only to rounding.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import scipy.sparse as sp

import thermal_ref as tr
from oracle import bpx_oracle as bo

K0, K_MIN = 1.0, 1e-3


def eliminated(K, pinned):
    """K with zero rows / columns and a unit diagonal on the pinned vertices (pinned: bool per vertex, or None)."""
    if pinned is None or not np.any(pinned):
        return K.tocsr()
    free = sp.diags(np.where(pinned, 0.0, 1.0))
    return (free @ K @ free + sp.diags(np.where(pinned, 1.0, 0.0))).tocsr()


def exact_interpolation(M: bo.BPX, x, level):
    """Pt_l: n_vert x nodes[l], exact fp64 weights, zero rows on pinned vertices."""
    return (sp.diags(M.free) @ bo.interpolation(x, M.lo, M.hi, M.bins[level], quantise=False)).tocsr()


def galerkin_diagonal(M: bo.BPX, x, A, level):
    """diag(Pt_l^T A Pt_l) by sparse products."""
    P = exact_interpolation(M, x, level)
    return np.asarray((P.T @ A @ P).diagonal())


def cell_gradients(x, conn):
    """(n_cell, d + 1, d) gradients of the barycentric coordinates and (n_cell,) volumes."""
    d = x.shape[1]
    p = x[conn]
    J = p[:, 1:] - p[:, :1]                          # rows: edge vectors
    Jinv = np.linalg.inv(J)
    g = np.zeros((len(conn), d + 1, d))
    g[:, 1:] = np.transpose(Jinv, (0, 2, 1))
    g[:, 0] = -g[:, 1:].sum(axis=1)
    return g, np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)


def cell_diagonal(M: bo.BPX, x, conn, kc, level):
    """G_l from the closed form: cell c adds k_c |T_c| |g_I|^2, g_I = sum_a w_aI free_a grad lambda_a, to every node I of
    its bin range on level l whose g_I is not exactly zero (a jittered cell straddles lattice lines: the range is not
    2^d nodes)."""
    d = x.shape[1]
    n = M.bins[level]
    b, t = bo._locate(x, M.lo, M.hi, n, quantise=False)
    g, vol = cell_gradients(x, conn)
    cb, ct, cf = b[conn], t[conn], M.free[conn]      # (n_cell, d + 1, d), (n_cell, d + 1)
    ilo, ihi = cb.min(axis=1), cb.max(axis=1) + 1    # node range per axis, inclusive
    span = int((ihi - ilo).max())
    stride = np.concatenate([[1], np.cumprod(n[:-1] + 1)])
    G = np.zeros(int(np.prod(n + 1)))
    for off in itertools.product(range(span + 1), repeat=d):
        node = ilo + np.array(off)                   # (n_cell, d)
        inside = np.all(node <= ihi, axis=1)
        w = cf.copy()
        for k in range(d):
            nk = node[:, None, k]
            w = w * np.where(nk == cb[:, :, k], 1.0 - ct[:, :, k], np.where(nk == cb[:, :, k] + 1, ct[:, :, k], 0.0))
        gI = np.einsum("ca,cak->ck", w, g)
        gg = (gI * gI).sum(axis=1)
        use = inside & (gg != 0.0)
        np.add.at(G, (node[use] * stride).sum(axis=1), (kc * vol * gg)[use])
    return G


class WeightedBPX(bo.BPX):
    """`bpx_oracle.BPX` of the operator A (K_theta eliminated with `pinned`) with C_l = keep_l theta / G_l."""

    def __init__(self, x, conn, kc, K, pinned=None, A=None):
        """``A``: the operator as the device holds it (its diagonal then carries the device's rounding into the
        single-precision scaling of `bpx_oracle.BPX`); default: K eliminated with ``pinned``."""
        x = np.asarray(x, float)
        self.A = eliminated(K, pinned) if A is None else A.tocsr()
        super().__init__(x, self.A.diagonal(), pinned)
        self.stock = [c.copy() for c in self.coef]
        self.G = [cell_diagonal(self, x, conn, kc, l) for l in range(self.levels)]
        for l in range(self.levels):
            keep, G = self.stock[l] != 0.0, self.G[l]
            with np.errstate(divide="ignore"):
                self.coef[l] = np.where(keep & (G != 0.0), bo.THETA / G, 0.0)


class Jacobi:
    """D^-1 with the interface `bpx_oracle.pcg` uses."""

    def __init__(self, diag):
        self.dinv = 1.0 / np.asarray(diag, float)

    def apply(self, r):
        return self.dinv * r


def pinned_mask(n_vert, sink):
    m = np.zeros(n_vert, dtype=bool)
    m[np.asarray(sink, dtype=np.int64)] = True
    return m


def sink_of(mesh):
    """The vertices on x = 0 (tests/test_gpu_conduction.py: _sink)."""
    return np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0].astype(np.int32)


def small_case(name, method="SIMP", seed=7, with_sink=True):
    """A mesh of thermal_ref.MESHES with random rho in [0.05, 1]: dict(mesh, rho, K, pinned, M, Q, b)."""
    mesh = tr.mesh(name)
    rho = np.random.default_rng(seed).uniform(0.05, 1.0, mesh.n_cell)
    return make_case(mesh, rho, method, with_sink)


def make_case(mesh, rho, method="SIMP", with_sink=True, k_min=K_MIN):
    kc = tr.conductivity(rho, K0, k_min, method)
    K = tr.conduction_matrix(mesh.x, mesh.conn, kc)
    sink = sink_of(mesh) if with_sink else np.zeros(0, np.int32)
    pinned = pinned_mask(mesh.n_vert, sink) if with_sink else None
    M = WeightedBPX(mesh.x, mesh.conn, kc, K, pinned)
    Q = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    b = Q.copy()
    b[sink] = 0.0                                     # the lifting of a zero sink temperature
    return dict(mesh=mesh, rho=rho, kc=kc, K=K, sink=sink, pinned=pinned, M=M, Q=Q, b=b)


# ------------------------------------------------------------------------------------- the cases of the count tests ----
COUNT_RTOL = 1e-13


@functools.lru_cache(maxsize=None)
def count_mesh(nelx, nely):
    from femo_amd.fea.mesh import createRectangleMesh
    return createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), nelx, nely)


@functools.lru_cache(maxsize=None)
def count_case(nelx, nely, kind):
    """The 2:1 cantilever box of the count tables (scripts/bench_topopt.py: conduction_counts): k0 = 1, k_min = 1e-3, SIMP, the
    sink on x = 0, a uniform source; rho = 0.5 or the black / white truss of elast_pc_ref."""
    import elast_pc_ref as pr
    mesh = count_mesh(nelx, nely)
    return make_case(mesh, pr.count_density(kind, mesh.centroids(), 80.0))


@functools.lru_cache(maxsize=None)
def count_iterations(nelx, nely, kind, which):
    """PCG iterations of the restatement to rtol 1e-13 with the weighted, the stock or the Jacobi preconditioner."""
    case = count_case(nelx, nely, kind)
    M = case["M"]
    if which == "jacobi":
        M = Jacobi(case["M"].A.diagonal())
    elif which == "stock":
        M = bo.BPX(case["mesh"].x, case["M"].A.diagonal(), case["pinned"])
    else:
        assert which == "weighted"
    _, it = bo.pcg(case["M"].A, case["b"], M, rtol=COUNT_RTOL, max_it=100000)
    return it
