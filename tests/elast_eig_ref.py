"""NumPy / SciPy restatement of the eigenfrequency path of the SIMP elasticity (csrc/elast_eig.hip,
femo_amd/fea/elasticity.py: ElasticityEigenvalues / EigenvalueAggregate), on top of tests/elasticity_ref.py, written from
the formulas alone: dense element matrices and SciPy sparse assembly.

  M(rho)   = rho0 sum_e m(rho_e) M0_e,  M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2))  (consistent P1)
  m        = rho ("linear") or rho for rho >= 0.1, 6e5 rho^6 - 5e6 rho^7 below ("du_olhoff": C^1 at 0.1)
  K phi = lambda M phi on the free dofs (dense scipy.linalg.eigh, refined by one cell-wise Rayleigh-Ritz step), phi^T M phi = 1
  d lambda_k / d rho_e = C'(rho_e) phi_e^T K0_e phi_e - lambda_k rho0 m'(rho_e) phi_e^T M0_e phi_e
  J        = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p),  dJ/d lambda_k = (1/n) lambda_k^(-p-1) J^(p+1)
  block_inverse_iteration: the device's outer loop with a solve callback (exact, or elast_multi_ref.pcg_multi)
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elasticity_ref as ref

MASS_LAWS = ("linear", "du_olhoff")


def mass_law(rho, law="linear"):
    rho = np.asarray(rho, dtype=np.float64)
    if law == "linear":
        return rho.copy()
    return np.where(rho >= 0.1, rho, 6e5 * rho ** 6 - 5e6 * rho ** 7)


def mass_law_d(rho, law="linear"):
    rho = np.asarray(rho, dtype=np.float64)
    if law == "linear":
        return np.ones_like(rho)
    return np.where(rho >= 0.1, 1.0, 36e5 * rho ** 5 - 35e6 * rho ** 6)


def element_mass_matrices(x, conn):
    """M0_e of every cell: (n_cell, d (d+1), d (d+1)), blocked dofs d * a + i."""
    d = x.shape[1]
    vol = ref.cell_volumes(x, conn)
    S = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    return vol[:, None, None] * np.kron(S, np.eye(d))[None, :, :]


def mass(x, conn, rho, law="linear", density=1.0, M0=None):
    d = x.shape[1]
    M0 = element_mass_matrices(x, conn) if M0 is None else M0
    dofs = ref.element_dofs(conn, d)
    vals = (density * mass_law(rho, law))[:, None, None] * M0
    rows = np.repeat(dofs, dofs.shape[1], axis=1).ravel()
    cols = np.tile(dofs, (1, dofs.shape[1])).ravel()
    n = d * x.shape[0]
    return sp.csr_matrix((vals.ravel(), (rows, cols)), shape=(n, n))


def masked(M, fixed_mask):
    """M_ff embedded in the full numbering: zero rows and columns on the fixed dofs."""
    free = sp.diags((np.asarray(fixed_mask) == 0).astype(np.float64))
    return (free @ M @ free).tocsr()


def dense_eigs(K, M, fixed_mask, n_modes=None):
    """(lambda ascending, Phi (n_dof, n) with zeros on the fixed dofs, Phi^T M Phi = I) by dense eigh on the free dofs.  The
    pencil is solved as M v = mu K v, mu = 1 / lambda: eigh's absolute error is then a rounding unit of the LARGEST mu, so the
    lowest lambda come out to full relative accuracy (from K v = lambda M v they carry an error of eps lambda_max)."""
    free = np.nonzero(np.asarray(fixed_mask) == 0)[0]
    Kf, Mf = K.tocsr()[free][:, free].toarray(), M.tocsr()[free][:, free].toarray()
    mu, V = sla.eigh(0.5 * (Mf + Mf.T), 0.5 * (Kf + Kf.T))           # ascending mu, V^T K V = I, V^T M V = diag(mu)
    mu, V = mu[::-1], V[:, ::-1]
    n_modes = len(mu) if n_modes is None else n_modes
    Phi = np.zeros((K.shape[0], n_modes))
    Phi[free] = V[:, :n_modes] / np.sqrt(mu[:n_modes])[None, :]
    return 1.0 / mu[:n_modes], Phi


def eig_drho_terms(x, conn, Phi, K0=None, M0=None):
    """(phi_k,e^T K0_e phi_k,e, phi_k,e^T M0_e phi_k,e), each (n_modes, n_cell)."""
    d = x.shape[1]
    K0 = ref.element_matrices(x, conn) if K0 is None else K0
    M0 = element_mass_matrices(x, conn) if M0 is None else M0
    dofs = ref.element_dofs(conn, d)
    P = np.asarray(Phi).T[:, dofs]                                    # (n_modes, n_cell, d (d+1))
    return np.einsum("kei,eij,kej->ke", P, K0, P), np.einsum("kei,eij,kej->ke", P, M0, P)


def refine_eigs(x, conn, cK, cM, Phi, E=1.0, nu=0.3):
    """One Rayleigh-Ritz step on span(Phi) with Gram matrices summed cell by cell from the cell strains,
    G_K[k, l] = sum_e cK_e |T_e| (lam tr eps_k tr eps_l + 2 mu eps_k : eps_l), G_M likewise from M0_e: sums of cell energies,
    which do not cancel the way the rows of K phi (or phi_e^T K0_e phi_e with an assembled K0_e) do.  An eigenvalue is of
    second order in the error of its eigenvector, so this takes the eigenvalues of eigh (relative error about eps cond(K))
    to about eps (L / h)^2.  Returns (lambda, Phi Q)."""
    d = x.shape[1]
    lam0, mu0 = ref.lame(E, nu)
    p = x[conn]
    Minv = np.linalg.inv(p[:, 1:, :] - p[:, :1, :])
    g = np.zeros((len(conn), d + 1, d))
    g[:, 1:, :] = np.transpose(Minv, (0, 2, 1))
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    vol = ref.cell_volumes(x, conn)
    U = np.asarray(Phi).T.reshape(Phi.shape[1], -1, d)[:, conn]        # (n, n_cell, d+1, d)
    G = np.einsum("kebi,ebj->keij", U, g)
    eps = 0.5 * (G + np.swapaxes(G, 2, 3))
    tr = np.trace(eps, axis1=2, axis2=3)
    GK = np.einsum("e,ke,le->kl", cK * vol * lam0, tr, tr) + np.einsum("e,keij,leij->kl", cK * vol * 2.0 * mu0, eps, eps)
    S = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    GM = np.einsum("e,keai,ab,lebi->kl", cM * vol, U, S, U)
    lam, Q = sla.eigh(0.5 * (GK + GK.T), 0.5 * (GM + GM.T))
    return lam, np.asarray(Phi) @ Q


def eig_drho(x, conn, rho, Phi, lam, c, method="SIMP", law="linear", density=1.0, K0=None, M0=None):
    """sum_k c_k [C'(rho_e) phi_k^T K0_e phi_k - lambda_k rho0 m'(rho_e) phi_k^T M0_e phi_k] per cell."""
    eK, eM = eig_drho_terms(x, conn, Phi, K0, M0)
    lam, c = np.asarray(lam, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return (c[:, None] * (ref.penal_d(rho, method)[None, :] * eK
                          - lam[:, None] * density * mass_law_d(rho, law)[None, :] * eM)).sum(axis=0)


def aggregate(lam, p=8.0):
    """J = ((1/n) sum lambda_k^-p)^(-1/p) and dJ/d lambda_k."""
    lam = np.asarray(lam, dtype=np.float64)
    n = len(lam)
    lo = lam.min()
    J = lo * np.mean((lam / lo) ** -p) ** (-1.0 / p)
    return J, (lam / J) ** (-p - 1.0) / n


def aggregate_gradient(x, conn, rho, fixed_mask, n_modes, p=8.0, method="SIMP", law="linear", density=1.0):
    """(J, dJ/drho, lambda) from the dense eigenpairs."""
    K = ref.stiffness(x, conn, rho, method)
    M = mass(x, conn, rho, law, density)
    lam, Phi = dense_eigs(K, M, fixed_mask, n_modes)
    lam, Phi = refine_eigs(x, conn, ref.penal(rho, method), density * mass_law(rho, law), Phi)
    J, c = aggregate(lam, p)
    return J, eig_drho(x, conn, rho, Phi, lam, c, method, law, density), lam


def exact_solver(K, fixed_mask):
    """solve(B (L, n), X0 (L, n)) -> Y with K_ff Y = B on the free dofs and zeros on the fixed ones (sparse LU)."""
    free = np.nonzero(np.asarray(fixed_mask) == 0)[0]
    lu = spla.splu(K.tocsr()[free][:, free].tocsc())

    def solve(B, X0):
        Y = np.zeros_like(B)
        Y[:, free] = lu.solve(B[:, free].T).T
        return Y, 0
    return solve


def pcg_solver(A, precond, fixed_mask, rtol):
    """The device's inner solve: the batched PCG from the first guess X0, which is PCG from zero on A D = B - A X0 (the same
    first residual, so the same stopping level).  Returns (Y, iterations of the batched loop)."""
    from elast_multi_ref import pcg_multi

    def solve(B, X0):
        out = pcg_multi(A, B - (A @ X0.T).T, precond, fixed_mask, rtol=rtol)
        assert all(ok for _, _, ok in out)
        return X0 + np.stack([y for y, _, _ in out]), max(it for _, it, _ in out)
    return solve


def block_inverse_iteration(K, M, fixed_mask, X0, n_modes, solve, rtol=1e-9, max_outer=200):
    """Block inverse iteration with Rayleigh-Ritz, as csrc/elast_eig.hip states it.  X0: (block, n_dof).  Per outer step
    B = M_ff X, Y = solve(B, X), G_M = Y M Y^T, G_K = Y K Y^T, their generalised eigenproblem (theta ascending, Q), X = Q^T Y;
    stops when |K phi_k - theta_k M phi_k|_2 <= rtol theta_k |M phi_k|_2 for k < n_modes.
    Returns dict(lam, X, outer, pcg, residual, converged)."""
    fm = np.asarray(fixed_mask)
    Mff, Kff = masked(M, fm), masked(K, fm)
    X = np.where(fm[None, :] == 1, 0.0, np.asarray(X0, dtype=np.float64))
    pcg_total, res, theta = 0, None, None
    for outer in range(1, max_outer + 1):
        B = (Mff @ X.T).T
        Y, its = solve(B, X)
        pcg_total += its
        MY, KY = (Mff @ Y.T).T, (Kff @ Y.T).T
        GM, GK = Y @ MY.T, Y @ KY.T
        theta, Q = sla.eigh(0.5 * (GK + GK.T), 0.5 * (GM + GM.T))
        X, MX, KX = Q.T @ Y, Q.T @ MY, Q.T @ KY
        R = KX - theta[:, None] * MX
        res = np.linalg.norm(R, axis=1) / (np.abs(theta) * np.linalg.norm(MX, axis=1))
        if np.all(res[:n_modes] <= rtol):
            return dict(lam=theta, X=fix_signs(X), outer=outer, pcg=pcg_total, residual=res, converged=True)
    return dict(lam=theta, X=fix_signs(X), outer=max_outer, pcg=pcg_total, residual=res, converged=False)


def fix_signs(X):
    """The entry of largest magnitude of every row positive."""
    X = np.array(X)
    for k in range(X.shape[0]):
        if X[k, np.argmax(np.abs(X[k]))] < 0.0:
            X[k] = -X[k]
    return X


def start_block(n_free_or_mask, L, seed=1):
    """default_rng(seed).standard_normal((n_free, L)) placed on the free dofs: (L, n_dof)."""
    fm = np.asarray(n_free_or_mask)
    free = np.nonzero(fm == 0)[0]
    X = np.zeros((L, fm.size))
    X[:, free] = np.random.default_rng(seed).standard_normal((free.size, L)).T
    return X
