"""NumPy / SciPy restatement of the linearised buckling path of the SIMP elasticity (csrc/elast_buckle.hip,
femo_amd/fea/elasticity.py: ElasticityBuckling / BucklingAggregate), on top of tests/elasticity_ref.py,
tests/elast_stress_ref.py, tests/elast_eig_ref.py and tests/elast_body_ref.py, written from the formulas alone: dense element
matrices, SciPy sparse assembly and dense eigh.

  state     K(rho) u = F(rho), one load case
  sigma_e   = C(rho_e) sigma_0(u_e),  sigma_0 = lambda_0 tr(eps) I + 2 mu_0 eps, the d x d in-plane block
  K_G,e[(a,i),(b,j)] = delta_ij |T_e| g_a . sigma_e g_b
  (K + lambda K_G) phi = 0 on the free dofs, as (-K_G) phi = mu K phi, mu = 1 / lambda, phi^T K phi = 1; the critical load
            factor is the smallest positive lambda = 1 / (largest positive mu)
  H_e(phi)  = (grad phi)^T (grad phi),  Sigma_H = lambda_0 tr(H) I + 2 mu_0 H
  d lambda_k / d rho_e   = lambda_k C'(rho_e) [phi_e^T K0_e phi_e + lambda_k |T_e| sigma_0(u_e) : H_e(phi_k)]
  d lambda_k / d u_(b,j) = lambda_k^2 sum_{e around b} C(rho_e) |T_e| (Sigma_H,e(phi_k) g_b)_j       (non-zero on clamped dofs)
  J         = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p), that of elast_eig_ref.aggregate
  dJ/drho   = dJ/drho|_u - C'(rho) w^T K0 u + G_b^T w,  K w = dJ/du on the free dofs, w = 0 on the clamped ones
  block_power_iteration: the device's outer loop with a solve callback (exact, or a zero-guess elast_multi_ref.pcg_multi)
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import elast_body_ref as br
import elast_eig_ref as er
import elast_stress_ref as sr
import elasticity_ref as ref


def cell_stress(x, conn, rho, u, method="SIMP"):
    """(n_cell, d, d): C(rho_e) sigma_0(u_e), the in-plane block."""
    d = x.shape[1]
    return ref.penal(rho, method)[:, None, None] * sr.solid_stress(x, conn, u)[:, :d, :d]


def stress_components(sig):
    """(d (d+1) / 2, n_cell): the diagonal first, then 01[, 02, 12] -- the layout of the device's stress buffer."""
    d = sig.shape[1]
    pairs = [(i, i) for i in range(d)] + [(i, k) for i in range(d) for k in range(i + 1, d)]
    return np.stack([sig[:, i, k] for i, k in pairs])


def element_geometric_matrices(x, conn, sig):
    """K_G,e of every cell for the cell stresses ``sig`` (n_cell, d, d): (n_cell, d (d+1), d (d+1)), blocked dofs d a + i."""
    d = x.shape[1]
    g, vol = sr.cell_gradients(x, conn)
    S = vol[:, None, None] * np.einsum("eak,ekl,ebl->eab", g, sig, g)          # |T| g_a . sigma g_b
    return np.einsum("eab,ij->eaibj", S, np.eye(d)).reshape(len(conn), d * (d + 1), d * (d + 1))


def geometric_stiffness(x, conn, rho, u, method="SIMP"):
    """K_G(u, rho), assembled."""
    d = x.shape[1]
    KGe = element_geometric_matrices(x, conn, cell_stress(x, conn, rho, u, method))
    dofs = ref.element_dofs(conn, d)
    rows = np.repeat(dofs, dofs.shape[1], axis=1).ravel()
    cols = np.tile(dofs, (1, dofs.shape[1])).ravel()
    n = d * x.shape[0]
    return sp.csr_matrix((KGe.ravel(), (rows, cols)), shape=(n, n))


def dense_buckling(K, KG, fixed_mask, n_modes=None):
    """dict(lam, Phi, mu): the n_modes smallest positive load factors ascending, their modes (n_dof, n) with zeros on the
    fixed dofs and Phi^T K Phi = I, and the whole spectrum mu (descending) of (-K_G)_ff v = mu K_ff v by dense eigh."""
    free = np.nonzero(np.asarray(fixed_mask) == 0)[0]
    Kf, Gf = K.tocsr()[free][:, free].toarray(), -KG.tocsr()[free][:, free].toarray()
    mu, V = sla.eigh(0.5 * (Gf + Gf.T), 0.5 * (Kf + Kf.T))           # ascending mu, V^T K V = I
    mu, V = mu[::-1], V[:, ::-1]
    n_modes = int((mu > 0.0).sum()) if n_modes is None else n_modes
    assert np.all(mu[:n_modes] > 0.0), "fewer positive load factors than asked for"
    Phi = np.zeros((K.shape[0], n_modes))
    Phi[free] = V[:, :n_modes]
    return dict(lam=1.0 / mu[:n_modes], Phi=Phi, mu=mu)


def mode_gradients(x, conn, Phi):
    """(n_modes, n_cell, d, d): G[k, e, i, l] = d_l phi_k,i in cell e."""
    d = x.shape[1]
    g, _ = sr.cell_gradients(x, conn)
    P = np.asarray(Phi).T.reshape(np.asarray(Phi).shape[1], -1, d)[:, conn]    # (n_modes, n_cell, d+1, d)
    return np.einsum("kebi,ebl->keil", P, g)


def mode_H(x, conn, Phi):
    """(n_modes, n_cell, d, d): H = (grad phi)^T (grad phi), H[k, l] = sum_i d_k phi_i d_l phi_i."""
    G = mode_gradients(x, conn, Phi)
    return np.einsum("keim,kein->kemn", G, G)


def buckle_du(x, conn, rho, Phi, w, method="SIMP", E=1.0, nu=0.3):
    """out[(b, j)] = sum_{e around b} C(rho_e) |T_e| (Sigma_Hbar g_b)_j with Hbar = sum_k w_k H(phi_k)."""
    d = x.shape[1]
    lam0, mu0 = ref.lame(E, nu)
    g, vol = sr.cell_gradients(x, conn)
    H = np.einsum("k,kemn->emn", np.asarray(w, dtype=np.float64), mode_H(x, conn, Phi))
    SH = lam0 * np.trace(H, axis1=1, axis2=2)[:, None, None] * np.eye(d) + 2.0 * mu0 * H
    f = (ref.penal(rho, method) * vol)[:, None, None] * np.einsum("ejm,ebm->ebj", SH, g)
    out = np.zeros(d * x.shape[0])
    np.add.at(out, ref.element_dofs(conn, d).ravel(), f.ravel())
    return out


def buckle_drho(x, conn, rho, u, Phi, w1, w2, method="SIMP", K0=None):
    """C'(rho_e) sum_k [w1_k phi_k,e^T K0_e phi_k,e + w2_k |T_e| sigma_0(u_e) : H_e(phi_k)] per cell."""
    d = x.shape[1]
    K0 = ref.element_matrices(x, conn) if K0 is None else K0
    dofs = ref.element_dofs(conn, d)
    P = np.asarray(Phi).T[:, dofs]
    eK = np.einsum("kei,eij,kej->ke", P, K0, P)
    s0 = sr.solid_stress(x, conn, u)[:, :d, :d]
    sH = ref.cell_volumes(x, conn)[None, :] * np.einsum("emn,kemn->ke", s0, mode_H(x, conn, Phi))
    w1, w2 = np.asarray(w1, dtype=np.float64), np.asarray(w2, dtype=np.float64)
    return ref.penal_d(rho, method) * (w1[:, None] * eK + w2[:, None] * sH).sum(axis=0)


aggregate = er.aggregate


# ------------------------------------------------------------------------------------------------- the whole chain ----
def end_face(mesh):
    """The facets of the face x = x_max."""
    from femo_amd.fea.mesh import locate_entities_boundary
    xmax = mesh.x[:, 0].max()
    return locate_entities_boundary(mesh, mesh.tdim - 1, lambda x: np.isclose(x[0], xmax))


def end_traction(mesh, sign=-1.0):
    """The unit traction along x on the end face: compressive for sign = -1."""
    t = np.zeros(mesh.tdim)
    t[0] = sign
    return t


def state(mesh, rho, fixed_mask, method="SIMP", traction=None, body=None):
    """dict(K, F, u, KG): K(rho) u = F(rho) with the end-face traction (compressive unit pull unless given) plus the body
    force ``body``, clamped on the fixed set, and K_G(u, rho)."""
    x, conn = mesh.x, mesh.conn
    t = end_traction(mesh) if traction is None else np.asarray(traction, dtype=np.float64)
    K = ref.stiffness(x, conn, rho, method)
    F = ref.traction_load(x, end_face(mesh), t)
    if body is not None:
        F = F + br.body_load(x, conn, rho, body)
    u = ref.solve_fixed(K, F, np.nonzero(np.asarray(fixed_mask) == 1)[0])
    return dict(K=K, F=F, u=u, KG=geometric_stiffness(x, conn, rho, u, method))


def aggregate_value(mesh, rho, fixed_mask, n_modes, p=8.0, method="SIMP", traction=None, body=None):
    S = state(mesh, rho, fixed_mask, method, traction, body)
    return aggregate(dense_buckling(S["K"], S["KG"], fixed_mask, n_modes)["lam"], p)[0]


def total_gradient(mesh, rho, fixed_mask, n_modes, p=8.0, method="SIMP", traction=None, body=None):
    """dict(J, grad, lam, Phi, u, du, drho, w): the aggregate of the dense load factors and its exact reduced gradient
    dJ/drho = dJ/drho|_u - w^T dR/drho with K w = dJ/du on the free dofs, R = K(rho) u - F(rho)."""
    x, conn = mesh.x, mesh.conn
    S = state(mesh, rho, fixed_mask, method, traction, body)
    D = dense_buckling(S["K"], S["KG"], fixed_mask, n_modes)
    lam, Phi = D["lam"], D["Phi"]
    J, c = aggregate(lam, p)
    du = buckle_du(x, conn, rho, Phi, c * lam ** 2, method)
    drho = buckle_drho(x, conn, rho, S["u"], Phi, c * lam, c * lam ** 2, method)
    w = ref.solve_fixed(S["K"], du, np.nonzero(np.asarray(fixed_mask) == 1)[0])
    grad = drho - ref.compliance_gradient(x, conn, rho, S["u"], w, method)
    if body is not None:
        grad = grad + br.body_drho_T(x, conn, w, body)
    return dict(J=J, grad=grad, lam=lam, Phi=Phi, u=S["u"], du=du, drho=drho, w=w, mu=D["mu"])


# --------------------------------------------------------------------------------------------------- the iteration ----
def zero_guess_pcg_solver(A, precond, fixed_mask, rtol):
    """The device's inner solve: the batched PCG on A Y = B from a zero first guess, so that the stopping level is relative
    to |B|.  Returns (Y, iterations of the batched loop)."""
    from elast_multi_ref import pcg_multi

    def solve(B, X0):
        out = pcg_multi(A, B, precond, fixed_mask, rtol=rtol)
        assert all(ok for _, _, ok in out)
        return np.stack([y for y, _, _ in out]), max(it for _, it, _ in out)
    return solve


def block_power_iteration(K, KG, fixed_mask, X0, n_modes, solve, rtol=1e-9, max_outer=400):
    """The block iteration on the pencil (-K_G, K), as csrc/elast_buckle.hip states it.  X0: (block, n_dof).  Per outer step
    B = (-K_G)_ff X, Y = solve(B, X) (K Y = B), G_K = Y K Y^T, G_G = Y (-K_G) Y^T, their generalised eigenproblem with the
    columns in DESCENDING mu, X = Q^T Y (so X K X^T = I), R = (-K_G) X - diag(mu) K X; stops when |R_k| <= rtol mu_k |K x_k| and
    mu_k > 0 for every k < n_modes.  Returns dict(lam = 1 / mu, mu, X, outer, pcg, residual, converged)."""
    fm = np.asarray(fixed_mask)
    Gff, Kff = er.masked(-KG, fm), er.masked(K, fm)
    X = np.where(fm[None, :] == 1, 0.0, np.asarray(X0, dtype=np.float64))
    pcg_total, res, mu, converged, outer = 0, None, None, False, 0
    for outer in range(1, max_outer + 1):
        B = (Gff @ X.T).T
        Y, its = solve(B, X)
        pcg_total += its
        KY, GY = (Kff @ Y.T).T, (Gff @ Y.T).T
        GK, GG = Y @ KY.T, Y @ GY.T
        mu, Q = sla.eigh(0.5 * (GG + GG.T), 0.5 * (GK + GK.T))
        mu, Q = mu[::-1], Q[:, ::-1]
        X, KX, GX = Q.T @ Y, Q.T @ KY, Q.T @ GY
        R = GX - mu[:, None] * KX
        res = np.linalg.norm(R, axis=1) / (np.abs(mu) * np.linalg.norm(KX, axis=1))
        if np.all(res[:n_modes] <= rtol) and np.all(mu[:n_modes] > 0.0):
            converged = True
            break
    return dict(lam=1.0 / mu, mu=mu, X=er.fix_signs(X), outer=outer, pcg=pcg_total, residual=res, converged=converged)
