"""NumPy / SciPy restatement of the harmonic response of the SIMP elasticity (csrc/elast_harm.hip,
femo_amd/fea/elasticity.py: HarmonicElasticityResidual / DynamicCompliance), on top of tests/elasticity_ref.py and
tests/elast_eig_ref.py, written from the formulas alone:

  S_l      = K(rho) - sigma_l M(rho), sigma_l = omega_l^2, with `elasticity_ref.stiffness` and `elast_eig_ref.mass`
  minres   the device's loop step by step: Paige & Saunders' MINRES with an SPD preconditioner, x = b on the fixed dofs,
           stopped on phibar <= max(rtol beta1, atol) with beta1 = sqrt(r0 . M^-1 r0)
  direct   sparse LU of S on the free dofs
  J        = sum_l w_l |c_l| or sum_l w_l c_l^2, c_l = F_l . u_l;  the adjoint of column l is w_l g'(c_l) u_l (S is symmetric),
           so dJ/drho_e = - sum_l w_l g'(c_l) u_l,e^T (C'(rho_e) K0_e - sigma_l rho0 m'(rho_e) M0_e) u_l,e
  problem  the set-up the host and the GPU tests share
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elast_eig_ref as er
import elast_pc_ref as pr
import elasticity_ref as ref

DENSITY = 1.3
CASES = (("SIMP", "linear"), ("RAMP", "du_olhoff"))       # (stiffness law, mass law)
EPS = float(np.finfo(np.float64).eps)


def shifted(K, M, sigma):
    return (K - sigma * M).tocsr()


def masked_shifted(K, M, sigma, fixed_mask):
    """K - sigma M with identity rows and columns on the fixed dofs."""
    return pr.masked_operator(shifted(K, M, sigma), fixed_mask)


def direct(K, M, sigma, F, fixed_mask):
    """u with zeros on the fixed dofs and (K - sigma M) u = F on the others."""
    free = np.nonzero(np.asarray(fixed_mask) == 0)[0]
    S = shifted(K, M, sigma)[free][:, free].tocsc()
    u = np.zeros(K.shape[0])
    u[free] = spla.splu(S).solve(np.asarray(F, dtype=np.float64)[free])
    return u


def minres(S, b, precond, fixed_mask=None, rtol=1e-12, atol=0.0, max_it=100000, x0=None, keep=False):
    """One column of the device's loop (the columns of a batched solve do not see one another).  Returns dict(x, iterations,
    converged (1, 0: max_it, -1: a non-finite value), phibar, beta1, history); with ``keep`` history[k] is x after iteration
    k + 1."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    if fixed_mask is not None:
        fx = np.asarray(fixed_mask) == 1
        x[fx] = b[fx]
    r2 = b - S @ x
    z = precond(r2)
    with np.errstate(invalid="ignore"):
        beta1 = float(np.sqrt(r2 @ z))
    out = dict(x=x, iterations=0, converged=0, phibar=beta1, beta1=beta1, history=[])
    tol = max(rtol * beta1, atol)
    if not np.isfinite(beta1):
        return dict(out, converged=-1)
    if beta1 <= tol:
        return dict(out, converged=1)
    beta, oldb, dbar, epsln, phibar, cs, sn = beta1, 0.0, 0.0, 0.0, beta1, -1.0, 0.0
    v = z / beta
    w1, w2, r1 = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    for it in range(1, max_it + 1):
        q = S @ v
        alfa = float(v @ q)
        t = q - (alfa / beta) * r2
        if it >= 2:
            t -= (beta / oldb) * r1
        r1, r2 = r2, t
        z = precond(r2)
        oldb = beta
        with np.errstate(invalid="ignore"):
            beta = float(np.sqrt(r2 @ z))
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = max(float(np.sqrt(gbar * gbar + beta * beta)), EPS)
        cs, sn = gbar / gamma, beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        if not (np.isfinite(beta) and np.isfinite(phi) and np.isfinite(delta)):
            return dict(out, x=x, iterations=it, converged=-1, phibar=phibar)
        w = (v - oldeps * w1 - delta * w2) / gamma
        w1, w2 = w2, w
        x = x + phi * w
        if keep:
            out["history"].append(x.copy())
        if phibar <= tol or beta == 0.0:
            return dict(out, x=x, iterations=it, converged=1, phibar=phibar)
        v = z / beta
    return dict(out, x=x, iterations=max_it, converged=0, phibar=phibar)


def jacobi(K, fixed_mask, d):
    """z = D^-1 r with the d x d diagonal blocks of the masked, unshifted K."""
    Dinv = pr.invert_blocks(pr.block_diagonal(pr.masked_operator(K, fixed_mask), d))
    return lambda r: np.einsum("nij,nj->ni", Dinv, r.reshape(-1, d)).ravel()


def mass_drho_matrix(x, conn, rho, u, law="linear", density=1.0, M0=None):
    """(n_dof, n_cell): column e = density m'(rho_e) M0_e u_e, the mass part of d(M u)/d rho."""
    d = x.shape[1]
    M0 = er.element_mass_matrices(x, conn) if M0 is None else M0
    dofs = ref.element_dofs(conn, d)
    t = (density * er.mass_law_d(rho, law))[:, None] * np.einsum("eij,ej->ei", M0, np.asarray(u)[dofs])
    cells = np.repeat(np.arange(len(conn)), dofs.shape[1])
    return sp.csr_matrix((t.ravel(), (dofs.ravel(), cells)), shape=(d * x.shape[0], len(conn)))


def compliance_value(c, weights=None, squared=False):
    """(J, dJ/dc) of J = sum_l w_l |c_l| or sum_l w_l c_l^2."""
    c = np.asarray(c, dtype=np.float64)
    w = np.ones_like(c) if weights is None else np.asarray(weights, dtype=np.float64)
    if squared:
        return float(w @ (c * c)), 2.0 * w * c
    return float(w @ np.abs(c)), w * np.sign(c)


def responses(x, conn, rho, fixed_mask, F, sigmas, method="SIMP", law="linear", density=1.0):
    """(U (L, n_dof) by direct solves, c_l = F_l . u_l)."""
    K = ref.stiffness(x, conn, rho, method)
    M = er.mass(x, conn, rho, law, density)
    U = np.stack([direct(K, M, s, Fl, fixed_mask) for s, Fl in zip(sigmas, F)])
    return U, np.einsum("li,li->l", np.asarray(F), U)


def adjoint_total(x, conn, rho, fixed_mask, F, sigmas, weights=None, squared=False, method="SIMP", law="linear", density=1.0):
    """(J, dJ/drho, c, U) with the direct solves."""
    U, c = responses(x, conn, rho, fixed_mask, F, sigmas, method, law, density)
    J, dJdc = compliance_value(c, weights, squared)
    return J, dJdc @ response_gradients(x, conn, rho, U, sigmas, method, law, density), c, U


def response_gradients(x, conn, rho, U, sigmas, method="SIMP", law="linear", density=1.0):
    """(L, n_cell): d c_l / d rho_e = - u_l,e^T (C'(rho_e) K0_e - sigma_l density m'(rho_e) M0_e) u_l,e."""
    eK, eM = er.eig_drho_terms(x, conn, np.asarray(U).T)
    s = np.asarray(sigmas, dtype=np.float64)
    return -(ref.penal_d(rho, method)[None, :] * eK - s[:, None] * (density * er.mass_law_d(rho, law))[None, :] * eM)


def end_face_load(mesh):
    """Traction (0, -1[, 0]) on the face x = x_max."""
    from femo_amd.fea.mesh import locate_entities_boundary
    xmax = mesh.x[:, 0].max()
    facets = locate_entities_boundary(mesh, mesh.tdim - 1, lambda x: np.isclose(x[0], xmax))
    t = np.zeros(mesh.tdim)
    t[1] = -1.0
    return facets, t, ref.traction_load(mesh.x, facets, t)


def shifts_of(lam):
    """sigma in {0, lambda_1 / 2, sqrt(lambda_1 lambda_2), sqrt(lambda_2 lambda_3), sqrt(lambda_5 lambda_6)}."""
    return np.array([0.0, 0.5 * lam[0], np.sqrt(lam[0] * lam[1]), np.sqrt(lam[1] * lam[2]), np.sqrt(lam[4] * lam[5])])


def problem(mesh, method, law, density=DENSITY):
    """Clamped on x = 0, rho = default_rng(7).uniform(0.3, 1), the end-face load, the dense pencil's first six eigenvalues
    and the five shifts of `shifts_of`."""
    mask = pr.clamped_face(mesh)
    rho = np.random.default_rng(7).uniform(0.3, 1.0, mesh.n_cell)
    K = ref.stiffness(mesh.x, mesh.conn, rho, method)
    M = er.mass(mesh.x, mesh.conn, rho, law, density)
    lam = er.dense_eigs(K, M, mask, 6)[0]
    facets, t, F = end_face_load(mesh)
    return dict(mesh=mesh, mask=mask, rho=rho, K=K, M=M, lam=lam, shifts=shifts_of(lam), facets=facets, traction=t, F=F,
                method=method, law=law, density=density)


def spectrum_gap(K, M, fixed_mask, sigma):
    """min_k |lambda_k - sigma| / lambda_k over the whole dense spectrum."""
    lam = er.dense_eigs(K, M, fixed_mask)[0]
    return float(np.min(np.abs(lam - sigma) / lam))
