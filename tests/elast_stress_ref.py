"""NumPy restatement of the aggregated von Mises stress of the SIMP elasticity (femo_amd/fea/elasticity.py:
ElasticityPnormStress / ElasticityVonMises; kernels in csrc/elasticity.hip), written from the definition alone, with full
3 x 3 tensors and vectorised over the cells.

  sigma_0(u) = lambda_0 tr(eps) I + 2 mu_0 eps, eps the 3 x 3 strain (2-D: plane strain, eps_zz = eps_xz = eps_yz = 0)
  sigma_vm   = sqrt(3/2 s : s),  s = sigma_0 - tr(sigma_0) / 3 I
  J          = (1/alpha) sum_e |T_e| (m rho_e^q sigma_vm,e)^p,  alpha = |Omega| unless given
  dJ/drho_e  = (1/alpha) |T_e| p q / rho_e (m rho_e^q sigma_vm,e)^p
  dJ/du_(v,r) = sum_{e containing v} (tau_e grad phi_v)_r,  tau = 2 mu_0 S + lambda_0 tr(S) I,
                S = dJ_e/dsigma = (1/alpha) |T_e| p (m rho_e^q)^p sigma_vm^(p-2) 3/2 s
A cell with sigma_vm == 0 contributes 0 to the value and to both partials; a non-finite sigma_vm is not zero.
Dofs are blocked: dof = d * vertex + component.
The total derivative of the filtered cantilever goes through elasticity_ref (filter, stiffness, SciPy spsolve)."""
from __future__ import annotations

import numpy as np

import elasticity_ref as ref


def cell_gradients(x, conn):
    """(n_cell, d+1, d) gradients of the barycentric coordinates and (n_cell,) volumes."""
    d = x.shape[1]
    p = x[conn]
    M = p[:, 1:, :] - p[:, :1, :]                      # rows: edge vectors
    g = np.zeros((len(conn), d + 1, d))
    g[:, 1:, :] = np.transpose(np.linalg.inv(M), (0, 2, 1))
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    return g, np.abs(np.linalg.det(M)) / (2.0 if d == 2 else 6.0)


def solid_stress(x, conn, u, E=1.0, nu=0.3):
    """(n_cell, 3, 3) sigma_0(u) per cell."""
    d = x.shape[1]
    lam, mu = ref.lame(E, nu)
    g, _ = cell_gradients(x, conn)
    uc = np.asarray(u, dtype=np.float64).reshape(-1, d)[conn]          # (n_cell, d+1, d)
    G = np.einsum("ebi,ebk->eik", uc, g)                               # du_i/dx_k
    eps = np.zeros((len(conn), 3, 3))
    eps[:, :d, :d] = 0.5 * (G + np.transpose(G, (0, 2, 1)))
    tr = np.trace(eps, axis1=1, axis2=2)
    return lam * tr[:, None, None] * np.eye(3) + 2.0 * mu * eps


def deviator(sig):
    return sig - np.trace(sig, axis1=1, axis2=2)[:, None, None] / 3.0 * np.eye(3)


def von_mises(x, conn, u, E=1.0, nu=0.3):
    s = deviator(solid_stress(x, conn, u, E, nu))
    return np.sqrt(1.5 * np.einsum("eij,eij->e", s, s))


def cell_field(x, conn, u, rho=None, q=0.0, E=1.0, nu=0.3):
    """rho_e^q sigma_vm,e (q = 0: the solid stress)."""
    vm = von_mises(x, conn, u, E, nu)
    return vm if q == 0.0 else np.asarray(rho, dtype=np.float64) ** q * vm


def pnorm_stress(x, conn, rho, u, m=1.0, p=8.0, q=0.5, alpha=None, E=1.0, nu=0.3, positive_guard=False):
    """dict(value, du, drho, field, vm, alpha).  The zero-stress guard is a test for sigma_vm == 0, so a cell whose stress is
    not finite is no zero cell: it shows in the value and in both partials.  ``positive_guard``: the earlier guard
    sigma_vm > 0, which took such a cell for a zero one; kept for the host test that pins the two to the same bits on
    finite inputs."""
    d = x.shape[1]
    lam, mu = ref.lame(E, nu)
    rho = np.asarray(rho, dtype=np.float64)
    g, vol = cell_gradients(x, conn)
    alpha = float(vol.sum()) if alpha is None else float(alpha)
    s = deviator(solid_stress(x, conn, u, E, nu))
    vm = np.sqrt(1.5 * np.einsum("eij,eij->e", s, s))
    live = vm > 0.0 if positive_guard else ~(vm == 0.0)
    relax = m * rho ** q
    term = np.where(live, vol / alpha * (relax * vm) ** p, 0.0)
    drho = np.where(live, p * q / rho * term, 0.0) if q != 0.0 else np.zeros(len(conn))
    safe = np.where(live, vm, 1.0)
    coef = np.where(live, vol / alpha * p * relax ** p * safe ** (p - 2.0) * 1.5, 0.0)
    S = coef[:, None, None] * s
    tau = 2.0 * mu * S + lam * np.trace(S, axis1=1, axis2=2)[:, None, None] * np.eye(3)
    f = np.einsum("erk,ebk->ebr", tau[:, :d, :d], g)                   # (tau grad phi_b)_r
    du = np.zeros(d * x.shape[0])
    np.add.at(du, ref.element_dofs(conn, d).ravel(), f.ravel())
    return dict(value=float(term.sum()), du=du, drho=drho, field=rho ** q * vm if q != 0.0 else vm, vm=vm, alpha=alpha)


def cantilever_problem(mesh, facets, h_avg, traction=(0.0, -0.25)):
    """The fixed data of the filtered cantilever: W, element matrices, load, clamped dofs at x = 0."""
    d = mesh.tdim
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    return dict(x=mesh.x, conn=mesh.conn, W=ref.filter_matrix(mesh.centroids(), 2.0 * h_avg),
                K0=ref.element_matrices(mesh.x, mesh.conn), F=ref.traction_load(mesh.x, facets, traction),
                fixed=(fixed_v[:, None] * d + np.arange(d)).ravel())


def cantilever_state(P, x0, method="SIMP"):
    rho = P["W"] @ x0
    K = ref.stiffness(P["x"], P["conn"], rho, method, K0=P["K0"])
    return rho, K, ref.solve_fixed(K, P["F"], P["fixed"])


def cantilever_total(P, x0, m, p=8.0, q=0.5, method="SIMP"):
    """rho = W x0, K(rho) u = F, J(rho, u); adjoint K lambda = dJ/du on the free dofs (lambda = 0 on the clamped ones);
    dJ/dx = W^T (dJ/drho - lambda^T dK/drho u).  dict(value, grad, rho, u, lam, du, drho, F, field)."""
    rho, K, u = cantilever_state(P, x0, method)
    R = pnorm_stress(P["x"], P["conn"], rho, u, m, p, q)
    lam_ = ref.solve_fixed(K, R["du"], P["fixed"])
    total_rho = R["drho"] - ref.compliance_gradient(P["x"], P["conn"], rho, u, lam_, method, K0=P["K0"])
    return dict(value=R["value"], grad=P["W"].T @ total_rho, rho=rho, u=u, lam=lam_, du=R["du"], drho=R["drho"], F=P["F"],
                field=R["field"], vm=R["vm"])


def cantilever_value(P, x0, m, p=8.0, q=0.5, method="SIMP"):
    rho, _, u = cantilever_state(P, x0, method)
    return pnorm_stress(P["x"], P["conn"], rho, u, m, p, q)["value"]


def cosine(a, b):
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


# ------------------------------------------------------------------------------------------- inputs of the tests ----
PQ_CASES = ((1.0, 0.0), (8.0, 0.5), (12.0, 0.5))


def random_inputs(x, conn, seed=0):
    """Random u, rho in U(1e-3, 1) and m = 1 / max sigma_vm, so that the terms of the aggregate are O(1)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(x.size)
    rho = rng.uniform(1e-3, 1.0, len(conn))
    return u, rho, 1.0 / von_mises(x, conn, u).max()


def linear_field(x, A):
    """u = A x at the vertices, blocked."""
    return (x @ np.asarray(A, dtype=np.float64).T).ravel()


def closed_forms(d, E=1.0, nu=0.3):
    """(name, A, sigma_vm): uniaxial strain e e_0 e_0^T -> 2 mu |e|; simple shear A_01 = gamma -> sqrt(3) mu gamma."""
    _, mu = ref.lame(E, nu)
    e, gamma = -0.013, 0.02
    A1 = np.zeros((d, d)); A1[0, 0] = e
    A2 = np.zeros((d, d)); A2[0, 1] = gamma
    return (("uniaxial", A1, 2.0 * mu * abs(e)), ("shear", A2, np.sqrt(3.0) * mu * gamma))
