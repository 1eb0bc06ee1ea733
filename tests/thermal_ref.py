"""NumPy / SciPy restatement of the thermal expansion load of the SIMP elasticity (csrc/elast_thermal.hip, ``thermal=`` of
femo_amd/fea/elasticity.py) and of the heat conduction with a penalised conductivity (csrc/conduction.hip,
femo_amd/fea/conduction.py), on top of tests/elasticity_ref.py, written from the formulas alone, cell by cell:

  sigma = C(rho) (sigma_0(u) - beta_0 theta I),  beta_0 = (3 lambda_0 + 2 mu_0) alpha,  theta = T - T_ref (P1)
  thermal_H      H(w; theta)[d v + i] = sum_{c around v} w_c beta_0 thetabar_c |T_c| d_i phi_v^c, thetabar_c the cell mean
  thermal_T_rho  y_c = C'(rho_c) beta_0 thetabar_c |T_c| div(x)_c,  div(x)_c = sum_a grad phi_a . x[a]
  thermal_T_temp y_v = sum_{c around v} C(rho_c) beta_0 |T_c| / (d + 1) div(x)_c
  conduction_matrix   K_theta(rho) = sum_c k(rho_c) |T_c| grad phi_a . grad phi_b,  k = k_min + (k0 - k_min) C(rho)
  conduction_drho / conduction_drho_T   (dR/drho d)_v = sum_c k'(rho_c) d_c |T_c| grad phi_v . grad T_c and its transpose
  heat_load      Q_v = sum_{c around v} q_c |T_c| / (d + 1) + flux sum_{f around v} |f| / d
  reference_cycle_thermoelastic   filter -> K_theta(rho) T = Q -> K(rho) u = F + H(C(rho); T - T_ref) -> J -> the exact reduced
                 gradient through both adjoints
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elasticity_ref as ref


# The meshes of the GPU tests: less than one wave of rows (rect8x4), the two jittered ones, two with more than one block of
# 256 rows (rect24x12: 325 vertices, cube6j: 343), and the fan, whose hub row is longer than 14 entries and whose slices carry
# dead visits.  Built once per process and shared: read only.
MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j", "fan40x8"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    from elast_pc_ref import small_meshes
    from femo_amd.fea.mesh import Mesh, createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    if name == "fan40x8":
        import wide_meshes
        return Mesh(*wide_meshes.fan(40, 8))
    return small_meshes()[name]()


def beta0(alpha, E=1.0, nu=0.3):
    lam, mu = ref.lame(E, nu)
    return (3.0 * lam + 2.0 * mu) * alpha


def _nodal(theta, n_vert):
    return np.full(n_vert, float(theta)) if np.ndim(theta) == 0 else np.asarray(theta, dtype=np.float64)


# ------------------------------------------------------------------------------------------ the thermal expansion load ----
def thermal_H(x, conn, w, theta, alpha, E=1.0, nu=0.3):
    """H(w; theta): cell c adds w_c beta_0 thetabar_c |T_c| grad phi_a to vertex a.  theta: nodal values or a number."""
    d = x.shape[1]
    b0 = beta0(alpha, E, nu)
    th = _nodal(theta, x.shape[0])
    F = np.zeros((x.shape[0], d))
    for c, cell in enumerate(conn):
        g, vol = ref.grads_and_volume(x[cell])
        q = w[c] * b0 * th[cell].mean() * vol
        for a, v in enumerate(cell):
            F[v] += q * g[a]
    return F.ravel()


def thermal_load(x, conn, rho, theta, alpha, method="SIMP", E=1.0, nu=0.3):
    """F_th = H(C(rho); theta)"""
    return thermal_H(x, conn, ref.penal(rho, method), theta, alpha, E, nu)


def cell_divergence(x, conn, xv):
    """div(x)_c = sum_a grad phi_a . x[a] of the blocked vertex vector xv."""
    d = x.shape[1]
    X = np.asarray(xv).reshape(-1, d)
    out = np.zeros(len(conn))
    for c, cell in enumerate(conn):
        g, _ = ref.grads_and_volume(x[cell])
        out[c] = np.sum(g * X[cell])
    return out


def thermal_T_rho(x, conn, rho, theta, xv, alpha, method="SIMP", E=1.0, nu=0.3):
    """The transpose of w -> H(C'(rho) w; theta) applied to xv: one number per cell."""
    th = _nodal(theta, x.shape[0])
    vol = ref.cell_volumes(x, conn)
    return ref.penal_d(rho, method) * beta0(alpha, E, nu) * th[conn].mean(axis=1) * vol * cell_divergence(x, conn, xv)


def thermal_T_temp(x, conn, rho, xv, alpha, method="SIMP", E=1.0, nu=0.3):
    """The transpose of theta -> H(C(rho); theta) applied to xv: one number per vertex."""
    d = x.shape[1]
    q = ref.penal(rho, method) * beta0(alpha, E, nu) * ref.cell_volumes(x, conn) / (d + 1) * cell_divergence(x, conn, xv)
    out = np.zeros(x.shape[0])
    for c, cell in enumerate(conn):
        for v in cell:
            out[v] += q[c]
    return out


def free_expansion(x, theta, alpha, nu=0.3):
    """u = e x with e = (1 + nu) alpha theta in plane strain and alpha theta in 3-D: the stress-free state of a uniform theta."""
    e = (1.0 + nu) * alpha * theta if x.shape[1] == 2 else alpha * theta
    return (e * x).ravel()


# ------------------------------------------------------------------------------------------------- heat conduction ----
def conductivity(rho, k0=1.0, k_min=0.0, method="SIMP"):
    return k_min + (k0 - k_min) * ref.penal(rho, method)


def conductivity_d(rho, k0=1.0, k_min=0.0, method="SIMP"):
    return (k0 - k_min) * ref.penal_d(rho, method)


def conduction_matrix(x, conn, kc):
    """sum_c kc_c |T_c| grad phi_a . grad phi_b, cell by cell (CSR)."""
    n = x.shape[0]
    rows, cols, vals = [], [], []
    for c, cell in enumerate(conn):
        g, vol = ref.grads_and_volume(x[cell])
        Ke = kc[c] * vol * (g @ g.T)
        rows.append(np.repeat(cell, len(cell))); cols.append(np.tile(cell, len(cell))); vals.append(Ke.ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def conduction_drho(x, conn, rho, T, dr, k0=1.0, k_min=0.0, method="SIMP"):
    """(dR/drho dr)_v = sum_c k'(rho_c) dr_c |T_c| grad phi_v . grad T_c"""
    kd = conductivity_d(rho, k0, k_min, method)
    out = np.zeros(x.shape[0])
    for c, cell in enumerate(conn):
        g, vol = ref.grads_and_volume(x[cell])
        gT = g.T @ T[cell]
        out[cell] += kd[c] * dr[c] * vol * (g @ gT)
    return out


def conduction_drho_T(x, conn, rho, T, xv, k0=1.0, k_min=0.0, method="SIMP"):
    """y_c = k'(rho_c) |T_c| grad x_c . grad T_c"""
    kd = conductivity_d(rho, k0, k_min, method)
    out = np.zeros(len(conn))
    for c, cell in enumerate(conn):
        g, vol = ref.grads_and_volume(x[cell])
        out[c] = kd[c] * vol * ((g.T @ xv[cell]) @ (g.T @ T[cell]))
    return out


def facet_measures(x, facets):
    d = x.shape[1]
    p = x[np.asarray(facets).reshape(-1, d)]
    if d == 2:
        return np.linalg.norm(p[:, 1] - p[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def heat_load(x, conn, source=None, flux=None, facets=None):
    """Q: the P1 load of the cell source q_c (a number or one per cell) plus the facet flux, lumped like the traction."""
    d = x.shape[1]
    Q = np.zeros(x.shape[0])
    if source is not None:
        q = np.broadcast_to(np.asarray(source, dtype=np.float64), (len(conn),))
        vol = ref.cell_volumes(x, conn)
        for c, cell in enumerate(conn):
            Q[cell] += q[c] * vol[c] / (d + 1)
    if flux is not None:
        f = np.asarray(facets).reshape(-1, d)
        for fv, m in zip(f, facet_measures(x, f)):
            Q[fv] += flux * m / d
    return Q


def solve_lifted(K, Q, fixed, g=None):
    """T with T = g on the fixed vertices (0 without g) and K T = Q on the others: the lifting b = Q - K g."""
    return ref.solve_fixed(K, Q, fixed, g)


# ------------------------------------------------------------------------------------------------------- the cycle ----
# The thermoelastic cantilever of the cycle tests: uniform heating SOURCE, the sink T = 0 on the clamped edge x = 0, the tip
# traction of the cantilever, and an expansion coefficient ALPHA at which the thermal and the mechanical part of u are of the
# same order on the 16 x 8 mesh (test_thermal_host.test_cycle_parts_are_of_the_same_order asserts it): a wrong thermal adjoint
# then shows in the total gradient.
SOURCE = 1e-2
ALPHA = 1e-2
TRACTION = (0.0, -0.25)


def cycle_case(nelx=16, nely=8):
    """(mesh, tip facets, h_avg, sink vertices) of the thermoelastic cantilever."""
    from elast_pc_ref import L_X, L_Y, cantilever_case
    from femo_amd.fea.mesh import createRectangleMesh, meshSize
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    _, facets, _ = cantilever_case(mesh.x, mesh.conn, L_X, L_Y, nely)
    h = meshSize(mesh)
    return mesh, facets, (h.max() + h.min()) / 2, np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]


def reference_cycle_thermoelastic(mesh, facets, traction, h_avg, x0, alpha, source, sink_vertices, T_ref=0.0, k0=1.0, k_min=1e-3,
                                  method="SIMP", objective="compliance", ell=None, filtered=True, E=1.0, nu=0.3):
    """filter -> K_theta(rho) T = Q (T = 0 on the sink) -> K(rho) u = F + H(C(rho); T - T_ref) (clamped at x = 0) -> J -> dJ/dx0.
    J = F_total . u ("compliance": the work of the total load) or ell . u ("displacement").  With R_u = K u - F(rho, T) and
    R_T = K_theta T - Q:  K lam_u = dJ/du,  K_theta lam_T = dJ/dT - (dR_u/dT)^T lam_u,  both zero on their fixed sets, and
    dJ/drho = dJ/drho|explicit - lam_u^T dR_u/drho - lam_T^T dR_T/drho."""
    x, conn = mesh.x, mesh.conn
    d = x.shape[1]
    W = ref.filter_matrix(mesh.centroids(), 2.0 * h_avg) if filtered else sp.identity(len(conn), format="csr")
    rho = W @ x0
    # heat conduction
    Kt = conduction_matrix(x, conn, conductivity(rho, k0, k_min, method))
    Q = heat_load(x, conn, source=source)
    sink = np.asarray(sink_vertices)
    T = solve_lifted(Kt, Q, sink)
    # elasticity
    K0 = ref.element_matrices(x, conn, E, nu)
    K = ref.stiffness(x, conn, rho, method, K0=K0)
    fixed_v = np.nonzero(np.isclose(x[:, 0], 0.0))[0]
    fixed = np.concatenate([d * fixed_v + k for k in range(d)])
    Ft = ref.traction_load(x, facets, traction)
    Fth = thermal_load(x, conn, rho, T - T_ref, alpha, method, E, nu)
    F = Ft + Fth
    u = ref.solve_fixed(K, F, fixed)
    u_mech, u_th = ref.solve_fixed(K, Ft, fixed), ref.solve_fixed(K, Fth, fixed)
    if objective == "compliance":
        J = float(F @ u)
        dJdu = F
        dJdrho = thermal_T_rho(x, conn, rho, T - T_ref, u, alpha, method, E, nu)
        dJdT = thermal_T_temp(x, conn, rho, u, alpha, method, E, nu)
    else:
        J = float(ell @ u)
        dJdu = np.asarray(ell, dtype=np.float64)
        dJdrho = np.zeros(len(conn))
        dJdT = np.zeros(x.shape[0])
    lam_u = ref.solve_fixed(K, dJdu, fixed)
    rhs_T = dJdT + thermal_T_temp(x, conn, rho, lam_u, alpha, method, E, nu)          # dR_u/dT = -H(C(rho); .)
    lam_T = solve_lifted(Kt, rhs_T, sink)
    g = (dJdrho - ref.compliance_gradient(x, conn, rho, u, lam_u, method, K0=K0)
         + thermal_T_rho(x, conn, rho, T - T_ref, lam_u, alpha, method, E, nu)
         - conduction_drho_T(x, conn, rho, T, lam_T, k0, k_min, method))
    return dict(rho=rho, T=T, u=u, u_mech=u_mech, u_th=u_th, J=J, grad=W.T @ g, F=F, K=K, Kt=Kt, Q=Q, fixed=fixed, W=W)
