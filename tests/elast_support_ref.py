"""NumPy / SciPy restatement of the elastic supports and displacement outputs of the SIMP elasticity (DESIGN.md section 10,
"Elastic supports and displacement outputs"), written from the formulas:

  K_s(rho) = K(rho) + diag(k)                              sprung_stiffness
  C_l = blockdiag_d(P_l^T A_s P_l)^-1                      multilevel: pr.Multilevel(..., K=K + diag(k))
  J = 1/alpha sum_v a_v (m |u_v|)^p and dJ/du             pnorm_disp, the guards written as == 0
  k of point springs and of a Winkler foundation           point_springs, facet_springs
  filter -> state -> l . u -> adjoint -> W^T               reference_cycle (and pnorm_cycle for the aggregate)
  the force inverter of scripts/run_topopt.py              inverter_case, inverter_loop

No device code, no femo_amd import: meshes come in as (x, conn) arrays."""
import numpy as np
import scipy.sparse as sp

import elast_pc_ref as pr
import elasticity_ref as ref


# ------------------------------------------------------------------------------------------------------ supports ----
def sprung_stiffness(x, conn, rho, k, method="SIMP", E=1.0, nu=0.3, K0=None):
    return (ref.stiffness(x, conn, rho, method, E, nu, K0=K0) + sp.diags(np.asarray(k, dtype=np.float64))).tocsr()


def multilevel(x, conn, rho, k, method="SIMP", fixed_mask=None, spacing_factor=0.0):
    return pr.Multilevel(x, conn, rho, method, fixed_mask, spacing_factor=spacing_factor,
                         K=sprung_stiffness(x, conn, rho, k, method))


def point_springs(n_dof, dofs, k):
    out = np.zeros(n_dof)
    np.add.at(out, np.atleast_1d(dofs), np.broadcast_to(np.asarray(k, dtype=np.float64), np.shape(np.atleast_1d(dofs))))
    return out


def facet_measure(x, f):
    p = x[f]
    if x.shape[1] == 2:
        return np.linalg.norm(p[1] - p[0])
    return 0.5 * np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0]))


def lumped_facets(x, facets):
    """(n_vert,) sum over the facets f around v of |f| / d."""
    d = x.shape[1]
    w = np.zeros(x.shape[0])
    for f in np.asarray(facets).reshape(-1, d):
        w[f] += facet_measure(x, f) / d
    return w


def facet_springs(x, facets, kappa):
    """k_{v,i} = kappa_i sum_{f around v} |f| / d."""
    d = x.shape[1]
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (d,))
    return (lumped_facets(x, facets)[:, None] * kap[None, :]).ravel()


def lumped_cells(x, conn):
    d = x.shape[1]
    w = np.zeros(x.shape[0])
    np.add.at(w, conn.ravel(), np.repeat(ref.cell_volumes(x, conn) / (d + 1), d + 1))
    return w


# ----------------------------------------------------------------------------------------------------- aggregate ----
def pnorm_disp(u, a, m, p, d, alpha=None):
    """(J, dJ/du) of one column: J = 1/alpha sum_v a_v (m |u_v|)^p, dJ/du_{v,i} = p/alpha a_v m (m |u_v|)^(p-1) u_{v,i} / |u_v|.
    A vertex with a_v == 0 is skipped whatever u holds there; a vertex with |u_v| == 0 gives zeros; a non-finite |u_v| makes
    the value and all d gradient entries of its vertex non-finite."""
    a = np.asarray(a, dtype=np.float64)
    alpha = a.sum() if alpha is None or alpha <= 0.0 else alpha
    U = np.asarray(u, dtype=np.float64).reshape(-1, d)
    J, g = 0.0, np.zeros_like(U)
    with np.errstate(all="ignore"):
        for v in np.nonzero(a != 0.0)[0]:
            nrm = np.sqrt(np.sum(U[v] * U[v]))
            if nrm == 0.0:
                continue
            J += a[v] / alpha * (m * nrm) ** p
            wt = p * a[v] / alpha * m * (m * nrm) ** (p - 1.0)
            g[v] = wt * (U[v] / nrm) if np.isfinite(nrm) else np.nan
    return J, g.ravel()


# --------------------------------------------------------------------------------------------------------- cycle ----
def _fixed(mask):
    return np.nonzero(np.asarray(mask) == 1)[0]


def reference_cycle(x, conn, W, x0, k, F, mask, ell, method="SIMP"):
    """filter -> K_s(rho) u = F -> J = l . u -> adjoint K_s lam = l -> dJ/drho = -C' lam^T K0 u -> W^T."""
    rho = W @ x0
    K0 = ref.element_matrices(x, conn)
    K = sprung_stiffness(x, conn, rho, k, method, K0=K0)
    fixed = _fixed(mask)
    u = ref.solve_fixed(K, F, fixed)
    lam = ref.solve_fixed(K, ell, fixed)
    dJ = -ref.compliance_gradient(x, conn, rho, u, lam, method, K0=K0)
    return dict(rho=rho, u=u, J=float(ell @ u), grad=W.T @ dJ, K=K)


def pnorm_cycle(x, conn, W, x0, k, F, mask, a, m, p, method="SIMP"):
    """`reference_cycle` with the aggregate in the place of l . u (the supports are homogeneous, so dJ/du on the fixed dofs
    does not reach the total)."""
    d = x.shape[1]
    rho = W @ x0
    K0 = ref.element_matrices(x, conn)
    K = sprung_stiffness(x, conn, rho, k, method, K0=K0)
    fixed = _fixed(mask)
    u = ref.solve_fixed(K, F, fixed)
    J, g = pnorm_disp(u, a, m, p, d)
    lam = ref.solve_fixed(K, g, fixed)
    dJ = -ref.compliance_gradient(x, conn, rho, u, lam, method, K0=K0)
    return dict(rho=rho, u=u, J=J, grad=W.T @ dJ, dJdu=g)


# ------------------------------------------------------------------------------------------------ force inverter ----
def inverter_case(x, lx=2.0, ly=1.0, kin=0.1, kout=0.1):
    """The half model of the force inverter on the lx x ly rectangle (a structured mesh): the symmetry axis is the top edge
    (a roller: u_y = 0), the clamp is x = 0, y <= 0.1 ly, the input is a unit force in +x on the top-left vertex
    with a spring kin on its x dof, the output the x dof of the top-right vertex with a spring
    kout.  Returns dict(mask, F, k, ell, dof_in, dof_out)."""
    n = x.shape[0]
    top = np.nonzero(np.isclose(x[:, 1], ly))[0]
    left = np.nonzero(np.isclose(x[:, 0], 0.0))[0]
    left = left[np.argsort(x[left, 1])]
    mask = np.zeros(2 * n, dtype=np.uint8)
    mask[2 * top + 1] = 1
    clamp = left[x[left, 1] <= 0.1 * ly + 1e-9]
    mask[2 * clamp] = 1
    mask[2 * clamp + 1] = 1
    v_in = int(left[-1])
    F = np.zeros(2 * n)
    F[2 * v_in] = 1.0
    v_out = int(top[np.argmax(x[top, 0])])
    k = point_springs(2 * n, [2 * v_in, 2 * v_out], [kin, kout])
    ell = np.zeros(2 * n)
    ell[2 * v_out] = 1.0
    return dict(mask=mask, F=F, k=k, ell=ell, dof_in=2 * v_in, dof_out=2 * v_out)


def inverter_loop(x, conn, steps, volume=0.3, move=0.2, kin=0.1, kout=0.1, xmin=1e-3):
    """The design loop of scripts/run_topopt.py --problem inverter with tests/mma_ref.py: minimise u_out / |u_out(x^1)| under
    mean density <= volume from x = volume.  Returns the history of u_out (one more entry than steps: the last design)."""
    import mma_ref
    case = inverter_case(x, x[:, 0].max(), x[:, 1].max(), kin, kout)
    h = ref.mesh_size(x, conn)
    W = ref.filter_matrix(x[conn].mean(axis=1), 2.0 * (h.max() + h.min()) / 2)
    vol = ref.cell_volumes(x, conn)
    nc = len(conn)
    opt = mma_ref.MMA(np.full(nc, xmin), np.ones(nc), 1, move=move)
    xd = np.full(nc, volume)
    hist, scale = [], None
    for _ in range(steps + 1):
        R = reference_cycle(x, conn, W, xd, case["k"], case["F"], case["mask"], case["ell"])
        hist.append(R["J"])
        if len(hist) == steps + 1:
            break
        scale = 1.0 / abs(R["J"]) if scale is None else scale
        g_vol = W.T @ (vol / vol.sum())
        xd = opt.update(xd, scale * R["grad"], [float(vol @ R["rho"] / vol.sum() - volume)], g_vol[None, :])
    return np.array(hist)
