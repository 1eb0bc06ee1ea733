"""NumPy / SciPy restatement of the batched multi-load path of the SIMP elasticity (csrc/elast_solve.hip,
femo_amd/fea/elasticity.py: MultiLoadElasticityResidual / MultiLoadCompliance), on top of tests/elasticity_ref.py and
tests/elast_pc_ref.py:

  pcg_multi              the device's batched PCG: all columns step together, each with its own scalars and its own
                         stopping test; a finished column is frozen (its x, r, p are not touched again)
  right_hand_sides, cantilever_loads   the inputs the host and the GPU tests share
  reference_cycle_multi  filter -> K(rho) u_l = F_l per load (direct solves) -> J = sum_l w_l F_l . u_l ->
                         dJ/dx = W^T sum_l w_l (-C'(rho) u_l^T K0 u_l)
"""
from __future__ import annotations

import numpy as np

import elasticity_ref as ref


def pcg_multi(A, B, precond, fixed_mask=None, rtol=1e-15, atol=0.0, max_it=100000):
    """B: (L, n).  The protocol of elast_pc_ref.pcg for every column, in lock step.  Returns a list of
    (x, iterations, converged) per column."""
    B = np.asarray(B, dtype=np.float64)
    L = B.shape[0]
    X = np.zeros_like(B)
    if fixed_mask is not None:
        fx = np.asarray(fixed_mask) == 1
        X[:, fx] = B[:, fx]
    R = np.empty_like(B)
    P = np.empty_like(B)
    rz = np.zeros(L)
    tol2 = np.zeros(L)
    done = np.zeros(L, dtype=bool)
    conv = np.zeros(L, dtype=bool)
    its = np.zeros(L, dtype=np.int64)
    for l in range(L):
        R[l] = B[l] - A @ X[l]
        z = precond(R[l])
        P[l] = z.copy()
        rz[l] = R[l] @ z
        tol2[l] = max(rtol * rtol * rz[l], atol * atol)
        if not rz[l] == rz[l]:
            done[l] = True                              # breakdown at the start
        elif rz[l] <= tol2[l]:
            done[l] = conv[l] = True
    for it in range(1, max_it + 1):
        if done.all():
            break
        for l in range(L):
            if done[l]:
                continue                                # frozen: nothing of this column is touched
            q = A @ P[l]
            pq = P[l] @ q
            if not pq > 0.0:
                done[l] = True
                continue
            alpha = rz[l] / pq
            X[l] += alpha * P[l]
            R[l] -= alpha * q
            z = precond(R[l])
            rz_new = R[l] @ z
            its[l] = it
            if not rz_new == rz_new:
                done[l] = True
            elif rz_new <= tol2[l]:
                done[l] = conv[l] = True
            else:
                P[l] = z + (rz_new / rz[l]) * P[l]
                rz[l] = rz_new
    return [(X[l], int(its[l]), bool(conv[l])) for l in range(L)]


def reference_cycle_multi(mesh, facets_list, tractions, weights, h_avg, x0, method="SIMP"):
    """filter -> one direct solve per load (clamped at x = 0) -> weighted compliance -> its gradient."""
    d = mesh.tdim
    W = ref.filter_matrix(mesh.centroids(), 2.0 * h_avg)
    rho = W @ x0
    K0 = ref.element_matrices(mesh.x, mesh.conn)
    K = ref.stiffness(mesh.x, mesh.conn, rho, method, K0=K0)
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    fixed = np.concatenate([d * fixed_v + k for k in range(d)])
    w = np.ones(len(tractions)) if weights is None else np.asarray(weights, dtype=np.float64)
    F = [ref.traction_load(mesh.x, f, t) for f, t in zip(facets_list, tractions)]
    u = [ref.solve_fixed(K, Fl, fixed) for Fl in F]
    J = float(sum(wl * (Fl @ ul) for wl, Fl, ul in zip(w, F, u)))
    dJ = np.zeros(mesh.n_cell)
    for wl, ul in zip(w, u):
        dJ -= wl * ref.compliance_gradient(mesh.x, mesh.conn, rho, ul, ul, method, K0=K0)
    return dict(rho=rho, u=u, J=J, grad=W.T @ dJ, K=K, F=F, fixed=fixed)


# --------------------------------------------------------------------------------- shared inputs of the two test files ----
def right_hand_sides(mesh, mask):
    """The five columns of the batched tests, in their order: a unit pull in component 0 on the face x = x_max, noise,
    zeros, 1e6 times the first, and -1 in the last component of the first vertex of that face.  Fixed entries zeroed."""
    d, n = mesh.tdim, mesh.tdim * mesh.n_vert
    face = np.nonzero(np.isclose(mesh.x[:, 0], mesh.x[:, 0].max()))[0]
    b0 = np.zeros(n)
    b0[d * face] = 1.0
    b4 = np.zeros(n)
    b4[d * face[0] + d - 1] = -1.0
    B = np.stack([b0, np.random.default_rng(11).standard_normal(n), np.zeros(n), 1e6 * b0, b4])
    B[:, mask == 1] = 0.0
    return B


def cantilever_loads(mesh, lx, ly, nely):
    """The three loads of the multi-load cycle: (facets, traction) per load."""
    from femo_amd.fea.mesh import locate_entities_boundary
    eps = 3e-6 * max(1.0, lx / 160.0)
    markers = [lambda x: np.logical_and(abs(x[1] - ly / 2) < ly / nely + eps, abs(x[0] - lx) < eps),
               lambda x: np.logical_and(abs(x[1] - ly) < eps, x[0] > 0.75 * lx - eps),
               lambda x: abs(x[0] - lx) < eps]
    facets = [locate_entities_boundary(mesh, mesh.tdim - 1, m) for m in markers]
    return facets, [(0.0, -0.25), (0.0, -0.25), (0.25, 0.0)]
