"""NumPy restatement of the aggregated von Mises stress over several load cases (femo_amd/fea/elasticity.py:
MultiLoadPnormStress / MultiLoadVonMises; kernels in csrc/elast_stress.hip), on top of tests/elast_stress_ref.py:

  J_l = (1/alpha) sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p       elast_stress_ref.pnorm_stress of column l with scale m_l
  J   = sum_l w_l J_l
  dJ/du: column l = w_l dJ_l/du_l;   dJ/drho = sum_l w_l dJ_l/drho, summed in ascending l
  envelope_e = max_l s_l rho_e^q sigma_vm,e(u_l)

The total derivative of the filtered multi-load cantilever has one adjoint solve per column, K lambda_l = w_l dJ_l/du_l
on the free dofs and lambda_l = 0 on the clamped ones:  dJ/dx = W^T (dJ/drho - sum_l lambda_l^T dK/drho u_l)."""
from __future__ import annotations

import numpy as np

import elast_stress_ref as sref
import elasticity_ref as ref


def pnorm_stress_multi(x, conn, rho, U, m, p=8.0, q=0.5, alpha=None, weights=None):
    """U: (L, n_dof).  dict(values (L,), value, du (L, n_dof), drho, fields (L, n_cell), alpha)."""
    U = np.asarray(U, dtype=np.float64)
    L = U.shape[0]
    m = np.full(L, float(m)) if np.ndim(m) == 0 else np.asarray(m, dtype=np.float64)
    w = np.ones(L) if weights is None else np.asarray(weights, dtype=np.float64)
    cols = [sref.pnorm_stress(x, conn, rho, U[l], m[l], p, q, alpha) for l in range(L)]
    drho = np.zeros(len(conn))
    for l in range(L):
        drho += w[l] * cols[l]["drho"]
    values = np.array([c["value"] for c in cols])
    return dict(values=values, value=float(w @ values), du=np.stack([w[l] * cols[l]["du"] for l in range(L)]), drho=drho,
                fields=np.stack([c["field"] for c in cols]), alpha=cols[0]["alpha"])


def envelope(fields, scales=None):
    """max_l s_l field_l over the rows of ``fields`` (L, n_cell)."""
    s = np.ones(len(fields)) if scales is None else np.asarray(scales, dtype=np.float64)
    return (s[:, None] * fields).max(axis=0)


def scales_from_state(x, conn, U, rho, q):
    """m_l = 1 / max_e rho_e^q sigma_vm,e(u_l)."""
    return np.array([1.0 / sref.cell_field(x, conn, u, rho, q).max() for u in U])


# ------------------------------------------------------------------------------------- the filtered multi-load cantilever ----
def cantilever_problem_multi(mesh, facets_list, tractions, h_avg):
    """elast_stress_ref.cantilever_problem with one load per (facets, traction) under "F" (L, n_dof)."""
    P = sref.cantilever_problem(mesh, facets_list[0], h_avg, tractions[0])
    P["F"] = np.stack([ref.traction_load(mesh.x, f, t) for f, t in zip(facets_list, tractions)])
    return P


def cantilever_states(P, x0, method="SIMP"):
    rho = P["W"] @ x0
    K = ref.stiffness(P["x"], P["conn"], rho, method, K0=P["K0"])
    return rho, K, np.stack([ref.solve_fixed(K, F, P["fixed"]) for F in P["F"]])


def cantilever_value_multi(P, x0, m, weights, p=8.0, q=0.5):
    rho, _, U = cantilever_states(P, x0)
    return pnorm_stress_multi(P["x"], P["conn"], rho, U, m, p, q, weights=weights)["value"]


def cantilever_total_multi(P, x0, m, weights, p=8.0, q=0.5, method="SIMP"):
    """dict(value, values, grad, rho, U, lam (L, n_dof), du, drho)."""
    rho, K, U = cantilever_states(P, x0, method)
    R = pnorm_stress_multi(P["x"], P["conn"], rho, U, m, p, q, weights=weights)
    lam = np.stack([ref.solve_fixed(K, R["du"][l], P["fixed"]) for l in range(len(U))])    # zero on the clamped dofs
    total_rho = R["drho"].copy()
    for l in range(len(U)):
        total_rho -= ref.compliance_gradient(P["x"], P["conn"], rho, U[l], lam[l], method, K0=P["K0"])
    return dict(value=R["value"], values=R["values"], grad=P["W"].T @ total_rho, rho=rho, U=U, lam=lam, du=R["du"],
                drho=R["drho"], fields=R["fields"])


# ------------------------------------------------------------------------------------------------ inputs of the tests ----
def random_columns(x, conn, L, seed=0):
    """L random columns whose magnitudes differ by 1e3 from the first to the last, rho in U(1e-3, 1), m_l = 1 / max
    sigma_vm(u_l) and random weights in U(0.25, 2)."""
    rng = np.random.default_rng(seed)
    mags = 10.0 ** np.linspace(0.0, -3.0, L) if L > 1 else np.ones(1)
    U = rng.standard_normal((L, x.size)) * mags[:, None]
    rho = rng.uniform(1e-3, 1.0, len(conn))
    m = np.array([1.0 / sref.von_mises(x, conn, u).max() for u in U])
    return U, rho, m, rng.uniform(0.25, 2.0, L)
