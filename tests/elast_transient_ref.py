"""NumPy / SciPy restatement of the transient response of the SIMP elasticity (csrc/elast_transient.hip,
femo_amd/fea/elasticity.py: TransientElasticityResidual / TransientCompliance), on top of tests/elasticity_ref.py,
tests/elast_eig_ref.py and tests/elast_harm_ref.py for K, M and their density derivatives, written from the formulas alone.

Newmark(beta, gamma) with Rayleigh damping C = c_m M + c_k K as its two-step recurrence in the displacements, from rest
(u_0 = u_-1 = 0, g_-1 = 0), for n = 0 ... N - 1:

  A1 u_{n+1} + A0 u_n + A- u_{n-1} = dt^2 (beta g_{n+1} + b0 g_n + b- g_{n-1}) F,     A_j = m_j M + k_j K

  blocks     the scalars (m_j, k_j), b0 = 1/2 + gamma - 2 beta, b- = 1/2 - gamma + beta
  operators  A1 with identity rows / columns on the fixed dofs, A0 and A- with zero ones (homogeneous supports)
  band       L as ONE sparse matrix on the history U = (u_1 ... u_N): block lower-banded, block-Toeplitz, symmetric blocks
  march      the recurrence with splu(A1); reverse = True runs it from the last column to the first and solves L^T
  drho_*     dR/drho of R = L U - B: column t is C'(rho) K0 uK_t + density m'(rho) M0 uM_t, uK_t = sum_j k_j u_{t+j}
  adjoint_total  J = sum_n w_n c_n or sum_n w_n c_n^2, c_n = F . u_n, with the discrete adjoint L^T Lambda = dJ/dU and
             dJ/drho = -(dR/drho)^T Lambda
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elast_eig_ref as er
import elast_harm_ref as hr
import elasticity_ref as ref

DENSITY = hr.DENSITY
CASES = hr.CASES                                           # (stiffness law, mass law)
# (beta, gamma, (c_m, c_k)): the average-acceleration rule undamped and damped, and a dissipative pair
SCHEMES = ((0.25, 0.5, (0.0, 0.0)), (0.25, 0.5, (0.05, 0.002)), (0.3025, 0.6, (0.0, 0.0)), (0.3025, 0.6, (0.05, 0.002)))
STEP_COUNTS = (1, 2, 8, 9, 19)


def blocks(dt, beta=0.25, gamma=0.5, rayleigh=(0.0, 0.0)):
    """dict(m=(m1, m0, m-), k=(k1, k0, k-), b0, bm, dt, beta)."""
    cm, ck = rayleigh
    b0, bm = 0.5 + gamma - 2.0 * beta, 0.5 - gamma + beta
    m = (1.0 + gamma * dt * cm, -2.0 + (1.0 - 2.0 * gamma) * dt * cm, 1.0 - (1.0 - gamma) * dt * cm)
    k = (gamma * dt * ck + beta * dt * dt, (1.0 - 2.0 * gamma) * dt * ck + b0 * dt * dt, -(1.0 - gamma) * dt * ck + bm * dt * dt)
    return dict(m=m, k=k, b0=b0, bm=bm, dt=dt, beta=beta, gamma=gamma, rayleigh=(cm, ck))


def operators(K, M, mask, c):
    """(A1, A0, A-); with a mask A1 carries identity rows / columns on the fixed dofs and A0, A- zero ones."""
    A = [(c["m"][j] * M + c["k"][j] * K).tocsr() for j in range(3)]
    if mask is None:
        return A
    fixed = np.asarray(mask, dtype=np.float64)
    free = sp.diags(1.0 - fixed)
    return [(free @ A[0] @ free + sp.diags(fixed)).tocsr(), (free @ A[1] @ free).tocsr(), (free @ A[2] @ free).tocsr()]


def band(K, M, mask, n_steps, c):
    """L (N n x N n) of the history, column t = u_{t+1} at t * n."""
    A1, A0, Am = operators(K, M, mask, c)
    N = n_steps
    sub = lambda k: sp.csr_matrix((np.ones(max(N - k, 0)), (np.arange(k, N), np.arange(0, max(N - k, 0)))), shape=(N, N))
    return (sp.kron(sp.identity(N), A1) + sp.kron(sub(1), A0) + sp.kron(sub(2), Am)).tocsr()


def signal_coefficients(g, c):
    """(N,): dt^2 (beta g_{t+1} + b0 g_t + b- g_{t-1}), g_-1 = 0, for the N + 1 samples g."""
    g = np.asarray(g, dtype=np.float64)
    gm = np.concatenate([[0.0], g[:-2]]) if len(g) >= 2 else np.zeros(0)
    return c["dt"] ** 2 * (c["beta"] * g[1:] + c["b0"] * g[:-1] + c["bm"] * gm)


def load_history(F, g, c, mask=None):
    """(N, n): the right-hand sides of the N steps, zero on the fixed dofs."""
    Fm = np.asarray(F, dtype=np.float64) if mask is None else np.where(np.asarray(mask) == 1, 0.0, F)
    return np.outer(signal_coefficients(g, c), Fm)


def march(K, M, mask, B, c, reverse=False):
    """(N, n): L U = B, or L^T U = B with ``reverse`` -- the same loop from the last column to the first."""
    A1, A0, Am = operators(K, M, mask, c)
    lu = spla.splu(A1.tocsc())
    B = np.asarray(B, dtype=np.float64)
    N, n = B.shape
    U = np.zeros((N, n))
    order = range(N - 1, -1, -1) if reverse else range(N)
    step = 1 if reverse else -1
    for t in order:
        b = B[t].copy()
        if 0 <= t + step < N:
            b -= A0 @ U[t + step]
        if 0 <= t + 2 * step < N:
            b -= Am @ U[t + 2 * step]
        U[t] = lu.solve(b)
    return U


def scalar_recurrence(lam, g, c):
    """q_1 ... q_N of one mode K phi = lam M phi under F = M phi: the recurrence with M -> 1, K -> lam."""
    a = [c["m"][j] + c["k"][j] * lam for j in range(3)]
    f = signal_coefficients(g, c)
    q = np.zeros(len(f) + 2)                               # q[t + 2] = q_{t+1}; q_0 = q_-1 = 0
    for t in range(len(f)):
        q[t + 2] = (f[t] - a[1] * q[t + 1] - a[2] * q[t]) / a[0]
    return q[2:]


def energies(K, M, U, dt):
    """E_{n+1/2} = 1/2 v^T M v + 1/2 ub^T K ub, v = (u_{n+1} - u_n) / dt, ub = (u_{n+1} + u_n) / 2, for n = 0 ... N - 1."""
    W = np.vstack([np.zeros((1, U.shape[1])), U])
    v, ub = (W[1:] - W[:-1]) / dt, 0.5 * (W[1:] + W[:-1])
    return 0.5 * np.einsum("ti,ti->t", v, (M @ v.T).T) + 0.5 * np.einsum("ti,ti->t", ub, (K @ ub.T).T)


def combined(U, c):
    """(uK, uM), each (N, n): uK_t = k1 u_{t+1} + k0 u_t + k- u_{t-1} in the columns of the history."""
    W = np.vstack([np.zeros((2, U.shape[1])), U])
    uK = c["k"][0] * W[2:] + c["k"][1] * W[1:-1] + c["k"][2] * W[:-2]
    uM = c["m"][0] * W[2:] + c["m"][1] * W[1:-1] + c["m"][2] * W[:-2]
    return uK, uM


def drho_T(x, conn, rho, U, X, c, method="SIMP", law="linear", density=1.0, K0=None, M0=None):
    """(n_cell,): sum_t (dR_t/drho)^T x_t, unmasked."""
    d = x.shape[1]
    K0 = ref.element_matrices(x, conn) if K0 is None else K0
    M0 = er.element_mass_matrices(x, conn) if M0 is None else M0
    dofs = ref.element_dofs(conn, d)
    uK, uM = combined(U, c)
    X = np.asarray(X)
    eK = np.einsum("tei,eij,tej->e", X[:, dofs], K0, uK[:, dofs])
    eM = np.einsum("tei,eij,tej->e", X[:, dofs], M0, uM[:, dofs])
    return ref.penal_d(rho, method) * eK + density * er.mass_law_d(rho, law) * eM


def drho_N(x, conn, rho, U, dr, c, method="SIMP", law="linear", density=1.0, K0=None, M0=None):
    """(N, n): dR_t/drho dr, unmasked."""
    d = x.shape[1]
    K0 = ref.element_matrices(x, conn) if K0 is None else K0
    M0 = er.element_mass_matrices(x, conn) if M0 is None else M0
    dofs = ref.element_dofs(conn, d)
    uK, uM = combined(U, c)
    tK = (ref.penal_d(rho, method) * dr)[None, :, None] * np.einsum("eij,tej->tei", K0, uK[:, dofs])
    tM = (density * er.mass_law_d(rho, law) * dr)[None, :, None] * np.einsum("eij,tej->tei", M0, uM[:, dofs])
    Y = np.zeros_like(U)
    for t in range(U.shape[0]):
        np.add.at(Y[t], dofs.ravel(), (tK[t] + tM[t]).ravel())
    return Y


def gradient_conditioning(x, conn, rho, U, Lam, c, method="SIMP", law="linear", density=1.0):
    """max_e of the sum of the magnitudes of the terms of (dR/drho)^T Lambda (per step, stiffness and mass apart) over
    max_e |its value|: how much a relative error of U and Lambda is amplified in the max norm of dJ/drho."""
    d = x.shape[1]
    K0, M0 = ref.element_matrices(x, conn), er.element_mass_matrices(x, conn)
    dofs = ref.element_dofs(conn, d)
    uK, uM = combined(U, c)
    eK = np.abs(np.einsum("tei,eij,tej->te", Lam[:, dofs], K0, uK[:, dofs])).sum(axis=0)
    eM = np.abs(np.einsum("tei,eij,tej->te", Lam[:, dofs], M0, uM[:, dofs])).sum(axis=0)
    mag = ref.penal_d(rho, method) * eK + density * np.abs(er.mass_law_d(rho, law)) * eM
    return float(mag.max() / np.abs(drho_T(x, conn, rho, U, Lam, c, method, law, density, K0, M0)).max())


def objective(cn, weights, squared=False):
    """(J, dJ/dc) of J = sum_n w_n c_n or sum_n w_n c_n^2."""
    cn, w = np.asarray(cn, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    return (float(w @ (cn * cn)), 2.0 * w * cn) if squared else (float(w @ cn), w.copy())


def state(x, conn, rho, mask, F, g, c, method="SIMP", law="linear", density=1.0):
    """(U, c_n, K, M)."""
    K = ref.stiffness(x, conn, rho, method)
    M = er.mass(x, conn, rho, law, density)
    U = march(K, M, mask, load_history(F, g, c, mask), c)
    return U, U @ np.asarray(F), K, M


def adjoint_total(x, conn, rho, mask, F, g, c, weights=None, squared=False, method="SIMP", law="linear", density=1.0):
    """(J, dJ/drho, c_n, U, Lambda) with the discrete adjoint; the default weights are dt."""
    U, cn, K, M = state(x, conn, rho, mask, F, g, c, method, law, density)
    w = np.full(len(cn), c["dt"]) if weights is None else np.asarray(weights, dtype=np.float64)
    J, dJdc = objective(cn, w, squared)
    S = np.outer(dJdc, np.where(np.asarray(mask) == 1, 0.0, F) if mask is not None else F)
    Lam = march(K, M, mask, S, c, reverse=True)
    return J, -drho_T(x, conn, rho, U, Lam, c, method, law, density), cn, U, Lam


def default_signal(n_steps):
    """N + 1 samples of a smooth pulse that is not symmetric in time."""
    t = np.arange(n_steps + 1, dtype=np.float64)
    return np.sin(0.7 * t + 0.3) * np.exp(-0.05 * t) + 0.25


def problem(mesh, method, law, density=DENSITY, void=False):
    """Clamped on x = 0, rho = default_rng(7).uniform(0.3, 1) (with ``void`` every fifth cell at 1e-3), the end-face load, the
    first eigenvalue of the dense pencil and dt = T_1 / 20."""
    P = hr.problem(mesh, method, law, density)
    if void:
        rho = P["rho"].copy()
        rho[::5] = 1e-3
        K = ref.stiffness(mesh.x, mesh.conn, rho, method)
        M = er.mass(mesh.x, mesh.conn, rho, law, density)
        P = dict(P, rho=rho, K=K, M=M, lam=er.dense_eigs(K, M, P["mask"], 6)[0])
    return dict(P, dt=2.0 * np.pi / np.sqrt(P["lam"][0]) / 20.0)
