"""NumPy / SciPy restatement of the damped harmonic response of the SIMP elasticity (csrc/elast_damp.hip,
femo_amd/fea/elasticity.py: DampedHarmonicElasticityResidual / DampedDynamicCompliance), on top of tests/elast_harm_ref.py,
written from the formulas alone:

  Z_l      = K(rho) - sigma_l M(rho) + i (cK_l K(rho) + cM_l M(rho)), sigma_l = omega_l^2, cK = eta + omega beta, cM = omega alpha
             for a structural loss factor eta and Rayleigh damping alpha M + beta K; complex symmetric
  direct   complex sparse LU of Z on the free dofs
  cocr     the device's loop step by step for one column: the preconditioned COCR of Sogabe & Zhang (2007) with a real SPD
           preconditioner applied to both parts, z = M^-1 r carried by its recurrence, x = b on the fixed dofs, stopped on
           sqrt(Re(r^H z)) <= max(rtol beta1, atol) with beta1 that of the first residual
  J        = sum_l w_l |c_l| or sum_l w_l |c_l|^2, c_l = F_l . u_l complex and unconjugated;
           dc_l/drho_e = - u_e^T [C'(rho_e) K0_e (1 + i cK) - density m'(rho_e) M0_e (sigma_l - i cM)] u_e, unconjugated (Z is
           symmetric: the adjoint of c_l is u_l itself), and dJ/drho = sum_l w_l Re(conj(c_l) / |c_l| dc_l/drho), the factor
           2 conj(c_l) for the square
  problem  the set-up the host and the GPU tests share: that of `elast_harm_ref.problem` with the shifts
           {lambda_1 / 2, lambda_1, sqrt(lambda_1 lambda_2), sqrt(lambda_5 lambda_6)} -- the second sits on a resonance
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elast_eig_ref as er
import elast_harm_ref as hr
import elasticity_ref as ref

# (stiffness law, mass law, eta, alpha, beta)
CASES = (("SIMP", "linear", 0.05, 0.0, 0.0), ("RAMP", "du_olhoff", 0.0, 0.02, 0.02))
RESONANT = 1            # the shift of `shifts_of` that equals lambda_1


def coefficients(sigmas, eta=0.0, alpha=0.0, beta=0.0):
    """(cK, cM) per shift."""
    om = np.sqrt(np.asarray(sigmas, dtype=np.float64))
    return eta + om * beta, om * alpha


def Z(K, M, sigma, ck, cm):
    return ((K - sigma * M) + 1j * (ck * K + cm * M)).tocsr()


def masked_Z(K, M, sigma, ck, cm, fixed_mask):
    """Z with identity rows and columns on the fixed dofs (of both parts)."""
    if fixed_mask is None:
        return Z(K, M, sigma, ck, cm)
    fm = np.asarray(fixed_mask)
    free = sp.diags((fm == 0).astype(np.float64))
    return (free @ Z(K, M, sigma, ck, cm) @ free + sp.diags(fm.astype(np.complex128))).tocsr()


def direct(K, M, sigma, ck, cm, F, fixed_mask):
    """Complex u with zeros on the fixed dofs and Z u = F on the others."""
    free = np.nonzero(np.asarray(fixed_mask) == 0)[0]
    Zf = Z(K, M, sigma, ck, cm)[free][:, free].tocsc()
    u = np.zeros(K.shape[0], dtype=np.complex128)
    u[free] = spla.splu(Zf).solve(np.asarray(F, dtype=np.complex128)[free])
    return u


def _div(a, b):
    """a / b as the device forms it; (quotient, False) when the denominator is zero or the quotient not finite."""
    ar, ai, br, bi = (np.float64(v) for v in (a.real, a.imag, b.real, b.imag))
    with np.errstate(all="ignore"):
        den = br * br + bi * bi
        q = complex((ar * br + ai * bi) / den, (ai * br - ar * bi) / den)
    return q, bool(den != 0.0 and np.isfinite(q.real) and np.isfinite(q.imag))


def cocr(Zm, b, precond, fixed_mask=None, rtol=1e-12, atol=0.0, max_it=100000, x0=None):
    """One column of the device's loop (the columns of a batched solve do not see one another).  ``precond``: the real
    preconditioner, applied to both parts.  Returns dict(x, iterations, converged (1, 0: max_it, -1: a non-finite value or a
    zero denominator of alpha or beta), res, beta1)."""
    b = np.asarray(b, dtype=np.complex128)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.complex128)
    if fixed_mask is not None:
        fx = np.asarray(fixed_mask) == 1
        x[fx] = b[fx]
    pc = lambda v: precond(v.real) + 1j * precond(v.imag)
    r = b - Zm @ x
    z = pc(r)
    with np.errstate(invalid="ignore"):
        beta1 = float(np.sqrt(np.vdot(r, z).real))
    out = dict(x=x, iterations=0, converged=0, res=beta1, beta1=beta1)
    tol = max(rtol * beta1, atol)
    if not np.isfinite(beta1):
        return dict(out, converged=-1)
    if beta1 <= tol:
        return dict(out, converged=1)
    rho, p, q, res = 0j, None, None, beta1
    for it in range(1, max_it + 1):
        w = Zm @ z
        rho_new = complex(z @ w)                                       # unconjugated
        if not (np.isfinite(rho_new.real) and np.isfinite(rho_new.imag)):
            return dict(out, x=x, iterations=it - 1, converged=-1, res=res)
        if it == 1:
            p, q = z.copy(), w
        else:
            beta, ok = _div(rho_new, rho)
            if not ok:
                return dict(out, x=x, iterations=it - 1, converged=-1, res=res)
            p, q = z + beta * p, w + beta * q
        rho = rho_new
        mq = pc(q)
        alpha, ok = _div(rho, complex(q @ mq))
        if not ok:
            return dict(out, x=x, iterations=it - 1, converged=-1, res=res)
        x = x + alpha * p
        r = r - alpha * q
        z = z - alpha * mq
        with np.errstate(invalid="ignore"):
            res = float(np.sqrt(np.vdot(r, z).real))
        if not np.isfinite(res):
            return dict(out, x=x, iterations=it, converged=-1, res=res)
        if res <= tol:
            return dict(out, x=x, iterations=it, converged=1, res=res)
    return dict(out, x=x, iterations=max_it, converged=0, res=res)


def backward_error(Zm, x, b):
    """|b - Z x|_2 / (|Z|_1 |x|_2 + |b|_2)"""
    return np.linalg.norm(b - Zm @ x) / (abs(Zm).sum(axis=0).max() * np.linalg.norm(x) + np.linalg.norm(b))


def compliance_value(c, weights=None, squared=False):
    """(J, g) of J = sum_l w_l |c_l| or sum_l w_l |c_l|^2 with dJ = sum_l Re(g_l dc_l): g = w conj(c) / |c|, or 2 w conj(c)."""
    c = np.asarray(c, dtype=np.complex128)
    w = np.ones(len(c)) if weights is None else np.asarray(weights, dtype=np.float64)
    a = np.abs(c)
    if squared:
        return float(w @ (a * a)), 2.0 * w * np.conj(c)
    return float(w @ a), w * np.conj(c) / a


def responses(x, conn, rho, fixed_mask, F, sigmas, ck, cm, method="SIMP", law="linear", density=1.0):
    """(U complex (L, n_dof) by direct solves, c_l = F_l . u_l)."""
    K = ref.stiffness(x, conn, rho, method)
    M = er.mass(x, conn, rho, law, density)
    U = np.stack([direct(K, M, s, a, b, Fl, fixed_mask) for s, a, b, Fl in zip(sigmas, ck, cm, F)])
    return U, np.einsum("li,li->l", np.asarray(F), U)


def response_gradients(x, conn, rho, U, sigmas, ck, cm, method="SIMP", law="linear", density=1.0):
    """(L, n_cell) complex: d c_l / d rho_e = - u_e^T [C'(rho_e) K0_e (1 + i cK) - density m'(rho_e) M0_e (sigma_l - i cM)] u_e."""
    eK, eM = er.eig_drho_terms(x, conn, np.asarray(U).T)              # unconjugated u^T K0 u, u^T M0 u
    s, ck, cm = (np.asarray(v, dtype=np.float64)[:, None] for v in (sigmas, ck, cm))
    return -(ref.penal_d(rho, method)[None, :] * eK * (1.0 + 1j * ck)
             - (density * er.mass_law_d(rho, law))[None, :] * eM * (s - 1j * cm))


def adjoint_total(x, conn, rho, fixed_mask, F, sigmas, ck, cm, weights=None, squared=False, method="SIMP", law="linear",
                  density=1.0):
    """(J, dJ/drho, c, U) with the direct solves."""
    U, c = responses(x, conn, rho, fixed_mask, F, sigmas, ck, cm, method, law, density)
    J, g = compliance_value(c, weights, squared)
    G = response_gradients(x, conn, rho, U, sigmas, ck, cm, method, law, density)
    return J, np.real(g @ G), c, U


def shifts_of(lam):
    """sigma in {lambda_1 / 2, lambda_1, sqrt(lambda_1 lambda_2), sqrt(lambda_5 lambda_6)}: the second sits on a resonance."""
    return np.array([0.5 * lam[0], lam[0], np.sqrt(lam[0] * lam[1]), np.sqrt(lam[4] * lam[5])])


def problem(mesh, method, law, eta, alpha, beta, density=hr.DENSITY):
    """`elast_harm_ref.problem` with the four shifts of `shifts_of` and the damping coefficients ck, cm per shift."""
    P = dict(hr.problem(mesh, method, law, density))
    P["shifts"] = shifts_of(P["lam"])
    P["ck"], P["cm"] = coefficients(P["shifts"], eta, alpha, beta)
    P.update(eta=eta, alpha=alpha, beta=beta)
    return P


def split(U):
    """(L, n) complex -> (2L, n) real: Re in row 2 l, Im in row 2 l + 1."""
    U = np.asarray(U)
    out = np.empty((2 * U.shape[0], U.shape[1]))
    out[0::2], out[1::2] = U.real, U.imag
    return out


def join(X):
    """(2L, n) real -> (L, n) complex."""
    X = np.asarray(X)
    return X[0::2] + 1j * X[1::2]
