"""NumPy restatement of the Heaviside projection of the SIMP design chain (include/femo_hip.h, "Heaviside projection";
csrc/project.hip), its volume-preserving threshold, both Jacobian products, the grayness measure and the continuation loop.

Every function takes ``dtype``: ``float`` restates the arithmetic, ``np.longdouble`` (64-bit significand on x86-64) is the
reference the device is measured against.  It shares no code with the kernels.

    D     = tanh(beta eta) + tanh(beta (1 - eta))
    H     = (tanh(beta eta) + tanh(beta (x - eta))) / D
    H_x   = beta (1 - tanh^2(beta (x - eta))) / D
    H_eta = (N_eta D - N D_eta) / D^2,  N = tanh(beta eta) + tanh(beta (x - eta)),
            N_eta = beta (tanh^2(beta (x - eta)) - tanh^2(beta eta)),  D_eta = beta (tanh^2(beta (1 - eta)) - tanh^2(beta eta))

beta = 0 is the identity: H = x, H_x = 1, H_eta = 0.

Error bounds of the fp64 evaluation (eps = 2^-52, one rounding <= eps / 2 relative; none of them is fitted to the kernels).
A tanh is taken to be within 2 eps of its value relative (twice the 1 ulp that the HIP math library documents for fp64 tanh;
the host's is closer), and its argument z = beta (x - eta) carries two roundings, relative eps in all, which move tanh by at
most z sech^2(z) eps <= 0.448 eps.  So every tanh is within t_err = 2.45 eps absolute (|tanh| <= 1).

  N, D      two tanh and one sum of magnitude <= 2:                 |dN|, |dD| <= 2 t_err + eps = 5.9 eps
  H         = N / D with |H| <= 1 for x in [0, 1]:                  |dH| <= (dN + dD) / D + eps / 2 <= eps (11.8 / D + 0.5)
  H_x       1 - t^2: 2 |t| t_err + two roundings <= 5.9 eps; times beta, by D (relative dD / D), two roundings:
                                                                    |dH_x| <= eps (beta / D) (5.9 + (1 - t^2) (1 + 5.9 / D))
  H_eta     N_eta, D_eta = beta (a^2 - b^2): 4 t_err + 3 roundings of terms <= 1: <= 11.3 beta eps each; the numerator
            N_eta D - N D_eta with |N_eta|, |D_eta| <= beta and N, D <= 2: 2 x 2 x 11.3 beta eps + 2 x 5.9 beta eps + three
            roundings of terms <= 2 beta <= 60 beta eps; by D^2 (relative 2 dD / D + eps):
                                                                    |dH_eta| <= eps (60 beta / D^2 + |H_eta| (1.5 + 11.8 / D))

``bound_H``, ``bound_Hx`` and ``bound_Heta`` return these with 5 % on top for the second-order terms."""
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
BISECT_STEPS = 53
T_ERR = 2.45 * EPS


# ---- the projection and its two partial derivatives -----------------------------------------------------------------------
def _parts(x, beta, eta, dtype):
    x = np.asarray(x, dtype=dtype)
    beta, eta = dtype(beta), dtype(eta)
    a = np.tanh(beta * eta)
    b = np.tanh(beta * (dtype(1.0) - eta))
    t = np.tanh(beta * (x - eta))
    return x, beta, a, b, t, a + b


def H(x, beta, eta, dtype=float):
    if beta == 0.0:
        return np.array(x, dtype=dtype, copy=True)
    x, beta, a, b, t, D = _parts(x, beta, eta, dtype)
    return (a + t) / D


def H_x(x, beta, eta, dtype=float):
    if beta == 0.0:
        return np.ones(np.shape(x), dtype=dtype)
    x, beta, a, b, t, D = _parts(x, beta, eta, dtype)
    return beta * (dtype(1.0) - t * t) / D


def H_eta(x, beta, eta, dtype=float):
    if beta == 0.0:
        return np.zeros(np.shape(x), dtype=dtype)
    x, beta, a, b, t, D = _parts(x, beta, eta, dtype)
    N = a + t
    N_eta = beta * (t * t - a * a)
    D_eta = beta * (b * b - a * a)
    return (N_eta * D - N * D_eta) / (D * D)


def denominator(beta, eta, dtype=float):
    return np.tanh(dtype(beta) * dtype(eta)) + np.tanh(dtype(beta) * (dtype(1.0) - dtype(eta)))


def bound_H(beta, eta):
    if beta == 0.0:
        return 0.0
    return 1.05 * EPS * (11.8 / float(denominator(beta, eta, LD)) + 0.5)


def bound_Hx(x, beta, eta):
    """Per entry."""
    if beta == 0.0:
        return np.zeros(np.shape(x))
    D = float(denominator(beta, eta, LD))
    s = np.asarray(H_x(x, beta, eta, LD) * LD(D) / LD(beta), dtype=float)          # 1 - t^2
    return 1.05 * EPS * (beta / D) * (5.9 + s * (1.0 + 5.9 / D))


def bound_Heta(x, beta, eta):
    """Per entry."""
    if beta == 0.0:
        return np.zeros(np.shape(x))
    D = float(denominator(beta, eta, LD))
    return 1.05 * EPS * (60.0 * beta / D ** 2 + np.abs(np.asarray(H_eta(x, beta, eta, LD), dtype=float)) * (1.5 + 11.8 / D))


# ---- passive cells --------------------------------------------------------------------------------------------------------
def flags(n, solid=(), void=()):
    """0 active, 1 solid, -1 void."""
    f = np.zeros(n, dtype=np.int8)
    f[np.asarray(solid, dtype=np.int64)] = 1
    f[np.asarray(void, dtype=np.int64)] = -1
    return f


def project(xt, beta, eta, flag=None, void_value=1e-4, dtype=float):
    rho = H(xt, beta, eta, dtype)
    if flag is not None:
        rho[flag > 0] = dtype(1.0)
        rho[flag < 0] = dtype(void_value)
    return rho


# ---- the volume-preserving threshold --------------------------------------------------------------------------------------
def g(eta, xt, v, beta, active, dtype=float):
    """sum_active v H(xt; beta, eta) - sum_active v xt"""
    xa, va = np.asarray(xt, dtype=dtype)[active], np.asarray(v, dtype=dtype)[active]
    return (va * H(xa, beta, eta, dtype)).sum() - (va * xa).sum()


def bisect_eta(xt, v, beta, flag=None, dtype=float):
    """53 steps on [0, 1]: mid = (lo + hi) / 2; g(mid) > 0: lo = mid, else hi = mid; eta = (lo + hi) / 2.  lo, hi and mid are
    float64 in either dtype (halving is exact), g is summed in ``dtype``."""
    n = np.size(xt)
    active = np.ones(n, bool) if flag is None else np.asarray(flag) == 0
    if not active.any():
        raise ValueError("the volume-preserving threshold needs an active cell")
    lo, hi = 0.0, 1.0
    for _ in range(BISECT_STEPS):
        mid = 0.5 * (lo + hi)
        if g(mid, xt, v, beta, active, dtype) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def fold_depth(n, n_cu=256):
    """Additions a term passes through in the device's sum of n terms: the thread's own stride loop, six shuffle levels, three
    waves, then the fold: its stride loop over the per-block partials, six levels, three waves."""
    nb = max(1, min(-(-n // 256), 4 * n_cu, 2048))
    return -(-n // (nb * 256)) + 9 + -(-nb // 256) + 9


# ---- Jacobian products ----------------------------------------------------------------------------------------------------
def _active(n, flag):
    return np.ones(n, bool) if flag is None else np.asarray(flag) == 0


def jac_reverse(xt, a, beta, eta, flag=None, v=None, volume=False, dtype=float):
    """J^T a at xt.  volume: eta is the root there, the rank-one term is added unless S_v == 0.  Returns (out, S_a, S_v)."""
    xt, a = np.asarray(xt, dtype=dtype), np.asarray(a, dtype=dtype)
    act = _active(xt.size, flag)
    hx = H_x(xt, beta, eta, dtype)
    out = np.where(act, a * hx, dtype(0.0))
    Sa = Sv = dtype(0.0)
    if volume:
        v = np.asarray(v, dtype=dtype)
        he = H_eta(xt, beta, eta, dtype)
        Sa, Sv = (a * he)[act].sum(), (v * he)[act].sum()
        if Sv != 0:
            out = out + np.where(act, (Sa / Sv) * v * (dtype(1.0) - hx), dtype(0.0))
    return out, Sa, Sv


def jac_forward(xt, d, beta, eta, flag=None, v=None, volume=False, dtype=float):
    """J d at xt.  Returns (out, T, S_v), T = sum_active v (1 - H_x) d."""
    xt, d = np.asarray(xt, dtype=dtype), np.asarray(d, dtype=dtype)
    act = _active(xt.size, flag)
    hx = H_x(xt, beta, eta, dtype)
    out = np.where(act, hx * d, dtype(0.0))
    T = Sv = dtype(0.0)
    if volume:
        v = np.asarray(v, dtype=dtype)
        he = H_eta(xt, beta, eta, dtype)
        T, Sv = (v * (dtype(1.0) - hx) * d)[act].sum(), (v * he)[act].sum()
        if Sv != 0:
            out = out + np.where(act, he * (T / Sv), dtype(0.0))
    return out, T, Sv


def volume_product_bounds(xt, a, beta, eta, flag, v, tangent):
    """Per-entry bound on the device's volume-mode product against ``jac_reverse`` / ``jac_forward`` in extended precision AT
    THE SAME eta, to first order: the entry bounds above carried through the two sums (depth ``fold_depth`` each), the
    quotient and the final expression.  Also returns (dS, |S_v|) for the caller to check that first order is enough."""
    n = np.size(xt)
    act = _active(n, flag)
    xt, a, v = (np.asarray(q, dtype=float) for q in (xt, a, v))
    hx, he = (np.asarray(f(xt, beta, eta, LD), dtype=float) for f in (H_x, H_eta))
    bx, be = bound_Hx(xt, beta, eta), bound_Heta(xt, beta, eta)
    dep = 0.5 * EPS * (fold_depth(n) + 1)
    Sv = float((v * he)[act].sum())
    dSv = float((v * be)[act].sum() + dep * np.abs(v * he)[act].sum())
    if tangent:
        S = float((v * (1.0 - hx) * a)[act].sum())
        dS = float((v * np.abs(a) * (bx + EPS))[act].sum() + dep * np.abs(v * (1.0 - hx) * a)[act].sum())
    else:
        S = float((a * he)[act].sum())
        dS = float((np.abs(a) * be)[act].sum() + dep * np.abs(a * he)[act].sum())
    if Sv == 0.0:
        return np.where(act, np.abs(a) * bx + EPS * np.abs(a * hx), 0.0), dSv, 0.0
    r = S / Sv
    dr = (dS + abs(r) * dSv) / abs(Sv) + 0.5 * EPS * abs(r)
    if tangent:
        err = np.abs(a) * bx + be * abs(r) + np.abs(he) * dr + 2.0 * EPS * (np.abs(hx * a) + np.abs(he * r))
    else:
        err = np.abs(a) * bx + dr * v * np.abs(1.0 - hx) + abs(r) * v * (bx + 0.5 * EPS) + 2.0 * EPS * (np.abs(a * hx) + np.abs(r * v * (1.0 - hx)))
    return np.where(act, 1.05 * err, 0.0), dSv, abs(Sv)


def g_error(xt, v, beta, eta, flag=None):
    """Bound on the error of the device's g at eta, and of sum v rho - sum v xt of its output: the two sums' (depth
    ``fold_depth``, products included) plus the entries' (``bound_H``), the latter twice: the bisection decides on entries
    that carry it, and the density written at the root carries it again."""
    n = np.size(xt)
    act = _active(n, flag)
    xa, va = np.asarray(xt, dtype=float)[act], np.asarray(v, dtype=float)[act]
    h = np.asarray(H(xa, beta, eta, LD), dtype=float)
    dep = 0.5 * EPS * (fold_depth(n) + 1)
    return float(dep * ((va * np.abs(h)).sum() + (va * np.abs(xa)).sum()) + 2.0 * bound_H(beta, eta) * va.sum())


# ---- grayness ----------------------------------------------------------------------------------------------------------------
def grayness(rho, v=None, dtype=float):
    """M_nd = 4 sum v rho (1 - rho) / sum v over all cells"""
    rho = np.asarray(rho, dtype=dtype)
    v = np.ones(rho.size, dtype=dtype) if v is None else np.asarray(v, dtype=dtype)
    return dtype(4.0) * (v * rho * (dtype(1.0) - rho)).sum() / v.sum()


# ---- continuation -------------------------------------------------------------------------------------------------------------
def stage_plan(betas, every, steps):
    """(beta of step k, steps that begin with a reset) for k = 1..steps when no stage ends early."""
    beta = [betas[min((k - 1) // every, len(betas) - 1)] for k in range(1, steps + 1)]
    resets = [1] + [s * every + 1 for s in range(1, len(betas)) if s * every + 1 <= steps]
    return beta, resets


def continuation_loop(mesh, facets, h_avg, betas, every, steps, eta=0.5, noise=0.0, vol_frac=0.4, x0=0.4):
    """The cantilever design loop of tests/test_gpu_mma.py with the projection between filter and state, restated on
    tests/mma_ref.py, tests/elasticity_ref.py: per step (J, f, x, Newton steps, beta, M_nd of the projected density), the
    values before the update.  A stage lasts ``every`` steps (tol = 0: none ends early); the history is reset at each
    stage's start.  noise: relative perturbation of the objective's gradient, entry by entry."""
    import elasticity_ref as eref
    import mma_ref
    X, conn = mesh.x, mesh.conn
    W = eref.filter_matrix(mesh.centroids(), 2.0 * h_avg)
    K0 = eref.element_matrices(X, conn)
    F = eref.traction_load(X, facets, (0.0, -0.25))
    fv = np.nonzero(np.isclose(X[:, 0], 0.0))[0]
    fixed = np.concatenate([2 * fv, 2 * fv + 1])
    vol = eref.cell_volumes(X, conn)
    n = mesh.n_cell
    rng = np.random.default_rng(1)
    opt = mma_ref.MMA(np.full(n, 1e-4), np.ones(n), 1)
    x, hist, J0 = np.full(n, x0), [], None
    plan, resets = stage_plan(betas, every, steps)
    for k in range(1, steps + 1):
        beta = plan[k - 1]
        if k in resets:
            opt.reset()
        xt = W @ x
        rho = project(xt, beta, eta)
        hx = H_x(xt, beta, eta)
        u = eref.solve_fixed(eref.stiffness(X, conn, rho, "SIMP", K0=K0), F, fixed)
        J = F @ u
        gJ = W.T @ (hx * -eref.compliance_gradient(X, conn, rho, u, u, "SIMP", K0=K0))
        f = vol @ rho / vol.sum() - vol_frac
        gc = W.T @ (hx * vol / vol.sum())
        J0 = J if J0 is None else J0
        if noise:
            gJ = gJ * (1.0 + noise * rng.standard_normal(n))
        xn = opt.update(x, gJ / J0, [f], gc[None, :])
        assert opt.last["rec"]["converged"] == 1
        hist.append((J, f, x.copy(), opt.last["rec"]["newton"], beta, float(grayness(rho, vol))))
        x = xn
    return hist
