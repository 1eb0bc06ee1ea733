"""NumPy restatement of the MMA update (Svanberg 1987; Svanberg 2007, "MMA and GCMMA -- two methods for nonlinear
optimization"), the specification the device code (femo_amd/csrc/mma.hip) is tested against.  Written step by step:
asymptotes, move limits, the approximations p, q, b, the primal-dual interior-point solver of the subproblem, and the KKT
residual of a subproblem at barrier 0.

Differences from Svanberg's note, the same as in the device code: his variable z and the constants a_i are dropped (a_i = 0
makes z = 0 at the optimum), so the unknowns are (x, y, lam, xsi, eta, mu, s) and the Newton system is m x m; and
rho = RAA0 / range carries no floor, because xmax > xmin everywhere is a precondition.  Out of scope: GCMMA's inner loop,
equality constraints, passive cells."""
import math

import numpy as np

ASYINIT, ASYINCR, ASYDECR = 0.5, 1.2, 0.7
ASYMIN, ASYMAX = 0.01, 10.0
ALBEFA = 0.1
RAA0 = 1e-5
MAX_NEWTON, MAX_HALVINGS = 200, 50


def asymptotes(k, x, xmin, xmax, x1, x2, low, upp):
    """L, U of design step k (1-based).  x1, x2: the two previous iterates; low, upp: the previous asymptotes."""
    rng = xmax - xmin
    if k <= 2:
        return x - ASYINIT * rng, x + ASYINIT * rng
    z = (x - x1) * (x1 - x2)
    gam = np.ones_like(x)
    gam[z > 0] = ASYINCR
    gam[z < 0] = ASYDECR
    L = x - gam * (x1 - low)
    U = x + gam * (upp - x1)
    L = np.minimum(np.maximum(L, x - ASYMAX * rng), x - ASYMIN * rng)
    U = np.maximum(np.minimum(U, x + ASYMAX * rng), x + ASYMIN * rng)
    return L, U


def move_limits(x, xmin, xmax, L, U, move):
    rng = xmax - xmin
    alfa = np.maximum(np.maximum(L + ALBEFA * (x - L), x - move * rng), xmin)
    beta = np.minimum(np.minimum(U - ALBEFA * (U - x), x + move * rng), xmax)
    return alfa, beta


def approximation(x, xmin, xmax, L, U, g):
    """p, q of one function with gradient g (n,) or of several (rows of g)."""
    rho = RAA0 / (xmax - xmin)
    gp, gm = np.maximum(g, 0.0), np.maximum(-g, 0.0)
    ux, xl = U - x, x - L
    p = (ux * ux) * (1.001 * gp + 0.001 * gm + rho)
    q = (xl * xl) * (0.001 * gp + 1.001 * gm + rho)
    return p, q


def constants_b(x, L, U, P, Q, f):
    """b_i = sum_j (p_ij / (U - x) + q_ij / (x - L)) - f_i, and the sums themselves (the scale of b's rounding)."""
    s = P @ (1.0 / (U - x)) + Q @ (1.0 / (x - L))
    return s - f, s


def n_stages(sub_tol):
    """Barrier values 10^0 ... 10^-K, K = ceil(-log10(sub_tol)): K + 1 stages, counted by an integer."""
    return int(math.ceil(-math.log10(sub_tol))) + 1


def barrier(stage):
    return 1.0 / float(10 ** stage)


def closed_form(L, U, alfa, beta, p0, q0):
    """m = 0: the minimiser of sum p0/(U - x) + q0/(x - L) over the box."""
    sp, sq = np.sqrt(p0), np.sqrt(q0)
    return np.minimum(np.maximum((sp * L + sq * U) / (sp + sq), alfa), beta)


def residual(eps, L, U, alfa, beta, p0, q0, P, Q, b, c, d, x, y, lam, xsi, eta, mu, s):
    """All rows of the perturbed KKT system at barrier eps, and g(x)."""
    ux, xl = U - x, x - L
    plam, qlam = p0 + lam @ P, q0 + lam @ Q
    gvec = P @ (1.0 / ux) + Q @ (1.0 / xl)
    rex = plam / (ux * ux) - qlam / (xl * xl) - xsi + eta
    rey = c + d * y - mu - lam
    relam = gvec - y + s - b
    rexsi = xsi * (x - alfa) - eps
    reeta = eta * (beta - x) - eps
    remu = mu * y - eps
    res = lam * s - eps
    return np.concatenate([rex, rey, relam, rexsi, reeta, remu, res])


def subsolve(L, U, alfa, beta, p0, q0, P, Q, b, c, d, sub_tol=1e-7):
    """Primal-dual interior-point Newton iteration on the subproblem.  P, Q: (m, n).  Returns x and a record with y, lam,
    xsi, eta, mu, s, stages, newton (Newton steps in all), halvings and converged (0 if a cap was hit)."""
    m, n = P.shape
    if m == 0:
        x = closed_form(L, U, alfa, beta, p0, q0)
        return x, dict(y=np.zeros(0), lam=np.zeros(0), xsi=None, eta=None, mu=np.zeros(0), s=np.zeros(0), stages=0, newton=0,
                       halvings=0, converged=1)
    x = 0.5 * (alfa + beta)
    y, lam, s = np.ones(m), np.ones(m), np.ones(m)
    xsi = np.maximum(1.0 / (x - alfa), 1.0)
    eta = np.maximum(1.0 / (beta - x), 1.0)
    mu = np.maximum(1.0, 0.5 * c)
    args = (L, U, alfa, beta, p0, q0, P, Q, b, c, d)
    newton = halvings = 0
    converged = 1
    stages = n_stages(sub_tol)
    for stage in range(stages):
        eps = barrier(stage)
        r = residual(eps, *args, x, y, lam, xsi, eta, mu, s)
        resmax, resi = np.abs(r).max(), np.linalg.norm(r)
        it = 0
        while resmax > 0.9 * eps and it < MAX_NEWTON:
            it += 1
            newton += 1
            ux, xl = U - x, x - L
            ux2, xl2 = ux * ux, xl * xl
            plam, qlam = p0 + lam @ P, q0 + lam @ Q
            gvec = P @ (1.0 / ux) + Q @ (1.0 / xl)
            GG = P / ux2 - Q / xl2
            delx = plam / ux2 - qlam / xl2 - eps / (x - alfa) + eps / (beta - x)
            dely = c + d * y - lam - eps / y
            dellam = gvec - y - b + eps / lam
            diagx = 2.0 * (plam / (ux2 * ux) + qlam / (xl2 * xl)) + xsi / (x - alfa) + eta / (beta - x)
            diagy = d + mu / y
            blam = dellam + dely / diagy - GG @ (delx / diagx)
            Alam = np.diag(s / lam + 1.0 / diagy) + (GG / diagx) @ GG.T
            dlam = np.linalg.solve(Alam, blam)
            dx = -delx / diagx - (dlam @ GG) / diagx
            dy = -dely / diagy + dlam / diagy
            dxsi = -xsi + eps / (x - alfa) - xsi * dx / (x - alfa)
            deta = -eta + eps / (beta - x) + eta * dx / (beta - x)
            dmu = -mu + eps / y - mu * dy / y
            ds = -s + eps / lam - s * dlam / lam
            pos = np.concatenate([y, lam, xsi, eta, mu, s])
            dpos = np.concatenate([dy, dlam, dxsi, deta, dmu, ds])
            stmax = max((-1.01 * dpos / pos).max(), (-1.01 * dx / (x - alfa)).max(), (1.01 * dx / (beta - x)).max(), 1.0)
            steg = 1.0 / stmax
            old = (x, y, lam, xsi, eta, mu, s)
            step = (dx, dy, dlam, dxsi, deta, dmu, ds)
            k = 0
            while True:
                k += 1
                x, y, lam, xsi, eta, mu, s = (o + steg * dv for o, dv in zip(old, step))
                r = residual(eps, *args, x, y, lam, xsi, eta, mu, s)
                resinew = np.linalg.norm(r)
                steg *= 0.5
                if not (resinew > resi) or k >= MAX_HALVINGS:
                    break
            halvings += k - 1
            if resinew > resi:
                converged = 0                       # 50 halvings did not bring the residual down
            resi, resmax = resinew, np.abs(r).max()
        if resmax > 0.9 * eps:
            converged = 0                           # 200 steps did not finish the stage
    return x, dict(y=y, lam=lam, xsi=xsi, eta=eta, mu=mu, s=s, stages=stages, newton=newton, halvings=halvings,
                   converged=converged)


def kkt_residual(L, U, alfa, beta, p0, q0, P, Q, b, c, d, x, rec):
    """Max-norm of the subproblem's KKT rows at barrier 0 for a point returned by subsolve (m >= 1)."""
    r = residual(0.0, L, U, alfa, beta, p0, q0, P, Q, b, c, d, x, rec['y'], rec['lam'], rec['xsi'], rec['eta'], rec['mu'],
                 rec['s'])
    return float(np.abs(r).max())


def random_subproblem(n, m, seed):
    """A subproblem with random p, q > 0 as a design step would hand it over: asymptotes around x, move limits inside
    them, b such that the current point misses some rows and satisfies others."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.1, 0.9, n)
    L, U = x - rng.uniform(0.2, 0.6, n), x + rng.uniform(0.2, 0.6, n)
    alfa, beta = np.maximum(L + 0.1 * (x - L), 0.0), np.minimum(U - 0.1 * (U - x), 1.0)
    p, q = rng.uniform(1e-3, 1.0, (m + 1, n)) / n, rng.uniform(1e-3, 1.0, (m + 1, n)) / n
    p[:, rng.random(n) < 0.2] *= 1e-3                                 # columns dominated by q, and the other way round
    q[:, rng.random(n) < 0.2] *= 1e-3
    g = p[1:] @ (1.0 / (U - x)) + q[1:] @ (1.0 / (x - L))
    b = g * rng.uniform(0.9, 1.1, m)
    return dict(L=L, U=U, alfa=alfa, beta=beta, p=p, q=q, b=b, c=np.full(m, 1000.0), d=np.ones(m))


def sub_args(s):
    return (s['L'], s['U'], s['alfa'], s['beta'], s['p'][0], s['q'][0], s['p'][1:], s['q'][1:], s['b'], s['c'], s['d'])


class MMA:
    """The design loop's state: asymptotes and the two previous iterates.  update() returns x^{k+1}."""

    def __init__(self, xmin, xmax, m, move=0.5, sub_tol=1e-7, c=1000.0, d=1.0):
        self.xmin, self.xmax = np.asarray(xmin, float), np.asarray(xmax, float)
        self.m, self.move, self.sub_tol = m, move, sub_tol
        self.c, self.d = np.full(m, float(c)), np.full(m, float(d))
        self.reset()

    def reset(self):
        self.k = 0
        self.x1 = self.x2 = self.low = self.upp = None
        self.last = None

    def update(self, x, df0, f, df):
        x = np.asarray(x, float)
        df = np.asarray(df, float).reshape(self.m, x.size)
        f = np.asarray(f, float).reshape(self.m)
        self.k += 1
        L, U = asymptotes(self.k, x, self.xmin, self.xmax, self.x1, self.x2, self.low, self.upp)
        alfa, beta = move_limits(x, self.xmin, self.xmax, L, U, self.move)
        p0, q0 = approximation(x, self.xmin, self.xmax, L, U, np.asarray(df0, float))
        P, Q = approximation(x, self.xmin, self.xmax, L, U, df)
        b, bsum = constants_b(x, L, U, P, Q, f)
        xn, rec = subsolve(L, U, alfa, beta, p0, q0, P, Q, b, self.c, self.d, self.sub_tol)
        self.last = dict(L=L, U=U, alfa=alfa, beta=beta, p=np.vstack([p0[None, :], P]), q=np.vstack([q0[None, :], Q]), b=b,
                         bsum=bsum, rec=rec)
        self.x2, self.x1, self.low, self.upp = self.x1, x.copy(), L, U
        return xn
