"""Host tests (no GPU) of the Heaviside projection's restatement (tests/projection_ref.py), of the Python layer's parameter
validation (femo_amd.csdl_opt.filter_model.check_projection_parameters) and of BetaContinuation's stage arithmetic."""
import numpy as np
import pytest

import projection_ref as P

LD = np.longdouble
BETAS = (1.0, 8.0, 64.0, 512.0)


def _field(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.02, 0.92, n), rng.uniform(0.5, 1.5, n), rng


# ---- the three functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("eta", [0.0, 0.3, 0.5, 1.0])
def test_end_points_and_threshold(beta, eta):
    """H(0) = 0 and H(1) = 1 exactly (tanh is odd; N = D bit for bit at x = 1), H(eta) = tanh(beta eta) / D, H is monotone,
    and nothing is NaN at beta = 512."""
    x = np.array([0.0, 1.0, eta])
    h = P.H(x, beta, eta)
    assert h[0] == 0.0 and h[1] == 1.0
    assert h[2] == np.tanh(beta * eta) / (np.tanh(beta * eta) + np.tanh(beta * (1.0 - eta)))
    grid = np.linspace(0.0, 1.0, 1001)
    for f in (P.H, P.H_x, P.H_eta):
        assert np.all(np.isfinite(f(grid, beta, eta)))
    assert np.all(np.diff(P.H(grid, beta, eta)) >= 0.0)
    assert np.all(P.H_x(grid, beta, eta) >= 0.0)
    assert P.H_eta(np.array([0.0, 1.0]), beta, eta).tolist() == [0.0, 0.0]        # saturated cells: exactly flat


def test_beta_zero_is_the_identity_and_its_limit():
    x, _, _ = _field(257, 3)
    assert np.array_equal(P.H(x, 0.0, 0.3), x)
    assert np.all(P.H_x(x, 0.0, 0.3) == 1.0) and np.all(P.H_eta(x, 0.0, 0.3) == 0.0)
    prev = np.inf
    for beta in (1e-1, 1e-2, 1e-3):
        # H - x = O(beta^2): the cubic term of tanh, coefficients of order one on [0, 1]
        err = np.abs(P.H(x, beta, 0.3, LD) - x).max()
        assert err <= beta ** 2 and err < prev
        assert np.abs(P.H_x(x, beta, 0.3, LD) - 1.0).max() <= beta ** 2
        prev = err


@pytest.mark.parametrize("beta", [1.0, 8.0, 64.0])
@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
def test_partials_against_central_differences(beta, eta):
    """H_x and H_eta against central differences of H in extended precision, step h = 1e-5 / beta: the truncation is
    h^2 beta^2 / 6 of the derivative's scale beta, the rounding 2^-63 / h of it."""
    x, _, _ = _field(65, 5)
    h = LD(1e-5) / LD(beta)
    fx = (P.H(x.astype(LD) + h, beta, eta, LD) - P.H(x.astype(LD) - h, beta, eta, LD)) / (2 * h)
    assert np.abs(fx - P.H_x(x, beta, eta, LD)).max() <= 1e-9 * beta
    e = min(max(eta, 1e-3), 1.0 - 1e-3)                                         # the difference needs room on both sides
    fe = (P.H(x, beta, LD(e) + h, LD) - P.H(x, beta, LD(e) - h, LD)) / (2 * h)
    assert np.abs(fe - P.H_eta(x, beta, LD(e), LD)).max() <= 1e-9 * beta


# ---- the volume-preserving threshold -------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.5, 1.0, 8.0, 64.0, 256.0])
@pytest.mark.parametrize("n", [1, 2, 65, 1025])
def test_bracket_and_root(beta, n):
    """g(0) >= 0 >= g(1), g does not increase, and the 53 steps leave |g(eta)| <= |S_v| 2^-53 plus the sum's rounding."""
    x, v, _ = _field(n, 7 * n)
    act = np.ones(n, bool)
    tiny = 1e-17 * v.sum()                                                     # longdouble sums of n terms of size <= v
    assert P.g(0.0, x, v, beta, act, LD) >= -tiny and P.g(1.0, x, v, beta, act, LD) <= tiny
    gs = [P.g(e, x, v, beta, act, LD) for e in np.linspace(0.0, 1.0, 41)]
    assert all(b <= a + tiny for a, b in zip(gs, gs[1:]))
    eta = P.bisect_eta(x, v, beta, dtype=LD)
    Sv = abs((v * P.H_eta(x, beta, eta, LD)).sum())
    assert abs(P.g(eta, x, v, beta, act, LD)) <= 2.0 ** -53 * Sv * 1.01 + tiny
    assert P.bisect_eta(x, v, beta, dtype=LD) == eta


def test_volume_mode_refuses_no_active_cell():
    with pytest.raises(ValueError):
        P.bisect_eta(np.full(3, 0.5), np.ones(3), 4.0, flag=np.array([1, -1, 1]))


@pytest.mark.parametrize("beta", [1.0, 8.0, 64.0])
@pytest.mark.parametrize("n", [1, 2, 65, 1025])
@pytest.mark.parametrize("passive", [False, True])
def test_volume_products_against_central_differences(beta, n, passive):
    """J d of the volume mode against (P(x + h d) - P(x - h d)) / 2h with eta re-solved at both points, and J^T a through
    <J^T a, d> = <a, J d>.  h = 1e-6: truncation h^2 beta^2 / 6 relative, the threshold's resolution 2^-54 beta / h; asserted
    at 1e-6 of the product's largest entry.  n = 1 without passive cells: J = 1, the projection must return the volume."""
    x, v, rng = _field(n, 11 * n + int(beta))
    flag = None
    if passive and n >= 65:
        flag = P.flags(n, solid=[3, 63, 64], void=[0, n - 1])
    d, a = rng.standard_normal(n), rng.standard_normal(n)
    eta = P.bisect_eta(x, v, beta, flag, LD)
    Jd, _, Sv = P.jac_forward(x, d, beta, eta, flag, v, True, LD)
    assert Sv != 0
    h = LD(1e-6)

    def rho(xp):
        return P.project(xp, beta, P.bisect_eta(xp, v, beta, flag, LD), flag, dtype=LD)
    fd = (rho(x.astype(LD) + h * d) - rho(x.astype(LD) - h * d)) / (2 * h)
    scale = max(float(np.abs(Jd).max()), 1e-300)
    assert np.abs(fd - Jd).max() <= 1e-6 * scale
    if flag is not None:
        assert np.all(Jd[flag != 0] == 0)
    JTa, _, _ = P.jac_reverse(x, a, beta, eta, flag, v, True, LD)
    lhs, rhs = (JTa * d).sum(), (a * Jd).sum()
    assert abs(lhs - rhs) <= 1e-15 * (np.abs(JTa * d).sum() + np.abs(a * Jd).sum())
    if n == 1:
        assert abs(Jd[0] - d[0]) <= 1e-12 * abs(d[0])


def test_flat_drops_the_rank_one_term():
    x = np.array([0.0, 1.0, 1.0, 0.0])
    v = np.ones(4)
    eta = P.bisect_eta(x, v, 512.0)
    out, Sa, Sv = P.jac_reverse(x, np.ones(4), 512.0, eta, None, v, True)
    assert Sv == 0.0 and np.all(np.isfinite(out))
    out, T, Sv = P.jac_forward(x, np.ones(4), 512.0, eta, None, v, True)
    assert Sv == 0.0 and np.all(np.isfinite(out))


def test_grayness():
    assert P.grayness(np.array([0.0, 1.0, 1.0])) == 0.0
    assert P.grayness(np.full(5, 0.5)) == 1.0
    assert P.grayness(np.array([0.5, 1.0]), np.array([1.0, 3.0])) == 0.25


# ---- the Python layer's validation ----------------------------------------------------------------------------------------
def test_parameter_refusals():
    from femo_amd.csdl_opt.filter_model import check_projection_parameters as chk
    ok = chk(10, 4.0, 0.5, np.ones(10), [1, 2], [3], 1e-4)
    assert ok[0] == 4.0 and ok[1] == 0.5 and ok[2] == 0 and ok[4].tolist() == [1, 2] and ok[5].tolist() == [3]
    assert chk(10, 0.0, "volume")[2] == 1
    bad = [dict(projection_beta=-1.0), dict(projection_beta=np.nan), dict(projection_beta=np.inf),
           dict(eta=-0.1), dict(eta=1.1), dict(eta=np.nan), dict(eta="mass"),
           dict(solid=[10]), dict(void=[-1]), dict(solid=[1, 2], void=[2, 3]), dict(solid=[1.5]),
           dict(void_value=0.0), dict(void_value=1.5), dict(void_value=np.nan),
           dict(volumes=np.ones(9)), dict(volumes=np.where(np.arange(10) == 4, 0.0, 1.0)),
           dict(volumes=np.where(np.arange(10) == 4, -1.0, 1.0)), dict(volumes=np.where(np.arange(10) == 4, np.inf, 1.0)),
           dict(volumes=np.where(np.arange(10) == 4, np.nan, 1.0)),
           dict(eta="volume", solid=np.arange(6), void=np.arange(6, 10))]
    for kw in bad:
        with pytest.raises(ValueError):
            chk(10, **kw)
    with pytest.raises(ValueError):
        chk(0)
    chk(10, 4.0, 0.5, solid=np.arange(6), void=np.arange(6, 10))           # all passive is fine with a fixed threshold


# ---- the continuation's stage arithmetic ------------------------------------------------------------------------------------
class _Op:
    def __init__(self):
        self.set = []

    @property
    def beta(self):
        return self.set[-1]

    @beta.setter
    def beta(self, value):
        self.set.append(value)


def _drive(cont, dx, tol, max_iter):
    """What MMA.solve does with a continuation, on a stub optimiser: (beta per step, steps that began with a reset)."""
    cont.start()
    betas, resets = [], [1]
    for k in range(1, max_iter + 1):
        betas.append(cont.op.beta)
        what = cont.after_step(dx[k - 1], tol)
        if what == 'stop':
            break
        if what == 'advance':
            resets.append(k + 1)
    return betas, resets


def test_stage_boundaries_and_resets():
    from femo_amd.opt import BetaContinuation
    op = _Op()
    betas, resets = _drive(BetaContinuation(op, (1, 2, 4, 8), 8), [1.0] * 32, 0.0, 32)
    assert betas == [1.0] * 8 + [2.0] * 8 + [4.0] * 8 + [8.0] * 8 and resets == [1, 9, 17, 25]
    assert (betas, resets) == P.stage_plan([1.0, 2.0, 4.0, 8.0], 8, 32)
    assert op.set == [1.0, 2.0, 4.0, 8.0]
    # max_iter caps the total; the last stage goes on past `every`
    betas, resets = _drive(BetaContinuation(_Op(), (1, 2), 3), [1.0] * 10, 0.0, 10)
    assert betas == [1.0] * 3 + [2.0] * 7 and resets == [1, 4]
    assert (betas, resets) == P.stage_plan([1.0, 2.0], 3, 10)


def test_tol_ends_a_stage_early_and_stops_only_in_the_last():
    from femo_amd.opt import BetaContinuation
    dx = [1.0, 1e-4, 1.0, 1.0, 1e-4, 1e-4, 1.0, 1e-4, 1.0]
    betas, resets = _drive(BetaContinuation(_Op(), (1, 2, 4), 3), dx, 1e-3, 9)
    #        step:  1    2 (small: stage ends)  3  4  5 (small)  6 (small, last stage: stop)
    assert betas == [1.0, 1.0, 2.0, 2.0, 2.0, 4.0] and resets == [1, 3, 6]
    # tol = 0 never ends anything early, not even on a zero step
    betas, resets = _drive(BetaContinuation(_Op(), (1, 2), 2), [0.0] * 6, 0.0, 6)
    assert betas == [1.0, 1.0, 2.0, 2.0, 2.0, 2.0] and resets == [1, 3]


def test_continuation_refusals():
    from femo_amd.opt import BetaContinuation
    for betas, every in (((), 4), ((1, -2), 4), ((1, np.nan), 4), ((1, 2), 0)):
        with pytest.raises(ValueError):
            BetaContinuation(_Op(), betas, every)


# ---- the restated design loop ------------------------------------------------------------------------------------------------
def test_continuation_lowers_the_grayness():
    """The restatement alone, 24 x 12 cantilever, 32 steps from x = 0.4 under avg_density <= 0.40: betas (1, 2, 4, 8), 8 steps
    each, ends at M_nd = 0.4498 and compliance 1300.05; beta = 0 (the filter alone) at M_nd = 0.7007 and 1929.88.  Asserted:
    the order, and that the constraint holds from step 2 on in both."""
    from femo_amd.fea.fea_hip import createRectangleMesh, locate_entities_boundary, meshSize
    LX, LY, nelx, nely = 160.0, 80.0, 24, 12
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), nelx, nely)
    facets = locate_entities_boundary(mesh, 1, lambda x: np.logical_and(abs(x[1] - LY / 2) < LY / nely + 3e-6, abs(x[0] - LX) < 3e-6))
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    proj = P.continuation_loop(mesh, facets, h_avg, (1.0, 2.0, 4.0, 8.0), 8, 32)
    plain = P.continuation_loop(mesh, facets, h_avg, (0.0,), 8, 32)
    print(f"M_nd after 32 steps: projected {proj[-1][5]:.4f} (J {proj[-1][0]:.2f}), filter alone {plain[-1][5]:.4f} (J {plain[-1][0]:.2f})")
    assert proj[-1][5] < plain[-1][5]
    assert [r[4] for r in proj] == [1.0] * 8 + [2.0] * 8 + [4.0] * 8 + [8.0] * 8
    # a new stage starts from a design that met the constraint under the previous beta; it may overshoot by what the sharper
    # projection adds until the next update takes it back
    assert all(r[1] <= 1e-9 for r in plain[1:])
    assert all(r[1] <= 1e-9 for k, r in enumerate(proj, start=1) if k > 1 and k not in (9, 17, 25))
