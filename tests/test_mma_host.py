"""CPU tests of the MMA restatement (tests/mma_ref.py, the specification of csrc/mma.hip) against answers known without it
-- Svanberg's five-variable cantilever, SciPy's SLSQP (ftol 1e-10) on random convex problems, the KKT conditions of single subproblems --
and of what femo_amd.opt refuses before any device work."""
import types

import numpy as np
import pytest
import scipy.optimize

import mma_ref as R

COEF = np.array([61.0, 37.0, 19.0, 7.0, 1.0])


def svanberg_cantilever(x):
    """f0, df0, f, df of Svanberg (1987), section 'a five-variable cantilever beam'."""
    return 0.0624 * x.sum(), np.full(5, 0.0624), np.array([(COEF / x ** 3).sum() - 1.0]), (-3.0 * COEF / x ** 4)[None, :]


def test_svanberg_cantilever():
    x = np.full(5, 5.0)
    opt = R.MMA(np.ones(5), np.full(5, 10.0), 1)
    for _ in range(30):
        f0, df0, f, df = svanberg_cantilever(x)
        x = opt.update(x, df0, f, df)
        assert opt.last['rec']['converged'] == 1
    f0, _, f, _ = svanberg_cantilever(x)
    assert round(f0, 4) == 1.3400
    assert np.abs(x - np.array([6.016, 5.309, 4.494, 3.502, 2.153])).max() <= 2e-3
    assert f[0] <= 1e-6


def random_convex(m, seed, n=40):
    """min sum (x - t)^2 s.t. A x <= a (m rows), 0 <= x <= 1.  The targets lie 0.3 to 1 outside the box, so that without
    the rows the minimiser is a corner of it; the rows cut that corner off by 1 to 3, which moves some variables inside.
    (|x - t| >= 0.3 everywhere also keeps MMA's approximation of the objective more convex than the objective itself: on
    targets inside the box plain MMA ends in a cycle of amplitude 1e-3, which only GCMMA's inner loop removes.)"""
    rng = np.random.default_rng(seed)
    t = 0.5 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.8, 1.5, n)
    A = rng.standard_normal((m, n))
    a = A @ np.clip(t, 0.0, 1.0) - rng.uniform(1.0, 3.0, m)
    return t, A, a


def solve_with_restatement(t, A, a, steps=80):
    m, n = A.shape
    x = np.full(n, 0.5)
    opt = R.MMA(np.zeros(n), np.ones(n), m)
    f0_start = ((x - t) ** 2).sum()
    for _ in range(steps):
        x = opt.update(x, 2.0 * (x - t) / f0_start, A @ x - a, A)
        assert opt.last['rec']['converged'] == 1
    return x


# Measured with this file (the print below): after 80 steps the restatement and SLSQP differ by at most 1.09e-3 in
# max|dx| over the nine problems (m = 2, seed 1; the others 2.3e-5 to 2.9e-4).  The largest differences sit in variables
# whose bound is only weakly active: the interior-point solver ends at barrier 1e-7 with xi (x - alpha) = 1e-7, which
# leaves x - alpha = 1e-7 / xi, 1e-3 for a reduced gradient of 1e-4.  Ten times the measured agreement:
SLSQP_BOUND = 1.09e-2


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_convex_against_slsqp(m, seed):
    t, A, a = random_convex(m, seed)
    x = solve_with_restatement(t, A, a)
    ref = scipy.optimize.minimize(lambda v: ((v - t) ** 2).sum(), np.full(t.size, 0.5), jac=lambda v: 2.0 * (v - t),
                                  bounds=[(0.0, 1.0)] * t.size, method='SLSQP',
                                  constraints=[dict(type='ineq', fun=lambda v: a - A @ v, jac=lambda v: -A)],
                                  options=dict(ftol=1e-10, maxiter=500))
    assert ref.success
    diff = np.abs(x - ref.x).max()
    print(f"m={m} seed={seed}: max|x_mma - x_slsqp| = {diff:.3e}, active rows {int(np.sum(A @ ref.x - a > -1e-9))}")
    assert diff <= SLSQP_BOUND


random_subproblem, sub_args = R.random_subproblem, R.sub_args


@pytest.mark.parametrize("n,m", [(1, 1), (7, 3), (64, 1), (200, 8), (1000, 2)])
@pytest.mark.parametrize("sub_tol", [1e-7, 1e-10])
def test_subproblem_kkt(n, m, sub_tol):
    """The last stage ends with residual <= 0.9 eps at barrier eps <= sub_tol, and the complementarity rows differ from
    their barrier-0 form by eps: the KKT residual at barrier 0 is at most 1.9 eps <= 2 sub_tol."""
    s = random_subproblem(n, m, seed=n + m)
    x, rec = R.subsolve(*sub_args(s), sub_tol=sub_tol)
    assert rec['converged'] == 1 and rec['stages'] == R.n_stages(sub_tol) == int(round(-np.log10(sub_tol))) + 1
    assert R.kkt_residual(*sub_args(s), x, rec) <= 2.0 * sub_tol
    assert np.all(x > s['alfa']) and np.all(x < s['beta'])


def test_subproblem_closed_form_m0():
    s = random_subproblem(50, 0, seed=3)
    x, rec = R.subsolve(*sub_args(s))
    assert rec['newton'] == 0 and rec['stages'] == 0
    inside = (x > s['alfa']) & (x < s['beta'])
    assert inside.any() and (~inside).any() or inside.all()
    d = s['p'][0] / (s['U'] - x) ** 2 - s['q'][0] / (x - s['L']) ** 2       # stationary inside, pushing outwards on a bound
    assert np.abs(d[inside]).max() <= 1e-12 * (s['p'][0] / (s['U'] - x) ** 2)[inside].max()
    assert np.all(d[x == s['alfa']] >= 0.0) and np.all(d[x == s['beta']] <= 0.0)


def test_stage_count_is_an_integer_count():
    assert 0.1 ** 7 > 1e-7                       # why the stages are not counted by comparing floats
    assert [R.n_stages(t) for t in (1.0, 1e-1, 1e-7, 1e-10, 3e-8)] == [1, 2, 8, 11, 9]
    assert R.barrier(7) == 1e-7 and R.barrier(0) == 1.0


# ---- what femo_amd.opt refuses (no device) ------------------------------------------------------------------------------
def _sim(n=6, lower=1e-4, upper=1.0, constraints=(('avg_density', dict(upper=0.4)),), objective=True, extra_dv=False):
    from femo_amd.csdl_opt._csdl_compat import Model
    model = Model()
    model.create_input('density_unfiltered', shape=n, val=0.4)
    model.add_design_variable('density_unfiltered', lower=lower, upper=upper)
    if extra_dv:
        model.create_input('thickness', shape=2, val=1.0)
        model.add_design_variable('thickness', lower=0.0, upper=1.0)
    if objective:
        model.add_objective('compliance')
    for name, kw in constraints:
        model.add_constraint(name, **kw)
    return types.SimpleNamespace(model=model, device=False)


def test_problem_reads_the_model():
    from femo_amd.opt import CSDLProblem
    prob = CSDLProblem(problem_name='t', simulator=_sim(lower=np.linspace(0.0, 0.1, 6), constraints=(
        ('avg_density', dict(upper=0.4, scaler=2.0)), ('stress', dict(lower=-1.0, upper=3.0)))))
    assert prob.n == 6 and prob.dv_name == 'density_unfiltered' and prob.objective == 'compliance'
    assert np.array_equal(prob.xmin, np.linspace(0.0, 0.1, 6)) and np.array_equal(prob.xmax, np.ones(6))
    assert [tuple(r) for r in prob.rows] == [('avg_density', 1.0, 0.4, 2.0), ('stress', 1.0, 3.0, 1.0), ('stress', -1.0, -1.0, 1.0)]


@pytest.mark.parametrize("kw,word", [
    (dict(extra_dv=True), "exactly one"),
    (dict(lower=None), "box"),
    (dict(upper=np.inf), "box"),
    (dict(lower=np.array([0.0, 0.0, np.nan, 0.0, 0.0, 0.0])), "box"),
    (dict(lower=1.0, upper=1.0), "passive"),
    (dict(upper=np.array([1.0, 1.0, 1e-4, 1.0, 1.0, 1.0])), "passive"),
    (dict(constraints=(('avg_density', dict(equals=0.4)),)), "equality"),
    (dict(constraints=(('avg_density', dict()),)), "neither"),
    (dict(constraints=(('avg_density', dict(upper=np.inf)),)), "finite"),
    (dict(objective=False), "objective"),
])
def test_problem_refusals(kw, word):
    from femo_amd.opt import CSDLProblem
    with pytest.raises(ValueError, match=word):
        CSDLProblem(problem_name='t', simulator=_sim(**kw))


def test_optimizer_refusals():
    from femo_amd.opt import MMA, CSDLProblem
    prob = CSDLProblem(problem_name='t', simulator=_sim())
    for kw in (dict(move=0.0), dict(move=-0.5), dict(move=np.nan), dict(sub_tol=0.0), dict(sub_tol=2.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            MMA(prob, **kw)
    nine = tuple((f'g{i}', dict(upper=1.0)) for i in range(9))
    with pytest.raises(ValueError, match="0 to 8"):
        MMA(CSDLProblem(problem_name='t', simulator=_sim(constraints=nine)))
    eight = tuple((f'g{i}', dict(lower=0.0, upper=1.0)) for i in range(4))
    assert MMA(CSDLProblem(problem_name='t', simulator=_sim(constraints=eight))).prob.m == 8
