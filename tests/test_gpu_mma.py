"""GPU tests of the device-resident MMA update (csrc/mma.hip, femo_amd.opt) against its NumPy restatement
(tests/mma_ref.py): the element-wise stage entry by entry, single subproblems from given arrays, Svanberg's five-variable
cantilever, the 24 x 12 cantilever design loop through CSDLProblem + MMA in device and host mode, the 8 x 4 loop with a
volume and a stress constraint, and a restart."""
import numpy as np
import pytest

import elasticity_ref as eref
import mma_ref as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SIZES = [1, 63, 64, 65, 1000, 100003]
ROWS = [0, 1, 3, 8]


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _vec(ctx, a):
    from femo_amd.engine import Vec
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return Vec(ctx, a.size).set(a)


# ---- element-wise stage -----------------------------------------------------------------------------------------------------
def _design_sequence(n, m, steps, seed):
    """Bounds, iterates and gradients that reach every branch of the element-wise stage.  Variable j follows pattern
    j % 5: 0 never moves (z = 0 exactly), 1 climbs steadily (z > 0: the asymptotes widen by 1.2 a step until both sit on
    the 10 range clamps), 2 alternates (z < 0: they narrow by 0.7 a step down to the 0.01 range clamps), 3 sits on xmin,
    4 on xmax.  Gradients have both signs and exact zeros."""
    rng = np.random.default_rng(seed)
    xmin = rng.uniform(-1.0, 0.0, n)
    xmax = xmin + rng.uniform(0.5, 2.0, n)
    span = xmax - xmin
    pat = np.arange(n) % 5
    base = xmin + rng.uniform(0.3, 0.6, n) * span
    xs, grads = [], []
    for k in range(steps):
        x = base.copy()
        x[pat == 1] += (1e-3 * k * span)[pat == 1]
        x[pat == 2] += (1e-3 * (k % 2) * span)[pat == 2]
        x[pat == 3] = xmin[pat == 3]
        x[pat == 4] = xmax[pat == 4]
        g = rng.standard_normal((m + 1, n)) * rng.choice([1e-3, 1.0, 1e3], (m + 1, 1))
        g[:, rng.random(n) < 0.15] = 0.0
        xs.append(x)
        grads.append(g)
    return xmin, xmax, xs, grads, [rng.standard_normal(m) for _ in range(steps)]


def _run_elementwise(ctx, n, m, steps, seed, keep):
    """The device's arrays after the steps listed in `keep` (1-based)."""
    from femo_amd.opt import DeviceMMA
    xmin, xmax, xs, grads, fs = _design_sequence(n, m, steps, seed)
    opt = DeviceMMA(ctx, _vec(ctx, xmin), _vec(ctx, xmax), m)
    out = {}
    for k in range(steps):
        x, df0, df = _vec(ctx, xs[k]), _vec(ctx, grads[k][0]), (_vec(ctx, grads[k][1:]) if m else None)
        info = opt.update(x, 1.0, df0, fs[k], df)
        assert info["step"] == k + 1
        if k + 1 in keep:
            out[k + 1] = dict(L=opt.get("L"), U=opt.get("U"), alfa=opt.get("alfa"), beta=opt.get("beta"),
                              p=np.array([opt.get("p", i) for i in range(m + 1)]), q=np.array([opt.get("q", i) for i in range(m + 1)]),
                              b=opt.get("b"), bsum=opt.get("bsum"), x=np.array(x.get()))
    return out


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", SIZES)
def test_elementwise_stage(gpu, n, m):
    """L, U, alpha, beta, p, q per entry to 16 eps relative (a handful of roundings each), b to 1e-13 of its sum, at steps
    1 to 4 and at step 20, where the asymptotes of the climbing and of the alternating variables sit on their four clamps
    (0.5 x 1.2^17 > 10 and 0.5 x 0.7^11 < 0.01: no earlier step reaches them); a second run gives the same bits."""
    steps, keep = 20, (1, 2, 3, 4, 20)
    xmin, xmax, xs, grads, fs = _design_sequence(n, m, steps, seed=7 * n + m)
    dev = _run_elementwise(gpu, n, m, steps, 7 * n + m, keep)
    ref = R.MMA(xmin, xmax, m)
    worst = 0.0
    for k in range(steps):
        x = xs[k]
        ref.k += 1
        L, U = R.asymptotes(ref.k, x, xmin, xmax, ref.x1, ref.x2, ref.low, ref.upp)
        alfa, beta = R.move_limits(x, xmin, xmax, L, U, 0.5)
        p, q = R.approximation(x, xmin, xmax, L, U, grads[k])
        b, bsum = R.constants_b(x, L, U, p[1:], q[1:], fs[k])
        ref.x2, ref.x1, ref.low, ref.upp = ref.x1, x.copy(), L, U
        if k + 1 not in keep:
            continue
        d = dev[k + 1]
        for name, a in (("L", L), ("U", U), ("alfa", alfa), ("beta", beta), ("p", p), ("q", q)):
            err = np.abs(d[name] - a)
            scale = np.abs(a)
            worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0)
            assert np.all(err <= 16 * EPS * scale), (name, k + 1, float((err / np.maximum(scale, 1e-300)).max()) / EPS)
        if m:
            assert np.all(np.abs(d["b"] - b) <= 1e-13 * bsum), (k + 1, np.abs(d["b"] - b) / bsum)
        if k + 1 == 20 and n >= 63:
            span, pat = xmax - xmin, np.arange(n) % 5
            assert np.all(d["L"][pat == 1] == (x - 10.0 * span)[pat == 1]) and np.all(d["U"][pat == 1] == (x + 10.0 * span)[pat == 1])
            assert np.all(d["L"][pat == 2] == (x - 0.01 * span)[pat == 2]) and np.all(d["U"][pat == 2] == (x + 0.01 * span)[pat == 2])
            assert np.all(d["alfa"][pat == 3] == xmin[pat == 3]) and np.all(d["beta"][pat == 4] == xmax[pat == 4])
    print(f"n={n} m={m}: largest relative difference {worst / EPS:.2f} eps")
    again = _run_elementwise(gpu, n, m, steps, 7 * n + m, keep)
    for k in keep:
        for name in dev[k]:
            assert np.array_equal(dev[k][name], again[k][name]), (name, k)


# ---- one subproblem from given arrays -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", SIZES)
def test_subproblem(gpu, n, m):
    """The KKT residual of the device's point, evaluated by the restatement, is <= 2 sub_tol (the last stage ends with
    residual <= 0.9 eps at barrier eps <= sub_tol, and the complementarity rows differ from their barrier-0 form by eps);
    stages and Newton steps equal the restatement's; x agrees within ten times what the restatement's own x moves between
    sub_tol 1e-7 and 1e-10, never looser than 1e-6 of the range (1 here).  m = 0: the closed form to 4 eps."""
    from femo_amd.opt import DeviceMMA
    s = R.random_subproblem(n, m, seed=11 * n + m)
    opt = DeviceMMA(gpu, _vec(gpu, np.zeros(n)), _vec(gpu, np.ones(n)), m)
    x, rec = opt.solve_subproblem(s["L"], s["U"], s["alfa"], s["beta"], s["p"], s["q"], s["b"])
    xr, rr = R.subsolve(*R.sub_args(s), sub_tol=1e-7)
    if m == 0:
        assert rec["newton"] == 0 and rec["stages"] == 0 and rec["converged"] == 1
        assert np.all(np.abs(x - xr) <= 4 * EPS * np.maximum(np.abs(xr), 1.0))
        return
    xt, _ = R.subsolve(*R.sub_args(s), sub_tol=1e-10)
    bound = min(10.0 * np.abs(xr - xt).max(), 1e-6)
    kkt = R.kkt_residual(*R.sub_args(s), x, rec)
    diff = np.abs(x - xr).max()
    print(f"n={n} m={m}: KKT {kkt:.2e}, newton {rec['newton']} (restatement {rr['newton']}), halvings {rec['halvings']} "
          f"({rr['halvings']}), max|x - x_ref| {diff:.2e}, bound {bound:.2e}, blocking copies {rec['blocking_copies']}")
    assert rec["converged"] == 1 and rr["converged"] == 1
    assert kkt <= 2e-7
    assert (rec["stages"], rec["newton"], rec["halvings"]) == (rr["stages"], rr["newton"], rr["halvings"])
    assert diff <= bound
    x2, rec2 = opt.solve_subproblem(s["L"], s["U"], s["alfa"], s["beta"], s["p"], s["q"], s["b"])
    assert np.array_equal(x, x2) and np.array_equal(rec["lam"], rec2["lam"])


# ---- Svanberg's cantilever -----------------------------------------------------------------------------------------------------
def test_svanberg_cantilever_on_the_device(gpu):
    from femo_amd.opt import DeviceMMA
    coef = np.array([61.0, 37.0, 19.0, 7.0, 1.0])
    opt = DeviceMMA(gpu, _vec(gpu, np.ones(5)), _vec(gpu, np.full(5, 10.0)), 1)
    x = _vec(gpu, np.full(5, 5.0))
    for _ in range(30):
        xh = np.array(x.get())
        info = opt.update(x, 0.0624 * xh.sum(), _vec(gpu, np.full(5, 0.0624)), [(coef / xh ** 3).sum() - 1.0],
                          _vec(gpu, -3.0 * coef / xh ** 4))
        assert info["converged"] == 1
    xh = np.array(x.get())
    assert round(0.0624 * xh.sum(), 4) == 1.3400
    assert np.abs(xh - np.array([6.016, 5.309, 4.494, 3.502, 2.153])).max() <= 2e-3


# ---- refusals through the library's error path ---------------------------------------------------------------------------------
def test_library_refusals(gpu):
    from femo_amd.opt import DeviceMMA
    lo, hi = _vec(gpu, np.zeros(70)), _vec(gpu, np.ones(70))
    bad = np.ones(70); bad[64] = 0.0
    for a, b in ((lo, _vec(gpu, bad)), (_vec(gpu, np.where(np.arange(70) == 3, np.nan, 0.0)), hi), (lo, _vec(gpu, np.full(70, np.inf)))):
        with pytest.raises(ValueError):
            DeviceMMA(gpu, a, b, 1)
    with pytest.raises(ValueError):
        DeviceMMA(gpu, lo, hi, 9)
    with pytest.raises(ValueError):
        DeviceMMA(gpu, lo, hi, 1, move=0.0)
    opt = DeviceMMA(gpu, lo, hi, 1)
    g, ok = _vec(gpu, np.ones(70)), np.full(70, 0.5)
    for xbad in (np.where(np.arange(70) == 69, 1.5, 0.5), np.where(np.arange(70) == 0, np.nan, 0.5)):
        with pytest.raises(ValueError):
            opt.update(_vec(gpu, xbad), 1.0, g, [0.0], g)
    with pytest.raises(ValueError):
        opt.update(_vec(gpu, ok), 1.0, _vec(gpu, np.where(np.arange(70) == 65, np.inf, 1.0)), [0.0], g)
    with pytest.raises(ValueError):
        opt.update(_vec(gpu, ok), 1.0, g, [np.nan], g)
    with pytest.raises(ValueError):
        opt.update(_vec(gpu, ok), np.inf, g, [0.0], g)
    info = opt.update(_vec(gpu, ok), 1.0, g, [0.0], g)          # the refused calls left no trace: this is step 1
    assert info["step"] == 1 and info["converged"] == 1


# ---- restart ---------------------------------------------------------------------------------------------------------------------
def test_reset_gives_the_same_bits(gpu):
    from femo_amd.opt import DeviceMMA
    n, m = 1000, 3
    rng = np.random.default_rng(5)
    t = 0.5 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.8, 1.5, n)
    A = rng.standard_normal((m, n)) / np.sqrt(n)                      # rows of norm one, an objective of order one
    a = A @ np.clip(t, 0.0, 1.0) - rng.uniform(0.2, 0.5, m)
    f00 = ((0.5 - t) ** 2).sum()
    opt = DeviceMMA(gpu, _vec(gpu, np.zeros(n)), _vec(gpu, np.ones(n)), m)
    runs = []
    for _ in range(2):
        opt.reset()
        x, hist = _vec(gpu, np.full(n, 0.5)), []
        for k in range(5):
            xh = np.array(x.get())
            info = opt.update(x, ((xh - t) ** 2).sum() / f00, _vec(gpu, 2.0 * (xh - t) / f00), A @ xh - a, _vec(gpu, A))
            assert info["step"] == k + 1 and info["converged"] == 1
            hist.append((np.array(x.get()), info["lam"], info["newton_steps"]))
        runs.append(hist)
    for (x0, l0, n0), (x1, l1, n1) in zip(*runs):
        assert np.array_equal(x0, x1) and np.array_equal(l0, l1) and n0 == n1
    assert not np.array_equal(runs[0][3][0], runs[0][4][0])


# ---- the design loop ---------------------------------------------------------------------------------------------------------------
NELX, NELY, STEPS = 24, 12, 30
_LOOP = {}


def _reference_loop(mesh, facets, h_avg, noise):
    """The 24 x 12 cantilever driven by the restatement and tests/elasticity_ref.py: (J_k, f_k, x_k) before every update.
    noise: relative perturbation of the objective's gradient, entry by entry (the sensitivity experiment)."""
    X, conn = mesh.x, mesh.conn
    W = eref.filter_matrix(mesh.centroids(), 2.0 * h_avg)
    K0 = eref.element_matrices(X, conn)
    F = eref.traction_load(X, facets, (0.0, -0.25))
    fv = np.nonzero(np.isclose(X[:, 0], 0.0))[0]
    fixed = np.concatenate([2 * fv, 2 * fv + 1])
    vol = eref.cell_volumes(X, conn)
    n = mesh.n_cell
    rng = np.random.default_rng(1)
    opt = R.MMA(np.full(n, 1e-4), np.ones(n), 1)
    x, hist, J0 = np.full(n, 0.4), [], None
    gc = W.T @ (vol / vol.sum())
    for _ in range(STEPS):
        rho = W @ x
        u = eref.solve_fixed(eref.stiffness(X, conn, rho, "SIMP", K0=K0), F, fixed)
        J = F @ u
        g = W.T @ (-eref.compliance_gradient(X, conn, rho, u, u, "SIMP", K0=K0))
        f = vol @ rho / vol.sum() - 0.4
        J0 = J if J0 is None else J0
        if noise:
            g = g * (1.0 + noise * rng.standard_normal(n))
        hist.append((J, f, x.copy(), None))
        x = opt.update(x, g / J0, [f], gc[None, :])
        hist[-1] = hist[-1][:3] + (opt.last["rec"]["newton"],)
        assert opt.last["rec"]["converged"] == 1
    return hist


def _loop_reference():
    """Computed once for both modes: the restatement's loop, and how far a relative 1e-8 in the gradients (the asserted
    parity bound of test_cantilever_cycle) moves it."""
    if not _LOOP:
        from test_gpu_topopt import build_cantilever
        _, _, mesh, aux = build_cantilever(NELX, NELY, device=False)
        clean = _reference_loop(mesh, aux["facets"], aux["h_avg"], 0.0)
        noisy = _reference_loop(mesh, aux["facets"], aux["h_avg"], 1e-8)
        dx = max(np.abs(a[2] - b[2]).max() for a, b in zip(clean, noisy))
        dJ = max(abs(a[0] - b[0]) / abs(a[0]) for a, b in zip(clean, noisy))
        _LOOP.update(clean=clean, dx=dx, dJ=dJ)
    return _LOOP


@pytest.mark.parametrize("device", [True, False])
def test_design_loop_cantilever(gpu, device):
    """24 x 12 cells on 160 x 80, SIMP, filter radius 2 h_avg, x = 0.4, avg_density <= 0.40, 30 steps, step by step against
    the restatement: x and J within ten times what a relative 1e-8 in the gradients moves the restatement's own loop
    (never looser than 1e-4 in x, 1e-5 relative in J).  And conditions: every constraint value <= 1e-9 from step 2 on,
    J_30 <= 0.35 J_1, every subproblem converged, and in device mode no vector-sized host copy during solve()."""
    from femo_amd import engine
    from femo_amd.opt import MMA, CSDLProblem
    from test_gpu_topopt import build_cantilever
    ref = _loop_reference()
    sim, fea, mesh, aux = build_cantilever(NELX, NELY, device=device)
    n = mesh.n_cell
    assert n == 576
    sim['density_unfiltered'] = np.full(n, 0.4)
    prob = CSDLProblem(problem_name='beam_topo_opt', simulator=sim)
    xs = []
    optimizer = MMA(prob, max_iter=STEPS, move=0.5, tol=0.0, sub_tol=1e-7, normalize=True).setup()
    run = sim.run

    def recording_run():                                   # the design every cycle starts from
        xs.append(sim.device_value('density_unfiltered').copy() if device else np.array(sim['density_unfiltered']))
        run()
    sim.run = recording_run
    gpu.sync()
    engine.host_stats(reset=True)
    res = optimizer.solve()
    stats = engine.host_stats()
    optimizer.print_results()
    xs = [np.asarray(v) for v in xs]
    bx, bJ = min(10.0 * ref["dx"], 1e-4), min(10.0 * ref["dJ"], 1e-5)
    ex = max(np.abs(x - r[2]).max() for x, r in zip(xs, ref["clean"]))
    eJ = max(abs(J - r[0]) / abs(r[0]) for J, r in zip(res["objective"], ref["clean"]))
    print(f"device={device}: J {res['objective'][0]:.2f} -> {res['objective'][-1]:.2f}; sensitivity of the restatement to 1e-8 in "
          f"the gradients: x {ref['dx']:.2e}, J {ref['dJ']:.2e}; device against restatement: x {ex:.2e} (bound {bx:.2e}), "
          f"J {eJ:.2e} (bound {bJ:.2e}); Newton steps {min(res['inner'])}..{max(res['inner'])}; "
          f"constraint from step 2: {min(f[0] for f in res['constraints'][1:]):.2e}..{max(f[0] for f in res['constraints'][1:]):.2e}")
    assert len(res["objective"]) == STEPS == len(xs)
    assert ex <= bx and eJ <= bJ
    assert res["inner"] == [r[3] for r in ref["clean"]]
    assert all(f[0] <= 1e-9 for f in res["constraints"][1:])
    assert res["objective"][-1] <= 0.35 * res["objective"][0]
    assert all(c == 1 for c in res["converged"])
    if device:
        # function values and solver records cross the link, 8 bytes at a time; x or a gradient crossing once per step
        # would be 8 n bytes a step.  Asserted: less than half a vector per step, over all copies in both directions.
        moved = {k: v for k, v in stats.items() if v and not k.startswith("h2d_skipped")}
        print("host traffic during solve():", moved)
        assert sum(v for k, v in moved.items() if k.endswith("_bytes")) < 8 * n * STEPS // 2, moved


# ---- two constraints: volume and the aggregated von Mises stress -----------------------------------------------------------------
def _two_constraint_reference(P, vol, m_scale, bound, noise, steps):
    import elast_stress_ref as sref
    n = vol.size
    rng = np.random.default_rng(2)
    opt = R.MMA(np.full(n, 1e-4), np.ones(n), 2)
    gc = P["W"].T @ (vol / vol.sum())
    x, hist, J0 = np.full(n, 0.4), [], None
    for _ in range(steps):
        T = sref.cantilever_total(P, x, m_scale)
        J = P["F"] @ T["u"]
        g = P["W"].T @ (-eref.compliance_gradient(P["x"], P["conn"], T["rho"], T["u"], T["u"], "SIMP", K0=P["K0"]))
        gs = T["grad"]
        J0 = J if J0 is None else J0
        if noise:
            g, gs = g * (1.0 + noise * rng.standard_normal(n)), gs * (1.0 + noise * rng.standard_normal(n))
        f = [vol @ T["rho"] / vol.sum() - 0.4, T["value"] - bound]
        hist.append((J, f, x.copy()))
        x = opt.update(x, g / J0, f, np.vstack([gc, gs]))
        assert opt.last["rec"]["converged"] == 1
        hist[-1] += (opt.last["rec"]["newton"],)
    return hist


def test_two_constraints_volume_and_stress(gpu):
    """8 x 4 cells on 160 x 80: compliance under avg_density <= 0.40 and pnorm_stress <= 0.9 times its value at the start
    design, 10 steps, step by step against the restatement (tests/elast_stress_ref.py for the aggregate and its total
    derivative), by the rule of the design loop: ten times what a relative 1e-8 in the gradients moves the restatement's
    own iterates, never looser than 1e-4 in x and 1e-5 relative in J.  The smallest case with m = 2 and gradients of both
    signs (the stress gradient)."""
    import argparse
    import importlib.util
    import os
    import elast_stress_ref as sref
    from femo_amd.fea.mesh import meshSize
    from femo_amd.opt import MMA, CSDLProblem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_topopt", os.path.join(root, "scripts", "run_topopt.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    steps = 10
    sim, model, mesh, stress = driver.build(argparse.Namespace(n3=0, nelx=8, nely=4, pc="jacobi", stress=True, device=True))
    n = mesh.n_cell
    from femo_amd.fea.mesh import locate_entities_boundary
    facets = locate_entities_boundary(mesh, 1, lambda x: np.logical_and(abs(x[1] - 40.0) < 80.0 / 4 + 3e-6, abs(x[0] - 160.0) < 3e-6))
    h = meshSize(mesh)
    P = sref.cantilever_problem(mesh, facets, (h.max() + h.min()) / 2)
    vol = eref.cell_volumes(mesh.x, mesh.conn)
    start = sref.cantilever_total(P, np.full(n, 0.4), 1.0)
    m_scale = 1.0 / float(start["field"].max())                 # the aggregate's scale, fixed from the start design
    bound = 0.9 * sref.cantilever_value(P, np.full(n, 0.4), m_scale)
    clean = _two_constraint_reference(P, vol, m_scale, bound, 0.0, steps)
    noisy = _two_constraint_reference(P, vol, m_scale, bound, 1e-8, steps)
    dx = max(np.abs(a[2] - b[2]).max() for a, b in zip(clean, noisy))
    dJ = max(abs(a[0] - b[0]) / abs(a[0]) for a, b in zip(clean, noisy))
    stress.m = m_scale
    model.add_constraint("stress", upper=bound)
    prob = CSDLProblem(problem_name="beam_topo_opt_stress", simulator=sim)
    assert prob.m == 2 and [r.name for r in prob.rows] == ["avg_density", "stress"]
    xs, run = [], sim.run

    def recording_run():
        xs.append(sim.device_value("density_unfiltered").copy())
        run()
    sim.run = recording_run
    res = MMA(prob, max_iter=steps, tol=0.0).solve()
    xs = [np.asarray(v) for v in xs]
    bx, bJ = min(10.0 * dx, 1e-4), min(10.0 * dJ, 1e-5)
    ex = max(np.abs(x - r[2]).max() for x, r in zip(xs, clean))
    eJ = max(abs(J - r[0]) / abs(r[0]) for J, r in zip(res["objective"], clean))
    ef = max(np.abs(np.array(f) - np.array(r[1])).max() for f, r in zip(res["constraints"], clean))
    print(f"two constraints: J {res['objective'][0]:.2f} -> {res['objective'][-1]:.2f}, rows at the last step {res['constraints'][-1]}; "
          f"sensitivity to 1e-8: x {dx:.2e}, J {dJ:.2e}; device against restatement: x {ex:.2e} (bound {bx:.2e}), J {eJ:.2e} "
          f"(bound {bJ:.2e}), rows {ef:.2e}; Newton steps {res['inner']} (restatement {[r[3] for r in clean]})")
    assert len(xs) == steps and ex <= bx and eJ <= bJ
    assert res["inner"] == [r[3] for r in clean]
    assert all(c == 1 for c in res["converged"])
