"""One SIMP design cycle of examples/beam_topo_opt on the HIP engine, timed: filter -> state solve -> compliance ->
adjoint -> W^T, through FEAModel + GeneralFilterModel + Simulator (host values, like a CSDL backend).  Prints one JSON
line: ms per cycle (wall clock between two device synchronisations), PCG iterations of the forward and adjoint solves, block-SpMV time
and its share of 8 TB/s, the filter build time, and a SciPy spsolve cycle of the same size timed beside it.

  python scripts/bench_topopt.py --nelx 640 --nely 320          (2-D cantilever, the reference's driver at that size)
  python scripts/bench_topopt.py --n3 48                        (3-D unit cube, clamped at x = 0, load on x = 1)
  ... --pc multilevel                                           (the lattice preconditioner of csrc/elast_pc.hip; default jacobi)
  ... --stress                                                  (adds the aggregated von Mises stress as a second scalar output and its
                                                                 total derivative to the cycle: one more adjoint solve, whose right-hand
                                                                 side is not the load; reported as extra keys of the JSON line)
  ... --load-cases L                                            (2 <= L <= 8: L load cases on one K(rho) through pdeRes_multiload /
                                                                 compliance_multiload, every solve of the cycle one batched PCG;
                                                                 the loads are listed under `load_cases` below.  Adds to the JSON
                                                                 line load_cases, the iteration counts per column, and the
                                                                 batched solve timed against L sequential single-column solves of
                                                                 the same right-hand sides: solve_ms_batched, solve_ms_sequential,
                                                                 and the spread of their 5 alternated repeats)
  ... --load-cases L --stress                                   (adds sum_l J_l, the aggregated von Mises stress of every load case
                                                                 (pnorm_stress_multiload, scales m_l from the first state), and its
                                                                 total derivative to the timed cycle: one more batched adjoint solve,
                                                                 whose right-hand sides are live on the clamped dofs.  Adds stress,
                                                                 stress_values, stress_m, the iterations per column of that solve,
                                                                 and the batched stress evaluation (value + dJ/du + dJ/drho in one
                                                                 call) timed against L single-column calls on the same columns:
                                                                 stress_ms_batched, stress_ms_sequential and their spread)
  ... --harmonic N                                              (1 <= N <= 8: the harmonic response (K - omega_l^2 M) u_l = F of the tip
                                                                 load at N frequencies through pdeRes_harmonic / dynamic_compliance,
                                                                 every solve of the cycle one batched MINRES.  The frequencies are
                                                                 spread below and between the first eigenfrequencies of the start
                                                                 design (`harmonic_frequencies`).  Adds the MINRES iterations per
                                                                 column next to the PCG counts of the static solve of the same load,
                                                                 and the fused product (K - sigma M) x timed against apply_multi
                                                                 followed by mass_apply_multi on the same vectors: a warm-up, then
                                                                 5 alternated repeats, medians and spread)
  ... --harmonic N --loss-factor X                              (N <= 4: the same frequencies through pdeRes_harmonic_damped /
                                                                 dynamic_compliance_damped with the structural loss factor X as
                                                                 well, every solve one batched COCR in complex arithmetic.  Adds
                                                                 the COCR iterations and ms per column, and the time per iteration
                                                                 of the COCR and the MINRES state solves, alternated: a warm-up of
                                                                 both, then 5 pairs, medians)
  ... --thermal [--counts]                                      (the thermoelastic chain rho -> T(rho) -> u(rho, T) -> J -- a conduction
                                                                 state with the sink on the clamped edge, its temperature as the
                                                                 thermal expansion load beside the tip load, two adjoint solves --
                                                                 alternated cycle by cycle with the mechanical-only cycle of the same
                                                                 build; the three launches of the thermal-load operator and the
                                                                 conduction assembly in windows of 200 launches; --counts adds the
                                                                 PCG iterations of the conduction solves at three sizes, Jacobi and
                                                                 the lattice preconditioner side by side; with --pc multilevel the
                                                                 conduction form takes the lattice preconditioner too, and a third
                                                                 leg, the same cycle with the conduction form on Jacobi, is alternated
                                                                 with the other two)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12


def build(args):
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel, HelmholtzFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, VectorFunctionSpace,
                                      createRectangleMesh, createUnitCubeMesh, locate_dofs_geometrical,
                                      locate_entities_boundary, meshSize, meshtags)
    if args.n3:
        mesh = createUnitCubeMesh(args.n3)
        marker = lambda x: np.logical_and(np.isclose(x[0], 1.0), x[2] < 0.25)
        t = (0.0, 0.0, -1.0)
    else:
        LX, LY = 160.0, 80.0
        mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), args.nelx, args.nely)
        marker = lambda x: np.logical_and(abs(x[1] - LY / 2) < LY / args.nely + 3e-6, abs(x[0] - LX) < 3e-6)
        t = (0.0, -0.25)
    d = mesh.tdim
    facets = locate_entities_boundary(mesh, d - 1, marker)
    ds_ = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 100, dtype=np.int32)))
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(V)
    f = Constant(mesh, t)
    res = pdeRes(u, None, rho, f, dss=ds_(100), preconditioner=args.pc)
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    fea.add_output(name="avg_density", type="scalar", form=averageFunc(rho), arguments=["density"])
    fea.add_output(name="compliance", type="scalar", form=compliance(u, f, dss=ds_(100)), arguments=["displacements"])
    stress = None
    if args.stress:
        from femo_amd.fea.elasticity import pnorm_stress
        stress = pnorm_stress(u, rho, p=8.0, q=0.5)                 # m is set from the first state (main)
        fea.add_output(name="stress", type="scalar", form=stress, arguments=["displacements", "density"])
        fea.consistent_bc_partials = True                           # dJ/du is not zero on the clamped dofs
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    t0 = time.perf_counter()
    h_avg = (h.max() + h.min()) / 2
    if args.filter == "helmholtz":
        fm = HelmholtzFilterModel(mesh=mesh, beta=args.radius_h, h_avg=h_avg)
    else:
        fm = GeneralFilterModel(nel=mesh.n_cell, beta=args.radius_h, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg)
    model.add(fm, name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    sim = Simulator(model)                                      # defines the filter operation: W, W^T built here
    from femo_amd.fea.utils_hip import get_context
    get_context().sync()
    filter_build_ms = (time.perf_counter() - t0) * 1e3
    return sim, mesh, res, facets, t, filter_build_ms, stress


def load_cases(d, n_cases, nely=None):
    """(marker, traction) of the first ``n_cases`` loads.  Load 0 is the tip load of the single-load cycle; the others act
    on further pieces of the boundary away from the clamped face x = 0:

      2-D, the 160 x 80 cantilever                          3-D, the unit cube
      0  right edge at mid-height (one cell up and down), t = (0, -1/4)    face x = 1 below z = 1/4, t = (0, 0, -1)
      1  top edge beyond x = 3/4 L_X,    t = (0, -1/4)      face z = 1 beyond x = 3/4, t = (0, 0, -1)
      2  the whole right edge,           t = (1/4, 0)       the whole face x = 1,      t = (1, 0, 0)
      3  bottom edge beyond x = 3/4 L_X, t = (0, 1/4)       face z = 0 beyond x = 3/4, t = (0, 0, 1)
      4  top edge, x in (1/2, 3/4) L_X,  t = (0, -1/4)      face y = 1 beyond x = 3/4, t = (0, -1, 0)
      5  bottom edge, same piece,        t = (0, 1/4)       face y = 0 beyond x = 3/4, t = (0, 1, 0)
      6  top edge beyond x = 3/4 L_X,    t = (1/4, 0)       face x = 1 below y = 1/4,  t = (0, -1, 0)
      7  the whole right edge,           t = (0, -1/4)      face x = 1 above z = 3/4,  t = (0, 0, 1)"""
    e = 3e-6
    if d == 2:
        LX, LY = 160.0, 80.0
        right = lambda x: abs(x[0] - LX) < e
        top = lambda lo, hi: (lambda x: np.logical_and(abs(x[1] - LY) < e, np.logical_and(x[0] > lo * LX - e, x[0] < hi * LX + e)))
        bot = lambda lo, hi: (lambda x: np.logical_and(abs(x[1]) < e, np.logical_and(x[0] > lo * LX - e, x[0] < hi * LX + e)))
        cases = [(lambda x: np.logical_and(abs(x[1] - LY / 2) < LY / nely + e, abs(x[0] - LX) < e), (0.0, -0.25)),
                 (top(0.75, 1.0), (0.0, -0.25)), (right, (0.25, 0.0)), (bot(0.75, 1.0), (0.0, 0.25)),
                 (top(0.5, 0.75), (0.0, -0.25)), (bot(0.5, 0.75), (0.0, 0.25)), (top(0.75, 1.0), (0.25, 0.0)),
                 (right, (0.0, -0.25))]
    else:
        on = lambda k, v: (lambda x: np.isclose(x[k], v))
        both = lambda a, b: (lambda x: np.logical_and(a(x), b(x)))
        far = lambda x: x[0] > 0.75 - e
        cases = [(both(on(0, 1.0), lambda x: x[2] < 0.25), (0.0, 0.0, -1.0)), (both(on(2, 1.0), far), (0.0, 0.0, -1.0)),
                 (on(0, 1.0), (1.0, 0.0, 0.0)), (both(on(2, 0.0), far), (0.0, 0.0, 1.0)),
                 (both(on(1, 1.0), far), (0.0, -1.0, 0.0)), (both(on(1, 0.0), far), (0.0, 1.0, 0.0)),
                 (both(on(0, 1.0), lambda x: x[1] < 0.25), (0.0, -1.0, 0.0)),
                 (both(on(0, 1.0), lambda x: x[2] > 0.75), (0.0, 0.0, 1.0))]
    return cases[:n_cases]


def build_multi(args):
    """The model of `build` with ``args.load_cases`` loads: the state is a Function(LoadCaseSpace(V, L))."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, VectorFunctionSpace,
                                      compliance_multiload, createRectangleMesh, createUnitCubeMesh,
                                      locate_dofs_geometrical, locate_entities_boundary, meshSize, meshtags, pdeRes_multiload)
    if args.n3:
        mesh = createUnitCubeMesh(args.n3)
    else:
        mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), args.nelx, args.nely)
    d = mesh.tdim
    dss, fs = [], []
    for l, (marker, t) in enumerate(load_cases(d, args.load_cases, args.nely)):
        facets = locate_entities_boundary(mesh, d - 1, marker)
        if len(facets) == 0:
            raise SystemExit(f"load case {l} has no facets on this mesh")
        dss.append(Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 100 + l, dtype=np.int32)))(100 + l))
        fs.append(Constant(mesh, t))
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(LoadCaseSpace(V, args.load_cases))
    res = pdeRes_multiload(u, None, rho, fs, dss, preconditioner=args.pc)
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    fea.add_output(name="compliance", type="scalar", form=compliance_multiload(u, fs, dss), arguments=["displacements"])
    stress = None
    if args.stress:
        from femo_amd.fea.fea_hip import pnorm_stress_multiload
        stress = pnorm_stress_multiload(u, rho, p=8.0, q=0.5)       # the m_l are set from the first state (main_multi)
        fea.add_output(name="stress", type="scalar", form=stress, arguments=["displacements", "density"])
        fea.consistent_bc_partials = True                           # dJ/du is not zero on the clamped dofs of any column
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    return Simulator(model), mesh, res, stress


def time_stress_multi(ctx, stress, L):
    """The batched stress evaluation (value, dJ/du and dJ/drho in one call) against L calls of the single-column
    `pnorm_stress` on the same columns with the same m_l: a warm-up of both, then 5 alternated repeats, each between two
    device synchronisations."""
    from femo_amd.engine import Vec
    dev, rho = stress.device(), stress.rho.vec
    n, nc = dev.n_dof, stress.mesh.n_cell
    U = np.array(stress.u.vec.get()).reshape(L, n)
    us = [Vec(ctx, n).set(U[l]) for l in range(L)]
    gm, gr = Vec(ctx, L * n), Vec(ctx, nc)
    g1, r1 = Vec(ctx, n), Vec(ctx, nc)

    def batched():
        ctx.sync()
        t0 = time.perf_counter()
        dev.pnorm_stress_multi(L, rho, stress.u.vec, stress.m, stress.p, stress.q, stress.alpha, weights=stress.weights,
                               grad_u=gm, grad_rho=gr)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def sequential():
        ctx.sync()
        t0 = time.perf_counter()
        for l in range(L):
            dev.pnorm_stress(rho, us[l], stress.m[l], stress.p, stress.q, stress.alpha, grad_u=g1, grad_rho=r1, accumulate=l > 0)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    batched(); sequential()
    tb, ts = [], []
    for _ in range(5):
        tb.append(batched())
        ts.append(sequential())
    spread = max(max(tb) - min(tb), max(ts) - min(ts))
    return dict(stress_ms_batched=float(np.median(tb)), stress_ms_sequential=float(np.median(ts)),
                stress_ms_batched_all=[float(v) for v in tb], stress_ms_sequential_all=[float(v) for v in ts],
                stress_ms_spread=float(spread), stress_batched_faster_than_spread=bool(np.median(ts) - np.median(tb) > spread))


def main_multi(args, ctx):
    """The cycle with L load cases, then the batched solve against L sequential single-column solves of the same
    right-hand sides on the same handle: a warm-up of both, then 5 alternated repeats, wall clock around calls that end in
    a device synchronisation."""
    from femo_amd.engine import Vec
    L = args.load_cases
    sim, mesh, res, stress = build_multi(args)
    x0 = np.array(sim["density_unfiltered"])
    times = []
    for k in range(args.cycles + 1):
        sim["density_unfiltered"] = x0 * (1.0 - 1e-3 * k)
        ctx.sync()
        t0 = time.perf_counter()
        sim.run()
        np.asarray(sim.compute_totals("compliance", "density_unfiltered"))
        if stress is not None:
            it_compliance_adjoint = res.last_info["adjoint"]["iterations"]
            if k == 0:                                              # scales of the aggregates, fixed from the first state
                stress.set_scales_from_state()
                sim.run()
            gs = np.asarray(sim.compute_totals("stress", "density_unfiltered"))
        ctx.sync()
        if k > 0:
            times.append((time.perf_counter() - t0) * 1e3)
    info = res.last_info
    dev = res.stiffness()
    n = dev.n_dof
    B = np.array(res._rhs(dev).get()).reshape(L, n)
    bm, xm = Vec(ctx, L * n).set(B.ravel()), Vec(ctx, L * n)
    bs, xs = [Vec(ctx, n).set(B[l]) for l in range(L)], Vec(ctx, n)

    def batched():
        ctx.sync()
        t0 = time.perf_counter()
        infos = dev.solve_multi(L, bm, xm, pc=args.pc)
        return (time.perf_counter() - t0) * 1e3, infos

    def sequential():
        ctx.sync()
        t0 = time.perf_counter()
        infos = [dev.solve(bs[l], xs, pc=args.pc) for l in range(L)]
        return (time.perf_counter() - t0) * 1e3, infos

    batched(); sequential()
    tb, ts = [], []
    for _ in range(5):
        t, ib = batched(); tb.append(t)
        t, isq = sequential(); ts.append(t)
    spread = max(max(tb) - min(tb), max(ts) - min(ts))
    out = dict(metric="topopt_cycle_multiload", mesh=(f"cube n={args.n3}" if args.n3 else f"rect {args.nelx}x{args.nely}"),
               n_dof=n, n_cell=mesh.n_cell, load_cases=L, pc=args.pc, cycle_ms=float(np.median(times)),
               cycle_ms_all=[float(v) for v in times], pcg_iterations_forward=info["state"]["iterations"],
               pcg_iterations_adjoint=info["adjoint"]["iterations"], compliance=float(sim["compliance"][0]),
               solve_ms_batched=float(np.median(tb)), solve_ms_sequential=float(np.median(ts)),
               solve_ms_batched_all=[float(v) for v in tb], solve_ms_sequential_all=[float(v) for v in ts], spread=float(spread),
               batched_faster_than_spread=bool(np.median(ts) - np.median(tb) > spread),
               device_ms_batched=float(ib[0].solve_ms), device_ms_sequential=float(sum(i.solve_ms for i in isq)),
               iterations_batched=[i.iterations for i in ib], iterations_sequential=[i.iterations for i in isq],
               converged=[i.converged for i in ib])
    if stress is not None:
        out.update(pcg_iterations_adjoint=it_compliance_adjoint, pcg_iterations_stress_adjoint=info["adjoint"]["iterations"],
                   stress=float(sim["stress"][0]), stress_values=[float(v) for v in stress.values()],
                   stress_m=[float(v) for v in stress.m], stress_p=stress.p, stress_q=stress.q,
                   stress_gradient_norm=float(np.linalg.norm(gs)))
        out.update(time_stress_multi(ctx, stress, L))
    if args.pc == "multilevel":
        pci = dev.pc_info()
        out.update(pc_levels=pci["levels"], pc_nodes=pci["nodes"], pc_lattice_bytes=pci["bytes"])
    print(json.dumps(out))


def harmonic_frequencies(lam, n):
    """``n`` shifts sigma = omega^2 from the ascending eigenvalues ``lam``: lambda_1 / 2 first, then the geometric means of the
    consecutive pairs that lie at least 10 % apart (a pair closer than that is a cluster: its mean would sit on a resonance),
    and, when those run out, further fractions of lambda_1 below the first one."""
    lam = np.asarray(lam, dtype=np.float64)
    between = [float(np.sqrt(a * b)) for a, b in zip(lam[:-1], lam[1:]) if b >= 1.1 * a][:max(n - 1, 0)]
    below = [0.5 * lam[0] * (k + 1) / (n - len(between)) for k in range(n - len(between))]
    return np.array(sorted(below + between))


def time_products(ctx, dev, rho, shifts, density):
    """One fused product (K - sigma_l M) x_l against `apply_multi` followed by `mass_apply_multi` on the same vectors (both
    masked), and the static product alone beside them: a warm-up, then 5 alternated repeats, each a window of about 0.2 s of
    launches between two device synchronisations."""
    from femo_amd.engine import Vec
    L, n = len(shifts), dev.n_dof
    xv = Vec(ctx, L * n).set(np.random.default_rng(1).standard_normal(L * n))
    y, yk, ym = Vec(ctx, L * n), Vec(ctx, L * n), Vec(ctx, L * n)

    def timed(body, reps):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            body()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    fused = lambda: dev.dyn_apply_multi(L, shifts, xv, y, masked=True)
    split = lambda: (dev.apply_multi(L, xv, yk, masked=True), dev.mass_apply_multi(L, rho, xv, ym, masked=True, density=density))
    static = lambda: dev.apply_multi(L, xv, yk, masked=True)
    timed(fused, 20); timed(split, 20)
    reps = max(20, int(200.0 / timed(static, 20)))                    # windows of about 0.2 s of the static product
    tf, ts, tk = [], [], []
    for _ in range(5):
        tf.append(timed(fused, reps)); ts.append(timed(split, reps)); tk.append(timed(static, reps))
    spread = max(max(tf) - min(tf), max(ts) - min(ts))
    return dict(product_ms_fused=float(np.median(tf)), product_ms_two_pass=float(np.median(ts)),
                product_ms_static=float(np.median(tk)), product_ms_fused_all=[float(v) for v in tf],
                product_ms_two_pass_all=[float(v) for v in ts], product_ms_static_all=[float(v) for v in tk],
                product_reps=reps, product_ms_spread=float(spread), fused_faster_than_spread=bool(np.median(ts) - np.median(tf) > spread))


def main_harmonic(args, ctx):
    """The cycle filter -> batched MINRES state -> dynamic compliance -> batched MINRES adjoint -> W^T at N frequencies."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import ElasticityEigenvalues
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, VectorFunctionSpace,
                                      createRectangleMesh, createUnitCubeMesh, dirichletbc, dynamic_compliance,
                                      locate_dofs_geometrical, locate_entities_boundary, meshSize, meshtags, pdeRes_harmonic)
    N, density = args.harmonic, 1.0
    mesh = createUnitCubeMesh(args.n3) if args.n3 else createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), args.nelx, args.nely)
    d = mesh.tdim
    marker, t = load_cases(d, 1, args.nely)[0]
    facets = locate_entities_boundary(mesh, d - 1, marker)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    fs, dss = [Constant(mesh, t)] * N, [ds] * N
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(LoadCaseSpace(V, N))
    res = pdeRes_harmonic(u, None, rho, fs, dss, omegas=np.zeros(N), density=density, preconditioner=args.pc)
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    fea.add_output(name="dynamic_compliance", type="scalar", form=dynamic_compliance(u, fs, dss), arguments=["displacements"])
    ubc = Function(V)
    ubc.vector.set(0.0)
    clamped = locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))
    fea.add_strong_bc(ubc, [clamped], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    sim = Simulator(model)
    x0 = np.array(sim["density_unfiltered"])
    sim.run()                                                         # omega = 0: the filtered start design reaches `rho`
    # the first eigenfrequencies of the start design place the frequencies
    n_modes = min(N + 2, 8)
    eig = ElasticityEigenvalues(rho, V, [dirichletbc(0.0, clamped, V)], n_modes, block=8, density=density, preconditioner=args.pc,
                                rtol=1e-6)                      # enough to place the frequencies
    t0 = time.perf_counter()
    lam = eig.eigenvalues()
    eig_ms = (time.perf_counter() - t0) * 1e3
    shifts = harmonic_frequencies(lam, N)
    res.omegas, res.shifts = np.sqrt(shifts), shifts
    times = []
    for k in range(args.cycles + 1):
        sim["density_unfiltered"] = x0 * (1.0 - 1e-3 * k)
        ctx.sync()
        t0 = time.perf_counter()
        sim.run()
        g = np.asarray(sim.compute_totals("dynamic_compliance", "density_unfiltered"))
        ctx.sync()
        if k > 0:
            times.append((time.perf_counter() - t0) * 1e3)
    info = res.last_info
    dev = res.dynamic()
    n = dev.n_dof
    # the static PCG of the same load, for the iteration counts
    b = res._rhs(dev)
    static = dev.solve_multi(N, b, Vec(ctx, N * n), rtol=res.rtol, pc=args.pc)
    minres_static = dev.dyn_solve_multi(N, np.zeros(N), b, Vec(ctx, N * n), rtol=res.rtol, pc=args.pc)
    out = dict(metric="topopt_cycle_harmonic", mesh=(f"cube n={args.n3}" if args.n3 else f"rect {args.nelx}x{args.nely}"),
               n_dof=n, n_cell=mesh.n_cell, frequencies=N, pc=args.pc, cycle_ms=float(np.median(times)),
               cycle_ms_all=[float(v) for v in times], eigenvalues=[float(v) for v in lam], eig_ms=eig_ms,
               shifts=[float(v) for v in shifts], shift_over_lambda1=[float(v / lam[0]) for v in shifts],
               minres_iterations_forward=info["state"]["iterations"], minres_iterations_adjoint=info["adjoint"]["iterations"],
               minres_solve_ms_forward=info["state"]["solve_ms"], minres_solve_ms_adjoint=info["adjoint"]["solve_ms"],
               minres_iteration_us=1e3 * info["state"]["solve_ms"] / max(max(info["state"]["iterations"]), 1),
               pcg_iterations_static=[i.iterations for i in static], pcg_solve_ms_static=float(static[0].solve_ms),
               minres_iterations_static=[i.iterations for i in minres_static], minres_solve_ms_static=float(minres_static[0].solve_ms),
               dynamic_compliance=float(sim["dynamic_compliance"][0]), responses=[float(v) for v in fea.outputs_dict["dynamic_compliance"]["form"].responses()],
               gradient_norm=float(np.linalg.norm(g)))
    out.update(time_products(ctx, dev, rho.vec, shifts, density))
    if args.loss_factor is not None:
        out.update(damped_solves(ctx, res, u, fs, dss, fea.bc, args.loss_factor))
    if args.pc == "multilevel":
        pci = dev.pc_info()
        out.update(pc_levels=pci["levels"], pc_nodes=pci["nodes"], pc_lattice_bytes=pci["bytes"])
    print(json.dumps(out))


def damped_solves(ctx, res, u, fs, dss, bcs, loss_factor, repeats=5):
    """The frequencies of the undamped cycle through the damped forms with the structural loss factor ``loss_factor``: the
    state solve of `pdeRes_harmonic_damped` and the adjoint solve of `dynamic_compliance_damped`, one batched COCR each, on
    the density the undamped cycle ended with; beside them the undamped MINRES state solve of ``res`` again, alternated
    with the damped one (``repeats`` pairs after a warm-up of both), for the time per iteration of the two loops."""
    from femo_amd.engine import Vec
    from femo_amd.fea.fea_hip import Function, LoadCaseSpace, dynamic_compliance_damped, pdeRes_harmonic_damped
    N = res.n_cases
    V = u.function_space.base
    ud = Function(LoadCaseSpace(V, 2 * N))
    dres = pdeRes_harmonic_damped(ud, None, res.rho, fs, dss, omegas=res.omegas, loss_factor=loss_factor, density=res.density,
                                  mass_law=res.mass_law, method=res.method, preconditioner=res.preconditioner)
    J = dynamic_compliance_damped(ud, fs, dss)
    us = Function(u.function_space)
    t_cocr, t_minres = [], []
    for k in range(repeats + 1):
        dres.solve_state(ud, bcs)
        res.solve_state(us, bcs)
        if k > 0:
            t_cocr.append(dres.last_info["state"]["solve_ms"] / max(max(dres.last_info["state"]["iterations"]), 1))
            t_minres.append(res.last_info["state"]["solve_ms"] / max(max(res.last_info["state"]["iterations"]), 1))
    A = dres.matrix_class(dres, masked=True)
    g = np.array(J.assemble_derivative(ud).get())
    g[np.tile(dres._mask, 2 * N) == 1] = 0.0
    A.backend_solve_transpose(Vec(ctx, g.size).set(g), Vec(ctx, g.size))
    st, ad = dres.last_info["state"], dres.last_info["adjoint"]
    return dict(loss_factor=loss_factor, cocr_iterations_forward=st["iterations"], cocr_iterations_adjoint=ad["iterations"],
                cocr_solve_ms_forward=st["solve_ms"], cocr_solve_ms_adjoint=ad["solve_ms"],
                cocr_iteration_us=1e3 * float(np.median(t_cocr)), cocr_iteration_us_all=[1e3 * float(v) for v in t_cocr],
                minres_iteration_us_alternated=1e3 * float(np.median(t_minres)),
                minres_iteration_us_alternated_all=[1e3 * float(v) for v in t_minres],
                minres_iterations_alternated=res.last_info["state"]["iterations"],
                cocr_over_minres_iteration=float(np.median(t_cocr) / np.median(t_minres)),
                damped_dynamic_compliance=float(J.assemble_scalar()), damped_responses_abs=[float(abs(c)) for c in J.responses()])


def build_thermoelastic(args, thermal: bool, cond_pc=None):
    """The cantilever of `build` as the thermoelastic chain rho -> T(rho) -> u(rho, T) -> J (two FEA objects: uniform heating
    with the sink on the clamped edge, the tip traction plus the thermal load of the computed temperature, J the work of the
    total load), or with ``thermal`` False the mechanical cycle alone in the same set-up.  ``cond_pc``: the preconditioner of
    the conduction form (default: --pc, like the elasticity)."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, ThermalExpansion, VectorFunctionSpace,
                                      createRectangleMesh, locate_dofs_geometrical, locate_entities_boundary, meshSize, meshtags,
                                      pdeRes_conduction)
    LX, LY = 160.0, 80.0
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), args.nelx, args.nely)
    marker, t = load_cases(2, 1, args.nely)[0]
    facets = locate_entities_boundary(mesh, 1, marker)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    Q, P, V = FunctionSpace(mesh, ("DG", 0)), FunctionSpace(mesh, ("CG", 1)), VectorFunctionSpace(mesh, ("CG", 1))
    clamp = lambda x: np.isclose(x[0], 0.0, atol=1e-6)
    feas, res_t, th = [], None, None
    if thermal:
        ft = FEA(mesh)
        ft.REPORT = False
        ft.consistent_bc_partials = True
        rho_t, T = Function(Q), Function(P)
        res_t = pdeRes_conduction(T, None, rho_t, source=1e-2, k0=1.0, k_min=1e-3, preconditioner=cond_pc or args.pc)
        ft.add_input("density", rho_t)
        ft.add_state(name="temperature", function=T, residual_form=res_t, arguments=["density"])
        Tbc = Function(P)
        Tbc.vector.set(0.0)
        ft.add_strong_bc(Tbc, [locate_dofs_geometrical((P, P), clamp)], P)
        feas.append(ft)
    fe = FEA(mesh)
    fe.REPORT = False
    fe.consistent_bc_partials = True
    rho, u, f = Function(Q), Function(V), Constant(mesh, t)
    fe.add_input("density", rho)
    args_u = ["density"]
    if thermal:
        T_in = Function(P)
        th = ThermalExpansion(1e-2, T_in)
        fe.add_input("temperature", T_in)
        args_u.append("temperature")
    res = pdeRes(u, None, rho, f, dss=ds, preconditioner=args.pc, thermal=th)
    fe.add_state(name="displacements", function=u, residual_form=res, arguments=args_u)
    fe.add_output(name="compliance", type="scalar", form=compliance(u, f, dss=ds, rho_e=rho if thermal else None, thermal=th),
                  arguments=["displacements"] + (args_u if thermal else []))
    ubc = Function(V)
    ubc.vector.set(0.0)
    fe.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), clamp)], V)
    feas.append(fe)
    model = FEAModel(fea=feas)
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    return Simulator(model), mesh, res, res_t


def conduction_counts(ctx, sizes=((80, 40), (320, 160), (640, 320))):
    """PCG iterations of the conduction state (uniform source) and of an adjoint-like solve (right-hand side: the state) at
    rho = 0.5 and on the black / white truss pattern, k_min = 1e-3, the sink on x = 0, rtol 1e-13, with both preconditioners
    side by side: Jacobi (relative in the Jacobi norm) and the lattice preconditioner weighted by the operator's Galerkin
    diagonals (relative in its own norm)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import elast_pc_ref as pr
    from femo_amd.fea.conduction import ConductionResidual
    from femo_amd.fea.fea_hip import Function, FunctionSpace, createRectangleMesh, dirichletbc, locate_dofs_geometrical
    out = []
    for nelx, nely in sizes:
        mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), nelx, nely)
        Q, P = FunctionSpace(mesh, ("DG", 0)), FunctionSpace(mesh, ("CG", 1))
        T, rho = Function(P), Function(Q)
        forms = {pc: ConductionResidual(T, rho, source=1e-2, k0=1.0, k_min=1e-3, preconditioner=pc) for pc in ("jacobi", "multilevel")}
        bcs = [dirichletbc(0.0, locate_dofs_geometrical((P, P), lambda x: np.isclose(x[0], 0.0, atol=1e-6)), P)]
        for kind in ("uniform", "truss"):
            rho.vector[:] = pr.count_density(kind, mesh.centroids(), 80.0)
            row = dict(mesh=f"rect {nelx}x{nely}", density=kind, n_vert=mesh.n_vert)
            for pc, form in forms.items():
                form.solve_state(T, bcs)
                form.solve_state(T, bcs)                       # the second solve: hierarchy, weights and work vectors exist
                st = dict(form.last_info["state"])
                A, _ = form.assemble_system(bcs, False, None, None)
                lam = Function(P)
                A.backend_solve(T.vec, lam.vec)
                ad = form.last_info["adjoint"]
                tag = "" if pc == "jacobi" else "multilevel_"
                row.update({tag + "state_iterations": st["iterations"], tag + "state_ms": st["solve_ms"],
                            tag + "adjoint_iterations": ad["iterations"], tag + "adjoint_ms": ad["solve_ms"]})
            out.append(row)
    return out


def main_thermal(args, ctx):
    """The thermoelastic cycle and the mechanical-only cycle of the same build in alternation, the three launches of the
    thermal-load operator and the conduction assembly timed in windows of launches, and the conduction iteration counts."""
    from femo_amd import _lib
    from femo_amd.engine import Vec
    legs = {name: build_thermoelastic(args, name == "thermoelastic") for name in ("thermoelastic", "mechanical")}
    if args.pc == "multilevel":
        # the same cycle with the conduction form on Jacobi, alternated with the other two: what the lattice path is judged against
        legs["thermoelastic_cond_jacobi"] = build_thermoelastic(args, True, cond_pc="jacobi")
    x0 = np.array(legs["mechanical"][0]["density_unfiltered"])
    times = {name: [] for name in legs}
    for k in range(args.cycles + 1):
        for name, (sim, *_rest) in legs.items():
            sim["density_unfiltered"] = x0 * (1.0 - 1e-3 * k)
            ctx.sync()
            t0 = time.perf_counter()
            sim.run()
            np.asarray(sim.compute_totals("compliance", "density_unfiltered"))
            ctx.sync()
            if k > 0:
                times[name].append((time.perf_counter() - t0) * 1e3)
    sim, mesh, res, res_t = legs["thermoelastic"]
    dev, n, nc, nv = res.device(), res.n_dof, mesh.n_cell, mesh.n_vert
    rho, T = res.rho.vec, res.thermal.thermal.function.vec
    y, yc, yv, one = Vec(ctx, n), Vec(ctx, nc), Vec(ctx, nv), np.ones(1)

    def timed(body, reps=200):
        body()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            body()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    cond = res_t.device()
    launches = dict(
        thermal_N_us=timed(lambda: dev.thermal_apply(_lib.ELAST_SIMP, "N", 1, one, 1e-2, rho, T, y)),
        thermal_T_rho_us=timed(lambda: dev.thermal_apply(_lib.ELAST_SIMP, "T_rho", 1, one, 1e-2, rho, T, yc, x=res.u.vec)),
        thermal_T_temp_us=timed(lambda: dev.thermal_apply(_lib.ELAST_SIMP, "T_temp", 1, one, 1e-2, rho, 0.0, yv, x=res.u.vec)),
        conduction_assemble_us=timed(lambda: cond.assemble(_lib.ELAST_SIMP, 1.0, 1e-3, res_t.rho.vec, res_t._bc)))
    it, ie, im = res_t.last_info, res.last_info, legs["mechanical"][2].last_info
    out = dict(metric="topopt_cycle_thermoelastic", mesh=f"rect {args.nelx}x{args.nely}", n_dof=n, n_cell=nc, pc=args.pc,
               cycle_ms_thermoelastic=float(np.median(times["thermoelastic"])), cycle_ms_mechanical=float(np.median(times["mechanical"])),
               cycle_ms_thermoelastic_all=[float(v) for v in times["thermoelastic"]],
               cycle_ms_mechanical_all=[float(v) for v in times["mechanical"]],
               conduction_iterations=[it["state"]["iterations"], it["adjoint"]["iterations"]],
               conduction_solve_ms=[it["state"]["solve_ms"], it["adjoint"]["solve_ms"]],
               elasticity_iterations=[ie["state"]["iterations"], ie["adjoint"]["iterations"]],
               elasticity_solve_ms=[ie["state"]["solve_ms"], ie["adjoint"]["solve_ms"]],
               mechanical_iterations=[im["state"]["iterations"], im["adjoint"]["iterations"]],
               compliance_thermoelastic=float(sim["compliance"][0]), compliance_mechanical=float(legs["mechanical"][0]["compliance"][0]),
               **launches)
    spread = lambda v: float(np.percentile(v, 75) - np.percentile(v, 25))
    out.update(conduction_pc=res_t.preconditioner, cycle_ms_thermoelastic_iqr=spread(times["thermoelastic"]),
               cycle_ms_mechanical_iqr=spread(times["mechanical"]))
    if "thermoelastic_cond_jacobi" in legs:
        tj, ij = times["thermoelastic_cond_jacobi"], legs["thermoelastic_cond_jacobi"][3].last_info
        out.update(cycle_ms_thermoelastic_cond_jacobi=float(np.median(tj)), cycle_ms_thermoelastic_cond_jacobi_iqr=spread(tj),
                   cycle_ms_thermoelastic_cond_jacobi_all=[float(v) for v in tj],
                   conduction_jacobi_iterations=[ij["state"]["iterations"], ij["adjoint"]["iterations"]],
                   conduction_jacobi_solve_ms=[ij["state"]["solve_ms"], ij["adjoint"]["solve_ms"]])
        # the Galerkin diagonals of the lattice weights: ms per assembly, assembly + build against the assembly alone
        one_rhs = Vec(ctx, nv).fill(1.0)
        zz = Vec(ctx, nv)
        both = timed(lambda: (cond.assemble(_lib.ELAST_SIMP, 1.0, 1e-3, res_t.rho.vec, res_t._bc), cond.pc_apply(one_rhs, zz)), reps=50)
        cond.pc_apply(one_rhs, zz)
        apply_only = timed(lambda: cond.pc_apply(one_rhs, zz), reps=50)
        out.update(conduction_pc_build_us=both - apply_only - launches["conduction_assemble_us"], conduction_pc_apply_us=apply_only,
                   conduction_ms_per_iteration=[it[k]["solve_ms"] / max(it[k]["iterations"], 1) for k in ("state", "adjoint")],
                   conduction_jacobi_ms_per_iteration=[ij[k]["solve_ms"] / max(ij[k]["iterations"], 1) for k in ("state", "adjoint")])
    if args.counts:
        out["conduction_counts"] = conduction_counts(ctx)
    print(json.dumps(out))


def scipy_cycle(mesh, facets, t, x0, radius):
    """The same cycle with SciPy: KD-tree filter, element-by-element assembly, spsolve forward and adjoint."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from scipy.spatial import cKDTree
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import elasticity_ref as ref
    t0 = time.perf_counter()
    c = mesh.centroids()
    pairs = cKDTree(c).query_pairs(radius, output_type="ndarray")
    i = np.concatenate([pairs[:, 0], pairs[:, 1], np.arange(len(c))])
    j = np.concatenate([pairs[:, 1], pairs[:, 0], np.arange(len(c))])
    w = radius - np.linalg.norm(c[i] - c[j], axis=1)
    W = sp.csr_matrix((w, (i, j)), shape=(len(c),) * 2)
    W = sp.diags(1.0 / np.asarray(W.sum(axis=1)).ravel()) @ W
    rho = W @ x0
    d = mesh.tdim
    # the element matrix of every cell from the restatement (vectorised over cells by the shape of its formula)
    K0 = ref.element_matrices(mesh.x, mesh.conn)
    K = ref.stiffness(mesh.x, mesh.conn, rho, K0=K0)
    F = ref.traction_load(mesh.x, facets, t)
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    fixed = (fixed_v[:, None] * d + np.arange(d)).ravel()
    free = np.setdiff1d(np.arange(K.shape[0]), fixed)
    Kff = K[free][:, free].tocsc()
    u = np.zeros(K.shape[0])
    u[free] = spla.spsolve(Kff, F[free])
    lam = np.zeros(K.shape[0])
    lam[free] = spla.spsolve(Kff, F[free])
    g = W.T @ (-ref.compliance_gradient(mesh.x, mesh.conn, rho, u, lam, K0=K0))
    return (time.perf_counter() - t0) * 1e3, float(F @ u), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nelx", type=int, default=80)
    ap.add_argument("--nely", type=int, default=40)
    ap.add_argument("--n3", type=int, default=0)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--pc", choices=("jacobi", "multilevel"), default="jacobi", help="preconditioner of the PCG solves")
    ap.add_argument("--stress", action="store_true", help="add the p-norm von Mises stress output and its total derivative")
    ap.add_argument("--load-cases", type=int, default=1,
                    help="number of load cases, 1 to 8; more than 1: the tip load plus loads on further pieces of the boundary "
                         "(top, bottom and right edge in 2-D; the faces z = 1, z = 0, y = 1, y = 0 beyond x = 3/4 and pieces of "
                         "x = 1 in 3-D; `load_cases` in this script lists them), solved as one batched PCG and timed against "
                         "sequential single-column solves")
    ap.add_argument("--loss-factor", type=float, default=None,
                    help="with --harmonic N <= 4: the same frequencies through the damped forms with this structural loss factor as "
                         "well (complex arithmetic, one batched COCR per solve); adds the COCR iterations and ms beside the MINRES fields")
    ap.add_argument("--harmonic", type=int, default=0,
                    help="N harmonic responses of the tip load, 1 to 8, at frequencies below and between the first eigenfrequencies "
                         "of the start design: every solve one batched MINRES; prints the iterations per column and the cycle time")
    ap.add_argument("--filter", choices=("neighbours", "helmholtz"), default="neighbours",
                    help="the explicit neighbour list (default) or the Helmholtz PDE filter; single load case, no --harmonic")
    ap.add_argument("--radius-h", type=float, default=2.0, help="filter radius in units of the mean cell size (default 2)")
    ap.add_argument("--thermal", action="store_true",
                    help="the thermoelastic cycle (conduction state, thermal expansion load, two adjoint solves) alternated with the "
                         "mechanical-only cycle of the same build; 2-D, single load case")
    ap.add_argument("--counts", action="store_true",
                    help="with --thermal: the PCG iteration counts of the conduction solves at 80x40, 320x160 and 640x320, Jacobi and the "
                         "lattice preconditioner side by side")
    args = ap.parse_args()
    if args.thermal and (args.n3 or args.load_cases > 1 or args.harmonic or args.stress or args.filter != "neighbours"):
        ap.error("--thermal: the 2-D cantilever with one load case and the neighbour filter")
    if (args.filter != "neighbours" or args.radius_h != 2.0) and (args.load_cases > 1 or args.harmonic):
        ap.error("--filter / --radius-h: with the single load case only")
    if not args.no_scipy and (args.filter != "neighbours" or args.radius_h != 2.0):
        ap.error("the SciPy cycle restates the neighbour filter at 2 h: add --no-scipy")
    if not 1 <= args.load_cases <= 8:
        ap.error("--load-cases: 1 to 8")
    if args.loss_factor is not None and not (1 <= args.harmonic <= 4 and np.isfinite(args.loss_factor) and args.loss_factor >= 0.0):
        ap.error("--loss-factor: a finite value >= 0, with --harmonic 1 to 4")
    if not 0 <= args.harmonic <= 8 or (args.harmonic and (args.load_cases > 1 or args.stress)):
        ap.error("--harmonic: 1 to 8, without --load-cases and --stress")
    from femo_amd import _lib
    from femo_amd.engine import Context, Vec
    from femo_amd.fea import utils_hip
    if _lib.device_count() < 1:
        raise SystemExit("bench_topopt needs a HIP device")
    ctx = Context(0)
    utils_hip.set_context(ctx)
    if args.load_cases > 1:
        return main_multi(args, ctx)
    if args.harmonic:
        return main_harmonic(args, ctx)
    if args.thermal:
        return main_thermal(args, ctx)
    sim, mesh, res, facets, t, filter_build_ms, stress = build(args)
    x0 = np.array(sim["density_unfiltered"])
    times = []
    for k in range(args.cycles + 1):
        sim["density_unfiltered"] = x0 * (1.0 - 1e-3 * k)
        ctx.sync()
        t0 = time.perf_counter()
        sim.run()
        g = np.asarray(sim.compute_totals("compliance", "density_unfiltered"))
        if stress is not None:
            it_compliance_adjoint = res.last_info["adjoint"]["iterations"]
            if k == 0:                                              # scale of the aggregate, fixed from the first state
                cells = Vec(ctx, mesh.n_cell)
                stress.m = 1.0 / float(np.max(stress.device().von_mises(stress.u.vec, cells, stress.rho.vec, stress.q).get()))
                sim.run()
            gs = np.asarray(sim.compute_totals("stress", "density_unfiltered"))
        ctx.sync()
        if k > 0:
            times.append((time.perf_counter() - t0) * 1e3)
    dev = res.stiffness()
    xv, yv = Vec(ctx, dev.n_dof).set(np.random.default_rng(1).standard_normal(dev.n_dof)), Vec(ctx, dev.n_dof)
    spmv_ms = dev.bench_spmv(xv, yv, 50)
    info = res.last_info
    out = dict(metric="topopt_cycle", mesh=(f"cube n={args.n3}" if args.n3 else f"rect {args.nelx}x{args.nely}"),
               n_dof=dev.n_dof, n_cell=mesh.n_cell, cycle_ms=float(np.median(times)), cycle_ms_all=[float(v) for v in times],
               pcg_iterations_forward=info["state"]["iterations"], pcg_iterations_adjoint=info["adjoint"]["iterations"],
               spmv_ms=spmv_ms, spmv_bytes=dev.info["spmv_bytes"],
               spmv_share_of_8TBps=dev.info["spmv_bytes"] / (spmv_ms * 1e-3) / PEAK_BYTES_PER_S,
               filter_build_ms=filter_build_ms, compliance=float(sim["compliance"][0]), pc=args.pc, pc_levels=0,
               pc_build_ms=0.0,
               pcg_iteration_us=1e3 * info["state"]["solve_ms"] / max(info["state"]["iterations"], 1))
    if stress is not None:
        out.update(pcg_iterations_adjoint=it_compliance_adjoint, pcg_iterations_stress_adjoint=info["adjoint"]["iterations"],
                   stress=float(sim["stress"][0]), stress_m=stress.m, stress_p=stress.p, stress_q=stress.q,
                   stress_gradient_norm=float(np.linalg.norm(gs)))
    if args.pc == "multilevel":
        pci = dev.pc_info()
        out.update(pc_levels=pci["levels"], pc_build_ms=pci["build_ms"], pc_nodes=pci["nodes"], pc_lattice_bytes=pci["bytes"])
    out.update(filter=args.filter, filter_radius_h=args.radius_h)
    if not args.no_scipy:
        h = np.asarray(__import__("femo_amd.fea.mesh", fromlist=["meshSize"]).meshSize(mesh))
        sc_ms, sc_J, sc_g = scipy_cycle(mesh, facets, t, np.array(sim["density_unfiltered"]), 2.0 * (h.max() + h.min()) / 2)
        out.update(scipy_spsolve_cycle_ms=sc_ms, scipy_rel_diff_compliance=abs(sc_J - out["compliance"]) / abs(sc_J),
                   scipy_rel_diff_gradient=float(np.abs(sc_g - g).max() / np.abs(sc_g).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
