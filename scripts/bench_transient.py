"""Transient response of the SIMP elasticity: ms per Newmark step and PCG iterations per step (csrc/elast_transient.hip).

    python scripts/bench_transient.py                    # the 640 x 320 cantilever, then the n = 48 cube
    python scripts/bench_transient.py --nelx 80 --nely 40 --n3 0

Per mesh: a fixed density (default_rng(0).uniform(0.3, 1)), clamped on x = 0, the traction (0, -1[, 0]) on the face
x = x_max, N = 64 steps of the average-acceleration rule with dt = T_1 / 20, T_1 from `ElasticityEigenvalues`; the signal is
a half-sine pulse over the first 16 steps.  The four legs -- block-Jacobi and multilevel, each with the extrapolated first
guess 2 u_n - u_{n-1} and from zero -- are ALTERNATED in one process: a warm-up of all four, then ``--repeats`` rounds of
the four.  One JSON line per mesh: per leg the median ms per step with its minimum and maximum over the rounds (wall time of
the whole march, which includes the PCG's flag polls) and the mean, minimum and maximum PCG iterations per step."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_mesh(ctx, mesh, n_steps, repeats, rtol):
    from femo_amd.fea.elasticity import ElasticityEigenvalues
    from femo_amd.fea.fea_hip import (Constant, Function, FunctionSpace, Measure, TimeHistorySpace, VectorFunctionSpace,
                                      dirichletbc, locate_dofs_geometrical, locate_entities_boundary, meshtags,
                                      pdeRes_transient)
    d = mesh.tdim
    xmax = mesh.x[:, 0].max()
    facets = locate_entities_boundary(mesh, d - 1, lambda x: np.isclose(x[0], xmax))
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    t = np.zeros(d)
    t[1] = -1.0
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(TimeHistorySpace(V, n_steps))
    rho.vector[:] = np.random.default_rng(0).uniform(0.3, 1.0, mesh.n_cell)
    clamped = locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))
    ubc = Function(V)
    ubc.vector.set(0.0)
    bcs = [dirichletbc(ubc, clamped)]
    eig = ElasticityEigenvalues(rho, V, [dirichletbc(0.0, clamped, V)], 1, block=4, preconditioner="multilevel", rtol=1e-6)
    lam1 = float(eig.eigenvalues()[0])
    dt = 2.0 * np.pi / np.sqrt(lam1) / 20.0
    g = np.zeros(n_steps + 1)
    g[:17] = np.sin(np.pi * np.arange(17) / 16.0)
    legs = [(pc, ex) for pc in ("jacobi", "multilevel") for ex in (True, False)]
    res = pdeRes_transient(u, None, rho, Constant(mesh, t), ds, signal=g, dt=dt, preconditioner="multilevel")
    res.rtol = rtol                                        # one form, one K, one M and one lattice plan for all four legs
    times = {leg: [] for leg in legs}
    last = {}
    for rnd in range(repeats + 1):                          # round 0 warms all four legs up
        for pc, ex in legs:
            res.preconditioner, res.extrapolate = pc, ex
            ctx.sync()
            t0 = time.perf_counter()
            res.solve_state(u, bcs)
            ctx.sync()
            if rnd:
                times[(pc, ex)].append((time.perf_counter() - t0) * 1e3 / n_steps)
            last[(pc, ex)] = res.last_info["state"]
    out = dict(mesh=f"{mesh.n_vert} vertices, {d}-D", n_dof=int(V.dim), n_steps=n_steps, lambda_1=lam1, dt=dt, rtol=rtol,
               repeats=repeats, legs={})
    for pc, ex in legs:
        ts = np.array(times[(pc, ex)])
        its = last[(pc, ex)]["iterations"]
        out["legs"][f"{pc}, {'extrapolated' if ex else 'zero'} guess"] = dict(
            ms_per_step=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
            iterations_per_step=float(np.mean(its)), iterations_min=int(min(its)), iterations_max=int(max(its)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nelx", type=int, default=640)
    ap.add_argument("--nely", type=int, default=320)
    ap.add_argument("--n3", type=int, default=48)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-8, help="PCG tolerance of a step, relative to its first residual")
    args = ap.parse_args()
    from femo_amd.engine import Context
    from femo_amd.fea import utils_hip
    from femo_amd.fea.fea_hip import createRectangleMesh, createUnitCubeMesh
    ctx = Context(0)
    utils_hip.set_context(ctx)
    if args.nelx:
        mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), args.nelx, args.nely)
        print(json.dumps(run_mesh(ctx, mesh, args.steps, args.repeats, args.rtol)), flush=True)
    if args.n3:
        print(json.dumps(run_mesh(ctx, createUnitCubeMesh(args.n3), args.steps, args.repeats, args.rtol)), flush=True)


if __name__ == "__main__":
    main()
