"""The stock Poisson BPX solve of tests/test_gpu_cond_pc.py::test_stock_solve_between_two_conduction_solves: the same system
in the test's own process, between two conduction solves with the weighted lattice preconditioner on the same mesh, and --
started as a program -- in a process that never made a conduction handle.

    python tests/cond_pc_stock.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, JITTER, RTOL = 40, 0.15, 1e-12


def stock_mesh():
    from femo_amd.fea.mesh import createUnitSquareMesh
    return createUnitSquareMesh(N, JITTER)


def stock_solve(ctx, mesh):
    """-lap u = f with random boundary values on `mesh`, `Mat.solve_cg(pc="bpx")`: (iterations, converged, solution)."""
    from femo_amd import engine as E
    dm = mesh.device(ctx)
    x = mesh.x
    bd = np.nonzero(np.isclose(x[:, 0], 0.0) | np.isclose(x[:, 0], 1.0) | np.isclose(x[:, 1], 0.0) |
                    np.isclose(x[:, 1], 1.0))[0].astype(np.int32)
    rng = np.random.default_rng(5)
    bc = E.DirichletSet(dm, bd, 0.3 * rng.standard_normal(len(bd)))
    f = 1.0 + rng.random(mesh.n_cell)
    A, b = E.Mat(dm), E.Vec(ctx, mesh.n_vert)
    E.assemble_system(dm, 0, None, E.Vec(ctx, mesh.n_vert).fill(0.0), E.Vec(ctx, mesh.n_cell).set(f), bc, None, A, b)
    u = E.Vec(ctx, mesh.n_vert)
    info = A.solve_cg(b, u, rtol=RTOL, pc="bpx")
    return int(info.iterations), int(info.converged), np.array(u.get())


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from femo_amd.engine import Context
    ctx = Context(0)
    it, conv, u = stock_solve(ctx, stock_mesh())
    np.savez(sys.argv[1], iterations=it, converged=conv, u=u)
