"""GPU tests of the host loop that the batched Krylov solves of the SIMP elasticity share (femo_elast_krylov_loop in
csrc/elast_solve.hip: the PCG of `solve_multi`, the MINRES of `dyn_solve_multi`, the COCR of `cdyn_solve_multi`): how often
the host polls the flags is not part of the result, and the iteration cap is exact where the burst between two polls does
not divide it.

rect8x4 (the smallest 2-D mesh of the elasticity tests: less than one wave of rows), clamped on x = 0, rho and the mass of
tests/elast_damp_ref.py's first case; block-Jacobi and multilevel.  Three columns of PCG with three different loads, three
MINRES columns with the end-face load at the shifts {0, lambda_1 / 2, sqrt(lambda_1 lambda_2)} -- the last above the first
eigenvalue, where K - sigma M is indefinite -- and two COCR columns at {lambda_1 / 2, sqrt(lambda_5 lambda_6)}.

The system has 80 free dofs, so under rtol alone every column runs into the finite termination of its recurrence within an
iteration or two of the others (74, 75, 74 of block-Jacobi PCG).  For columns that stop far apart, column l is scaled by
1e-4^l and the solves share one absolute level atol = 1e-2 rtol beta1 of column 0 (its `rhs_norm` from a first solve):
column 0 stops on rtol = 1e-10, column 1 on a reduction of 1e-8, column 2 on one of 1e-4.  Everything compared is compared
bit for bit: one column's launches and their order do not depend on when the host looks.
"""
import functools

import numpy as np
import pytest

import elast_damp_ref as dr
import elast_pc_ref as pr

pytestmark = pytest.mark.gpu

RTOL = 1e-10
KINDS = ("solve_multi", "dyn_solve_multi", "cdyn_solve_multi")
PCS = ("jacobi", "multilevel")


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def problem():
    """Built once, read only."""
    return dr.problem(pr.small_meshes()["rect8x4"](), *dr.CASES[0])


def _device(gpu, pc):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    P = problem()
    dev = DeviceElasticity(gpu, P["mesh"], 1.0, 0.3)
    dev.set_fixed(P["mask"])
    rv = Vec(gpu, P["mesh"].n_cell).set(P["rho"])
    dev.assemble(METHODS[P["method"]], rv)
    dev.mass_assemble(rv, density=P["density"], mass_law=P["law"])
    if pc == "multilevel":
        dev.pc_setup()
    return dev


def _solver(gpu, dev, kind, pc):
    """solve(**opts) -> (the solution's columns, iterations, converged and rhs_norm per column), each call from a zero
    guess into a vector of its own."""
    from femo_amd.engine import Vec
    P = problem()
    n, mask, lam = dev.n_dof, P["mask"], P["lam"]
    free = lambda v: np.where(mask == 1, 0.0, v)
    b = free(P["F"])
    if kind == "solve_multi":
        # the end-face load, a rough load and a smooth one (every dof pulled along +1)
        B = np.stack([b, 1e-4 * free(np.random.default_rng(5).standard_normal(n)), 1e-8 * free(np.ones(n))])
        call = lambda bv, xv, **o: dev.solve_multi(3, bv, xv, rtol=RTOL, pc=pc, **o)
    elif kind == "dyn_solve_multi":
        B = np.stack([b, 1e-4 * b, 1e-8 * b])
        shifts = np.array([0.0, 0.5 * lam[0], np.sqrt(lam[0] * lam[1])])
        assert (shifts > lam[0]).sum() == 1
        call = lambda bv, xv, **o: dev.dyn_solve_multi(3, shifts, bv, xv, rtol=RTOL, pc=pc, **o)
    else:
        B = np.zeros((4, n))
        B[0], B[2] = b, 1e-4 * b                                          # real right-hand sides
        sel = np.array([0, 3])
        call = lambda bv, xv, **o: dev.cdyn_solve_multi(2, P["shifts"][sel], P["ck"][sel], P["cm"][sel], bv, xv, rtol=RTOL, pc=pc, **o)

    def solve(**opts):
        xv = Vec(gpu, B.size)
        infos = call(Vec(gpu, B.size).set(B.ravel()), xv, **opts)
        return (np.array(xv.get()).reshape(len(B), n), [i.iterations for i in infos], [i.converged for i in infos],
                [i.rhs_norm for i in infos])
    return solve


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("kind", KINDS)
def test_poll_interval_is_not_part_of_the_result(gpu, kind, pc):
    solve = _solver(gpu, _device(gpu, pc), kind, pc)
    atol = 1e-2 * RTOL * solve()[3][0]
    X, its, conv, _ = solve(atol=atol)                                    # the default interval
    print(f"{kind} {pc}: iterations {its}")
    assert all(c == 1 for c in conv)
    assert len(set(its)) == len(its)                                      # every column stops at an iteration of its own
    for every in (1, 3):
        Xe, ite, conve, _ = solve(atol=atol, check_every=every)
        assert ite == its and conve == conv, (every, ite, conve)
        assert np.array_equal(Xe, X), every


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("kind", KINDS)
def test_cap_is_exact_when_the_burst_does_not_divide_it(gpu, kind, pc):
    solve = _solver(gpu, _device(gpu, pc), kind, pc)
    _, its, _, _ = solve()
    assert min(its) > 5                                                   # every column needs more than the cap
    X3, it3, conv3, _ = solve(max_it=5, check_every=3)                    # bursts of 3 and 2
    print(f"{kind} {pc}: uncapped {its}, capped {it3} {conv3}")
    assert it3 == [5] * len(its) and conv3 == [0] * len(its)
    X1, it1, conv1, _ = solve(max_it=5, check_every=1)
    assert it1 == it3 and conv1 == conv3
    assert np.array_equal(X3, X1)
