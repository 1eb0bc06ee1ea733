"""Host tests of tests/cond_pc_ref.py, the restatement of the lattice preconditioner of the penalised heat conduction solves:
the two derivations of the Galerkin diagonals agree, the operator is symmetric positive definite, PCG with it reaches the
direct solution, and its iteration counts behave as the preconditioner is meant to -- fewer than the stock lattice weights,
which need fewer than Jacobi, and no growth with the mesh at uniform density.  The counts are compared with one another,
computed here; none is a fixed number."""
import numpy as np
import pytest

import cond_pc_ref as cr
import elasticity_ref as ref
import thermal_ref as tr
from oracle import bpx_oracle as bo

HOST_MESHES = ["rect8x4", "square9j", "cube4j", "fan40x8"]


@pytest.mark.parametrize("name", HOST_MESHES)
def test_the_two_derivations_of_G_agree(name):
    case = cr.small_case(name)
    M, mesh = case["M"], case["mesh"]
    g, vol = cr.cell_gradients(mesh.x, mesh.conn)
    for c in (0, mesh.n_cell // 2, mesh.n_cell - 1):                      # the vectorised gradients are those of the reference
        g1, v1 = ref.grads_and_volume(mesh.x[mesh.conn[c]])
        assert np.abs(g[c] - g1).max() <= 1e-13 * np.abs(g1).max() and abs(vol[c] - v1) <= 1e-14 * v1
    assert M.levels >= 1
    for l in range(M.levels):
        triple = cr.galerkin_diagonal(M, mesh.x, M.A, l)
        cells = M.G[l]
        err = np.abs(triple - cells).max() / np.abs(cells).max()
        print(f"{name} level {l}: {len(cells)} nodes, {int((cells == 0).sum())} untouched, the two derivations differ by {err:.1e}")
        assert err <= 1e-12
        # a kept node has a free vertex under its hat, so its diagonal is positive and its weight finite
        keep = M.stock[l] != 0.0
        assert np.all(cells[keep] > 0.0) and np.all(np.isfinite(M.coef[l]))
        assert np.all(M.coef[l][~keep] == 0.0)


def test_the_diagonals_do_not_depend_on_the_sink_being_eliminated_or_masked():
    """Pt_l has zero rows on the pinned vertices, so the eliminated operator and the plain one give the same G."""
    case = cr.small_case("square9j")
    M, mesh = case["M"], case["mesh"]
    for l in range(M.levels):
        a, b = cr.galerkin_diagonal(M, mesh.x, M.A, l), cr.galerkin_diagonal(M, mesh.x, case["K"], l)
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()


def test_dense_operator_is_symmetric_positive_definite():
    M = cr.small_case("rect8x4")["M"]
    D = M.matrix()
    assert np.abs(D - D.T).max() <= 1e-13 * np.abs(D).max()
    w = np.linalg.eigvalsh(0.5 * (D + D.T))
    print(f"rect8x4: eigenvalues of M^-1 in [{w.min():.3e}, {w.max():.3e}]")
    assert w.min() > 0.0


@pytest.mark.parametrize("name", tr.MESHES)
def test_pcg_reaches_the_direct_solution(name):
    case = cr.small_case(name)
    M = case["M"]
    want = tr.solve_lifted(case["K"], case["Q"], case["sink"])
    x, it = bo.pcg(M.A, case["b"], M, rtol=1e-13)
    err = np.abs(x - want).max() / np.abs(want).max()
    print(f"{name}: {it} iterations, {err:.1e} from the direct solution")
    assert err <= 1e-10


def test_iteration_counts():
    n = {(nx, kind, which): cr.count_iterations(nx, nx // 2, kind, which)
         for nx, kind, which in [(80, "truss", "weighted"), (80, "truss", "stock"), (80, "truss", "jacobi"),
                                 (80, "uniform", "weighted"), (160, "uniform", "weighted")]}
    print(f"80x40 truss: weighted {n[80, 'truss', 'weighted']}, stock {n[80, 'truss', 'stock']}, Jacobi {n[80, 'truss', 'jacobi']}; "
          f"uniform weighted: 80x40 {n[80, 'uniform', 'weighted']}, 160x80 {n[160, 'uniform', 'weighted']}")
    assert n[80, "truss", "weighted"] < n[80, "truss", "stock"] < n[80, "truss", "jacobi"]
    # mesh independence at uniform density: the Jacobi count doubles from 80x40 to 160x80
    assert n[160, "uniform", "weighted"] <= 1.25 * n[80, "uniform", "weighted"]
    # every column reaches the direct solution
    case = cr.count_case(80, 40, "truss")
    x, _ = bo.pcg(case["M"].A, case["b"], case["M"], rtol=cr.COUNT_RTOL)
    want = tr.solve_lifted(case["K"], case["Q"], case["sink"])
    assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max()
