"""CPU tests of the multi-load restatement (tests/elast_multi_ref.py) and of the Python surface that needs no device:
the batched PCG with frozen columns against the column-wise one, the weighted-compliance gradient against central
differences, and LoadCaseSpace.  The GPU parity is tests/test_gpu_elast_multi.py."""
import numpy as np
import pytest

import elast_multi_ref as mr
import elast_pc_ref as pr
from elast_pc_ref import clamped_face
from elast_pc_ref import small_meshes as _meshes
from elast_multi_ref import cantilever_loads, right_hand_sides


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_pcg_multi_equals_columnwise(name, pc):
    mesh = _meshes()[name]()
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask)
    precond = M.jacobi if pc == "jacobi" else M.apply
    B = right_hand_sides(mesh, mask)
    out = mr.pcg_multi(M.A, B, precond, mask)
    counts = []
    for l, (x, it, ok) in enumerate(out):
        xs, its, oks = pr.pcg(M.A, B[l], precond, mask)
        assert (it, ok) == (its, oks)
        assert np.array_equal(x, xs)
        counts.append(it)
    print(f"{name} {pc}: iterations per column {counts}")
    assert counts[2] == 0 and np.all(out[2][0] == 0.0)                  # the zero column is finished at the start
    assert all(ok for _, _, ok in out)


def test_reference_gradient_against_central_differences():
    """8 x 4 rectangle, 3 loads, weights (1, 0.5, 2); step 1e-5 and tolerance 1e-6 as
    test_elast_stress_host.test_total_derivative_of_the_filtered_cantilever."""
    from femo_amd.fea.mesh import createRectangleMesh, meshSize
    mesh = createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4)
    facets, tractions = cantilever_loads(mesh, 2.0, 1.0, 4)
    assert all(len(f) > 0 for f in facets)
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    w = (1.0, 0.5, 2.0)
    rng = np.random.default_rng(0)
    x0 = 1e-2 + 0.86 * rng.random(mesh.n_cell)
    R = mr.reference_cycle_multi(mesh, facets, tractions, w, h_avg, x0)
    J = lambda x: mr.reference_cycle_multi(mesh, facets, tractions, w, h_avg, x)["J"]
    for k in range(3):
        dx = rng.standard_normal(mesh.n_cell)
        fd = (J(x0 + 1e-5 * dx) - J(x0 - 1e-5 * dx)) / 2e-5
        err = abs(fd - R["grad"] @ dx) / abs(fd)
        print(f"direction {k}: adjoint {R['grad'] @ dx:.12e}, central difference {fd:.12e}, rel {err:.1e}")
        assert err <= 1e-6


def test_load_case_space():
    from femo_amd import _lib
    from femo_amd.fea.fea_hip import compliance_multiload, pdeRes_multiload  # noqa: F401  exported beside pdeRes
    from femo_amd.fea.function import FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _meshes()["rect8x4"]()
    V = VectorFunctionSpace(mesh)
    S = LoadCaseSpace(V, 3)
    assert S.dim == 3 * V.dim and S.base is V and S.n_cases == 3
    assert S.column(1) == slice(V.dim, 2 * V.dim)
    assert S.tabulate_dof_coordinates() is V.tabulate_dof_coordinates()
    assert S == LoadCaseSpace(V, 3) and S != LoadCaseSpace(V, 2)
    with pytest.raises(IndexError):
        S.column(3)
    for bad in (0, _lib.ELAST_MAX_COLS + 1):
        with pytest.raises(ValueError):
            LoadCaseSpace(V, bad)
    with pytest.raises(NotImplementedError):
        LoadCaseSpace(FunctionSpace(mesh, ("CG", 1)), 2)
