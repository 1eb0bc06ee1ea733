"""CPU tests of the aggregated von Mises stress of the SIMP elasticity: the NumPy restatement (tests/elast_stress_ref.py)
against closed forms, its own central differences and the total derivative of the filtered 16 x 8 cantilever, and the
Python surface of the two forms (what they refuse, the default alpha).  The GPU parity is tests/test_gpu_elast_stress.py."""
import types

import numpy as np
import pytest

import elast_stress_ref as sref
import elasticity_ref as ref

L_X, L_Y = 160.0, 80.0


def _meshes():
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh, createUnitSquareMesh
    return {"rect8x4": lambda: createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4),
            "square9j": lambda: createUnitSquareMesh(9, 0.25),
            "cube4j": lambda: createUnitCubeMesh(4, 0.2)}


MESHES = ["rect8x4", "square9j", "cube4j"]


@pytest.mark.parametrize("name", MESHES)
def test_closed_forms(name):
    mesh = _meshes()[name]()
    rho = np.full(mesh.n_cell, 0.7)
    m, p, q = 3.0, 8.0, 0.5
    for label, A, vm in sref.closed_forms(mesh.tdim):
        u = sref.linear_field(mesh.x, A)
        R = sref.pnorm_stress(mesh.x, mesh.conn, rho, u, m, p, q)
        exact = (m * 0.7 ** q * vm) ** p
        err = abs(R["value"] - exact) / exact
        print(f"{name} {label}: J = {R['value']:.16e}, exact {exact:.16e}, rel {err:.1e}")
        assert err <= 1e-13
        assert np.abs(R["vm"] - vm).max() <= 1e-13 * vm
        assert np.abs(R["field"] - 0.7 ** q * vm).max() <= 1e-13 * vm


@pytest.mark.parametrize("name", MESHES)
def test_zero_displacement(name):
    mesh = _meshes()[name]()
    rho = np.random.default_rng(1).uniform(1e-3, 1.0, mesh.n_cell)
    for p, q in sref.PQ_CASES:
        R = sref.pnorm_stress(mesh.x, mesh.conn, rho, np.zeros(mesh.x.size), 2.0, p, q)
        assert R["value"] == 0.0
        assert np.all(R["du"] == 0.0) and np.all(R["drho"] == 0.0)
        assert np.all(np.isfinite(R["du"])) and np.all(np.isfinite(R["drho"]))


@pytest.mark.parametrize("name", MESHES)
def test_zero_guard_is_exact_and_hides_no_non_finite_state(name):
    """The guard sigma_vm == 0 and the earlier sigma_vm > 0 give the same bits on finite inputs (random, all zero, and a
    state with some cells at exactly zero stress).  With one entry of the state at NaN, +Inf or -Inf the value is not
    finite and neither are the partials of the cells and vertices around it, where the earlier guard returned finite numbers."""
    mesh = _meshes()[name]()
    x, conn, d = mesh.x, mesh.conn, mesh.tdim
    u, rho, m = sref.random_inputs(x, conn, seed=5)
    some_zero = u.copy().reshape(-1, d)
    some_zero[np.unique(conn[: mesh.n_cell // 3])] = 0.0                # whole cells without displacement
    assert 0 < (sref.von_mises(x, conn, some_zero.ravel()) == 0.0).sum() < mesh.n_cell
    for state in (u, np.zeros_like(u), some_zero.ravel()):
        for p, q in sref.PQ_CASES:
            new = sref.pnorm_stress(x, conn, rho, state, m, p, q)
            old = sref.pnorm_stress(x, conn, rho, state, m, p, q, positive_guard=True)
            assert new["value"] == old["value"] and np.isfinite(new["value"])
            assert np.array_equal(new["du"], old["du"]) and np.array_equal(new["drho"], old["drho"])
    vertex = mesh.n_vert // 2
    touching = np.any(conn == vertex, axis=1)
    for bad in (np.nan, np.inf, -np.inf):
        state = u.copy()
        state[vertex * d + 1] = bad
        with np.errstate(all="ignore"):
            new = sref.pnorm_stress(x, conn, rho, state, m, 8.0, 0.5)
            old = sref.pnorm_stress(x, conn, rho, state, m, 8.0, 0.5, positive_guard=True)
        assert not np.isfinite(new["value"])
        assert not np.isfinite(new["drho"][touching]).any() and np.isfinite(new["drho"][~touching]).all()
        assert not np.isfinite(new["du"].reshape(-1, d)[np.unique(conn[touching])]).any()
        if bad != bad:
            assert np.isfinite(old["value"]) and np.isfinite(old["drho"]).all()      # what the earlier guard hid


def test_hydrostatic_is_finite():
    mesh = _meshes()["cube4j"]()
    rho = np.random.default_rng(2).uniform(1e-3, 1.0, mesh.n_cell)
    u = sref.linear_field(mesh.x, 0.01 * np.eye(3))
    for p, q in sref.PQ_CASES:
        with np.errstate(all="raise", under="ignore"):
            R = sref.pnorm_stress(mesh.x, mesh.conn, rho, u, 1.0, p, q)
        assert np.isfinite(R["value"]) and np.all(np.isfinite(R["du"])) and np.all(np.isfinite(R["drho"]))
        assert R["vm"].max() <= 1e-12                                   # rounding only: the deviator of a multiple of I


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p,q", sref.PQ_CASES)
def test_partials_against_central_differences(name, p, q):
    mesh = _meshes()[name]()
    x, conn = mesh.x, mesh.conn
    u, rho, m = sref.random_inputs(x, conn, seed=5)
    R = sref.pnorm_stress(x, conn, rho, u, m, p, q)
    J = lambda uu, rr: sref.pnorm_stress(x, conn, rr, uu, m, p, q, alpha=R["alpha"])["value"]
    rng = np.random.default_rng(6)
    worst = 0.0
    for _ in range(3):
        du = rng.standard_normal(u.size)
        fd = (J(u + 1e-5 * du, rho) - J(u - 1e-5 * du, rho)) / 2e-5
        worst = max(worst, abs(fd - R["du"] @ du) / abs(fd))
        if q != 0.0:
            dr = rng.standard_normal(rho.size) * rho                    # keeps rho > 0 at the step
            fd = (J(u, rho + 1e-6 * dr) - J(u, rho - 1e-6 * dr)) / 2e-6
            worst = max(worst, abs(fd - R["drho"] @ dr) / abs(fd))
    if q == 0.0:
        assert np.all(R["drho"] == 0.0)
    print(f"{name} p={p} q={q}: worst relative error against central differences {worst:.1e}")
    assert worst <= 1e-6


def cantilever_mesh(nelx=16, nely=8):
    """Mesh, traction facets and h_avg of run_topo_opt_cantilever_beam.py at nelx x nely."""
    from femo_amd.fea.mesh import createRectangleMesh, locate_entities_boundary, meshSize
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    marker = lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / nely + 3e-6, abs(x[0] - L_X) < 3e-6)
    facets = locate_entities_boundary(mesh, mesh.tdim - 1, marker)
    h = meshSize(mesh)
    return mesh, facets, (h.max() + h.min()) / 2


def test_total_derivative_of_the_filtered_cantilever():
    mesh, facets, h_avg = cantilever_mesh()
    P = sref.cantilever_problem(mesh, facets, h_avg)
    rng = np.random.default_rng(0)
    x0 = 1e-2 + 0.86 * rng.random(mesh.n_cell)
    p, q = 8.0, 0.5
    rho, _, u = sref.cantilever_state(P, x0)
    m = 1.0 / sref.cell_field(mesh.x, mesh.conn, u, rho, q).max()       # fixed once: not a function of the design
    T = sref.cantilever_total(P, x0, m, p, q)
    cos = sref.cosine(T["du"], T["F"])
    print(f"cos(dJ/du, F) = {cos:.2e}")
    assert abs(cos) < 0.1                                               # the adjoint right-hand side is not the load
    for k in range(3):
        dx = rng.standard_normal(mesh.n_cell)
        fd = (sref.cantilever_value(P, x0 + 1e-5 * dx, m, p, q) - sref.cantilever_value(P, x0 - 1e-5 * dx, m, p, q)) / 2e-5
        err = abs(fd - T["grad"] @ dx) / abs(fd)
        print(f"direction {k}: adjoint {T['grad'] @ dx:.12e}, central difference {fd:.12e}, rel {err:.1e}")
        assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ Python surface ----
def _spaces(mesh):
    from femo_amd.fea.function import FunctionSpace, VectorFunctionSpace
    fn = lambda V: types.SimpleNamespace(function_space=V)             # what the constructors read of a Function
    return fn(VectorFunctionSpace(mesh)), fn(FunctionSpace(mesh, ("DG", 0))), fn(FunctionSpace(mesh, ("CG", 1)))


@pytest.mark.parametrize("cls", ["ElasticityPnormStress", "ElasticityVonMises"])
def test_forms_refuse_what_the_residual_refuses(cls):
    from femo_amd.fea import elasticity as el
    form = getattr(el, cls)
    mesh, other = _meshes()["rect8x4"](), _meshes()["rect8x4"]()
    u, rho, scalar = _spaces(mesh)
    _, rho_other, _ = _spaces(other)
    for bad_u, bad_rho, word in ((scalar, rho, "VectorFunctionSpace"), (u, scalar, "DG0 density"), (u, rho_other, "DG0 density")):
        with pytest.raises(NotImplementedError, match=word):
            form(bad_u, bad_rho)
        with pytest.raises(NotImplementedError, match=word):           # the same refusal, the same error type
            el.ElasticityResidual(bad_u, bad_rho, np.zeros(2))
    f = form(u, rho)
    assert f.mesh is mesh and f.rank == 0 and f.functions() == (u, rho)


def test_defaults_and_parameter_checks():
    from femo_amd.fea import elasticity as el
    from femo_amd.fea import fea_hip
    mesh = _meshes()["square9j"]()
    u, rho, _ = _spaces(mesh)
    f = el.pnorm_stress(u, rho)
    assert isinstance(f, el.ElasticityPnormStress) and (f.m, f.p, f.q, f.E, f.nu) == (1.0, 8.0, 0.5, 1.0, 0.3)
    assert f.alpha == float(el.cell_volumes(mesh).sum())
    assert el.pnorm_stress(u, rho, alpha=2.5).alpha == 2.5
    for bad in (dict(m=0.0), dict(p=0.5), dict(q=-0.1), dict(alpha=0.0)):
        with pytest.raises(ValueError):
            el.pnorm_stress(u, rho, **bad)
    v = el.von_Mises_stress(u)
    assert isinstance(v, el.ElasticityVonMises) and v.q == 0.0 and v.functions() == (u,)
    assert el.von_Mises_stress(u, rho, q=0.5).functions() == (u, rho)
    with pytest.raises(ValueError):
        el.von_Mises_stress(u, q=0.5)                                   # q > 0 needs the density
    assert fea_hip.pnorm_stress is el.pnorm_stress and fea_hip.von_Mises_stress is el.von_Mises_stress
    from femo_amd import _lib
    assert {"femo_elast_pnorm_stress", "femo_elast_von_mises"} <= set(_lib.PROTOTYPES)
