"""CPU tests of the thermoelastic restatement (tests/thermal_ref.py) and of the Python surface that needs no device: the
free-expansion identities of the thermal load, the transposes, the reduced gradient of the restated thermoelastic cycle
against central differences, the constructor arguments and the new entry points.  The GPU parity is
tests/test_gpu_elast_thermal.py, tests/test_gpu_conduction.py and tests/test_gpu_thermoelastic_cycle.py."""
import inspect
import types

import numpy as np
import pytest

import elasticity_ref as ref
import thermal_ref as tr
from elast_pc_ref import small_meshes as _meshes

ALPHA, THETA = 0.7, 1.3


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_free_expansion(name, method):
    """Uniform theta, any density: u = e x makes the cell stress zero cell by cell, so K(rho) u - F_th(rho, theta) = 0 at
    every vertex, the boundary included."""
    mesh = _meshes()[name]()
    rho = np.random.default_rng(3).uniform(0.05, 1.0, mesh.n_cell)
    F = tr.thermal_load(mesh.x, mesh.conn, rho, THETA, ALPHA, method)
    u = tr.free_expansion(mesh.x, THETA, ALPHA)
    res = ref.stiffness(mesh.x, mesh.conn, rho, method) @ u - F
    err = np.abs(res).max() / np.abs(F).max()
    print(f"{name} {method}: |K u - F_th| / max |F_th| = {err:.1e} (max |F_th| = {np.abs(F).max():.2f})")
    assert err <= 1e-13


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_uniform_density_and_temperature(name):
    """Uniform rho and theta: the load is the boundary term alone -- zero at interior vertices, non-zero on the boundary."""
    mesh = _meshes()[name]()
    d = mesh.tdim
    F = tr.thermal_load(mesh.x, mesh.conn, np.full(mesh.n_cell, 0.6), THETA, ALPHA).reshape(-1, d)
    x = mesh.x
    interior = np.all((x > x.min(axis=0) + 1e-9) & (x < x.max(axis=0) - 1e-9), axis=1)
    assert 0 < interior.sum() < mesh.n_vert
    err = np.abs(F[interior]).max() / np.abs(F).max()
    print(f"{name}: interior load {err:.1e} of the largest entry")
    assert err <= 1e-13
    assert np.all(np.abs(F[~interior]).max(axis=1) > 1e-3 * np.abs(F).max())


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_transpose_identities(name):
    mesh = _meshes()[name]()
    d = mesh.tdim
    rng = np.random.default_rng(5)
    rho, th = rng.uniform(0.05, 1.0, mesh.n_cell), rng.standard_normal(mesh.n_vert)
    w, dT, xv = rng.standard_normal(mesh.n_cell), rng.standard_normal(mesh.n_vert), rng.standard_normal(d * mesh.n_vert)
    for method in ("SIMP", "RAMP"):
        Nw = tr.thermal_H(mesh.x, mesh.conn, ref.penal_d(rho, method) * w, th, ALPHA)
        a1, a2 = xv @ Nw, w @ tr.thermal_T_rho(mesh.x, mesh.conn, rho, th, xv, ALPHA, method)
        assert abs(a1 - a2) <= 1e-13 * np.linalg.norm(xv) * np.linalg.norm(Nw)
        NT = tr.thermal_H(mesh.x, mesh.conn, ref.penal(rho, method), dT, ALPHA)
        b1, b2 = xv @ NT, dT @ tr.thermal_T_temp(mesh.x, mesh.conn, rho, xv, ALPHA, method)
        assert abs(b1 - b2) <= 1e-13 * np.linalg.norm(xv) * np.linalg.norm(NT)
        T = rng.standard_normal(mesh.n_vert)
        Dw = tr.conduction_drho(mesh.x, mesh.conn, rho, T, w, 1.0, 1e-3, method)
        c1, c2 = dT @ Dw, w @ tr.conduction_drho_T(mesh.x, mesh.conn, rho, T, dT, 1.0, 1e-3, method)
        assert abs(c1 - c2) <= 1e-13 * np.linalg.norm(dT) * np.linalg.norm(Dw)


def test_conduction_matrix_and_its_derivative():
    """K_theta(rho) T is linear in k(rho): its derivative along dr is conduction_drho, and k = 1 gives the P1 Laplacian,
    whose rows sum to zero and which a linear field solves."""
    mesh = _meshes()["square9j"]()
    rng = np.random.default_rng(2)
    rho, T, dr = rng.uniform(0.05, 1.0, mesh.n_cell), rng.standard_normal(mesh.n_vert), rng.standard_normal(mesh.n_cell)
    K = lambda r: tr.conduction_matrix(mesh.x, mesh.conn, tr.conductivity(r, 1.0, 1e-3, "RAMP"))
    fd = (K(rho + 1e-6 * dr) @ T - K(rho - 1e-6 * dr) @ T) / 2e-6
    D = tr.conduction_drho(mesh.x, mesh.conn, rho, T, dr, 1.0, 1e-3, "RAMP")
    assert np.abs(fd - D).max() <= 1e-8 * np.abs(D).max()
    L = tr.conduction_matrix(mesh.x, mesh.conn, np.ones(mesh.n_cell))
    assert np.abs(L @ np.ones(mesh.n_vert)).max() <= 1e-13 * np.abs(L.diagonal()).max()
    x = mesh.x
    on = np.nonzero(np.isclose(x[:, 0], 0.0) | np.isclose(x[:, 0], 1.0))[0]
    g = 2.0 + 3.0 * x[:, 0]
    Tl = tr.solve_lifted(K(np.full(mesh.n_cell, 0.5)), np.zeros(mesh.n_vert), on, g)
    assert np.abs(Tl - g).max() <= 1e-12


def test_cycle_parts_are_of_the_same_order():
    mesh, facets, h_avg, sink = tr.cycle_case()
    x0 = np.random.default_rng(0).random(mesh.n_cell) * 0.86
    R = tr.reference_cycle_thermoelastic(mesh, facets, tr.TRACTION, h_avg, x0, tr.ALPHA, tr.SOURCE, sink)
    ratio = np.abs(R["u_th"]).max() / np.abs(R["u_mech"]).max()
    print(f"max |u_thermal| / max |u_mechanical| = {ratio:.2f}")
    assert 0.2 <= ratio <= 5.0


@pytest.mark.parametrize("objective", ["compliance", "displacement"])
def test_reference_gradient_against_central_differences(objective):
    """16 x 8 rectangle, step 1e-4, three random directions, 1e-6: the bound check_totals gets in test_gpu_elast_body.py."""
    mesh, facets, h_avg, sink = tr.cycle_case()
    rng = np.random.default_rng(0)
    x0 = 1e-2 + 0.86 * rng.random(mesh.n_cell)
    ell = None
    if objective == "displacement":                                  # the mean displacement of the tip facets along -y
        ell = ref.traction_load(mesh.x, facets, (0.0, -1.0))
        ell /= -ell.reshape(-1, 2)[:, 1].sum()
    cycle = lambda x: tr.reference_cycle_thermoelastic(mesh, facets, tr.TRACTION, h_avg, x, tr.ALPHA, tr.SOURCE, sink,
                                                       objective=objective, ell=ell)
    R = cycle(x0)
    for k in range(3):
        dx = rng.standard_normal(mesh.n_cell)
        fd = (cycle(x0 + 1e-4 * dx)["J"] - cycle(x0 - 1e-4 * dx)["J"]) / 2e-4
        err = abs(fd - R["grad"] @ dx) / abs(fd)
        print(f"{objective} direction {k}: adjoint {R['grad'] @ dx:.12e}, central difference {fd:.12e}, rel {err:.1e}")
        assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ the Python surface ----
def _spaces(L=None):
    from femo_amd.fea.function import FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    fn = lambda V: types.SimpleNamespace(function_space=V)              # what the constructors read of a Function
    mesh = _meshes()["rect8x4"]()
    V = VectorFunctionSpace(mesh)
    return mesh, V, fn(V if L is None else LoadCaseSpace(V, L)), fn(FunctionSpace(mesh, ("DG", 0)))


def test_thermal_expansion_arguments():
    from femo_amd.fea.elasticity import (Compliance, DampedHarmonicElasticityResidual, ElasticityResidual,
                                         HarmonicElasticityResidual, MultiLoadCompliance, MultiLoadElasticityResidual,
                                         ThermalExpansion, TransientElasticityResidual)
    mesh, V, u, rho = _spaces()
    th = ThermalExpansion(1e-2, 3.0, T_ref=1.0)
    res = ElasticityResidual(u, rho, None, thermal=th)                # a thermal load alone is a load
    assert res.thermal is not None and res.body is None and res.functions() == (u, rho)
    assert np.array_equal(res.thermal.scales, [1.0])
    assert ElasticityResidual(u, rho, (0.0, -0.25)).thermal is None
    J = Compliance(u, (0.0, -0.25), thermal=th, rho=rho)
    assert J.functions() == (u, rho) and J.body is None
    with pytest.raises(ValueError, match="rho"):
        Compliance(u, (0.0, -0.25), thermal=th)
    for bad in (dict(alpha=np.nan), dict(alpha=np.inf), dict(T_ref=np.nan), dict(scales=[1.0, np.inf])):
        with pytest.raises(ValueError, match="finite"):
            ThermalExpansion(**{**dict(alpha=1e-2, temperature=1.0), **bad})
    with pytest.raises(ValueError, match="thermal scales"):
        ElasticityResidual(u, rho, None, thermal=ThermalExpansion(1e-2, 3.0, scales=[1.0, 2.0]))
    with pytest.raises(TypeError):
        ElasticityResidual(u, rho, None, thermal=1e-2)

    mesh, V, u3, rho = _spaces(3)
    ts = [None, (0.0, -0.25), (0.25, 0.0)]
    th3 = ThermalExpansion(1e-2, 3.0, scales=[1.0, 0.0, -2.0])
    res = MultiLoadElasticityResidual(u3, rho, ts, thermal=th3)
    assert np.array_equal(res.thermal.scales, [1.0, 0.0, -2.0])
    assert np.array_equal(MultiLoadElasticityResidual(u3, rho, ts, thermal=th).thermal.scales, np.ones(3))
    J = MultiLoadCompliance(u3, ts, weights=(1.0, 0.5, 2.0), thermal=th3, rho=rho)
    assert np.array_equal(J.thermal.scales, [1.0, 0.0, -4.0])        # w_l s_l
    with pytest.raises(ValueError, match="thermal scales"):
        MultiLoadElasticityResidual(u3, rho, ts, thermal=ThermalExpansion(1e-2, 3.0, scales=[1.0, 2.0]))
    # the dynamic forms refuse it with the wording they use for body forces
    for make in (lambda: HarmonicElasticityResidual(u3, rho, ts[1:] + ts[1:2], omegas=[0.1] * 3, thermal=th),
                 lambda: DampedHarmonicElasticityResidual(u3, rho, ts[1:] + ts[1:2], omegas=[0.1] * 3, thermal=th),
                 lambda: TransientElasticityResidual(u, rho, (0.0, -0.25), signal=[0.0, 1.0], dt=0.1, thermal=th)):
        with pytest.raises(NotImplementedError, match="thermal loads are out of scope"):
            make()


def test_builders():
    from femo_amd.fea import elasticity, fea_hip
    for fn in (elasticity.pdeRes, fea_hip.pdeRes_multiload, elasticity.compliance, fea_hip.compliance_multiload):
        assert inspect.signature(fn).parameters["thermal"].default is None
    assert fea_hip.ThermalExpansion is elasticity.ThermalExpansion
    mesh, V, u, rho = _spaces()
    th = elasticity.ThermalExpansion(1e-2, 3.0)
    assert elasticity.pdeRes(u, None, rho, None, thermal=th).thermal is not None
    assert elasticity.compliance(u, None, thermal=th, rho_e=rho).functions() == (u, rho)
    for name in ("pdeRes_conduction", "thermal_compliance", "ConductionResidual", "ThermalCompliance", "DeviceConduction"):
        assert hasattr(fea_hip, name), name


def test_entry_points():
    from femo_amd import _lib
    names = ["femo_elast_thermal_apply", "femo_cond_create", "femo_cond_destroy", "femo_cond_assemble", "femo_cond_apply",
             "femo_cond_solve", "femo_cond_drho", "femo_cond_export_csr"]
    lib = _lib.load()
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert len(_lib.PROTOTYPES["femo_elast_thermal_apply"][1]) == 16
    assert _lib.ABI_VERSION == 10                                    # a pure addition
