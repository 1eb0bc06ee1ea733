"""CPU tests of the restatement of the harmonic response (tests/elast_harm_ref.py) and of the surface that needs no device.
The GPU parity is tests/test_gpu_elast_harm.py.

Set-up of both files: the meshes of tests/test_gpu_elast_eig.py, clamped on x = 0, rho = default_rng(7).uniform(0.3, 1), mass
density 1.3, traction (0, -1[, 0]) on the face x = max, SIMP with the linear mass law and RAMP with du_olhoff, and the shifts
sigma in {0, lambda_1 / 2, sqrt(lambda_1 lambda_2), sqrt(lambda_2 lambda_3), sqrt(lambda_5 lambda_6)} of the dense pencil.

Measured here (all five meshes, both laws, block-Jacobi of the unshifted K, rtol = 1e-12): the restated MINRES converges in
77 ... 355 iterations to 1.7e-12 of the largest entry of the direct solve or better; every relative gap of a shift to the
spectrum is at least 0.0069; c_l = F_l . u_l takes both signs and min |c_l| = 1.8 (square9j, SIMP); central differences of c_l
(step 1e-6) agree with the formula to 9e-7 or better."""
import functools

import numpy as np
import pytest

import elast_eig_ref as er
import elast_harm_ref as hr
import elast_pc_ref as pr
import elasticity_ref as ref

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    return pr.small_meshes()[name]()


@functools.lru_cache(maxsize=None)
def problem(name, method, law):
    return hr.problem(_mesh(name), method, law)


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ---------------------------------------------------------------------------------------------------------- MINRES ----
@pytest.mark.parametrize("method,law", hr.CASES)
@pytest.mark.parametrize("name", MESHES)
def test_minres_against_direct(name, method, law):
    """Every shift of the set-up: the restated loop converges, to the direct solve; the shifts keep clear of the spectrum,
    the matrix is indefinite from the third one on, and the dynamic compliance takes both signs."""
    P = problem(name, method, law)
    mesh, mask, K, M = P["mesh"], P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, mesh.tdim)
    b = np.where(mask == 1, 0.0, P["F"])
    its, errs, cs = [], [], []
    for k, sg in enumerate(P["shifts"]):
        out = hr.minres(hr.masked_shifted(K, M, sg, mask), b, pc, mask, rtol=1e-12)
        u = hr.direct(K, M, sg, P["F"], mask)
        assert out["converged"] == 1 and out["phibar"] <= 1e-12 * out["beta1"]
        assert np.all(out["x"][mask == 1] == 0.0)
        its.append(out["iterations"])
        errs.append(_maxrel(out["x"], u))
        cs.append(float(P["F"] @ u))
        gap = np.min(np.abs(P["lam"] - sg) / P["lam"])
        assert gap >= 0.005, (name, k, gap)
        assert (sg > P["lam"][0]) == (k >= 2)                          # indefinite from sqrt(lambda_1 lambda_2) on
    print(f"{name} {method}/{law}: {its} iterations, error {max(errs):.1e}, c = {np.round(cs, 3)}")
    assert max(errs) <= 1e-9                                          # the bound of the GPU test
    assert min(cs) < 0.0 < max(cs) and np.min(np.abs(cs)) >= 1.0


def test_minres_exits():
    P = problem("rect8x4", "SIMP", "linear")
    mask, K, M = P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, 2)
    S = hr.masked_shifted(K, M, P["shifts"][3], mask)
    b = np.where(mask == 1, 0.0, P["F"])
    zero = hr.minres(S, np.zeros_like(b), pc, mask)
    assert zero["converged"] == 1 and zero["iterations"] == 0 and not zero["x"].any()
    short = hr.minres(S, b, pc, mask, max_it=10)
    assert short["converged"] == 0 and short["iterations"] == 10
    bad = hr.minres(S, np.where(mask == 1, 0.0, np.nan), pc, mask)
    assert bad["converged"] == -1
    # the history is that of a shorter run: an iterate does not depend on what follows
    full = hr.minres(S, b, pc, mask, keep=True)
    assert np.array_equal(full["history"][9], short["x"])
    # phibar is the recurrence's estimate of sqrt(r . M^-1 r)
    r = b - S @ full["x"]
    true = np.sqrt(r @ pc(r))
    assert true <= 1e-9 * full["beta1"]
    # at sigma = 0 the matrix is positive definite and MINRES and the PCG restatement meet
    x_cg, it_cg, ok = pr.pcg(pr.masked_operator(K, mask), b, pc, mask, rtol=1e-12)
    out = hr.minres(hr.masked_shifted(K, M, 0.0, mask), b, pc, mask, rtol=1e-12)
    assert ok and _maxrel(out["x"], x_cg) <= 1e-9
    # a preconditioner that is not positive definite is reported, not iterated on
    assert hr.minres(S, b, lambda r: -pc(r), mask)["converged"] == -1


def test_pcg_breaks_down_above_the_first_resonance():
    """Why the loop is MINRES: p . A p <= 0 turns up in the PCG restatement on an indefinite shift."""
    import elast_multi_ref as mr
    P = problem("rect8x4", "SIMP", "linear")
    mask, K, M = P["mask"], P["K"], P["M"]
    S = hr.masked_shifted(K, M, P["shifts"][2], mask)
    (_, _, conv), = mr.pcg_multi(S, np.where(mask == 1, 0.0, P["F"])[None, :], hr.jacobi(K, mask, 2), mask, rtol=1e-12)
    assert not conv


# ------------------------------------------------------------------------------------------------------- gradients ----
@pytest.mark.parametrize("method,law", hr.CASES)
@pytest.mark.parametrize("name", ["rect8x4", "cube4j"])
def test_response_gradient_against_central_differences(name, method, law):
    """d c_l / d rho along a direction, every shift, step 1e-6."""
    P = problem(name, method, law)
    mesh, mask, rho = P["mesh"], P["mask"], P["rho"]
    L = len(P["shifts"])
    F = np.tile(P["F"], (L, 1))
    kw = dict(method=method, law=law, density=hr.DENSITY)
    U, c = hr.responses(mesh.x, mesh.conn, rho, mask, F, P["shifts"], **kw)
    G = hr.response_gradients(mesh.x, mesh.conn, rho, U, P["shifts"], **kw)
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    cp = hr.responses(mesh.x, mesh.conn, rho + h * d, mask, F, P["shifts"], **kw)[1]
    cm = hr.responses(mesh.x, mesh.conn, rho - h * d, mask, F, P["shifts"], **kw)[1]
    fd, an = (cp - cm) / (2 * h), G @ d
    err = np.abs(fd - an) / np.abs(an)
    print(f"{name} {method}/{law}: central differences of c_l {err.max():.1e}")
    assert err.max() <= 1e-5                                          # the project's bound for directional differences


@pytest.mark.parametrize("squared", [False, True])
def test_adjoint_total_against_central_differences(squared):
    P = problem("square9j", "RAMP", "du_olhoff")
    mesh, mask, rho = P["mesh"], P["mask"], P["rho"]
    L = len(P["shifts"])
    F = np.tile(P["F"], (L, 1))
    w = np.array([1.0, 0.5, 2.0, 1.5, 0.25])
    kw = dict(weights=w, squared=squared, method="RAMP", law="du_olhoff", density=hr.DENSITY)
    J, g, c, _ = hr.adjoint_total(mesh.x, mesh.conn, rho, mask, F, P["shifts"], **kw)
    assert J == pytest.approx(w @ (c * c if squared else np.abs(c)), rel=1e-14)
    d = np.random.default_rng(9).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    Jp = hr.adjoint_total(mesh.x, mesh.conn, rho + h * d, mask, F, P["shifts"], **kw)[0]
    Jm = hr.adjoint_total(mesh.x, mesh.conn, rho - h * d, mask, F, P["shifts"], **kw)[0]
    fd, an = (Jp - Jm) / (2 * h), float(g @ d)
    print(f"squared={squared}: dJ/drho . d = {an:.9e}, central differences {fd:.9e}")
    assert abs(fd - an) <= 1e-5 * abs(an)


@pytest.mark.parametrize("law", er.MASS_LAWS)
def test_mass_drho_matrix(law):
    """d(M u)/d rho against central differences of the assembled mass (exact for the linear law), cells on both branches of
    du_olhoff."""
    mesh = _mesh("cube4j")
    rho = np.random.default_rng(7).uniform(0.02, 1.0, mesh.n_cell)
    u = np.random.default_rng(3).standard_normal(3 * mesh.n_vert)
    D = hr.mass_drho_matrix(mesh.x, mesh.conn, rho, u, law, hr.DENSITY)
    x = np.random.default_rng(4).standard_normal(mesh.n_cell)
    h = 1e-7
    fd = (er.mass(mesh.x, mesh.conn, rho + h * x, law, hr.DENSITY) - er.mass(mesh.x, mesh.conn, rho - h * x, law, hr.DENSITY)) @ u / (2 * h)
    assert _maxrel(D @ x, fd) <= 1e-6


# ----------------------------------------------------------------------------------------------------- the surface ----
def test_entry_points_are_bound():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_mass_assemble", "femo_elast_dyn_apply_multi", "femo_elast_dyn_solve_multi",
                 "femo_elast_mass_drho_multi"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.PROTOTYPES["femo_elast_dyn_solve_multi"][1][-2:] == _lib.PROTOTYPES["femo_elast_solve_multi"][1][-2:]
    assert _lib.ABI_VERSION == 10 and lib.femo_abi_version() == 10    # a pure addition


def test_builders_are_exported():
    from femo_amd.fea import fea_hip
    from femo_amd.fea.elasticity import (DeviceElasticity, DynamicCompliance, HarmonicElasticityResidual,
                                         MultiLoadElasticityResidual, dynamic_compliance, pdeRes_harmonic)
    assert fea_hip.pdeRes_harmonic is pdeRes_harmonic and fea_hip.dynamic_compliance is dynamic_compliance
    assert issubclass(HarmonicElasticityResidual, MultiLoadElasticityResidual) and HarmonicElasticityResidual.is_symmetric
    assert DynamicCompliance.rank == 0
    for name in ("mass_assemble", "dyn_apply_multi", "dyn_solve_multi", "mass_drho_multi"):
        assert callable(getattr(DeviceElasticity, name))


def test_host_mass_matches_the_restatement():
    from femo_amd.fea.elasticity import _host_mass
    mesh = _mesh("cube4j")
    rho = np.random.default_rng(7).uniform(0.02, 1.0, mesh.n_cell)
    for law in er.MASS_LAWS:
        M = er.mass(mesh.x, mesh.conn, rho, law, hr.DENSITY)
        assert abs(_host_mass(mesh, rho, law, hr.DENSITY) - M).max() <= 1e-15 * abs(M).max()
