"""CPU tests of the restatement of the damped harmonic response (tests/elast_damp_ref.py) and of the surface that needs no
device.  The GPU parity is tests/test_gpu_elast_damp.py.

Set-up of both files: that of tests/test_elast_harm_host.py with the shifts {lambda_1 / 2, lambda_1, sqrt(lambda_1 lambda_2),
sqrt(lambda_5 lambda_6)} of the dense pencil -- the second sits exactly on a resonance -- and the two damping sets (eta, alpha,
beta) = (0.05, 0, 0) with SIMP and the linear mass law, (0, 0.02, 0.02) with RAMP and du_olhoff.

Bounds: the restated COCR against the complex sparse LU 1e-9 of the largest entry and a backward error of 1e-12 (block-Jacobi
of the unshifted K, rtol = 1e-12); directional central differences (step 1e-6) 1e-5, the project's bound for them."""
import functools

import numpy as np
import pytest

import elast_damp_ref as dr
import elast_harm_ref as hr
import elast_pc_ref as pr

MESHES = ["rect8x4", "square9j", "cube4j"]
WEIGHTS = (1.0, 0.5, 2.0, 1.5)


@functools.lru_cache(maxsize=None)
def problem(name, case):
    return dr.problem(pr.small_meshes()[name](), *dr.CASES[case])


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("case", range(len(dr.CASES)))
@pytest.mark.parametrize("name", MESHES)
def test_cocr_against_direct(name, case):
    """Every shift, the resonant one included: the restated loop converges to the complex LU."""
    P = problem(name, case)
    mesh, mask, K, M = P["mesh"], P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, mesh.tdim)
    b = np.where(mask == 1, 0.0, P["F"])
    its, errs, etas = [], [], []
    for sg, ck, cm in zip(P["shifts"], P["ck"], P["cm"]):
        Zm = dr.masked_Z(K, M, sg, ck, cm, mask)
        out = dr.cocr(Zm, b, pc, mask, rtol=1e-12)
        u = dr.direct(K, M, sg, ck, cm, P["F"], mask)
        assert out["converged"] == 1 and out["res"] <= 1e-12 * out["beta1"]
        assert np.all(out["x"][mask == 1] == 0.0)
        its.append(out["iterations"])
        errs.append(_maxrel(out["x"], u))
        etas.append(dr.backward_error(Zm, out["x"], b))
    print(f"{name} {dr.CASES[case]}: {its} iterations, error {max(errs):.1e}, backward error {max(etas):.1e}")
    assert P["shifts"][dr.RESONANT] == P["lam"][0]
    assert max(errs) <= 1e-9
    assert max(etas) <= 1e-12


def test_cocr_exits():
    P = problem("rect8x4", 0)
    mask, K, M = P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, 2)
    Zm = dr.masked_Z(K, M, P["shifts"][2], P["ck"][2], P["cm"][2], mask)
    b = np.where(mask == 1, 0.0, P["F"])
    zero = dr.cocr(Zm, np.zeros_like(b), pc, mask)
    assert zero["converged"] == 1 and zero["iterations"] == 0 and not zero["x"].any()
    short = dr.cocr(Zm, b, pc, mask, max_it=10)
    assert short["converged"] == 0 and short["iterations"] == 10 and short["res"] > 1e-12 * short["beta1"]
    bad = dr.cocr(Zm, np.where(mask == 1, 0.0, np.nan), pc, mask)
    assert bad["converged"] == -1 and bad["iterations"] == 0
    # a zero denominator of alpha: a "preconditioner" that returns zero after the first residual gives q^T M^-1 q = 0
    calls = []
    dead = dr.cocr(Zm, b, lambda r: pc(r) if len(calls) < 2 and not calls.append(1) else np.zeros_like(r), mask)
    assert dead["converged"] == -1 and dead["iterations"] == 0
    # without damping and below the first resonance Z is real SPD, and COCR and the PCG restatement meet
    x_cg, _, ok = pr.pcg(pr.masked_operator(K, mask), b, pc, mask, rtol=1e-12)
    out = dr.cocr(dr.masked_Z(K, M, 0.0, 0.0, 0.0, mask), b, pc, mask, rtol=1e-12)
    assert ok and out["converged"] == 1 and not out["x"].imag.any() and _maxrel(out["x"].real, x_cg) <= 1e-9
    # conj(Z) on a real right-hand side gives the conjugate solution
    cj = dr.cocr(Zm.conj(), b, pc, mask, rtol=1e-12)
    full = dr.cocr(Zm, b, pc, mask, rtol=1e-12)
    assert _maxrel(cj["x"], full["x"].conj()) <= 1e-9


def test_undamped_minres_fails_at_a_resonance_where_the_damped_solve_converges():
    P = problem("rect8x4", 0)
    mask, K, M = P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, 2)
    b = np.where(mask == 1, 0.0, P["F"])
    k = dr.RESONANT
    und = hr.minres(hr.masked_shifted(K, M, P["shifts"][k], mask), b, pc, mask, rtol=1e-12, max_it=2000)
    assert und["converged"] != 1
    out = dr.cocr(dr.masked_Z(K, M, P["shifts"][k], P["ck"][k], P["cm"][k], mask), b, pc, mask, rtol=1e-12)
    print(f"sigma = lambda_1: undamped MINRES {und['iterations']} iterations, converged {und['converged']}; damped COCR "
          f"{out['iterations']} iterations")
    assert out["converged"] == 1 and out["iterations"] < 200


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("case", range(len(dr.CASES)))
def test_adjoint_total_against_central_differences(case, squared):
    P = problem("rect8x4", case)
    mesh, mask, rho = P["mesh"], P["mask"], P["rho"]
    method, law = dr.CASES[case][:2]
    L = len(P["shifts"])
    F = np.tile(P["F"], (L, 1))
    kw = dict(weights=np.array(WEIGHTS), squared=squared, method=method, law=law, density=hr.DENSITY)
    args = (mask, F, P["shifts"], P["ck"], P["cm"])
    J, g, c, _ = dr.adjoint_total(mesh.x, mesh.conn, rho, *args, **kw)
    a = np.abs(c)
    assert J == pytest.approx(np.array(WEIGHTS) @ (a * a if squared else a), rel=1e-14)
    assert np.abs(c.imag).min() > 0.0                                  # the response is out of phase with the load
    d = np.random.default_rng(9).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    Jp = dr.adjoint_total(mesh.x, mesh.conn, rho + h * d, *args, **kw)[0]
    Jm = dr.adjoint_total(mesh.x, mesh.conn, rho - h * d, *args, **kw)[0]
    fd, an = (Jp - Jm) / (2 * h), float(g @ d)
    print(f"{dr.CASES[case]} squared={squared}: dJ/drho . d = {an:.9e}, central differences {fd:.9e}, "
          f"relative {abs(fd - an) / abs(an):.1e}")
    assert abs(fd - an) <= 1e-5 * abs(an)


def test_split_and_join():
    U = np.arange(6).reshape(2, 3) + 1j * (10 + np.arange(6).reshape(2, 3))
    X = dr.split(U)
    assert X.shape == (4, 3) and np.array_equal(X[1], U[0].imag) and np.array_equal(dr.join(X), U)


# ----------------------------------------------------------------------------------------------------- the surface ----
def test_entry_points_are_bound():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_cdyn_apply_multi", "femo_elast_cdyn_solve_multi"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.PROTOTYPES["femo_elast_cdyn_solve_multi"][1][-2:] == _lib.PROTOTYPES["femo_elast_dyn_solve_multi"][1][-2:]
    assert lib.femo_abi_version() == _lib.ABI_VERSION                 # a pure addition


def test_builders_are_exported():
    from femo_amd.fea import fea_hip
    from femo_amd.fea.elasticity import (DampedDynamicCompliance, DampedHarmonicElasticityMatrix,
                                         DampedHarmonicElasticityResidual, DeviceElasticity, HarmonicElasticityResidual,
                                         dynamic_compliance_damped, pdeRes_harmonic_damped)
    import femo_amd.fea as fea
    assert fea.pdeRes_harmonic_damped is pdeRes_harmonic_damped and fea.dynamic_compliance_damped is dynamic_compliance_damped
    assert fea.DampedHarmonicElasticityResidual is DampedHarmonicElasticityResidual
    assert fea.DampedDynamicCompliance is DampedDynamicCompliance
    assert fea_hip.pdeRes_harmonic_damped is pdeRes_harmonic_damped
    assert fea_hip.dynamic_compliance_damped is dynamic_compliance_damped
    assert issubclass(DampedHarmonicElasticityResidual, HarmonicElasticityResidual)
    assert not DampedHarmonicElasticityResidual.is_symmetric and not DampedHarmonicElasticityMatrix.symmetric
    assert callable(DampedHarmonicElasticityMatrix.backend_solve_transpose)
    assert DampedDynamicCompliance.rank == 0
    for name in ("cdyn_apply_multi", "cdyn_solve_multi"):
        assert callable(getattr(DeviceElasticity, name))


def test_ksp_hands_a_transposed_solve_to_the_operator():
    """`KSP.solve` on transpose(A) calls `backend_solve_transpose` where the operator has one, `backend_solve` otherwise."""
    from femo_amd.fea import utils_hip

    class Both:
        info = "info"
        calls = []

        def backend_solve(self, b, x, options):
            self.calls.append("plain")

        def backend_solve_transpose(self, b, x, options):
            self.calls.append("transposed")

    class Plain:
        info = None
        calls = []

        def backend_solve(self, b, x, options):
            self.calls.append("plain")

    orig = utils_hip._as_vec
    utils_hip._as_vec = lambda v: v
    try:
        A = Both()
        utils_hip.KSP(A).solve(None, None)
        k = utils_hip.KSP(utils_hip.transpose(A))
        k.solve(None, None)
        assert A.calls == ["plain", "transposed"] and k.info == "info"
        B = Plain()
        utils_hip.KSP(utils_hip.transpose(B)).solve(None, None)
        assert B.calls == ["plain"]
    finally:
        utils_hip._as_vec = orig
