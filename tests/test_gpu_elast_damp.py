"""GPU tests of the damped harmonic response of the SIMP elasticity (csrc/elast_damp.hip, `DeviceElasticity.cdyn_apply_multi /
cdyn_solve_multi`, `DampedHarmonicElasticityResidual`, `DampedDynamicCompliance`) against the restatement
tests/elast_damp_ref.py, its sparse complex matrices and its complex LU.

The meshes are those of tests/test_gpu_elast_harm.py: less than one wave of rows (rect8x4), the two jittered ones, two with
more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343), and fan40 (a hub row of 40 entries) for the product.
The set-up is that of the harmonic tests with the shifts {lambda_1 / 2, lambda_1, sqrt(lambda_1 lambda_2), sqrt(lambda_5 lambda_6)}
-- the second exactly on a resonance -- and the damping sets (eta, alpha, beta) = (0.05, 0, 0) with SIMP / linear mass and
(0, 0.02, 0.02) with RAMP / du_olhoff.

Bounds.  Product: 1e-13 of the largest entry (sums of at most ~40 terms per part, twice that with damping).  Solve: 1e-9 of
the largest entry of the complex LU and a backward error of 1e-12 -- the restatement reaches 2.1e-12 and 9.2e-16 on the CPU;
residual_norm <= rtol rhs_norm; block-Jacobi iterations at most those of the restated loop plus max(2, 10 %), the margin of the
MINRES test (the multilevel preconditioner has no restated loop to count against, as there).  Forms: J to 1e-10, the total
dJ/drho to 1e-6, directional central differences to 1e-5, the bounds of the undamped forms.

MEASURED on the MI355X (all meshes, both damping sets; the tests print every figure):
  Z x against the sparse complex product     9.9e-16 at the most over L = 1 ... 4, masked and not, conj 0 and 1, fan40 included; column l
                                             bit-identical to the one-column call; ck = cm = 0: both parts bit-identical to
                                             `dyn_apply_multi`
  solve against the complex LU               6.8e-12 at the most (rect24x12, block-Jacobi); res / beta1 7.1e-13 ... 1.0e-12
  backward error of the true residual        3.5e-15 at the most (rect8x4, multilevel); block-Jacobi 9.9e-16
  conj(Z) against the conjugate solution     0 (bit for bit)
  iterations, block-Jacobi, device / restatement (the four shifts in their order)
    rect8x4    80 83 85 93 / 80 83 86 93          square9j  138 144 152 172 / 138 144 150 172      (eta = 0.05, SIMP, linear)
    cube4j    115 127 127 155 / 115 127 127 154   rect24x12 273 282 298 352 / 273 282 314 352
    cube6j    173 189 190 232 / 173 189 190 232
    alpha = beta = 0.02, RAMP, du_olhoff: within 1 of the restatement
  multilevel                                 rect8x4 59 63 65 83 and 56 58 62 81, cube4j 65 76 76 97 and 65 76 76 98 iterations.  The lattice
                                             blocks are rebuilt per assembly and their bits are not pinned: counts move by 1-5
  columns scaled 1, 1e3, 1e-3, 1 + 0.5 i take 115, 154, 127, 127 iterations (multilevel 65, 99, 75, 76) and each has the bits of its own
  one-column solve
  forms: J 6.0e-13 at the most, c_l 7.6e-12, total dJ/drho 2.1e-10, directional central differences 8.2e-8 (rect24x12);
  w . (dR/drho v) against v . (dR/drho^T w) 1.2e-17
"""
import functools
import re

import numpy as np
import pytest

import elast_damp_ref as dr
import elast_eig_ref as er
import elast_harm_ref as hr
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BOTH_PC = ("rect8x4", "cube4j")
RTOL = 1e-12
CASES = list(range(len(dr.CASES)))


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def _mesh(name):
    from femo_amd.fea.mesh import Mesh, createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    if name == "fan40":
        import wide_meshes as W
        return Mesh(*W.fan(40, 8))
    return pr.small_meshes()[name]()


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


def _complex(v, L):
    """The L complex columns of a vector of 2L real ones."""
    return dr.join(_columns(v, 2 * L))


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@functools.lru_cache(maxsize=None)
def problem(name, case):
    """K, M, the load, the shifts and the damping coefficients: built once, read only."""
    return dr.problem(_mesh(name), *dr.CASES[case])


@functools.lru_cache(maxsize=None)
def restated(name, case):
    """Per shift: the complex LU and the restated block-Jacobi COCR at the device's tolerance."""
    P = problem(name, case)
    mask, K, M = P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, P["mesh"].tdim)
    b = np.where(mask == 1, 0.0, P["F"])
    runs = [dr.cocr(dr.masked_Z(K, M, sg, ck, cm, mask), b, pc, mask, rtol=RTOL) for sg, ck, cm in zip(P["shifts"], P["ck"], P["cm"])]
    assert all(r["converged"] == 1 for r in runs)
    U = np.stack([dr.direct(K, M, sg, ck, cm, P["F"], mask) for sg, ck, cm in zip(P["shifts"], P["ck"], P["cm"])])
    return dict(U=U, iterations=[r["iterations"] for r in runs], b=b)


def _device(gpu, P, fixed=True, mass=True):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    mesh = P["mesh"]
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    if fixed:
        dev.set_fixed(P["mask"])
    rv = Vec(gpu, mesh.n_cell).set(P["rho"])
    dev.assemble(METHODS[P["method"]], rv)
    if mass:
        dev.mass_assemble(rv, density=P["density"], mass_law=P["law"])
    return dev, rv


def _fan_problem(case):
    method, law, eta, alpha, beta = dr.CASES[case]
    mesh = _mesh("fan40")
    rho = np.random.default_rng(7).uniform(0.3, 1.0, mesh.n_cell)
    shifts = np.array([0.3, 1.1, 2.9, 7.3])
    ck, cm = dr.coefficients(shifts, eta, alpha, beta)
    return dict(mesh=mesh, mask=clamped_face(mesh), rho=rho, K=ref.stiffness(mesh.x, mesh.conn, rho, method),
                M=er.mass(mesh.x, mesh.conn, rho, law, hr.DENSITY), method=method, law=law, density=hr.DENSITY, shifts=shifts,
                ck=ck, cm=cm)


def _any_problem(name, case):
    return _fan_problem(case) if name == "fan40" else problem(name, case)


def _rhs(b, L, scales=None):
    """(2L, n): the real right-hand side b in the real part of every complex column."""
    B = np.zeros((2 * L, len(b)))
    B[0::2] = b if scales is None else np.outer(scales, b)
    return B


# ---------------------------------------------------------------------------------------------------------- product ----
@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("name", MESHES + ["fan40"])
def test_cdyn_apply(gpu, name, L):
    from femo_amd.engine import Vec
    worst = 0.0
    for case in CASES:
        P = _any_problem(name, case)
        mask, K, M = P["mask"], P["K"], P["M"]
        dev, _ = _device(gpu, P)
        n = dev.n_dof
        sel = np.array([3, 1, 0, 2])[:L]                                  # distinct, not in order
        shifts, ck, cm = P["shifts"][sel], P["ck"][sel], P["cm"][sel]
        rng = np.random.default_rng(12)
        X = rng.standard_normal((L, n)) + 1j * rng.standard_normal((L, n))
        Fv = rng.standard_normal((L, n)) + 1j * rng.standard_normal((L, n))
        xv, fv, yv = Vec(gpu, 2 * L * n).set(dr.split(X).ravel()), Vec(gpu, 2 * L * n).set(dr.split(Fv).ravel()), Vec(gpu, 2 * L * n)
        a, b = -1.5, 0.5
        for masked in (False, True):
            ops = [dr.masked_Z(K, M, sg, k, m, mask if masked else None) for sg, k, m in zip(shifts, ck, cm)]
            for conj in (False, True):
                Y = _complex(dev.cdyn_apply_multi(L, shifts, ck, cm, xv, yv, masked=masked, conj=conj, a=a, b=b, f=fv), L)
                want = np.stack([a * ((S.conj() if conj else S) @ x) + b * f for S, x, f in zip(ops, X, Fv)])
                err = max(_maxrel(Y[l], want[l]) for l in range(L))
                worst = max(worst, err)
                assert err <= 1e-13, (case, masked, conj, err)
                if masked:                                                # identity rows: y = a x + b f on the fixed dofs
                    assert np.abs(Y - (a * X + b * Fv))[:, mask == 1].max() <= 1e-15 * np.abs(Y).max()
                for l in range(L):                                        # a column does not depend on L
                    one = _complex(dev.cdyn_apply_multi(1, shifts[l:l + 1], ck[l:l + 1], cm[l:l + 1],
                                                        Vec(gpu, 2 * n).set(dr.split(X[l:l + 1]).ravel()), Vec(gpu, 2 * n),
                                                        masked=masked, conj=conj, a=a, b=b,
                                                        f=Vec(gpu, 2 * n).set(dr.split(Fv[l:l + 1]).ravel())), 1)[0]
                    assert np.array_equal(one, Y[l]), (l, masked, conj)
                # without the load term
                Y0 = _complex(dev.cdyn_apply_multi(L, shifts, ck, cm, xv, yv, masked=masked, conj=conj), L)
                assert max(_maxrel(Y0[l], (ops[l].conj() if conj else ops[l]) @ X[l]) for l in range(L)) <= 1e-13
                if masked:                                                # ... and exactly x without scaling and load
                    assert np.array_equal(Y0[:, mask == 1], X[:, mask == 1])
            # no damping: each part has the bits of the real shifted product on that real column
            zero = np.zeros(L)
            Yr = _columns(dev.cdyn_apply_multi(L, shifts, zero, zero, xv, yv, masked=masked, a=a, b=b, f=fv), 2 * L)
            Yd = _columns(dev.dyn_apply_multi(2 * L, np.repeat(shifts, 2), xv, Vec(gpu, 2 * L * n), masked=masked, a=a, b=b, f=fv), 2 * L)
            assert np.array_equal(Yr, Yd), (case, masked)
            Yc = _columns(dev.cdyn_apply_multi(L, shifts, zero, zero, xv, yv, masked=masked, conj=True, a=a, b=b, f=fv), 2 * L)
            assert np.array_equal(Yc, Yd), (case, masked)
    print(f"{name} L={L}: Z x against the sparse product {worst:.1e}")


# ------------------------------------------------------------------------------------------------------------ solve ----
def _solve_cases():
    for name in MESHES:
        for pc in (("jacobi", "multilevel") if name in BOTH_PC else ("jacobi",)):
            yield name, pc


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name,pc", list(_solve_cases()))
def test_cdyn_solve(gpu, name, pc, case):
    """All four shifts, the resonant one included, in one batched COCR against the complex LU; block-Jacobi counts against the
    restated loop; conj(Z) gives the conjugate solution for the real right-hand side."""
    from femo_amd.engine import Vec
    P, R = problem(name, case), restated(name, case)
    mask, L = P["mask"], len(P["shifts"])
    dev, _ = _device(gpu, P)
    if pc == "multilevel":
        dev.pc_setup()
    n = dev.n_dof
    bv, xv = Vec(gpu, 2 * L * n).set(_rhs(R["b"], L).ravel()), Vec(gpu, 2 * L * n).fill(7.0)   # zero_guess: the 7s are ignored
    infos = dev.cdyn_solve_multi(L, P["shifts"], P["ck"], P["cm"], bv, xv, rtol=RTOL, pc=pc)
    X = _complex(xv, L)
    errs = [_maxrel(X[l], R["U"][l]) for l in range(L)]
    its = [i.iterations for i in infos]
    eta = max(dr.backward_error(dr.masked_Z(P["K"], P["M"], sg, ck, cm, mask), X[l], R["b"])
              for l, (sg, ck, cm) in enumerate(zip(P["shifts"], P["ck"], P["cm"])))
    print(f"{name} {pc} {dr.CASES[case]}: COCR iterations {its} (restated block-Jacobi {R['iterations']}), error against the "
          f"complex LU {max(errs):.1e}, backward error {eta:.1e}, res / beta1 {max(i.residual_norm / i.rhs_norm for i in infos):.1e}")
    assert all(i.converged == 1 for i in infos)
    assert max(errs) <= 1e-9
    assert eta <= 1e-12
    assert np.all(X[:, mask == 1] == 0.0)
    assert all(i.residual_norm <= RTOL * i.rhs_norm for i in infos)
    if pc == "jacobi":
        for l in range(L):
            assert its[l] <= R["iterations"][l] + max(2.0, 0.1 * R["iterations"][l]), (l, its, R["iterations"])
    cv = Vec(gpu, 2 * L * n)
    cinfos = dev.cdyn_solve_multi(L, P["shifts"], P["ck"], P["cm"], bv, cv, conj=True, rtol=RTOL, pc=pc)
    errc = max(_maxrel(_complex(cv, L)[l], X[l].conj()) for l in range(L))
    print(f"{name} {pc} {dr.CASES[case]}: conj(Z) against the conjugate solution {errc:.1e}")
    assert all(i.converged == 1 for i in cinfos) and errc <= 1e-9


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_columns_are_independent(gpu, pc):
    """Four columns with right-hand sides scaled 1, 1e3, 1e-3, 1 (one of them complex, one zero column in a second solve): a
    column that finishes early is frozen while the others run, and each has the bits of its own one-column solve."""
    from femo_amd.engine import Vec
    P, R = problem("cube4j", 0), restated("cube4j", 0)
    dev, _ = _device(gpu, P)
    if pc == "multilevel":
        dev.pc_setup()
    n = dev.n_dof
    sel = np.array([0, 3, 1, 2])
    shifts, ck, cm = P["shifts"][sel], P["ck"][sel], P["cm"][sel]
    B = _rhs(R["b"], 4, scales=[1.0, 1e3, 1e-3, 1.0])
    B[7] = 0.5 * R["b"]                                                   # the last right-hand side is (1 + 0.5 i) b
    xv = Vec(gpu, 8 * n)
    infos = dev.cdyn_solve_multi(4, shifts, ck, cm, Vec(gpu, 8 * n).set(B.ravel()), xv, rtol=RTOL, pc=pc)
    X = _columns(xv, 8)
    its = [i.iterations for i in infos]
    print(f"cube4j {pc}: iterations {its}")
    assert [i.converged for i in infos] == [1, 1, 1, 1]
    assert min(its) < max(its)                                            # the first to finish was frozen while the slowest went on
    x1 = Vec(gpu, 2 * n)
    for l in range(4):
        one = dev.cdyn_solve_multi(1, shifts[l:l + 1], ck[l:l + 1], cm[l:l + 1], Vec(gpu, 2 * n).set(B[2 * l:2 * l + 2].ravel()), x1,
                                   rtol=RTOL, pc=pc)[0]
        assert one.iterations == its[l] and np.array_equal(_columns(x1, 2), X[2 * l:2 * l + 2]), l
    assert _maxrel(dr.join(X)[1], 1e3 * R["U"][3]) <= 1e-9
    assert _maxrel(dr.join(X)[3], (1.0 + 0.5j) * R["U"][2]) <= 1e-9
    # a zero column converges at iteration 0
    B[2:4] = 0.0
    infos = dev.cdyn_solve_multi(4, shifts, ck, cm, Vec(gpu, 8 * n).set(B.ravel()), xv, rtol=RTOL, pc=pc)
    assert infos[1].converged == 1 and infos[1].iterations == 0 and infos[1].rhs_norm == 0.0 and not _columns(xv, 8)[2:4].any()
    assert [i.iterations for i in infos][::2] == its[::2]
    # from the solution as the first guess, with an absolute level the first residual already meets: done at once
    keep = _columns(xv, 8)
    again = dev.cdyn_solve_multi(4, shifts, ck, cm, Vec(gpu, 8 * n).set(B.ravel()), xv, rtol=0.0, atol=1e-6 * infos[0].rhs_norm,
                                 zero_guess=False, pc=pc)
    assert [i.iterations for i in again] == [0, 0, 0, 0] and all(i.converged == 1 for i in again)
    assert np.array_equal(_columns(xv, 8), keep)


def test_max_it_and_non_finite(gpu):
    from femo_amd.engine import Vec
    P, R = problem("rect8x4", 0), restated("rect8x4", 0)
    dev, _ = _device(gpu, P)
    n = dev.n_dof
    sel = np.array([0, 3])
    shifts, ck, cm = P["shifts"][sel], P["ck"][sel], P["cm"][sel]
    xv = Vec(gpu, 4 * n)
    k0 = dev.cdyn_solve_multi(1, shifts[:1], ck[:1], cm[:1], Vec(gpu, 2 * n).set(_rhs(R["b"], 1).ravel()), Vec(gpu, 2 * n),
                              rtol=RTOL)[0].iterations
    assert k0 < R["iterations"][3] - 5                                    # the last shift needs more
    B = _rhs(R["b"], 2)
    infos = dev.cdyn_solve_multi(2, shifts, ck, cm, Vec(gpu, 4 * n).set(B.ravel()), xv, rtol=RTOL, max_it=k0)
    assert infos[0].converged == 1 and infos[0].iterations == k0
    assert infos[1].converged == 0 and infos[1].iterations == k0 and infos[1].residual_norm > RTOL * infos[1].rhs_norm
    short = dr.cocr(dr.masked_Z(P["K"], P["M"], shifts[1], ck[1], cm[1], P["mask"]), R["b"], hr.jacobi(P["K"], P["mask"], 2),
                    P["mask"], rtol=RTOL, max_it=k0)
    # the iterate of that many steps (an unconverged short recurrence amplifies rounding: 1e-6, as for the MINRES)
    assert _maxrel(_complex(xv, 2)[1], short["x"]) <= 1e-6
    bad = B.copy()
    bad[3, 5 * 2] = np.nan                                                # in the imaginary part of the second column
    infos = dev.cdyn_solve_multi(2, shifts, ck, cm, Vec(gpu, 4 * n).set(bad.ravel()), xv, rtol=RTOL)
    assert infos[0].converged == 1 and infos[1].converged == -1
    assert _maxrel(_complex(xv, 2)[0], R["U"][0]) <= 1e-9


# ------------------------------------------------------------------------------------------------------------ forms ----
WEIGHTS = (1.0, 0.5, 2.0, 1.5)


def _damped_model(P, squared, pc="multilevel"):
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, TestFunction,
                                      VectorFunctionSpace, dynamic_compliance_damped, meshtags, pdeRes_harmonic_damped)
    mesh, L = P["mesh"], len(P["shifts"])
    ds = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, P["facets"],
                                                            np.full(len(P["facets"]), 100, dtype=np.int32)))(100)
    fs, dss = [Constant(mesh, P["traction"])] * L, [ds] * L
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(LoadCaseSpace(V, 2 * L))
    res = pdeRes_harmonic_damped(u_fn, TestFunction(V), rho_fn, fs, dss, omegas=np.sqrt(P["shifts"]), loss_factor=P["eta"],
                                 rayleigh=(P["alpha"], P["beta"]), density=P["density"], mass_law=P["law"], method=P["method"],
                                 preconditioner=pc)
    out = dynamic_compliance_damped(u_fn, fs, dss, weights=WEIGHTS, squared=squared)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='dynamic_compliance', type='scalar', form=out, arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [np.nonzero(P["mask"])[0].astype(np.int32)], V)
    model = FEAModel(fea=[fea])
    model.create_input('density', shape=mesh.n_cell, val=P["rho"])
    model.add_design_variable('density', upper=1.0, lower=1e-4)
    model.add_objective('dynamic_compliance')
    return Simulator(model), res, out


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", MESHES)
def test_form(gpu, name, case, squared):
    """`DampedHarmonicElasticityResidual` and `DampedDynamicCompliance` through FEA.add_input / add_state / add_output and
    Simulator: J, the adjoint total and directional central differences (step 1e-6) of the device's own J."""
    P = problem(name, case)
    mesh, mask, L = P["mesh"], P["mask"], len(P["shifts"])
    method, law = dr.CASES[case][:2]
    sim, res, out = _damped_model(P, squared, pc="multilevel" if name in BOTH_PC else "jacobi")
    sim.run()
    F = np.tile(P["F"], (L, 1))
    J, g, c, U = dr.adjoint_total(mesh.x, mesh.conn, P["rho"], mask, F, P["shifts"], P["ck"], P["cm"], weights=WEIGHTS,
                                  squared=squared, method=method, law=law, density=P["density"])
    Jd = float(sim['dynamic_compliance'][0])
    errJ = abs(Jd - J) / abs(J)
    errc = _maxrel(out.responses(), c)
    gd = np.asarray(sim.compute_totals('dynamic_compliance', 'density')).ravel()
    errg = _maxrel(gd, g)
    assert res.solve_counts == {"state": 1, "adjoint": 1, "forward": 0}   # one batched COCR each
    assert res.last_info["state"]["converged"] == [1] * L and res.last_info["adjoint"]["converged"] == [1] * L
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    Js = []
    for sgn in (1.0, -1.0):
        sim['density'] = P["rho"] + sgn * h * d
        sim.run()
        Js.append(float(sim['dynamic_compliance'][0]))
    fd, an = (Js[0] - Js[1]) / (2 * h), float(gd @ d)
    errd = abs(fd - an) / abs(an)
    print(f"{name} {dr.CASES[case]} squared={squared}: J {errJ:.1e}, c_l {errc:.1e}, dJ/drho {errg:.1e}, central differences "
          f"{errd:.1e} (state {res.last_info['state']['iterations']}, adjoint {res.last_info['adjoint']['iterations']} iterations)")
    assert errJ <= 1e-10
    assert errg <= 1e-6
    assert errd <= 1e-5


def test_form_products_and_solves(gpu):
    """The residual vanishes at the solved state; dR/du, its transpose and a forward-mode solve against the SciPy operator;
    dR/drho forward against reverse and against the restatement."""
    import scipy.sparse.linalg as spla
    from femo_amd.engine import Vec
    from femo_amd.fea import utils_hip
    P = problem("cube4j", 1)
    mesh, mask, L = P["mesh"], P["mask"], len(P["shifts"])
    sim, res, _ = _damped_model(P, False, pc="jacobi")
    sim.run()
    n = res.n_dof
    U = dr.join(np.asarray(sim['displacements']).reshape(2 * L, n))
    r = _complex(res.assemble_vector(), L)
    for l, (sg, ck, cm) in enumerate(zip(P["shifts"], P["ck"], P["cm"])):     # the residual form at the solved state
        S = dr.Z(P["K"], P["M"], sg, ck, cm)
        assert np.linalg.norm(r[l, mask == 0]) <= 1e-12 * (abs(S).sum(axis=0).max() * np.linalg.norm(U[l]) + np.linalg.norm(P["F"]))
    rng = np.random.default_rng(2)
    A = res.new_matrix()
    assert not A.symmetric
    x = rng.standard_normal(2 * L * n)
    Xc = dr.join(x.reshape(2 * L, n))
    ops = [dr.Z(P["K"], P["M"], sg, ck, cm) for sg, ck, cm in zip(P["shifts"], P["ck"], P["cm"])]
    y = _complex(A.mult(Vec(gpu, 2 * L * n).set(x), Vec(gpu, 2 * L * n)), L)
    assert _maxrel(y, np.stack([S @ v for S, v in zip(ops, Xc)])) <= 1e-13
    yt = _complex(A.multTranspose(Vec(gpu, 2 * L * n).set(x), Vec(gpu, 2 * L * n)), L)
    assert _maxrel(yt, np.stack([S.conj() @ v for S, v in zip(ops, Xc)])) <= 1e-13
    S = A.to_scipy()                                                      # the real block operator of the 2L columns
    assert _maxrel(S @ x, dr.split(y).ravel()) <= 1e-12 and _maxrel(S.T @ x, dr.split(yt).ravel()) <= 1e-12
    # forward mode: a product and a solve with the masked operator, the adjoint solve with its transpose
    Am = res.matrix_class(res, masked=True)
    Sm = Am.to_scipy().tocsc()
    ym = np.array(Am.mult(Vec(gpu, 2 * L * n).set(x), Vec(gpu, 2 * L * n)).get())
    assert _maxrel(ym, Sm @ x) <= 1e-13
    b = np.where(np.tile(mask, 2 * L) == 1, 0.0, x)
    before = dict(res.solve_counts)
    sol = Vec(gpu, 2 * L * n)
    utils_hip.KSP(Am).solve(Vec(gpu, 2 * L * n).set(b), sol)
    assert res.solve_counts == dict(before, forward=before["forward"] + 1)
    assert _maxrel(np.array(sol.get()), spla.splu(Sm).solve(b)) <= 1e-9
    utils_hip.KSP(utils_hip.transpose(Am)).solve(Vec(gpu, 2 * L * n).set(b), sol)
    assert res.solve_counts == dict(before, forward=before["forward"] + 1, adjoint=before["adjoint"] + 1)
    assert _maxrel(np.array(sol.get()), spla.splu(Sm.T.tocsc()).solve(b)) <= 1e-9
    # dR/drho
    D = res.partial_matrix(res.rho)
    dvec, w = rng.standard_normal(mesh.n_cell), rng.standard_normal(2 * L * n)
    fwd = np.array(D.mult(Vec(gpu, mesh.n_cell).set(dvec), Vec(gpu, 2 * L * n)).get())
    rev = np.array(D.multTranspose(Vec(gpu, 2 * L * n).set(w), Vec(gpu, mesh.n_cell)).get())
    tr = abs(w @ fwd - dvec @ rev) / (np.linalg.norm(w) * np.linalg.norm(fwd))
    print(f"dR/drho: w.(D v) against v.(D^T w) {tr:.1e}")
    assert tr <= 1e-12
    # -u^T dR/drho, unconjugated, is dc/drho: with w = -(Re u, -Im u) the reverse product is its real part
    G = dr.response_gradients(mesh.x, mesh.conn, P["rho"], U, P["shifts"], P["ck"], P["cm"], P["method"], P["law"], P["density"])
    revu = np.array(D.multTranspose(Vec(gpu, 2 * L * n).set(-dr.split(U.conj()).ravel()), Vec(gpu, mesh.n_cell)).get())
    assert _maxrel(revu, G.real.sum(axis=0)) <= 1e-8                      # twice the bound of the state
    # and a forward-mode product of dR/drho against finite differences of the operator in the density
    h = 1e-6
    Zp = [dr.Z(ref.stiffness(mesh.x, mesh.conn, P["rho"] + s * h * dvec, P["method"]),
               er.mass(mesh.x, mesh.conn, P["rho"] + s * h * dvec, P["law"], P["density"]), sg, ck, cm) @ u
          for s in (1.0, -1.0) for sg, ck, cm, u in zip(P["shifts"], P["ck"], P["cm"], U)]
    fd = (np.stack(Zp[:L]) - np.stack(Zp[L:])) / (2 * h)
    assert _maxrel(dr.join(fwd.reshape(2 * L, n)), fd) <= 1e-6


def test_form_raises_when_a_column_does_not_converge(gpu):
    P = problem("square9j", 0)
    sim, res, _ = _damped_model(P, False, pc="jacobi")
    res.max_it = 5
    om = np.sqrt(P["shifts"])
    with pytest.raises(RuntimeError, match=re.escape(f"column 0 of 4, omega = {om[0]:.6g})")):
        sim.run()
    its = restated("square9j", 0)["iterations"]
    cut = (max(its[:3]) + its[3]) // 2
    assert max(its[:3]) + 4 <= cut <= its[3] - 4                          # the first three columns make it, the fourth does not
    res.max_it = cut
    with pytest.raises(RuntimeError, match=re.escape(f"column 3 of 4, omega = {om[3]:.6g})")):
        sim.run()


# ------------------------------------------------------------------------------------------------ limits and errors ----
def test_refusals(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DampedDynamicCompliance, DampedHarmonicElasticityResidual
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    P = problem("rect8x4", 0)
    mesh = P["mesh"]
    dev, rv = _device(gpu, P, fixed=False, mass=False)
    n = dev.n_dof
    CM = ELAST_MAX_COLS // 2
    big, y = Vec(gpu, 2 * (CM + 1) * n).fill(1.0), Vec(gpu, 2 * (CM + 1) * n)
    one = np.ones(CM + 1)
    with pytest.raises(FemoError, match="assemble M"):
        dev.cdyn_apply_multi(2, one[:2], one[:2], one[:2], big, y)
    with pytest.raises(FemoError, match="assemble M"):
        dev.cdyn_solve_multi(2, one[:2], one[:2], one[:2], big, y)
    dev.mass_assemble(rv)
    for bad in (0, CM + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.cdyn_apply_multi(bad, one[:bad], one[:bad], one[:bad], big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.cdyn_solve_multi(bad, one[:bad], one[:bad], one[:bad], big, y)
        with pytest.raises(FemoError, match="columns"):                   # the library's own check
            _raw_solve(dev, bad, big, y)
    with pytest.raises(FemoError, match="as many shifts"):
        dev.cdyn_apply_multi(3, one[:2], one[:3], one[:3], big, y)
    with pytest.raises(FemoError, match="as many ck"):
        dev.cdyn_solve_multi(3, one[:3], one[:2], one[:3], big, y)
    for k in range(3):
        for v in (-1e-3, np.nan, np.inf):
            args = [one[:2].copy() for _ in range(3)]
            args[k][1] = v
            with pytest.raises(FemoError, match="finite and >= 0"):
                dev.cdyn_apply_multi(2, *args, big, y)
            with pytest.raises(FemoError, match="finite and >= 0"):
                dev.cdyn_solve_multi(2, *args, big, y)
    with pytest.raises(FemoError, match="fixed set"):
        dev.cdyn_apply_multi(2, one[:2], one[:2], one[:2], big, y, masked=True)
    with pytest.raises(FemoError, match="differ"):
        dev.cdyn_apply_multi(2, one[:2], one[:2], one[:2], y, y)
    with pytest.raises(FemoError):
        dev.cdyn_solve_multi(2, one[:2], one[:2], one[:2], y, y)
    with pytest.raises(FemoError):
        dev.cdyn_apply_multi(2, one[:2], one[:2], one[:2], Vec(gpu, 4 * n - 1), y)
    with pytest.raises(FemoError):
        dev.cdyn_solve_multi(2, one[:2], one[:2], one[:2], big, Vec(gpu, 4 * n - 1))
    with pytest.raises(ValueError):
        dev.cdyn_solve_multi(2, one[:2], one[:2], one[:2], big, y, pc="ilu")
    with pytest.raises(FemoError, match="multilevel"):
        dev.cdyn_solve_multi(2, one[:2], one[:2], one[:2], big, y, pc="multilevel")   # no pc_setup
    # the forms
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    u, rho = Function(LoadCaseSpace(V, 4)), Function(Q)
    t = [(0.0, -1.0)] * 2
    ok = dict(omegas=[0.0, 1.0])
    with pytest.raises(ValueError, match="load cases"):                   # more than 4 frequencies: no state to hold them
        LoadCaseSpace(V, 10)
    u8 = Function(LoadCaseSpace(V, 8))
    with pytest.raises(ValueError, match="as many tractions"):
        DampedHarmonicElasticityResidual(u8, rho, [(0.0, -1.0)] * 5, omegas=np.ones(5))
    with pytest.raises(ValueError, match="as many tractions"):
        DampedDynamicCompliance(u8, [(0.0, -1.0)] * 5)
    with pytest.raises(ValueError, match="even number"):                  # a state of odd column count
        DampedHarmonicElasticityResidual(Function(LoadCaseSpace(V, 3)), rho, t, **ok)
    with pytest.raises(ValueError, match="even number"):
        DampedDynamicCompliance(Function(LoadCaseSpace(V, 3)), t)
    for kw in (dict(loss_factor=-0.01), dict(rayleigh=(-0.1, 0.0)), dict(rayleigh=(0.0, -0.1)), dict(loss_factor=np.nan),
               dict(rayleigh=(0.0, np.inf)), dict(rayleigh=(0.1,))):
        with pytest.raises(ValueError, match="damping"):
            DampedHarmonicElasticityResidual(u, rho, t, **ok, **kw)
    with pytest.raises(ValueError, match="omega"):
        DampedHarmonicElasticityResidual(u, rho, t, omegas=[1.0, -0.5])
    with pytest.raises(ValueError, match="omega"):
        DampedHarmonicElasticityResidual(u, rho, t)
    with pytest.raises(ValueError):
        DampedHarmonicElasticityResidual(u, rho, t, omegas=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="as many tractions"):
        DampedHarmonicElasticityResidual(u, rho, t * 2, omegas=[1.0] * 4)   # one traction per frequency, not per column
    with pytest.raises(NotImplementedError, match="body forces"):
        DampedHarmonicElasticityResidual(u, rho, t, body_forces=[(0.0, -1.0), None], **ok)
    with pytest.raises(ValueError, match="traction"):
        DampedHarmonicElasticityResidual(u, rho, [(0.0, -1.0), None], **ok)
    with pytest.raises(NotImplementedError):
        DampedHarmonicElasticityResidual(Function(V), rho, t[:1], omegas=[1.0])        # not a LoadCaseSpace state
    with pytest.raises(NotImplementedError):
        DampedHarmonicElasticityResidual(u, Function(V), t, **ok)                       # the density is DG0
    with pytest.raises(ValueError, match="mass law"):
        DampedHarmonicElasticityResidual(u, rho, t, mass_law="lumped", **ok)
    with pytest.raises(ValueError):
        DampedHarmonicElasticityResidual(u, rho, t, preconditioner="ilu", **ok)
    res = DampedHarmonicElasticityResidual(u, rho, t, loss_factor=0.1, rayleigh=(0.2, 0.3), omegas=[0.0, 2.0])
    assert np.array_equal(res.shifts, [0.0, 4.0]) and np.allclose(res.ck, [0.1, 0.7]) and np.allclose(res.cm, [0.0, 0.4])
    assert res.n_freq == 2 and res.n_cases == 4
    dofs = np.nonzero(P["mask"])[0].astype(np.int32)
    with pytest.raises(NotImplementedError, match="inhomogeneous"):
        res.solve_state(u, [dirichletbc(0.5, dofs, V)])
    with pytest.raises(ValueError, match="weights"):
        DampedDynamicCompliance(u, t, weights=[1.0])
    with pytest.raises(NotImplementedError):
        DampedDynamicCompliance(Function(V), t[:1])


def _raw_solve(dev, n_cols, b, x):
    """femo_elast_cdyn_solve_multi past the Python checks."""
    import ctypes as C
    from femo_amd import _lib
    one = np.ones(max(n_cols, 1))
    p = one.ctypes.data_as(_lib.c_f64p)
    opts = dev._solver_opts(1e-12, 0.0, 10, None, True, "jacobi")
    _lib.check(dev.lib.femo_elast_cdyn_solve_multi(dev.handle, 0, n_cols, p, p, p, b.handle, x.handle, C.byref(opts), None))
