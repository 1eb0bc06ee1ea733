"""GPU tests of the harmonic response of the SIMP elasticity (csrc/elast_harm.hip, `DeviceElasticity.mass_assemble /
dyn_apply_multi / dyn_solve_multi / mass_drho_multi`, `HarmonicElasticityResidual`, `DynamicCompliance`) against the
restatement tests/elast_harm_ref.py, its dense matrices and its sparse direct solves.

The meshes are those of tests/test_gpu_elast_eig.py: less than one wave of rows (rect8x4), the two jittered ones, and two
with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343); fan40 of tests/wide_meshes.py (a hub row of 40
entries) for assembly and product.  Clamped on x = 0, rho = default_rng(7).uniform(0.3, 1), mass density 1.3, traction
(0, -1[, 0]) on the face x = max, SIMP with the linear mass law and RAMP with du_olhoff, and the five shifts
sigma in {0, lambda_1 / 2, sqrt(lambda_1 lambda_2), sqrt(lambda_2 lambda_3), sqrt(lambda_5 lambda_6)} of the dense pencil: K - sigma M is
indefinite from the third on.

Bounds.  Products and dR/drho: 1e-13 of the largest entry (sums of at most ~40 terms of one sign pattern each).  Solve: 1e-9
of the largest entry of the direct solve -- the restatement reaches 1.7e-12 on the CPU, the margin absorbs another summation
order; iterations at most those of the restated loop (block-Jacobi, the same stopping test) plus max(2, 10 %).  Forms: J to
1e-10, the total dJ/drho to 1e-6 and directional central differences to 1e-5, the bounds of the eigen and buckling outputs.

MEASURED on the MI355X (all meshes, both law pairs; the tests print every figure):
  assembled M against the restatement        6.4e-16 at the most, symmetric bit for bit, the pattern of the restatement
  (K - sigma M) x against the dense product  1.1e-15 at the most over 96 cases (L = 1, 3, 5, 8, masked and not, fan40 included);
                                             column l bit-identical to the one-column call, sigma = 0 to `apply_multi`
  mass part of dR/drho                       forward 1.3e-15, reverse 1.9e-15, transposes 2.5e-17
  solve against the direct solve             2.3e-12 at the most (cube4j, block-Jacobi); bound 1e-9; phibar / beta1 7.8e-13 ... 9.9e-13
  backward error of the true residual        2.6e-14 at the most (the restatement: 3.9e-14); bound 1e-12
  iterations, block-Jacobi, device / restatement (the five shifts in their order)
    rect8x4    79 80 79 82 92 / 79 80 79 85 93        square9j  136 138 139 155 168 / 136 138 139 155 172   (SIMP, linear)
    cube4j    110 115 134 122 157 / 109 115 133 122 157    rect24x12 270 273 271 309 344 / 270 273 271 309 355
    cube6j    164 173 192 184 237 / 164 173 192 184 237
    RAMP / du_olhoff: within 10 of the restatement (rect24x12: 315 against 305 on the fourth shift).  The restated count of
    a column next to a resonance moves with the host's BLAS (cube4j, RAMP, third shift: 135 on one machine, 158 on another;
    the device takes 135)
  multilevel                                 rect8x4 58 59 59 66 82, cube4j 59 65 82 73 96 iterations, errors 1.0e-12 at the most.  The
                                             lattice blocks are rebuilt per assembly and their bits are not pinned: counts move by 1-3
  a zero column 0 iterations; columns (sigma_0, 0, sigma_4, sigma_2) take 110, 0, 157, 134 iterations and each has the bits of its own
  one-column solve
  forms: J 6.4e-11 at the most (cube4j, RAMP, next to the cluster lambda_1, lambda_2; 1.7e-12 elsewhere), bound 1e-10; total dJ/drho
  4.4e-11, bound 1e-6; directional central differences 7.4e-7 at the most (cube4j), 3.0e-8 elsewhere, bound 1e-5
"""
import functools

import numpy as np
import pytest

import elast_eig_ref as er
import elast_harm_ref as hr
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BOTH_PC = ("rect8x4", "cube4j")
RTOL = 1e-12


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


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _backward_error(S, x, b):
    """|b - S x|_2 / (|S|_1 |x|_2 + |b|_2): the restated MINRES leaves 3.9e-14 at the most on these cases (about 4e-9 of |b| on
    the columns next to a resonance, where |x| is large); the tests ask for 1e-12."""
    return np.linalg.norm(b - S @ x) / (abs(S).sum(axis=0).max() * np.linalg.norm(x) + np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def problem(name, method, law):
    """K, M, the load, the shifts: built once, read only."""
    return hr.problem(_mesh(name), method, law)


@functools.lru_cache(maxsize=None)
def restated(name, method, law):
    """Per shift: the direct solve and the restated block-Jacobi MINRES at the device's tolerance."""
    P = problem(name, method, law)
    mask, K, M = P["mask"], P["K"], P["M"]
    pc = hr.jacobi(K, mask, P["mesh"].tdim)
    b = np.where(mask == 1, 0.0, P["F"])
    runs = [hr.minres(hr.masked_shifted(K, M, sg, mask), b, pc, mask, rtol=RTOL) for sg in P["shifts"]]
    assert all(r["converged"] == 1 for r in runs)
    U = np.stack([hr.direct(K, M, sg, P["F"], mask) for sg in P["shifts"]])
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


def _fan_problem(method, law):
    mesh = _mesh("fan40")
    rho = np.random.default_rng(7).uniform(0.3, 1.0, mesh.n_cell)
    return dict(mesh=mesh, mask=clamped_face(mesh), rho=rho, K=ref.stiffness(mesh.x, mesh.conn, rho, method),
                M=er.mass(mesh.x, mesh.conn, rho, law, hr.DENSITY), method=method, law=law, density=hr.DENSITY,
                shifts=np.array([0.0, 0.3, 1.1, 2.9, 7.3]))


def _any_problem(name, method, law):
    return _fan_problem(method, law) if name == "fan40" else problem(name, method, law)


# ------------------------------------------------------------------------------------------- assembly and product ----
@pytest.mark.parametrize("law", er.MASS_LAWS)
@pytest.mark.parametrize("name", MESHES + ["fan40"])
def test_mass_assemble(gpu, name, law):
    """The assembled M, column by column through products with unit vectors on a handle whose K is exactly zero (SIMP of a
    zero density), where -(K - 1 M) e_j = M e_j bit for bit: against the restatement, and symmetric bit for bit.  Densities
    on both branches of du_olhoff."""
    from femo_amd._lib import ELAST_MAX_COLS as EMC
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.02, 1.0, mesh.n_cell)
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    dev.assemble(METHODS["SIMP"], Vec(gpu, mesh.n_cell).fill(0.0))
    dev.mass_assemble(Vec(gpu, mesh.n_cell).set(rho), density=2.5, mass_law=law)
    n = dev.n_dof
    Md = np.zeros((n, n))
    xv, yv = Vec(gpu, EMC * n), Vec(gpu, EMC * n)
    for j0 in range(0, n, EMC):
        L = min(EMC, n - j0)
        X = np.zeros((EMC, n))
        X[np.arange(L), j0 + np.arange(L)] = 1.0
        Md[:, j0:j0 + L] = _columns(dev.dyn_apply_multi(L, np.ones(L), xv.set(X.ravel()), yv, a=-1.0), EMC)[:L].T
    want = er.mass(mesh.x, mesh.conn, rho, law, 2.5).toarray()
    err = np.abs(Md - want).max() / np.abs(want).max()
    print(f"{name} {law}: assembled M against the restatement {err:.1e}")
    assert err <= 1e-13
    assert np.array_equal(Md, Md.T)                                   # bit for bit
    assert np.array_equal(Md != 0.0, want != 0.0)
    # assembling again gives the same bits (no atomics), and a new density replaces the old one
    dev.mass_assemble(Vec(gpu, mesh.n_cell).set(rho), density=2.5, mass_law=law)
    X = np.random.default_rng(3).standard_normal(n)
    y1 = np.array(dev.dyn_apply_multi(1, [1.0], Vec(gpu, n).set(X), Vec(gpu, n), a=-1.0).get())
    assert _maxrel(y1, want @ X) <= 1e-13


@pytest.mark.parametrize("L", [1, 3, 5, 8])
@pytest.mark.parametrize("name", MESHES + ["fan40"])
def test_dyn_apply(gpu, name, L):
    from femo_amd.engine import Vec
    for method, law in hr.CASES:
        P = _any_problem(name, method, law)
        mask, K, M = P["mask"], P["K"], P["M"]
        dev, _ = _device(gpu, P)
        n = dev.n_dof
        shifts = np.resize(np.concatenate([P["shifts"][1:], P["shifts"][:1], 1.7 * P["shifts"][1:4]]), 8)[:L]   # distinct, one zero
        rng = np.random.default_rng(12)
        X, Fv = rng.standard_normal((L, n)), rng.standard_normal((L, n))
        xv, fv, yv, x1, y1 = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(Fv.ravel()), Vec(gpu, L * n), Vec(gpu, n), Vec(gpu, n)
        a, b = -1.5, 0.5
        for masked in (False, True):
            Y = _columns(dev.dyn_apply_multi(L, shifts, xv, yv, masked=masked, a=a, b=b, f=fv), L)
            ops = [hr.masked_shifted(K, M, sg, mask) if masked else hr.shifted(K, M, sg) for sg in shifts]
            want = np.stack([a * (S @ x) + b * f for S, x, f in zip(ops, X, Fv)])
            err = max(np.abs(Y[l] - want[l]).max() / np.abs(want[l]).max() for l in range(L))
            print(f"{name} {method}/{law} L={L} masked={masked}: (K - sigma M) x against the dense product {err:.1e}")
            assert err <= 1e-13
            assert np.array_equal(_columns(dev.dyn_apply_multi(L, shifts, xv, yv, masked=masked, a=a, b=b, f=fv), L), Y)
            for l in range(L):                                        # a column does not depend on L
                one = np.array(dev.dyn_apply_multi(1, shifts[l:l + 1], x1.set(X[l]), y1, masked=masked, a=a, b=b,
                                                   f=Vec(gpu, n).set(Fv[l])).get())
                assert np.array_equal(one, Y[l]), (l, masked)
            # sigma = 0: the bits of the static product, with and without the load term
            Z = _columns(dev.dyn_apply_multi(L, np.zeros(L), xv, yv, masked=masked, a=a, b=b, f=fv), L)
            assert np.array_equal(Z, _columns(dev.apply_multi(L, xv, Vec(gpu, L * n), masked=masked, a=a, b=b, f=fv), L))
            Z = _columns(dev.dyn_apply_multi(L, np.zeros(L), xv, yv, masked=masked), L)
            assert np.array_equal(Z, _columns(dev.apply_multi(L, xv, Vec(gpu, L * n), masked=masked), L))
            if masked:                                                # identity rows: y = a x + b f on the fixed dofs
                assert np.abs(Y - (a * X + b * Fv))[:, mask == 1].max() <= 1e-15 * np.abs(Y).max()


@pytest.mark.parametrize("law", er.MASS_LAWS)
@pytest.mark.parametrize("name", MESHES)
def test_mass_drho(gpu, name, law):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.02, 1.0, mesh.n_cell)    # cells on both branches of du_olhoff
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    rv = Vec(gpu, mesh.n_cell).set(rho)
    n, nc, L = dev.n_dof, mesh.n_cell, 3
    rng = np.random.default_rng(5)
    U, Xn, xc, s = rng.standard_normal((L, n)), rng.standard_normal((L, n)), rng.standard_normal(nc), np.array([-0.7, 0.0, -3.1])
    D = [hr.mass_drho_matrix(mesh.x, mesh.conn, rho, U[l], law, hr.DENSITY) for l in range(L)]
    uv, xnv, xcv = Vec(gpu, L * n).set(U.ravel()), Vec(gpu, L * n).set(Xn.ravel()), Vec(gpu, nc).set(xc)
    kw = dict(density=hr.DENSITY, mass_law=law)
    fwd = _columns(dev.mass_drho_multi(False, L, s, rv, uv, xcv, Vec(gpu, L * n), **kw), L)
    want_f = np.stack([s[l] * (D[l] @ xc) for l in range(L)])
    rev = np.array(dev.mass_drho_multi(True, L, s, rv, uv, xnv, Vec(gpu, nc), **kw).get())
    want_r = sum(s[l] * (D[l].T @ Xn[l]) for l in range(L))
    ef, er_ = _maxrel(fwd, want_f), _maxrel(rev, want_r)
    tr = abs(np.sum(fwd * Xn) - rev @ xc) / (np.linalg.norm(fwd) * np.linalg.norm(Xn))
    print(f"{name} {law}: mass dR/drho forward {ef:.1e}, reverse {er_:.1e}, transposes {tr:.1e}")
    assert ef <= 1e-13 and er_ <= 1e-13 and tr <= 1e-13
    assert np.all(fwd[1] == 0.0)                                      # the column of scale 0
    # accumulate
    base_n, base_c = rng.standard_normal((L, n)), rng.standard_normal(nc)
    fa = _columns(dev.mass_drho_multi(False, L, s, rv, uv, xcv, Vec(gpu, L * n).set(base_n.ravel()), accumulate=True, **kw), L)
    ra = np.array(dev.mass_drho_multi(True, L, s, rv, uv, xnv, Vec(gpu, nc).set(base_c), accumulate=True, **kw).get())
    assert _maxrel(fa, base_n + want_f) <= 1e-13 and _maxrel(ra, base_c + want_r) <= 1e-13
    # a column does not depend on how many go with it
    one = np.array(dev.mass_drho_multi(False, 1, s[2:], rv, Vec(gpu, n).set(U[2]), xcv, Vec(gpu, n), **kw).get())
    assert np.array_equal(one, fwd[2])


# -------------------------------------------------------------------------------------------------------- the solve ----
def _solve_cases():
    for name in MESHES:
        for pc in (("jacobi", "multilevel") if name in BOTH_PC else ("jacobi",)):
            yield name, pc


@pytest.mark.parametrize("method,law", hr.CASES)
@pytest.mark.parametrize("name,pc", list(_solve_cases()))
def test_dyn_solve(gpu, name, pc, method, law):
    """All five shifts in one batched MINRES against the direct solves; block-Jacobi counts against the restated loop."""
    from femo_amd.engine import Vec
    P, R = problem(name, method, law), restated(name, method, law)
    mask, L = P["mask"], len(P["shifts"])
    dev, _ = _device(gpu, P)
    if pc == "multilevel":
        dev.pc_setup()
    n = dev.n_dof
    bv, xv = Vec(gpu, L * n).set(np.tile(R["b"], L)), Vec(gpu, L * n).fill(7.0)      # zero_guess: the 7s are ignored
    infos = dev.dyn_solve_multi(L, P["shifts"], bv, xv, rtol=RTOL, pc=pc)
    X = _columns(xv, L)
    errs = [_maxrel(X[l], R["U"][l]) for l in range(L)]
    its = [i.iterations for i in infos]
    print(f"{name} {pc} {method}/{law}: MINRES iterations {its} (restated block-Jacobi {R['iterations']}), "
          f"error against the direct solve {max(errs):.1e}, phibar / beta1 {max(i.residual_norm / i.rhs_norm for i in infos):.1e}")
    assert all(i.converged == 1 for i in infos)
    assert max(errs) <= 1e-9
    assert np.all(X[:, mask == 1] == 0.0)
    assert all(i.residual_norm <= RTOL * i.rhs_norm for i in infos)
    if pc == "jacobi":
        for l in range(L):
            assert its[l] <= R["iterations"][l] + max(2.0, 0.1 * R["iterations"][l]), (l, its, R["iterations"])
    # the true residual: phibar is the recurrence's estimate, which parts from it by about eps cond(S)
    eta = max(_backward_error(hr.masked_shifted(P["K"], P["M"], sg, mask), X[l], R["b"]) for l, sg in enumerate(P["shifts"]))
    print(f"{name} {pc} {method}/{law}: backward error of the true residual {eta:.1e}")
    assert eta <= 1e-12


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_columns_are_independent(gpu, pc):
    """A zero column converges at iteration 0; a column that finishes early keeps its bits while the others run; a column
    has the same bits whatever travels with it; a first guess is honoured."""
    from femo_amd.engine import Vec
    P, R = problem("cube4j", "SIMP", "linear"), restated("cube4j", "SIMP", "linear")
    dev, _ = _device(gpu, P)
    if pc == "multilevel":
        dev.pc_setup()
    n, sh = dev.n_dof, P["shifts"]
    B = np.stack([R["b"], np.zeros(n), R["b"], 1e3 * R["b"]])
    shifts = np.array([sh[0], sh[3], sh[4], sh[2]])
    xv = Vec(gpu, 4 * n)
    infos = dev.dyn_solve_multi(4, shifts, Vec(gpu, 4 * n).set(B.ravel()), xv, rtol=RTOL, pc=pc)
    X = _columns(xv, 4)
    its = [i.iterations for i in infos]
    print(f"cube4j {pc}: iterations {its}")
    assert [i.converged for i in infos] == [1, 1, 1, 1]
    assert its[1] == 0 and infos[1].rhs_norm == 0.0 and not X[1].any()
    assert its[0] < its[2]                                            # column 0 was frozen while column 2 went on
    x1 = Vec(gpu, n)
    for l in (0, 2, 3):
        one = dev.dyn_solve_multi(1, shifts[l:l + 1], Vec(gpu, n).set(B[l]), x1, rtol=RTOL, pc=pc)[0]
        assert one.iterations == its[l] and np.array_equal(np.array(x1.get()), X[l]), l
    assert _maxrel(X[3], 1e3 * R["U"][2]) <= 1e-9
    # from the solution as the first guess, with an absolute level the first residual already meets: done at once
    again = dev.dyn_solve_multi(4, shifts, Vec(gpu, 4 * n).set(B.ravel()), xv, rtol=0.0, atol=1e-6 * infos[0].rhs_norm,
                                zero_guess=False, pc=pc)
    assert [i.iterations for i in again] == [0, 0, 0, 0] and all(i.converged == 1 for i in again)
    assert np.array_equal(_columns(xv, 4), X)


def test_max_it_and_non_finite(gpu):
    from femo_amd.engine import Vec
    P, R = problem("rect8x4", "SIMP", "linear"), restated("rect8x4", "SIMP", "linear")
    dev, _ = _device(gpu, P)
    n, sh = dev.n_dof, P["shifts"]
    xv = Vec(gpu, 2 * n)
    k0 = dev.dyn_solve_multi(1, sh[:1], Vec(gpu, n).set(R["b"]), Vec(gpu, n), rtol=RTOL)[0].iterations
    assert k0 < R["iterations"][4] - 5                                # the last shift needs more
    infos = dev.dyn_solve_multi(2, sh[[0, 4]], Vec(gpu, 2 * n).set(np.tile(R["b"], 2)), xv, rtol=RTOL, max_it=k0)
    assert infos[0].converged == 1 and infos[0].iterations == k0
    assert infos[1].converged == 0 and infos[1].iterations == k0 and infos[1].residual_norm > RTOL * infos[1].rhs_norm
    short = hr.minres(hr.masked_shifted(P["K"], P["M"], sh[4], P["mask"]), R["b"], hr.jacobi(P["K"], P["mask"], 2), P["mask"],
                      rtol=RTOL, max_it=k0)
    # the iterate of that many steps, the last one included (an unconverged Lanczos recurrence amplifies rounding: 1e-6)
    assert _maxrel(_columns(xv, 2)[1], short["x"]) <= 1e-6
    bad = np.tile(R["b"], 2)
    bad[n + 5 * 2] = np.nan
    infos = dev.dyn_solve_multi(2, sh[[0, 4]], Vec(gpu, 2 * n).set(bad), xv, rtol=RTOL)
    assert infos[0].converged == 1 and infos[1].converged == -1


# ---------------------------------------------------------------------------------------------------------- the forms ----
WEIGHTS = (1.0, 0.5, 2.0, 1.5, 0.25)


def _harmonic_model(P, squared, pc="multilevel"):
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, TestFunction,
                                      VectorFunctionSpace, dirichletbc, dynamic_compliance, meshtags, pdeRes_harmonic)
    mesh, L = P["mesh"], len(P["shifts"])
    ds = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, P["facets"],
                                                            np.full(len(P["facets"]), 100, dtype=np.int32)))(100)
    fs, dss = [Constant(mesh, P["traction"])] * L, [ds] * L
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(LoadCaseSpace(V, L))
    res = pdeRes_harmonic(u_fn, TestFunction(V), rho_fn, fs, dss, omegas=np.sqrt(P["shifts"]), density=P["density"],
                          mass_law=P["law"], method=P["method"], preconditioner=pc)
    out = dynamic_compliance(u_fn, fs, dss, weights=WEIGHTS, squared=squared)
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
@pytest.mark.parametrize("method,law", hr.CASES)
@pytest.mark.parametrize("name", MESHES)
def test_form(gpu, name, method, law, squared):
    """`HarmonicElasticityResidual` and `DynamicCompliance` through FEA.add_input / add_state / add_output and Simulator: J, the
    adjoint total and directional central differences (step 1e-6) of the device's own J."""
    P = problem(name, method, law)
    mesh, mask, L = P["mesh"], P["mask"], len(P["shifts"])
    sim, res, out = _harmonic_model(P, squared, pc="multilevel" if name in BOTH_PC else "jacobi")
    sim.run()
    F = np.tile(P["F"], (L, 1))
    J, g, c, U = hr.adjoint_total(mesh.x, mesh.conn, P["rho"], mask, F, P["shifts"], weights=WEIGHTS, squared=squared,
                                  method=method, law=law, density=P["density"])
    Jd = float(sim['dynamic_compliance'][0])
    errJ = abs(Jd - J) / abs(J)
    errc = _maxrel(out.responses(), c)
    gd = np.asarray(sim.compute_totals('dynamic_compliance', 'density')).ravel()
    errg = _maxrel(gd, g)
    assert res.solve_counts == {"state": 1, "adjoint": 1}            # one batched MINRES each
    assert res.last_info["adjoint"]["converged"] == [1] * L
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    Js = []
    for sgn in (1.0, -1.0):
        sim['density'] = P["rho"] + sgn * h * d
        sim.run()
        Js.append(float(sim['dynamic_compliance'][0]))
    fd, an = (Js[0] - Js[1]) / (2 * h), float(gd @ d)
    errd = abs(fd - an) / abs(an)
    print(f"{name} {method}/{law} squared={squared}: J {errJ:.1e}, c_l {errc:.1e}, dJ/drho {errg:.1e}, central differences {errd:.1e} "
          f"(state {res.last_info['state']['iterations']}, adjoint {res.last_info['adjoint']['iterations']} iterations)")
    assert errJ <= 1e-10
    assert errg <= 1e-6
    assert errd <= 1e-5


def test_form_products_and_caching(gpu):
    """The residual vanishes at the solved state; dR/du and dR/drho against the restatement; forward mode against the reverse
    product; M is reassembled only when the density, the mass density or the law changed."""
    from femo_amd.engine import Vec
    from femo_amd.fea.fea_hip import dirichletbc
    P = problem("cube4j", "RAMP", "du_olhoff")
    mesh, mask, L = P["mesh"], P["mask"], len(P["shifts"])
    sim, res, _ = _harmonic_model(P, False, pc="jacobi")
    sim.run()
    n = res.n_dof
    U = np.asarray(sim['displacements']).reshape(L, n)
    r = _columns(res.assemble_vector(), L)
    for l, sg in enumerate(P["shifts"]):                              # the residual form at the solved state
        S = hr.shifted(P["K"], P["M"], sg)
        assert np.linalg.norm(r[l, mask == 0]) <= 1e-12 * (abs(S).sum(axis=0).max() * np.linalg.norm(U[l]) + np.linalg.norm(P["F"]))
    dev = res.dynamic()
    calls = []
    real = dev.mass_assemble
    dev.mass_assemble = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    res.dynamic(); res.assemble_vector()
    assert calls == []                                                # cached
    res.rho.vector[:] = P["rho"]                                      # a new version of the density
    res.dynamic()
    assert calls == [1]
    res.density = 2.0 * P["density"]
    res.dynamic()
    assert calls == [1, 1]
    res.density = P["density"]
    res.dynamic()
    # the operators
    rng = np.random.default_rng(2)
    A = res.new_matrix()
    x = rng.standard_normal(L * n)
    y = _columns(A.mult(Vec(gpu, L * n).set(x), Vec(gpu, L * n)), L)
    want = np.stack([hr.shifted(P["K"], P["M"], sg) @ x.reshape(L, n)[l] for l, sg in enumerate(P["shifts"])])
    assert _maxrel(y, want) <= 1e-13
    S = A.to_scipy()
    assert _maxrel(S @ x, want.ravel()) <= 1e-12
    D = res.partial_matrix(res.rho)
    dvec, w = rng.standard_normal(mesh.n_cell), rng.standard_normal(L * n)
    fwd = np.array(D.mult(Vec(gpu, mesh.n_cell).set(dvec), Vec(gpu, L * n)).get())
    rev = np.array(D.multTranspose(Vec(gpu, L * n).set(w), Vec(gpu, mesh.n_cell)).get())
    assert abs(w @ fwd - dvec @ rev) <= 1e-12 * np.linalg.norm(w) * np.linalg.norm(fwd)
    G = hr.response_gradients(mesh.x, mesh.conn, P["rho"], U, P["shifts"], P["method"], P["law"], P["density"])
    revu = np.array(D.multTranspose(Vec(gpu, L * n).set(-U.ravel()), Vec(gpu, mesh.n_cell)).get())   # -sum_l u_l^T dR_l/drho
    assert _maxrel(revu, G.sum(axis=0)) <= 1e-8                       # twice the bound of the state


def test_form_raises_when_a_column_does_not_converge(gpu):
    from femo_amd.fea.fea_hip import dirichletbc
    import re
    P = problem("square9j", "SIMP", "linear")
    sim, res, _ = _harmonic_model(P, False, pc="jacobi")
    res.max_it = 5
    with pytest.raises(RuntimeError, match=r"column 0 of 5, omega = 0\)"):
        sim.run()
    its = restated("square9j", "SIMP", "linear")["iterations"]
    assert max(its[:3]) + 4 <= 147 <= its[3] - 4                      # the first three columns make it, the fourth does not
    res.max_it = 147
    om = np.sqrt(P["shifts"][3])
    with pytest.raises(RuntimeError, match=re.escape(f"column 3 of 5, omega = {om:.6g})")):
        sim.run()


# ------------------------------------------------------------------------------------------------ limits and errors ----
def test_refusals(gpu):
    import types
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DynamicCompliance, HarmonicElasticityResidual
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    P = problem("rect8x4", "SIMP", "linear")
    mesh = P["mesh"]
    dev, rv = _device(gpu, P, fixed=False, mass=False)
    n, nc = dev.n_dof, mesh.n_cell
    big, y, cells = Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(1.0), Vec(gpu, (ELAST_MAX_COLS + 1) * n), Vec(gpu, nc)
    one = np.ones(ELAST_MAX_COLS + 1)
    with pytest.raises(FemoError, match="assemble M"):
        dev.dyn_apply_multi(2, one[:2], big, y)
    with pytest.raises(FemoError, match="assemble M"):
        dev.dyn_solve_multi(2, one[:2], big, y)
    with pytest.raises(FemoError, match="mass law"):
        dev.mass_assemble(rv, mass_law="lumped")
    dev.mass_assemble(rv)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.dyn_apply_multi(bad, one[:bad], big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.dyn_solve_multi(bad, one[:bad], big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.mass_drho_multi(True, bad, one[:bad], rv, big, big, cells)
    with pytest.raises(FemoError, match="as many shifts"):
        dev.dyn_apply_multi(3, one[:2], big, y)
    with pytest.raises(FemoError, match="shifts"):
        dev.dyn_apply_multi(2, [1.0, -1e-3], big, y)
    with pytest.raises(FemoError, match="shifts"):
        dev.dyn_solve_multi(2, [np.nan, 1.0], big, y)
    with pytest.raises(FemoError, match="fixed set"):
        dev.dyn_apply_multi(2, one[:2], big, y, masked=True)
    with pytest.raises(FemoError, match="differ"):
        dev.dyn_apply_multi(2, one[:2], y, y)
    with pytest.raises(FemoError):
        dev.dyn_apply_multi(3, one[:3], Vec(gpu, 3 * n - 1), y)
    with pytest.raises(FemoError, match="aliases"):
        dev.mass_drho_multi(False, 2, one[:2], rv, big, cells, big)
    with pytest.raises(FemoError, match="mass law"):
        dev.mass_drho_multi(True, 2, one[:2], rv, big, big, cells, mass_law="lumped")
    with pytest.raises(ValueError):
        dev.dyn_solve_multi(2, one[:2], big, y, pc="ilu")
    with pytest.raises(FemoError, match="multilevel"):
        dev.dyn_solve_multi(2, one[:2], big, y, pc="multilevel")      # no pc_setup
    # the forms
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    u, rho = Function(LoadCaseSpace(V, 2)), Function(Q)
    t = [(0.0, -1.0)] * 2
    ok = dict(omegas=[0.0, 1.0])
    with pytest.raises(ValueError, match="omega"):
        HarmonicElasticityResidual(u, rho, t, omegas=[1.0, -0.5])
    with pytest.raises(ValueError, match="omega"):
        HarmonicElasticityResidual(u, rho, t)
    with pytest.raises(ValueError):
        HarmonicElasticityResidual(u, rho, t, omegas=[1.0, 2.0, 3.0])
    with pytest.raises(NotImplementedError, match="body forces"):
        HarmonicElasticityResidual(u, rho, t, body_forces=[(0.0, -1.0), None], **ok)
    with pytest.raises(ValueError, match="traction"):
        HarmonicElasticityResidual(u, rho, [(0.0, -1.0), None], **ok)
    with pytest.raises(NotImplementedError):
        HarmonicElasticityResidual(Function(V), rho, t[:1], omegas=[1.0])            # not a LoadCaseSpace state
    with pytest.raises(NotImplementedError):
        HarmonicElasticityResidual(u, Function(V), t, **ok)                           # the density is DG0
    with pytest.raises(ValueError, match="mass law"):
        HarmonicElasticityResidual(u, rho, t, mass_law="lumped", **ok)
    with pytest.raises(ValueError):
        HarmonicElasticityResidual(u, rho, t, preconditioner="ilu", **ok)
    res = HarmonicElasticityResidual(u, rho, t, **ok)
    dofs = np.nonzero(P["mask"])[0].astype(np.int32)
    with pytest.raises(NotImplementedError, match="inhomogeneous"):
        res.solve_state(u, [dirichletbc(0.5, dofs, V)])
    part = types.SimpleNamespace(local=types.SimpleNamespace(nranks=2))
    Sp = LoadCaseSpace(VectorFunctionSpace(mesh), 2)
    up = Function(Sp)
    Sp.mesh = part
    with pytest.raises(NotImplementedError, match="partitioned"):
        HarmonicElasticityResidual(up, rho, t, **ok)
    with pytest.raises(NotImplementedError, match="partitioned"):
        DynamicCompliance(up, t)
    with pytest.raises(ValueError, match="weights"):
        DynamicCompliance(u, t, weights=[1.0])
    with pytest.raises(NotImplementedError):
        DynamicCompliance(Function(V), t[:1])
