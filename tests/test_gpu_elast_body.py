"""GPU tests of the body loads of the SIMP elasticity (csrc/elast_body.hip, ``body_force`` / ``body_forces`` of the
residuals and compliances) against the restatement tests/elast_body_ref.py.

The meshes are those of tests/test_gpu_elast_multi.py: less than one wave of rows (rect8x4), the two jittered ones, and two
with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343).  L = 1, 3, 5 load cases with distinct body
forces, one of them zero."""
import functools

import numpy as np
import pytest

import elast_body_ref as br
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_multi_ref import cantilever_loads
from elast_pc_ref import L_X, L_Y, clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BODY = np.array([[0.3, -1.0, 0.7], [-2.5, 0.4, 0.1], [0.0, 0.0, 0.0], [0.0, 2.5, -1.0], [1.0, 0.0, 0.25]])
WEIGHTS = (1.0, 0.5, 2.0)
# The stopping level of the state solves below, on the device and in the restatement alike.  With a body load on these
# meshes the Jacobi-PCG is at its rounding floor well before 1e-15: the restatement reaches its final accuracy (1e-13 of the
# direct solve) at rtol = 1e-11 already, and below 1e-13 its recurrence residual falls in steps, so that its own iteration
# count moves by up to 20 % (rect24x12, case 0: 321 ... 393) when the right-hand side is perturbed by 1e-16 relative --
# more than the 10 % the count bound allows.  At 1e-13 the same perturbations move it by at most one iteration on every
# mesh, load and preconditioner used here, so the bound compares like with like.
RTOL = 1e-13
G = 1e-3                    # the weight of the 160 x 80 cantilever at mean density 0.43 is then about the tip load


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def _mesh(name):
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    return pr.small_meshes()[name]()


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------------------- the two kernels ----
@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("name", MESHES)
def test_body_apply(gpu, name, L):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh(name)
    d, nc = mesh.tdim, mesh.n_cell
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n = dev.n_dof
    B = BODY[:L, :d]
    rng = np.random.default_rng(12)
    w, X, base = rng.standard_normal(nc), rng.standard_normal((L, n)), rng.standard_normal((L, n))
    wv, xv, bv = Vec(gpu, nc).set(w), Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(base.ravel())
    yv, tv, w1, y1 = Vec(gpu, L * n), Vec(gpu, nc), Vec(gpu, nc), Vec(gpu, n)

    # G_B: cells to vertices
    Gw = np.stack([br.body_load(mesh.x, mesh.conn, w, B[l]) for l in range(L)])
    Y = _columns(dev.body_apply(L, B, wv, yv), L)
    err = np.abs(Y - Gw).max() / np.abs(Gw).max()
    print(f"{name} L={L}: G_B against the restatement {err:.1e}")
    assert err <= 1e-13                                               # sums over the at most ~30 cells around a vertex
    assert np.array_equal(_columns(dev.body_apply(L, B, wv, yv), L), Y)                  # the same bits again
    for l in range(L):
        assert np.array_equal(np.array(dev.body_apply(1, B[l:l + 1], wv, y1).get()), Y[l])   # independent of L
    if L >= 3:
        assert np.all(Y[2] == 0.0)                                    # the zero body force
    Ya = _columns(dev.body_apply(L, B, wv, yv, a=-1.5, base=bv), L)
    assert np.abs(Ya - (base - 1.5 * Gw)).max() <= 1e-13 * np.abs(base - 1.5 * Gw).max()
    Yb = _columns(dev.body_apply(L, B, wv, yv, a=0.5, accumulate=True), L)
    assert np.abs(Yb - (base - Gw)).max() <= 1e-13 * np.abs(base - Gw).max()
    # zero_fixed on the clamped face: exact zeros there, the free dofs untouched
    mask = clamped_face(mesh)
    dev.set_fixed(mask)
    Yz = _columns(dev.body_apply(L, B, wv, yv, a=-1.5, base=bv, zero_fixed=True), L)
    assert np.all(Yz[:, mask == 1] == 0.0) and np.array_equal(Yz[:, mask == 0], Ya[:, mask == 0])

    # G_B^T: vertices to cells
    GTx = sum(br.body_drho_T(mesh.x, mesh.conn, X[l], B[l]) for l in range(L))
    T = np.array(dev.body_apply(L, B, xv, tv, transpose=True).get())
    errT = np.abs(T - GTx).max() / np.abs(GTx).max()
    print(f"{name} L={L}: G_B^T against the restatement {errT:.1e}")
    assert errT <= 1e-13
    assert np.array_equal(np.array(dev.body_apply(L, B, xv, tv, transpose=True).get()), T)
    T2 = np.array(dev.body_apply(L, B, xv, tv, transpose=True, a=-2.0, accumulate=True).get())
    assert np.abs(T2 + GTx).max() <= 1e-13 * np.abs(GTx).max()
    # <x, G_B w> = <G_B^T x, w>
    lhs, rhs = np.sum(X * Y), T @ w
    print(f"{name} L={L}: x.(G w) = {lhs:.15e}, (G^T x).w = {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Y)


def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh("rect8x4")
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n, nc = dev.n_dof, mesh.n_cell
    w, y, t = Vec(gpu, nc).fill(1.0), Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(0.0), Vec(gpu, nc)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.body_apply(bad, np.zeros((bad, 2)), w, y)
    with pytest.raises(FemoError):
        dev.body_apply(3, np.zeros((2, 2)), w, y)                     # as many body forces as columns
    with pytest.raises(FemoError):
        dev.body_apply(3, np.zeros((3, 2)), w, Vec(gpu, 3 * n - 1))
    with pytest.raises(FemoError):
        dev.body_apply(2, np.zeros((2, 2)), Vec(gpu, nc - 1), y)
    with pytest.raises(FemoError):
        dev.body_apply(2, np.zeros((2, 2)), Vec(gpu, 2 * n - 1), t, transpose=True)
    with pytest.raises(FemoError, match="aliases"):
        dev.body_apply(2, np.zeros((2, 2)), y, y, transpose=True)
    with pytest.raises(FemoError, match="aliases"):
        dev.body_apply(2, np.zeros((2, 2)), w, y, base=y)
    with pytest.raises(FemoError, match="fixed set"):
        dev.body_apply(2, np.zeros((2, 2)), w, y, zero_fixed=True)
    with pytest.raises(FemoError, match="forward"):
        dev.body_apply(2, np.zeros((2, 2)), y, t, transpose=True, zero_fixed=True)
    assert np.all(np.array(dev.body_apply(ELAST_MAX_COLS, np.zeros((ELAST_MAX_COLS, 2)), w, y).get()) == 0.0)


# ----------------------------------------------------------------------------------------------------------- state ----
def _loads(mesh, load):
    """(facets, tractions, body forces) of the three load cases: with tractions (a pure body force, both, a pure traction)
    or body forces alone."""
    facets, tractions, bodies = br.body_cases(mesh)
    if load == "body":
        d = mesh.tdim
        return [None] * 3, [None] * 3, [tuple(BODY[l, :d]) for l in (0, 1, 3)]
    return facets, tractions, bodies


@functools.lru_cache(maxsize=None)
def state_ref(name, load, k):
    """Density k (0: the first, 1: after the change), its restatement solves and PCG counts: built once, read only."""
    mesh = _mesh(name)
    rho = np.random.default_rng(7 + k).uniform(0.05, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    facets, tractions, bodies = _loads(mesh, load)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, "RAMP", mask)
    K = ref.stiffness(mesh.x, mesh.conn, rho, "RAMP")
    F = br.total_loads(mesh, rho, facets, tractions, bodies)
    fixed = np.nonzero(mask)[0]
    u = [ref.solve_fixed(K, Fl, fixed) for Fl in F]
    counts = {}
    for pc in ("jacobi", "multilevel") if k == 0 else ():
        for l, Fl in enumerate(F):
            b = np.where(mask == 1, 0.0, Fl)
            _, it, ok = pr.pcg(M.A, b, M.jacobi if pc == "jacobi" else M.apply, mask, rtol=RTOL)
            assert ok
            counts[pc, l] = it
    return dict(rho=rho, mask=mask, K=K, F=F, u=u, counts=counts)


def _state_form(mesh, load, pc):
    from femo_amd.fea.elasticity import Measure, MultiLoadElasticityResidual, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    facets, tractions, bodies = _loads(mesh, load)
    d = mesh.tdim
    dss = [None if f is None else
           Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, f, np.full(len(f), 7, dtype=np.int32)))(7)
           for f in facets]
    V = VectorFunctionSpace(mesh)
    u, rho = Function(LoadCaseSpace(V, 3)), Function(FunctionSpace(mesh, ("DG", 0)))
    form = MultiLoadElasticityResidual(u, rho, tractions, dss, method="RAMP", preconditioner=pc, body_forces=bodies)
    return form, u, rho, [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]


@pytest.mark.parametrize("load", ["body", "body+traction"])
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("name", ["rect8x4", "cube4j", "rect24x12"])
def test_state(gpu, name, pc, load):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    form, u, rho, bcs = _state_form(mesh, load, pc)
    form.rtol = RTOL
    n = form.n_dof
    for k in (0, 1):                                                  # k = 1: a new density must reach the load and the rhs
        R = state_ref(name, load, k)
        rho.vector[:] = R["rho"]
        form.solve_state(u, bcs)
        info = form.last_info["state"]
        U = np.array(u.vec.get()).reshape(3, n)
        Fd = np.array(form.load().get()).reshape(3, n)
        for l in range(3):
            err, errF = _maxrel(U[l], R["u"][l]), _maxrel(Fd[l], R["F"][l])
            print(f"{name} {pc} {load} density {k} case {l}: {info['iterations'][l]} it"
                  f"{' (restatement %d)' % R['counts'][pc, l] if k == 0 else ''}, u {err:.1e}, F {errF:.1e}")
            assert info["converged"][l] == 1
            assert err <= 1e-9
            assert errF <= 1e-13
            if k == 0:
                assert info["iterations"][l] <= 1.1 * R["counts"][pc, l] + 2
    # the residual K u - F(rho) at a state that is not the solution
    uh = np.random.default_rng(2).standard_normal(3 * n)
    u.vector[:] = uh
    res = np.array(form.assemble_vector(Vec(gpu, 3 * n)).get()).reshape(3, n)
    for l in range(3):
        want = R["K"] @ uh.reshape(3, n)[l] - R["F"][l]
        assert np.abs(res[l] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", ["rect8x4", "cube4j", "rect24x12"])
def test_drho_with_body_forces(gpu, name, method):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import MultiLoadElasticityResidual
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _mesh(name)
    d, nc = mesh.tdim, mesh.n_cell
    _, tractions, bodies = br.body_cases(mesh)
    V = VectorFunctionSpace(mesh)
    u, rho = Function(LoadCaseSpace(V, 3)), Function(FunctionSpace(mesh, ("DG", 0)))
    form = MultiLoadElasticityResidual(u, rho, tractions, method=method, body_forces=bodies)
    n = form.n_dof
    rng = np.random.default_rng(9)
    rh, U, X, dr = rng.uniform(0.05, 1.0, nc), rng.standard_normal((3, n)), rng.standard_normal((3, n)), rng.standard_normal(nc)
    rho.vector[:] = rh
    u.vector[:] = U.ravel()
    D = form.partial_matrix(rho)
    assert D.getSizes() == (3 * n, nc)
    Dd = np.array(D.mult(Vec(gpu, nc).set(dr), Vec(gpu, 3 * n)).get()).reshape(3, n)
    DTx = np.array(D.multTranspose(Vec(gpu, 3 * n).set(X.ravel()), Vec(gpu, nc)).get())
    K0 = ref.element_matrices(mesh.x, mesh.conn)
    zero = np.zeros(d)
    want_T = np.zeros(nc)
    for l in range(3):
        b = zero if bodies[l] is None else bodies[l]
        want = br.drho_forward(mesh.x, mesh.conn, rh, U[l], dr, method, K0=K0) - br.body_load(mesh.x, mesh.conn, dr, b)
        err = _maxrel(Dd[l], want)
        print(f"{name} {method} case {l}: dR/drho d {err:.1e}")
        assert err <= 1e-12
        want_T += ref.compliance_gradient(mesh.x, mesh.conn, rh, U[l], X[l], method, K0=K0) - br.body_drho_T(mesh.x, mesh.conn, X[l], b)
    errT = _maxrel(DTx, want_T)
    a, b = np.sum(X * Dd), dr @ DTx
    print(f"{name} {method}: dR/drho^T x {errT:.1e}; x.(D d) = {a:.15e}, d.(D^T x) = {b:.15e}")
    assert errT <= 1e-12
    assert abs(a - b) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Dd)


# ------------------------------------------------------------------------------------------- the cycle of a Simulator ----
def _cycle_loads(mesh, n_cases, nely):
    facets, tractions = cantilever_loads(mesh, L_X, L_Y, nely)
    if n_cases == 1:                                                  # gravity beside the tip load
        return facets[:1], tractions[:1], [(0.0, -G)]
    # gravity beside the tip load; a 2.5 g pull-up without a traction; the end pull without a body force
    return [facets[0], None, facets[2]], [tractions[0], None, tractions[2]], [(0.0, -G), (0.0, -2.5 * G), None]


def build_cycle(device, n_cases, nelx=16, nely=8):
    """The L_X x L_Y cantilever with self-weight through FEAModel + GeneralFilterModel + Simulator."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, TestFunction,
                                      VectorFunctionSpace, compliance_multiload, createRectangleMesh,
                                      locate_dofs_geometrical, meshSize, meshtags, pdeRes_multiload)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    facets, tractions, bodies = _cycle_loads(mesh, n_cases, nely)
    dss = [None if f is None else
           Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, f, np.full(len(f), 100 + l, dtype=np.int32)))(100 + l)
           for l, f in enumerate(facets)]
    fs = [None if t is None else Constant(mesh, t) for t in tractions]
    fea = FEA(mesh)
    fea.REPORT = False
    fea.consistent_bc_partials = True          # F(rho) is non-zero on the clamped vertices, and so is the multiplier
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn = Function(Q)
    if n_cases == 1:
        u_fn = Function(V)
        res = pdeRes(u_fn, TestFunction(V), rho_fn, fs[0], dss=dss[0], body_force=bodies[0])
        J = compliance(u_fn, fs[0], dss=dss[0], body_force=bodies[0], rho_e=rho_fn)
    else:
        u_fn = Function(LoadCaseSpace(V, n_cases))
        res = pdeRes_multiload(u_fn, TestFunction(V), rho_fn, fs, dss, body_forces=bodies)
        J = compliance_multiload(u_fn, fs, dss, weights=WEIGHTS, body_forces=bodies, rho_e=rho_fn)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=J, arguments=['displacements', 'density'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    model.add_objective('compliance')
    aux = dict(facets=facets, tractions=tractions, bodies=bodies, h_avg=h_avg, res=res, n=V.dim)
    return Simulator(model, device=device), mesh, aux


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n_cases", [1, 3])
def test_body_cycle(gpu, n_cases, device):
    """16 x 8 cantilever with self-weight: the tolerances of test_cantilever_cycle."""
    sim, mesh, aux = build_cycle(device, n_cases)
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    w = None if n_cases == 1 else WEIGHTS
    R = br.reference_cycle_body(mesh, aux['facets'], aux['tractions'], aux['bodies'], w, aux['h_avg'], x0)
    assert np.abs(np.asarray(sim['density']) - R['rho']).max() <= 1e-14
    u = np.asarray(sim['displacements']).reshape(n_cases, aux['n'])
    err_u = max(_maxrel(u[l], R['u'][l]) for l in range(n_cases))
    err_J = abs(float(sim['compliance'][0]) - R['J']) / abs(R['J'])
    g = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    err_g = _maxrel(g, R['grad'])
    info = aux['res'].last_info
    print(f"16x8 cantilever with self-weight, {n_cases} case(s), device={device}: u {err_u:.1e}, J {err_J:.1e}, total {err_g:.1e}; "
          f"state PCG {info['state']['iterations']} it, adjoint {info['adjoint']['iterations']} it")
    assert err_u <= 1e-9
    assert err_J <= 1e-9
    assert err_g <= 1e-8
    if n_cases == 3:
        assert aux['res'].solve_counts == {"state": 1, "adjoint": 1}  # one batched solve each, not one per load case
    if not device:
        chk = sim.check_totals('compliance', 'density_unfiltered', step=1e-4, n_dir=3, seed=0)
        print(f"central differences: {chk['rel_error']}")
        assert max(chk['rel_error']) <= 1e-6, chk


# ------------------------------------------------------------------------------------------- no change when absent ----
def test_zero_body_force_changes_nothing(gpu):
    """body_force=None and an all-zero body force: the same bits in the load, the solution and the compliance gradient."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import Compliance, ElasticityResidual, Measure, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh("rect8x4")
    facets, tractions, _ = br.body_cases(mesh)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets[1], np.full(len(facets[1]), 7, dtype=np.int32)))(7)
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    rh = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    out = []
    for body in (None, (0.0, 0.0)):
        u, rho = Function(V), Function(Q)
        rho.vector[:] = rh
        form = ElasticityResidual(u, rho, tractions[1], ds, body_force=body)
        J = Compliance(u, tractions[1], ds, body_force=body, rho=rho)
        assert (form.body is None) == (body is None)
        form.solve_state(u, bcs)
        D = form.partial_matrix(rho)
        g = np.array(D.multTranspose(u.vec, Vec(gpu, mesh.n_cell)).get())
        out.append(dict(F=np.array(form.load().get()), u=np.array(u.vec.get()), it=form.last_info["state"]["iterations"],
                        J=J.assemble_scalar(), dJdu=np.array(J.assemble_derivative(u).get()),
                        dJdrho=np.array(J.assemble_derivative(rho).get()), g=g))
    a, b = out
    assert a["it"] == b["it"] and a["J"] == b["J"]
    for k in ("F", "u", "dJdu", "dJdrho", "g"):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a["dJdrho"] == 0.0) and np.abs(a["u"]).max() > 0.0
