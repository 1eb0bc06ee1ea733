"""GPU tests of the batched multi-load path of the SIMP elasticity (csrc/elast_solve.hip, the step of csrc/elast_pc.hip
with several columns, MultiLoadElasticityResidual / MultiLoadCompliance) against the one-column launches of the same
kernels and the restatements (tests/elasticity_ref.py, tests/elast_pc_ref.py, tests/elast_multi_ref.py).

The meshes are small on purpose: less than one wave of rows (rect8x4), the three meshes of the preconditioner tests, and
two with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343), so that the per-column folds of the
partial sums cross blocks.  L = 1, 3, 5 covers one column, a chunk that is not full, and a second pass of the product
(4 + 1 columns)."""
import functools

import numpy as np
import pytest

import elast_multi_ref as mr
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import L_X, L_Y, clamped_face
from elast_multi_ref import cantilever_loads, right_hand_sides

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _mesh(name):
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    return pr.small_meshes()[name]()


@functools.lru_cache(maxsize=None)
def case(name):
    """Mesh, density, mask, the five right-hand sides and the restatement of one mesh: built once, read only."""
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask)
    B = right_hand_sides(mesh, mask)
    B.setflags(write=False)
    return dict(mesh=mesh, rho=rho, mask=mask, M=M, B=B)


@functools.lru_cache(maxsize=None)
def direct(name, l):
    c = case(name)
    u = ref.solve_fixed(c["M"].A, c["B"][l], np.nonzero(c["mask"])[0], g=c["B"][l])
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def ref_count(name, pc, l):
    c = case(name)
    M = c["M"]
    _, n_ref, ok = pr.pcg(M.A, c["B"][l], M.jacobi if pc == "jacobi" else M.apply, c["mask"])
    assert ok
    return n_ref


def _device(gpu, name, setup=True):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    c = case(name)
    dev = DeviceElasticity(gpu, c["mesh"], 1.0, 0.3)
    dev.set_fixed(c["mask"])
    rv = Vec(gpu, c["mesh"].n_cell).set(c["rho"])
    dev.assemble(METHODS["SIMP"], rv)
    if setup:
        dev.pc_setup()
    return dev, rv


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("name", MESHES)
def test_apply_multi(gpu, name, L):
    from femo_amd.engine import Vec
    c = case(name)
    dev, _ = _device(gpu, name, setup=False)
    n = dev.n_dof
    K = dev.export_csr()
    free = (c["mask"] == 0).astype(np.float64)
    X = np.random.default_rng(3).standard_normal((L, n))
    Fh = np.random.default_rng(4).standard_normal((L, n))
    xv, fv, yv = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(Fh.ravel()), Vec(gpu, L * n)
    x1, f1, y1 = Vec(gpu, n), Vec(gpu, n), Vec(gpu, n)
    for masked in (False, True):
        dev.apply_multi(L, xv, yv, masked=masked, a=1.5, b=-0.5, f=fv)
        Y = _columns(yv, L)
        for l in range(L):
            x1.set(X[l]); f1.set(Fh[l])
            dev.apply(x1, y1, masked=masked, a=1.5, b=-0.5, f=f1)
            ys = np.array(y1.get())
            Kx = free * (K @ (free * X[l])) + (1.0 - free) * X[l] if masked else K @ X[l]
            yr = 1.5 * Kx - 0.5 * Fh[l]
            e1 = np.abs(Y[l] - ys).max() / np.abs(ys).max()
            e2 = np.abs(Y[l] - yr).max() / np.abs(yr).max()
            print(f"{name} L={L} masked={masked} column {l}: vs single {e1:.1e}, vs SciPy {e2:.1e}")
            assert e1 <= 1e-14
            assert e2 <= 1e-13                                        # summation order of a row of at most ~30 blocks
        dev.apply_multi(L, xv, yv, masked=masked, a=1.5, b=-0.5, f=fv)
        assert np.array_equal(_columns(yv, L), Y)                     # the same bits again
        dev.apply_multi(L, xv, yv, masked=masked)                     # f = None
        assert np.abs(_columns(yv, L)[L - 1] - (Y[L - 1] + 0.5 * Fh[L - 1]) / 1.5).max() <= 1e-13 * np.abs(Y).max()


@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("name", MESHES)
def test_solve_multi(gpu, name, pc, L):
    from femo_amd.engine import Vec
    c = case(name)
    dev, _ = _device(gpu, name)
    n = dev.n_dof
    bv, xv = Vec(gpu, L * n).set(c["B"][:L].ravel()), Vec(gpu, L * n)
    infos = dev.solve_multi(L, bv, xv, rtol=1e-15, pc=pc)
    X = _columns(xv, L)
    b1, x1 = Vec(gpu, n), Vec(gpu, n)
    for l in range(L):
        single = dev.solve(b1.set(c["B"][l]), x1, rtol=1e-15, pc=pc)
        u, n_ref = direct(name, l), ref_count(name, pc, l)
        err = np.abs(X[l] - u).max() / max(np.abs(u).max(), 1e-300)
        print(f"{name} {pc} L={L} column {l}: batched {infos[l].iterations} it, single-column {single.iterations} it, "
              f"restatement {n_ref} it, error {err:.1e}, batched solve {infos[l].solve_ms:.2f} ms")
        assert infos[l].converged == 1
        assert np.abs(X[l] - u).max() <= 1e-9 * np.abs(u).max()
        assert infos[l].iterations <= 1.1 * n_ref + 2
    if L >= 3:
        assert infos[2].iterations == 0 and np.all(X[2] == 0.0)      # the zero column: finished at the start, exactly zero
    if L >= 4:
        assert np.abs(X[3] - 1e6 * X[0]).max() <= 1e-9 * np.abs(X[3]).max()
    assert len({i.solve_ms for i in infos}) == 1                      # the time of the whole batched solve in every record


def test_frozen_column(gpu):
    """A restart from the converged x.  The stopping test is absolute here (rtol = 0, atol = 1e-8 of the smaller
    right-hand-side norm): relative to a restart's own initial residual no column could be finished at the start.  The true
    residual of the converged x differs from the recurrence residual by rounding, orders below the 1e-8, so every column
    meets the test at iteration 0 or after one more step, and is frozen there."""
    from femo_amd.engine import Vec
    c = case("rect24x12")
    dev, _ = _device(gpu, "rect24x12")
    L, n, M = 3, dev.n_dof, c["M"]
    atol = 1e-8 * min(np.sqrt(c["B"][l] @ M.apply(c["B"][l])) for l in (0, 1))
    bv, xv = Vec(gpu, L * n).set(c["B"][:L].ravel()), Vec(gpu, L * n)
    first = dev.solve_multi(L, bv, xv, rtol=0.0, atol=atol, pc="multilevel")
    X = _columns(xv, L)
    again = dev.solve_multi(L, bv, xv, rtol=0.0, atol=atol, pc="multilevel", zero_guess=False)
    X2 = _columns(xv, L)
    print(f"first {[i.iterations for i in first]}, restart {[i.iterations for i in again]}, "
          f"change {np.abs(X2 - X).max() / np.abs(X).max():.1e}")
    assert all(i.converged == 1 for i in first) and first[0].iterations > 1 and first[1].iterations > 1
    for l in range(L):
        assert again[l].converged == 1 and again[l].iterations in (0, 1)
        assert np.abs(X2[l] - X[l]).max() <= 1e-12 * max(np.abs(X[l]).max(), 1e-300)


def test_breakdown_is_per_column(gpu):
    """A NaN in the data of column 1: that column reports the breakdown, its neighbours converge as if it were not there."""
    from femo_amd.engine import Vec
    c = case("square9j")
    dev, _ = _device(gpu, "square9j")
    L, n = 3, dev.n_dof
    B = c["B"][:L].copy()
    B[1, np.nonzero(c["mask"] == 0)[0][5]] = np.nan
    bv, xv = Vec(gpu, L * n).set(B.ravel()), Vec(gpu, L * n)
    for pc in ("jacobi", "multilevel"):
        infos = dev.solve_multi(L, bv, xv, rtol=1e-15, pc=pc)
        X = _columns(xv, L)
        assert infos[1].converged == -1
        for l in (0, 2):
            u = direct("square9j", l)
            assert infos[l].converged == 1
            assert np.abs(X[l] - u).max() <= 1e-9 * np.abs(u).max()
            assert infos[l].iterations <= 1.1 * ref_count("square9j", pc, l) + 2


def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    dev, _ = _device(gpu, "rect8x4", setup=False)
    n = dev.n_dof
    big = (ELAST_MAX_COLS + 1) * n
    b, x = Vec(gpu, big).fill(0.0), Vec(gpu, big)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.solve_multi(bad, b, x)
        with pytest.raises(FemoError, match="columns"):
            dev.apply_multi(bad, b, x)
    with pytest.raises(FemoError, match="femo_elast_pc_setup"):
        dev.solve_multi(2, b, x, pc="multilevel")
    with pytest.raises(ValueError):
        dev.solve_multi(2, b, x, pc="ilu")
    short = Vec(gpu, 3 * n - 1)
    with pytest.raises(FemoError):
        dev.solve_multi(3, b, short)
    with pytest.raises(FemoError):
        dev.apply_multi(3, short, x)
    assert all(i.converged == 1 for i in dev.solve_multi(2, b, x))   # Jacobi needs no set-up


@pytest.mark.parametrize("name", ["rect8x4", "cube4j"])
def test_drho_multi_transpose(gpu, name):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    c = case(name)
    dev, rv = _device(gpu, name, setup=False)
    L, n, nc = 3, dev.n_dof, c["mesh"].n_cell
    rng = np.random.default_rng(8)
    U, X, dr = rng.standard_normal((L, n)), rng.standard_normal((L, n)), rng.standard_normal(nc)
    uv, xv, drv = Vec(gpu, L * n).set(U.ravel()), Vec(gpu, L * n).set(X.ravel()), Vec(gpu, nc).set(dr)
    yn, yt = Vec(gpu, L * n), Vec(gpu, nc)
    m = METHODS["SIMP"]
    Dy = _columns(dev.drho_multi(m, False, L, rv, uv, drv, yn), L)                 # D dr, one column per load
    DTx = np.array(dev.drho_multi(m, True, L, rv, uv, xv, yt).get())               # D^T x, summed over the loads
    a, b = np.sum(X * Dy), dr @ DTx
    print(f"{name}: x.(D y) = {a:.15e}, y.(D^T x) = {b:.15e}")
    assert abs(a - b) <= 1e-13 * abs(a)
    u1, x1, y1, t1 = Vec(gpu, n), Vec(gpu, n), Vec(gpu, n), Vec(gpu, nc)
    tsum = np.zeros(nc)
    for l in range(L):
        u1.set(U[l]); x1.set(X[l])
        fwd = np.array(dev.drho(m, False, rv, u1, drv, y1).get())
        assert np.abs(Dy[l] - fwd).max() <= 1e-13 * np.abs(fwd).max()
        tsum += np.array(dev.drho(m, True, rv, u1, x1, t1).get())
    assert np.abs(DTx - tsum).max() <= 1e-13 * np.abs(tsum).max()
    dev.drho_multi(m, True, L, rv, uv, xv, yt, accumulate=True)
    assert np.abs(np.array(yt.get()) - 2.0 * DTx).max() <= 1e-13 * np.abs(DTx).max()


WEIGHTS = (1.0, 0.5, 2.0)


def build_multiload(device, nelx=16, nely=8):
    """The L_X x L_Y cantilever with three load cases through FEAModel + GeneralFilterModel + Simulator."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, TestFunction,
                                      VectorFunctionSpace, compliance_multiload, createRectangleMesh,
                                      locate_dofs_geometrical, meshSize, meshtags, pdeRes_multiload)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    facets, tractions = cantilever_loads(mesh, L_X, L_Y, nely)
    dss = [Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, f, np.full(len(f), 100 + l, dtype=np.int32)))(100 + l)
           for l, f in enumerate(facets)]
    fs = [Constant(mesh, t) for t in tractions]
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    S = LoadCaseSpace(V, len(fs))
    rho_fn, u_fn = Function(Q), Function(S)
    res = pdeRes_multiload(u_fn, TestFunction(V), rho_fn, fs, dss, preconditioner="multilevel")
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance_multiload(u_fn, fs, dss, weights=WEIGHTS),
                   arguments=['displacements'])
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
    return Simulator(model, device=device), mesh, dict(facets=facets, tractions=tractions, h_avg=h_avg, res=res, space=S)


@pytest.mark.parametrize("device", [False, True])
def test_multiload_cycle(gpu, device):
    """16 x 8 cantilever, three loads, weights (1, 0.5, 2), multilevel: the tolerances of test_cantilever_cycle_multilevel."""
    sim, mesh, aux = build_multiload(device)
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    R = mr.reference_cycle_multi(mesh, aux['facets'], aux['tractions'], WEIGHTS, aux['h_avg'], x0)
    assert np.abs(np.asarray(sim['density']) - R['rho']).max() <= 1e-14
    u = np.asarray(sim['displacements'])
    S = aux['space']
    for l in range(S.n_cases):
        assert np.abs(u[S.column(l)] - R['u'][l]).max() <= 1e-9 * np.abs(R['u'][l]).max()
    assert abs(float(sim['compliance'][0]) - R['J']) <= 1e-9 * abs(R['J'])
    g = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    assert np.abs(g - R['grad']).max() <= 1e-8 * np.abs(R['grad']).max()
    res = aux['res']
    info = res.last_info
    print(f"16x8 cantilever, 3 loads: state PCG {info['state']['iterations']} it, adjoint {info['adjoint']['iterations']} it")
    assert res.solve_counts == {"state": 1, "adjoint": 1}            # one batched solve each, not one per load
    for kind in ("state", "adjoint"):
        assert len(info[kind]['columns']) == 3 and info[kind]['converged'] == [1, 1, 1]
        assert info[kind]['preconditioner'] == "multilevel"
    # forward mode against the reverse product: w . (dR/drho d) = d . (dR/drho^T w)
    op = [o for _, o in sim.ops if hasattr(o, 'apply_inverse_jacobian')][0]
    rng = np.random.default_rng(2)
    d, w = rng.standard_normal(mesh.n_cell), rng.standard_normal(S.dim)
    ins, outs = {'density': np.asarray(sim['density'])}, {'displacements': u}
    d_res = {'displacements': np.zeros(S.dim)}
    op.compute_jacvec_product(ins, outs, {'density': d}, {}, d_res, 'fwd')
    d_in = {'density': np.zeros(mesh.n_cell)}
    op.compute_jacvec_product(ins, outs, d_in, {}, {'displacements': w}, 'rev')
    a, b = w @ np.asarray(d_res['displacements']), d @ np.asarray(d_in['density'])
    print(f"w.(D d) = {a:.15e}, d.(D^T w) = {b:.15e}")
    assert abs(a - b) <= 1e-12 * abs(a)
    # the forward-mode solve is one batched solve as well
    d_o = {'displacements': np.zeros(S.dim)}
    op.apply_inverse_jacobian(d_o, {'displacements': np.asarray(d_res['displacements'])}, 'fwd')
    assert res.solve_counts["adjoint"] == 2 and np.all(np.isfinite(np.asarray(d_o['displacements'])))


def test_multiload_error_names_the_column(gpu):
    from femo_amd.fea.elasticity import MultiLoadElasticityResidual
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _mesh("rect8x4")
    V = VectorFunctionSpace(mesh)
    u, rho = Function(LoadCaseSpace(V, 2)), Function(FunctionSpace(mesh, ("DG", 0)))
    form = MultiLoadElasticityResidual(u, rho, [np.zeros(2), np.zeros(2)])
    bad = [type("I", (), dict(iterations=3, converged=c, residual_norm=1.0, rhs_norm=2.0, solve_ms=0.1))() for c in (1, 0)]
    with pytest.raises(RuntimeError, match="load case 1 of 2"):
        form._record(bad, "state")
    with pytest.raises(ValueError):
        MultiLoadElasticityResidual(u, rho, [np.zeros(2)])
    with pytest.raises(NotImplementedError):
        MultiLoadElasticityResidual(Function(V), rho, [np.zeros(2)])


def test_single_column_unchanged(gpu):
    """The batched path shares K, the fixed set and the Galerkin blocks with the single-column one and leaves them alone."""
    from femo_amd.engine import Vec
    c = case("square9j")
    dev, _ = _device(gpu, "square9j")
    n = dev.n_dof
    b1, x1 = Vec(gpu, n).set(c["B"][1]), Vec(gpu, n)
    bv, xv = Vec(gpu, 3 * n).set(c["B"][:3].ravel()), Vec(gpu, 3 * n)
    for pc in ("jacobi", "multilevel"):
        before = dev.solve(b1, x1, rtol=1e-15, pc=pc)
        xb, builds = np.array(x1.get()), dev.pc_info()["builds"]
        assert all(i.converged == 1 for i in dev.solve_multi(3, bv, xv, rtol=1e-15, pc=pc))
        after = dev.solve(b1, x1, rtol=1e-15, pc=pc)
        assert after.iterations == before.iterations
        assert np.array_equal(np.array(x1.get()), xb)
        assert dev.pc_info()["builds"] == builds == (1 if pc == "multilevel" else 0)   # built lazily, once, by dev.solve


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_work_vectors_grow(gpu, name):
    """One set of PCG and lattice work vectors serves every column count: it grows at 3 and at 5 columns, serves 3 again
    below its capacity, and the one-column solves and preconditioner applications in between keep their bits."""
    from femo_amd.engine import Vec
    c = case(name)
    dev, _ = _device(gpu, name)
    n = dev.n_dof
    bytes_setup = dev.pc_plan["bytes"]
    per = sum(dev.pc_plan["nodes"]) * dev.d
    b1, x1 = Vec(gpu, n).set(c["B"][1]), Vec(gpu, n)
    rv, zv = Vec(gpu, n).set(np.random.default_rng(11).standard_normal(n)), Vec(gpu, n)
    bv, xv = Vec(gpu, 5 * n).set(c["B"].ravel()), Vec(gpu, 5 * n)
    PCS = ("jacobi", "multilevel")

    def single():
        out = []
        for pc in PCS:
            i = dev.solve(b1, x1, rtol=1e-15, pc=pc)
            assert i.converged == 1
            out.append((np.array(x1.get()), i.iterations))
        return out

    def apply():
        return np.array(dev.pc_apply(rv, zv).get())

    def multi(L):
        out = []
        for pc in PCS:
            infos = dev.solve_multi(L, bv, xv, rtol=1e-15, pc=pc)
            assert all(i.converged == 1 for i in infos)
            out.append((np.array(xv.get())[:L * n].reshape(L, n), [i.iterations for i in infos]))
        return out

    def same(a, b):
        return all(np.array_equal(xa, xb) and ia == ib for (xa, ia), (xb, ib) in zip(a, b))

    s1 = single()
    z1 = apply()
    m3 = multi(3)
    assert same(single(), s1)
    multi(5)
    assert dev.pc_info()["bytes"] == bytes_setup + 4 * 2 * per * 8   # five columns of g and e where one was
    assert same(multi(3), m3)
    assert same(single(), s1)
    assert np.array_equal(apply(), z1)
    assert dev.pc_info()["builds"] == 1


@pytest.mark.slow
def test_full_size_multi(gpu):
    """640 x 320, 4 load cases, multilevel: the batched solve against four sequential single-column solves."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    from femo_amd.fea.mesh import createRectangleMesh
    mesh = createRectangleMesh([0.0, 0.0], [L_X, L_Y], 640, 320)
    facets, tractions = cantilever_loads(mesh, L_X, L_Y, 320)
    facets.append(facets[1]); tractions.append((0.25, 0.0))           # a fourth load: shear on the loaded piece of the top edge
    mask = clamped_face(mesh)
    L, n = 4, 2 * mesh.n_vert
    B = np.stack([ref.traction_load(mesh.x, f, t) for f, t in zip(facets, tractions)])
    B[:, mask == 1] = 0.0
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    dev.set_fixed(mask)
    rv = Vec(gpu, mesh.n_cell).set(np.random.default_rng(2).uniform(0.3, 1.0, mesh.n_cell))
    dev.assemble(METHODS["SIMP"], rv)
    dev.pc_setup()
    bv, xv = Vec(gpu, L * n).set(B.ravel()), Vec(gpu, L * n)
    b1, x1, Kd = Vec(gpu, n), Vec(gpu, n), Vec(gpu, n)
    seq, seq_ms = [], 0.0
    for l in range(L):
        i = dev.solve(b1.set(B[l]), x1, pc="multilevel")
        assert i.converged == 1
        seq.append((np.array(x1.get()), i.iterations))
        seq_ms += i.solve_ms
    infos = dev.solve_multi(L, bv, xv, pc="multilevel")
    X = _columns(xv, L)
    print(f"640x320, 4 loads: batched {infos[0].solve_ms:.1f} ms ({[i.iterations for i in infos]} it), "
          f"sequential {seq_ms:.1f} ms ({[s[1] for s in seq]} it)")

    def knorm(v):
        b1.set(v)
        dev.apply(b1, Kd, masked=True)
        return np.sqrt(b1.dot(Kd, n))

    for l in range(L):
        assert infos[l].converged == 1
        assert knorm(X[l] - seq[l][0]) <= 1e-9 * knorm(seq[l][0])
