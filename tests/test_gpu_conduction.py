"""GPU tests of the heat conduction with a penalised conductivity (csrc/conduction.hip, femo_amd/fea/conduction.py) against
the restatement tests/thermal_ref.py, on the meshes of tests/test_gpu_elast_thermal.py."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import nonfinite as nf
import thermal_ref as tr
from thermal_ref import MESHES, mesh as _mesh

pytestmark = pytest.mark.gpu

K0, K_MIN = 1.0, 1e-3


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _sink(mesh):
    """The vertices on x = 0 (the fan: its hub and the ring points above and below it)."""
    return np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0].astype(np.int32)


def _patch_set(mesh, name):
    """Where the linear field is imposed: the two x-faces of a box, the outer ring of the fan (no flat faces there)."""
    x = mesh.x
    if name == "fan40x8":
        r = np.linalg.norm(x, axis=1)
        return np.nonzero(r >= r.max() - 1e-9)[0].astype(np.int32)
    return np.nonzero(np.isclose(x[:, 0], x[:, 0].min()) | np.isclose(x[:, 0], x[:, 0].max()))[0].astype(np.int32)


def _forms(mesh, method="SIMP", source=1.0, k_min=K_MIN):
    from femo_amd.fea.conduction import ConductionResidual
    from femo_amd.fea.function import Function, FunctionSpace
    T, rho = Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0)))
    return ConductionResidual(T, rho, source=source, k0=K0, k_min=k_min, method=method), T, rho


# ------------------------------------------------------------------------------------------------------ the matrix ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_matrix(gpu, name, method):
    from femo_amd import _lib
    from femo_amd.engine import DirichletSet, Vec
    from femo_amd.fea.conduction import DeviceConduction
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev = DeviceConduction(gpu, mesh)
    sink = _sink(mesh)
    bc = DirichletSet(mesh.device(gpu), sink, np.zeros(len(sink)))
    mid = _lib.ELAST_SIMP if method == "SIMP" else _lib.ELAST_RAMP
    dev.assemble(mid, K0, K_MIN, Vec(gpu, mesh.n_cell).set(rho), bc)
    K, A = dev.export_csr(), dev.export_csr(eliminated=True)
    want = tr.conduction_matrix(mesh.x, mesh.conn, tr.conductivity(rho, K0, K_MIN, method))
    err = abs(K - want).max() / abs(want).max()
    print(f"{name} {method}: K_theta against the restatement {err:.1e}")
    assert err <= 1e-13
    assert abs(K - K.T).max() == 0.0 and abs(A - A.T).max() == 0.0                          # symmetric bit for bit
    free = np.ones(mesh.n_vert)
    free[sink] = 0.0
    wantA = sp.diags(free) @ want @ sp.diags(free) + sp.diags(1.0 - free)
    assert abs(A - wantA).max() <= 1e-13 * abs(want).max()
    assert np.all(A.diagonal()[sink] == 1.0) and abs(A[sink]).sum() == len(sink)
    # the same bits on a second build, and without a Dirichlet set
    dev.assemble(mid, K0, K_MIN, Vec(gpu, mesh.n_cell).set(rho), None)
    assert abs(dev.export_csr() - K).max() == 0.0
    # the products
    xh = np.random.default_rng(1).standard_normal(mesh.n_vert)
    y = np.array(dev.apply(Vec(gpu, mesh.n_vert).set(xh), Vec(gpu, mesh.n_vert)).get())
    assert np.abs(y - want @ xh).max() <= 1e-13 * np.abs(want @ xh).max()


@pytest.mark.parametrize("name", MESHES)
def test_unit_conductivity_is_the_poisson_operator(gpu, name):
    from femo_amd import _lib
    from femo_amd import engine as E
    from femo_amd.fea.conduction import DeviceConduction
    mesh = _mesh(name)
    dm = mesh.device(gpu)
    dev = DeviceConduction(gpu, mesh)
    dev.assemble(_lib.ELAST_SIMP, 1.0, 0.0, E.Vec(gpu, mesh.n_cell).fill(1.0), None)
    K = dev.export_csr()
    P = E.assemble_jacobian(dm, _lib.PDE_POISSON, None, None, None, None, E.Mat(dm)).to_scipy()
    err = abs(K - P).max() / abs(P).max()
    print(f"{name}: k = 1 against the Poisson Jacobian {err:.1e}")
    assert err <= 1e-14


# ---------------------------------------------------------------------------------------------------------- solves ----
@pytest.mark.parametrize("name", MESHES)
def test_patch(gpu, name):
    """Uniform rho, no source, T = 2 + 3 x imposed: the solve returns it at every vertex (the lifting with non-zero values)."""
    from femo_amd.fea.function import Function
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh(name)
    form, T, rho = _forms(mesh, source=0.0)
    rho.vector[:] = np.full(mesh.n_cell, 0.6)
    g = 2.0 + 3.0 * mesh.x[:, 0]
    on = _patch_set(mesh, name)
    gf = Function(T.function_space)
    gf.vector[:] = g
    form.solve_state(T, [dirichletbc(gf, on, T.function_space)])
    info = form.last_info["state"]
    err = np.abs(np.array(T.vec.get()) - g).max()
    print(f"{name}: patch test {err:.1e} after {info['iterations']} iterations")
    assert info["converged"] == 1
    assert err <= 1e-10


@functools.lru_cache(maxsize=None)
def state_ref(name, method, k):
    mesh = _mesh(name)
    rho = np.random.default_rng(7 + k).uniform(0.05, 1.0, mesh.n_cell)
    K = tr.conduction_matrix(mesh.x, mesh.conn, tr.conductivity(rho, K0, K_MIN, method))
    Q = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    return dict(rho=rho, K=K, Q=Q, T=tr.solve_lifted(K, Q, _sink(mesh)))


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_state(gpu, name, method):
    """Random rho in [0.05, 1], k_min = 1e-3, uniform source, the sink T = 0 on x = 0; two successive densities."""
    from femo_amd.engine import Vec
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh(name)
    form, T, rho = _forms(mesh, method)
    bcs = [dirichletbc(0.0, _sink(mesh), T.function_space)]
    for k in (0, 1):
        R = state_ref(name, method, k)
        rho.vector[:] = R["rho"]
        form.solve_state(T, bcs)
        info = form.last_info["state"]
        err = _maxrel(np.array(T.vec.get()), R["T"])
        print(f"{name} {method} density {k}: {info['iterations']} Jacobi-PCG iterations, T {err:.1e}")
        assert info["converged"] == 1
        assert err <= 1e-9
    assert _maxrel(np.array(form.load().get()), R["Q"]) <= 1e-14
    th = np.random.default_rng(2).standard_normal(mesh.n_vert)
    T.vector[:] = th
    res = np.array(form.assemble_vector(Vec(gpu, mesh.n_vert)).get())
    want = R["K"] @ th - R["Q"]
    assert np.abs(res - want).max() <= 1e-12 * np.abs(want).max()
    # the adjoint solve through the matrix of the form: the eliminated operator, identity on the sink
    A, _ = form.assemble_system(bcs, False, None, None)
    b = np.random.default_rng(3).standard_normal(mesh.n_vert)
    xv = Vec(gpu, mesh.n_vert)
    A.backend_solve(Vec(gpu, mesh.n_vert).set(b), xv)
    lam = np.array(xv.get())
    sink = _sink(mesh)
    want = tr.solve_lifted(R["K"], b, sink)                          # K_ff lam_f = b_f: the columns of the sink are eliminated
    want[sink] = b[sink]
    assert form.last_info["adjoint"]["converged"] == 1
    assert _maxrel(lam, want) <= 1e-9


def test_load_with_flux_and_cell_source(gpu):
    from femo_amd.fea.conduction import ConductionResidual, ThermalCompliance
    from femo_amd.fea.elasticity import Measure, meshtags
    from femo_amd.fea.function import Function, FunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    mesh = _mesh("cube4j")
    face = locate_entities_boundary(mesh, 2, lambda x: np.isclose(x[0], mesh.x[:, 0].max()))
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 2, face, np.full(len(face), 7, dtype=np.int32)))(7)
    T, rho, q = (Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0))),
                 Function(FunctionSpace(mesh, ("DG", 0))))
    qc = np.random.default_rng(5).uniform(0.0, 2.0, mesh.n_cell)
    q.vector[:] = qc
    form = ConductionResidual(T, rho, source=q, flux=0.75, ds=ds)
    want = tr.heat_load(mesh.x, mesh.conn, source=qc, flux=0.75, facets=face)
    assert _maxrel(np.array(form.load().get()), want) <= 1e-14
    q.vector[:] = 2.0 * qc                                           # a written source reaches the load
    want2 = tr.heat_load(mesh.x, mesh.conn, source=2.0 * qc, flux=0.75, facets=face)
    assert _maxrel(np.array(form.load().get()), want2) <= 1e-14
    th = np.random.default_rng(6).standard_normal(mesh.n_vert)
    T.vector[:] = th
    J = ThermalCompliance(T, source=q, flux=0.75, ds=ds)
    assert J.functions() == (T,)
    assert abs(J.assemble_scalar() - want2 @ th) <= 1e-13 * np.linalg.norm(want2) * np.linalg.norm(th)
    assert _maxrel(np.array(J.assemble_derivative(T).get()), want2) <= 1e-14
    assert np.all(np.array(J.assemble_derivative(rho).get()) == 0.0)


# ------------------------------------------------------------------------------------------------------- dR/drho ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_drho(gpu, name, method):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    nc, nv = mesh.n_cell, mesh.n_vert
    form, T, rho = _forms(mesh, method)
    rng = np.random.default_rng(9)
    rh, Th, dr, xv = rng.uniform(0.05, 1.0, nc), rng.standard_normal(nv), rng.standard_normal(nc), rng.standard_normal(nv)
    rho.vector[:] = rh
    T.vector[:] = Th
    D = form.partial_matrix(rho)
    assert D.getSizes() == (nv, nc)
    Dd = np.array(D.mult(Vec(gpu, nc).set(dr), Vec(gpu, nv)).get())
    DTx = np.array(D.multTranspose(Vec(gpu, nv).set(xv), Vec(gpu, nc)).get())
    e1 = _maxrel(Dd, tr.conduction_drho(mesh.x, mesh.conn, rh, Th, dr, K0, K_MIN, method))
    e2 = _maxrel(DTx, tr.conduction_drho_T(mesh.x, mesh.conn, rh, Th, xv, K0, K_MIN, method))
    a, b = xv @ Dd, dr @ DTx
    print(f"{name} {method}: dR/drho d {e1:.1e}, dR/drho^T x {e2:.1e}; x.(D d) = {a:.15e}, d.(D^T x) = {b:.15e}")
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert abs(a - b) <= 1e-13 * np.linalg.norm(xv) * np.linalg.norm(Dd)
    assert np.array_equal(np.array(D.mult(Vec(gpu, nc).set(dr), Vec(gpu, nv)).get()), Dd)  # the same bits again
    dev = form.device()
    acc = Vec(gpu, nc).set(DTx)
    dev.drho(form.method_id, K0, K_MIN, True, rho.vec, T.vec, Vec(gpu, nv).set(xv), acc, a=-2.0, accumulate=True)
    assert np.abs(np.array(acc.get()) + DTx).max() <= 1e-13 * np.abs(DTx).max()


# -------------------------------------------------------------------------------------------------------- refusals ----
def test_refusals(gpu):
    from femo_amd._lib import FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.conduction import ConductionResidual, DeviceConduction, ThermalCompliance
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    mesh, other = _mesh("rect8x4"), _mesh("square9j")
    P, Q = FunctionSpace(mesh, ("CG", 1)), FunctionSpace(mesh, ("DG", 0))
    T, rho = Function(P), Function(Q)
    with pytest.raises(NotImplementedError):
        ConductionResidual(Function(VectorFunctionSpace(mesh)), rho, source=1.0)
    with pytest.raises(NotImplementedError):
        ConductionResidual(T, Function(FunctionSpace(other, ("DG", 0))), source=1.0)
    with pytest.raises(NotImplementedError):
        ConductionResidual(T, rho, source=Function(P))
    with pytest.raises(ValueError, match="source or a flux"):
        ConductionResidual(T, rho)
    with pytest.raises(ValueError, match="source or a flux"):
        ThermalCompliance(T)
    for bad in (dict(k0=0.0), dict(k_min=-1.0), dict(k0=np.inf), dict(k0=1.0, k_min=1.0)):
        with pytest.raises(ValueError, match="k_min"):
            ConductionResidual(T, rho, source=1.0, **bad)
    with pytest.raises(ValueError, match="method"):
        ConductionResidual(T, rho, source=1.0, method="linear")
    dev = DeviceConduction(gpu, mesh)
    x, y, r = Vec(gpu, mesh.n_vert).fill(1.0), Vec(gpu, mesh.n_vert), Vec(gpu, mesh.n_cell).fill(0.5)
    with pytest.raises(FemoError, match="before"):
        dev.apply(x, y)
    with pytest.raises(FemoError, match="before"):
        dev.solve(x, y)
    with pytest.raises(FemoError, match="shorter"):
        dev.assemble(0, 1.0, 0.0, Vec(gpu, mesh.n_cell - 1))
    with pytest.raises(FemoError, match="k_min"):
        dev.assemble(0, 1.0, 2.0, r)
    dev.assemble(0, 1.0, 1e-3, r)
    with pytest.raises(FemoError, match="Dirichlet set"):
        dev.apply(x, y, eliminated=True)
    with pytest.raises(FemoError, match="Dirichlet set"):
        dev.lift(x, y)
    with pytest.raises(FemoError, match="aliasing"):
        dev.apply(x, x)
    with pytest.raises(FemoError, match="size"):
        dev.drho(0, 1.0, 1e-3, False, r, x, x, y)                    # the forward product reads a cell vector
    with pytest.raises(FemoError, match="aliases"):
        dev.drho(0, 1.0, 1e-3, True, r, x, x, r)


# ------------------------------------------------------------------------------------------------ non-finite inputs ----
@pytest.mark.parametrize("value", nf.VALUES)
def test_nonfinite(gpu, value):
    """No output hides a non-finite state: the solve with a non-finite density or source raises, the thermal compliance of a
    non-finite load is non-finite, the density products carry a poisoned entry where the restatement has it and nowhere
    else, and after a refused call the next clean call gives the clean bits."""
    from femo_amd.engine import Vec
    from femo_amd.fea.conduction import ConductionResidual, ThermalCompliance
    from femo_amd.fea.function import Function, FunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh("rect24x12")
    x, conn, nc, nv = mesh.x, mesh.conn, mesh.n_cell, mesh.n_vert
    T, rho, q = (Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0))),
                 Function(FunctionSpace(mesh, ("DG", 0))))
    form = ConductionResidual(T, rho, source=q, k0=K0, k_min=K_MIN, method="RAMP")
    J = ThermalCompliance(T, source=q)
    bcs = [dirichletbc(0.0, _sink(mesh), T.function_space)]
    rh = np.random.default_rng(7).uniform(0.1, 1.0, nc)
    qc = np.ones(nc)
    rho.vector[:] = rh
    q.vector[:] = qc
    form.solve_state(T, bcs)
    clean, J0 = np.array(T.vec.get()), J.assemble_scalar()
    assert np.isfinite(J0)
    for fn, good in ((rho, rh), (q, qc)):
        for c in nf.cell_positions(nc):
            fn.vector[:] = nf.poison(good, c, value)
            with pytest.raises(RuntimeError):
                form.solve_state(T, bcs)
            fn.vector[:] = good
            form.solve_state(T, bcs)
            assert np.array_equal(np.array(T.vec.get()), clean)
    q.vector[:] = nf.poison(qc, 5, value)
    assert not np.isfinite(J.assemble_scalar())
    q.vector[:] = qc
    assert J.assemble_scalar() == J0
    # the density products
    rng = np.random.default_rng(3)
    dr, xv = rng.standard_normal(nc), rng.standard_normal(nv)
    dev = form.device()

    def device(r, t):
        rv, tv = Vec(gpu, nc).set(r), Vec(gpu, nv).set(t)
        return (np.array(dev.drho(form.method_id, K0, K_MIN, False, rv, tv, Vec(gpu, nc).set(dr), Vec(gpu, nv)).get()),
                np.array(dev.drho(form.method_id, K0, K_MIN, True, rv, tv, Vec(gpu, nv).set(xv), Vec(gpu, nc)).get()))

    def restated(r, t):
        with np.errstate(all="ignore"):
            return (tr.conduction_drho(x, conn, r, t, dr, K0, K_MIN, "RAMP"), tr.conduction_drho_T(x, conn, r, t, xv, K0, K_MIN, "RAMP"))

    base = device(rh, clean)
    bad = []
    for c in nf.cell_positions(nc):
        cells = nf.one_cell(nc, c)
        got, want = device(nf.poison(rh, c, value), clean), restated(nf.poison(rh, c, value), clean)
        bad += nf.violations(got[0], want[0], base[0], nf.entries_of_cells(conn, cells, nv), label=f"rho[{c}] forward")
        bad += nf.violations(got[1], want[1], base[1], cells, label=f"rho[{c}] reverse")
    for e in nf.positions(conn, 1):
        cells = nf.cells_of_vertex(conn, e)
        got, want = device(rh, nf.poison(clean, e, value)), restated(rh, nf.poison(clean, e, value))
        bad += nf.violations(got[0], want[0], base[0], nf.entries_of_cells(conn, cells, nv), label=f"T[{e}] forward")
        bad += nf.violations(got[1], want[1], base[1], cells, label=f"T[{e}] reverse")
    assert not bad, "\n".join(bad)
