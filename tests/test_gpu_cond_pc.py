"""GPU tests of the lattice preconditioner of the penalised heat conduction solves (csrc/conduction.hip: k_cond_pc_diag and the
wiring, csrc/bpx.hip: pc_prepare; `preconditioner="multilevel"` of femo_amd/fea/conduction.py) against the restatement
tests/cond_pc_ref.py: the level weights, the operator, the solves through the form, the iteration counts, operators solved
alternately on one mesh, the thermoelastic chain, and the refusals.

The Galerkin diagonals are summed with fp64 atomics, and so are the node sums of the lattice restriction: nothing that goes
through the lattice path is compared bit for bit, here or in tests/test_gpu_bpx.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cond_pc_ref as cr
import cond_pc_stock as stock
import nonfinite as nf
import thermal_ref as tr
from cond_pc_ref import K0, K_MIN
from oracle import bpx_oracle as bo
from oracle import femo_oracle as fo
from thermal_ref import MESHES, mesh as _mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _assembled(gpu, mesh, rho, method="SIMP", with_sink=True, dev=None):
    """(handle, restated operator) of K_theta(rho) on `mesh`, the sink on x = 0 or no Dirichlet set.  The restatement takes the
    matrix from the device: its diagonal enters the single-precision scaling of the mesh transfers, where a last-bit
    difference of the assembly would show as 6e-8."""
    from femo_amd import _lib
    from femo_amd.engine import DirichletSet, Vec
    from femo_amd.fea.conduction import DeviceConduction
    dev = dev or DeviceConduction(gpu, mesh)
    sink = cr.sink_of(mesh)
    bc = DirichletSet(mesh.device(gpu), sink, np.zeros(len(sink))) if with_sink else None
    dev.assemble(_lib.ELAST_SIMP if method == "SIMP" else _lib.ELAST_RAMP, K0, K_MIN, Vec(gpu, mesh.n_cell).set(rho), bc)
    pinned = cr.pinned_mask(mesh.n_vert, sink) if with_sink else None
    M = cr.WeightedBPX(mesh.x, mesh.conn, tr.conductivity(rho, K0, K_MIN, method), None, pinned,
                       A=dev.export_csr(eliminated=with_sink))
    return dev, M


def _check_weights(dev, M, label):
    info = dev.pc_info()
    assert info["levels"] == M.levels and info["nodes"] == [int(np.prod(n + 1)) for n in M.bins], (label, info)
    for l in range(M.levels):
        got, want = dev.pc_level_weights(l), M.coef[l]
        assert np.array_equal(got == 0.0, want == 0.0), f"{label} level {l}: the zeros differ"
        nz = want != 0.0
        err = (np.abs(got - want)[nz] / np.abs(want)[nz]).max() if nz.any() else 0.0
        print(f"{label} level {l}: {len(want)} nodes, {int((~nz).sum())} zero, weights {err:.1e} from the restatement")
        assert err <= 1e-11


def _check_apply(gpu, dev, M, n_vert, label):
    """The bar of test_gpu_bpx.py::test_pc_apply_matches_the_oracle_operator."""
    from femo_amd.engine import Vec
    rng = np.random.default_rng(4)
    R, Z = Vec(gpu, n_vert), Vec(gpu, n_vert)
    zs = []
    for k in range(2):
        r = rng.standard_normal(n_vert)
        z = np.array(dev.pc_apply(R.set(r), Z).get())
        want = M.apply(r)
        err = np.abs(z - want).max() / np.abs(want).max()
        print(f"{label}: apply {k} {err:.1e} from the restatement")
        assert err < 1e-12
        zs.append((r, z))
    (r0, z0), (r1, z1) = zs
    assert abs(r1 @ z0 - r0 @ z1) < 1e-12 * abs(r1 @ z0)              # <r1, M^-1 r0> = <r0, M^-1 r1>


# ------------------------------------------------------------------------------------------------------ the weights ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_weights(gpu, name, method):
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev, M = _assembled(gpu, mesh, rho, method)
    before = dev.pc_info()["builds"]
    _check_weights(dev, M, f"{name} {method}")
    assert dev.pc_info()["builds"] == before + 1                      # one build serves every level and every later call


# -------------------------------------------------------------------------------------------------------- the apply ----
@pytest.mark.parametrize("with_sink", [True, False])
@pytest.mark.parametrize("name", MESHES)
def test_apply(gpu, name, with_sink):
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev, M = _assembled(gpu, mesh, rho, "SIMP", with_sink)
    _check_apply(gpu, dev, M, mesh.n_vert, f"{name} sink={with_sink}")


def test_apply_through_the_fused_lattice_cycle(gpu):
    """unit_square_mesh(110, 0.2): the smallest mesh on which the apply runs its fused lattice cycle (tests/test_gpu_bpx.py)."""
    from femo_amd.fea.mesh import Mesh
    m = fo.unit_square_mesh(110, 0.2)
    mesh = Mesh(m.x, m.conn)
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev, M = _assembled(gpu, mesh, rho)
    assert M.levels == 6
    _check_weights(dev, M, "square 110")
    _check_apply(gpu, dev, M, mesh.n_vert, "square 110")


def test_apply_and_solve_where_the_merged_loop_runs(gpu):
    """The jittered cube of 27^3 cells is the smallest on which BPX-PCG solves take the merged loop (four lattice levels: the
    26^3 one has three).  The apply there, and a solve, which reads the weighted arrays in the merged kernels."""
    from femo_amd.engine import Vec
    from femo_amd.fea.mesh import createUnitCubeMesh
    assert not createUnitCubeMesh(26, 0.2).device(gpu).pcg_info()["merged"]
    mesh = createUnitCubeMesh(27, 0.2)
    assert mesh.device(gpu).pcg_info()["merged"]
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev, M = _assembled(gpu, mesh, rho)
    _check_apply(gpu, dev, M, mesh.n_vert, "cube 27")
    b = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    b[cr.sink_of(mesh)] = 0.0
    B, X, Xj = Vec(gpu, mesh.n_vert).set(b), Vec(gpu, mesh.n_vert), Vec(gpu, mesh.n_vert)
    info = dev.solve(B, X, pc="multilevel")
    jac = dev.solve(B, Xj, pc="jacobi")
    _, want = bo.pcg(M.A, b, M, rtol=1e-13)
    err = _maxrel(np.array(X.get()), np.array(Xj.get()))
    print(f"cube 27: merged loop {info.iterations} iterations (restatement {want}), Jacobi {jac.iterations}, solutions {err:.1e} apart")
    assert info.converged == 1 and jac.converged == 1
    assert info.iterations <= 1.1 * want + 2
    assert err <= 1e-9


# ------------------------------------------------------------------------------------------------------- the solves ----
SINK_VALUE = 0.75


@functools.lru_cache(maxsize=None)
def state_ref(name, method):
    mesh = _mesh(name)
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    K = tr.conduction_matrix(mesh.x, mesh.conn, tr.conductivity(rho, K0, K_MIN, method))
    Q = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    sink = cr.sink_of(mesh)
    return dict(rho=rho, K=K, Q=Q, sink=sink, T=tr.solve_lifted(K, Q, sink, np.full(len(sink), SINK_VALUE)))


def _form(mesh, method="SIMP", source=1.0, preconditioner="multilevel"):
    from femo_amd.fea.conduction import ConductionResidual
    from femo_amd.fea.function import Function, FunctionSpace
    T, rho = Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0)))
    return ConductionResidual(T, rho, source=source, k0=K0, k_min=K_MIN, method=method, preconditioner=preconditioner), T, rho


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_state_and_adjoint(gpu, name, method):
    """The state with a non-zero sink temperature (the lifting) and the adjoint through the matrix of the form, to the
    tolerance tests/test_gpu_conduction.py::test_state has for Jacobi."""
    from femo_amd.engine import Vec
    from femo_amd.fea.utils_hip import LAST_KSP_INFO, dirichletbc
    mesh = _mesh(name)
    R = state_ref(name, method)
    form, T, rho = _form(mesh, method)
    bcs = [dirichletbc(SINK_VALUE, R["sink"], T.function_space)]
    rho.vector[:] = R["rho"]
    builds = form.device().pc_info()["builds"]
    form.solve_state(T, bcs)
    info = form.last_info["state"]
    err = _maxrel(np.array(T.vec.get()), R["T"])
    assert info["converged"] == 1 and info["preconditioner"] == "multilevel"
    assert LAST_KSP_INFO[-1]["kind"] == "conduction_state" and LAST_KSP_INFO[-1]["preconditioner"] == "multilevel"
    assert err <= 1e-9
    A, _ = form.assemble_system(bcs, False, None, None)
    b = np.random.default_rng(3).standard_normal(mesh.n_vert)
    xv = Vec(gpu, mesh.n_vert)
    A.backend_solve(Vec(gpu, mesh.n_vert).set(b), xv)
    want = tr.solve_lifted(R["K"], b, R["sink"])
    want[R["sink"]] = b[R["sink"]]
    ad = form.last_info["adjoint"]
    print(f"{name} {method}: state {info['iterations']} iterations, T {err:.1e}; adjoint {ad['iterations']} iterations, "
          f"{_maxrel(np.array(xv.get()), want):.1e}")
    assert ad["converged"] == 1 and ad["preconditioner"] == "multilevel"
    assert _maxrel(np.array(xv.get()), want) <= 1e-9
    assert form.device().pc_info()["builds"] == builds + 1            # the state and the adjoint solve share one build


# ------------------------------------------------------------------------------------------------------- the counts ----
@pytest.mark.parametrize("kind", ["uniform", "truss"])
@pytest.mark.parametrize("nelx,factor", [(80, 4), (160, 8)])
def test_iteration_counts(gpu, nelx, factor, kind):
    """The device count against the restatement's with the margin tests/test_gpu_elast_pc.py gives a preconditioner whose
    diagonals are summed with atomics, and the Jacobi count of the same handle against it: the restatement has 321 / 39,
    460 / 64 (80 x 40) and 633 / 43, 995 / 78 (160 x 80), ratios 8.2, 7.2, 14.7 and 12.8; the bounds stand well under them."""
    from femo_amd.engine import Vec
    case = cr.count_case(nelx, nelx // 2, kind)
    mesh = case["mesh"]
    dev, _ = _assembled(gpu, mesh, case["rho"])
    B, X, Xj = Vec(gpu, mesh.n_vert).set(case["b"]), Vec(gpu, mesh.n_vert), Vec(gpu, mesh.n_vert)
    info = dev.solve(B, X, rtol=cr.COUNT_RTOL, pc="multilevel")
    jac = dev.solve(B, Xj, rtol=cr.COUNT_RTOL, pc="jacobi")
    want = cr.count_iterations(nelx, nelx // 2, kind, "weighted")
    print(f"{nelx}x{nelx // 2} {kind}: lattice {info.iterations} iterations in {info.solve_ms:.2f} ms (restatement {want}), "
          f"Jacobi {jac.iterations} in {jac.solve_ms:.2f} ms")
    assert info.converged == 1 and jac.converged == 1
    assert info.iterations <= 1.1 * want + 2
    assert jac.iterations >= factor * info.iterations
    assert _maxrel(np.array(X.get()), np.array(Xj.get())) <= 1e-9


# ----------------------------------------------------------------------------------------------- change of operator ----
def test_second_density_on_the_same_handle(gpu):
    from femo_amd.engine import Vec
    mesh = _mesh("rect24x12")
    rng = np.random.default_rng(11)
    rho1, rho2 = rng.uniform(0.05, 1.0, mesh.n_cell), rng.uniform(0.05, 1.0, mesh.n_cell)
    b = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    b[cr.sink_of(mesh)] = 0.0
    B = Vec(gpu, mesh.n_vert).set(b)
    dev, _ = _assembled(gpu, mesh, rho1)
    X1 = Vec(gpu, mesh.n_vert)
    assert dev.solve(B, X1, pc="multilevel").converged == 1
    dev, M2 = _assembled(gpu, mesh, rho2, dev=dev)
    X2 = Vec(gpu, mesh.n_vert)
    i2 = dev.solve(B, X2, pc="multilevel")
    fresh, _ = _assembled(gpu, mesh, rho2)
    Xf = Vec(gpu, mesh.n_vert)
    i_f = fresh.solve(B, Xf, pc="multilevel")
    assert i2.converged == 1 and i_f.converged == 1 and i2.iterations == i_f.iterations
    assert _maxrel(np.array(X2.get()), np.array(Xf.get())) <= 1e-12
    assert _maxrel(np.array(X1.get()), np.array(X2.get())) > 1e-3    # the two densities are different problems
    _check_weights(dev, M2, "second density")


def test_stock_solve_between_two_conduction_solves(gpu, tmp_path):
    """A weighted and a stock operator solved alternately on one mesh each see their own weights: the Poisson BPX solve
    between two conduction solves has the iteration count and the solution of the same solve in a process that never made
    a conduction handle (to 1e-12: the stock path repeats to the rounding of its atomics, tests/test_gpu_bpx.py)."""
    from femo_amd.engine import Vec
    mesh = stock.stock_mesh()
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    dev, M = _assembled(gpu, mesh, rho)
    b = tr.heat_load(mesh.x, mesh.conn, source=1.0)
    b[cr.sink_of(mesh)] = 0.0
    B, X1, X2 = Vec(gpu, mesh.n_vert).set(b), Vec(gpu, mesh.n_vert), Vec(gpu, mesh.n_vert)
    i1 = dev.solve(B, X1, pc="multilevel")
    it, conv, u = stock.stock_solve(gpu, mesh)
    i2 = dev.solve(B, X2, pc="multilevel")
    out = tmp_path / "stock.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cond_pc_stock.py"), str(out)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    alone = np.load(out)
    print(f"stock Poisson BPX: {it} iterations between the conduction solves, {int(alone['iterations'])} alone, solutions "
          f"{_maxrel(u, alone['u']):.1e} apart; conduction {i1.iterations} and {i2.iterations} iterations")
    assert conv == 1 and int(alone["converged"]) == 1
    assert it == int(alone["iterations"])
    assert _maxrel(u, alone["u"]) <= 1e-12
    # ... and the conduction solve behind it found its own weights again
    assert i1.converged == 1 and i2.converged == 1 and i1.iterations == i2.iterations
    assert _maxrel(np.array(X2.get()), np.array(X1.get())) <= 1e-12
    _check_weights(dev, M, "after the stock solve")


# -------------------------------------------------------------------------------------------------------- the chain ----
def build_cycle(device, objective, nelx=16, nely=8):
    """build_cycle of tests/test_gpu_thermoelastic_cycle.py with the lattice preconditioner on the conduction form."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, ThermalExpansion,
                                      VectorFunctionSpace, displacement, locate_dofs_geometrical, mean_displacement, meshtags,
                                      pdeRes_conduction)
    from femo_amd.fea.elasticity import compliance, pdeRes
    mesh, facets, h_avg, sink = tr.cycle_case(nelx, nely)
    ds = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    Q, P, V = FunctionSpace(mesh, ('DG', 0)), FunctionSpace(mesh, ('CG', 1)), VectorFunctionSpace(mesh, ('CG', 1))
    on_clamp = lambda x: np.isclose(x[0], 0., atol=1e-6)

    thermal = FEA(mesh)
    thermal.REPORT = False
    thermal.consistent_bc_partials = True
    rho_t, T = Function(Q), Function(P)
    res_t = pdeRes_conduction(T, TestFunction(P), rho_t, source=tr.SOURCE, k0=1.0, k_min=1e-3, preconditioner="multilevel")
    thermal.add_input('density', rho_t)
    thermal.add_state(name='temperature', function=T, residual_form=res_t, arguments=['density'])
    Tbc = Function(P)
    Tbc.vector.set(0.0)
    thermal.add_strong_bc(Tbc, [locate_dofs_geometrical((P, P), on_clamp)], P)

    elastic = FEA(mesh)
    elastic.REPORT = False
    elastic.consistent_bc_partials = True
    rho_e, T_in, u = Function(Q), Function(P), Function(V)
    f = Constant(mesh, tr.TRACTION)
    th = ThermalExpansion(tr.ALPHA, T_in)
    res_e = pdeRes(u, TestFunction(V), rho_e, f, dss=ds, thermal=th)
    elastic.add_input('density', rho_e)
    elastic.add_input('temperature', T_in)
    elastic.add_state(name='displacements', function=u, residual_form=res_e, arguments=['density', 'temperature'])
    ell = None
    if objective == "compliance":
        elastic.add_output(name='objective', type='scalar', form=compliance(u, f, dss=ds, rho_e=rho_e, thermal=th),
                           arguments=['displacements', 'density', 'temperature'])
    else:
        ell = mean_displacement(V, (0.0, -1.0), ds)
        elastic.add_output(name='objective', type='scalar', form=displacement(u, ell), arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    elastic.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), on_clamp)], V)

    model = FEAModel(fea=[thermal, elastic])
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    model.add_objective('objective')
    aux = dict(facets=facets, h_avg=h_avg, sink=sink, res_t=res_t, res_e=res_e, ell=ell)
    return Simulator(model, device=device), mesh, aux


@pytest.mark.parametrize("objective", ["compliance", "displacement"])
def test_thermoelastic_cycle(gpu, objective):
    sim, mesh, aux = build_cycle(True, objective)
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    R = tr.reference_cycle_thermoelastic(mesh, aux['facets'], tr.TRACTION, aux['h_avg'], x0, tr.ALPHA, tr.SOURCE, aux['sink'],
                                         objective=objective, ell=aux['ell'])
    err_T = _maxrel(np.asarray(sim['temperature']), R['T'])
    err_u = _maxrel(np.asarray(sim['displacements']), R['u'])
    err_J = abs(float(sim['objective'][0]) - R['J']) / abs(R['J'])
    g = np.asarray(sim.compute_totals('objective', 'density_unfiltered'))
    err_g = _maxrel(g, R['grad'])
    it = aux['res_t'].last_info
    print(f"thermoelastic 16x8 cantilever, J = {objective}, lattice preconditioner on the conduction form: T {err_T:.1e}, "
          f"u {err_u:.1e}, J {err_J:.1e}, total {err_g:.1e}; conduction PCG {it['state']['iterations']} + "
          f"{it['adjoint']['iterations']} it")
    assert it['state']['preconditioner'] == "multilevel" and it['adjoint']['preconditioner'] == "multilevel"
    assert err_T <= 1e-9
    assert err_u <= 1e-9
    assert err_J <= 1e-9
    assert err_g <= 1e-8


# ------------------------------------------------------------------------------------- refusals and non-finite inputs ----
def test_refusals(gpu):
    from femo_amd import _lib
    from femo_amd._lib import FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.conduction import ConductionResidual, DeviceConduction, pdeRes_conduction
    from femo_amd.fea.function import Function, FunctionSpace
    import ctypes as C
    mesh = _mesh("rect8x4")
    T, rho = Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0)))
    with pytest.raises(ValueError, match="preconditioner"):
        ConductionResidual(T, rho, source=1.0, preconditioner="bpx")
    with pytest.raises(ValueError, match="preconditioner"):
        pdeRes_conduction(T, None, rho, source=1.0, preconditioner="ilu")
    dev = DeviceConduction(gpu, mesh)
    x, y = Vec(gpu, mesh.n_vert).fill(1.0), Vec(gpu, mesh.n_vert)
    with pytest.raises(FemoError, match="before"):
        dev.pc_apply(x, y)
    with pytest.raises(FemoError, match="before"):
        dev.pc_level_weights(0)
    dev.assemble(0, 1.0, 1e-3, Vec(gpu, mesh.n_cell).fill(0.5))
    with pytest.raises(ValueError, match="preconditioner"):
        dev.solve(x, y, pc="bpx")
    with pytest.raises(ValueError, match="level"):
        dev.pc_level_weights(dev.pc_info()["levels"])
    with pytest.raises(FemoError, match="aliasing"):
        dev.pc_apply(x, x)
    opts = _lib.SolverOpts(1e-13, 0.0, 100, 1, 8, 2, 0.0)                # pc = 2: no such preconditioner
    with pytest.raises(FemoError, match="preconditioner"):
        _lib.check(dev.lib.femo_cond_solve(dev.handle, x.handle, y.handle, C.byref(opts), C.byref(_lib.SolveInfo())))


@pytest.mark.parametrize("value", nf.VALUES)
def test_nonfinite(gpu, value):
    """The loop of tests/test_gpu_conduction.py::test_nonfinite with the lattice path: a non-finite density or source is
    refused, and the next clean call gives the clean solution -- to 1e-12, not bit for bit: the Galerkin diagonals and the
    lattice restriction are summed with atomics, so two clean solves differ in the last bits too."""
    from femo_amd.fea.conduction import ConductionResidual
    from femo_amd.fea.function import Function, FunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh("rect24x12")
    nc = mesh.n_cell
    T, rho, q = (Function(FunctionSpace(mesh, ("CG", 1))), Function(FunctionSpace(mesh, ("DG", 0))),
                 Function(FunctionSpace(mesh, ("DG", 0))))
    form = ConductionResidual(T, rho, source=q, k0=K0, k_min=K_MIN, method="RAMP", preconditioner="multilevel")
    bcs = [dirichletbc(0.0, cr.sink_of(mesh), T.function_space)]
    rh = np.random.default_rng(7).uniform(0.1, 1.0, nc)
    qc = np.ones(nc)
    rho.vector[:] = rh
    q.vector[:] = qc
    form.solve_state(T, bcs)
    clean = np.array(T.vec.get())
    want = tr.solve_lifted(tr.conduction_matrix(mesh.x, mesh.conn, tr.conductivity(rh, K0, K_MIN, "RAMP")),
                           tr.heat_load(mesh.x, mesh.conn, source=qc), cr.sink_of(mesh))
    assert _maxrel(clean, want) <= 1e-9
    for fn, good in ((rho, rh), (q, qc)):
        for c in nf.cell_positions(nc):
            fn.vector[:] = nf.poison(good, c, value)
            with pytest.raises(RuntimeError):
                form.solve_state(T, bcs)
            fn.vector[:] = good
            form.solve_state(T, bcs)
            assert form.last_info["state"]["converged"] == 1
            assert _maxrel(np.array(T.vec.get()), clean) <= 1e-12
