"""GPU tests of the aggregated von Mises stress of the SIMP elasticity (csrc/elast_stress.hip: the one-column instantiations
of k_elast_stress_cell_multi and k_elast_stress_du_multi; femo_elast_pnorm_stress / femo_elast_von_mises) against the
restatement tests/elast_stress_ref.py: kernel parity, closed forms, the zero-stress guard, a non-finite state, bitwise
reproducibility, the projected field, and the 16 x 8 cantilever
through FEAModel + GeneralFilterModel + Simulator with the first adjoint right-hand side that is not the load."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import elast_stress_ref as sref
import elasticity_ref as ref
from test_elast_stress_host import L_X, L_Y, cantilever_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _meshes():
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh, createUnitSquareMesh
    return {"rect8x4": lambda: createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4),       # 64 cells: an under-filled block
            "square9j": lambda: createUnitSquareMesh(9, 0.25),                          # 162 cells, ragged
            "cube4j": lambda: createUnitCubeMesh(4, 0.2),                               # 384 cells: two blocks of 256
            "cube6j": lambda: createUnitCubeMesh(6, 0.2)}                               # 1296 cells, 343 vertices: two vertex blocks


def _device(ctx, mesh, rho, u):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    return DeviceElasticity(ctx, mesh), Vec(ctx, mesh.n_cell).set(rho), Vec(ctx, mesh.x.size).set(u)


def _all_three(ctx, dev, rv, uv, m, p, q, alpha):
    from femo_amd.engine import Vec
    gu, gr = Vec(ctx, uv.n), Vec(ctx, rv.n)
    J = dev.pnorm_stress(rv, uv, m, p, q, alpha, grad_u=gu, grad_rho=gr)
    return J, np.array(gu.get()), np.array(gr.get())


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j", "cube6j"])
@pytest.mark.parametrize("p,q", sref.PQ_CASES)
def test_kernel_parity(gpu, name, p, q):
    from femo_amd.engine import Vec
    mesh = _meshes()[name]()
    assert (name != "cube6j" or (mesh.n_cell, mesh.n_vert) == (1296, 343)) and (name != "cube4j" or mesh.n_cell == 384)
    u, rho, m = sref.random_inputs(mesh.x, mesh.conn, seed=5)
    R = sref.pnorm_stress(mesh.x, mesh.conn, rho, u, m, p, q)
    dev, rv, uv = _device(gpu, mesh, rho, u)
    J, du, drho = _all_three(gpu, dev, rv, uv, m, p, q, R["alpha"])
    field = np.array(dev.von_mises(uv, Vec(gpu, mesh.n_cell), rv, q).get())
    errs = dict(value=abs(J - R["value"]) / R["value"], du=np.abs(du - R["du"]).max() / np.abs(R["du"]).max(),
                field=np.abs(field - R["field"]).max() / np.abs(R["field"]).max())
    if q != 0.0:
        errs["drho"] = np.abs(drho - R["drho"]).max() / np.abs(R["drho"]).max()
    else:
        assert np.all(drho == 0.0)
        solid = np.array(dev.von_mises(uv, Vec(gpu, mesh.n_cell)).get())            # q = 0 needs no density
        assert np.array_equal(solid, field)
    print(f"{name} p={p} q={q}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12
    # accumulate = 1 adds onto what is there
    fill_u, fill_r = np.linspace(-1.0, 1.0, u.size), np.linspace(2.0, 3.0, rho.size)
    gu, gr = Vec(gpu, u.size).set(fill_u), Vec(gpu, rho.size).set(fill_r)
    assert dev.pnorm_stress(rv, uv, m, p, q, R["alpha"], value=False, grad_u=gu, grad_rho=gr, accumulate=True) is None
    assert np.abs(gu.get() - (fill_u + R["du"])).max() <= 1e-12 * max(np.abs(R["du"]).max(), 1.0)
    assert np.abs(gr.get() - (fill_r + R["drho"])).max() <= 1e-12 * max(np.abs(R["drho"]).max(), 3.0)
    # one output at a time: the same numbers as all three at once
    assert dev.pnorm_stress(rv, uv, m, p, q, R["alpha"]) == J
    only_u, only_r = Vec(gpu, u.size), Vec(gpu, rho.size)
    dev.pnorm_stress(rv, uv, m, p, q, R["alpha"], value=False, grad_u=only_u)
    dev.pnorm_stress(rv, uv, m, p, q, R["alpha"], value=False, grad_rho=only_r)
    assert np.array_equal(only_u.get(), du) and np.array_equal(only_r.get(), drho)


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_closed_forms(gpu, name):
    mesh = _meshes()[name]()
    rho = np.full(mesh.n_cell, 0.7)
    m, p, q = 3.0, 8.0, 0.5
    alpha = float(ref.cell_volumes(mesh.x, mesh.conn).sum())
    for label, A, vm in sref.closed_forms(mesh.tdim):
        dev, rv, uv = _device(gpu, mesh, rho, sref.linear_field(mesh.x, A))
        J = dev.pnorm_stress(rv, uv, m, p, q, alpha)
        exact = (m * 0.7 ** q * vm) ** p
        print(f"{name} {label}: J = {J:.16e}, exact {exact:.16e}, rel {abs(J - exact) / exact:.1e}")
        assert abs(J - exact) <= 1e-12 * exact


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_zero_displacement(gpu, name):
    """sigma_vm = 0 in every cell: the value and both partials are exactly zero, with no NaN from sigma_vm^(p-2)."""
    mesh = _meshes()[name]()
    rho = np.random.default_rng(1).uniform(1e-3, 1.0, mesh.n_cell)
    dev, rv, uv = _device(gpu, mesh, rho, np.zeros(mesh.x.size))
    for p, q in sref.PQ_CASES:
        J, du, drho = _all_three(gpu, dev, rv, uv, 2.0, p, q, 1.0)
        assert J == 0.0
        assert np.all(np.isfinite(du)) and np.all(du == 0.0) and np.all(np.isfinite(drho)) and np.all(drho == 0.0)


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_non_finite_state_shows_in_the_field(gpu, name):
    """One NaN entry of the state: NaN in exactly the cells that touch that vertex (the field is written as it is, not
    through a maximum that would turn it into 0), finite values elsewhere, and the handle still works afterwards."""
    from femo_amd.engine import Vec
    mesh = _meshes()[name]()
    u, rho, m = sref.random_inputs(mesh.x, mesh.conn, seed=5)
    good = sref.pnorm_stress(mesh.x, mesh.conn, rho, u, m, 8.0, 0.5)
    vertex = mesh.n_vert // 2
    bad = u.copy()
    bad[vertex * mesh.tdim + 1] = np.nan
    touching = np.any(mesh.conn == vertex, axis=1)
    assert 0 < touching.sum() < mesh.n_cell
    dev, rv, uv = _device(gpu, mesh, rho, bad)
    cells = Vec(gpu, mesh.n_cell)
    for field in (np.array(dev.von_mises(uv, cells, rv, 0.5).get()), np.array(dev.von_mises(uv, cells).get())):
        assert np.array_equal(np.isnan(field), touching) and np.all(np.isfinite(field[~touching]))
    uv.set(u)
    field = np.array(dev.von_mises(uv, cells, rv, 0.5).get())
    assert np.abs(field - good["field"]).max() <= 1e-12 * np.abs(good["field"]).max()
    assert abs(dev.pnorm_stress(rv, uv, m, 8.0, 0.5, good["alpha"]) - good["value"]) <= 1e-12 * good["value"]


def test_reproducible_bit_for_bit(gpu):
    mesh = _meshes()["cube6j"]()
    u, rho, m = sref.random_inputs(mesh.x, mesh.conn, seed=9)
    dev, rv, uv = _device(gpu, mesh, rho, u)
    J1, du1, dr1 = _all_three(gpu, dev, rv, uv, m, 8.0, 0.5, 1.0)
    J2, du2, dr2 = _all_three(gpu, dev, rv, uv, m, 8.0, 0.5, 1.0)
    assert J1 == J2 and np.array_equal(du1, du2) and np.array_equal(dr1, dr2)


def _p1_mass_projection(mesh, cells, lump):
    """L2 projection of a cell-wise constant onto CG1: M x = b with the P1 mass matrix, or b / (M 1) when lumped."""
    d = mesh.tdim
    vol = ref.cell_volumes(mesh.x, mesh.conn)
    b = np.zeros(mesh.n_vert)
    np.add.at(b, mesh.conn.ravel(), np.repeat(cells * vol / (d + 1), d + 1))
    if lump:
        w = np.zeros(mesh.n_vert)
        np.add.at(w, mesh.conn.ravel(), np.repeat(vol, d + 1))            # sum of |T_c| around the vertex, (d + 1) (M 1)
        return (d + 1) * b / w
    Me = vol[:, None, None] / ((d + 1) * (d + 2)) * (np.ones((d + 1, d + 1)) + np.eye(d + 1))
    rows = np.repeat(mesh.conn, d + 1, axis=1).ravel()
    cols = np.tile(mesh.conn, (1, d + 1)).ravel()
    M = sp.csc_matrix((Me.ravel(), (rows, cols)), shape=(mesh.n_vert,) * 2)
    return spla.spsolve(M, b)


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_projected_field(gpu, name):
    from femo_amd.fea.elasticity import von_Mises_stress
    from femo_amd.fea.fea_hip import Function, FunctionSpace, VectorFunctionSpace, project
    mesh = _meshes()[name]()
    u_h, rho_h, _ = sref.random_inputs(mesh.x, mesh.conn, seed=4)
    u, rho = Function(VectorFunctionSpace(mesh)), Function(FunctionSpace(mesh, ("DG", 0)))
    u.vector[:] = u_h
    rho.vector[:] = rho_h
    cells = sref.cell_field(mesh.x, mesh.conn, u_h, rho_h, 0.5)
    form = von_Mises_stress(u, rho, q=0.5)
    dg, cg = Function(FunctionSpace(mesh, ("DG", 0))), Function(FunctionSpace(mesh, ("CG", 1)))
    project(form, dg)
    assert np.abs(dg.vector.getArray() - cells).max() <= 1e-12 * cells.max()
    project(form, cg, lump_mass=True)
    lumped = _p1_mass_projection(mesh, cells, True)
    assert np.abs(cg.vector.getArray() - lumped).max() <= 1e-12 * np.abs(lumped).max()
    project(form, cg)
    full = _p1_mass_projection(mesh, cells, False)
    # the bar test_gpu_fields.py::test_project_matches_oracle puts on project(PowerExpr(w, 3.0), out)
    assert np.abs(cg.vector.getArray() - full).max() / np.abs(full).max() < 1e-10
    solid = sref.cell_field(mesh.x, mesh.conn, u_h)
    project(von_Mises_stress(u), dg)                                      # q = 0: no density
    assert np.abs(dg.vector.getArray() - solid).max() <= 1e-12 * solid.max()


# ------------------------------------------------------------------------------------------ through the operators ----
P_STRESS, Q_STRESS = 8.0, 0.5


@pytest.fixture(scope="module")
def cantilever_ref():
    """The restatement of the filtered 16 x 8 cantilever, once: the design, m from its first state, value and total."""
    mesh, facets, h_avg = cantilever_mesh()
    P = sref.cantilever_problem(mesh, facets, h_avg)
    x0 = 1e-2 + 0.86 * np.random.default_rng(0).random(mesh.n_cell)
    rho, _, u = sref.cantilever_state(P, x0)
    m = 1.0 / sref.cell_field(mesh.x, mesh.conn, u, rho, Q_STRESS).max()
    T = sref.cantilever_total(P, x0, m, P_STRESS, Q_STRESS)
    vol = ref.cell_volumes(mesh.x, mesh.conn)
    T.update(x0=x0, m=m, W=P["W"], J_c=P["F"] @ T["u"], avg=vol @ T["rho"] / vol.sum(),
             grad_c=P["W"].T @ -ref.compliance_gradient(mesh.x, mesh.conn, T["rho"], T["u"], T["u"], K0=P["K0"]))
    for v in T.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return T


def build_cantilever(x0, m, pc="jacobi", nelx=16, nely=8):
    """build_cantilever of test_gpu_topopt.py with the stress output beside the compliance."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, VectorFunctionSpace,
                                      createRectangleMesh, locate_dofs_geometrical, locate_entities_boundary, meshSize,
                                      meshtags, pnorm_stress)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    marker = lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / nely + 3e-6, abs(x[0] - L_X) < 3e-6)
    fdim = mesh.tdim - 1
    facets = locate_entities_boundary(mesh, fdim, marker)
    ds_ = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, fdim, facets, np.full(len(facets), 100, dtype=np.int32)))
    fea = FEA(mesh)
    fea.REPORT = False
    # dJ/du of the stress is not zero on the clamped dofs (the load is): the multiplier is zeroed there, which makes the
    # adjoint total the exact reduced gradient that the restatement and the central differences give
    fea.consistent_bc_partials = True
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(V)
    f = Constant(mesh, (0, -1 / 4))
    res = pdeRes(u_fn, TestFunction(V), rho_fn, f, dss=ds_(100), preconditioner=pc)
    stress = pnorm_stress(u_fn, rho_fn, m=m, p=P_STRESS, q=Q_STRESS)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='avg_density', type='scalar', form=averageFunc(rho_fn), arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance(u_fn, f, dss=ds_(100)), arguments=['displacements'])
    fea.add_output(name='stress', type='scalar', form=stress, arguments=['displacements', 'density'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.array(x0))
    return Simulator(model), dict(res=res, stress=stress, u=u_fn)


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_cantilever_stress_cycle(gpu, cantilever_ref, pc):
    T = cantilever_ref
    sim, aux = build_cantilever(T["x0"], T["m"], pc)
    sim.run()
    J = float(sim['stress'][0])
    g = np.asarray(sim.compute_totals('stress', 'density_unfiltered'))
    info = aux['res'].last_info
    err_J, err_g = abs(J - T["value"]) / abs(T["value"]), np.abs(g - T["grad"]).max() / np.abs(T["grad"]).max()
    print(f"16x8 cantilever, {pc}: J {err_J:.1e}, total {err_g:.1e}; state PCG {info['state']['iterations']} it, "
          f"stress adjoint {info['adjoint']['iterations']} it")
    assert err_J <= 1e-9
    assert err_g <= 1e-8
    assert info['adjoint']['converged'] == 1 and info['adjoint']['preconditioner'] == pc
    # the right-hand side of that adjoint solve was not the load
    dJdu = np.array(aux['stress'].assemble_derivative(aux['u']).get())
    F = np.array(aux['res'].load().get())
    cos = sref.cosine(dJdu, F)
    print(f"cos(dJ/du, F) = {cos:.2e} (restatement {sref.cosine(T['du'], T['F']):.2e})")
    assert abs(cos) < 0.1
    chk = sim.check_totals('stress', 'density_unfiltered', step=1e-5, n_dir=3, seed=0)
    print(f"central differences: {chk['rel_error']}")
    assert max(chk['rel_error']) <= 1e-6, chk


def test_existing_outputs_unchanged(gpu, cantilever_ref):
    """The extra output changes nothing that was there: the bars of test_gpu_topopt.py::test_cantilever_cycle."""
    T = cantilever_ref
    sim, aux = build_cantilever(T["x0"], T["m"])
    sim.run()
    assert np.abs(np.asarray(sim['density']) - T['rho']).max() <= 1e-14
    u = np.asarray(sim['displacements'])
    assert np.abs(u - T['u']).max() <= 1e-9 * np.abs(T['u']).max()
    assert abs(float(sim['compliance'][0]) - T['J_c']) <= 1e-9 * abs(T['J_c'])
    assert abs(float(sim['avg_density'][0]) - T['avg']) <= 1e-14
    sim.compute_totals('stress', 'density_unfiltered')                    # in between: leaves the compliance adjoint alone
    g = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    assert np.abs(g - T['grad_c']).max() <= 1e-8 * np.abs(T['grad_c']).max()
    assert aux['res'].last_info['adjoint']['converged'] == 1
