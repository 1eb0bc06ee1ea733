"""GPU tests of the aggregated von Mises stress over several load cases (csrc/elast_stress.hip:
k_elast_stress_cell_multi, k_elast_stress_du_multi; femo_elast_pnorm_stress_multi / femo_elast_von_mises_multi;
MultiLoadPnormStress / MultiLoadVonMises) against the restatement tests/elast_stress_multi_ref.py and the single-column
entry points: kernel parity, accumulate, one output at a time, zero columns and zero weights, bitwise reproducibility,
the partials buffer shared with the single-column entry point, limits, the batched solve with right-hand sides that are live on the fixed dofs, the projected fields, and the 16 x 8
cantilever with three loads through FEAModel + GeneralFilterModel + Simulator with the Dirichlet filter in every column.

L = 1, 3, 5, 8: one column, a chunk of the dJ/du kernel that is not full, a ragged second chunk (4 + 1), the maximum."""
import functools

import numpy as np
import pytest

import elast_multi_ref as mr
import elast_stress_multi_ref as smr
import elast_stress_ref as sref
from elast_pc_ref import L_X, L_Y
from test_elast_stress_multi_host import P_STRESS, Q_STRESS, WEIGHTS, cantilever_inputs
from test_gpu_elast_stress import _meshes, _p1_mass_projection

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "cube6j"]
COLUMNS = [1, 3, 5, 8]


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def inputs(name, L):
    """Mesh, columns (magnitudes 1 ... 1e-3), density, scales and weights of one (mesh, L): built once, read only."""
    mesh = _meshes()[name]()
    U, rho, m, w = smr.random_columns(mesh.x, mesh.conn, L, seed=5)
    for a in (U, rho, m, w):
        a.setflags(write=False)
    return mesh, U, rho, m, w


@functools.lru_cache(maxsize=None)
def restated(name, L, p, q):
    mesh, U, rho, m, w = inputs(name, L)
    R = smr.pnorm_stress_multi(mesh.x, mesh.conn, rho, U, m, p, q, weights=w)
    for v in R.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return R


def _device(ctx, mesh, rho, U):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    return DeviceElasticity(ctx, mesh), Vec(ctx, mesh.n_cell).set(rho), Vec(ctx, U.size).set(U.ravel())


def _all_three(ctx, dev, L, rv, uv, m, p, q, alpha, w=None, **kw):
    from femo_amd.engine import Vec
    gu, gr = Vec(ctx, uv.n), Vec(ctx, rv.n)
    J = dev.pnorm_stress_multi(L, rv, uv, m, p, q, alpha, weights=w, grad_u=gu, grad_rho=gr, **kw)
    return J, np.array(gu.get()).reshape(L, -1), np.array(gr.get())


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("L", COLUMNS)
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p,q", sref.PQ_CASES)
def test_kernel_parity(gpu, name, L, p, q):
    from femo_amd.engine import Vec
    mesh, U, rho, m, w = inputs(name, L)
    assert (name != "cube6j" or (mesh.n_cell, mesh.n_vert) == (1296, 343)) and (name != "cube4j" or mesh.n_cell == 384)
    R = restated(name, L, p, q)
    dev, rv, uv = _device(gpu, mesh, rho, U)
    J, du, drho = _all_three(gpu, dev, L, rv, uv, m, p, q, R["alpha"], w)
    errs = dict(value=max(abs(J[l] - R["values"][l]) / R["values"][l] for l in range(L)),
                du=max(_rel(du[l], R["du"][l]) for l in range(L)))
    if q != 0.0:
        errs["drho"] = _rel(drho, R["drho"])
    else:
        assert np.all(drho == 0.0)
    cells = Vec(gpu, mesh.n_cell)
    errs["envelope"] = _rel(np.array(dev.von_mises_multi(L, uv, cells, rv, q).get()), smr.envelope(R["fields"]))
    # scaled by m the columns are of one size, so that every load case owns cells of the envelope
    scaled = smr.envelope(R["fields"], m)
    assert L == 1 or len(set(np.argmax(m[:, None] * R["fields"], axis=0))) == L
    errs["envelope_scaled"] = _rel(np.array(dev.von_mises_multi(L, uv, cells, rv, q, scales=m).get()), scaled)
    errs["column"] = max(_rel(np.array(dev.von_mises_multi(L, uv, cells, rv, q, column=l).get()), R["fields"][l]) for l in range(L))
    if q == 0.0:                                                       # q = 0 needs no density
        errs["solid"] = _rel(np.array(dev.von_mises_multi(L, uv, cells).get()), smr.envelope(R["fields"]))
    print(f"{name} L={L} p={p} q={q}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12


@pytest.mark.parametrize("L", COLUMNS)
@pytest.mark.parametrize("name", MESHES)
def test_matches_single_column(gpu, name, L):
    """Column by column against femo_elast_pnorm_stress / femo_elast_von_mises with m_l, and dJ/drho against their
    accumulated calls in ascending l: the chunked instantiations of the two kernels against the one-column ones."""
    from femo_amd.engine import Vec
    mesh, U, rho, m, w = inputs(name, L)
    p, q = 8.0, 0.5
    alpha = restated(name, L, p, q)["alpha"]
    dev, rv, uv = _device(gpu, mesh, rho, U)
    J, du, drho = _all_three(gpu, dev, L, rv, uv, m, p, q, alpha)                     # weights: 1
    _, duw, drhow = _all_three(gpu, dev, L, rv, uv, m, p, q, alpha, w, value=False)
    n = U.shape[1]
    u1, g1, f1, fl = Vec(gpu, n), Vec(gpu, n), Vec(gpu, mesh.n_cell), Vec(gpu, mesh.n_cell)
    acc, one, accw = Vec(gpu, mesh.n_cell), Vec(gpu, mesh.n_cell), np.zeros(mesh.n_cell)
    worst = 0.0
    for l in range(L):
        u1.set(U[l])
        Jl = dev.pnorm_stress(rv, u1, m[l], p, q, alpha, grad_u=g1)
        gl = np.array(g1.get())
        dev.pnorm_stress(rv, u1, m[l], p, q, alpha, value=False, grad_rho=acc, accumulate=l > 0)
        dev.pnorm_stress(rv, u1, m[l], p, q, alpha, value=False, grad_rho=one)
        accw += w[l] * np.array(one.get())
        single = np.array(dev.von_mises(u1, f1, rv, q).get())
        worst = max(worst, abs(J[l] - Jl) / Jl, _rel(du[l], gl), _rel(duw[l], w[l] * gl),
                    _rel(np.array(dev.von_mises_multi(L, uv, fl, rv, q, column=l).get()), single))
    worst = max(worst, _rel(drho, np.array(acc.get())), _rel(drhow, accw))
    print(f"{name} L={L}: worst relative difference to the single-column entry points {worst:.1e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("name,L", [("square9j", 3), ("cube4j", 5), ("cube6j", 8)])
def test_accumulate_and_one_output_at_a_time(gpu, name, L):
    from femo_amd.engine import Vec
    mesh, U, rho, m, w = inputs(name, L)
    p, q = 8.0, 0.5
    R = restated(name, L, p, q)
    dev, rv, uv = _device(gpu, mesh, rho, U)
    J, du, drho = _all_three(gpu, dev, L, rv, uv, m, p, q, R["alpha"], w)
    # accumulate adds onto what is there
    fill_u, fill_r = np.linspace(-1.0, 1.0, U.size), np.linspace(2.0, 3.0, rho.size)
    gu, gr = Vec(gpu, U.size).set(fill_u), Vec(gpu, rho.size).set(fill_r)
    assert dev.pnorm_stress_multi(L, rv, uv, m, p, q, R["alpha"], weights=w, value=False, grad_u=gu, grad_rho=gr,
                                  accumulate=True) is None
    assert np.abs(gu.get() - (fill_u + R["du"].ravel())).max() <= 1e-12 * max(np.abs(R["du"]).max(), 1.0)
    assert np.abs(gr.get() - (fill_r + R["drho"])).max() <= 1e-12 * max(np.abs(R["drho"]).max(), 3.0)
    # one output at a time: the same bits as all three at once
    assert np.array_equal(dev.pnorm_stress_multi(L, rv, uv, m, p, q, R["alpha"], weights=w), J)
    only_u, only_r = Vec(gpu, U.size), Vec(gpu, rho.size)
    dev.pnorm_stress_multi(L, rv, uv, m, p, q, R["alpha"], weights=w, value=False, grad_u=only_u)
    dev.pnorm_stress_multi(L, rv, uv, m, p, q, R["alpha"], weights=w, value=False, grad_rho=only_r)
    assert np.array_equal(np.array(only_u.get()).reshape(L, -1), du) and np.array_equal(only_r.get(), drho)
    # a scalar m is the same scale for every column
    Js = dev.pnorm_stress_multi(L, rv, uv, 2.0, p, q, R["alpha"])
    assert np.array_equal(Js, dev.pnorm_stress_multi(L, rv, uv, np.full(L, 2.0), p, q, R["alpha"]))


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_zero_column_and_zero_weight(gpu, name):
    """Column 1 is zero and column 3 has weight zero among live ones (L = 5): exact zeros for the zero column's value and for
    both grad_u blocks, nothing of either in dJ/drho, and the live columns keep the bits they have when all five are live;
    then all columns zero."""
    from femo_amd.engine import Vec
    L = 5
    mesh, U, rho, m, w = inputs(name, L)
    U0, w0 = U.copy(), w.copy()
    U0[1] = 0.0
    w0[3] = 0.0
    live = [0, 2, 4]
    for p, q in sref.PQ_CASES:
        dev, rv, uv = _device(gpu, mesh, rho, U)
        Jf, duf, _ = _all_three(gpu, dev, L, rv, uv, m, p, q, 1.0, w)
        uv.set(U0.ravel())
        J, du, drho = _all_three(gpu, dev, L, rv, uv, m, p, q, 1.0, w0)
        assert np.all(np.isfinite(J)) and np.all(np.isfinite(du)) and np.all(np.isfinite(drho))
        assert J[1] == 0.0 and np.all(du[1] == 0.0) and np.all(du[3] == 0.0)
        assert J[3] == Jf[3] and Jf[3] > 0.0                           # the values are unweighted
        assert np.array_equal(J[live], Jf[live]) and np.array_equal(du[live], duf[live])
        R = smr.pnorm_stress_multi(mesh.x, mesh.conn, rho, U0, m, p, q, alpha=1.0, weights=w0)
        assert np.abs(drho - R["drho"]).max() <= 1e-12 * max(np.abs(R["drho"]).max(), 1e-300)
        # without accumulate the blocks of both are written as zeros, not left as they were
        gu = Vec(gpu, U.size).fill(7.0)
        dev.pnorm_stress_multi(L, rv, uv, m, p, q, 1.0, weights=w0, value=False, grad_u=gu)
        assert np.array_equal(np.array(gu.get()).reshape(L, -1), du)
        uv.set(np.zeros(U.size))
        J, du, drho = _all_three(gpu, dev, L, rv, uv, m, p, q, 1.0, w)
        assert np.all(J == 0.0) and np.all(du == 0.0) and np.all(drho == 0.0)
        assert np.all(np.array(dev.von_mises_multi(L, uv, Vec(gpu, mesh.n_cell), rv, q).get()) == 0.0)


def test_reproducible_bit_for_bit(gpu):
    mesh, U, rho, m, w = inputs("cube6j", 5)
    dev, rv, uv = _device(gpu, mesh, rho, U)
    J1, du1, dr1 = _all_three(gpu, dev, 5, rv, uv, m, 8.0, 0.5, 1.0, w)
    J2, du2, dr2 = _all_three(gpu, dev, 5, rv, uv, m, 8.0, 0.5, 1.0, w)
    assert np.array_equal(J1, J2) and np.array_equal(du1, du2) and np.array_equal(dr1, dr2)


def test_partials_buffer_shared_with_single_column(gpu):
    """The single-column and the batched aggregate fold through one partials buffer, sized for all columns by whichever call
    allocates it: one column, eight, one again on one handle, and eight first on a fresh one, give the same bits."""
    name, L, p, q = "cube6j", 8, 8.0, 0.5
    mesh, U, rho, m, w = inputs(name, L)
    assert (mesh.n_cell + 255) // 256 == 6
    R = restated(name, L, p, q)
    dev, rv, uv = _device(gpu, mesh, rho, U)
    from femo_amd.engine import Vec
    u0 = Vec(gpu, U.shape[1]).set(U[0])
    first = dev.pnorm_stress(rv, u0, m[0], p, q, R["alpha"])
    eight = dev.pnorm_stress_multi(L, rv, uv, m, p, q, R["alpha"])
    again = dev.pnorm_stress(rv, u0, m[0], p, q, R["alpha"])
    fresh, rv2, uv2 = _device(gpu, mesh, rho, U)
    eight_first = fresh.pnorm_stress_multi(L, rv2, uv2, m, p, q, R["alpha"])
    u02 = Vec(gpu, U.shape[1]).set(U[0])
    then_one = fresh.pnorm_stress(rv2, u02, m[0], p, q, R["alpha"])
    print(f"one column {first!r}, eight {eight!r}")
    assert first == again == then_one and np.array_equal(eight, eight_first)
    assert max(abs(eight[l] - R["values"][l]) / R["values"][l] for l in range(L)) <= 1e-12


def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    mesh, U, rho, m, w = inputs("rect8x4", 3)
    dev, rv, _ = _device(gpu, mesh, rho, U)
    n = U.shape[1]
    big = Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(0.0)
    cells = Vec(gpu, mesh.n_cell)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.pnorm_stress_multi(bad, rv, big, 1.0, 8.0, 0.5, 1.0)
        with pytest.raises(FemoError, match="columns"):
            dev.von_mises_multi(bad, big, cells, rv, 0.5)
    u3, g3 = Vec(gpu, 3 * n).set(U.ravel()), Vec(gpu, 3 * n)
    short, short_cells = Vec(gpu, 3 * n - 1), Vec(gpu, mesh.n_cell - 1)
    for kw in (dict(u=short), dict(grad_u=short), dict(grad_rho=short_cells), dict(rho=short_cells)):
        a = dict(rho=rv, u=u3, grad_u=None, grad_rho=None)
        a.update(kw)
        with pytest.raises(FemoError):
            dev.pnorm_stress_multi(3, a["rho"], a["u"], m, 8.0, 0.5, 1.0, grad_u=a["grad_u"], grad_rho=a["grad_rho"])
    with pytest.raises(FemoError):
        dev.von_mises_multi(3, short, cells, rv, 0.5)
    with pytest.raises(FemoError):
        dev.von_mises_multi(3, u3, short_cells, rv, 0.5)
    for kw in (dict(grad_u=u3), dict(grad_rho=rv)):                                   # an output that is an input
        with pytest.raises(FemoError, match="aliases"):
            dev.pnorm_stress_multi(3, rv, u3, m, 8.0, 0.5, 1.0, **kw)
    with pytest.raises(FemoError, match="aliases"):
        dev.von_mises_multi(3, u3, rv, rv, 0.5)
    for bad_m in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, np.nan, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0)):
        with pytest.raises(FemoError):
            dev.pnorm_stress_multi(3, rv, u3, bad_m, 8.0, 0.5, 1.0)
    for bad_w in ((1.0, -0.5, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, 1.0, 1.0)):
        with pytest.raises(FemoError):
            dev.pnorm_stress_multi(3, rv, u3, m, 8.0, 0.5, 1.0, weights=bad_w)
    for p, q, alpha in ((0.5, 0.5, 1.0), (8.0, -0.1, 1.0), (8.0, 0.5, 0.0), (np.nan, 0.5, 1.0), (8.0, 0.5, np.inf)):
        with pytest.raises(FemoError, match="stress aggregate"):
            dev.pnorm_stress_multi(3, rv, u3, m, p, q, alpha)
    with pytest.raises(FemoError):
        dev.von_mises_multi(3, u3, cells, None, 0.5)                                  # q > 0 needs the density
    with pytest.raises(FemoError):
        dev.von_mises_multi(3, u3, cells, rv, 0.5, column=3)
    with pytest.raises(FemoError):
        dev.von_mises_multi(3, u3, cells, rv, 0.5, scales=(1.0, 0.0, 1.0))
    assert np.all(np.isfinite(dev.pnorm_stress_multi(3, rv, u3, m, 8.0, 0.5, 1.0, grad_u=g3)))   # and the handle still works


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_solve_multi_with_live_fixed_entries(gpu, pc):
    """Right-hand sides that are non-zero on the fixed dofs in every column, as the stress adjoint's are: x = b there, and
    the free part solves K_ff x_f = b_f (the masked operator has identity rows and columns on the fixed dofs)."""
    import scipy.sparse.linalg as spla
    from femo_amd.engine import Vec
    from test_gpu_elast_multi import _columns, _device as solve_device, case
    c = case("square9j")
    dev, _ = solve_device(gpu, "square9j")
    L, n = 3, dev.n_dof
    fixed, free = np.nonzero(c["mask"] == 1)[0], np.nonzero(c["mask"] == 0)[0]
    B = np.random.default_rng(12).standard_normal((L, n)) * np.array([1.0, 1e-3, 50.0])[:, None]
    assert np.abs(B[:, fixed]).min() > 0.0
    bv, xv = Vec(gpu, L * n).set(B.ravel()), Vec(gpu, L * n)
    infos = dev.solve_multi(L, bv, xv, rtol=1e-15, pc=pc)
    X = _columns(xv, L)
    Kff = dev.export_csr()[free][:, free].tocsc()
    lu = spla.splu(Kff)
    for l in range(L):
        xf = lu.solve(B[l][free])
        err = np.abs(X[l][free] - xf).max() / np.abs(xf).max()
        print(f"square9j {pc} column {l}: {infos[l].iterations} it, free part error {err:.1e}")
        assert infos[l].converged == 1
        assert np.array_equal(X[l][fixed], B[l][fixed])
        assert err <= 1e-9


@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_projected_field(gpu, name):
    from femo_amd.fea.elasticity import von_Mises_stress_multiload
    from femo_amd.fea.fea_hip import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace, project
    L = 3
    mesh, U, rho_h, m, _ = inputs(name, L)
    u, rho = Function(LoadCaseSpace(VectorFunctionSpace(mesh), L)), Function(FunctionSpace(mesh, ("DG", 0)))
    u.vector[:] = U.ravel()
    rho.vector[:] = rho_h
    fields = restated(name, L, 8.0, 0.5)["fields"]                     # rho^0.5 sigma_vm per load case
    dg, cg = Function(FunctionSpace(mesh, ("DG", 0))), Function(FunctionSpace(mesh, ("CG", 1)))
    for form, cells in ((von_Mises_stress_multiload(u, rho, q=0.5, scales=m), smr.envelope(fields, m)),
                        (von_Mises_stress_multiload(u, rho, q=0.5, load_case=1), fields[1])):
        project(form, dg)
        assert np.abs(dg.vector.getArray() - cells).max() <= 1e-12 * cells.max()
        project(form, cg, lump_mass=True)
        lumped = _p1_mass_projection(mesh, cells, True)
        assert np.abs(cg.vector.getArray() - lumped).max() <= 1e-12 * np.abs(lumped).max()
        project(form, cg)
        full = _p1_mass_projection(mesh, cells, False)
        # the bar test_gpu_fields.py::test_project_matches_oracle puts on project(PowerExpr(w, 3.0), out)
        assert np.abs(cg.vector.getArray() - full).max() / np.abs(full).max() < 1e-10
    solid = np.stack([sref.cell_field(mesh.x, mesh.conn, U[l]) for l in range(L)]).max(axis=0)
    project(von_Mises_stress_multiload(u), dg)                         # q = 0: no density
    assert np.abs(dg.vector.getArray() - solid).max() <= 1e-12 * solid.max()


# ------------------------------------------------------------------------------------------ through the operators ----
@pytest.fixture(scope="module")
def cantilever_ref():
    """The restatement of the filtered 16 x 8 cantilever with three loads, once: m from its first state, value, total, and
    the weighted compliance of test_gpu_elast_multi.py::test_multiload_cycle beside them."""
    mesh, P, x0, m = cantilever_inputs()
    T = smr.cantilever_total_multi(P, x0, m, WEIGHTS, P_STRESS, Q_STRESS)
    T.update(x0=x0, m=m)
    for v in T.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return T


def build_multiload_stress(x0, m, pc, device, nelx=16, nely=8):
    """build_multiload of test_gpu_elast_multi.py with the multi-load stress output beside the compliance."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, LoadCaseSpace, Measure, TestFunction,
                                      VectorFunctionSpace, compliance_multiload, createRectangleMesh,
                                      locate_dofs_geometrical, meshSize, meshtags, pdeRes_multiload, pnorm_stress_multiload)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    facets, tractions = mr.cantilever_loads(mesh, L_X, L_Y, nely)
    dss = [Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, f, np.full(len(f), 100 + l, dtype=np.int32)))(100 + l)
           for l, f in enumerate(facets)]
    fs = [Constant(mesh, t) for t in tractions]
    fea = FEA(mesh)
    fea.REPORT = False
    fea.consistent_bc_partials = True          # dJ/du of the stress is live on the clamped dofs of every column
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    S = LoadCaseSpace(V, len(fs))
    rho_fn, u_fn = Function(Q), Function(S)
    res = pdeRes_multiload(u_fn, TestFunction(V), rho_fn, fs, dss, preconditioner=pc)
    stress = pnorm_stress_multiload(u_fn, rho_fn, m=m, p=P_STRESS, q=Q_STRESS, weights=WEIGHTS)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance_multiload(u_fn, fs, dss, weights=WEIGHTS),
                   arguments=['displacements'])
    fea.add_output(name='stress', type='scalar', form=stress, arguments=['displacements', 'density'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.array(x0))
    return Simulator(model, device=device), mesh, dict(facets=facets, tractions=tractions, h_avg=h_avg, res=res, stress=stress,
                                                       u=u_fn, rho=rho_fn)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_multiload_stress_cycle(gpu, cantilever_ref, pc, device):
    """Fails on a build whose Dirichlet filter reaches the first column only: the multiplier of the other columns then keeps
    its clamped entries, which puts an error of several per cent into the total."""
    from femo_amd.fea.elasticity import pnorm_stress_multiload
    T = cantilever_ref
    sim, mesh, aux = build_multiload_stress(T["x0"], T["m"], pc, device)
    sim.run()
    res, stress = aux['res'], aux['stress']
    J = float(np.asarray(sim['stress']).ravel()[0])
    g = np.asarray(sim.compute_totals('stress', 'density_unfiltered'))
    info = res.last_info
    err_J, err_g = abs(J - T["value"]) / abs(T["value"]), np.abs(g - T["grad"]).max() / np.abs(T["grad"]).max()
    err_v = np.abs(stress.values() - T["values"]).max() / np.abs(T["values"]).max()
    print(f"16x8 cantilever, 3 loads, {pc}, device arrays {device}: J {err_J:.1e}, J_l {err_v:.1e}, total {err_g:.1e}; "
          f"state PCG {info['state']['iterations']} it, stress adjoint {info['adjoint']['iterations']} it")
    assert err_J <= 1e-9 and err_v <= 1e-9
    assert err_g <= 1e-8
    assert res.solve_counts == {"state": 1, "adjoint": 1}             # the stress adjoint is one batched solve
    assert info['adjoint']['converged'] == [1, 1, 1] and info['adjoint']['preconditioner'] == pc
    # its right-hand sides are live on the clamped dofs of every column
    dJdu = np.array(stress.assemble_derivative(aux['u']).get()).reshape(3, -1)
    fixed = np.nonzero(res._mask == 1)[0]
    for l in range(3):
        assert np.abs(dJdu[l][fixed]).max() > 0.1 * np.abs(dJdu[l]).max()
    # the scales the restatement took from the first state
    probe = pnorm_stress_multiload(aux['u'], aux['rho'], p=P_STRESS, q=Q_STRESS)
    assert np.abs(probe.set_scales_from_state() - T["m"]).max() <= 1e-8 * T["m"].max()
    chk = sim.check_totals('stress', 'density_unfiltered', step=1e-5, n_dir=3, seed=0)
    print(f"central differences: {chk['rel_error']}")
    assert max(chk['rel_error']) <= 1e-6, chk
    # after the stress totals the compliance total still meets the bar of test_multiload_cycle
    sim.run()
    R = mr.reference_cycle_multi(mesh, aux['facets'], aux['tractions'], WEIGHTS, aux['h_avg'], np.array(sim['density_unfiltered']))
    gc = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    assert abs(float(np.asarray(sim['compliance']).ravel()[0]) - R['J']) <= 1e-9 * abs(R['J'])
    assert np.abs(gc - R['grad']).max() <= 1e-8 * np.abs(R['grad']).max()
    assert res.last_info['adjoint']['converged'] == [1, 1, 1]
