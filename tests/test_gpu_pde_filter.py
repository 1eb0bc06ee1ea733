"""GPU tests of the Helmholtz (PDE) density filter (csrc/pde_filter.hip, `DevicePdeFilter`, `DeviceProjection.filter_forward`,
`HelmholtzFilterModel`, `ProjectedFilterModel(filter="helmholtz")`) against the restatement tests/pde_filter_ref.py, its SciPy
matrices and its sparse direct solves.

The meshes are those of tests/test_gpu_elast_harm.py: less than one wave of rows (rect8x4), the two jittered ones, two with
more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343) and fan40 (a hub row of 40 entries); r in {h, 2 h, 4 h},
both masses.

Bounds.  A: 1e-13 of its largest entry (sums of at most ~40 terms).  An application against the direct solve: 1e-9 of the
largest entry, the project's bound for an iterative solve against a direct one; W 1 = 1, the volume and <y, W x> = <x, W^T y>
to 1e-9 as well (two inexact solves stand between the sides).  Iterations: at most those of the restated loop (the same
stopping test) plus max(2, 10 %); the same margin between rect24x12 and the rectangle at 48 x 24 at equal r / h.  Models: the
bounds of tests/test_gpu_topopt.py (u, J 1e-9; total gradient 1e-8; check_totals 1e-6; directional central differences 1e-5),
the density to 1e-9 because the filter is a solve.

MEASURED on the MI355X (6 meshes x 3 radii x 2 masses; the tests print every figure):
  A against the restatement                  9.5e-16 at the most (fan40, consistent), symmetric bit for bit, two builds equal bits
  W x, W^T y against the direct solve        1.6e-13 and 1.3e-13 at the most (fan40, consistent, r = h); bound 1e-9
  iterations, device / restatement           equal in all 72 solves: rect8x4 14 23 32, square9j 15 26 44, cube4j 17 28 40,
                                             rect24x12 14 25 48, cube6j 17 30 50, fan40 37 53 72 (lumped, W x, r = h, 2 h, 4 h)
  24 x 12 against 48 x 24 at equal r / h     lumped 14 25 48 / 14 25 48, consistent 13 22 46 / 13 22 47
  |W 1 - 1|, volume, <y, W x> - <x, W^T y>   4.1e-13, 4.2e-15, 9.3e-15 at the most; bounds 1e-9
  two applications                           equal bits, both products
  warm start after a 1e-3 change of x        7.4e-14 (rect24x12) and 6.3e-14 (cube4j) from the cold result; 20 against 25 and
                                             22 against 28 iterations; the transpose has the cold handle's bits
  fused projection                           xt and rho bit for bit in fixed AND in volume mode (eta equal to the last digit);
                                             2 launches after the solve in fixed mode (mean + fold of the info), 110 in volume mode
  non-finite input                           NaN, +Inf, -Inf: refused in all 36 calls (both products, the fused projection, cold and
                                             warm handles); the next call has the clean bits
  max_it = 3                                 "pde_filter: the solve did not converge in 3 iterations (residual 7.636e-03, ...)"
  16 x 8 cantilever, HelmholtzFilterModel    density 3.3e-14, u 1.8e-14, J 1.4e-14, total gradient 1.7e-13, check_totals 1.2e-8,
                                             directional central differences 3.4e-8; host and device mode alike
  ProjectedFilterModel("helmholtz"), beta 4  density 6.6e-14, u 8.0e-14, J 7.9e-14, total gradient 3.8e-13, check_totals 3.6e-8,
                                             directional central differences 1.7e-8
  operation products                         fwd against central differences 4.1e-11 / 1.4e-10, rev against fwd 1.7e-16 / 1.4e-15
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import elasticity_ref as eref
import pde_filter_ref as pf
import projection_ref as P

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j", "fan40"]
RADII_H = (1.0, 2.0, 4.0)
L_X, L_Y, NELX, NELY = 160.0, 80.0, 16, 8


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def _mesh(name):
    import elast_pc_ref as pr
    from femo_amd.fea.mesh import Mesh, createRectangleMesh, createUnitCubeMesh
    if name == "rect24x12":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12)
    if name == "rect48x24":
        return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 48, 24)
    if name == "cube6j":
        return createUnitCubeMesh(6, 0.2)
    if name == "fan40":
        import wide_meshes as W
        return Mesh(*W.fan(40, 8))
    return pr.small_meshes()[name]()


@functools.lru_cache(maxsize=None)
def restated(name, k, kind):
    """The restated filter, an input pair, both direct products and the restated PCG counts: built once, read only."""
    m = _mesh(name)
    F = pf.Filter(m.x, m.conn, k * pf.h_of(name), kind)
    rng = np.random.default_rng(17)
    x, y = rng.uniform(0.0, 1.0, m.n_cell), rng.uniform(-1.0, 1.0, m.n_cell)
    runs = [pf.pcg(F.A, F.load(v, t), rtol=1e-13) for v, t in ((x, False), (y, True))]
    assert all(r["converged"] == 1 for r in runs)
    return dict(F=F, x=x, y=y, Wx=F.apply(x), WTy=F.apply(y, transpose=True), iterations=[r["iterations"] for r in runs])


def _margin(n):
    return max(2, int(np.ceil(0.1 * n)))


def _device(gpu, name, k, kind, **kw):
    from femo_amd.fea.elasticity import DevicePdeFilter
    return DevicePdeFilter(gpu, _mesh(name), k * pf.h_of(name), mass=kind, **kw)


def _csr(dev):
    rowptr, col, val = dev.export_csr()
    n = len(rowptr) - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


# ------------------------------------------------------------------------------------------------------- the operator ----
@pytest.mark.parametrize("kind", pf.MASSES)
@pytest.mark.parametrize("name", MESHES)
def test_operator(gpu, name, kind):
    """A against the restatement to 1e-13 of its largest entry on the restatement's pattern, symmetric bit for bit, and the same
    bits from a second build."""
    worst = 0.0
    for k in RADII_H:
        A = _csr(_device(gpu, name, k, kind))
        Ar = restated(name, k, kind)["F"].A
        worst = max(worst, abs(A - Ar).max() / abs(Ar).max())
        assert (A != A.T).nnz == 0
        B = _csr(_device(gpu, name, k, kind))
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)
    print(f"{name} {kind}: A against the restatement {worst:.2e}")
    assert worst <= 1e-13


# ---------------------------------------------------------------------------------------------------- the application ----
@pytest.mark.parametrize("kind", pf.MASSES)
@pytest.mark.parametrize("name", MESHES)
def test_apply(gpu, name, kind):
    """W x and W^T y against the direct solve, iteration counts against the restated loop, two applications bit for bit, and the
    three identities."""
    from femo_amd.engine import Vec
    m = _mesh(name)
    n = m.n_cell
    for k in RADII_H:
        R = restated(name, k, kind)
        dev = _device(gpu, name, k, kind)
        dx, dy, out, out2 = Vec(gpu, n).set(R["x"]), Vec(gpu, n).set(R["y"]), Vec(gpu, n), Vec(gpu, n)
        Wx = np.array(dev.apply(dx, out).get())
        it_f = dev.last_info["iterations"]
        assert dev.last_info["converged"] == 1
        assert np.array_equal(Wx, np.array(dev.apply(dx, out2).get()))
        WTy = np.array(dev.apply(dy, out, transpose=True).get())
        it_t = dev.last_info["iterations"]
        assert np.array_equal(WTy, np.array(dev.apply(dy, out2, transpose=True).get()))
        e_f = np.abs(Wx - R["Wx"]).max() / np.abs(R["Wx"]).max()
        e_t = np.abs(WTy - R["WTy"]).max() / np.abs(R["WTy"]).max()
        one = np.abs(np.array(dev.apply(Vec(gpu, n).fill(1.0), out).get()) - 1.0).max()
        vol = R["F"].vol
        e_v = abs(vol @ Wx - vol @ R["x"]) / abs(vol @ R["x"])
        e_a = abs(R["y"] @ Wx - R["x"] @ WTy) / (np.linalg.norm(R["x"]) * np.linalg.norm(R["y"]))
        print(f"{name} {kind} r = {k:g} h: W x {e_f:.2e}, W^T y {e_t:.2e}, iterations {it_f} {it_t} / restated {R['iterations']}, "
              f"|W 1 - 1| {one:.2e}, volume {e_v:.2e}, transpose {e_a:.2e}, bytes {dev.bytes}")
        assert e_f <= 1e-9 and e_t <= 1e-9
        assert it_f <= R["iterations"][0] + _margin(R["iterations"][0])
        assert it_t <= R["iterations"][1] + _margin(R["iterations"][1])
        assert one <= 1e-9 and e_v <= 1e-9 and e_a <= 1e-9


@pytest.mark.parametrize("kind", pf.MASSES)
def test_iterations_do_not_grow_with_the_mesh(gpu, kind):
    """At equal r / h the counts on rect24x12 and on the same rectangle at 48 x 24 differ by no more than the margin."""
    from femo_amd.engine import Vec
    for k in RADII_H:
        its = []
        for name in ("rect24x12", "rect48x24"):
            m = _mesh(name)
            dev = _device(gpu, name, k, kind)
            x = Vec(gpu, m.n_cell).set(np.random.default_rng(17).uniform(0.0, 1.0, m.n_cell))
            dev.apply(x, Vec(gpu, m.n_cell))
            its.append(dev.last_info["iterations"])
        print(f"{kind} r = {k:g} h: iterations {its[0]} at 24 x 12, {its[1]} at 48 x 24")
        assert abs(its[0] - its[1]) <= _margin(min(its))


@pytest.mark.parametrize("name", ["rect24x12", "cube4j"])
def test_warm_start(gpu, name):
    """warm_start agrees with the cold result to 1e-9; after a 1e-3 change of x it takes no more iterations than the cold
    solve, and the transpose never warm-starts (its bits are the cold handle's)."""
    from femo_amd.engine import Vec
    R = restated(name, 2.0, "lumped")
    n = len(R["x"])
    cold, warm = _device(gpu, name, 2.0, "lumped"), _device(gpu, name, 2.0, "lumped", warm_start=True)
    x1 = R["x"] + 1e-3 * np.random.default_rng(2).uniform(-1.0, 1.0, n)
    out = Vec(gpu, n)
    y0 = np.array(cold.apply(Vec(gpu, n).set(R["x"]), out).get())
    y1 = np.array(cold.apply(Vec(gpu, n).set(x1), out).get())
    it_cold = cold.last_info["iterations"]
    w0 = np.array(warm.apply(Vec(gpu, n).set(R["x"]), out).get())
    assert np.array_equal(w0, y0)                                   # nothing to start from yet: the cold solve
    t_cold = np.array(cold.apply(Vec(gpu, n).set(R["y"]), out, transpose=True).get())
    t_warm = np.array(warm.apply(Vec(gpu, n).set(R["y"]), out, transpose=True).get())
    assert np.array_equal(t_cold, t_warm)
    w1 = np.array(warm.apply(Vec(gpu, n).set(x1), out).get())
    it_warm = warm.last_info["iterations"]
    err = np.abs(w1 - y1).max() / np.abs(y1).max()
    print(f"{name}: warm against cold {err:.2e}, iterations {it_warm} warm, {it_cold} cold")
    assert err <= 1e-9 and it_warm <= it_cold


# ------------------------------------------------------------------------------------------------------ the projection ----
@pytest.mark.parametrize("eta", [0.4, "volume"])
@pytest.mark.parametrize("name", ["rect24x12", "cube4j"])
def test_project(gpu, name, eta):
    """filter_forward equals apply followed by DeviceProjection.forward: xt bit for bit; rho bit for bit in fixed mode, to 1e-14
    in volume mode.  Passive cells and volumes as the projection's own tests have them."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    R = restated(name, 2.0, "lumped")
    n = len(R["x"])
    dev = _device(gpu, name, 2.0, "lumped")
    proj = DeviceProjection(gpu, n, 6.0, eta, R["F"].vol, solid=[1, 5], void=[2, n - 1])
    x, xt, rho, xt2, rho2 = Vec(gpu, n).set(R["x"]), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n)
    i1 = proj.filter_forward(dev, x, xt, rho)
    dev.apply(x, xt2)
    i2 = proj.forward(xt2, rho2)
    a, b = np.array(rho.get()), np.array(rho2.get())
    assert np.array_equal(np.array(xt.get()), np.array(xt2.get()))
    d = np.abs(a - b).max()
    print(f"{name} eta = {eta}: rho fused against apply + forward {d:.2e}, eta {i1['eta']:.17g} / {i2['eta']:.17g}, launches {i1['launches']}")
    if eta == "volume":
        assert d <= 1e-14
    else:
        assert np.array_equal(a, b)
    assert a[1] == 1.0 and a[2] == 1e-4 and abs(i1["vol_in"] - i2["vol_in"]) <= 1e-14 * abs(i2["vol_in"])


# ------------------------------------------------------------------------------------------- refusals, non-finite input ----
def _raw_create(gpu, dm, radius, lumped=1):
    from femo_amd import _lib
    h = _lib.H()
    rc = gpu.lib.femo_pde_filter_create(dm.handle, float(radius), lumped, C.byref(h))
    if rc == 0:
        gpu.lib.femo_pde_filter_destroy(h)
    return rc, (gpu.lib.femo_last_error() or b"").decode()


def test_refusals(gpu):
    from femo_amd import engine as E
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DevicePdeFilter
    m = _mesh("rect8x4")
    n = m.n_cell
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            DevicePdeFilter(gpu, m, r)
    with pytest.raises(ValueError, match="mass"):
        DevicePdeFilter(gpu, m, 0.5, mass="row-sum")
    with pytest.raises(ValueError, match="rtol"):
        DevicePdeFilter(gpu, m, 0.5, rtol=0.0)
    # a partitioned mesh: the last vertices are ghosts
    dm = E.DeviceMesh(gpu, m.x, m.conn, n_rows=m.n_vert - 3)
    rc, msg = _raw_create(gpu, dm, 0.5)
    assert rc == 2 and "one rank" in msg
    dev = DevicePdeFilter(gpu, m, 0.5)
    R = pf.Filter(m.x, m.conn, 0.5)
    x = np.random.default_rng(1).uniform(0.0, 1.0, n)
    good, out = Vec(gpu, n).set(x), Vec(gpu, n)
    for bad_x, bad_y in ((Vec(gpu, n - 1), out), (good, Vec(gpu, n - 1))):
        with pytest.raises(ValueError, match="shorter"):
            dev.apply(bad_x, bad_y)
        y = np.array(dev.apply(good, out).get())                      # the call after a refusal works
        assert np.abs(y - R.apply(x)).max() <= 1e-9
    with pytest.raises(ValueError, match="overlaps"):
        dev.apply(good, good)
    # a solve that does not converge names its iteration count
    from femo_amd import _lib
    opts = _lib.SolverOpts(rtol=1e-13, atol=0.0, max_it=3, zero_guess=1, check_every=0, pc=0, atol_pc=0.0)
    info = _lib.SolveInfo()
    rc = gpu.lib.femo_pde_filter_apply(dev.handle, 0, good.handle, out.handle, C.byref(opts), C.byref(info))
    msg = gpu.lib.femo_last_error().decode()
    print(f"three iterations allowed: rc {rc}, '{msg}'")
    assert rc == 1 and "did not converge in 3 iterations" in msg and info.converged == 0
    assert np.array_equal(np.array(dev.apply(good, out).get()), y)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("name", ["rect24x12", "cube4j"])
def test_non_finite_input(gpu, name, bad):
    """One bad entry in x: the call refuses, or every output entry is non-finite (the dependent set of a global solve is every
    cell); the handle then gives the clean result bit for bit.  Both products, and the fused projection."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    R = restated(name, 2.0, "lumped")
    n = len(R["x"])
    xb = R["x"].copy()
    xb[n // 3] = bad
    proj = DeviceProjection(gpu, n, 4.0, 0.5, R["F"].vol)
    outcomes = []
    for warm in (False, True):
        dev = _device(gpu, name, 2.0, "lumped", warm_start=warm)
        good, out, rho = Vec(gpu, n).set(R["x"]), Vec(gpu, n), Vec(gpu, n)
        clean = {t: np.array(dev.apply(good, out, transpose=t).get()) for t in (False, True)}
        proj.filter_forward(dev, good, out, rho)
        clean_rho = np.array(rho.get())
        for t in (False, True):
            try:
                y = np.array(dev.apply(Vec(gpu, n).set(xb), out, transpose=t).get())
                assert not np.any(np.isfinite(y))
                outcomes.append("non-finite")
            except ValueError as e:
                assert "not finite" in str(e)
                outcomes.append("refused")
            if warm and not t:
                y = np.array(dev.apply(good, out).get())              # a warm start was dropped: the cold solve's bits
                assert np.array_equal(y, _clean_cold(gpu, name)), "warm start after a refusal"
            else:
                assert np.array_equal(np.array(dev.apply(good, out, transpose=t).get()), clean[t])
        try:
            proj.filter_forward(dev, Vec(gpu, n).set(xb), out, rho)
            assert not np.any(np.isfinite(np.array(out.get()))) and not np.any(np.isfinite(np.array(rho.get())))
            outcomes.append("non-finite")
        except ValueError as e:
            assert "not finite" in str(e)
            outcomes.append("refused")
        if not warm:
            proj.filter_forward(dev, good, out, rho)
            assert np.array_equal(np.array(rho.get()), clean_rho) and np.array_equal(np.array(out.get()), clean[False])
    print(f"{name} {bad}: {outcomes}")


def _clean_cold(gpu, name):
    from femo_amd.engine import Vec
    R = restated(name, 2.0, "lumped")
    n = len(R["x"])
    return np.array(_device(gpu, name, 2.0, "lumped").apply(Vec(gpu, n).set(R["x"]), Vec(gpu, n)).get())


# --------------------------------------------------------------------------------------------------------- model level ----
def build_cantilever(kind, device=False, seed=0):
    """tests/test_gpu_topopt.build_cantilever at 16 x 8 with the Helmholtz filter: kind "helmholtz" (HelmholtzFilterModel) or
    "projected" (ProjectedFilterModel(filter="helmholtz") at beta = 4)."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import HelmholtzFilterModel, ProjectedFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, VectorFunctionSpace,
                                      createRectangleMesh, locate_dofs_geometrical, locate_entities_boundary, meshSize,
                                      meshtags)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), NELX, NELY)
    traction_facets = locate_entities_boundary(
        mesh, 1, lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / NELY + 3e-6, abs(x[0] - L_X) < 3e-6))
    facet_tag = meshtags(mesh, 1, traction_facets, np.full(len(traction_facets), 100, dtype=np.int32))
    ds_ = Measure('ds', domain=mesh, subdomain_data=facet_tag, metadata={"quadrature_degree": 4})
    fea = FEA(mesh)
    fea.REPORT = False
    fea.consistent_bc_partials = True
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(V)
    f = Constant(mesh, (0, -1 / 4))
    res = pdeRes(u_fn, TestFunction(V), rho_fn, f, dss=ds_(100), method="SIMP")
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='avg_density', type='scalar', form=averageFunc(rho_fn), arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance(u_fn, f, dss=ds_(100)), arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    fea_model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    nel = mesh.n_cell
    if kind == "projected":
        filt = ProjectedFilterModel(nel=nel, filter="helmholtz", mesh=mesh, h_avg=h_avg, projection_beta=4.0, eta=0.5)
    else:
        filt = HelmholtzFilterModel(mesh=mesh, beta=2.0, h_avg=h_avg)
    fea_model.add(filt, name='general_filter_model')
    fea_model.create_input('density_unfiltered', shape=nel, val=np.random.default_rng(seed).random(nel) * 0.86)
    fea_model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    fea_model.add_objective('compliance')
    fea_model.add_constraint('avg_density', upper=0.40)
    return Simulator(fea_model, device=device), filt, mesh, dict(facets=traction_facets, h_avg=h_avg)


def _reference_cycle(mesh, facets, h_avg, x0, projected):
    F = pf.Filter(mesh.x, mesh.conn, 2.0 * h_avg)
    xt = F.apply(x0)
    rho = P.H(xt, 4.0, 0.5) if projected else xt
    K0 = eref.element_matrices(mesh.x, mesh.conn)
    K = eref.stiffness(mesh.x, mesh.conn, rho, "SIMP", K0=K0)
    Fv = eref.traction_load(mesh.x, facets, (0.0, -0.25))
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    fixed = np.concatenate([2 * fixed_v, 2 * fixed_v + 1])
    u = eref.solve_fixed(K, Fv, fixed)
    dJ = -eref.compliance_gradient(mesh.x, mesh.conn, rho, u, u, "SIMP", K0=K0)
    if projected:
        dJ = dJ * P.H_x(xt, 4.0, 0.5)
    return dict(rho=rho, u=u, J=Fv @ u, grad=F.apply(dJ, transpose=True))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kind", ["helmholtz", "projected"])
def test_cantilever_cycle(gpu, kind, device):
    """The 16 x 8 cantilever through FEAModel + the filter model + Simulator: density, u and J to 1e-9, the total gradient to
    1e-8, check_totals (step 1e-4) to 1e-6, central differences of J along three directions to 1e-5."""
    sim, filt, mesh, aux = build_cantilever(kind, device=device)
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    R = _reference_cycle(mesh, aux['facets'], aux['h_avg'], x0, kind == "projected")
    e_rho = np.abs(np.asarray(sim['density']) - R['rho']).max()
    e_u = np.abs(np.asarray(sim['displacements']) - R['u']).max() / np.abs(R['u']).max()
    J = float(np.asarray(sim['compliance'])[0])
    e_J = abs(J - R['J']) / abs(R['J'])
    g = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    e_g = np.abs(g - R['grad']).max() / np.abs(R['grad']).max()
    print(f"{kind} device={device}: density {e_rho:.2e}, u {e_u:.2e}, J {e_J:.2e}, total gradient {e_g:.2e}")
    assert e_rho <= 1e-9 and e_u <= 1e-9 and e_J <= 1e-9 and e_g <= 1e-8
    if device:
        return
    chk = sim.check_totals('compliance', 'density_unfiltered', step=1e-4, n_dir=3, seed=0)
    print(f"{kind}: check_totals {chk['rel_error']}")
    assert max(chk['rel_error']) <= 1e-6, chk
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(3):
        d = rng.standard_normal(x0.size)
        vals = []
        for s in (1.0, -1.0):
            sim['density_unfiltered'] = x0 + s * 1e-5 * d
            sim.run()
            vals.append(float(np.asarray(sim['compliance'])[0]))
        fd = (vals[0] - vals[1]) / 2e-5
        worst = max(worst, abs(fd - g @ d) / abs(fd))
    print(f"{kind}: directional central differences {worst:.2e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("kind", ["helmholtz", "projected"])
def test_operation_products(gpu, kind):
    """compute_jacvec_product of the operation alone, both modes: fwd against central differences of compute (step 1e-5) to
    1e-6, rev against fwd as a transpose to 1e-9."""
    _, filt, mesh, _ = build_cantilever(kind)
    op = filt.operation
    n = mesh.n_cell
    rng = np.random.default_rng(8)
    x, d, a = rng.uniform(0.1, 0.9, n), rng.standard_normal(n), rng.standard_normal(n)

    def f(v):
        out = {}
        op.compute({'density_unfiltered': v}, out)
        return np.array(out['density'])

    fd = (f(x + 1e-5 * d) - f(x - 1e-5 * d)) / 2e-5
    d_out = {'density': np.zeros(n)}
    op.compute_jacvec_product({'density_unfiltered': x}, {'density_unfiltered': d}, d_out, 'fwd')
    d_in = {'density_unfiltered': np.zeros(n)}
    op.compute_jacvec_product({'density_unfiltered': x}, d_in, {'density': a}, 'rev')
    Jd, JTa = np.asarray(d_out['density']), np.asarray(d_in['density_unfiltered'])
    e_fd = np.abs(Jd - fd).max() / np.abs(fd).max()
    e_t = abs(a @ Jd - d @ JTa) / (np.linalg.norm(a) * np.linalg.norm(Jd))
    print(f"{kind}: fwd product against central differences {e_fd:.2e}, rev against fwd {e_t:.2e}")
    assert e_fd <= 1e-6 and e_t <= 1e-9
    with pytest.raises(ValueError):
        op.compute_jacvec_product({'density_unfiltered': x}, d_in, {'density': a}, 'sideways')
