"""GPU tests of the thermal expansion load of the SIMP elasticity (csrc/elast_thermal.hip, ``thermal=`` of the static
residuals and compliances) against the restatement tests/thermal_ref.py.

The meshes (tests/thermal_ref.py, MESHES) are those of tests/test_gpu_elast_body.py and the fan, whose hub row is longer
than 14 entries and whose slices carry dead visits.  L = 1, 3, 5 columns with distinct scales, one of them 0; theta is a random nodal
field and a uniform number.  RTOL: see the top of tests/test_gpu_elast_body.py."""
import functools

import numpy as np
import pytest

import elast_body_ref as br
import elasticity_ref as ref
import nonfinite as nf
import thermal_ref as tr
from elast_pc_ref import clamped_face
from thermal_ref import MESHES, mesh as _mesh

pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, -0.5, 0.0, 2.0, 0.25])
ALPHA, T_REF = 0.7, 0.4
RTOL = 1e-13


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------------------ the three kernels ----
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("name", MESHES)
def test_thermal_apply(gpu, name, L, uniform):
    from femo_amd import _lib
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh(name)
    x, conn, d, nc, nv = mesh.x, mesh.conn, mesh.tdim, mesh.n_cell, mesh.n_vert
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n = dev.n_dof
    s = SCALES[:L]
    method, mid = ("RAMP", _lib.ELAST_RAMP) if L == 3 else ("SIMP", _lib.ELAST_SIMP)
    rng = np.random.default_rng(12)
    rho, w, X = rng.uniform(0.05, 1.0, nc), rng.standard_normal(nc), rng.standard_normal((L, n))
    base, Th = rng.standard_normal((L, n)), rng.standard_normal(nv)
    theta = 1.3 - T_REF if uniform else Th - T_REF
    rv, wv, xv, bv = Vec(gpu, nc).set(rho), Vec(gpu, nc).set(w), Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(base.ravel())
    temp = 1.3 if uniform else Vec(gpu, nv).set(Th)
    yv, y1, tc, tn = Vec(gpu, L * n), Vec(gpu, n), Vec(gpu, nc), Vec(gpu, nv)
    N = lambda n_cols, sc, y, **kw: dev.thermal_apply(mid, "N", n_cols, sc, ALPHA, rv, temp, y, T_ref=T_REF, **kw)

    # N with w = C(rho): the load
    H = tr.thermal_load(x, conn, rho, theta, ALPHA, method)
    want = s[:, None] * H[None, :]
    Y = _columns(N(L, s, yv), L)
    err = np.abs(Y - want).max() / np.abs(want).max()
    print(f"{name} L={L} uniform={uniform}: N against the restatement {err:.1e}")
    assert err <= 1e-13
    assert np.array_equal(_columns(N(L, s, yv), L), Y)                                   # the same bits again
    for l in range(L):
        assert np.array_equal(np.array(N(1, s[l:l + 1], y1).get()), Y[l])                # independent of L
    if L >= 3:
        assert np.all(Y[2] == 0.0)                                                       # the zero scale
    Ya = _columns(N(L, s, yv, a=-1.5, base=bv), L)
    assert np.abs(Ya - (base - 1.5 * want)).max() <= 1e-13 * np.abs(base - 1.5 * want).max()
    Yb = _columns(N(L, s, yv, a=0.5, accumulate=True), L)
    assert np.abs(Yb - (base - want)).max() <= 1e-13 * np.abs(base - want).max()
    # N with w = C'(rho) x: dR/drho forward
    Hw = tr.thermal_H(x, conn, ref.penal_d(rho, method) * w, theta, ALPHA)
    Yw = _columns(N(L, s, yv, x=wv), L)
    assert np.abs(Yw - s[:, None] * Hw[None, :]).max() <= 1e-13 * np.abs(s).max() * np.abs(Hw).max()
    # zero_fixed on the clamped face: exact zeros there, the free dofs untouched
    mask = clamped_face(mesh)
    assert mask.any()
    dev.set_fixed(mask)
    Yz = _columns(N(L, s, yv, a=-1.5, base=bv, zero_fixed=True), L)
    assert np.all(Yz[:, mask == 1] == 0.0) and np.array_equal(Yz[:, mask == 0], Ya[:, mask == 0])

    # T_rho: the transpose of w -> N(C'(rho) w)
    T = lambda y, **kw: dev.thermal_apply(mid, "T_rho", L, s, ALPHA, rv, temp, y, T_ref=T_REF, x=xv, **kw)
    wantT = sum(s[l] * tr.thermal_T_rho(x, conn, rho, theta, X[l], ALPHA, method) for l in range(L))
    Tr = np.array(T(tc).get())
    errT = np.abs(Tr - wantT).max() / np.abs(wantT).max()
    print(f"{name} L={L} uniform={uniform}: T_rho against the restatement {errT:.1e}")
    assert errT <= 1e-13
    assert np.array_equal(np.array(T(tc).get()), Tr)
    T2 = np.array(T(tc, a=-2.0, accumulate=True).get())
    assert np.abs(T2 + wantT).max() <= 1e-13 * np.abs(wantT).max()
    lhs, rhs = np.sum(X * Yw), Tr @ w
    print(f"{name} L={L}: x.(N w) = {lhs:.15e}, (T_rho x).w = {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Yw)

    # T_temp: the transpose of theta -> N(C(rho); theta)
    dT = rng.standard_normal(nv)
    dv = Vec(gpu, nv).set(dT)
    Yt = _columns(dev.thermal_apply(mid, "N", L, s, ALPHA, rv, dv, yv), L)
    HT = tr.thermal_load(x, conn, rho, dT, ALPHA, method)
    assert np.abs(Yt - s[:, None] * HT[None, :]).max() <= 1e-13 * np.abs(s).max() * np.abs(HT).max()
    TT = lambda y, **kw: dev.thermal_apply(mid, "T_temp", L, s, ALPHA, rv, 0.0, y, x=xv, **kw)
    wantTT = sum(s[l] * tr.thermal_T_temp(x, conn, rho, X[l], ALPHA, method) for l in range(L))
    Tt = np.array(TT(tn).get())
    errTT = np.abs(Tt - wantTT).max() / np.abs(wantTT).max()
    print(f"{name} L={L}: T_temp against the restatement {errTT:.1e}")
    assert errTT <= 1e-13
    assert np.array_equal(np.array(TT(tn).get()), Tt)
    Tt2 = np.array(TT(tn, a=-2.0, accumulate=True).get())
    assert np.abs(Tt2 + wantTT).max() <= 1e-13 * np.abs(wantTT).max()
    lhs, rhs = np.sum(X * Yt), Tt @ dT
    print(f"{name} L={L}: x.(N dT) = {lhs:.15e}, (T_temp x).dT = {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Yt)


def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, ELAST_SIMP, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh("rect8x4")
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n, nc, nv = dev.n_dof, mesh.n_cell, mesh.n_vert
    rho, y, t = Vec(gpu, nc).fill(0.5), Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(0.0), Vec(gpu, nc)
    call = lambda product, L, y_, **kw: dev.thermal_apply(kw.pop("method", ELAST_SIMP), product, L, kw.pop("s", np.ones(max(L, 0))),
                                                          1e-2, kw.pop("rho", rho), kw.pop("temp", 1.0), y_, **kw)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            call("N", bad, y)
    with pytest.raises(FemoError, match="scales"):
        call("N", 3, y, s=np.ones(2))
    with pytest.raises(FemoError, match="product"):
        call("T", 2, y)
    with pytest.raises(FemoError, match="method"):
        call("N", 2, y, method=7)
    with pytest.raises(FemoError):
        call("N", 3, Vec(gpu, 3 * n - 1))
    with pytest.raises(FemoError, match="size"):
        call("N", 2, y, rho=Vec(gpu, nc - 1))
    with pytest.raises(FemoError, match="size"):
        call("N", 2, y, temp=Vec(gpu, nv - 1))
    with pytest.raises(FemoError, match="size"):
        call("N", 2, y, x=Vec(gpu, nc - 1))
    with pytest.raises(FemoError):
        call("T_rho", 2, t, x=Vec(gpu, 2 * n - 1))
    with pytest.raises(FemoError, match="size"):
        call("T_temp", 2, Vec(gpu, nv - 1), x=y)
    with pytest.raises(FemoError, match="needs x"):
        call("T_rho", 2, t)
    with pytest.raises(FemoError, match="aliases"):
        call("T_rho", 2, y, x=y)
    with pytest.raises(FemoError, match="aliases"):
        call("N", 2, y, base=y)
    with pytest.raises(FemoError, match="aliases"):
        call("T_rho", 2, rho, x=y)
    with pytest.raises(FemoError, match="fixed set"):
        call("N", 2, y, zero_fixed=True)
    with pytest.raises(FemoError, match="forward"):
        call("T_temp", 2, Vec(gpu, nv), x=y, base=y)
    assert np.all(np.array(call("N", ELAST_MAX_COLS, y, s=np.zeros(ELAST_MAX_COLS)).get()) == 0.0)


# ------------------------------------------------------------------------------------------- identity 1 on the device ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", ["square9j", "cube4j"])
def test_free_expansion(gpu, name, method):
    """Uniform theta, random rho, u = e x: the unmasked residual K(rho) u - F_th(rho, theta) is zero."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import ElasticityResidual, ThermalExpansion
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    mesh = _mesh(name)
    V = VectorFunctionSpace(mesh)
    u, rho = Function(V), Function(FunctionSpace(mesh, ("DG", 0)))
    form = ElasticityResidual(u, rho, None, method=method, thermal=ThermalExpansion(ALPHA, 1.3 + T_REF, T_ref=T_REF))
    rho.vector[:] = np.random.default_rng(3).uniform(0.05, 1.0, mesh.n_cell)
    u.vector[:] = tr.free_expansion(mesh.x, 1.3, ALPHA)
    res = np.array(form.assemble_vector(Vec(gpu, V.dim)).get())
    F = np.array(form.load().get())
    err = np.abs(res).max() / np.abs(F).max()
    print(f"{name} {method}: |K u - F_th| / max |F_th| = {err:.1e} (max |F_th| = {np.abs(F).max():.2f})")
    assert np.abs(F).max() > 0.01
    assert err <= 1e-12


# ----------------------------------------------------------------------------------------------------------- state ----
def _loads(mesh):
    """Three load cases clamped at x = 0: the thermal load alone, a traction with the thermal load reversed, the traction
    alone (scale 0)."""
    facets, tractions, _ = br.body_cases(mesh)
    return [None, facets[1], facets[2]], [None, tractions[1], tractions[2]], np.array([1.0, -0.5, 0.0])


@functools.lru_cache(maxsize=None)
def state_ref(name, k):
    """Step k: (density, temperature) = (0, 0), (1, 0), (1, 1); the restatement's loads and direct solves: read only."""
    mesh = _mesh(name)
    rho = np.random.default_rng(7 + min(k, 1)).uniform(0.05, 1.0, mesh.n_cell)
    T = np.random.default_rng(70 + k // 2).uniform(0.0, 2.0, mesh.n_vert)
    mask = clamped_face(mesh)
    facets, tractions, scales = _loads(mesh)
    K = ref.stiffness(mesh.x, mesh.conn, rho, "RAMP")
    H = tr.thermal_load(mesh.x, mesh.conn, rho, T - T_REF, ALPHA, "RAMP")
    n = mesh.tdim * mesh.n_vert
    F = [(np.zeros(n) if t is None else ref.traction_load(mesh.x, f, t)) + s * H for f, t, s in zip(facets, tractions, scales)]
    fixed = np.nonzero(mask)[0]
    return dict(rho=rho, T=T, K=K, F=F, u=[ref.solve_fixed(K, Fl, fixed) for Fl in F])


def _state_form(mesh, pc, body=False):
    from femo_amd.fea.elasticity import Measure, MultiLoadElasticityResidual, ThermalExpansion, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    facets, tractions, scales = _loads(mesh)
    d = mesh.tdim
    dss = [None if f is None else
           Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, f, np.full(len(f), 7, dtype=np.int32)))(7)
           for f in facets]
    V = VectorFunctionSpace(mesh)
    u, rho, T = Function(LoadCaseSpace(V, 3)), Function(FunctionSpace(mesh, ("DG", 0))), Function(FunctionSpace(mesh, ("CG", 1)))
    bodies = br.body_cases(mesh)[2] if body else None
    form = MultiLoadElasticityResidual(u, rho, tractions, dss, method="RAMP", preconditioner=pc, body_forces=bodies,
                                       thermal=ThermalExpansion(ALPHA, T, T_ref=T_REF, scales=scales))
    return form, u, rho, T, [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("name", ["rect8x4", "cube4j", "rect24x12"])
def test_state(gpu, name, pc):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    form, u, rho, T, bcs = _state_form(mesh, pc)
    assert form.functions() == (u, rho, T)
    form.rtol = RTOL
    n = form.n_dof
    for k in (0, 1, 2):                       # a new density, then a new temperature: each must reach the load and the rhs
        R = state_ref(name, k)
        if k != 2:
            rho.vector[:] = R["rho"]
        if k != 1:
            T.vector[:] = R["T"]
        form.solve_state(u, bcs)
        info = form.last_info["state"]
        U = np.array(u.vec.get()).reshape(3, n)
        Fd = np.array(form.load().get()).reshape(3, n)
        for l in range(3):
            err, errF = _maxrel(U[l], R["u"][l]), _maxrel(Fd[l], R["F"][l])
            print(f"{name} {pc} step {k} case {l}: {info['iterations'][l]} it, u {err:.1e}, F {errF:.1e}")
            assert info["converged"][l] == 1
            assert err <= 1e-9
            assert errF <= 1e-13
    # the residual K u - F(rho, T) at a state that is not the solution
    uh = np.random.default_rng(2).standard_normal(3 * n)
    u.vector[:] = uh
    res = np.array(form.assemble_vector(Vec(gpu, 3 * n)).get()).reshape(3, n)
    for l in range(3):
        want = R["K"] @ uh.reshape(3, n)[l] - R["F"][l]
        assert np.abs(res[l] - want).max() <= 1e-12 * np.abs(want).max()


def test_state_with_nonzero_supports(gpu):
    """Inhomogeneous Dirichlet values take the lifting path of the right-hand side: the thermal load must be in it."""
    from femo_amd.fea.utils_hip import dirichletbc
    from femo_amd.fea.function import VectorFunctionSpace
    mesh = _mesh("rect8x4")
    form, u, rho, T, _ = _state_form(mesh, "jacobi")
    form.rtol = RTOL
    R = state_ref("rect8x4", 0)
    rho.vector[:] = R["rho"]
    T.vector[:] = R["T"]
    fixed = np.nonzero(clamped_face(mesh))[0]
    form.solve_state(u, [dirichletbc(0.01, fixed.astype(np.int32), VectorFunctionSpace(mesh))])
    U = np.array(u.vec.get()).reshape(3, -1)
    for l in range(3):
        want = ref.solve_fixed(R["K"], R["F"][l], fixed, 0.01)
        assert _maxrel(U[l], want) <= 1e-9


# ------------------------------------------------------------------------------------------------- dR/drho and dR/dT ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", ["rect8x4", "cube4j", "rect24x12"])
def test_partials(gpu, name, method):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import MultiLoadElasticityResidual, ThermalExpansion
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _mesh(name)
    x, conn, d, nc, nv = mesh.x, mesh.conn, mesh.tdim, mesh.n_cell, mesh.n_vert
    _, tractions, bodies = br.body_cases(mesh)
    scales = np.array([1.0, -0.5, 0.0])
    V = VectorFunctionSpace(mesh)
    u, rho, T = Function(LoadCaseSpace(V, 3)), Function(FunctionSpace(mesh, ("DG", 0))), Function(FunctionSpace(mesh, ("CG", 1)))
    form = MultiLoadElasticityResidual(u, rho, tractions, method=method, body_forces=bodies,
                                       thermal=ThermalExpansion(ALPHA, T, T_ref=T_REF, scales=scales))
    n = form.n_dof
    rng = np.random.default_rng(9)
    rh, U, X = rng.uniform(0.05, 1.0, nc), rng.standard_normal((3, n)), rng.standard_normal((3, n))
    dr, Th, dT = rng.standard_normal(nc), rng.uniform(0.0, 2.0, nv), rng.standard_normal(nv)
    rho.vector[:] = rh
    u.vector[:] = U.ravel()
    T.vector[:] = Th
    D = form.partial_matrix(rho)
    assert D.getSizes() == (3 * n, nc)
    Dd = np.array(D.mult(Vec(gpu, nc).set(dr), Vec(gpu, 3 * n)).get()).reshape(3, n)
    DTx = np.array(D.multTranspose(Vec(gpu, 3 * n).set(X.ravel()), Vec(gpu, nc)).get())
    K0 = ref.element_matrices(x, conn)
    Hd = tr.thermal_H(x, conn, ref.penal_d(rh, method) * dr, Th - T_REF, ALPHA)
    want_T = np.zeros(nc)
    for l in range(3):
        b = np.zeros(d) if bodies[l] is None else bodies[l]
        want = br.drho_forward(x, conn, rh, U[l], dr, method, K0=K0) - br.body_load(x, conn, dr, b) - scales[l] * Hd
        err = _maxrel(Dd[l], want)
        print(f"{name} {method} case {l}: dR/drho d {err:.1e}")
        assert err <= 1e-12
        want_T += (ref.compliance_gradient(x, conn, rh, U[l], X[l], method, K0=K0) - br.body_drho_T(x, conn, X[l], b)
                   - scales[l] * tr.thermal_T_rho(x, conn, rh, Th - T_REF, X[l], ALPHA, method))
    errT = _maxrel(DTx, want_T)
    a, b = np.sum(X * Dd), dr @ DTx
    print(f"{name} {method}: dR/drho^T x {errT:.1e}; x.(D d) = {a:.15e}, d.(D^T x) = {b:.15e}")
    assert errT <= 1e-12
    assert abs(a - b) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Dd)

    G = form.partial_matrix(T)
    assert G.getSizes() == (3 * n, nv)
    assert G.new_row_vec().n == 3 * n and G.new_col_vec().n == nv
    Gd = np.array(G.mult(Vec(gpu, nv).set(dT), Vec(gpu, 3 * n)).get()).reshape(3, n)
    GTx = np.array(G.multTranspose(Vec(gpu, 3 * n).set(X.ravel()), Vec(gpu, nv)).get())
    HT = tr.thermal_load(x, conn, rh, dT, ALPHA, method)
    for l in (0, 1):
        assert _maxrel(Gd[l], -scales[l] * HT) <= 1e-12
    assert np.all(Gd[2] == 0.0)
    wantG = -sum(scales[l] * tr.thermal_T_temp(x, conn, rh, X[l], ALPHA, method) for l in range(3))
    errG = _maxrel(GTx, wantG)
    a, b = np.sum(X * Gd), dT @ GTx
    print(f"{name} {method}: dR/dT^T x {errG:.1e}; x.(G d) = {a:.15e}, d.(G^T x) = {b:.15e}")
    assert errG <= 1e-12
    assert abs(a - b) <= 1e-13 * np.linalg.norm(X) * np.linalg.norm(Gd)
    with pytest.raises(ValueError):
        form.partial_matrix(Function(FunctionSpace(mesh, ("CG", 1))))


def test_compliance(gpu):
    """J = sum_l w_l F_l(rho, T) . u_l and its three partials, with body forces beside the thermal load."""
    from femo_amd.fea.elasticity import MultiLoadCompliance, ThermalExpansion
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _mesh("cube4j")
    x, conn, nc, nv = mesh.x, mesh.conn, mesh.n_cell, mesh.n_vert
    facets, tractions, bodies = br.body_cases(mesh)
    scales, w = np.array([1.0, -0.5, 0.0]), np.array([1.0, 0.5, 2.0])
    V = VectorFunctionSpace(mesh)
    u, rho, T = Function(LoadCaseSpace(V, 3)), Function(FunctionSpace(mesh, ("DG", 0))), Function(FunctionSpace(mesh, ("CG", 1)))
    from femo_amd.fea.elasticity import Measure, meshtags
    dss = [None if f is None else
           Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 2, f, np.full(len(f), 7, dtype=np.int32)))(7) for f in facets]
    J = MultiLoadCompliance(u, tractions, dss, weights=w, body_forces=bodies, rho=rho, method="RAMP",
                            thermal=ThermalExpansion(ALPHA, T, T_ref=T_REF, scales=scales))
    assert J.functions() == (u, rho, T)
    rng = np.random.default_rng(4)
    rh, U, Th = rng.uniform(0.05, 1.0, nc), rng.standard_normal((3, V.dim)), rng.uniform(0.0, 2.0, nv)
    rho.vector[:] = rh
    u.vector[:] = U.ravel()
    T.vector[:] = Th
    H = tr.thermal_load(x, conn, rh, Th - T_REF, ALPHA, "RAMP")
    F = [wl * (Fl + s * H) for wl, Fl, s in zip(w, br.total_loads(mesh, rh, facets, tractions, bodies), scales)]
    want = sum(Fl @ Ul for Fl, Ul in zip(F, U))
    assert abs(J.assemble_scalar() - want) <= 1e-12 * sum(np.linalg.norm(Fl) * np.linalg.norm(Ul) for Fl, Ul in zip(F, U))
    assert _maxrel(np.array(J.assemble_derivative(u).get()), np.concatenate(F)) <= 1e-13
    g_rho = sum(w[l] * ((0.0 if bodies[l] is None else br.body_drho_T(x, conn, U[l], bodies[l]))
                        + scales[l] * tr.thermal_T_rho(x, conn, rh, Th - T_REF, U[l], ALPHA, "RAMP")) for l in range(3))
    assert _maxrel(np.array(J.assemble_derivative(rho).get()), g_rho) <= 1e-12
    g_T = sum(w[l] * scales[l] * tr.thermal_T_temp(x, conn, rh, U[l], ALPHA, "RAMP") for l in range(3))
    assert _maxrel(np.array(J.assemble_derivative(T).get()), g_T) <= 1e-12


# -------------------------------------------------------------------------------------------------------- refusals ----
def test_refusals(gpu):
    from femo_amd.fea.elasticity import ElasticityBuckling, ElasticityResidual, ThermalExpansion
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    mesh, other = _mesh("rect8x4"), _mesh("square9j")
    V = VectorFunctionSpace(mesh)
    u, rho = Function(V), Function(FunctionSpace(mesh, ("DG", 0)))
    with pytest.raises(NotImplementedError, match="state's mesh"):
        ElasticityResidual(u, rho, None, thermal=ThermalExpansion(1e-2, Function(FunctionSpace(other, ("CG", 1)))))
    with pytest.raises(NotImplementedError, match="CG"):
        ThermalExpansion(1e-2, Function(FunctionSpace(mesh, ("DG", 0))))
    with pytest.raises(NotImplementedError, match="CG"):
        ThermalExpansion(1e-2, Function(V))
    with pytest.raises(NotImplementedError, match="thermal loads are out of scope"):
        ElasticityBuckling(ElasticityResidual(u, rho, None, thermal=ThermalExpansion(1e-2, 1.0)), 2)


# ------------------------------------------------------------------------------------------- no change when absent ----
def test_zero_expansion_changes_nothing(gpu):
    """thermal=None and a ThermalExpansion with alpha = 0: the same bits in the load, the solution, the iteration count, J
    and the partials."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import Compliance, ElasticityResidual, Measure, ThermalExpansion, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh("rect8x4")
    facets, tractions, _ = br.body_cases(mesh)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets[1], np.full(len(facets[1]), 7, dtype=np.int32)))(7)
    V, Q, P = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0)), FunctionSpace(mesh, ("CG", 1))
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    rh = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    out = []
    for kind in (None, "uniform", "field"):
        u, rho, T = Function(V), Function(Q), Function(P)
        rho.vector[:] = rh
        T.vector[:] = np.random.default_rng(8).uniform(0.0, 2.0, mesh.n_vert)
        th = None if kind is None else ThermalExpansion(0.0, 1.5 if kind == "uniform" else T, T_ref=0.25)
        form = ElasticityResidual(u, rho, tractions[1], ds, thermal=th)
        J = Compliance(u, tractions[1], ds, thermal=th, rho=rho if th is not None else None)
        assert (form.thermal is None) == (th is None)
        form.solve_state(u, bcs)
        D = form.partial_matrix(rho)
        g = np.array(D.multTranspose(u.vec, Vec(gpu, mesh.n_cell)).get())
        dd = np.array(D.mult(Vec(gpu, mesh.n_cell).set(rh), Vec(gpu, V.dim)).get())
        out.append(dict(F=np.array(form.load().get()), u=np.array(u.vec.get()), it=form.last_info["state"]["iterations"],
                        J=J.assemble_scalar(), dJdu=np.array(J.assemble_derivative(u).get()),
                        dJdrho=np.array(J.assemble_derivative(rho).get()), g=g, dd=dd,
                        res=np.array(form.assemble_vector(Vec(gpu, V.dim)).get())))
        if kind == "field":
            assert np.all(np.array(J.assemble_derivative(T).get()) == 0.0)
            assert np.all(np.array(form.partial_matrix(T).multTranspose(u.vec, Vec(gpu, mesh.n_vert)).get()) == 0.0)
    a = out[0]
    for b in out[1:]:
        assert a["it"] == b["it"] and a["J"] == b["J"]
        for k in ("F", "u", "dJdu", "dJdrho", "g", "dd", "res"):
            assert np.array_equal(a[k], b[k]), k
    assert np.all(a["dJdrho"] == 0.0) and np.abs(a["u"]).max() > 0.0


# ------------------------------------------------------------------------------------------------ non-finite inputs ----
@pytest.mark.parametrize("value", nf.VALUES)
def test_nonfinite_reaches_the_load(gpu, value):
    """No output hides a non-finite state: one poisoned density cell or temperature vertex shows in the load and in both
    transposes wherever the restatement has it, and nowhere else; the next clean call gives the clean bits."""
    from femo_amd import _lib
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh("rect24x12")
    x, conn, d, nc, nv = mesh.x, mesh.conn, mesh.tdim, mesh.n_cell, mesh.n_vert
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n, L, s = dev.n_dof, 3, SCALES[:3]
    rng = np.random.default_rng(21)
    rho, Th, X = rng.uniform(0.1, 1.0, nc), rng.uniform(0.5, 2.0, nv), rng.standard_normal((L, n))
    xv = Vec(gpu, L * n).set(X.ravel())

    def device(r, t):
        rv, tv = Vec(gpu, nc).set(r), Vec(gpu, nv).set(t)
        N = _columns(dev.thermal_apply(_lib.ELAST_RAMP, "N", L, s, ALPHA, rv, tv, Vec(gpu, L * n), T_ref=T_REF), L)
        Tr = np.array(dev.thermal_apply(_lib.ELAST_RAMP, "T_rho", L, s, ALPHA, rv, tv, Vec(gpu, nc), T_ref=T_REF, x=xv).get())
        Tt = np.array(dev.thermal_apply(_lib.ELAST_RAMP, "T_temp", L, s, ALPHA, rv, 0.0, Vec(gpu, nv), x=xv).get())
        return N, Tr, Tt

    def restated(r, t):
        with np.errstate(all="ignore"):
            H = tr.thermal_load(x, conn, r, t - T_REF, ALPHA, "RAMP")
            return (s[:, None] * H[None, :], sum(s[l] * tr.thermal_T_rho(x, conn, r, t - T_REF, X[l], ALPHA, "RAMP") for l in range(L)),
                    sum(s[l] * tr.thermal_T_temp(x, conn, r, X[l], ALPHA, "RAMP") for l in range(L)))

    clean = device(rho, Th)
    bad = []
    for c in nf.cell_positions(nc):
        cells = nf.one_cell(nc, c)
        verts = nf.entries_of_cells(conn, cells, nv)
        got, want = device(nf.poison(rho, c, value), Th), restated(nf.poison(rho, c, value), Th)
        deps = (np.tile(nf.vertex_dofs(verts, d), (L, 1)), cells, verts)
        for k, name in enumerate(("N", "T_rho", "T_temp")):
            bad += nf.violations(got[k], want[k], clean[k], deps[k], label=f"rho[{c}] {name}")
    for e in nf.positions(conn, 1):
        cells = nf.cells_of_vertex(conn, e)
        verts = nf.entries_of_cells(conn, cells, nv)
        got, want = device(rho, nf.poison(Th, e, value)), restated(rho, nf.poison(Th, e, value))
        deps = (np.tile(nf.vertex_dofs(verts, d), (L, 1)), cells, np.zeros(nv, dtype=bool))
        for k, name in enumerate(("N", "T_rho", "T_temp")):
            bad += nf.violations(got[k], want[k], clean[k], deps[k], label=f"T[{e}] {name}")
    assert not bad, "\n".join(bad)
    again = device(rho, Th)
    assert all(np.array_equal(a, b) for a, b in zip(again, clean))


def test_nonfinite_state_is_refused(gpu):
    """A NaN temperature or density reaches the load; the solve refuses it through its non-finite right-hand-side norm, the
    compliance is non-finite, and the next clean call gives the clean bits."""
    from femo_amd.fea.elasticity import Compliance, ThermalExpansion
    mesh = _mesh("rect8x4")
    form, u, rho, T, bcs = _state_form(mesh, "jacobi")
    form.rtol = RTOL
    R = state_ref("rect8x4", 0)
    rho.vector[:] = R["rho"]
    T.vector[:] = R["T"]
    form.solve_state(u, bcs)
    clean = np.array(u.vec.get())
    for which in ("T", "rho"):
        fn, good = (T, R["T"]) if which == "T" else (rho, R["rho"])
        fn.vector[:] = nf.poison(good, 5, np.nan)
        assert not np.all(np.isfinite(np.array(form.load().get())))
        with pytest.raises(RuntimeError):
            form.solve_state(u, bcs)
        fn.vector[:] = good
        form.solve_state(u, bcs)
        assert np.array_equal(np.array(u.vec.get()), clean)
    # the compliance of a single-column state with a poisoned temperature
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    V = VectorFunctionSpace(mesh)
    u1, T1 = Function(V), Function(FunctionSpace(mesh, ("CG", 1)))
    u1.vector[:] = np.ones(V.dim)
    T1.vector[:] = nf.poison(R["T"], 5, np.inf)
    J = Compliance(u1, (0.0, -0.25), thermal=ThermalExpansion(ALPHA, T1), rho=rho)
    assert not np.isfinite(J.assemble_scalar())
    T1.vector[:] = R["T"]
    assert np.isfinite(J.assemble_scalar())
