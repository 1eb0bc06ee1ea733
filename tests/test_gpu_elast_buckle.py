"""GPU tests of the buckling path of the SIMP elasticity (csrc/elast_buckle.hip, `DeviceElasticity.buckle`,
`ElasticityBuckling`, `BucklingAggregate`) against the restatement tests/elast_buckle_ref.py and its dense eigh.

The meshes are those of tests/test_gpu_elast_eig.py: less than one wave of rows (rect8x4), the two jittered ones, and two
with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343).  Clamped on x = 0, a compressive unit traction
(-1, 0[, 0]) on the face x = x_max, rho = default_rng(7).uniform(0.3, 1), start block
default_rng(1).standard_normal((n_free, L)).  Under this load the positive mu = 1 / lambda dominate on every case (mu_1 between
20 and 108, no negative mu beyond 0.52 in magnitude: tests/test_elast_buckle_host.py), so the sign limitation of the
iteration is exercised by `test_tensile_load_fails` alone.

The outer iteration count of `buckle` is bounded by that of the restated iteration from the same start block with
`pcg_multi` from a zero first guess at the same inner tolerance, plus 10 % and at least 2, as in test_eigs.  Both inner
solves stop on r.M^-1 r relative to that of the right-hand side B; the inner tolerance 1e-12 lies three decades below the
outer rtol 1e-9, so the outer count is that of exact solves (tests/test_elast_buckle_host.py: equal on every case) whatever
the preconditioner is; the restatement therefore runs block-Jacobi, the cheaper one on the CPU, for both device
preconditioners.

MEASURED on the MI355X (SIMP and RAMP, all meshes and both preconditioners; the tests print every figure):
  cell stress 4.5e-15, K_G x 4.2e-15, buckle_du 9.5e-16, buckle_drho 1.1e-15 plain and accumulated (2.1e-16 against eig_drho
  without the stress term), each of the largest entry and at the most
  load factor error against the dense eigh  4.9e-13 at the most (rect24x12; 5e-14 or better on the other meshes); bound 1e-8
  outer steps, device / restatement         equal on all 28 cases: 15 ... 31 for (1, 3), 31 ... 85 for (3, 8)
  inner PCG iterations per outer step       58 ... 103 (multilevel) and 78 ... 112 (block-Jacobi: 1168 ... 9518 over a whole solve,
                                            within 2 of the restatement's)
  reported residuals                        2.3e-10 ... 1.0e-9, bound 1e-9; within a factor 2 of the recomputed ones
  warm start after a change of 1e-3 in rho  24 -> 15 outer steps (rect8x4), 27 -> 15 (cube6j); no assembly besides the state's
  J through FEA / Simulator                 3.9e-13 at the most; bound 1e-8
  total dJ/drho against the restated total  1.5e-10 at the most (cube4j; 8.5e-14 with the body force); bound 1e-6
  directional central differences of J      1.9e-9 on rect24x12; bound 1e-5
  tensile load, (3, 3), 40 outer steps      all three Ritz values negative: raises "block is too small ... no positive load factor"
  buckle, eigs, buckle on one handle        the bits of fresh handles (rect8x4, cube4j; block-Jacobi)
"""
import functools

import numpy as np
import pytest

import elast_buckle_ref as bk
import elast_eig_ref as er
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BOTH_PC = ("rect8x4", "cube4j")              # one 2-D and one 3-D mesh run both preconditioners
RTOL, PCG_RTOL = 1e-9, 1e-12
BODY = (0.0, -0.5)                           # the body force of the one body-load case (rect8x4, RAMP)


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


def _rho(mesh, lo=0.3):
    return np.random.default_rng(7).uniform(lo, 1.0, mesh.n_cell)


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@functools.lru_cache(maxsize=None)
def problem(name, method):
    """The restated state under the compressive end load, K, K_G and the nine smallest dense load factors: built once, read
    only."""
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh)
    S = bk.state(mesh, rho, mask, method)
    D = bk.dense_buckling(S["K"], S["KG"], mask, 9)
    return dict(mesh=mesh, mask=mask, rho=rho, K=S["K"], KG=S["KG"], u=S["u"], lam=D["lam"], Phi=D["Phi"])


@functools.lru_cache(maxsize=None)
def restated_iteration(name, method, n_modes, block):
    """The restated iteration with the zero-guess `pcg_multi` (block-Jacobi) at the device's tolerances from its start block."""
    P = problem(name, method)
    d = P["mesh"].tdim
    A = pr.masked_operator(P["K"], P["mask"])
    Dinv = pr.invert_blocks(pr.block_diagonal(A, d))
    jacobi = lambda r: np.einsum("nij,nj->ni", Dinv, r.reshape(-1, d)).ravel()
    out = bk.block_power_iteration(P["K"], P["KG"], P["mask"], er.start_block(P["mask"], block), n_modes,
                                   bk.zero_guess_pcg_solver(A, jacobi, P["mask"], PCG_RTOL), rtol=RTOL)
    assert out["converged"]
    return out


def _device(gpu, mesh, method=None, rho=None, fixed=True):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    if fixed:
        dev.set_fixed(clamped_face(mesh))
    rv = None
    if rho is not None:
        rv = Vec(gpu, mesh.n_cell).set(rho)
        if method is not None:
            dev.assemble(METHODS[method], rv)
    return dev, rv


# ------------------------------------------------------------------------------------------------------ the kernels ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_cell_stress(gpu, name, method):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    P = problem(name, method)
    mesh, d = P["mesh"], P["mesh"].tdim
    dev, rv = _device(gpu, mesh, rho=P["rho"], fixed=False)
    uv, out = Vec(gpu, dev.n_dof).set(P["u"]), Vec(gpu, d * (d + 1) // 2 * mesh.n_cell)
    got = _columns(dev.geom_stress(METHODS[method], rv, uv, out), d * (d + 1) // 2)
    want = bk.stress_components(bk.cell_stress(mesh.x, mesh.conn, P["rho"], P["u"], method))
    err = _maxrel(got, want)
    print(f"{name} {method}: cell stress against the restatement {err:.1e}")
    assert err <= 1e-13
    assert np.array_equal(_columns(dev.geom_stress(METHODS[method], rv, uv, out), d * (d + 1) // 2), got)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("name", MESHES)
def test_geom_apply(gpu, name, L):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    P = problem(name, "SIMP")
    mesh, mask, KG = P["mesh"], P["mask"], P["KG"]
    dev, rv = _device(gpu, mesh, rho=P["rho"])
    n, a = dev.n_dof, -1.5
    dev.geom_stress(METHODS["SIMP"], rv, Vec(gpu, n).set(P["u"]))
    rng = np.random.default_rng(12)
    X, Z = rng.standard_normal((L, n)), rng.standard_normal((L, n))
    xv, zv, yv, y1, x1 = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(Z.ravel()), Vec(gpu, L * n), Vec(gpu, n), Vec(gpu, n)
    Y = _columns(dev.geom_apply_multi(L, xv, yv, a=a), L)
    want = a * (KG @ X.T).T
    err = _maxrel(Y, want)
    print(f"{name} L={L}: K_G x against the restatement {err:.1e}")
    assert err <= 1e-13                                               # sums over the at most ~30 cells around a vertex
    assert np.array_equal(_columns(dev.geom_apply_multi(L, xv, yv, a=a), L), Y)          # the same bits again
    for l in range(L):                                                # independent of L
        assert np.array_equal(np.array(dev.geom_apply_multi(1, x1.set(X[l]), y1, a=a).get()), Y[l])
    # symmetric: x . K_G z = z . K_G x
    GZ = _columns(dev.geom_apply_multi(L, zv, yv, a=a), L)
    for l in range(L):
        assert abs(X[l] @ GZ[l] - Z[l] @ Y[l]) <= 1e-13 * np.linalg.norm(X[l]) * np.linalg.norm(GZ[l])
    # masked: (K_G)_ff -- exact zeros on the fixed dofs, fixed entries of x ignored
    Ym = _columns(dev.geom_apply_multi(L, xv, yv, masked=True, a=a), L)
    wantm = a * (er.masked(KG, mask) @ X.T).T
    assert np.all(Ym[:, mask == 1] == 0.0)
    assert _maxrel(Ym, wantm) <= 1e-13
    X0 = np.where(mask[None, :] == 1, 0.0, X)
    assert np.array_equal(_columns(dev.geom_apply_multi(L, Vec(gpu, L * n).set(X0.ravel()), yv, masked=True, a=a), L), Ym)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_buckle_du(gpu, name, method, L):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    mesh = _mesh(name)
    rho = _rho(mesh, 0.02)
    dev, rv = _device(gpu, mesh, rho=rho, fixed=False)
    n = dev.n_dof
    rng = np.random.default_rng(5)
    Phi, w = rng.standard_normal((L, n)), rng.standard_normal(L)
    pv, out = Vec(gpu, L * n).set(Phi.ravel()), Vec(gpu, n)
    got = np.array(dev.buckle_du(METHODS[method], L, rv, pv, w, out).get())
    err = _maxrel(got, bk.buckle_du(mesh.x, mesh.conn, rho, Phi.T, w, method))
    print(f"{name} {method} L={L}: buckle_du {err:.1e}")
    assert err <= 1e-12
    assert np.array_equal(np.array(dev.buckle_du(METHODS[method], L, rv, pv, w, out).get()), got)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_buckle_drho(gpu, name, method, L):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    mesh = _mesh(name)
    rho = _rho(mesh, 0.02)
    dev, rv = _device(gpu, mesh, rho=rho, fixed=False)
    n, nc = dev.n_dof, mesh.n_cell
    rng = np.random.default_rng(6)
    Phi, u, w1, w2, base = (rng.standard_normal((L, n)), rng.standard_normal(n), rng.standard_normal(L), rng.standard_normal(L),
                            rng.standard_normal(nc))
    pv, uv, yv = Vec(gpu, L * n).set(Phi.ravel()), Vec(gpu, n).set(u), Vec(gpu, nc)
    want = bk.buckle_drho(mesh.x, mesh.conn, rho, u, Phi.T, w1, w2, method)
    g = np.array(dev.buckle_drho(METHODS[method], L, rv, uv, pv, w1, w2, yv).get())
    err = _maxrel(g, want)
    ga = np.array(dev.buckle_drho(METHODS[method], L, rv, uv, pv, w1, w2, yv.set(base), accumulate=True).get())
    erra = _maxrel(ga, base + want)
    # without the stress term it is the stiffness part of eig_drho (no mass: density 0) with c = w1
    gk = np.array(dev.buckle_drho(METHODS[method], L, rv, uv, pv, w1, np.zeros(L), yv).get())
    ge = np.array(dev.eig_drho(METHODS[method], L, rv, pv, np.ones(L), w1, Vec(gpu, nc), density=0.0).get())
    errk = _maxrel(gk, ge)
    print(f"{name} {method} L={L}: buckle_drho {err:.1e}, accumulated {erra:.1e}, against eig_drho without the stress term {errk:.1e}")
    assert err <= 1e-12 and erra <= 1e-12 and errk <= 1e-12


# -------------------------------------------------------------------------------------------------------- the solve ----
def _buckle_cases():
    for name in MESHES:
        for pc in (("jacobi", "multilevel") if name in BOTH_PC else ("multilevel",)):
            yield name, pc


@pytest.mark.parametrize("n_modes,block", [(1, 3), (3, 8)])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name,pc", list(_buckle_cases()))
def test_buckle(gpu, name, pc, method, n_modes, block):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    P = problem(name, method)
    mesh, mask = P["mesh"], P["mask"]
    dev, rv = _device(gpu, mesh, method, P["rho"])
    if pc == "multilevel":
        dev.pc_setup()
    n = dev.n_dof
    uv = Vec(gpu, n).set(P["u"])
    xv = Vec(gpu, block * n).set(er.start_block(mask, block).ravel())
    lam, info = dev.buckle(n_modes, rv, uv, xv, block=block, method=METHODS[method], rtol=RTOL, pcg_rtol=PCG_RTOL, pc=pc)
    R = restated_iteration(name, method, n_modes, block)
    err = (np.abs(lam[:n_modes] - P["lam"][:n_modes]) / P["lam"][:n_modes]).max()
    print(f"{name} {pc} {method} ({n_modes}, {block}): load factor error {err:.1e}, outer steps {info['outer_iterations']} "
          f"(restatement {R['outer']}), {info['pcg_iterations']} PCG iterations (restatement, block-Jacobi: {R['pcg']}), "
          f"residuals {info['residual'][:n_modes].max():.1e}")
    assert info["converged"] == 1
    assert err <= 1e-8                                                # ten times the residual level
    assert np.all(lam[:n_modes] > 0.0) and np.all(np.diff(lam[:n_modes]) >= 0.0)
    Phi = _columns(xv, block)
    assert np.all(Phi[:, mask == 1] == 0.0)
    assert np.all(Phi[np.arange(block), np.argmax(np.abs(Phi), axis=1)] > 0.0)
    kv, gv = Vec(gpu, block * n), Vec(gpu, block * n)
    dev.apply_multi(block, xv, kv, masked=True)
    dev.geom_apply_multi(block, xv, gv, masked=True, a=-1.0)          # the stress buffer is the one the solve filled
    G = dev.block_gram(block, xv, block, kv)
    assert np.abs(G - np.eye(block)).max() <= 1e-10
    KP, GP = _columns(kv, block), _columns(gv, block)
    mu = 1.0 / lam
    res = np.linalg.norm(GP - mu[:, None] * KP, axis=1) / (np.abs(mu) * np.linalg.norm(KP, axis=1))
    assert np.all(info["residual"][:n_modes] <= RTOL)
    for k in range(n_modes):
        assert 0.5 * res[k] <= info["residual"][k] <= 2.0 * res[k] or max(res[k], info["residual"][k]) <= 1e-13, (k, res, info)
    assert info["outer_iterations"] <= R["outer"] + max(2.0, 0.1 * R["outer"])


@pytest.mark.parametrize("name", ["rect8x4", "cube4j"])
def test_solves_leave_no_trace(gpu, name):
    """`buckle` and `eigs` run through one block iteration on the handle's shared reserves (the right-hand-side block, the
    Gram partials, the PCG work vectors): buckle (1, 3), eigs (3, 5) and buckle (1, 3) again, interleaved on one handle, give
    the bits of the same calls on fresh handles -- lambda, the residuals, both iteration counts and the modes.  Block-Jacobi
    only: the multilevel preconditioner adds with fp64 atomics and is not bit-repeatable.  MEASURED on the MI355X: equal bits
    on both meshes, with the library of the commit before the two loops became one as well."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    P = problem(name, "SIMP")
    mesh, mask = P["mesh"], P["mask"]

    def handle():
        dev, rv = _device(gpu, mesh, "SIMP", P["rho"])
        return dev, rv, Vec(gpu, dev.n_dof).set(P["u"])

    def buckle(dev, rv, uv):
        xv = Vec(gpu, 3 * dev.n_dof).set(er.start_block(mask, 3).ravel())
        lam, info = dev.buckle(1, rv, uv, xv, block=3, method=METHODS["SIMP"], rtol=RTOL, pcg_rtol=PCG_RTOL, pc="jacobi")
        return lam, info, _columns(xv, 3)

    def eigs(dev, rv):
        xv = Vec(gpu, 5 * dev.n_dof).set(er.start_block(mask, 5).ravel())
        lam, info = dev.eigs(3, rv, xv, block=5, rtol=RTOL, pcg_rtol=PCG_RTOL, pc="jacobi")
        return lam, info, _columns(xv, 5)

    fresh_buckle = buckle(*handle())
    fresh_eigs = eigs(*handle()[:2])
    dev, rv, uv = handle()
    mixed = [buckle(dev, rv, uv), eigs(dev, rv), buckle(dev, rv, uv)]
    for what, (lam, info, Phi), (lam0, info0, Phi0) in zip(("buckle", "eigs", "buckle again"), mixed,
                                                           (fresh_buckle, fresh_eigs, fresh_buckle)):
        print(f"{name} {what}: lambda {lam}, fresh {lam0}; outer steps {info['outer_iterations']} / {info0['outer_iterations']}, "
              f"PCG iterations {info['pcg_iterations']} / {info0['pcg_iterations']}, modes differ by {np.abs(Phi - Phi0).max():.1e}")
        assert info["converged"] == 1 and info0["converged"] == 1
        assert np.array_equal(lam, lam0) and np.array_equal(info["residual"], info0["residual"])
        assert info["outer_iterations"] == info0["outer_iterations"] and info["pcg_iterations"] == info0["pcg_iterations"]
        assert np.array_equal(Phi, Phi0)


def _setup(mesh, method="SIMP", pc="multilevel", body=None, sign=-1.0):
    """(residual, u, rho, V, bcs, ds, traction) of the clamped mesh under the end-face traction."""
    from femo_amd.fea.elasticity import Constant, ElasticityResidual, Measure, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    u, rho = Function(V), Function(Q)
    facets = bk.end_face(mesh)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, facets, np.full(len(facets), 7, dtype=np.int32)))(7)
    t = Constant(mesh, bk.end_traction(mesh, sign))
    res = ElasticityResidual(u, rho, t, ds, method=method, preconditioner=pc, body_force=body)
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    return res, u, rho, V, bcs


@pytest.mark.parametrize("name", ["rect8x4", "cube6j"])
def test_warm_start(gpu, name):
    """A second solve after a change of 1e-3 in the density (state re-solved) starts from the modes of the first; unchanged
    (rho, u) do not solve at all; K is the residual's own: the handle keeps the residual's ownership key and is not
    assembled by the buckling object."""
    P = problem(name, "SIMP")
    mesh = P["mesh"]
    res, u, rho, V, bcs = _setup(mesh)
    rho.vector[:] = P["rho"]
    res.solve_state(u, bcs)
    dev = res.device()
    owner = dev._owner
    assert owner[-1] == id(res)
    assemblies = []
    assemble = dev.assemble
    dev.assemble = lambda *a, **k: (assemblies.append(1), assemble(*a, **k))[1]
    try:
        _warm_start(name, P, res, u, rho, bcs, dev, owner, assemblies)
    finally:
        del dev.assemble                                              # the handle is shared by the tests on this mesh


def _warm_start(name, P, res, u, rho, bcs, dev, owner, assemblies):
    from femo_amd.fea.elasticity import ElasticityBuckling
    from femo_amd.fea.utils_hip import LAST_KSP_INFO
    mesh = P["mesh"]
    buck = ElasticityBuckling(res, 2, block=8)
    n0 = len(LAST_KSP_INFO)
    lam = buck.load_factors()
    cold = buck.last_info["outer_iterations"]
    assert LAST_KSP_INFO[-1]["kind"] == "elasticity_buckling" and len(LAST_KSP_INFO) == n0 + 1
    assert dev._owner == owner and not assemblies                     # the residual's K, no assembly of our own
    assert (np.abs(lam - P["lam"][:2]) / P["lam"][:2]).max() <= 1e-8
    assert np.array_equal(buck.load_factors(), lam) and len(LAST_KSP_INFO) == n0 + 1      # cached
    rho2 = P["rho"] * (1.0 + 1e-3 * np.random.default_rng(2).uniform(-1.0, 1.0, mesh.n_cell))
    rho.vector[:] = rho2
    res.solve_state(u, bcs)
    assert len(assemblies) == 1 and dev._owner[-1] == id(res)        # the state solve's
    lam2 = buck.load_factors()
    warm = buck.last_info["outer_iterations"]
    assert len(assemblies) == 1 and dev._owner[-1] == id(res)
    S2 = bk.state(mesh, rho2, P["mask"], "SIMP")
    want = bk.dense_buckling(S2["K"], S2["KG"], P["mask"], 2)["lam"]
    print(f"{name}: {cold} outer steps cold, {warm} warm")
    assert (np.abs(lam2 - want) / want).max() <= 1e-8
    assert warm < cold


# --------------------------------------------------------------------------------------------------------- the form ----
def _simulator(mesh, method, rho0, body=None):
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, VectorFunctionSpace,
                                      buckling_aggregate, locate_dofs_geometrical, meshtags)
    fea = FEA(mesh)
    fea.REPORT = False
    fea.consistent_bc_partials = True          # dJ/du of the load factors is non-zero on the clamped dofs
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(V)
    facets = bk.end_face(mesh)
    ds = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, mesh.tdim - 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    res = pdeRes(u_fn, TestFunction(V), rho_fn, Constant(mesh, bk.end_traction(mesh)), dss=ds, method=method,
                 preconditioner="multilevel", body_force=body)
    form = buckling_aggregate(res, n_modes=2, p=8.0, block=8)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='buckling', type='scalar', form=form, arguments=['displacements', 'density'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    model.create_input('density', shape=mesh.n_cell, val=rho0)
    model.add_design_variable('density', upper=1.0, lower=1e-4)
    model.add_objective('buckling')
    return Simulator(model), form


def _form_cases():
    for name in MESHES:
        for method in ("SIMP", "RAMP"):
            yield name, method, None
    yield "rect8x4", "RAMP", BODY


@pytest.mark.parametrize("name,method,body", list(_form_cases()))
def test_form(gpu, name, method, body):
    """`BucklingAggregate` registered through FEA.add_output: J and the total dJ/drho through OutputOperation and the
    framework's adjoint solve against the restatement's dense load factors and its adjoint total.  n_modes = 2 never
    splits a cluster (lambda_3 / lambda_2 >= 1.14)."""
    mesh = _mesh(name)
    mask, rho = clamped_face(mesh), _rho(mesh)
    sim, form = _simulator(mesh, method, rho, body)
    sim.run()
    T = bk.total_gradient(mesh, rho, mask, 2, 8.0, method, body=body)
    errJ = abs(float(sim['buckling'][0]) - T["J"]) / T["J"]
    gd = np.asarray(sim.compute_totals('buckling', 'density')).ravel()
    errg = _maxrel(gd, T["grad"])
    print(f"{name} {method} body={body}: J {errJ:.1e}, total dJ/drho {errg:.1e} "
          f"({form.buckling.last_info['outer_iterations']} outer steps)")
    assert errJ <= 1e-8
    assert errg <= 1e-6                                               # eigenvector error of the order rtol / gap


def test_directional_derivative(gpu):
    """Central differences of the device's own J (state re-solved) along one direction on rect24x12, step 1e-5, 1e-5
    relative, as in test_gpu_elast_eig.py: the direction has positive entries, so that the derivative is of the size of J
    itself and the rounding of J stays below the bound after the division."""
    mesh = _mesh("rect24x12")
    rho = _rho(mesh)
    sim, _ = _simulator(mesh, "SIMP", rho)
    sim.run()
    g = np.asarray(sim.compute_totals('buckling', 'density')).ravel()
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h, vals = 1e-5, []
    for s in (+1.0, -1.0):
        sim['density'] = rho + s * h * d
        sim.run()
        vals.append(float(np.asarray(sim['buckling']).ravel()[0]))
    fd, an = (vals[0] - vals[1]) / (2 * h), float(g @ d)
    print(f"rect24x12: directional derivative {an:.9e}, central differences {fd:.9e}, {abs(fd - an) / abs(an):.1e}")
    assert abs(fd - an) <= 1e-5 * abs(an)


# ------------------------------------------------------------------------------------------------ limits and errors ----
def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import (METHODS, BucklingAggregate, ElasticityBuckling, MultiLoadElasticityResidual,
                                         buckling_aggregate)
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    mesh = _mesh("rect8x4")
    rho = _rho(mesh)
    SIMP = METHODS["SIMP"]
    dev, rv = _device(gpu, mesh, rho=rho, fixed=False)
    n, nc = dev.n_dof, mesh.n_cell
    big, y, cells = Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(1.0), Vec(gpu, (ELAST_MAX_COLS + 1) * n), Vec(gpu, nc)
    uv = Vec(gpu, n).fill(0.5)
    w = np.ones(ELAST_MAX_COLS + 1)
    with pytest.raises(FemoError, match="geom_stress"):
        dev.geom_apply_multi(2, big, y)                               # no cell stress yet
    dev.geom_stress(SIMP, rv, uv)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.geom_apply_multi(bad, big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.buckle_du(SIMP, bad, rv, big, w[:bad], uv)
        with pytest.raises(FemoError, match="columns"):
            dev.buckle_drho(SIMP, bad, rv, uv, big, w[:bad], w[:bad], cells)
        with pytest.raises(FemoError, match="columns"):
            dev.buckle(1, rv, uv, big, block=bad)
    with pytest.raises(FemoError):                                    # sizes
        dev.geom_apply_multi(3, Vec(gpu, 3 * n - 1), y)
    with pytest.raises(FemoError):
        dev.geom_stress(SIMP, rv, Vec(gpu, n - 1))
    with pytest.raises(FemoError):
        dev.buckle_du(SIMP, 3, rv, big, w[:3], Vec(gpu, n - 1))
    with pytest.raises(FemoError):
        dev.buckle_drho(SIMP, 3, rv, uv, big, w[:3], w[:3], Vec(gpu, nc - 1))
    with pytest.raises(FemoError):
        dev.buckle_du(SIMP, 3, rv, big, w[:2], Vec(gpu, n))          # weights
    with pytest.raises(FemoError):
        dev.buckle_drho(SIMP, 3, rv, uv, big, w[:3], w[:2], cells)
    with pytest.raises(FemoError, match="aliases"):
        dev.geom_apply_multi(2, y, y)
    with pytest.raises(FemoError, match="aliases"):
        dev.buckle_du(SIMP, 1, rv, big, w[:1], big)
    with pytest.raises(FemoError, match="aliases"):
        dev.buckle_drho(SIMP, 1, rv, uv, big, w[:1], w[:1], rv)
    with pytest.raises(FemoError, match="fixed set"):
        dev.geom_apply_multi(2, big, y, masked=True)
    with pytest.raises(FemoError, match="assemble"):
        dev.buckle(1, rv, uv, big, block=3)                           # no K yet
    dev.assemble(SIMP, rv)
    with pytest.raises(FemoError, match="fixed set"):
        dev.buckle(1, rv, uv, big, block=3)                           # K is singular without supports
    dev.set_fixed(clamped_face(mesh))
    dev.assemble(SIMP, rv)
    with pytest.raises(FemoError, match="modes"):
        dev.buckle(4, rv, uv, big, block=3)
    with pytest.raises(FemoError, match="aliases"):
        dev.buckle(1, rv, big, big, block=1)
    with pytest.raises(ValueError):
        dev.buckle(1, rv, uv, big, block=3, pc="ilu")
    with pytest.raises(FemoError, match="multilevel"):
        dev.buckle(1, rv, uv, big, block=3, pc="multilevel")          # no pc_setup
    # the forms
    res, u, rho_fn, V, bcs = _setup(mesh, pc="jacobi")
    with pytest.raises(NotImplementedError):
        ElasticityBuckling(object(), 2)
    UL = Function(LoadCaseSpace(V, 2))
    t = bk.end_traction(mesh)
    with pytest.raises(NotImplementedError, match="load cases"):
        ElasticityBuckling(MultiLoadElasticityResidual(UL, rho_fn, [t, t]), 2)
    with pytest.raises(ValueError):
        ElasticityBuckling(res, 4, block=3)
    with pytest.raises(ValueError):
        buckling_aggregate(res, n_modes=2, p=0.5)
    with pytest.raises(NotImplementedError):
        BucklingAggregate(res)
    rho_fn.vector[:] = rho
    with pytest.raises(RuntimeError, match="solve the state first"):
        ElasticityBuckling(res, 2).load_factors()                     # the supports reach the residual with the state solve
    import types
    real = res.mesh
    res.mesh = types.SimpleNamespace(local=types.SimpleNamespace(nranks=2))
    with pytest.raises(NotImplementedError, match="partitioned"):
        ElasticityBuckling(res, 2)
    res.mesh = real
    from femo_amd.fea.utils_hip import dirichletbc
    res.solve_state(u, [dirichletbc(0.01, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)])
    with pytest.raises(NotImplementedError, match="inhomogeneous"):
        ElasticityBuckling(res, 2).load_factors()


def test_tensile_load_fails(gpu):
    """The reversed load (+1, 0) on rect8x4 with n_modes = 3 in a block of 3: the block fills up with negative mu (buckling
    under the compressive load) and the call says that it is too small instead of returning them.  With a block of 8 and
    the compressive load the same object converges."""
    from femo_amd._lib import FemoError
    from femo_amd.fea.elasticity import ElasticityBuckling
    mesh = _mesh("rect8x4")
    res, u, rho, V, bcs = _setup(mesh, pc="jacobi", sign=+1.0)
    rho.vector[:] = _rho(mesh)
    res.solve_state(u, bcs)
    buck = ElasticityBuckling(res, 3, block=3)
    buck.max_outer = 40
    with pytest.raises(FemoError, match="too small.*no positive load factor"):
        buck.load_factors()
    print(f"rect8x4, tensile load, (3, 3): raised after {buck.max_outer} outer steps")
