"""GPU tests of the eigenfrequency path of the SIMP elasticity (csrc/elast_eig.hip, `DeviceElasticity.eigs`,
`ElasticityEigenvalues`, `EigenvalueAggregate`) against the restatement tests/elast_eig_ref.py and its dense eigh.

The meshes are those of tests/test_gpu_elast_body.py: less than one wave of rows (rect8x4), the two jittered ones, and two
with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343).  Clamped on x = 0,
rho = default_rng(7).uniform(0.3, 1), consistent P1 mass, start block default_rng(1).standard_normal((n_free, L)).

The outer iteration count of `eigs` is bounded by that of the restated iteration from the same start block with
`pcg_multi` at the same inner tolerance, plus 10 % and at least 2.  The stopping levels are comparable: the device's inner
PCG starts from the previous block and stops on r.M^-1 r relative to its first residual; the restatement runs `pcg_multi`
from zero on K D = B - K X, which has the same first residual and therefore the same stopping level, and both stop the
outer loop on the same residual |K phi - lambda M phi| <= rtol lambda |M phi|.  The inner tolerance 1e-12 lies three decades
below the eigen rtol 1e-9, so the outer count is that of exact solves (tests/test_elast_eig_host.py: equal on every case)
whatever the preconditioner is; the restatement therefore runs block-Jacobi, the cheaper one on the CPU, for both device
preconditioners.

MEASURED on the MI355X (SIMP and RAMP, all meshes and both preconditioners; the tests print every figure):
  eigenvalue error against the dense eigh   5.2e-13 at the most (rect24x12; 4e-14 or better on the other meshes); bound 1e-8
  outer steps, device / restatement         equal on all 42 cases: 6 ... 14 for (1, 3), 10 ... 19 for (3, 5), 26 ... 54 for (6, 8)
  inner PCG iterations per outer step       about 60 (multilevel) and 80 ... 110 (block-Jacobi, within 2 of the restatement's)
  reported residuals                        3e-11 ... 9.2e-10, bound 1e-9
  warm start after a change of 1e-3 in rho  10 -> 6 outer steps (rect8x4), 18 -> 9 (cube6j)
  dJ/drho against the dense eigenvectors    1.4e-12 at the most (the totals re-solve from converged modes); bound 1e-6
  directional central differences of J      9.0e-10 on rect24x12; bound 1e-5
  mass product 6.5e-16, Gram 4.8e-17 of |a_i| |b_j|, rotate exact, eig_drho 1.7e-15
"""
import functools

import numpy as np
import pytest

import elast_eig_ref as er
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BOTH_PC = ("rect8x4", "cube4j")              # one 2-D and one 3-D mesh run both preconditioners
RTOL, PCG_RTOL = 1e-9, 1e-12
DENSITY = 1.3


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
    """K, M (density 1), the nine lowest dense eigenpairs: built once, read only."""
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh)
    K = ref.stiffness(mesh.x, mesh.conn, rho, method)
    M = er.mass(mesh.x, mesh.conn, rho)
    lam, Phi = er.dense_eigs(K, M, mask, 9)
    return dict(mesh=mesh, mask=mask, rho=rho, K=K, M=M, lam=lam, Phi=Phi)


@functools.lru_cache(maxsize=None)
def restated_iteration(name, method, n_modes, block):
    """The restated iteration with `pcg_multi` (block-Jacobi) at the device's tolerances from the device's start block."""
    P = problem(name, method)
    A = pr.masked_operator(P["K"], P["mask"])
    Dinv = pr.invert_blocks(pr.block_diagonal(A, P["mesh"].tdim))
    d = P["mesh"].tdim
    jacobi = lambda r: np.einsum("nij,nj->ni", Dinv, r.reshape(-1, d)).ravel()
    out = er.block_inverse_iteration(P["K"], P["M"], P["mask"], er.start_block(P["mask"], block), n_modes,
                                     er.pcg_solver(A, jacobi, P["mask"], PCG_RTOL), rtol=RTOL)
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
@pytest.mark.parametrize("law", er.MASS_LAWS)
@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("name", MESHES)
def test_mass_apply(gpu, name, L, law):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    rho = _rho(mesh, 0.02)                                            # cells on both branches of du_olhoff
    dev, rv = _device(gpu, mesh, rho=rho)
    n, a, rho0 = dev.n_dof, -1.5, 2.5
    mask = clamped_face(mesh)
    M = er.mass(mesh.x, mesh.conn, rho, law, rho0)
    rng = np.random.default_rng(12)
    X, Z = rng.standard_normal((L, n)), rng.standard_normal((L, n))
    xv, zv, yv, y1, x1 = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n).set(Z.ravel()), Vec(gpu, L * n), Vec(gpu, n), Vec(gpu, n)
    kw = dict(a=a, density=rho0, mass_law=law)
    Y = _columns(dev.mass_apply_multi(L, rv, xv, yv, **kw), L)
    want = a * (M @ X.T).T
    err = _maxrel(Y, want)
    print(f"{name} L={L} {law}: M x against the restatement {err:.1e}")
    assert err <= 1e-13                                               # sums over the at most ~30 cells around a vertex
    assert np.array_equal(_columns(dev.mass_apply_multi(L, rv, xv, yv, **kw), L), Y)       # the same bits again
    for l in range(L):                                                # independent of L
        assert np.array_equal(np.array(dev.mass_apply_multi(1, rv, x1.set(X[l]), y1, **kw).get()), Y[l])
    # symmetric: x . M z = z . M x
    MZ = _columns(dev.mass_apply_multi(L, rv, zv, yv, **kw), L)
    for l in range(L):
        assert abs(X[l] @ MZ[l] - Z[l] @ Y[l]) <= 1e-13 * np.linalg.norm(X[l]) * np.linalg.norm(MZ[l])
    # masked: M_ff -- exact zeros on the fixed dofs, fixed entries of x ignored
    Ym = _columns(dev.mass_apply_multi(L, rv, xv, yv, masked=True, **kw), L)
    wantm = a * (er.masked(M, mask) @ X.T).T
    assert np.all(Ym[:, mask == 1] == 0.0)
    assert _maxrel(Ym, wantm) <= 1e-13
    X0 = np.where(mask[None, :] == 1, 0.0, X)
    assert np.array_equal(_columns(dev.mass_apply_multi(L, rv, Vec(gpu, L * n).set(X0.ravel()), yv, masked=True, **kw), L), Ym)


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 5), (8, 8)])
@pytest.mark.parametrize("name", MESHES)
def test_block_gram(gpu, name, na, nb):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    dev, _ = _device(gpu, mesh, fixed=False)
    n = dev.n_dof
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((na, n)), rng.standard_normal((nb, n))
    av, bv = Vec(gpu, na * n).set(A.ravel()), Vec(gpu, nb * n).set(B.ravel())
    G = dev.block_gram(na, av, nb, bv)
    scale = np.outer(np.linalg.norm(A, axis=1), np.linalg.norm(B, axis=1))
    err = (np.abs(G - A @ B.T) / scale).max()
    print(f"{name} ({na}, {nb}): Gram against A B^T {err:.1e} of |a_i| |b_j|")
    assert G.shape == (na, nb) and err <= 1e-13
    assert np.array_equal(dev.block_gram(na, av, nb, bv), G)           # the same bits again
    assert dev.block_gram(1, av, 1, bv)[0, 0] == G[0, 0]               # a pair does not depend on how many go with it


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("name", MESHES)
def test_block_rotate(gpu, name, L):
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    dev, _ = _device(gpu, mesh, fixed=False)
    n = dev.n_dof
    rng = np.random.default_rng(4)
    X, Q = rng.standard_normal((L, n)), rng.standard_normal((L, L))
    xv, yv = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n)
    Y = _columns(dev.block_rotate(L, Q, xv, yv), L)
    err = _maxrel(Y, Q.T @ X)
    print(f"{name} L={L}: X Q {err:.1e}")
    assert err <= 1e-14
    assert np.array_equal(_columns(dev.block_rotate(L, Q, xv, xv), L), Y)      # in place: the same bits


@pytest.mark.parametrize("law", er.MASS_LAWS)
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_eig_drho(gpu, name, method, law):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    mesh = _mesh(name)
    rho = _rho(mesh, 0.02)
    dev, rv = _device(gpu, mesh, rho=rho, fixed=False)
    n, nc, L = dev.n_dof, mesh.n_cell, 3
    rng = np.random.default_rng(5)
    Phi, lam, c, base = rng.standard_normal((L, n)), rng.uniform(0.5, 2.0, L), rng.standard_normal(L), rng.standard_normal(nc)
    pv, yv = Vec(gpu, L * n).set(Phi.ravel()), Vec(gpu, nc)
    want = er.eig_drho(mesh.x, mesh.conn, rho, Phi.T, lam, c, method, law, DENSITY)
    kw = dict(density=DENSITY, mass_law=law)
    g = np.array(dev.eig_drho(METHODS[method], L, rv, pv, lam, c, yv, **kw).get())
    err = _maxrel(g, want)
    ga = np.array(dev.eig_drho(METHODS[method], L, rv, pv, lam, c, yv.set(base), accumulate=True, **kw).get())
    erra = _maxrel(ga, base + want)
    print(f"{name} {method} {law}: eig_drho {err:.1e}, accumulated {erra:.1e}")
    assert err <= 1e-12 and erra <= 1e-12
    # the stiffness part alone (no mass: density 0) is dR/drho^T with x_k = c_k phi_k
    gk = np.array(dev.eig_drho(METHODS[method], L, rv, pv, lam, c, yv, density=0.0, mass_law=law).get())
    cp = Vec(gpu, L * n).set((c[:, None] * Phi).ravel())
    gd = np.array(dev.drho_multi(METHODS[method], True, L, rv, pv, cp, Vec(gpu, nc)).get())
    assert _maxrel(gk, gd) <= 1e-12


# -------------------------------------------------------------------------------------------------------- the solve ----
def _eigs_cases():
    for name in MESHES:
        for pc in (("jacobi", "multilevel") if name in BOTH_PC else ("multilevel",)):
            yield name, pc


@pytest.mark.parametrize("n_modes,block", [(1, 3), (3, 5), (6, 8)])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name,pc", list(_eigs_cases()))
def test_eigs(gpu, name, pc, method, n_modes, block):
    from femo_amd.engine import Vec
    P = problem(name, method)
    mesh, mask = P["mesh"], P["mask"]
    dev, rv = _device(gpu, mesh, method, P["rho"])
    if pc == "multilevel":
        dev.pc_setup()
    n = dev.n_dof
    xv = Vec(gpu, block * n).set(er.start_block(mask, block).ravel())
    lam, info = dev.eigs(n_modes, rv, xv, block=block, rtol=RTOL, pcg_rtol=PCG_RTOL, pc=pc)
    R = restated_iteration(name, method, n_modes, block)
    err = (np.abs(lam[:n_modes] - P["lam"][:n_modes]) / P["lam"][:n_modes]).max()
    print(f"{name} {pc} {method} ({n_modes}, {block}): eigenvalue error {err:.1e}, outer steps {info['outer_iterations']} "
          f"(restatement {R['outer']}), {info['pcg_iterations']} PCG iterations (restatement, block-Jacobi: {R['pcg']}), "
          f"residuals {info['residual'][:n_modes].max():.1e}")
    assert info["converged"] == 1
    assert err <= 1e-8                                                # ten times the residual level
    assert np.all(np.diff(lam) >= 0.0)
    Phi = _columns(xv, block)
    assert np.all(Phi[:, mask == 1] == 0.0)
    assert np.all(Phi[np.arange(block), np.argmax(np.abs(Phi), axis=1)] > 0.0)
    mv, kv = Vec(gpu, block * n), Vec(gpu, block * n)
    dev.mass_apply_multi(block, rv, xv, mv, masked=True)
    dev.apply_multi(block, xv, kv, masked=True)
    G = dev.block_gram(block, xv, block, mv)
    assert np.abs(G - np.eye(block)).max() <= 1e-10
    MP, KP = _columns(mv, block), _columns(kv, block)
    res = np.linalg.norm(KP - lam[:, None] * MP, axis=1) / (lam * np.linalg.norm(MP, axis=1))
    assert np.all(info["residual"][:n_modes] <= RTOL)
    for k in range(n_modes):
        assert 0.5 * res[k] <= info["residual"][k] <= 2.0 * res[k] or max(res[k], info["residual"][k]) <= 1e-13, (k, res, info)
    assert info["outer_iterations"] <= R["outer"] + max(2.0, 0.1 * R["outer"])


def _eigen(mesh, method="SIMP", n_modes=3, pc="multilevel", **kw):
    from femo_amd.fea.elasticity import ElasticityEigenvalues
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    V = VectorFunctionSpace(mesh)
    rho = Function(FunctionSpace(mesh, ("DG", 0)))
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    return ElasticityEigenvalues(rho, V, bcs, n_modes, method=method, preconditioner=pc, **kw), rho, V, bcs


@pytest.mark.parametrize("name", ["rect8x4", "cube6j"])
def test_warm_start(gpu, name):
    """A second solve after a change of 1e-3 in the density starts from the modes of the first; an unchanged density does
    not solve at all; a static residual on the same mesh keeps its own K."""
    from femo_amd.fea.utils_hip import LAST_KSP_INFO
    P = problem(name, "SIMP")
    mesh = P["mesh"]
    eig, rho, V, bcs = _eigen(mesh)
    rho.vector[:] = P["rho"]
    n0 = len(LAST_KSP_INFO)
    lam = eig.eigenvalues()
    cold = eig.last_info["outer_iterations"]
    assert LAST_KSP_INFO[-1]["kind"] == "elasticity_eigs" and len(LAST_KSP_INFO) == n0 + 1
    assert (np.abs(lam - P["lam"][:3]) / P["lam"][:3]).max() <= 1e-8
    assert np.array_equal(eig.eigenvalues(), lam) and len(LAST_KSP_INFO) == n0 + 1     # cached
    rho2 = P["rho"] * (1.0 + 1e-3 * np.random.default_rng(2).uniform(-1.0, 1.0, mesh.n_cell))
    rho.vector[:] = rho2
    lam2 = eig.eigenvalues()
    warm = eig.last_info["outer_iterations"]
    K2, M2 = ref.stiffness(mesh.x, mesh.conn, rho2, "SIMP"), er.mass(mesh.x, mesh.conn, rho2)
    want = er.dense_eigs(K2, M2, P["mask"], 3)[0]
    print(f"{name}: {cold} outer steps cold, {warm} warm")
    assert (np.abs(lam2 - want) / want).max() <= 1e-8
    assert warm < cold


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_form(gpu, name, method):
    """`EigenvalueAggregate` registered through FEA.add_output: J and dJ/drho through OutputOperation against the restatement's
    dense eigenpairs.  n_modes = 3 keeps the near-pair of the cubes inside; the gap to lambda_4 is at least 2.1."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import FEA, Function, FunctionSpace, VectorFunctionSpace, dirichletbc, eigenvalue_aggregate
    P = problem(name, method)
    mesh, mask = P["mesh"], P["mask"]
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn = Function(Q)
    bcs = [dirichletbc(0.0, np.nonzero(mask)[0].astype(np.int32), V)]
    form = eigenvalue_aggregate(rho_fn, V, bcs, n_modes=3, p=8.0, method=method, density=DENSITY, preconditioner="multilevel")
    fea.add_input('density', rho_fn)
    fea.add_output(name='eigenvalue', type='scalar', form=form, arguments=['density'])
    model = FEAModel(fea=[fea])
    model.create_input('density', shape=mesh.n_cell, val=P["rho"])
    model.add_design_variable('density', upper=1.0, lower=1e-4)
    model.add_objective('eigenvalue')
    sim = Simulator(model)
    sim.run()
    J, g, lam = er.aggregate_gradient(mesh.x, mesh.conn, P["rho"], mask, 3, 8.0, method, "linear", DENSITY)
    errJ = abs(float(sim['eigenvalue'][0]) - J) / J
    gd = np.asarray(sim.compute_totals('eigenvalue', 'density')).ravel()
    errg = _maxrel(gd, g)
    print(f"{name} {method}: J {errJ:.1e}, dJ/drho {errg:.1e} ({form.eigen.last_info['outer_iterations']} outer steps)")
    assert errJ <= 1e-8
    assert errg <= 1e-6                                               # eigenvector error of the order rtol / gap


def test_directional_derivative(gpu):
    """Central differences of the device's own J along one direction on rect24x12, step 1e-5, 1e-5 relative.  The direction
    has positive entries (a change of the overall density), so that the derivative is of the size of J itself and the
    rounding of J, about 1e-11 relative through the Rayleigh-Ritz Gram matrices, stays below the bound after the division."""
    from femo_amd.fea.elasticity import EigenvalueAggregate
    P = problem("rect24x12", "SIMP")
    mesh = P["mesh"]
    eig, rho, _, _ = _eigen(mesh, density=DENSITY)
    form = EigenvalueAggregate(eig, p=8.0)
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    rho.vector[:] = P["rho"]
    g = np.array(form.assemble_derivative(rho).get())
    h = 1e-5
    rho.vector[:] = P["rho"] + h * d
    Jp = form.assemble_scalar()
    rho.vector[:] = P["rho"] - h * d
    Jm = form.assemble_scalar()
    fd, an = (Jp - Jm) / (2 * h), float(g @ d)
    print(f"rect24x12: directional derivative {an:.9e}, central differences {fd:.9e}, {abs(fd - an) / abs(an):.1e}")
    assert abs(fd - an) <= 1e-5 * abs(an)


# ------------------------------------------------------------------------------------------------ limits and errors ----
def test_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, ElasticityEigenvalues, eigenvalue_aggregate
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.utils_hip import dirichletbc
    mesh = _mesh("rect8x4")
    rho = _rho(mesh)
    dev, rv = _device(gpu, mesh, rho=rho, fixed=False)
    n, nc = dev.n_dof, mesh.n_cell
    big, y, cells = Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(1.0), Vec(gpu, (ELAST_MAX_COLS + 1) * n), Vec(gpu, nc)
    lam = np.ones(ELAST_MAX_COLS + 1)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.mass_apply_multi(bad, rv, big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.block_gram(bad, big, 1, big)
        with pytest.raises(FemoError, match="columns"):
            dev.block_gram(1, big, bad, big)
        with pytest.raises(FemoError, match="columns"):
            dev.block_rotate(bad, np.eye(bad), big, y)
        with pytest.raises(FemoError, match="columns"):
            dev.eig_drho(METHODS["SIMP"], bad, rv, big, lam[:bad], lam[:bad], cells)
        with pytest.raises(FemoError, match="columns"):
            dev.eigs(1, rv, big, block=bad)
    with pytest.raises(FemoError):
        dev.mass_apply_multi(3, rv, Vec(gpu, 3 * n - 1), y)
    with pytest.raises(FemoError, match="aliases"):
        dev.mass_apply_multi(2, rv, y, y)
    with pytest.raises(FemoError, match="mass law"):
        dev.mass_apply_multi(2, rv, big, y, mass_law="lumped")
    with pytest.raises(FemoError, match="mass law"):
        dev.eig_drho(METHODS["SIMP"], 2, rv, big, lam[:2], lam[:2], cells, mass_law="lumped")
    with pytest.raises(FemoError, match="fixed set"):
        dev.mass_apply_multi(2, rv, big, y, masked=True)
    with pytest.raises(FemoError):
        dev.block_rotate(3, np.eye(2), big, y)
    with pytest.raises(FemoError):
        dev.eig_drho(METHODS["SIMP"], 3, rv, big, lam[:2], lam[:3], cells)
    with pytest.raises(FemoError, match="assemble"):
        dev.eigs(1, rv, big, block=3)                                 # no K yet
    dev.assemble(METHODS["SIMP"], rv)
    with pytest.raises(FemoError, match="fixed set"):
        dev.eigs(1, rv, big, block=3)                                 # K is singular without supports
    dev.set_fixed(clamped_face(mesh))
    dev.assemble(METHODS["SIMP"], rv)
    with pytest.raises(FemoError, match="modes"):
        dev.eigs(4, rv, big, block=3)
    with pytest.raises(FemoError, match="mass law"):
        dev.eigs(1, rv, big, block=3, mass_law="lumped")
    with pytest.raises(ValueError):
        dev.eigs(1, rv, big, block=3, pc="ilu")
    with pytest.raises(FemoError, match="multilevel"):
        dev.eigs(1, rv, big, block=3, pc="multilevel")                # no pc_setup
    # the forms
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    rho_fn = Function(Q)
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    with pytest.raises(NotImplementedError):
        ElasticityEigenvalues(rho_fn, LoadCaseSpace(V, 2), bcs, 3)
    with pytest.raises(NotImplementedError, match="free-free"):
        ElasticityEigenvalues(rho_fn, V, [], 3)
    with pytest.raises(NotImplementedError):
        ElasticityEigenvalues(Function(V), V, bcs, 3)                 # the density is DG0
    with pytest.raises(ValueError):
        ElasticityEigenvalues(rho_fn, V, bcs, 4, block=3)
    with pytest.raises(ValueError):
        ElasticityEigenvalues(rho_fn, V, bcs, 3, mass_law="lumped")
    with pytest.raises(ValueError):
        eigenvalue_aggregate(rho_fn, V, bcs, n_modes=3, p=0.5)
    import types
    part = types.SimpleNamespace(local=types.SimpleNamespace(nranks=2))
    Vp = VectorFunctionSpace(mesh)
    Vp.mesh = part
    with pytest.raises(NotImplementedError, match="partitioned"):
        ElasticityEigenvalues(rho_fn, Vp, bcs, 3)
