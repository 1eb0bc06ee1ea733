"""GPU tests of the elastic supports and displacement outputs of the SIMP elasticity (femo_elast_set_springs: k_elast_springs in
csrc/elasticity.hip, k_pc_springs in csrc/elast_pc.hip; femo_elast_pnorm_disp_multi: csrc/elast_disp.hip; ``springs`` of the
static residuals, `displacement`, `pnorm_displacement`) against the restatement tests/elast_support_ref.py.

The meshes are those of tests/test_gpu_elast_body.py: less than one wave of rows (rect8x4), the two jittered ones, and two
with more than one block of 256 rows (rect24x12: 325 vertices, cube6j: 343), so that the partial fold and the tail block of
the vertex kernels are live.  Tolerances are those of tests/test_gpu_elast_body.py, tests/test_gpu_elast_pc.py and
tests/test_gpu_topopt.py."""
import functools

import numpy as np
import pytest

import elast_pc_ref as pr
import elast_support_ref as sr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

pytestmark = pytest.mark.gpu

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
WEIGHTS = (1.0, 0.5, 2.0)
RTOL = 1e-13                # of the counted solves, as tests/test_gpu_elast_body.py argues
PATH_CASE = "rect52x26"     # of pr.path_meshes(): its finest level (561 nodes) is built by the global-atomic k_pc_blocks


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
    if name == PATH_CASE:
        return pr.path_meshes()[name][0]()
    return pr.small_meshes()[name]()


def _spacing(name):
    return pr.path_meshes()[name][1] if name == PATH_CASE else 0.0


def _columns(v, L):
    return np.array(v.get()).reshape(L, -1)


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _device(gpu, mesh, method, rho, mask=None, k=None):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    if mask is not None:
        dev.set_fixed(mask)
    if k is not None:
        dev.set_springs(k)
    rv = Vec(gpu, mesh.n_cell).set(rho)
    dev.assemble(METHODS[method], rv)
    return dev, rv


def _random_springs(mesh, mask, seed=5):
    """Springs on about a fifth of the dofs, some of them on clamped dofs."""
    rng = np.random.default_rng(seed)
    n = mesh.tdim * mesh.n_vert
    k = np.where(rng.random(n) < 0.2, rng.uniform(0.1, 10.0, n), 0.0)
    fixed = np.nonzero(mask)[0]
    k[fixed[::3]] = rng.uniform(0.1, 10.0, len(fixed[::3]))
    return k


# ------------------------------------------------------------------------------------------------------- 1. operator ----
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_operator(gpu, name, method):
    from femo_amd._lib import FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    mesh = _mesh(name)
    n = mesh.tdim * mesh.n_vert
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    k = _random_springs(mesh, mask)
    assert np.any(k[mask == 1] > 0.0) and 0.1 < np.count_nonzero(k) / n < 0.4
    dev, rv = _device(gpu, mesh, method, rho, mask)
    plain = dev.export_csr()
    dev.set_springs(k)
    x1, y1 = Vec(gpu, n).fill(1.0), Vec(gpu, n)
    with pytest.raises(FemoError, match="assemble"):                  # not silently stale
        dev.apply_multi(1, x1, y1)
    with pytest.raises(FemoError, match="assemble"):
        dev.solve(x1, y1)
    dev.assemble(METHODS[method], rv)
    Ks = dev.export_csr()
    want = sr.sprung_stiffness(mesh.x, mesh.conn, rho, k, method)
    scale = np.abs(ref.stiffness(mesh.x, mesh.conn, rho, method)).max()
    err = np.abs(Ks - want).max() / scale
    print(f"{name} {method}: K + diag(k) against the restatement {err:.1e}")
    assert err <= 1e-12
    assert np.array_equal(Ks.indptr, plain.indptr) and np.array_equal(Ks.indices, plain.indices)       # the same pattern
    assert np.abs(Ks - Ks.T).max() == 0.0                                                              # entry for entry
    assert np.abs((Ks - plain).diagonal() - k).max() <= 1e-12 * scale
    A = pr.masked_operator(want, mask)
    rng = np.random.default_rng(3)
    for L in (1, 3, 5):
        X = rng.standard_normal((L, n))
        xv, yv = Vec(gpu, L * n).set(X.ravel()), Vec(gpu, L * n)
        for masked, op in ((False, want), (True, A)):
            Y = _columns(dev.apply_multi(L, xv, yv, masked=masked), L)
            wantY = (op @ X.T).T
            e = np.abs(Y - wantY).max() / np.abs(wantY).max()
            print(f"{name} {method} L={L} masked={masked}: product {e:.1e}")
            assert e <= 1e-12
    # without springs again: bit for bit the operator of a handle that never had any (None and all zeros both clear)
    fresh, _ = _device(gpu, mesh, method, rho, mask)
    F = fresh.export_csr()
    for clear in (None, np.zeros(n)):
        dev.set_springs(k)
        dev.set_springs(clear)
        assert dev.springs_key is None
        dev.assemble(METHODS[method], rv)
        back = dev.export_csr()
        assert np.array_equal(back.data, F.data) and np.array_equal(back.indices, F.indices)
        Y0 = np.array(dev.apply_multi(1, x1, y1, masked=True).get())
        assert np.array_equal(Y0, np.array(fresh.apply_multi(1, x1, Vec(gpu, n), masked=True).get()))


# --------------------------------------------------------------------------- 2. a known answer without a Dirichlet set ----
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("name", ["rect8x4", "rect24x12", "cube4j", "cube6j"])
def test_rigid_motion_on_springs_alone(gpu, name, pc):
    """K r = 0 for a rigid motion r and any density, so (K + diag(k)) u = diag(k) r has the solution u = r."""
    from femo_amd.engine import Vec
    mesh = _mesh(name)
    n = mesh.tdim * mesh.n_vert
    rng = np.random.default_rng(11)
    rho = rng.uniform(0.05, 1.0, mesh.n_cell)
    k = rng.uniform(0.5, 2.0, n)
    modes = ref.rigid_body_modes(mesh.x)
    r = modes @ rng.standard_normal(modes.shape[1])
    dev, _ = _device(gpu, mesh, "SIMP", rho, None, k)
    if pc == "multilevel":
        dev.pc_setup()
    x = Vec(gpu, n)
    info = dev.solve(Vec(gpu, n).set(k * r), x, rtol=RTOL, pc=pc)
    err = np.abs(np.array(x.get()) - r).max() / np.abs(r).max()
    print(f"{name} {pc}: {info.iterations} iterations, u against the rigid motion {err:.1e}")
    assert info.converged == 1
    assert err <= 1e-9


# ------------------------------------------------------------------------------------- 3. lattice blocks, 4. counts ----
PC_CASES = ["rect8x4", "rect24x12", "cube6j", PATH_CASE]


@functools.lru_cache(maxsize=None)
def sprung_case(name):
    """A clamp at x = 0 and springs k = 10 on the y dofs of the bottom edge (2-D) or face (3-D), the corner vertices both
    sprung and clamped; the restated preconditioner on K + diag(k), a right-hand side, its direct solve and the restated
    PCG counts.  Built once, read only."""
    mesh = _mesh(name)
    d = mesh.tdim
    n = d * mesh.n_vert
    rho = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    bottom = np.nonzero(np.isclose(mesh.x[:, 1], mesh.x[:, 1].min()))[0]
    k = np.zeros(n)
    k[d * bottom + 1] = 10.0
    assert np.any((k > 0.0) & (mask == 1))
    M = sr.multilevel(mesh.x, mesh.conn, rho, k, "SIMP", mask, spacing_factor=_spacing(name))
    b = np.where(mask == 1, 0.0, np.random.default_rng(2).standard_normal(n))
    Ks = sr.sprung_stiffness(mesh.x, mesh.conn, rho, k)
    u = ref.solve_fixed(Ks, b, np.nonzero(mask)[0])
    counts = {}
    for pc in ("jacobi", "multilevel"):
        _, it, ok = pr.pcg(M.A, b, M.jacobi if pc == "jacobi" else M.apply, mask, rtol=RTOL)
        assert ok
        counts[pc] = it
    return dict(mesh=mesh, rho=rho, mask=mask, k=k, M=M, b=b, u=u, counts=counts)


@pytest.mark.parametrize("name", PC_CASES)
def test_lattice_blocks(gpu, name):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    R = sprung_case(name)
    mesh, M = R["mesh"], R["M"]
    if name == PATH_CASE:
        assert pr.path_levels(M.plan["nodes"], mesh.tdim)[0] == [M.plan["n_levels"] - 1]        # the atomic path, finest level
    dev, rv = _device(gpu, mesh, "SIMP", R["rho"], R["mask"], R["k"])
    info = dev.pc_setup(_spacing(name))
    assert info["levels"] == M.plan["n_levels"] and info["nodes"] == M.plan["nodes"]
    plain = pr.Multilevel(mesh.x, mesh.conn, R["rho"], "SIMP", R["mask"], spacing_factor=_spacing(name))
    for l in range(info["levels"]):
        B = dev.pc_level(l)
        err = np.abs(B - M.G[l]).max() / np.abs(M.G[l]).max()
        missing = np.abs(plain.G[l] - M.G[l]).max() / np.abs(M.G[l]).max()
        print(f"{name} level {l}: {info['nodes'][l]} nodes, block error {err:.2e} (the springs are {missing:.1e} of the level)")
        assert err <= 1e-12
        assert np.array_equal(B, np.transpose(B, (0, 2, 1)))
        assert missing > 1e-3                                          # the comparison sees them
    assert dev.pc_info()["builds"] == 1
    # new springs after a build: the plan is dirty, and the next solve rebuilds exactly once
    n = dev.n_dof
    b, x = Vec(gpu, n).set(R["b"]), Vec(gpu, n)
    dev.set_springs(2.0 * R["k"])
    dev.assemble(METHODS["SIMP"], rv)
    assert dev.pc_info()["builds"] == 1
    assert dev.solve(b, x, rtol=RTOL, pc="multilevel").converged == 1
    assert dev.pc_info()["builds"] == 2
    last = info["levels"] - 1
    M2 = sr.multilevel(mesh.x, mesh.conn, R["rho"], 2.0 * R["k"], "SIMP", R["mask"], spacing_factor=_spacing(name))
    assert np.abs(dev.pc_level(last) - M2.G[last]).max() <= 1e-12 * np.abs(M2.G[last]).max()
    dev.solve(b, x, rtol=RTOL, pc="multilevel")
    assert dev.pc_info()["builds"] == 2                               # nothing changed: no rebuild


@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("name", PC_CASES)
def test_counts(gpu, name, pc):
    """With the springs in the operator but not in the lattice blocks the multilevel solve takes twice the restatement's
    iterations and more (restated with this right-hand side: 273 against a bound of 141.7 on rect24x12, 218 against 95.5 on
    cube6j)."""
    from femo_amd.engine import Vec
    R = sprung_case(name)
    mesh = R["mesh"]
    dev, _ = _device(gpu, mesh, "SIMP", R["rho"], R["mask"], R["k"])
    if pc == "multilevel":
        dev.pc_setup(_spacing(name))
    n = dev.n_dof
    x = Vec(gpu, n)
    info = dev.solve(Vec(gpu, n).set(R["b"]), x, rtol=RTOL, pc=pc)
    err = _maxrel(np.array(x.get()), R["u"])
    print(f"{name} {pc}: {info.iterations} iterations (restatement {R['counts'][pc]}), u {err:.1e}")
    assert info.converged == 1
    assert info.iterations <= 1.1 * R["counts"][pc] + 2
    assert err <= 1e-9


# --------------------------------------------------------------------------------------------- 5. aggregate kernel ----
def _regions(mesh):
    """name -> nodal weights: all vertices with their lumped cell volume, a vertex list, the facets of the face x = x_max."""
    from femo_amd.fea.mesh import locate_entities_boundary
    xmax = mesh.x[:, 0].max()
    facets = locate_entities_boundary(mesh, mesh.tdim - 1, lambda x: np.isclose(x[0], xmax))
    ones = np.zeros(mesh.n_vert)
    ones[np.random.default_rng(4).choice(mesh.n_vert, mesh.n_vert // 3, replace=False)] = 1.0
    ones[mesh.n_vert - 1] = 1.0                                       # the last thread of the tail block
    return dict(all=sr.lumped_cells(mesh.x, mesh.conn), vertices=ones, facets=sr.lumped_facets(mesh.x, facets))


@pytest.mark.parametrize("p", [1.0, 2.0, 8.0])
@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("name", ["rect8x4", "cube4j", "rect24x12", "cube6j"])
def test_aggregate(gpu, name, L, p):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh(name)
    d = mesh.tdim
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n = dev.n_dof
    rng = np.random.default_rng(9)
    U = rng.standard_normal((L, n))
    U[0].reshape(-1, d)[5] = 0.0                                      # a vertex at rest inside a moving column
    if L >= 3:
        U[2] = 0.0                                                    # a zero column
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5])[:L]                       # column 3: no weight
    m = np.array([1.0, 0.7, 2.0, 1.3, 0.4])[:L]
    uv = Vec(gpu, L * n).set(U.ravel())
    for rname, a in _regions(mesh).items():
        av = Vec(gpu, mesh.n_vert).set(a)
        want = [sr.pnorm_disp(U[l], a, m[l], p, d) for l in range(L)]
        wantJ, wantG = np.array([t[0] for t in want]), np.stack([w[l] * want[l][1] for l in range(L)])
        gv = Vec(gpu, L * n).fill(7.0)
        vals = dev.pnorm_disp_multi(L, uv, av, m, p, weights=w, grad_u=gv)
        G = _columns(gv, L)
        eJ, eG = np.abs(vals - wantJ).max() / np.abs(wantJ).max(), np.abs(G - wantG).max() / np.abs(wantG).max()
        print(f"{name} L={L} p={p} {rname}: values {eJ:.1e}, dJ/du {eG:.1e}")
        assert eJ <= 1e-12 and eG <= 1e-12
        assert np.all(G[0].reshape(-1, d)[5] == 0.0)
        if L >= 3:
            assert vals[2] == 0.0 and np.all(G[2] == 0.0)             # exact zeros, never a NaN
        if L == 5:
            assert vals[3] > 0.0 and np.all(G[3] == 0.0)              # written as zeros over the 7s
        # the same bits again, one output at a time, and alpha given
        g2 = Vec(gpu, L * n)
        assert np.array_equal(dev.pnorm_disp_multi(L, uv, av, m, p, weights=w, grad_u=g2), vals) and np.array_equal(_columns(g2, L), G)
        assert np.array_equal(dev.pnorm_disp_multi(L, uv, av, m, p, weights=w), vals)
        g2.fill(3.0)
        assert dev.pnorm_disp_multi(L, uv, av, m, p, weights=w, value=False, grad_u=g2) is None
        assert np.array_equal(_columns(g2, L), G)
        # (NumPy's pairwise sum and the library's sequential one may differ in the last bit of alpha)
        assert np.abs(dev.pnorm_disp_multi(L, uv, av, m, p, alpha=a.sum()) - vals).max() <= 1e-14 * np.abs(vals).max()
        assert np.abs(dev.pnorm_disp_multi(L, uv, av, m, p, alpha=2.0 * a.sum()) - 0.5 * wantJ).max() <= 1e-12 * np.abs(wantJ).max()
        # column l does not depend on the number of columns
        u1, g1 = Vec(gpu, n), Vec(gpu, n)
        for l in range(L):
            u1.set(U[l])
            v1 = dev.pnorm_disp_multi(1, u1, av, m[l], p, weights=w[l:l + 1], grad_u=g1)
            assert v1[0] == vals[l] and np.array_equal(np.array(g1.get()), G[l])
        # accumulate adds; a column without weight is left alone
        base = rng.standard_normal((L, n))
        g2.set(base.ravel())
        dev.pnorm_disp_multi(L, uv, av, m, p, weights=w, value=False, grad_u=g2, accumulate=True)
        Ga = _columns(g2, L)
        assert np.abs(Ga - (base + wantG)).max() <= 1e-12 * max(np.abs(wantG).max(), np.abs(base).max())
        if L == 5:
            assert np.array_equal(Ga[3], base[3])


def test_aggregate_limits(gpu):
    from femo_amd._lib import ELAST_MAX_COLS, FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh("rect8x4")
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n, nv = dev.n_dof, mesh.n_vert
    u, g, a = Vec(gpu, (ELAST_MAX_COLS + 1) * n).fill(1.0), Vec(gpu, (ELAST_MAX_COLS + 1) * n), Vec(gpu, nv).fill(1.0)
    for bad in (0, ELAST_MAX_COLS + 1):
        with pytest.raises(FemoError, match="columns"):
            dev.pnorm_disp_multi(bad, u, a, 1.0, 8.0)
    for p in (0.5, np.inf, np.nan):
        with pytest.raises(FemoError, match="p >= 1"):
            dev.pnorm_disp_multi(2, u, a, 1.0, p)
    for m in (0.0, -1.0, np.nan, [1.0, np.inf]):
        with pytest.raises(FemoError, match="m > 0"):
            dev.pnorm_disp_multi(2, u, a, m, 8.0)
    with pytest.raises(FemoError, match="weight"):
        dev.pnorm_disp_multi(2, u, a, 1.0, 8.0, weights=[1.0, -1.0])
    with pytest.raises(FemoError):
        dev.pnorm_disp_multi(2, u, a, [1.0], 8.0)                     # as many scales as columns
    for bad in (-1.0, np.nan, np.inf):
        ah = np.ones(nv)
        ah[nv // 2] = bad
        with pytest.raises(FemoError, match="weight of vertex"):
            dev.pnorm_disp_multi(2, u, Vec(gpu, nv).set(ah), 1.0, 8.0)
    with pytest.raises(FemoError, match="alpha"):
        dev.pnorm_disp_multi(2, u, Vec(gpu, nv).fill(0.0), 1.0, 8.0)  # an empty region
    with pytest.raises(FemoError):
        dev.pnorm_disp_multi(2, Vec(gpu, 2 * n - 1), a, 1.0, 8.0)
    with pytest.raises(FemoError):
        dev.pnorm_disp_multi(2, u, Vec(gpu, nv - 1), 1.0, 8.0)
    with pytest.raises(FemoError):
        dev.pnorm_disp_multi(2, u, a, 1.0, 8.0, grad_u=Vec(gpu, 2 * n - 1))
    with pytest.raises(FemoError, match="aliases"):
        dev.pnorm_disp_multi(2, u, a, 1.0, 8.0, grad_u=u)
    vals = dev.pnorm_disp_multi(ELAST_MAX_COLS, u, a, 1.0, 8.0, grad_u=g)        # and the call after the refusals works
    assert np.abs(vals - 2.0 ** 4).max() <= 1e-12 * 2.0 ** 4             # |u_v| = sqrt 2 everywhere


# --------------------------------------------------------------------------- 7. the cycle through the operator surface ----
def _inverter_simulator(device, pc, output, n_cases=1):
    """The inverter set-up of scripts/run_topopt.py on rect24x12 through FEAModel + GeneralFilterModel + Simulator, from a
    random design: the port displacement or the aggregate over the right edge as the objective."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import pdeRes
    from femo_amd.fea.fea_hip import (FEA, Function, FunctionSpace, LoadCaseSpace, Measure, VectorFunctionSpace, displacement,
                                      locate_dofs_geometrical, locate_entities_boundary, meshSize, meshtags, pdeRes_multiload,
                                      pnorm_displacement, point_springs, port_displacement)
    mesh = _mesh("rect24x12")
    c = sr.inverter_case(mesh.x)
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho = Function(Q)
    springs = point_springs(V, [c["dof_in"], c["dof_out"]], [0.1, 0.1])
    assert np.array_equal(springs, c["k"])
    aux = dict(case=c, n=V.dim)
    if n_cases == 1:
        u = Function(V)
        res = pdeRes(u, None, rho, None, preconditioner=pc, springs=springs, point_load=port_displacement(V, [c["dof_in"]]))
        aux["F"] = [c["F"]]
    else:
        # load case l: the traction t_l on the left edge above the clamp (the point load is for one load case)
        facets = locate_entities_boundary(mesh, 1, lambda x: np.logical_and(np.isclose(x[0], 0.0), x[1] > 0.45))
        ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 9, dtype=np.int32)))(9)
        ts = [(1.0, 0.0), (0.5, -0.5), (0.0, 1.0)]
        u = Function(LoadCaseSpace(V, n_cases))
        res = pdeRes_multiload(u, None, rho, ts, [ds] * n_cases, preconditioner=pc, springs=springs)
        aux["F"] = [ref.traction_load(mesh.x, facets, t) for t in ts]
    res.rtol = RTOL
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    if output == "port":
        J = displacement(u, port_displacement(V, [c["dof_out"]]), weights=None if n_cases == 1 else WEIGHTS)
    else:
        fea.consistent_bc_partials = True
        right = locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 2.0))
        dsr = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, right, np.full(len(right), 8, dtype=np.int32)))(8)
        J = pnorm_displacement(u, region=dsr, m=0.05, p=8.0)
        aux["a"] = sr.lumped_facets(mesh.x, right)
    fea.add_output(name="J", type="scalar", form=J, arguments=["displacements"])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.logical_and(np.isclose(x[0], 0.0), x[1] <= 0.1 + 1e-9)),
                            locate_dofs_geometrical(V.sub(1), lambda x: np.isclose(x[1], 1.0))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=0.05 + np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    model.add_design_variable("density_unfiltered", upper=1.0, lower=1e-3)
    model.add_objective("J")
    aux.update(res=res, form=J, W=ref.filter_matrix(mesh.centroids(), 2.0 * (h.max() + h.min()) / 2))
    return Simulator(model, device=device), mesh, aux


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
@pytest.mark.parametrize("output", ["port", "pnorm"])
def test_cycle(gpu, output, pc, device):
    """State to 1e-9, the output to 1e-9 and the total gradient to 1e-8 of the restatement's cycle; central differences of the
    host simulator to 1e-6 (`Simulator.check_totals`, as the cantilever cycles)."""
    sim, mesh, aux = _inverter_simulator(device, pc, output)
    sim.run()
    c = aux["case"]
    x0 = np.array(np.asarray(sim["density_unfiltered"]), dtype=np.float64)
    if output == "port":
        R = sr.reference_cycle(mesh.x, mesh.conn, aux["W"], x0, c["k"], c["F"], c["mask"], c["ell"])
    else:
        R = sr.pnorm_cycle(mesh.x, mesh.conn, aux["W"], x0, c["k"], c["F"], c["mask"], aux["a"], 0.05, 8.0)
    err_u = _maxrel(np.asarray(sim["displacements"]), R["u"])
    err_J = abs(float(np.asarray(sim["J"]).ravel()[0]) - R["J"]) / abs(R["J"])
    g = np.asarray(sim.compute_totals("J", "density_unfiltered"))
    err_g = _maxrel(g, R["grad"])
    info = aux["res"].last_info
    print(f"inverter 24x12 {output} {pc} device={device}: u {err_u:.1e}, J {err_J:.1e} (J = {R['J']:.6e}), total {err_g:.1e}; "
          f"state PCG {info['state']['iterations']} it, adjoint {info['adjoint']['iterations']} it")
    assert err_u <= 1e-9
    assert err_J <= 1e-9
    assert err_g <= 1e-8
    if output == "pnorm":
        est = aux["form"].max_estimate()[0]
        peak = np.linalg.norm(R["u"].reshape(-1, 2)[aux["a"] > 0], axis=1).max()
        assert 0.5 * peak <= est <= peak                              # the p-mean from below
    if not device:
        chk = sim.check_totals("J", "density_unfiltered", step=1e-4, n_dir=3, seed=0)
        print(f"central differences: {chk['rel_error']}")
        assert max(chk["rel_error"]) <= 1e-6, chk


@pytest.mark.parametrize("output", ["port", "pnorm"])
def test_cycle_multiload(gpu, output):
    """One MultiLoadElasticityResidual with springs, L = 3 and weights (1, 0.5, 2): one batched solve each way."""
    L = 3
    sim, mesh, aux = _inverter_simulator(True, "multilevel", output, n_cases=L)
    sim.run()
    c = aux["case"]
    x0 = np.array(np.asarray(sim["density_unfiltered"]), dtype=np.float64)
    w = WEIGHTS if output == "port" else (1.0,) * L
    J, grad, us = 0.0, 0.0, []
    for l in range(L):
        if output == "port":
            R = sr.reference_cycle(mesh.x, mesh.conn, aux["W"], x0, c["k"], aux["F"][l], c["mask"], c["ell"])
        else:
            R = sr.pnorm_cycle(mesh.x, mesh.conn, aux["W"], x0, c["k"], aux["F"][l], c["mask"], aux["a"], 0.05, 8.0)
        J, grad = J + w[l] * R["J"], grad + w[l] * R["grad"]
        us.append(R["u"])
    U = np.asarray(sim["displacements"]).reshape(L, aux["n"])
    err_u = max(_maxrel(U[l], us[l]) for l in range(L))
    err_J = abs(float(np.asarray(sim["J"]).ravel()[0]) - J) / abs(J)
    err_g = _maxrel(np.asarray(sim.compute_totals("J", "density_unfiltered")), grad)
    print(f"inverter 24x12, 3 load cases, {output}: u {err_u:.1e}, J {err_J:.1e}, total {err_g:.1e}")
    assert err_u <= 1e-9 and err_J <= 1e-9 and err_g <= 1e-8
    assert aux["res"].solve_counts == {"state": 1, "adjoint": 1}


def _sprung_residual(mesh, springs, pc="jacobi", sign=-1.0):
    """A residual on the clamped mesh under the unit end-face traction along x (compressive for sign = -1)."""
    from femo_amd.fea.elasticity import Constant, ElasticityResidual, Measure, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    from femo_amd.fea.utils_hip import dirichletbc
    d = mesh.tdim
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    u, rho = Function(V), Function(Q)
    xmax = mesh.x[:, 0].max()
    facets = locate_entities_boundary(mesh, d - 1, lambda x: np.isclose(x[0], xmax))
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 7, dtype=np.int32)))(7)
    t = np.zeros(d)
    t[0] = sign
    res = ElasticityResidual(u, rho, Constant(mesh, t), ds, preconditioner=pc, springs=springs)
    bcs = [dirichletbc(0.0, np.nonzero(clamped_face(mesh))[0].astype(np.int32), V)]
    return res, u, rho, bcs, ref.traction_load(mesh.x, facets, t)


def test_buckling_on_a_sprung_residual(gpu):
    """The load factors of a strut on a Winkler foundation, through the residual's own K_s: against SciPy's eigsh on
    (-K_G)_ff v = mu (K_s)_ff v, to the 1e-8 of tests/test_gpu_elast_buckle.py."""
    import scipy.sparse.linalg as spla

    import elast_buckle_ref as bk
    from femo_amd.fea.elasticity import ElasticityBuckling, Measure, facet_springs, meshtags
    from femo_amd.fea.function import VectorFunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    mesh = _mesh("rect8x4")
    bottom = locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0.0))
    dsb = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, bottom, np.full(len(bottom), 3, dtype=np.int32)))(3)
    k = facet_springs(VectorFunctionSpace(mesh), dsb, (0.0, 0.05))
    res, u, rho, bcs, F = _sprung_residual(mesh, k)
    rh = np.random.default_rng(7).uniform(0.3, 1.0, mesh.n_cell)
    rho.vector[:] = rh
    res.solve_state(u, bcs)
    mask = clamped_face(mesh)
    Ks = sr.sprung_stiffness(mesh.x, mesh.conn, rh, k)
    uh = ref.solve_fixed(Ks, F, np.nonzero(mask)[0])
    assert _maxrel(np.array(u.vec.get()), uh) <= 1e-9
    KG = bk.geometric_stiffness(mesh.x, mesh.conn, rh, uh)
    free = np.nonzero(mask == 0)[0]
    mu = spla.eigsh((-KG).tocsr()[free][:, free].tocsc(), k=2, M=Ks[free][:, free].tocsc(), which="LA", tol=1e-13)[0]
    want = np.sort(1.0 / mu[mu > 0.0])
    lam = ElasticityBuckling(res, 2, block=8).load_factors()
    plain = bk.dense_buckling(ref.stiffness(mesh.x, mesh.conn, rh), KG, mask, 2)["lam"]
    print(f"load factors {lam} (eigsh {want}; without the foundation about {plain})")
    assert len(want) == 2 and (np.abs(lam - want) / want).max() <= 1e-8
    assert abs(plain[0] - want[0]) / want[0] > 1e-4                   # the foundation is seen


# ------------------------------------------------------------------------------------------------ 8. handle sharing ----
@pytest.mark.parametrize("pc", ["jacobi", "multilevel"])
def test_handle_sharing(gpu, pc):
    """A sprung and a plain residual on the same mesh (the same handle), solved alternately twice: each its own operator."""
    mesh = _mesh("rect24x12")
    mask = clamped_face(mesh)
    bottom = np.nonzero(np.isclose(mesh.x[:, 1], 0.0))[0]
    k = np.zeros(2 * mesh.n_vert)
    k[2 * bottom + 1] = 10.0
    rh = np.random.default_rng(7).uniform(0.05, 1.0, mesh.n_cell)
    forms = [_sprung_residual(mesh, k, pc), _sprung_residual(mesh, None, pc)]
    assert forms[0][0].device() is forms[1][0].device()
    fixed = np.nonzero(mask)[0]
    want = [ref.solve_fixed(sr.sprung_stiffness(mesh.x, mesh.conn, rh, kk), forms[0][4], fixed) for kk in (k, 0.0 * k)]
    assert _maxrel(want[0], want[1]) > 1e-2
    for rnd in range(2):
        for (res, u, rho, bcs, _), w in zip(forms, want):
            rho.vector[:] = rh
            res.rtol = RTOL
            res.solve_state(u, bcs)
            err = _maxrel(np.array(u.vec.get()), w)
            print(f"{pc} round {rnd} springs={'yes' if res.springs is not None else 'no'}: u {err:.1e}, "
                  f"{res.last_info['state']['iterations']} it")
            assert err <= 1e-9
            assert (res.device().springs_key is None) == (res.springs is None)
            # the residual at a state that is not the solution carries the owner's operator as well
            u.vector[:] = 1.0
            r = np.array(res.assemble_vector().get())
            Kw = sr.sprung_stiffness(mesh.x, mesh.conn, rh, k if res.springs is not None else 0.0 * k)
            wr = Kw @ np.ones(Kw.shape[0]) - forms[0][4]
            assert np.abs(r - wr).max() <= 1e-12 * np.abs(wr).max()


def test_constructor_arguments(gpu):
    """The new constructor arguments and their checks (Functions live on the device)."""
    from femo_amd.fea.elasticity import (ElasticityDisplacement, ElasticityPnormDisplacement, ElasticityResidual, Measure,
                                         MultiLoadElasticityResidual, displacement, meshtags, pdeRes, pdeRes_multiload,
                                         pnorm_displacement, point_springs, port_displacement)
    from femo_amd.fea.function import Function, FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    mesh = _mesh("rect8x4")
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    n = V.dim
    k = point_springs(V, [3, 10], [3.0, 0.75])
    ell = port_displacement(V, [4, 7], [1.0, -1.0])
    facets = locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 2.0))
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 5, dtype=np.int32)))(5)
    u, rho = Function(V), Function(Q)
    res = pdeRes(u, None, rho, (0.0, -1.0), dss=ds, springs=k)
    assert isinstance(res, ElasticityResidual) and np.array_equal(res.springs, k) and res.springs is not k
    assert pdeRes(u, None, rho, (0.0, -1.0), dss=ds).springs is None
    assert pdeRes(u, None, rho, (0.0, -1.0), dss=ds, springs=np.zeros(n)).springs is None          # all zeros: none
    pl = pdeRes(u, None, rho, None, springs=k, point_load=ell)          # a port force in the place of the traction
    assert np.array_equal(pl.point_load, ell) and np.array_equal(np.array(pl.load().get()), ell)
    both = pdeRes(u, None, rho, (0.0, -1.0), dss=ds, point_load=ell)
    assert np.abs(np.array(both.load().get()) - (ref.traction_load(mesh.x, facets, (0.0, -1.0)) + ell)).max() <= 1e-15
    with pytest.raises(ValueError):
        pdeRes(u, None, rho, None, springs=k)                           # no load at all
    for bad in (np.zeros(n - 1), -k, np.full(n, np.nan)):
        with pytest.raises(ValueError):
            pdeRes(u, None, rho, (0.0, -1.0), dss=ds, springs=bad)
    with pytest.raises(ValueError):
        pdeRes(u, None, rho, None, point_load=np.zeros(n + 1))
    um = Function(LoadCaseSpace(V, 3))
    rm = pdeRes_multiload(um, None, rho, [(0.0, -1.0)] * 3, [ds] * 3, springs=k)
    assert isinstance(rm, MultiLoadElasticityResidual) and np.array_equal(rm.springs, k)
    with pytest.raises(ValueError):
        pdeRes_multiload(um, None, rho, [(0.0, -1.0)] * 3, [ds] * 3, springs=np.zeros(3 * n))      # the base space's numbering
    J = displacement(u, ell)
    assert isinstance(J, ElasticityDisplacement) and J.functions() == (u,) and J.n_cases == 1
    uh = np.random.default_rng(1).standard_normal(n)
    u.vector[:] = uh
    assert abs(J.assemble_scalar() - ell @ uh) <= 1e-14 * np.abs(uh).max() and np.array_equal(np.array(J.assemble_derivative(u).get()), ell)
    Jm = displacement(um, ell, weights=(1.0, 0.5, 2.0))
    assert Jm.ell.shape == (3, n) and np.array_equal(Jm.weights, [1.0, 0.5, 2.0])
    assert np.array_equal(np.array(Jm.assemble_derivative(um).get()).reshape(3, n), np.outer([1.0, 0.5, 2.0], ell))
    for bad in (dict(ell=np.zeros(n + 1)), dict(ell=np.zeros((2, n))), dict(ell=np.full(n, np.nan)), dict(ell=ell, weights=(1.0, 2.0))):
        with pytest.raises(ValueError):
            displacement(um, **bad)
    A = pnorm_displacement(u, region=[1, 2, 2, 5])
    assert isinstance(A, ElasticityPnormDisplacement) and A.alpha == 3.0 and np.count_nonzero(A.a) == 3
    Ad = pnorm_displacement(um, region=ds, m=(1.0, 2.0, 3.0), p=2.0)
    assert abs(Ad.alpha - 1.0) <= 1e-15 and np.abs(Ad.a - sr.lumped_facets(mesh.x, facets)).max() <= 1e-15 and Ad.n_cases == 3
    Aall = pnorm_displacement(u)
    assert abs(Aall.alpha - 2.0) <= 1e-14 and np.abs(Aall.a - sr.lumped_cells(mesh.x, mesh.conn)).max() <= 1e-15
    want = sr.pnorm_disp(uh, A.a, 1.0, 8.0, 2)
    assert abs(A.assemble_scalar() - want[0]) <= 1e-12 * want[0]
    assert np.abs(np.array(A.assemble_derivative(u).get()) - want[1]).max() <= 1e-12 * np.abs(want[1]).max()
    assert abs(A.max_estimate()[0] - want[0] ** 0.125) <= 1e-12 * want[0] ** 0.125
    for bad in (dict(region=[]), dict(region=[mesh.n_vert]), dict(p=0.5), dict(m=0.0), dict(m=(1.0, 2.0)), dict(weights=-1.0),
                dict(p=np.inf)):
        with pytest.raises(ValueError):
            pnorm_displacement(u, **bad)
