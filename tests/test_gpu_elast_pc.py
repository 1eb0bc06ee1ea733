"""GPU tests of the multilevel preconditioner of the SIMP elasticity solves (csrc/elast_pc.hip) against the restatement
(tests/elast_pc_ref.py): the Galerkin blocks, one application, the 80 x 40 cantilever through FEAModel + GeneralFilterModel +
Simulator, iteration counts on fixed densities, the lazy rebuild, and (slow) the full-size meshes."""
import numpy as np
import pytest

import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import L_X, L_Y, clamped_face, count_case
from elast_pc_ref import small_meshes as _meshes

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _device(gpu, mesh, rho, method, mask, setup=True):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    dev.set_fixed(mask)
    rv = Vec(gpu, mesh.n_cell).set(rho)
    dev.assemble(METHODS[method], rv)
    if setup:
        dev.pc_setup()
    return dev, rv


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
def test_blocks(gpu, name, method):
    mesh = _meshes()[name]()
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    dev, _ = _device(gpu, mesh, rho, method, mask)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, method, mask)
    info = dev.pc_info()
    assert info["levels"] == M.plan["n_levels"] and info["nodes"] == M.plan["nodes"]
    assert info["bytes"] == sum(M.plan["nodes"]) * 8 * (2 * mesh.tdim ** 2 + 2 * mesh.tdim)
    for l in range(info["levels"]):
        B = dev.pc_level(l)
        err = np.abs(B - M.G[l]).max() / np.abs(M.G[l]).max()
        print(f"{name} {method} level {l}: {info['nodes'][l]} nodes, block error {err:.2e}")
        assert err <= 1e-12
        assert np.array_equal(B, np.transpose(B, (0, 2, 1)))
    assert dev.pc_info()["builds"] == 1


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_apply(gpu, name):
    from femo_amd.engine import Vec
    mesh = _meshes()[name]()
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    dev, _ = _device(gpu, mesh, rho, "SIMP", mask)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask)
    rng = np.random.default_rng(5)
    n = dev.n_dof
    rv, zv = Vec(gpu, n), Vec(gpu, n)

    def apply(v):
        rv.set(v)
        dev.pc_apply(rv, zv)
        return np.array(zv.get())

    x = rng.standard_normal(n)
    y = x + 0.5 * rng.standard_normal(n)
    zx, zy = apply(x), apply(y)
    zr = M.apply(x)
    err = np.abs(zx - zr).max() / np.abs(zr).max()
    a, b = x @ zy, y @ zx
    print(f"{name}: apply error {err:.2e}, x.M^-1 y = {a:.15e}, y.M^-1 x = {b:.15e}")
    assert err <= 1e-12
    assert abs(a - b) <= 1e-12 * abs(a)
    assert x @ zx > 0.0
    assert np.array_equal(zx[mask == 1], x[mask == 1])               # fixed dofs: as the block-Jacobi inverse maps them
    assert np.array_equal(apply(x), zx)                              # fixed summation order: the same bits again


def test_without_setup_is_an_error(gpu):
    from femo_amd._lib import FemoError
    from femo_amd.engine import Vec
    mesh = _meshes()["rect8x4"]()
    mask = clamped_face(mesh)
    dev, _ = _device(gpu, mesh, np.full(mesh.n_cell, 0.5), "SIMP", mask, setup=False)
    b, x = Vec(gpu, dev.n_dof).set(np.where(mask == 1, 0.0, 1.0)), Vec(gpu, dev.n_dof)
    with pytest.raises(FemoError, match="femo_elast_pc_setup"):
        dev.solve(b, x, pc="multilevel")
    with pytest.raises(ValueError):
        dev.solve(b, x, pc="ilu")
    assert dev.solve(b, x).converged == 1                            # Jacobi needs none


def test_form_keyword(gpu):
    from femo_amd.fea.elasticity import ElasticityResidual, pdeRes
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    mesh = _meshes()["rect8x4"]()
    u, rho = Function(VectorFunctionSpace(mesh)), Function(FunctionSpace(mesh, ("DG", 0)))
    assert ElasticityResidual(u, rho, np.zeros(2)).preconditioner == "jacobi"
    assert pdeRes(u, None, rho, np.zeros(2), preconditioner="multilevel").preconditioner == "multilevel"
    with pytest.raises(ValueError):
        ElasticityResidual(u, rho, np.zeros(2), preconditioner="ilu")


@pytest.mark.parametrize("device", [False, True])
def test_cantilever_cycle_multilevel(gpu, device):
    """The 80 x 40 cycle of test_gpu_topopt.test_cantilever_cycle with preconditioner = "multilevel": its tolerances."""
    from femo_amd.fea.utils_hip import LAST_KSP_INFO
    sim, mesh, aux = pr.build_cantilever("multilevel", device=device)
    assert aux['res'].preconditioner == "multilevel"
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    R = pr.reference_cycle(mesh, aux['facets'], aux['h_avg'], x0)
    assert np.abs(np.asarray(sim['density']) - R['rho']).max() <= 1e-14
    u = np.asarray(sim['displacements'])
    assert np.abs(u - R['u']).max() <= 1e-9 * np.abs(R['u']).max()
    assert abs(float(sim['compliance'][0]) - R['J']) <= 1e-9 * abs(R['J'])
    g = np.asarray(sim.compute_totals('compliance', 'density_unfiltered'))
    assert np.abs(g - R['grad']).max() <= 1e-8 * np.abs(R['grad']).max()
    info = aux['res'].last_info
    print(f"80x40 cantilever, multilevel: state PCG {info['state']['iterations']} it, adjoint {info['adjoint']['iterations']} it")
    assert info['state']['preconditioner'] == info['adjoint']['preconditioner'] == "multilevel"
    assert LAST_KSP_INFO[-1]['preconditioner'] == "multilevel"
    # the restatement's PCG on the same problem (filtered density, same fixed set) bounds the count
    mask = np.zeros(2 * mesh.n_vert, dtype=np.uint8)
    mask[R['fixed']] = 1
    M = pr.Multilevel(mesh.x, mesh.conn, R['rho'], "SIMP", mask, K=R['K'])
    F = R['F'].copy()
    F[mask == 1] = 0.0
    _, n_ref, ok = pr.pcg(M.A, F, M.apply, mask)
    assert ok and info['state']['iterations'] <= 1.1 * n_ref + 2
    assert dev_builds(aux['res']) >= 1


def dev_builds(form):
    return form.device().pc_info()["builds"]


def _device_counts(gpu, nelx, nely, kind):
    from femo_amd.engine import Vec
    mesh, rho, mask, facets, F = count_case(nelx, nely, kind)
    dev, _ = _device(gpu, mesh, rho, "SIMP", mask)
    b, x = Vec(gpu, dev.n_dof).set(F), Vec(gpu, dev.n_dof)
    ij = dev.solve(b, x, rtol=1e-15)
    im = dev.solve(b, x, rtol=1e-15, pc="multilevel")
    assert ij.converged == 1 and im.converged == 1
    return (mesh, rho, mask, F), ij, im


@pytest.mark.parametrize("kind", ["uniform", "truss"])
def test_counts(gpu, kind):
    """Fixed densities, rtol 1e-15, 80 x 40 and 320 x 160:
    (a) device count <= 1.1 x the restatement's count + 2 on the same problem (the margin covers summation order only),
    (b) Jacobi count >= 4 x the multilevel count at 80 x 40 and >= 10 x at 320 x 160,
    (c) count(320 x 160) <= 1.3 x count(80 x 40)."""
    dev_counts = {}
    for nelx, nely in ((80, 40), (320, 160)):
        (mesh, rho, mask, F), ij, im = _device_counts(gpu, nelx, nely, kind)
        M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask)
        _, n_ref, ok = pr.pcg(M.A, F, M.apply, mask)
        assert ok
        print(f"{kind} {nelx}x{nely}: Jacobi {ij.iterations} it {ij.solve_ms:.1f} ms, multilevel {im.iterations} it "
              f"{im.solve_ms:.1f} ms, restatement {n_ref} it")
        assert im.iterations <= 1.1 * n_ref + 2                                            # (a)
        assert ij.iterations >= (4 if nelx == 80 else 10) * im.iterations                  # (b)
        dev_counts[nelx] = im.iterations
    assert dev_counts[320] <= 1.3 * dev_counts[80]                                         # (c)


def test_counts_noise_reported(gpu):
    """Unfiltered cell noise U(1e-3, 1): reported, not capped (the restatement's count grows with the mesh)."""
    for nelx, nely in ((80, 40), (320, 160)):
        _, ij, im = _device_counts(gpu, nelx, nely, "noise")
        print(f"noise {nelx}x{nely}: Jacobi {ij.iterations} it {ij.solve_ms:.1f} ms, multilevel {im.iterations} it {im.solve_ms:.1f} ms")


def test_rebuild(gpu):
    """New rho or a new fixed set: the next solve rebuilds the blocks before it iterates, and the exported level follows."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS
    mesh = _meshes()["square9j"]()
    rng = np.random.default_rng(9)
    rho1, rho2 = rng.uniform(1e-3, 1.0, mesh.n_cell), rng.uniform(1e-3, 1.0, mesh.n_cell)
    mask = clamped_face(mesh)
    dev, rv = _device(gpu, mesh, rho1, "SIMP", mask)
    last = dev.pc_plan["levels"] - 1
    bh = np.where(mask == 1, 0.0, rng.standard_normal(dev.n_dof))
    b, x = Vec(gpu, dev.n_dof).set(bh), Vec(gpu, dev.n_dof)

    def check(rho, mk, builds):
        info = dev.solve(b, x, pc="multilevel")
        assert info.converged == 1
        assert dev.pc_info()["builds"] == builds                     # built by the solve, not by the export below
        M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mk)
        for l in (0, last):
            assert np.abs(dev.pc_level(l) - M.G[l]).max() <= 1e-12 * np.abs(M.G[l]).max()
        assert dev.pc_info()["builds"] == builds
        _, n_ref, _ = pr.pcg(M.A, bh, M.apply, mk)
        assert info.iterations <= 1.1 * n_ref + 2
        u = ref.solve_fixed(M.A, bh, np.nonzero(mk)[0], g=bh)
        assert np.abs(np.array(x.get()) - u).max() <= 1e-9 * np.abs(u).max()

    check(rho1, mask, 1)
    dev.solve(b, x, pc="multilevel")
    assert dev.pc_info()["builds"] == 1                              # nothing changed: no rebuild
    rv.set(rho2)
    dev.assemble(METHODS["SIMP"], rv)
    check(rho2, mask, 2)
    mask2 = mask.copy()
    top = np.nonzero(np.isclose(mesh.x[:, 1], 1.0))[0]
    mask2[2 * top + 1] = 1                                           # rollers on y = 1: one component of a vertex fixed
    bh[mask2 == 1] = 0.0
    b.set(bh)
    dev.set_fixed(mask2)
    dev.assemble(METHODS["SIMP"], rv)                                # the block-Jacobi inverse follows the fixed set at assembly
    check(rho2, mask2, 3)


@pytest.mark.slow
@pytest.mark.parametrize("size", ["rect640x320", "cube48"])
def test_full_size_multilevel(gpu, size):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import ElasticityResidual, Measure, meshtags
    from femo_amd.fea.function import Function, FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh, locate_entities_boundary
    from femo_amd.fea.utils_hip import dirichletbc
    if size == "rect640x320":
        mesh = createRectangleMesh([0.0, 0.0], [L_X, L_Y], 640, 320)
        tmark = lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / 320 + 3e-6, abs(x[0] - L_X) < 3e-6)
        t = np.array([0.0, -0.25])
    else:
        mesh = createUnitCubeMesh(48)
        tmark = lambda x: np.logical_and(np.isclose(x[0], 1.0), x[2] < 0.25)
        t = np.array([0.0, 0.0, -1.0])
    d = mesh.tdim
    V, Q = VectorFunctionSpace(mesh), FunctionSpace(mesh, ("DG", 0))
    u, rho = Function(V), Function(Q)
    rho.vector[:] = np.random.default_rng(2).uniform(0.3, 1.0, mesh.n_cell)
    facets = locate_entities_boundary(mesh, d - 1, tmark)
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 1)))(1)
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    dofs = (fixed_v[:, None] * d + np.arange(d)).ravel()
    form = ElasticityResidual(u, rho, t, ds)
    bcs = [dirichletbc(0.0, dofs, V)]
    sols = {}
    for pc in ("jacobi", "multilevel"):
        form.preconditioner = pc
        form.solve_state(u, bcs)
        info = form.last_info['state']
        print(f"{size} {pc}: {V.dim} dofs, PCG {info['iterations']} iterations, {info['solve_ms']:.1f} ms")
        assert info['converged'] == 1 and info['preconditioner'] == pc
        sols[pc] = (np.array(u.vec.get()), info)
    dev = form.stiffness()
    pci = dev.pc_info()
    print(f"{size}: {pci['levels']} lattices {pci['nodes']}, {pci['bytes'] / 1e6:.2f} MB, block build {pci['build_ms']:.3f} ms")
    dv, Kd = Vec(gpu, V.dim), Vec(gpu, V.dim)

    def knorm(v):
        dv.set(v)
        dev.apply(dv, Kd, masked=True)
        return np.sqrt(dv.dot(Kd, V.dim))

    uj, um = sols["jacobi"][0], sols["multilevel"][0]
    rel = knorm(um - uj) / knorm(uj)
    print(f"{size}: K-norm of the difference / K-norm of u = {rel:.2e}")
    assert rel <= 1e-9
    assert sols["multilevel"][1]['iterations'] < sols["jacobi"][1]['iterations']
