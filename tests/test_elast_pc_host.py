"""Host checks of the multilevel elasticity preconditioner: the restatement (tests/elast_pc_ref.py) against its own
definitions, the caps of the GPU count tests met by the restatement alone, the plans, dead nodes and bounds of the path
cases (tests/test_gpu_elast_pc_paths.py) met by the restatement alone, and the binding of the new entry points."""
import numpy as np
import pytest

import elast_pc_ref as pr
import elasticity_ref as ref

def _case(name, method="SIMP"):
    mesh = pr.small_meshes()[name]()
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    mask = pr.clamped_face(mesh)
    return mesh, rho, mask, pr.Multilevel(mesh.x, mesh.conn, rho, method, mask)


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_plan(name):
    mesh = pr.small_meshes()[name]()
    plan = pr.lattice_plan(mesh.x, mesh.conn)
    assert min(plan["n"][0]) == 1                                    # one bin along the shortest axis
    for l in range(1, plan["n_levels"]):
        assert np.array_equal(plan["n"][l], 2 * plan["n"][l - 1]) and plan["H"][l] == plan["H"][l - 1] / 2
    h = pr.mean_edge_length(mesh.x, mesh.conn)
    assert 2.0 ** -0.5 <= plan["H"][-1] / (2.0 * h) <= 2.0 ** 0.5 or plan["n_levels"] == 1
    if name == "rect8x4":
        assert plan["nodes"][0] == 6


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_symmetric_positive(name):
    mesh, rho, mask, M = _case(name)
    rng = np.random.default_rng(3)
    n = mesh.tdim * mesh.n_vert
    for _ in range(4):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        Mx, My = M.apply(x), M.apply(y)
        assert abs(x @ My - y @ Mx) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(My)
        assert x @ Mx > 0.0
    # fixed dofs map as the block-Jacobi inverse maps them: z = r there
    x = rng.standard_normal(n)
    assert np.array_equal(M.apply(x)[mask == 1], x[mask == 1])


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_lattices_are_nested(name):
    mesh = pr.small_meshes()[name]()
    plan = pr.lattice_plan(mesh.x, mesh.conn)
    last = plan["n_levels"] - 1
    assert last >= 1
    PL = pr.interpolation(plan, mesh.x, last)
    assert abs(PL.sum(axis=1) - 1.0).max() <= 1e-14                  # partition of unity
    for l in range(last):
        P = pr.interpolation(plan, mesh.x, l)
        assert abs(P - PL @ pr.lattice_transfer(plan, last, l)).max() <= 1e-14


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
def test_cell_formula_matches_sparse_product(name, method):
    mesh, rho, mask, M = _case(name, method)
    coef = ref.penal(rho, method)
    for l in range(M.plan["n_levels"]):
        B = pr.cell_blocks(M.plan, mesh.x, mesh.conn, coef, l, mask)
        assert np.abs(B - M.G[l]).max() <= 1e-13 * np.abs(M.G[l]).max()


def reference_counts(nelx, nely, kind):
    mesh, rho, mask, facets, F = pr.count_case(nelx, nely, kind)
    M = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask)
    _, nj, cj = pr.pcg(M.A, F, M.jacobi, mask)
    _, nm, cm = pr.pcg(M.A, F, M.apply, mask)
    assert cj and cm
    return nj, nm


@pytest.mark.parametrize("kind", ["uniform", "truss"])
def test_reference_counts_meet_the_caps(kind):
    """The caps of tests/test_gpu_elast_pc.py::test_counts hold for the restatement itself on the same inputs:
    Jacobi >= 4 x multilevel at 80 x 40 and >= 10 x at 320 x 160, and count(320 x 160) <= 1.3 count(80 x 40)."""
    j80, m80 = reference_counts(80, 40, kind)
    j320, m320 = reference_counts(320, 160, kind)
    print(f"{kind}: 80x40 jacobi {j80} multilevel {m80}; 320x160 jacobi {j320} multilevel {m320}")
    assert j80 >= 4 * m80
    assert j320 >= 10 * m320
    assert m320 <= 1.3 * m80


# ------------------------------------------------------------------------------ the path cases (pr.path_meshes) ----
# The bounds of tests/test_gpu_elast_pc_paths.py are met by the restatement alone, before any device number is read.
@pytest.mark.parametrize("name", sorted(pr.PATH_PLANS))
def test_path_plan(name):
    """The plan each case was chosen for: levels, nodes, the levels beyond LDS_DOUBLES / d^2 nodes (global-atomic block
    path) and the levels below the finest beyond COARSE_THREADS nodes (several trips of the one-workgroup sweep)."""
    make, f = pr.path_meshes()[name]
    mesh = make()
    plan = pr.lattice_plan(mesh.x, mesh.conn, f)
    n_vert, n_cell, nodes = pr.PATH_PLANS[name]
    assert (mesh.n_vert, mesh.n_cell) == (n_vert, n_cell)
    assert plan["n_levels"] == len(nodes) and plan["nodes"] == nodes
    assert pr.path_levels(plan["nodes"], mesh.tdim) == pr.PATH_LEVELS[name]
    if name.startswith("fan"):
        hub, rows = pr.max_valence(mesh.conn)
        assert rows == int(name[3:5])                                # the hub row
        if name == "fan64x24_random":
            assert hub != 0 and not pr.is_lexicographic(mesh.x)
    if name == "cube5_8":
        assert pr.max_valence(mesh.conn)[1] == 18
    if name == "rect30x20_wide":                                     # the lattice sticks out of the bounding box
        assert (plan["n"][0] * plan["H"][0] > mesh.x.max(axis=0) - mesh.x.min(axis=0) + 0.25).any()
    if name == "box8j_fine":                                         # the largest of 0.5, 0.25 with > 1024 nodes below the finest
        assert pr.path_levels(pr.lattice_plan(mesh.x, mesh.conn, 0.5)["nodes"], 3)[1] == []


@pytest.mark.parametrize("name", sorted(pr.PATH_DEAD))
def test_path_dead_nodes(name):
    mesh, f, rho, mask, M = pr.path_case(name)
    dead, partly = zip(*(pr.dead_counts(G) for G in M.G))
    print(f"{name}: all-zero blocks {list(dead)}, partly dead {list(partly)}")
    assert (list(dead), list(partly)) == pr.PATH_DEAD[name]
    assert sum(partly) > 0                                           # every case has the region of rollers
    # a dead component has an exactly zero row and column in the block and in its inverse
    for G, Ci in zip(M.G, M.C):
        z = np.diagonal(G, axis1=1, axis2=2) == 0.0
        assert not G[z].any() and not np.transpose(G, (0, 2, 1))[z].any()
        assert not Ci[z].any() and not np.transpose(Ci, (0, 2, 1))[z].any()


@pytest.mark.parametrize("name", ["fan40x8", "rect30x20_wide"])
def test_path_block_bound(name):
    """The two derivations of the blocks (sparse products, cell by cell) within a quarter of block_bound, and of the
    entry-wise block_entry_bound, at every node of every level."""
    mesh, f, rho, mask, M = pr.path_case(name)
    coef = ref.penal(rho, "SIMP")
    for l, G in enumerate(M.G):
        B = pr.cell_blocks(M.plan, mesh.x, mesh.conn, coef, l, mask)
        assert np.array_equal(np.diagonal(B, axis1=1, axis2=2) == 0.0, np.diagonal(G, axis1=1, axis2=2) == 0.0)
        bn, be = pr.block_bound(G, mesh.n_cell), pr.block_entry_bound(G, mesh.n_cell)
        err = np.abs(B - G)
        live = bn > 0.0
        rn = (err[live].max(axis=(1, 2)) / bn[live]).max()
        re = (err[be > 0.0] / be[be > 0.0]).max()
        print(f"{name} level {l}: |cell - product| / bound: per node {rn:.4f}, per entry {re:.4f}")
        assert not err[~live].any() and not err[be == 0.0].any()
        assert rn <= 0.25 and re <= 0.25


@pytest.mark.parametrize("name", sorted(pr.PATH_PLANS))
def test_path_apply_bound(name):
    """fp64 application against the same one in np.longdouble: a tenth of gamma_s a entry by entry."""
    mesh, f, rho, mask, M = pr.path_case(name)
    x = np.random.default_rng(5).standard_normal(mesh.tdim * mesh.n_vert)
    z, zl, a = M.apply(x), M.apply_long(x), M.apply_abs(x)
    assert (a > 0.0).all()
    ratio = float((np.abs(z - zl) / (pr.apply_gamma(M) * a)).max())
    print(f"{name}: |fp64 - longdouble| / (gamma_s a) = {ratio:.4f}, {float(np.abs(z - zl).max() / np.abs(z).max()):.2e} of max |z|")
    assert ratio <= 0.1


@pytest.mark.parametrize("name", sorted(pr.PATH_PLANS))
def test_path_block_conditioning(name):
    mesh, f, rho, mask, M = pr.path_case(name)
    worst = [float(np.nanmax(pr.block_conditions(G))) for G in M.G]
    print(f"{name}: largest condition number of a live block, level by level: {[round(w, 2) for w in worst]}")
    assert max(worst) <= 4.0


def test_lib_binds_the_entry_points():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_pc_setup", "femo_elast_pc_info", "femo_elast_pc_export_level", "femo_elast_pc_apply"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.ELAST_PC == {"jacobi": 0, "multilevel": 1}

