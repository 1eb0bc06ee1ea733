"""GPU tests of the multilevel elasticity preconditioner (csrc/elast_pc.hip) where its other paths engage: the cases of
elast_pc_ref.path_meshes() against the restatement, node by node and entry by entry.  Every test first asserts, from the
restatement's plan and from the device's, the path it exists for: a level on the global-atomic block path, a lattice below
the finest that the one-workgroup sweep takes in several trips, nodes with an all-zero and with a partly zero block, a
numbering that is not lexicographic.  tests/test_elast_pc_host.py shows that the restatement alone meets the same bounds."""
import numpy as np
import pytest

import elast_pc_ref as pr
import elasticity_ref as ref

pytestmark = pytest.mark.gpu

CASES = pr.PATH_GPU_CASES
DEAD_CASES = ["rect30x20_wide", "rect64x32_fine", "fan64x24_random", "cube8j", "cube5_8", "box8j_fine"]
SWEEP_CASES = ["rect64x32_fine", "box8j_fine"]


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _device(gpu, name, method="SIMP"):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    mesh, f, rho, mask, M = pr.path_case(name, method)
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    dev.set_fixed(mask)
    rv = Vec(gpu, mesh.n_cell).set(rho)
    dev.assemble(METHODS[method], rv)
    dev.pc_setup(f)
    return dev, rv


def _preconditions(name, dev, mesh, M):
    """The plan of the device is the restatement's, and it takes the paths the case was chosen for."""
    info = dev.pc_info()
    d = M.d
    assert info["levels"] == M.plan["n_levels"] and info["nodes"] == M.plan["nodes"] == pr.PATH_PLANS[name][2]
    atomic, sweeps = pr.path_levels(info["nodes"], d)
    assert (atomic, sweeps) == pr.PATH_LEVELS[name]
    assert atomic and atomic[0] > 0                                  # an atomic level, and an LDS level beside it
    assert bool(sweeps) == (name in SWEEP_CASES)
    dead, partly = zip(*(pr.dead_counts(G) for G in M.G))
    assert (list(dead), list(partly)) == pr.PATH_DEAD[name]
    assert sum(partly) > 0 and (sum(dead) > 0) == (name in DEAD_CASES)
    if name == "fan64x24_random":
        hub, rows = pr.max_valence(mesh.conn)
        assert rows == 64 and hub != 0 and not pr.is_lexicographic(mesh.x)
    return info


def _check_level(B, G, n_cell):
    """One level of device blocks against the restatement's; returns the worst ratios to the per-node and the per-entry
    bound and the level-wide relative error."""
    dB, dG = np.diagonal(B, axis1=1, axis2=2), np.diagonal(G, axis1=1, axis2=2)
    assert np.array_equal(dB == 0.0, dG == 0.0)                      # the same dead components
    z = dG == 0.0
    assert not B[z].any() and not np.transpose(B, (0, 2, 1))[z].any()   # their rows and columns: exact zeros
    assert np.array_equal(B, np.transpose(B, (0, 2, 1)))
    err = np.abs(B - G)
    bn, be = pr.block_bound(G, n_cell), pr.block_entry_bound(G, n_cell)
    live = bn > 0.0
    rn = float((err[live].max(axis=(1, 2)) / bn[live]).max())
    re = float((err[be > 0.0] / be[be > 0.0]).max())
    return rn, re, float(err.max() / np.abs(G).max())


@pytest.mark.parametrize("name,method", [(n, "SIMP") for n in CASES] + [("rect52x26", "RAMP"), ("cube8j", "RAMP")])
def test_blocks_per_node(gpu, name, method):
    """Every entry of every block within 2 (n_cell + 64) 2^-53 ((lam0 + mu0) / mu0) of the node's largest diagonal entry
    (pr.block_bound), and of sqrt(G_rr G_cc) (pr.block_entry_bound: never looser); the level-wide 1e-12 beside them."""
    mesh, f, rho, mask, M = pr.path_case(name, method)
    dev, _ = _device(gpu, name, method)
    info = _preconditions(name, dev, mesh, M)
    worst = []
    for l in range(info["levels"]):
        rn, re, lv = _check_level(dev.pc_level(l), M.G[l], mesh.n_cell)
        print(f"{name} {method} level {l}: {info['nodes'][l]} nodes, |B - G| / bound: per node {rn:.4f}, per entry {re:.4f}; "
              f"level-wide {lv:.2e}")
        worst.append((rn, re, lv))
    assert max(w[0] for w in worst) <= 1.0
    assert max(w[1] for w in worst) <= 1.0
    assert max(w[2] for w in worst) <= 1e-12
    assert dev.pc_info()["builds"] == 1


@pytest.mark.parametrize("name", CASES)
def test_apply_per_entry(gpu, name):
    """|z_dev - z_ref|_i <= (gamma_s + 4 beta) a_i with a = |D^-1| |r| + sum_l |P_l| |C_l| |P_l^T| |r| (pr.apply_bound)."""
    from femo_amd.engine import Vec
    mesh, f, rho, mask, M = pr.path_case(name)
    dev, _ = _device(gpu, name)
    _preconditions(name, dev, mesh, M)
    assert max(float(np.nanmax(pr.block_conditions(G))) for G in M.G) <= 4.0
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
    bound = pr.apply_bound(M, mesh.n_cell, x)
    assert (bound > 0.0).all()
    ratio = float((np.abs(zx - zr) / bound).max())
    a, b = x @ zy, y @ zx
    print(f"{name}: |z_dev - z_ref| / ((gamma_s + 4 beta) a) = {ratio:.4f}, {np.abs(zx - zr).max() / np.abs(zr).max():.2e} of "
          f"max |z|; x.M^-1 y = {a:.15e}, y.M^-1 x = {b:.15e}")
    assert ratio <= 1.0
    assert x @ zx > 0.0
    assert abs(a - b) <= 1e-12 * abs(a)
    assert np.array_equal(zx[mask == 1], x[mask == 1])               # fixed dofs: as the block-Jacobi inverse maps them
    assert np.array_equal(apply(x), zx)                              # no rebuild in between: the same bits again
    assert dev.pc_info()["builds"] == 1


_SOLVES = {}


def _reference_solve(name):
    """(right-hand side, the restatement's PCG count, the direct solution), once per case."""
    if name not in _SOLVES:
        mesh, f, rho, mask, M = pr.path_case(name)
        bh = np.where(mask == 1, 0.0, np.random.default_rng(9).standard_normal(mesh.tdim * mesh.n_vert))
        _, n_ref, ok = pr.pcg(M.A, bh, M.apply, mask)
        assert ok
        _SOLVES[name] = (bh, n_ref, ref.solve_fixed(M.A, bh, np.nonzero(mask)[0], g=bh))
    return _SOLVES[name]


@pytest.mark.parametrize("name", CASES)
def test_solve(gpu, name):
    from femo_amd.engine import Vec
    mesh, f, rho, mask, M = pr.path_case(name)
    dev, _ = _device(gpu, name)
    _preconditions(name, dev, mesh, M)
    bh, n_ref, u = _reference_solve(name)
    b, x = Vec(gpu, dev.n_dof).set(bh), Vec(gpu, dev.n_dof)
    info = dev.solve(b, x, rtol=1e-15, pc="multilevel")
    err = np.abs(np.array(x.get()) - u).max() / np.abs(u).max()
    print(f"{name}: device {info.iterations} it, restatement {n_ref} it, error {err:.2e}")
    assert info.converged == 1
    assert info.iterations <= 1.1 * n_ref + 2
    assert err <= 1e-9


def test_columns(gpu):
    """Three columns on rect64x32_fine: each the bits and the count of its one-column solve, with the lattice vectors of a
    column 11 310 d doubles apart and the one-workgroup sweep in three trips per column."""
    from femo_amd.engine import Vec
    name = "rect64x32_fine"
    mesh, f, rho, mask, M = pr.path_case(name)
    dev, _ = _device(gpu, name)
    info = _preconditions(name, dev, mesh, M)
    assert sum(info["nodes"]) == 11310
    n, L = dev.n_dof, 3
    rng = np.random.default_rng(13)
    B = np.where(mask == 1, 0.0, rng.standard_normal((L, n)))
    b1, x1 = Vec(gpu, n), Vec(gpu, n)
    single = []
    for l in range(L):
        i = dev.solve(b1.set(B[l]), x1, rtol=1e-15, pc="multilevel")
        assert i.converged == 1
        single.append((np.array(x1.get()), i.iterations))
    bv, xv = Vec(gpu, L * n).set(B.ravel()), Vec(gpu, L * n)
    infos = dev.solve_multi(L, bv, xv, rtol=1e-15, pc="multilevel")
    X = np.array(xv.get())[:L * n].reshape(L, n)
    print(f"{name}: one-column {[s[1] for s in single]} it, batched {[i.iterations for i in infos]} it")
    for l in range(L):
        assert infos[l].converged == 1 and infos[l].iterations == single[l][1]
        assert np.array_equal(X[l], single[l][0])
    assert dev.pc_info()["builds"] == 1


def test_setup_again(gpu):
    """pc_setup(0), then pc_setup(1) on one handle: plan, last level's blocks and the build count follow each."""
    from femo_amd.engine import Vec
    name = "rect30x20_wide"
    mesh, f, rho, mask, M1 = pr.path_case(name)
    dev, _ = _device(gpu, name)
    bh, n_ref, u = _reference_solve(name)
    b, x = Vec(gpu, dev.n_dof).set(bh), Vec(gpu, dev.n_dof)
    M0 = pr.Multilevel(mesh.x, mesh.conn, rho, "SIMP", mask, spacing_factor=0.0)
    assert M0.plan["n_levels"] < M1.plan["n_levels"]
    for factor, M in ((0.0, M0), (1.0, M1)):
        dev.pc_setup(factor)
        info = dev.pc_info()
        assert info["levels"] == M.plan["n_levels"] and info["nodes"] == M.plan["nodes"]
        assert info["builds"] == 0                                   # a new plan: nothing built yet
        last = info["levels"] - 1
        rn, re, lv = _check_level(dev.pc_level(last), M.G[last], mesh.n_cell)
        print(f"{name} spacing factor {factor}: levels {info['nodes']}, last level |B - G| / bound: per node {rn:.4f}, "
              f"per entry {re:.4f}; level-wide {lv:.2e}")
        assert rn <= 1.0 and re <= 1.0 and lv <= 1e-12
        assert dev.pc_info()["builds"] == 1
        si = dev.solve(b, x, rtol=1e-15, pc="multilevel")
        assert si.converged == 1 and dev.pc_info()["builds"] == 1
        assert np.abs(np.array(x.get()) - u).max() <= 1e-9 * np.abs(u).max()
    assert si.iterations <= 1.1 * n_ref + 2
    assert pr.path_levels(dev.pc_info()["nodes"], 2)[0] == [4]       # the last level compared went through the atomic path
