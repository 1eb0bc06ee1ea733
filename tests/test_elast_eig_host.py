"""CPU tests of the eigenfrequency restatement (tests/elast_eig_ref.py) and of the surface that needs no device.  The GPU
parity is tests/test_gpu_elast_eig.py.

Set-up of both files: the meshes of tests/test_gpu_elast_body.py, clamped on x = 0, rho = default_rng(7).uniform(0.3, 1),
consistent P1 mass, start block default_rng(1).standard_normal((n_free, L)).

Measured here (block inverse iteration with exact solves, rtol = 1e-9, SIMP / RAMP): the eigenvalues agree with the dense
eigh to 4e-13 or better; outer steps 6-14 for (n_modes, block) = (1, 3), 10-19 for (3, 5), 26-54 for (6, 8)."""
import functools

import numpy as np
import pytest

import elast_eig_ref as er
import elast_pc_ref as pr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]


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


# ------------------------------------------------------------------------------------------------------- the mass ----
@pytest.mark.parametrize("law", er.MASS_LAWS)
@pytest.mark.parametrize("name", MESHES)
def test_mass_matrix(name, law):
    """Symmetric, positive definite, and 1^T M 1 = d rho0 sum_e m(rho_e) |T_e| (every component carries the whole mass)."""
    mesh = _mesh(name)
    d, rho0 = mesh.tdim, 2.5
    rho = _rho(mesh, 0.02)                                            # some cells below the cut-off of du_olhoff
    M = er.mass(mesh.x, mesh.conn, rho, law, rho0)
    assert abs(M - M.T).max() <= 1e-16 * abs(M).max()
    Md = M.toarray()
    assert np.linalg.eigvalsh(0.5 * (Md + Md.T)).min() > 0.0
    one = np.ones(M.shape[0])
    want = d * rho0 * er.mass_law(rho, law) @ ref.cell_volumes(mesh.x, mesh.conn)
    err = abs(one @ (M @ one) - want) / want
    print(f"{name} {law}: total mass error {err:.1e}")
    assert err <= 1e-13
    # M_ff: zero rows and columns on the clamped dofs, the free block untouched
    mask = clamped_face(mesh)
    Mff = er.masked(M, mask).toarray()
    assert np.all(Mff[mask == 1] == 0.0) and np.all(Mff[:, mask == 1] == 0.0)
    assert np.array_equal(Mff[np.ix_(mask == 0, mask == 0)], Md[np.ix_(mask == 0, mask == 0)])


def test_element_mass_against_quadrature():
    """M0 of one triangle against the degree-2 edge-midpoint rule, which is exact for products of P1 functions."""
    p = np.array([[0.1, 0.2], [1.3, 0.1], [0.4, 0.9]])
    M0 = er.element_mass_matrices(p, np.array([[0, 1, 2]]))[0]
    area = ref.cell_volumes(p, np.array([[0, 1, 2]]))[0]
    mid = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]])  # barycentric values at the three midpoints
    S = area / 3.0 * mid.T @ mid
    assert np.abs(M0 - np.kron(S, np.eye(2))).max() <= 1e-16


def test_du_olhoff_law():
    """C^1 at 0.1: value 0.1 and slope exactly 1 from both sides; the derivative matches central differences."""
    eps = 1e-9
    lo, hi = er.mass_law(0.1 - eps, "du_olhoff"), er.mass_law(0.1 + eps, "du_olhoff")
    assert abs(er.mass_law(0.1, "du_olhoff") - 0.1) <= 1e-17
    assert abs(6e5 * 0.1 ** 6 - 5e6 * 0.1 ** 7 - 0.1) <= 1e-16      # the polynomial branch meets the value at 0.1
    assert abs(36e5 * 0.1 ** 5 - 35e6 * 0.1 ** 6 - 1.0) <= 1e-14     # ... and the slope 1
    # slope 1 across the joint: the curvature m'' = -300 of the polynomial adds 1.5e-16 over eps, rounding of the two
    # terms 0.6 and 0.5 a few ulp (1e-15 at the most)
    assert abs(hi - lo - 2 * eps) <= 2e-15
    assert abs(er.mass_law_d(0.1 - eps, "du_olhoff") - 1.0) <= 1e-6 and er.mass_law_d(0.1 + eps, "du_olhoff") == 1.0
    r = np.array([0.01, 0.03, 0.05, 0.08, 0.099, 0.2, 0.7])
    h = 1e-6
    fd = (er.mass_law(r + h, "du_olhoff") - er.mass_law(r - h, "du_olhoff")) / (2 * h)
    assert np.abs(fd - er.mass_law_d(r, "du_olhoff")).max() <= 1e-8
    assert np.array_equal(er.mass_law(r, "linear"), r) and np.all(er.mass_law_d(r, "linear") == 1.0)
    assert np.all(er.mass_law(r, "du_olhoff") <= r + 1e-18)          # the cut-off only lowers the mass


# --------------------------------------------------------------------------------------------------- the gradient ----
def _J(mesh, rho, mask, method, law, n_modes=3, p=8.0, density=1.3):
    return er.aggregate_gradient(mesh.x, mesh.conn, rho, mask, n_modes, p, method, law, density)[0]


@pytest.mark.parametrize("method,law,lo", [("SIMP", "linear", 0.3), ("RAMP", "linear", 0.3), ("RAMP", "du_olhoff", 0.05)])
@pytest.mark.parametrize("name", MESHES)
def test_gradient_against_central_differences(name, method, law, lo):
    """dJ/drho from the dense eigenvectors against central differences of the dense eigh on 5 cells: step 1e-6, 1e-6 of the
    largest entry of the gradient.  The truncation error of the central difference is O(h^2) = 1e-12 relative.  The noise
    of J is divided by 2 h = 2e-6 and by the size of a gradient entry relative to J (about 1e-3 on the larger meshes): the
    eigenvalues of eigh alone (relative error eps cond(K), 1e-11 on rect24x12) would miss the bound, so the restatement
    refines them by a cell-wise Rayleigh-Ritz step (`refine_eigs`).  With lo = 0.05 some cells lie below the cut-off of the
    du_olhoff law."""
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh, lo)
    J, g, lam = er.aggregate_gradient(mesh.x, mesh.conn, rho, mask, 3, 8.0, method, law, 1.3)
    assert lam[0] <= J <= 3 ** (1 / 8.0) * lam[0]
    cells = np.random.default_rng(11).choice(mesh.n_cell, 5, replace=False)
    if law == "du_olhoff":
        cells[0] = int(np.argmin(rho))                                # one cell on the polynomial branch for certain
        assert rho[cells[0]] < 0.1
    h = 1e-6
    worst = 0.0
    for c in cells:
        rp, rm = rho.copy(), rho.copy()
        rp[c] += h
        rm[c] -= h
        fd = (_J(mesh, rp, mask, method, law) - _J(mesh, rm, mask, method, law)) / (2 * h)
        worst = max(worst, abs(fd - g[c]) / np.abs(g).max())
    print(f"{name} {method} {law}: lambda {lam}, J {J:.6e}, central differences {worst:.1e}")
    assert worst <= 1e-6


def test_aggregate_derivative():
    lam = np.array([1.3, 1.35, 4.0])
    J, c = er.aggregate(lam, 8.0)
    h = 1e-6
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd = (er.aggregate(lam + e, 8.0)[0] - er.aggregate(lam - e, 8.0)[0]) / (2 * h)
        assert abs(fd - c[k]) <= 1e-8
    assert lam[0] <= J <= 3 ** (1 / 8.0) * lam[0]
    assert abs(er.aggregate(np.array([2.0, 2.0]), 3.0)[0] - 2.0) <= 1e-15


# ------------------------------------------------------------------------------------------------ the iteration ----
@functools.lru_cache(maxsize=None)
def problem(name, method):
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh)
    K = ref.stiffness(mesh.x, mesh.conn, rho, method)
    M = er.mass(mesh.x, mesh.conn, rho)
    lam, Phi = er.dense_eigs(K, M, mask, 9)
    return dict(mesh=mesh, mask=mask, rho=rho, K=K, M=M, lam=lam, Phi=Phi)


@pytest.mark.parametrize("n_modes,block", [(1, 3), (3, 5), (6, 8)])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_iteration_reaches_dense_eigenvalues(name, method, n_modes, block):
    """Exact solves, rtol 1e-9: the eigenvalue error of a symmetric pencil is of second order in the eigenvector error and
    bounded in first order by the relative residual, so 1e-8 holds with a decade to spare."""
    P = problem(name, method)
    X0 = er.start_block(P["mask"], block)
    out = er.block_inverse_iteration(P["K"], P["M"], P["mask"], X0, n_modes, er.exact_solver(P["K"], P["mask"]), rtol=1e-9)
    err = np.abs(out["lam"][:n_modes] - P["lam"][:n_modes]) / P["lam"][:n_modes]
    X = out["X"]
    G = X @ (P["M"] @ X.T)
    print(f"{name} {method} ({n_modes}, {block}): {out['outer']} outer steps, eigenvalue error {err.max():.1e}, "
          f"gap lambda_4 / lambda_3 {P['lam'][3] / P['lam'][2]:.2f}")
    assert out["converged"]
    assert err.max() <= 1e-8
    assert np.abs(G - np.eye(block)).max() <= 1e-10
    assert np.all(X[:, P["mask"] == 1] == 0.0)
    assert np.all(X[np.arange(block), np.argmax(np.abs(X), axis=1)] > 0.0)


def test_iteration_with_pcg_solves():
    """The inner solve the device uses: the batched PCG from the previous block, at rtol 1e-12."""
    P = problem("rect8x4", "SIMP")
    mesh = P["mesh"]
    Mp = pr.Multilevel(mesh.x, mesh.conn, P["rho"], "SIMP", P["mask"], K=P["K"])
    X0 = er.start_block(P["mask"], 5)
    exact = er.block_inverse_iteration(P["K"], P["M"], P["mask"], X0, 3, er.exact_solver(P["K"], P["mask"]))
    for pc in (Mp.jacobi, Mp.apply):
        out = er.block_inverse_iteration(P["K"], P["M"], P["mask"], X0, 3, er.pcg_solver(Mp.A, pc, P["mask"], 1e-12))
        err = np.abs(out["lam"][:3] - P["lam"][:3]) / P["lam"][:3]
        print(f"rect8x4 (3, 5): {out['outer']} outer steps ({exact['outer']} with exact solves), {out['pcg']} PCG iterations, "
              f"eigenvalue error {err.max():.1e}")
        assert out["converged"] and err.max() <= 1e-8
        assert abs(out["outer"] - exact["outer"]) <= 1


def test_spectra_do_not_split_a_cluster():
    """n_modes = 3 keeps the near-pair {lambda_1, lambda_2} of the cubes inside and leaves a gap of at least 2.1."""
    for name in MESHES:
        for method in ("SIMP", "RAMP"):
            lam = problem(name, method)["lam"]
            assert lam[3] / lam[2] >= 2.1, (name, method, lam[:4])


# ----------------------------------------------------------------------------------------------------- the surface ----
def test_entry_points_are_bound():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_mass_apply_multi", "femo_elast_block_gram", "femo_elast_block_rotate", "femo_elast_eig_drho",
                 "femo_elast_eigs"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.ELAST_MASS_LAWS == {"linear": 0, "du_olhoff": 1}
    import ctypes
    assert ctypes.sizeof(_lib.EigOpts) == 32 and ctypes.sizeof(_lib.EigInfo) == 16 + 8 * _lib.ELAST_MAX_COLS + 8


def test_builder_is_exported():
    from femo_amd.fea import fea_hip
    from femo_amd.fea.elasticity import EigenvalueAggregate, ElasticityEigenvalues, eigenvalue_aggregate
    assert fea_hip.eigenvalue_aggregate is eigenvalue_aggregate
    assert EigenvalueAggregate.rank == 0 and "cluster" in EigenvalueAggregate.__doc__
    assert "free-free" in ElasticityEigenvalues.__doc__
