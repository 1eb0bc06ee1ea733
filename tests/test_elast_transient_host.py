"""CPU checks of the restated Newmark march (tests/elast_transient_ref.py) against facts that do not depend on it: the
energy balance of the average-acceleration rule, the exact history of a single mode, one sparse solve with the whole banded
matrix, and central differences of its own J.

Measured here (rect8x4 and cube4j): the load-free energy is constant to 5e-14 relative, and the adjoint total agrees with
directional central differences (step 1e-6) to 3e-9 or better on both law pairs."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import elast_eig_ref as er
import elast_pc_ref as pr
import elast_transient_ref as tr

MESHES = ["rect8x4", "cube4j"]


@functools.lru_cache(maxsize=None)
def problem(name, case=0):
    return tr.problem(pr.small_meshes()[name](), *tr.CASES[case])


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("name", MESHES)
def test_energy_is_constant_without_load(name):
    """beta = 1/4, gamma = 1/2, no damping, the load switched off after step 4: E_{n+1/2} is constant over the load-free steps
    (it follows exactly from the recurrence)."""
    P = problem(name)
    N = 19
    g = np.zeros(N + 1)
    g[:5] = [0.0, 0.5, 1.0, 1.0, 0.5]
    c = tr.blocks(P["dt"])
    U = tr.march(P["K"], P["M"], P["mask"], tr.load_history(P["F"], g, c, P["mask"]), c)
    E = tr.energies(P["K"], P["M"], U, P["dt"])
    # step n -> n + 1 carries g_{n+1}, g_n, g_{n-1}: from n = 6 on (g_5 = 0 onwards) no load enters, so E_{5+1/2} ... are equal
    free = E[5:]
    spread = np.abs(free - free[0]).max() / free[0]
    print(f"{name}: load-free energy {free[0]:.6e}, relative spread {spread:.1e}")
    assert free[0] > 0.0 and spread <= 1e-10


@pytest.mark.parametrize("rayleigh", [(0.0, 0.0), (0.05, 0.002)])
@pytest.mark.parametrize("name", MESHES)
def test_single_mode(name, rayleigh):
    """F = M phi with K phi = lambda M phi: the history is q_n phi, q_n from the scalar recurrence; Rayleigh damping keeps
    the modes uncoupled."""
    P = problem(name)
    lam, Phi = er.dense_eigs(P["K"], P["M"], P["mask"], 3)
    N = 19
    g = tr.default_signal(N)
    for beta, gamma in ((0.25, 0.5), (0.3025, 0.6)):
        c = tr.blocks(P["dt"], beta, gamma, rayleigh)
        for k in (0, 2):
            F = er.masked(P["M"], P["mask"]) @ Phi[:, k]
            U = tr.march(P["K"], P["M"], P["mask"], tr.load_history(F, g, c, P["mask"]), c)
            q = tr.scalar_recurrence(lam[k], g, c)
            assert _maxrel(U, np.outer(q, Phi[:, k])) <= 1e-10


@pytest.mark.parametrize("scheme", tr.SCHEMES)
@pytest.mark.parametrize("n_steps", tr.STEP_COUNTS)
def test_march_against_sparse_solve(n_steps, scheme):
    P = problem("rect8x4")
    beta, gamma, rayleigh = scheme
    c = tr.blocks(P["dt"], beta, gamma, rayleigh)
    L = tr.band(P["K"], P["M"], P["mask"], n_steps, c)
    B = tr.load_history(P["F"], tr.default_signal(n_steps), c, P["mask"])
    U = tr.march(P["K"], P["M"], P["mask"], B, c)
    assert _maxrel(U.ravel(), spla.spsolve(L.tocsc(), B.ravel())) <= 1e-10
    S = np.random.default_rng(3).standard_normal(B.shape)
    Lam = tr.march(P["K"], P["M"], P["mask"], S, c, reverse=True)
    assert _maxrel(Lam.ravel(), spla.spsolve(L.T.tocsc(), S.ravel())) <= 1e-10


def test_band_is_block_toeplitz_with_symmetric_blocks():
    P = problem("rect8x4")
    c = tr.blocks(P["dt"], 0.3025, 0.6, (0.05, 0.002))
    n = P["K"].shape[0]
    L = tr.band(P["K"], P["M"], P["mask"], 4, c).tocsr()
    for j in range(3):
        blk = L[j * n:(j + 1) * n, :n]
        assert abs(blk - blk.T).max() <= 1e-15 * abs(blk).max()
        assert abs(L[(j + 1) * n:(j + 2) * n, n:2 * n] - blk).max() == 0.0
    assert L[:n, n:].nnz == 0


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("case", range(len(tr.CASES)))
def test_adjoint_total_against_central_differences(case, squared):
    """dJ/drho of the discrete adjoint along a direction, step 1e-6, the project's bound for directional differences."""
    P = problem("rect8x4", case)
    mesh, mask = P["mesh"], P["mask"]
    method, law = tr.CASES[case]
    N = 9
    g = tr.default_signal(N)
    c = tr.blocks(P["dt"], 0.3025, 0.6, (0.05, 0.002))
    args = dict(squared=squared, method=method, law=law, density=P["density"])
    J, grad, cn, U, Lam = tr.adjoint_total(mesh.x, mesh.conn, P["rho"], mask, P["F"], g, c, **args)
    assert J == pytest.approx(P["dt"] * np.sum(cn * cn if squared else cn), rel=1e-14)
    d = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-6
    Jp = tr.adjoint_total(mesh.x, mesh.conn, P["rho"] + h * d, mask, P["F"], g, c, **args)[0]
    Jm = tr.adjoint_total(mesh.x, mesh.conn, P["rho"] - h * d, mask, P["F"], g, c, **args)[0]
    fd, an = (Jp - Jm) / (2 * h), float(grad @ d)
    print(f"{tr.CASES[case]} squared={squared}: central differences {abs(fd - an) / abs(an):.1e}")
    assert abs(fd - an) <= 1e-5 * abs(an)


def test_drho_forward_and_transpose_are_transposes():
    P = problem("cube4j", 1)
    mesh = P["mesh"]
    rng = np.random.default_rng(5)
    N = 9
    c = tr.blocks(P["dt"], 0.3025, 0.6, (0.05, 0.002))
    U, X, dr = rng.standard_normal((N, P["K"].shape[0])), rng.standard_normal((N, P["K"].shape[0])), rng.standard_normal(mesh.n_cell)
    args = dict(method="RAMP", law="du_olhoff", density=P["density"])
    a = float(np.sum(X * tr.drho_N(mesh.x, mesh.conn, P["rho"], U, dr, c, **args)))
    b = float(dr @ tr.drho_T(mesh.x, mesh.conn, P["rho"], U, X, c, **args))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b))


def test_entry_points_are_bound():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_newmark_rhs", "femo_elast_newmark_march", "femo_elast_newmark_apply", "femo_elast_newmark_drho",
                 "femo_elast_newmark_dots", "femo_elast_newmark_outer"):
        assert hasattr(lib, name)


def test_builders_are_exported():
    from femo_amd.fea import fea_hip
    from femo_amd.fea.function import TimeHistorySpace
    for name in ("pdeRes_transient", "transient_compliance", "TimeHistorySpace", "TransientElasticityResidual",
                 "TransientCompliance"):
        assert hasattr(fea_hip, name), name
    assert TimeHistorySpace is fea_hip.TimeHistorySpace
