"""CPU tests of the buckling restatement (tests/elast_buckle_ref.py) and of the surface that needs no device.  The GPU parity
is tests/test_gpu_elast_buckle.py.

Set-up of both files: the meshes of tests/test_gpu_elast_eig.py, clamped on x = 0, a compressive unit traction (-1, 0[, 0])
on the face x = x_max, rho = default_rng(7).uniform(0.3, 1), start block default_rng(1).standard_normal((n_free, L)).

Measured here (SIMP / RAMP, all five meshes): the largest positive mu = 1 / lambda lies between 20 and 108 and no negative mu
exceeds 0.52 in magnitude, so the positive end of the spectrum dominates; lambda_3 / lambda_2 between 1.14 and 1.98; the
restated total gradient agrees with central differences to 4e-9 or better; the block iteration with exact solves, rtol =
1e-9, takes 15-31 outer steps for (n_modes, block) = (1, 3) and 31-85 for (3, 8) and reaches the dense load factors to
3e-13 or better; with the zero-guess pcg_multi at 1e-12 the outer counts are the same."""
import functools

import numpy as np
import pytest

import elast_buckle_ref as bk
import elast_eig_ref as er
import elast_pc_ref as pr
import elast_stress_ref as sr
import elasticity_ref as ref
from elast_pc_ref import clamped_face

MESHES = ["rect8x4", "square9j", "cube4j", "rect24x12", "cube6j"]
BODY = (0.0, -0.5)                                                    # the body force of the one body-load case (rect8x4, RAMP)


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


@functools.lru_cache(maxsize=None)
def problem(name, method):
    """The state under the compressive end load, K_G and the dense load factors: built once, read only."""
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh)
    S = bk.state(mesh, rho, mask, method)
    D = bk.dense_buckling(S["K"], S["KG"], mask, 9)
    return dict(mesh=mesh, mask=mask, rho=rho, K=S["K"], KG=S["KG"], u=S["u"], lam=D["lam"], Phi=D["Phi"], mu=D["mu"])


# ------------------------------------------------------------------------------------------ the element matrix ----
@pytest.mark.parametrize("d", [2, 3])
def test_element_geometric_matrix(d):
    """K_G,e is symmetric, annihilates the rigid translations, and phi^T K_G,e phi = |T| sigma : H on a linear field phi = A x
    (whose gradient is A in the cell, so H = A^T A)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((d + 1, d))
    conn = np.arange(d + 1, dtype=np.int32)[None, :]
    s = rng.standard_normal((d, d))
    sig = 0.5 * (s + s.T)[None, :, :]
    KG = bk.element_geometric_matrices(x, conn, sig)[0]
    vol = ref.cell_volumes(x, conn)[0]
    assert np.abs(KG - KG.T).max() <= 1e-14 * np.abs(KG).max()
    for k in range(d):
        t = np.zeros((d + 1, d))
        t[:, k] = 1.0
        assert np.abs(KG @ t.ravel()).max() <= 1e-13 * np.abs(KG).max()
    A = rng.standard_normal((d, d))
    phi = sr.linear_field(x, A)
    want = vol * np.sum(sig[0] * (A.T @ A))
    err = abs(phi @ KG @ phi - want) / abs(want)
    H = bk.mode_H(x, conn, phi[:, None])[0, 0]
    print(f"d = {d}: phi^T K_G phi against |T| sigma : H {err:.1e}")
    assert err <= 1e-12
    assert np.abs(H - A.T @ A).max() <= 1e-12 * np.abs(A.T @ A).max()


@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_assembled_geometric_stiffness(name, method):
    """Symmetric; x^T K_G x = sum_e |T_e| sigma_e : H_e(x); the stress buffer layout lists every component once."""
    P = problem(name, method)
    mesh, KG = P["mesh"], P["KG"]
    assert abs(KG - KG.T).max() <= 1e-14 * abs(KG).max()
    xv = np.random.default_rng(4).standard_normal(KG.shape[0])
    sig = bk.cell_stress(mesh.x, mesh.conn, P["rho"], P["u"], method)
    want = np.sum(ref.cell_volumes(mesh.x, mesh.conn) * np.einsum("emn,emn->e", sig, bk.mode_H(mesh.x, mesh.conn, xv[:, None])[0]))
    assert abs(xv @ (KG @ xv) - want) <= 1e-12 * abs(want)
    d = mesh.tdim
    assert bk.stress_components(sig).shape == (d * (d + 1) // 2, mesh.n_cell)


# --------------------------------------------------------------------------------------------------- the gradient ----
def _gradient_cases():
    for name in MESHES:
        for method in ("SIMP", "RAMP"):
            yield name, method, None
    yield "rect8x4", "RAMP", BODY


@pytest.mark.parametrize("name,method,body", list(_gradient_cases()))
def test_total_gradient_against_central_differences(name, method, body):
    """The restated adjoint total gradient of J (n_modes = 2, p = 8) against central differences of the dense J along one
    direction: step 1e-5 along default_rng(8).uniform(0.5, 1.5), 1e-6 relative.  The direction has positive entries, so the
    derivative is of the size of J itself; the truncation error is O(h^2) = 1e-10 relative, and the rounding of the dense
    eigh (the wanted mu are the LARGEST of the pencil, so they carry its full relative accuracy, about 1e-13) divided by
    2 h stays below 1e-8."""
    mesh = _mesh(name)
    mask = clamped_face(mesh)
    rho = _rho(mesh)
    T = bk.total_gradient(mesh, rho, mask, 2, 8.0, method, body=body)
    dvec = np.random.default_rng(8).uniform(0.5, 1.5, mesh.n_cell)
    h = 1e-5
    Jp = bk.aggregate_value(mesh, rho + h * dvec, mask, 2, 8.0, method, body=body)
    Jm = bk.aggregate_value(mesh, rho - h * dvec, mask, 2, 8.0, method, body=body)
    fd, an = (Jp - Jm) / (2 * h), float(T["grad"] @ dvec)
    err = abs(fd - an) / abs(an)
    print(f"{name} {method} body={body}: lambda {T['lam']}, J {T['J']:.6e}, directional derivative {an:.9e}, "
          f"central differences {fd:.9e}, {err:.1e}")
    assert T["lam"][0] <= T["J"] <= 2 ** (1 / 8.0) * T["lam"][0]
    assert err <= 1e-6


def test_partials_against_central_differences():
    """Each partial alone on rect8x4: d/drho at fixed u and d/du at fixed rho (the latter along a direction that is live on
    the clamped dofs as well), against central differences of the dense aggregate with the other argument frozen."""
    P = problem("rect8x4", "RAMP")
    mesh, mask, rho, u = P["mesh"], P["mask"], P["rho"], P["u"]
    x, conn = mesh.x, mesh.conn

    def J(rho_, u_):
        KG = bk.geometric_stiffness(x, conn, rho_, u_, "RAMP")
        return bk.aggregate(bk.dense_buckling(ref.stiffness(x, conn, rho_, "RAMP"), KG, mask, 2)["lam"], 8.0)[0]

    lam, Phi = P["lam"][:2], P["Phi"][:, :2]
    _, c = bk.aggregate(lam, 8.0)
    du = bk.buckle_du(x, conn, rho, Phi, c * lam ** 2, "RAMP")
    drho = bk.buckle_drho(x, conn, rho, u, Phi, c * lam, c * lam ** 2, "RAMP")
    rng = np.random.default_rng(9)
    dr, dv = rng.uniform(0.5, 1.5, mesh.n_cell), rng.standard_normal(u.size) * np.abs(u).max()
    h = 1e-5
    fr = (J(rho + h * dr, u) - J(rho - h * dr, u)) / (2 * h)
    fu = (J(rho, u + h * dv) - J(rho, u - h * dv)) / (2 * h)
    er_, eu = abs(fr - drho @ dr) / abs(fr), abs(fu - du @ dv) / abs(fu)
    print(f"rect8x4 RAMP: d/drho {er_:.1e}, d/du {eu:.1e}; |dJ/du| on the clamped dofs {np.abs(du[mask == 1]).max():.2e}")
    assert er_ <= 1e-6 and eu <= 1e-6
    assert np.abs(du[mask == 1]).max() > 0.0                          # why the totals need consistent_bc_partials


def test_aggregate_is_shared():
    """The aggregate is that of the eigenfrequency restatement, and the library's forms share one formula too."""
    from femo_amd.fea import elasticity as el
    assert bk.aggregate is er.aggregate
    lam = np.array([1.3, 1.35, 4.0])
    J, c = el._reciprocal_power_mean(lam, 8.0)
    Jr, cr = er.aggregate(lam, 8.0)
    assert J == Jr and np.array_equal(c, cr)


# ------------------------------------------------------------------------------------------------ the iteration ----
@functools.lru_cache(maxsize=None)
def exact_iteration(name, method, n_modes, block):
    P = problem(name, method)
    return bk.block_power_iteration(P["K"], P["KG"], P["mask"], er.start_block(P["mask"], block), n_modes,
                                    er.exact_solver(P["K"], P["mask"]), rtol=1e-9)


@pytest.mark.parametrize("n_modes,block", [(1, 3), (3, 8)])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_iteration_reaches_dense_load_factors(name, method, n_modes, block):
    """Exact solves, rtol 1e-9: the error of an eigenvalue of a symmetric pencil is of second order in the eigenvector error
    and bounded in first order by the relative residual, so 1e-8 holds with a decade to spare."""
    P = problem(name, method)
    out = exact_iteration(name, method, n_modes, block)
    err = np.abs(out["lam"][:n_modes] - P["lam"][:n_modes]) / P["lam"][:n_modes]
    X = out["X"]
    G = X @ (P["K"] @ X.T)
    print(f"{name} {method} ({n_modes}, {block}): {out['outer']} outer steps, load factor error {err.max():.1e}, "
          f"mu_1 {P['mu'][0]:.1f}, most negative mu {P['mu'][-1]:.2f}")
    assert out["converged"]
    assert err.max() <= 1e-8
    assert np.all(np.diff(out["lam"][:n_modes]) >= 0.0) and np.all(out["lam"][:n_modes] > 0.0)
    assert np.abs(G - np.eye(block)).max() <= 1e-10
    assert np.all(X[:, P["mask"] == 1] == 0.0)
    assert np.all(X[np.arange(block), np.argmax(np.abs(X), axis=1)] > 0.0)


@pytest.mark.parametrize("n_modes,block", [(1, 3), (3, 8)])
@pytest.mark.parametrize("method", ["SIMP", "RAMP"])
@pytest.mark.parametrize("name", MESHES)
def test_iteration_with_pcg_solves(name, method, n_modes, block):
    """The inner solve the device uses: the batched PCG from a zero first guess at rtol 1e-12 (block-Jacobi here).  Three
    decades below the outer rtol, so the outer count is that of exact solves, give or take one."""
    P = problem(name, method)
    d = P["mesh"].tdim
    A = pr.masked_operator(P["K"], P["mask"])
    Dinv = pr.invert_blocks(pr.block_diagonal(A, d))
    jacobi = lambda r: np.einsum("nij,nj->ni", Dinv, r.reshape(-1, d)).ravel()
    out = bk.block_power_iteration(P["K"], P["KG"], P["mask"], er.start_block(P["mask"], block), n_modes,
                                   bk.zero_guess_pcg_solver(A, jacobi, P["mask"], 1e-12), rtol=1e-9)
    exact = exact_iteration(name, method, n_modes, block)
    err = np.abs(out["lam"][:n_modes] - P["lam"][:n_modes]) / P["lam"][:n_modes]
    print(f"{name} {method} ({n_modes}, {block}): {out['outer']} outer steps ({exact['outer']} with exact solves), "
          f"{out['pcg']} PCG iterations, load factor error {err.max():.1e}")
    assert out["converged"] and err.max() <= 1e-8
    assert abs(out["outer"] - exact["outer"]) <= 1


def test_spectra_do_not_split_a_cluster():
    """n_modes = 2 never splits a cluster: lambda_3 / lambda_2 >= 1.1 on all ten cases; and the positive end of the spectrum
    dominates under the compressive load, so the sign limitation of the iteration is not in play."""
    for name in MESHES:
        for method in ("SIMP", "RAMP"):
            P = problem(name, method)
            assert P["lam"][2] / P["lam"][1] >= 1.1, (name, method, P["lam"][:4])
            assert P["mu"][0] > 10.0 * abs(P["mu"][-1]), (name, method, P["mu"][0], P["mu"][-1])


def test_tensile_load_has_a_negative_spectrum():
    """Under the reversed (tensile) load K_G changes sign: the dominant mu are negative, which is what the device's
    'block too small' error is about."""
    mesh = _mesh("rect8x4")
    mask = clamped_face(mesh)
    S = bk.state(mesh, _rho(mesh), mask, "SIMP", traction=bk.end_traction(mesh, +1.0))
    mu = bk.dense_buckling(S["K"], S["KG"], mask, 0)["mu"]
    P = problem("rect8x4", "SIMP")
    assert np.abs(mu + P["mu"][::-1]).max() <= 1e-10 * np.abs(mu).max()        # the spectrum of the compressive load, mirrored
    out = bk.block_power_iteration(S["K"], S["KG"], mask, er.start_block(mask, 3), 3, er.exact_solver(S["K"], mask), max_outer=50)
    assert not out["converged"] and np.all(out["mu"][:3] < 0.0)
    assert out["residual"][2] <= 1e-9 and abs(out["mu"][2] + P["mu"][0]) <= 1e-8 * P["mu"][0]    # the dominant one has converged


# ----------------------------------------------------------------------------------------------------- the surface ----
def test_entry_points_are_bound():
    from femo_amd import _lib
    lib = _lib.load()
    for name in ("femo_elast_geom_stress", "femo_elast_geom_apply_multi", "femo_elast_buckle_du", "femo_elast_buckle_drho",
                 "femo_elast_buckle", "femo_elast_geom_stress_get"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 10 and lib.femo_abi_version() == 10    # a pure addition


def test_builder_is_exported():
    from femo_amd.fea import fea_hip
    from femo_amd.fea.elasticity import (BucklingAggregate, DeviceElasticity, ElasticityBuckling, ElasticityEigenvalues,
                                         buckling_aggregate)
    assert fea_hip.buckling_aggregate is buckling_aggregate
    assert BucklingAggregate.rank == 0 and "consistent_bc_partials" in BucklingAggregate.__doc__
    assert "raise ``block``" in ElasticityBuckling.__doc__ and "Out of scope" in ElasticityBuckling.__doc__
    assert "ElasticityBuckling" in ElasticityEigenvalues.__doc__
    for name in ("geom_stress", "geom_apply_multi", "buckle_du", "buckle_drho", "buckle"):
        assert callable(getattr(DeviceElasticity, name))
