"""CPU tests of the restatement of the elastic supports and displacement outputs (tests/elast_support_ref.py) and of the
Python surface that needs no device: the total gradients against central differences, the resultant of a Winkler
foundation, the builders and the argument checks.  The GPU parity is tests/test_gpu_elast_support.py."""
import numpy as np
import pytest

import elast_support_ref as sr
import elasticity_ref as ref
from elast_pc_ref import small_meshes as _meshes


def _inverter(nelx=12, nely=6):
    from femo_amd.fea.mesh import createRectangleMesh
    mesh = createRectangleMesh([0.0, 0.0], [2.0, 1.0], nelx, nely)
    case = sr.inverter_case(mesh.x)
    h = ref.mesh_size(mesh.x, mesh.conn)
    W = ref.filter_matrix(mesh.centroids(), 2.0 * (h.max() + h.min()) / 2)
    return mesh, case, W


def _central_differences(J, grad, x0, rng, n_dir=3):
    """Step 1e-5 and tolerance 1e-6 as test_elast_multi_host.test_reference_gradient_against_central_differences."""
    for k in range(n_dir):
        dx = rng.standard_normal(x0.size)
        fd = (J(x0 + 1e-5 * dx) - J(x0 - 1e-5 * dx)) / 2e-5
        err = abs(fd - grad @ dx) / abs(fd)
        print(f"direction {k}: adjoint {grad @ dx:.12e}, central difference {fd:.12e}, rel {err:.1e}")
        assert err <= 1e-6


def test_port_displacement_gradient_against_central_differences():
    mesh, c, W = _inverter()
    rng = np.random.default_rng(0)
    x0 = 1e-2 + 0.86 * rng.random(mesh.n_cell)
    cyc = lambda x: sr.reference_cycle(mesh.x, mesh.conn, W, x, c["k"], c["F"], c["mask"], c["ell"])
    _central_differences(lambda x: cyc(x)["J"], cyc(x0)["grad"], x0, rng)


@pytest.mark.parametrize("p", [1.0, 2.0, 8.0])
def test_aggregate_gradient_through_the_state_against_central_differences(p):
    mesh, c, W = _inverter()
    rng = np.random.default_rng(1)
    x0 = 1e-2 + 0.86 * rng.random(mesh.n_cell)
    right = np.isclose(mesh.x[:, 0], 2.0)
    a = np.where(right, sr.lumped_cells(mesh.x, mesh.conn), 0.0)
    u0 = sr.reference_cycle(mesh.x, mesh.conn, W, x0, c["k"], c["F"], c["mask"], c["ell"])["u"]
    m = 1.0 / np.abs(u0).max()
    cyc = lambda x: sr.pnorm_cycle(mesh.x, mesh.conn, W, x, c["k"], c["F"], c["mask"], a, m, p)
    _central_differences(lambda x: cyc(x)["J"], cyc(x0)["grad"], x0, rng)


def test_aggregate_guards():
    """A zero state gives exact zeros, a vertex without weight is not read, a non-finite entry shows in its vertex only."""
    rng = np.random.default_rng(3)
    u, a = rng.standard_normal(20), rng.uniform(0.5, 1.0, 10)
    J, g = sr.pnorm_disp(np.zeros(20), a, 2.0, 8.0, 2)
    assert J == 0.0 and np.all(g == 0.0)
    a[4] = 0.0
    up = u.copy()
    up[9] = np.nan
    assert sr.pnorm_disp(up, a, 2.0, 8.0, 2)[0] == sr.pnorm_disp(u, a, 2.0, 8.0, 2)[0]
    for p in (1.0, 2.0, 8.0):
        for bad in (np.nan, np.inf, -np.inf):
            up = u.copy()
            up[6] = bad
            Jp, gp = sr.pnorm_disp(up, a, 2.0, p, 2)
            g0 = sr.pnorm_disp(u, a, 2.0, p, 2)[1]
            assert not np.isfinite(Jp) and not np.isfinite(gp[6:8]).any()
            assert np.array_equal(np.delete(gp, [6, 7]), np.delete(g0, [6, 7]))
    # the value is the p-mean: (J)^(1/p) / m between the weighted mean and the maximum of |u_v|
    nrm = np.linalg.norm(u.reshape(-1, 2), axis=1)
    J = sr.pnorm_disp(u, a, 2.0, 8.0, 2)[0]
    assert (a @ nrm) / a.sum() <= J ** (1 / 8.0) / 2.0 <= nrm[a > 0].max()


@pytest.mark.parametrize("name", ["rect8x4", "square9j", "cube4j"])
def test_facet_springs_resultant(name):
    from femo_amd.fea.elasticity import Measure, facet_measures, facet_springs, meshtags
    from femo_amd.fea.function import LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    mesh = _meshes()[name]()
    d = mesh.tdim
    facets = locate_entities_boundary(mesh, d - 1, lambda x: np.isclose(x[1], 0.0))
    assert len(facets) > 0
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 5, dtype=np.int32)))(5)
    V = VectorFunctionSpace(mesh)
    area = facet_measures(mesh, facets).sum()
    assert abs(area - sum(sr.facet_measure(mesh.x, f) for f in facets)) <= 1e-14 * area
    kappa = np.array([3.0, 0.5, 7.0])[:d]
    k = facet_springs(V, ds, kappa)
    assert k.shape == (V.dim,) and np.all(k >= 0.0)
    assert np.abs(k.reshape(-1, d).sum(axis=0) - kappa * area).max() <= 1e-14 * kappa.max() * area     # sum_v k_v = kappa |Gamma|
    assert np.abs(k - sr.facet_springs(mesh.x, facets, kappa)).max() <= 1e-14 * k.max()
    ks = facet_springs(LoadCaseSpace(V, 3), ds, 2.0)                  # a scalar: every component; the base space's numbering
    assert ks.shape == (V.dim,) and abs(ks.sum() - 2.0 * d * area) <= 1e-14 * 2.0 * d * area
    for bad in (-1.0, np.nan, [1.0] * (d + 1)):
        with pytest.raises(ValueError):
            facet_springs(V, ds, bad)


def test_builders_and_arguments():
    from femo_amd import _lib
    from femo_amd.fea import fea_hip
    from femo_amd.fea.elasticity import (Measure, _check_springs, mean_displacement, meshtags, point_springs,
                                         port_displacement)
    from femo_amd.fea.function import VectorFunctionSpace
    from femo_amd.fea.mesh import locate_entities_boundary
    assert {"femo_elast_set_springs", "femo_elast_pnorm_disp_multi"} <= set(_lib.PROTOTYPES)
    for name in ("point_springs", "facet_springs", "displacement", "port_displacement", "mean_displacement", "pnorm_displacement"):
        assert hasattr(fea_hip, name)                                  # exported beside pdeRes_multiload
    mesh = _meshes()["rect8x4"]()
    V = VectorFunctionSpace(mesh)
    n = V.dim
    k = point_springs(V, [3, 3, 10], [1.0, 2.0, 0.5]) + point_springs(V, 10, 0.25)       # repeated dofs and arrays add
    assert k[3] == 3.0 and k[10] == 0.75 and k.sum() == 3.75 and k.shape == (n,)
    assert np.array_equal(k, sr.point_springs(n, [3, 10], [3.0, 0.75]))
    for bad in ((n, 1.0), (-1, 1.0), (0, -1.0), (0, np.inf)):
        with pytest.raises(ValueError):
            point_springs(V, *bad)
    ell = port_displacement(V, [4, 7], [1.0, -1.0])
    assert ell[4] == 1.0 and ell[7] == -1.0 and np.count_nonzero(ell) == 2
    with pytest.raises(ValueError):
        port_displacement(V, [n])
    facets = locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 2.0))
    ds = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 5, dtype=np.int32)))(5)
    em = mean_displacement(V, (0.0, 1.0), ds)
    assert np.abs(em - ref.traction_load(mesh.x, facets, (0.0, 1.0)) / 1.0).max() <= 1e-15       # |Gamma| = 1
    assert abs(em @ np.tile([0.0, 1.0], mesh.n_vert) - 1.0) <= 1e-15    # a unit translation has mean displacement 1
    # what the residuals do with their ``springs`` argument (the constructors themselves need a device: the GPU tests)
    kc = _check_springs("test", k, n)
    assert np.array_equal(kc, k) and kc is not k
    assert _check_springs("test", None, n) is None and _check_springs("test", np.zeros(n), n) is None
    for bad in (np.zeros(n - 1), -k, np.full(n, np.nan), np.full(n, np.inf)):
        with pytest.raises(ValueError):
            _check_springs("test", bad, n)


def test_inverter_restatement_moves_the_output_backwards():
    """The restated design loop on 20 x 10: the output moves with the input at the start design and against it after ten
    steps -- the sign convention the GPU design-loop test relies on."""
    from femo_amd.fea.mesh import createRectangleMesh
    mesh = createRectangleMesh([0.0, 0.0], [2.0, 1.0], 20, 10)
    hist = sr.inverter_loop(mesh.x, mesh.conn, 10)
    print("u_out / |u_out(x1)| by step:", np.round(hist / abs(hist[0]), 3))
    assert hist[0] > 0.0 and hist[-1] < -abs(hist[0])
