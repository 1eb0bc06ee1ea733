"""CPU tests of the SIMP topology-optimisation surface: the vector CG1 space and its dof layout, facet location and tags,
the restatement's self-checks, the constraint record of the CSDL stubs and the reverse step of the in-repo Simulator
through an explicit operation (examples/beam_topo_opt/run_topo_opt_cantilever_beam.py)."""
import numpy as np
import pytest

import elasticity_ref as ref

L_X, L_Y = 160.0, 80.0


def _cantilever_mesh(nx=80, ny=40):
    from femo_amd.fea.mesh import createRectangleMesh
    return createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nx, ny)


def _traction_marker(ny=40):
    eps = 3e-16
    return lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / ny + eps * 1e10, abs(x[0] - L_X) < eps * 1e10)


def test_vector_space_dof_layout():
    from femo_amd.fea.function import FunctionSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = _cantilever_mesh()
    V = VectorFunctionSpace(mesh, ("CG", 1))
    assert V.bs == 2 and V.dim == 2 * mesh.n_vert and V.num_sub_spaces == 2
    assert np.array_equal(V.tabulate_dof_coordinates(), mesh.x)
    assert np.array_equal(V.sub(1).dofs, 2 * np.arange(mesh.n_vert) + 1)
    V3 = VectorFunctionSpace(createUnitCubeMesh(3), ("CG", 1))
    assert V3.bs == 3 and V3.dim == 3 * 64
    with pytest.raises(NotImplementedError):
        VectorFunctionSpace(mesh, ("CG", 2))
    with pytest.raises(NotImplementedError):           # the scalar space keeps refusing what it does not know
        FunctionSpace(mesh, ("N1curl", 1))


def test_locate_dofs_geometrical_vector_pair():
    from femo_amd.fea.function import VectorFunctionSpace
    from femo_amd.fea.mesh import locate_dofs_geometrical
    mesh = _cantilever_mesh()
    V = VectorFunctionSpace(mesh, ("CG", 1))
    dofs = locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))
    verts = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    assert verts.size == 41 and dofs.size == 82
    assert np.array_equal(np.sort(dofs), np.sort(np.concatenate([2 * verts, 2 * verts + 1])))
    one = locate_dofs_geometrical(V.sub(1), lambda x: np.isclose(x[0], 0.0, atol=1e-6))
    assert np.array_equal(np.sort(one), np.sort(2 * verts + 1))


def test_traction_facets_and_resultant():
    from femo_amd.fea.elasticity import Constant, Measure, meshtags
    from femo_amd.fea.mesh import locate_entities_boundary
    mesh = _cantilever_mesh()
    facets = locate_entities_boundary(mesh, mesh.tdim - 1, _traction_marker())
    assert facets.shape == (2, 2)
    ys = sorted(tuple(sorted(mesh.x[f, 1])) for f in facets)
    assert ys == [(38.0, 40.0), (40.0, 42.0)]
    assert np.all(mesh.x[facets, 0] == L_X)
    tags = meshtags(mesh, 1, facets, np.full(len(facets), 100, dtype=np.int32))
    ds_ = Measure("ds", domain=mesh, subdomain_data=tags, metadata={"quadrature_degree": 4})
    assert np.array_equal(ds_(100).facets(), facets)
    assert ds_(7).facets().shape[0] == 0
    f = Constant(mesh, (0, -1 / 4))
    F = ref.traction_load(mesh.x, ds_(100).facets(), f.value)
    res = F.reshape(-1, 2).sum(axis=0)
    assert abs(res[0]) <= 1e-15 and abs(res[1] + 1.0) <= 1e-15
    # the whole boundary when no tag is given
    assert Measure("ds", domain=mesh).facets().shape[0] == 2 * (80 + 40)


@pytest.mark.parametrize("d", [2, 3])
def test_restatement_rigid_body_modes(d):
    from femo_amd.fea.mesh import createUnitCubeMesh, createUnitSquareMesh
    mesh = createUnitSquareMesh(6, 0.2) if d == 2 else createUnitCubeMesh(3, 0.2)
    rho = np.random.default_rng(1).uniform(1e-3, 1.0, mesh.n_cell)
    K = ref.stiffness(mesh.x, mesh.conn, rho)
    R = ref.rigid_body_modes(mesh.x)
    assert R.shape[1] == (3 if d == 2 else 6)
    nK = abs(K).sum(axis=1).max()
    assert np.abs(K @ R).max() <= 1e-12 * nK * np.abs(R).max()
    assert abs(K - K.T).max() <= 1e-14 * nK
    # and nothing else in the kernel: K + rigid-mode projection is SPD
    ev = np.linalg.eigvalsh(K.toarray() + R @ R.T)
    assert ev.min() > 0


def test_restatement_filter_rows_sum_to_one():
    from femo_amd.fea.mesh import meshSize
    mesh = _cantilever_mesh(20, 10)
    h = meshSize(mesh)
    W = ref.filter_matrix(mesh.centroids(), 2.0 * (h.max() + h.min()) / 2)
    assert np.allclose(np.asarray(W.sum(axis=1)).ravel(), 1.0, rtol=0, atol=1e-14)
    assert W.min() >= 0.0 and np.all(W.diagonal() > 0)


def test_model_records_constraint():
    from femo_amd.csdl_opt._csdl_compat import HAVE_CSDL, Model
    if HAVE_CSDL:
        pytest.skip("real csdl installed")
    m = Model()
    m.add_constraint('avg_density', upper=0.40)
    assert m.constraints['avg_density'] == dict(lower=None, upper=0.40, equals=None, scaler=None)


def test_simulator_reverse_through_explicit_op():
    """compute_totals reaches the design variable through an explicit op whose output only feeds other ops."""
    from femo_amd.csdl_opt._csdl_compat import HAVE_CSDL, CustomExplicitOperation, Model, custom
    from femo_amd.csdl_opt.simulator import Simulator
    if HAVE_CSDL:
        pytest.skip("real csdl installed")
    A = np.array([[2.0, 1.0, 0.0], [0.0, 1.0, 3.0]])

    class Lin(CustomExplicitOperation):
        def define(self):
            self.add_input('a', shape=(3,)); self.add_output('b', shape=(2,))

        def compute(self, inputs, outputs):
            outputs['b'] = A @ np.asarray(inputs['a'])

        def compute_jacvec_product(self, inputs, d_inputs, d_outputs, mode):
            assert mode == 'rev'
            d_inputs['a'] = d_inputs['a'] + A.T @ np.asarray(d_outputs['b'])

    class Sq(CustomExplicitOperation):
        def define(self):
            self.add_input('b', shape=(2,)); self.add_output('J', shape=(1,))

        def compute(self, inputs, outputs):
            outputs['J'] = np.array([np.sum(np.asarray(inputs['b']) ** 2)])

        def compute_derivatives(self, inputs, derivatives):
            derivatives['J', 'b'] = 2.0 * np.asarray(inputs['b'])

    class M1(Model):
        def define(self):
            self.register_output('b', custom(self.declare_variable('a', shape=(3,)), op=Lin()))

    class M2(Model):
        def define(self):
            self.register_output('J', custom(self.declare_variable('b', shape=(2,)), op=Sq()))

    top = Model()
    top.add(M1(), name='m1')
    top.add(M2(), name='m2')
    top.create_input('a', shape=(3,), val=np.array([1.0, -2.0, 0.5]))
    sim = Simulator(top, pinned=False)
    sim.run()
    a = np.array([1.0, -2.0, 0.5])
    assert np.allclose(sim['J'], np.sum((A @ a) ** 2))
    g = np.asarray(sim.compute_totals('J', 'a'))
    assert np.allclose(g, 2.0 * A.T @ (A @ a), rtol=1e-14)
