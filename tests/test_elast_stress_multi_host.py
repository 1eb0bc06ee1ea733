"""CPU tests of the aggregated von Mises stress over several load cases: the NumPy restatement
(tests/elast_stress_multi_ref.py) against its own central differences on the filtered 16 x 8 cantilever with three loads,
what the two forms refuse, and the Dirichlet filter of the multiplier of a multi-column state.  The GPU parity is
tests/test_gpu_elast_stress_multi.py."""
import types

import numpy as np
import pytest

import elast_stress_multi_ref as smr
from elast_multi_ref import cantilever_loads
from test_elast_stress_host import L_X, L_Y, cantilever_mesh

WEIGHTS = (1.0, 0.5, 2.0)
P_STRESS, Q_STRESS = 8.0, 0.5


def cantilever_inputs():
    """Problem data, design and scales of the three-load 16 x 8 cantilever (shared with the GPU tests)."""
    mesh, _, h_avg = cantilever_mesh()
    facets, tractions = cantilever_loads(mesh, L_X, L_Y, 8)
    P = smr.cantilever_problem_multi(mesh, facets, tractions, h_avg)
    x0 = 1e-2 + 0.86 * np.random.default_rng(0).random(mesh.n_cell)
    rho, _, U = smr.cantilever_states(P, x0)
    m = smr.scales_from_state(mesh.x, mesh.conn, U, rho, Q_STRESS)      # fixed once: not a function of the design
    return mesh, P, x0, m


def test_total_derivative_of_the_multiload_cantilever():
    mesh, P, x0, m = cantilever_inputs()
    T = smr.cantilever_total_multi(P, x0, m, WEIGHTS, P_STRESS, Q_STRESS)
    fixed = P["fixed"]
    for l in range(3):                                                  # the adjoint right-hand sides are live on the clamped dofs
        print(f"load case {l}: max |w dJ/du| on the clamped dofs {np.abs(T['du'][l][fixed]).max():.2e}, "
              f"overall {np.abs(T['du'][l]).max():.2e}")
        assert np.abs(T["du"][l][fixed]).max() > 0.1 * np.abs(T["du"][l]).max()
        assert np.all(T["lam"][l][fixed] == 0.0)
    assert abs(T["value"] - np.dot(WEIGHTS, T["values"])) <= 1e-15 * T["value"]
    rng = np.random.default_rng(1)
    for k in range(3):
        dx = rng.standard_normal(mesh.n_cell)
        fd = (smr.cantilever_value_multi(P, x0 + 1e-5 * dx, m, WEIGHTS, P_STRESS, Q_STRESS)
              - smr.cantilever_value_multi(P, x0 - 1e-5 * dx, m, WEIGHTS, P_STRESS, Q_STRESS)) / 2e-5
        err = abs(fd - T["grad"] @ dx) / abs(fd)
        print(f"direction {k}: adjoint {T['grad'] @ dx:.12e}, central difference {fd:.12e}, rel {err:.1e}")
        assert err <= 1e-6


def test_restatement_is_the_sum_of_its_columns():
    import elast_stress_ref as sref
    from femo_amd.fea.mesh import createUnitSquareMesh
    mesh = createUnitSquareMesh(9, 0.25)
    U, rho, m, w = smr.random_columns(mesh.x, mesh.conn, 3, seed=2)
    R = smr.pnorm_stress_multi(mesh.x, mesh.conn, rho, U, m, 8.0, 0.5, weights=w)
    for l in range(3):
        S = sref.pnorm_stress(mesh.x, mesh.conn, rho, U[l], m[l], 8.0, 0.5)
        assert R["values"][l] == S["value"] and np.array_equal(R["du"][l], w[l] * S["du"])
        assert np.array_equal(R["fields"][l], S["field"])
    assert np.array_equal(smr.envelope(R["fields"]), R["fields"].max(axis=0))
    Z = smr.pnorm_stress_multi(mesh.x, mesh.conn, rho, np.stack([U[0], 0.0 * U[1]]), m[:2], 8.0, 0.5)
    assert Z["values"][1] == 0.0 and np.all(Z["du"][1] == 0.0) and np.all(np.isfinite(Z["drho"]))


# ------------------------------------------------------------------------------------------------ Python surface ----
def _spaces(mesh, n_cases=3):
    from femo_amd.fea.function import FunctionSpace, LoadCaseSpace, VectorFunctionSpace
    fn = lambda V: types.SimpleNamespace(function_space=V)              # what the constructors read of a Function
    V = VectorFunctionSpace(mesh)
    return fn(LoadCaseSpace(V, n_cases)), fn(V), fn(FunctionSpace(mesh, ("DG", 0))), fn(FunctionSpace(mesh, ("CG", 1)))


def test_constructor_refusals():
    from femo_amd.fea import elasticity as el
    from femo_amd.fea import fea_hip
    from femo_amd.fea.mesh import createRectangleMesh
    mesh, other = createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4), createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4)
    U, u1, rho, scalar = _spaces(mesh)
    _, _, rho_other, _ = _spaces(other)
    for form in (el.MultiLoadPnormStress, el.MultiLoadVonMises):
        with pytest.raises(NotImplementedError, match="LoadCaseSpace"):
            form(u1, rho)                                               # a single-column state
        with pytest.raises(NotImplementedError, match="LoadCaseSpace"):
            form(scalar, rho)
        for bad_rho in (scalar, rho_other):
            with pytest.raises(NotImplementedError, match="DG0 density"):
                form(U, bad_rho)
    # the single-column forms keep refusing a multi-column state, and say where to go
    for form in (el.ElasticityPnormStress, el.ElasticityVonMises):
        with pytest.raises(NotImplementedError, match="MultiLoadPnormStress / MultiLoadVonMises"):
            form(U, rho)
    f = el.pnorm_stress_multiload(U, rho)
    assert isinstance(f, el.MultiLoadPnormStress) and f.rank == 0 and f.functions() == (U, rho) and f.n_cases == 3
    assert np.array_equal(f.m, np.ones(3)) and np.array_equal(f.weights, np.ones(3)) and (f.p, f.q) == (8.0, 0.5)
    assert f.alpha == float(el.cell_volumes(mesh).sum()) and f.values() is None
    assert np.array_equal(el.pnorm_stress_multiload(U, rho, m=2.5).m, np.full(3, 2.5))        # a scalar: every load case
    g = el.pnorm_stress_multiload(U, rho, m=(1.0, 2.0, 3.0), weights=WEIGHTS, alpha=2.5)
    assert np.array_equal(g.m, [1.0, 2.0, 3.0]) and np.array_equal(g.weights, WEIGHTS) and g.alpha == 2.5
    for bad in (dict(m=(1.0, 2.0)), dict(m=(1.0, 2.0, 3.0, 4.0)), dict(weights=(1.0, 2.0)), dict(m=0.0), dict(m=(1.0, -1.0, 1.0)),
                dict(weights=(1.0, -0.5, 1.0)), dict(p=0.5), dict(q=-0.1), dict(alpha=0.0)):
        with pytest.raises(ValueError):
            el.pnorm_stress_multiload(U, rho, **bad)
    assert el.pnorm_stress_multiload(U, rho, weights=(1.0, 0.0, 1.0)).weights[1] == 0.0       # a zero weight is allowed
    v = el.von_Mises_stress_multiload(U)
    assert isinstance(v, el.MultiLoadVonMises) and v.q == 0.0 and v.functions() == (U,) and v.load_case is None
    assert el.von_Mises_stress_multiload(U, rho, q=0.5, load_case=2).functions() == (U, rho)
    for bad in (dict(q=0.5), dict(load_case=3), dict(load_case=-1), dict(scales=(1.0, 2.0)), dict(scales=(1.0, 0.0, 1.0))):
        with pytest.raises(ValueError):
            el.von_Mises_stress_multiload(U, **bad)
    assert fea_hip.pnorm_stress_multiload is el.pnorm_stress_multiload
    assert fea_hip.von_Mises_stress_multiload is el.von_Mises_stress_multiload
    from femo_amd import _lib
    assert {"femo_elast_pnorm_stress_multi", "femo_elast_von_mises_multi"} <= set(_lib.PROTOTYPES)


@pytest.mark.parametrize("on", [True, False])
def test_dirichlet_filter_reaches_every_column(on):
    from femo_amd.csdl_opt.state_model import StateOperation
    from femo_amd.fea.function import LoadCaseSpace, VectorFunctionSpace
    from femo_amd.fea.mesh import createRectangleMesh
    mesh = createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4)
    V = VectorFunctionSpace(mesh)
    S = LoadCaseSpace(V, 3)
    left = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    bcs = [types.SimpleNamespace(dofs=2 * left), types.SimpleNamespace(dofs=np.concatenate([2 * left + 1, 2 * left[:2]]))]
    fixed = np.unique(np.concatenate([b.dofs for b in bcs]))
    lam = np.random.default_rng(3).standard_normal(S.dim) + 3.0          # no entry is zero by accident
    keep = lam.copy()

    def run(space):
        op = types.SimpleNamespace(fea=types.SimpleNamespace(consistent_bc_partials=on), bcs=bcs,
                                   state={"function": types.SimpleNamespace(function_space=space)})
        return StateOperation._dirichlet_filtered(op, lam)

    out = run(S)
    assert np.array_equal(lam, keep)                                    # the input is not written
    if not on:
        assert out is lam
        return
    cols = out.reshape(3, V.dim)
    free = np.setdiff1d(np.arange(V.dim), fixed)
    for l in range(3):
        assert np.all(cols[l][fixed] == 0.0)
        assert np.array_equal(cols[l][free], keep.reshape(3, V.dim)[l][free])
    # any other space: the bc numbering as it is (the first V.dim entries of the same array here)
    single = run(V)
    assert np.all(single[fixed] == 0.0) and np.array_equal(np.delete(single, fixed), np.delete(keep, fixed))
