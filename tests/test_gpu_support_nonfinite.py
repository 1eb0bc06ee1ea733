"""GPU tests of the contract "no output hides a non-finite state" (rules (1), (2) and (4)) for the
displacement aggregate femo_elast_pnorm_disp_multi, with the helpers of tests/nonfinite.py, and of the refusals of
femo_elast_set_springs.  One poisoned entry of u shows in J_l of its column and in the d gradient entries of its vertex, and
nowhere else; under a vertex without weight it changes nothing."""
import functools

import numpy as np
import pytest

import elast_pc_ref as pr
import elast_support_ref as sr
import nonfinite as nf
from nonfinite import VALUES

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def _mesh(name):
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh
    return createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12) if name == "rect24x12" else createUnitCubeMesh(6, 0.2)


def _case(mesh, L, p):
    d, nv = mesh.tdim, mesh.n_vert
    rng = np.random.default_rng(5)
    U = rng.standard_normal((L, d * nv)) * (10.0 ** -np.arange(L))[:, None]
    a = sr.lumped_cells(mesh.x, mesh.conn)
    m = 1.0 / np.array([np.linalg.norm(u.reshape(-1, d), axis=1).max() for u in U])
    return dict(U=U, a=a, m=m, w=rng.uniform(0.25, 2.0, L), p=p)


def _call(gpu, dev, A):
    from femo_amd.engine import Vec
    L = len(A["U"])
    g = Vec(gpu, A["U"].size).fill(0.0)
    vals = dev.pnorm_disp_multi(L, Vec(gpu, A["U"].size).set(A["U"].ravel()), Vec(gpu, A["a"].size).set(A["a"]), A["m"], A["p"],
                                weights=A["w"], grad_u=g)
    return np.array(vals), np.array(g.get()).reshape(L, -1)


def _restate(mesh, A):
    out = [sr.pnorm_disp(u, A["a"], m, A["p"], mesh.tdim) for u, m in zip(A["U"], A["m"])]
    return np.array([t[0] for t in out]), np.stack([w * t[1] for w, t in zip(A["w"], out)])


@pytest.mark.parametrize("p", [1.0, 8.0])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("name", ["rect24x12", "cube6j"])
def test_poisoned_state(gpu, name, L, p):
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh(name)
    d, nv = mesh.tdim, mesh.n_vert
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    A = _case(mesh, L, p)
    cleanJ, cleanG = _call(gpu, dev, A)
    bad = []
    for col in sorted({0, L - 1}):
        for entry in nf.positions(mesh.conn, d):
            vertex = np.zeros(nv, dtype=bool)
            vertex[entry // d] = True
            for value in VALUES:
                B = dict(A, U=nf.poison(A["U"], col * d * nv + entry, value))
                gotJ, gotG = _call(gpu, dev, B)
                wantJ, wantG = _restate(mesh, B)
                label = f"{name} L={L} p={p} column {col} entry {entry} <- {value}"
                assert not np.isfinite(wantJ[col]) and not np.isfinite(wantG[col].reshape(-1, d)[entry // d]).any(), label
                bad += nf.violations(gotJ, wantJ, cleanJ, np.arange(L) == col, label=label + ": values")
                bad += nf.violations(gotG, wantG, cleanG, nf.in_column(nf.vertex_dofs(vertex, d), L, col), label=label + ": dJ/du")
                # stated outright: the value of the column and all d entries of the vertex
                if np.isfinite(gotJ[col]) or np.isfinite(gotG[col].reshape(-1, d)[entry // d]).any():
                    bad.append(label + ": the poisoned entry does not show in its value or in its vertex")
    assert not bad, "\n".join(bad)


def test_poison_under_a_vertex_without_weight_changes_nothing(gpu):
    from femo_amd.fea.elasticity import DeviceElasticity
    mesh = _mesh("rect24x12")
    d = mesh.tdim
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    A = _case(mesh, 3, 8.0)
    entries = nf.positions(mesh.conn, d)
    A["a"] = A["a"].copy()
    A["a"][[e // d for e in entries]] = 0.0
    cleanJ, cleanG = _call(gpu, dev, A)
    for entry in entries:
        for value in VALUES:
            gotJ, gotG = _call(gpu, dev, dict(A, U=nf.poison(A["U"], d * mesh.n_vert + entry, value)))
            assert np.array_equal(gotJ, cleanJ) and np.array_equal(gotG, cleanG), (entry, value)


def test_set_springs_refuses_bad_entries(gpu):
    from femo_amd._lib import FemoError
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    mesh = pr.small_meshes()["rect8x4"]()
    dev = DeviceElasticity(gpu, mesh, 1.0, 0.3)
    n = dev.n_dof
    rho = Vec(gpu, mesh.n_cell).fill(0.5)
    k = np.random.default_rng(1).uniform(0.0, 2.0, n)
    dev.set_springs(k)
    dev.assemble(METHODS["SIMP"], rho)
    good = dev.export_csr()
    key = dev.springs_key
    for value in VALUES + (-1.0,):
        with pytest.raises(FemoError, match="set_springs"):
            dev.set_springs(nf.poison(k, n // 2, value))
        with pytest.raises(FemoError):
            dev.set_springs(k[:-1])
        assert dev.springs_key == key                                 # the handle is as it was: products go on ...
        x, y = Vec(gpu, n).fill(1.0), Vec(gpu, n)
        assert np.abs(np.array(dev.apply_multi(1, x, y).get()) - good @ np.ones(n)).max() <= 1e-12 * np.abs(good).max()
    dev.set_springs(2.0 * k)                                          # ... and the call after a refusal works
    dev.assemble(METHODS["SIMP"], rho)
    assert np.abs((dev.export_csr() - good).diagonal() - k).max() <= 1e-12 * np.abs(good).max()
