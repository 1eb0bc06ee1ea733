"""One operator assembly per cycle for a form with constant partials (linear Poisson): Newton assembles dR/du and A once
-- or takes StateOperation's early linearisation of the same cycle -- and forms every right-hand side by a product
(`_NewtonBase.linear_reuse`), against the path that walks the mesh for every residual."""
import numpy as np
import pytest

from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

TOL = 1e-10           # tests/test_gpu_hostmem.py::test_early_linearisation_is_the_same_cycle; not bitwise: the brick
#                       restriction of the preconditioner accumulates with fp64 atomics
N = 24


def _rel2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


class _Passes:
    """Counts, per cycle, the passes over the mesh that write a matrix, those that write only a right-hand side or residual,
    and the right-hand sides formed by product."""

    def __init__(self, monkeypatch):
        from femo_amd import _lib
        from femo_amd import engine as E
        self.matrix = self.rhs_only = self.products = 0
        sys_, jac_, res_, prod_ = E.assemble_system, E.assemble_jacobian, E.assemble_residual, E.newton_rhs_linear

        def assemble_system(mesh, pde, params, u, f, bc, J_nobc, A_bc, rhs, aux=None):
            if J_nobc is not None or A_bc is not None:
                self.matrix += 1
            else:
                self.rhs_only += 1
            return sys_(mesh, pde, params, u, f, bc, J_nobc, A_bc, rhs, aux=aux)

        def assemble_jacobian(mesh, pde, *a, **k):
            if pde in (_lib.PDE_POISSON, _lib.PDE_NL_POISSON):
                self.matrix += 1
            return jac_(mesh, pde, *a, **k)

        def assemble_residual(*a, **k):
            self.rhs_only += 1
            return res_(*a, **k)

        def newton_rhs_linear(*a, **k):
            self.products += 1
            return prod_(*a, **k)

        monkeypatch.setattr(E, "assemble_system", assemble_system)
        monkeypatch.setattr(E, "assemble_jacobian", assemble_jacobian)
        monkeypatch.setattr(E, "assemble_residual", assemble_residual)
        monkeypatch.setattr(E, "newton_rhs_linear", newton_rhs_linear)

    def take(self):
        out = (self.matrix, self.rhs_only, self.products)
        self.matrix = self.rhs_only = self.products = 0
        return out


@pytest.fixture(scope="module")
def problem():
    from bench import source_fields
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(N, jitter=0.2)
    fs = source_fields(mesh, 2)
    om = fo.unit_cube_mesh(N, jitter=0.2)
    bd = fo.boundary_vertices_box(om.x)
    ref = fo.reference_cycle(om, fs[1], fo.u_target(om.x), bd, np.zeros(len(bd)))      # once, shared, never written
    for v in ref.values():
        v.setflags(write=False)
    return mesh, fs, ref


def _cycles(ctx, mesh, fs, reuse, early, passes, start=0.0, noise=None):
    """Two cycles through the operator surface (the second one has the early linearisation, when it is on); returns the
    second cycle's state, gradient, functional, CG counts per Newton pass and pass counts."""
    from bench import build_problem
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    base = utils_hip._NewtonBase
    reuse0, noise0 = base.linear_reuse, base.NOISE_FACTOR
    base.linear_reuse = reuse
    if noise is not None:
        base.NOISE_FACTOR = noise
    try:
        sim, fea = build_problem(mesh, device=False)
        fea.early_linearisation = early
        ufn = fea.states_dict['u']['function']
        u0 = E.pinned_full(mesh.n_vert, start)

        def cycle(f):
            sim['f'] = E.pinned_array(f)
            ufn.vector.set(start)
            sim['u'] = u0
            sim.run()
            return sim.compute_totals('l2_functional', 'f')

        cycle(fs[0])
        passes.take()
        del utils_hip.LAST_KSP_INFO[:]
        g = cycle(fs[1])
        its = [i["iterations"] for i in utils_hip.LAST_KSP_INFO]
        out = dict(u=np.array(E.host_wait(sim['u']), copy=True), g=np.array(E.host_wait(g), copy=True).ravel(),
                   J=float(np.asarray(sim['l2_functional']).ravel()[0]), its=its, passes=passes.take())
        utils_hip.clear_workspaces()
        return out
    finally:
        base.linear_reuse, base.NOISE_FACTOR = reuse0, noise0


def test_the_two_newton_paths_agree(ctx, problem, monkeypatch):
    mesh, fs, ref = problem
    passes = _Passes(monkeypatch)
    new = _cycles(ctx, mesh, fs, True, True, passes)
    old = _cycles(ctx, mesh, fs, False, True, passes)
    print("CG iterations per solve:", new["its"], old["its"], "passes (matrix, rhs only, products):", new["passes"], old["passes"])
    for key in ("u", "g"):
        e2, em = _rel2(new[key], old[key]), _relmax(new[key], old[key])
        print(f"{key}: reuse vs walk {e2:.2e} (2-norm) {em:.2e} (max norm)")
        assert e2 < TOL and em < TOL
    assert abs(new["J"] - old["J"]) <= TOL * abs(old["J"])
    # three Newton iterations and an adjoint solve on both paths, the same CG counts in each
    assert len(new["its"]) == 4 and new["its"] == old["its"]
    for key, rkey in (("u", "u"), ("g", "grad")):
        e = _relmax(new[key], ref[rkey])
        print(f"{key}: reuse vs oracle {e:.2e}")
        assert e < TOL
    assert abs(new["J"] - ref["J"][0]) <= TOL * abs(ref["J"][0])
    # the walk: Newton's three A + rhs passes and its last residual, and the early dR/du + A pass
    assert old["passes"] == (4, 1, 0)


def test_one_assembly_pass_per_cycle(ctx, problem, monkeypatch):
    mesh, fs, _ = problem
    passes = _Passes(monkeypatch)
    early = _cycles(ctx, mesh, fs, True, True, passes)
    late = _cycles(ctx, mesh, fs, True, False, passes)
    print("passes (matrix, rhs only, products): early", early["passes"], "late", late["passes"])
    assert early["passes"] == (1, 0, 4)          # StateOperation's linearisation serves Newton and the adjoint
    assert late["passes"] == (2, 0, 4)           # Newton's own, then compute_derivatives'
    assert early["its"] == late["its"]
    assert _rel2(early["u"], late["u"]) < TOL and _rel2(early["g"], late["g"]) < TOL


def test_from_the_default_state(ctx, problem, monkeypatch):
    """From u = 1 (CSDL's default state value) the first correction is O(1) and the second Newton solve does real work."""
    mesh, fs, ref = problem
    passes = _Passes(monkeypatch)
    new = _cycles(ctx, mesh, fs, True, True, passes, start=1.0)
    old = _cycles(ctx, mesh, fs, False, True, passes, start=1.0)
    print("CG iterations per solve:", new["its"], old["its"])
    assert len(new["its"]) == 4 and new["its"][1] > 0
    assert new["its"] == old["its"]
    e2, em = _rel2(new["u"], old["u"]), _relmax(new["u"], old["u"])
    print(f"u: reuse vs walk {e2:.2e} (2-norm) {em:.2e} (max norm); vs oracle {_relmax(new['u'], ref['u']):.2e}")
    assert e2 < TOL and em < TOL
    assert _relmax(new["u"], ref["u"]) < TOL
    assert new["passes"] == (1, 0, 4)


def test_a_form_without_constant_partials_is_untouched(ctx, monkeypatch):
    """Nonlinear Poisson: a pass with the Jacobian per Newton iteration, whatever `linear_reuse` says, and no product."""
    from bench import build_problem_nl
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitSquareMesh
    utils_hip.set_context(ctx)
    passes = _Passes(monkeypatch)
    mesh = createUnitSquareMesh(16)
    xc = mesh.centroids()
    f = 0.1 * (1.0 + 0.2 * np.sin(np.pi * xc[:, 0]) * xc[:, 1])
    seen = {}
    base = utils_hip._NewtonBase
    reuse0 = base.linear_reuse
    try:
        for reuse in (True, False):
            base.linear_reuse = reuse
            sim, fea = build_problem_nl(mesh)
            ufn = fea.states_dict['u']['function']
            for k in range(2):
                passes.take()
                del utils_hip.LAST_KSP_INFO[:]
                sim['f'] = E.pinned_array(f)
                ufn.vector.set(1.0)
                sim['u'] = E.pinned_full(mesh.n_vert, 1.0)
                sim.run()
                sim.compute_totals('l2_functional', 'f')
            newton_solves = len(utils_hip.LAST_KSP_INFO) - 1               # all but the adjoint solve
            seen[reuse] = (passes.take(), newton_solves)
            utils_hip.clear_workspaces()
    finally:
        base.linear_reuse = reuse0
    print("passes (matrix, rhs only, products), Newton solves:", seen)
    assert seen[True] == seen[False]
    (matrix, rhs_only, products), solves = seen[True]
    # a Jacobian with the first residual and with each one after an iteration, and the linearisation of compute_derivatives
    assert solves >= 2 and products == 0 and rhs_only == 0 and matrix == solves + 1 + 1
