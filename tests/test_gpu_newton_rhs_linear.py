"""femo_newton_rhs_linear: the Newton right-hand side of the linear Poisson form from its assembled operator,
b = K u' - L outside the Dirichlet set (u' = u with g on the set), b = u - g on it -- one SELL-64 product with the
rest in its epilogue -- against the NumPy oracle and against the pass over the mesh it replaces."""
import numpy as np
import pytest

from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

RTOL = 1e-12          # relative, max norm: the bar of the existing newton_rhs parity tests

CASES = ["cube6_jittered", "cube2", "square9", "cube12_structured", "cube12_reordered", "cube36_reordered"]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _mesh(name):
    from femo_amd.fea.mesh import createUnitCubeMesh, createUnitSquareMesh
    if name == "cube6_jittered":
        return createUnitCubeMesh(6, jitter=0.2)            # 343 rows: 6 slices, the last one ragged
    if name == "cube2":
        return createUnitCubeMesh(2, jitter=0.2)            # 27 rows: less than one slice
    if name == "square9":
        return createUnitSquareMesh(9, jitter=0.2)
    base = createUnitCubeMesh(12, jitter=0.0)               # structured numbering: regular slices
    if name == "cube12_structured":
        return base
    if name == "cube12_reordered":
        return base.permuted(seed=5).reordered()            # Morton numbering: 16-bit deltas (2,197 rows: every delta fits)
    # 50,653 rows: deltas beyond 16 bits appear, so the Morton numbering has slices of 16-bit deltas AND of 32-bit columns
    return createUnitCubeMesh(36, jitter=0.0).permuted(seed=5).reordered()


_CACHE = {}


def _case(ctx, name):
    """Everything the tests of one mesh share, computed once: inputs, the oracle's right-hand side and residual, the walk's
    and the product's results."""
    if name in _CACHE:
        return _CACHE[name]
    from femo_amd import engine as E
    mesh = _mesh(name)
    om = fo.OMesh(mesh.tdim, mesh.x, mesh.conn)
    dm = E.DeviceMesh(ctx, mesh.x, mesh.conn)
    rng = np.random.default_rng(11)
    u, f = rng.standard_normal(mesh.n_vert), rng.standard_normal(mesh.n_cell)
    bd = fo.boundary_vertices_box(mesh.x)
    g = 0.3 + 0.1 * rng.standard_normal(len(bd))                        # non-zero Dirichlet values
    U, F = E.Vec(ctx, mesh.n_vert).set(u), E.Vec(ctx, mesh.n_cell).set(f)
    ds = E.DirichletSet(dm, bd, g)
    K, A = E.Mat(dm), E.Mat(dm)
    E.assemble_system(dm, 0, None, U, F, ds, K, A, None)                # the one dR/du + A pass
    B = E.Vec(ctx, mesh.n_vert)
    c = dict(info=dm.info, n=mesh.n_vert)
    c["prod"] = np.array(E.newton_rhs_linear(K, F, U, ds, B).get())
    c["prod_nobc"] = np.array(E.newton_rhs_linear(K, F, U, None, B).get())
    A2 = E.Mat(dm)
    E.assemble_system(dm, 0, None, U, F, ds, None, A2, B)
    c["walk"] = np.array(B.get())
    c["walk_nobc"] = np.array(E.assemble_residual(dm, 0, None, U, F, B).get())
    R = fo.residual(om, u, f)
    c["ref"] = fo.newton_rhs(fo.stiffness(om), R, u, bd, g)
    c["ref_nobc"] = R
    _CACHE[name] = c
    return c


@pytest.mark.parametrize("name", CASES)
def test_product_matches_the_oracle(ctx, name):
    c = _case(ctx, name)
    info = c["info"]
    if name == "cube12_structured":
        assert info["regular_slices"] > 0
    if name == "cube12_reordered":
        assert info["regular_slices"] == 0 and info["short_slices"] == info["n_slices"]        # 16-bit deltas throughout
    if name == "cube36_reordered":
        assert info["regular_slices"] == 0 and 0 < info["short_slices"] < info["n_slices"]     # both other classes
    if name == "cube2":
        assert c["n"] < 64
    if name == "cube6_jittered":
        assert info["n_slices"] <= 6 and c["n"] % 64 != 0
    e, e0 = _rel(c["prod"], c["ref"]), _rel(c["prod_nobc"], c["ref_nobc"])
    print(f"{name}: product vs oracle {e:.2e} (with the set), {e0:.2e} (bc = None)")
    assert e < RTOL and e0 < RTOL


@pytest.mark.parametrize("name", CASES)
def test_product_equals_the_walk(ctx, name):
    c = _case(ctx, name)
    e, e0 = _rel(c["prod"], c["walk"]), _rel(c["prod_nobc"], c["walk_nobc"])
    print(f"{name}: product vs walk {e:.2e} (with the set), {e0:.2e} (bc = None)")
    assert e < RTOL and e0 < RTOL


def test_the_call_invalidates_host_copies_of_b(ctx):
    """A host array handed out for b mirrors it until the entry point writes b: the upload after the call must be real."""
    import os
    from femo_amd import engine as E
    from femo_amd.fea.mesh import createUnitSquareMesh
    mesh = createUnitSquareMesh(6, jitter=0.1)
    dm = mesh.device(ctx)
    n, nc = mesh.n_vert, mesh.n_cell
    rng = np.random.default_rng(5)
    u, f, r = E.Vec(ctx, n), E.Vec(ctx, nc), E.Vec(ctx, n)
    u.set(rng.standard_normal(n)); f.set(rng.standard_normal(nc))
    bd = fo.boundary_vertices_box(mesh.x)
    ds = E.DirichletSet(dm, bd, np.zeros(len(bd)))
    A, K = E.Mat(dm), E.Mat(dm)
    E.assemble_system(dm, 0, None, u, f, ds, K, A, None)

    def writes(vec, fn):
        marker = np.full(vec.n, 7.25)
        vec.set(marker)
        h = vec.get()                                   # mirrors vec
        fn()                                            # device-side write
        after = np.array(vec.get())
        vec.set(h)                                      # must really upload (FEMO_HOST_VERIFY would also catch a wrong skip)
        assert np.array_equal(vec.get(), marker), fn
        return after

    old = os.environ.get("FEMO_HOST_VERIFY")
    os.environ["FEMO_HOST_VERIFY"] = "1"
    try:
        after = writes(r, lambda: E.newton_rhs_linear(K, f, u, ds, r))
        assert not np.array_equal(after, np.full(n, 7.25))
        writes(r, lambda: E.newton_rhs_linear(K, f, u, None, r))
    finally:
        if old is None:
            os.environ.pop("FEMO_HOST_VERIFY", None)
        else:
            os.environ["FEMO_HOST_VERIFY"] = old


def test_two_emulated_ranks_equal_one(ctx):
    """Partitioned mesh: the ghosts of u are refreshed, then the product runs over the owned rows with ghost columns read in
    place.  Owned rows of both ranks against the one-rank result."""
    from femo_amd import engine as E
    from femo_amd.dist.partition import build_local_mesh, rcb_partition
    from test_gpu_emulated_ranks import _run_ranks, _set_halo
    one = _case(ctx, "cube12_structured")
    mesh = _mesh("cube12_structured")
    rng = np.random.default_rng(11)                                     # the inputs of _case
    u, f = rng.standard_normal(mesh.n_vert), rng.standard_normal(mesh.n_cell)
    bd_g = fo.boundary_vertices_box(mesh.x)
    g_global = np.zeros(mesh.n_vert)
    g_global[bd_g] = 0.3 + 0.1 * rng.standard_normal(len(bd_g))
    world = 2
    part = rcb_partition(mesh.x, world)

    def rank_fn(rank, rctx):
        L = build_local_mesh(mesh.x, mesh.conn, part, rank, world)
        dm = E.DeviceMesh(rctx, L.x, L.conn, n_rows=L.n_owned)
        dm.set_global(mesh.x.min(axis=0), mesh.x.max(axis=0), mesh.n_vert)
        _set_halo(rctx, dm, L)
        nloc = len(L.x)
        ul = np.full(nloc, 1e30)                                        # ghosts hold garbage until the exchange
        ul[:L.n_owned] = u[L.vert_global[:L.n_owned]]
        U, F = E.Vec(rctx, nloc).set(ul), E.Vec(rctx, len(L.conn)).set(f[L.cell_global])
        bd = fo.boundary_vertices_box(L.x)                              # local indices, owned and ghost
        ds = E.DirichletSet(dm, bd, g_global[L.vert_global[bd]])
        K, A, B = E.Mat(dm), E.Mat(dm), E.Vec(rctx, nloc)
        E.assemble_system(dm, 0, None, U, F, ds, K, A, None)
        b = np.array(E.newton_rhs_linear(K, F, U, ds, B).get(L.n_owned))
        b0 = np.array(E.newton_rhs_linear(K, F, U, None, B).get(L.n_owned))
        return dict(gid=L.vert_global[:L.n_owned], b=b, b0=b0)

    res = _run_ranks(world, rank_fn)
    b, b0 = np.full(mesh.n_vert, np.nan), np.full(mesh.n_vert, np.nan)
    for r in res:
        b[r["gid"]] = r["b"]
        b0[r["gid"]] = r["b0"]
    e, e0 = _rel(b, one["prod"]), _rel(b0, one["prod_nobc"])
    print(f"two ranks vs one: {e:.2e} (with the set), {e0:.2e} (bc = None)")
    assert e < RTOL and e0 < RTOL
