"""Newton's flagged passes (DESIGN_LOG R18): a pass that does not solve leaves dx = 0 off the Dirichlet rows and u_i - g_i on
them; femo_mat_identity_solve_flag raises a device-side flag when an entry of dx is anything but +0.0, and the update of u
and the product of the next right-hand side are handed that flag and leave early while it is down.

Every case is compared with THE SAME CALL under FEMO_NEWTON_FLAG=0 (the plain launches) bit for bit -- the right-hand side
after every pass, the state, the norms, the iteration counts and every field of the solve records but the timings -- and
the library is asked what the flagged launches did (Context.newton_flag_info, femo_ctx_newton_flag_info of femo_hip_test.h).
Bits are compared with the Jacobi-preconditioned CG: the BPX preconditioner accumulates its brick restriction with fp64
atomics and two runs of the same cycle differ in the last bits by themselves (tests/test_gpu_streamed_head.py); one case
runs the BPX cycle bench.py measures and holds it to the distance of two plain runs.

Which rule ends Newton's passes 2 and 3 depends on the mesh (tests/test_gpu_round6.py): a noise factor of 1e7, the same
in both runs, puts these small meshes on the rule Newton evaluates itself, as the 10 M-DOF cube is."""
import os
import threading
import types

import numpy as np
import pytest

import wide_meshes as W
from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

TIMINGS = ("thread", "solve_ms", "spmv_ms")
_MESHES = {}


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in ("FEMO_NEWTON_FLAG", "FEMO_HOST_VERIFY")}
    pc, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], "jacobi"
    noise, utils_hip._NewtonBase.NOISE_FACTOR = utils_hip._NewtonBase.NOISE_FACTOR, 1e7
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    utils_hip._NewtonBase.NOISE_FACTOR = noise
    _MESHES.clear()
    utils_hip.clear_workspaces()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _mesh(name):
    if name not in _MESHES:
        from femo_amd.fea.mesh import Mesh, createUnitCubeMesh, createUnitSquareMesh
        if name == "cube8":
            m = createUnitCubeMesh(8)
        elif name == "cube12":
            m = createUnitCubeMesh(12, jitter=0.2)
        elif name == "square32":
            m = createUnitSquareMesh(32)
        else:                                           # rows of 18 entries: beyond the pipelined residual's 16
            m = Mesh(*W.cube5(8))
        _MESHES[name] = m
    return _MESHES[name]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _source(mesh):
    xc = mesh.centroids()
    return np.sin(np.pi * xc[:, 0]) * np.sin(np.pi * xc[:, 1]) * (0.5 + 0.3 * np.cos(2 * np.pi * xc[:, 0]) + 0.2 * xc[:, -1])


def _newton(ctx, monkeypatch, mesh, u0, g, flag, between=None):
    """One Newton solve of the linear Poisson form from u0 with the value g on the box boundary.  between(k, u, b): called
    after the k-th right-hand side (1-based) with the device vectors."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip as U
    from femo_amd.fea.fea_hip import Function, FunctionSpace
    from femo_amd.fea.forms import PoissonResidual
    os.environ["FEMO_NEWTON_FLAG"] = "1" if flag else "0"
    Vf, Vu = FunctionSpace(mesh, ('DG', 0)), FunctionSpace(mesh, ('CG', 1))
    f, u = Function(Vf), Function(Vu)
    f.vector[:] = _source(mesh)
    u.vector[:] = u0
    bd = fo.boundary_vertices_box(mesh.x)
    bc = U.dirichletbc(float(g), bd, Vu)
    solver = U.NewtonSolver(PoissonResidual(u, f), u, [bc])
    passes = []
    plain = E.newton_rhs_linear

    def spy(K, f_, u_, bc_, b, flagged=False):
        plain(K, f_, u_, bc_, b, flagged=flagged)
        passes.append(np.array(b.get(), copy=True))
        if between is not None:
            between(len(passes), u_, b)
        return b

    monkeypatch.setattr(E, "newton_rhs_linear", spy)
    before = np.array(ctx.newton_flag_info())
    del U.LAST_KSP_INFO[:]
    try:
        solver.solve(u)
    finally:
        monkeypatch.setattr(E, "newton_rhs_linear", plain)
    count = np.array(ctx.newton_flag_info()) - before
    infos = [{k: v for k, v in d.items() if k not in TIMINGS} for d in U.LAST_KSP_INFO]
    return types.SimpleNamespace(b=passes, u=np.array(u.vector.getArray(), copy=True), norms=list(solver.residual_norms),
                                 its=list(solver.ksp_iterations), iterations=solver.iterations, infos=infos,
                                 skipped=[bool(d.get("skipped_by_newton")) for d in infos],
                                 left=(int(count[0]), int(count[2])), ran=(int(count[1]), int(count[3])), handed=int(count[4]))


def _same_solve(new, old, what):
    print(f"{what}: CG iterations {new.its} / {old.its}, skipped by Newton {new.skipped}, flagged launches (axpy, product) "
          f"left early {new.left}, ran {new.ran}, handed the flag {new.handed}; norms {new.norms}")
    assert len(new.b) == len(old.b) == 4
    for k, (x, y) in enumerate(zip(new.b, old.b)):
        assert _same_bits(x, y), f"{what}: right-hand side of pass {k + 1}"
    assert _same_bits(new.u, old.u), what
    assert _same_bits(new.norms, old.norms) and new.its == old.its and new.iterations == old.iterations, what
    assert len(new.infos) == len(old.infos)
    for a, b in zip(new.infos, old.infos):
        assert a.keys() == b.keys()
        for k in a:
            assert _same_bits([a[k]], [b[k]]), f"{what}: record field {k}"
    assert old.handed == 0 and old.left == (0, 0) and old.ran == (0, 0)      # FEMO_NEWTON_FLAG=0: the plain launches
    # every launch that was handed the flag either left or ran, and nothing else was counted
    assert new.left[0] + new.ran[0] + new.left[1] + new.ran[1] == new.handed


def _both(ctx, monkeypatch, name, u0, g, what, between=None):
    mesh = _mesh(name)
    start = np.full(mesh.n_vert, float(u0)) if np.isscalar(u0) else u0
    old = _newton(ctx, monkeypatch, mesh, start, g, False, between)
    new = _newton(ctx, monkeypatch, mesh, start, g, True, between)
    _same_solve(new, old, f"{name}, {what}")
    return new


@pytest.mark.parametrize("name", ["cube8", "cube12", "square32"])
def test_state_on_its_boundary_values_skips_both_passes(ctx, monkeypatch, name):
    new = _both(ctx, monkeypatch, name, 0.0, 0.0, "u0 = 0, g = 0")
    assert new.its[0] > 0 and new.skipped == [False, True, True]
    assert new.left == (2, 2) and new.ran == (0, 0)


@pytest.mark.parametrize("name", ["cube8", "cube12", "square32"])
def test_rounded_boundary_value_raises_the_flag_once(ctx, monkeypatch, name):
    """1 - (1 - 0.3) is not 0.3: the first pass that does not solve still moves the Dirichlet rows by one rounding."""
    assert 1.0 - (1.0 - 0.3) != 0.3
    new = _both(ctx, monkeypatch, name, 1.0, 0.3, "u0 = 1, g = 0.3")
    assert new.ran[0] >= 1 and new.ran[1] >= 1
    assert new.handed == 2 * sum(new.skipped)


@pytest.mark.parametrize("name", ["cube8", "square32"])
def test_second_pass_that_solves_gets_no_flag(ctx, monkeypatch, name):
    """Far from the solution, a first solve to 1e-3 only and the threshold of the second pass back at 1e-14 of the first
    right-hand side: the second pass iterates, and the update and the product behind a real solve are never handed the flag.
    The third pass, with the threshold at 1e-3 again, does not solve and is handed it.  (Newton copies the solver's options
    when it starts and reads the threshold's factor at every pass: the solves keep rtol = 1e-3 throughout.)"""
    from femo_amd.fea import utils_hip as U
    mesh = _mesh(name)
    u0 = 1.0 + np.random.default_rng(5).standard_normal(mesh.n_vert)
    monkeypatch.setattr(U._NewtonBase, "NOISE_FACTOR", 0.0)
    monkeypatch.setitem(U.KSP_OPTIONS, "rtol", 1e-3)

    def thresholds(k, u, b):
        U.KSP_OPTIONS["rtol"] = {2: 1e-14, 3: 1e-3}.get(k, U.KSP_OPTIONS["rtol"])

    def reset(k, u, b):
        if k == 1:
            U.KSP_OPTIONS["rtol"] = 1e-3                # (each of the two runs starts from the same options)
        thresholds(k, u, b)

    new = _both(ctx, monkeypatch, name, u0, 0.3, "u0 = 1 + noise, rtol 1e-3 / 1e-14 / 1e-3", reset)
    assert new.its[0] > 0 and new.its[1] > 0 and new.skipped == [False, False, True]
    assert new.handed == 2 and new.left[0] + new.ran[0] == 1 and new.left[1] + new.ran[1] == 1


def test_passes_left_to_the_solver_get_no_flag(ctx, monkeypatch):
    """newton_probe = False leaves the decision not to iterate to the solver: every pass goes through it, none is flagged."""
    from femo_amd.fea import utils_hip as U
    monkeypatch.setattr(U._NewtonBase, "newton_probe", False)
    new = _both(ctx, monkeypatch, "cube8", 0.0, 0.0, "u0 = 0, g = 0, no probe")
    assert new.skipped == [False, False, False] and new.handed == 0


def _engine_case(ctx, name):
    from femo_amd import engine as E
    mesh = _mesh(name)
    dm = mesh.device(ctx)
    rng = np.random.default_rng(23)
    bd = fo.boundary_vertices_box(mesh.x)
    g = np.zeros(len(bd))
    g[1::2] = 0.3 + 0.1 * rng.standard_normal(len(g[1::2]))
    ds = E.DirichletSet(dm, bd, g)
    F = E.Vec(ctx, mesh.n_cell).set(_source(mesh))
    U, B, DX = (E.Vec(ctx, mesh.n_vert).fill(0.0) for _ in range(3))
    K, A = E.Mat(dm), E.Mat(dm)
    E.assemble_system(dm, 0, None, U, F, ds, K, A, None)
    u = rng.standard_normal(mesh.n_vert)
    u[bd] = g                                            # on its boundary values, exactly
    return types.SimpleNamespace(E=E, mesh=mesh, ds=ds, F=F, U=U, B=B, DX=DX, K=K, A=A, u=u, bd=bd, g=g)


def _engine_pass(ctx, c, u_host, flag, between=None):
    """right-hand side, identity solve, update, right-hand side -- Newton's pass that does not solve, entry point by entry point"""
    E = c.E
    c.U.set(u_host)
    before = np.array(ctx.newton_flag_info())
    E.newton_rhs_linear(c.K, c.F, c.U, c.ds, c.B)
    b0 = np.array(c.B.get(), copy=True)
    c.A.identity_solve(c.B, c.DX, flagged=flag)
    if between is not None:
        between(c)
    c.U.axpy(-1.0, c.DX, flagged=flag)
    E.newton_rhs_linear(c.K, c.F, c.U, c.ds, c.B, flagged=flag)
    out = types.SimpleNamespace(b0=b0, b=np.array(c.B.get(), copy=True), u=np.array(c.U.get(), copy=True),
                                dx=np.array(c.DX.get(), copy=True))
    count = np.array(ctx.newton_flag_info()) - before
    out.left, out.ran, out.handed = (int(count[0]), int(count[2])), (int(count[1]), int(count[3])), int(count[4])
    return out


def _engine_both(ctx, c, u_host, what, between=None):
    old, new = _engine_pass(ctx, c, u_host, False, between), _engine_pass(ctx, c, u_host, True, between)
    print(f"{what}: left early {new.left}, ran {new.ran}, handed the flag {new.handed}")
    for key in ("b0", "dx", "u", "b"):
        assert _same_bits(getattr(new, key), getattr(old, key)), f"{what}: {key}"
    assert old.handed == 0 and old.left == (0, 0) and old.ran == (0, 0)
    return new


@pytest.mark.parametrize("name", ["cube8", "square32"])
def test_negative_zero_and_nan_count_as_nonzero(ctx, name):
    c = _engine_case(ctx, name)
    clean = _engine_both(ctx, c, c.u, "on the boundary values")
    assert clean.left == (1, 1) and clean.ran == (0, 0) and not _bits(clean.dx).any()
    zero_rows = c.bd[0::2]                               # rows whose prescribed value is +0.0
    u = c.u.copy()
    u[zero_rows[3]] = -0.0                               # -0.0 - +0.0 = -0.0 on that row; the update turns the state's -0.0 into +0.0
    neg = _engine_both(ctx, c, u, "-0.0 on a Dirichlet row")
    assert np.signbit(neg.b0[zero_rows[3]]) and neg.b0[zero_rows[3]] == 0.0 and not np.signbit(neg.u[zero_rows[3]])
    assert neg.left == (0, 0) and neg.ran == (1, 1)
    u = c.u.copy()
    u[c.bd[len(c.bd) // 2]] = np.nan
    nan = _engine_both(ctx, c, u, "NaN on a Dirichlet row")
    assert np.isnan(nan.b0[c.bd[len(c.bd) // 2]]) and np.isnan(nan.u[c.bd[len(c.bd) // 2]])
    assert nan.left == (0, 0) and nan.ran == (1, 1)
    u = c.u.copy()
    u[c.bd[-1]] += 0.25                                  # an ordinary non-zero entry, in the last block of the set
    off = _engine_both(ctx, c, u, "a Dirichlet row off its value")
    assert off.left == (0, 0) and off.ran == (1, 1)


def test_vectors_touched_between_the_passes_get_no_flag(ctx, monkeypatch):
    c = _engine_case(ctx, "cube8")
    E = c.E
    T = E.Vec(ctx, c.mesh.n_vert)

    def rewrite(v):                                      # the same bits through the public API: a new generation
        T.copy_from(v)
        v.copy_from(T)

    # (dx is still the vector the flag describes when b is rewritten: the update leaves early, exactly; the product runs)
    for what, between, left in (("b rewritten", lambda c: rewrite(c.B), (1, 0)), ("u rewritten", lambda c: rewrite(c.U), (0, 0)),
                                ("dx rewritten", lambda c: rewrite(c.DX), (0, 0)), ("nothing rewritten", None, (1, 1))):
        r = _engine_both(ctx, c, c.u, what, between)
        assert r.handed == sum(left) and r.ran == (0, 0) and r.left == left, what
    # another operator content behind the same handle: the right-hand side in place is not this operator's
    r = _engine_both(ctx, c, c.u, "matrix assembled again",
                     lambda c: E.assemble_system(c.mesh.device(ctx), 0, None, c.U, c.F, c.ds, c.K, c.A, None))
    assert r.handed == 1 and r.left == (1, 0)            # the update is still exact; the product runs as the plain one
    # ... and through the Newton solve: u rewritten after the second right-hand side
    mesh = _mesh("cube8")
    touched = _both(ctx, monkeypatch, "cube8", 0.0, 0.0, "u rewritten after pass 2",
                    lambda k, u, b: rewrite(u) if k == 2 else None)
    assert touched.skipped == [False, True, True] and touched.handed == 2 and touched.left == (1, 1)
    assert mesh is _mesh("cube8")


def test_wide_rows_take_the_plain_launches(ctx, monkeypatch):
    mesh = _mesh("wide")
    assert mesh.device(ctx).info["max_rowlen"] == 18
    new = _both(ctx, monkeypatch, "wide", 0.0, 0.0, "u0 = 0, g = 0")
    assert new.skipped == [False, True, True]
    assert new.handed == 0 and new.left == (0, 0) and new.ran == (0, 0)


def _run_ranks(world, fn):
    """fn(rank, ctx) on `world` threads (the harness of tests/test_gpu_emulated_ranks.py)"""
    from femo_amd.dist import ThreadControl
    from femo_amd.engine import Context, EmuGroup
    group = EmuGroup(world)
    shared = ThreadControl.Shared(world)
    out, err = [None] * world, [None] * world

    def body(rank):
        try:
            c = Context(0)
            ThreadControl(rank, shared, group).init_comm(c)
            out[rank] = fn(rank, c)
            c.sync()
        except BaseException as e:          # noqa: BLE001 - reported below, the other ranks time out on their own
            err[rank] = e

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=180)
    assert not any(t.is_alive() for t in threads), "a rank hung"
    for e in err:
        if e is not None:
            raise e
    return out


def test_partitioned_meshes_take_the_plain_launches():
    import bench as B
    from femo_amd.dist import DistMesh
    from femo_amd.dist.partition import build_local_mesh, rcb_partition
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    world, n = 2, 8
    gmesh = createUnitCubeMesh(n, jitter=0.2)
    part = rcb_partition(gmesh.x, world)
    f_global = B.source_fields(gmesh, 1)[0]
    occupancy = gmesh.lattice_occupancy()

    def rank_fn(rank, c):
        utils_hip.set_context(c, thread_local=True)
        try:
            L = build_local_mesh(gmesh.x, gmesh.conn, part, rank, world)
            mesh = DistMesh(L, gmesh.n_vert, gmesh.n_cell, bbox=(gmesh.x.min(axis=0), gmesh.x.max(axis=0)))
            mesh._occupancy = occupancy
            sim, fea = B.build_problem(mesh, device=True)
            g = np.asarray(B.one_cycle(sim, fea, f_global[L.cell_global])).ravel()
            return dict(u=np.array(np.asarray(sim['u'])[:L.n_owned], copy=True), g=g[L.cell_owned].copy(),
                        info=c.newton_flag_info())
        finally:
            utils_hip.set_context(None, thread_local=True)

    runs = {}
    for flag in ("0", "1"):
        os.environ["FEMO_NEWTON_FLAG"] = flag
        runs[flag] = _run_ranks(world, rank_fn)
    for a, b in zip(runs["1"], runs["0"]):
        print("rank: flagged launches", a["info"], "max |u - u0|", np.abs(a["u"] - b["u"]).max())
        assert a["info"][:5] == (0, 0, 0, 0, 0) and a["info"][6] == 0
        assert _same_bits(a["u"], b["u"]) and _same_bits(a["g"], b["g"])


def test_bpx_cycle_through_the_operator_surface(ctx):
    """The cycle bench.py measures, n = 32: BPX-preconditioned CG, NumPy arrays at the boundary.  Two runs of it differ in the
    last bits by themselves (fp64 atomics in the brick restriction), so the flagged cycle is held to that self-distance:
    relative max-norm distance to a plain run within 8 x max(distance of two plain runs, 2.3e-16), the rule of
    test_gpu_pcg_ring.py for the same noise.  The flagged cycle skips both passes, and its solves find the preconditioner's
    weights in place (formed with the prescale); under FEMO_NEWTON_FLAG=0 neither happens."""
    from bench import build_problem, one_cycle, source_fields
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(32)
    fs = source_fields(mesh, 2)
    utils_hip.KSP_OPTIONS["pc"] = "bpx"
    try:
        sim, fea = build_problem(mesh, device=False)

        def cycle(flag, f):
            os.environ["FEMO_NEWTON_FLAG"] = flag
            before = np.array(ctx.newton_flag_info())
            del utils_hip.LAST_KSP_INFO[:]
            g = one_cycle(sim, fea, E.pinned_array(f), E.pinned_full(mesh.n_vert, 0.0))
            r = types.SimpleNamespace(u=np.array(E.host_wait(sim['u']), copy=True), g=np.array(E.host_wait(g), copy=True).ravel(),
                                      J=float(np.asarray(sim['l2_functional']).ravel()[0]),
                                      its=[i["iterations"] for i in utils_hip.LAST_KSP_INFO],
                                      skipped=sum(1 for i in utils_hip.LAST_KSP_INFO if i.get("skipped_by_newton")))
            r.count = np.array(ctx.newton_flag_info()) - before
            return r

        cycle("0", fs[0])                                    # (the first BPX cycle builds the lattice; the second linearises early)
        cycle("0", fs[0])
        a, b, c = cycle("0", fs[1]), cycle("0", fs[1]), cycle("1", fs[1])
    finally:
        utils_hip.KSP_OPTIONS["pc"] = "jacobi"
    print("CG iterations per solve:", a.its, b.its, c.its, "counters plain", a.count, b.count, "flagged", c.count)
    assert not a.count[:5].any() and not b.count[:5].any() and a.count[6] == 0 and b.count[6] == 0
    assert c.its == a.its and len(c.its) == 4
    assert c.skipped == a.skipped == 2
    assert c.count[4] == 4 and c.count[0] == c.count[2] == 2 and c.count[1] == c.count[3] == 0
    assert c.count[6] >= 1
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    for what, x, y, z in (("u", a.u, b.u, c.u), ("dJ/df", a.g, b.g, c.g),
                          ("J", np.array([a.J]), np.array([b.J]), np.array([c.J]))):
        s0, d = rel(x, y), max(rel(z, x), rel(z, y))
        print(f"BPX cycle, {what}: plain against plain {s0:.3e}, flagged against plain {d:.3e}")
        assert d <= 8 * max(s0, 2.3e-16), what
