"""Tapered ranges of the streamed head and tail (csrc/range_plan.h): the pieces of f's chunked upload shrink towards its end,
the ranges of the streamed gradient grow from its start.

Every case compares against THE SAME CALL with chunk = 0 (FEMO_H2D_CHUNK_MB=0 / FEMO_D2H_CHUNK_MB=0: one copy and the single
launches) with np.array_equal on uint64 views: whatever the plan, the ranges run the same kernels on the same rows and cells,
so the bits are the same and no tolerance is involved (tests/test_gpu_streamed_head.py, tests/test_gpu_streamed_tail.py).
The arrays are theirs (n = 56 cube: 1,053,696 cells; the cube less its last cell; the 725^2 square; the randomly numbered
cube); chunks of 1 MiB with a floor of 1/8 MiB and a factor of 2 give three taper steps at either end, and the download's
ranges grow on to 2 MiB.  The number of ranges the library reports is the host plan's (femo_range_plan_host).

The one BPX cycle (n = 32, 196,608 cells in chunks of 1/4 MiB tapering to 1/32 MiB) is held to 8 x max(distance of two plain
runs, 2.3e-16) in the relative maximum norm, the bound of the streamed tail's and the compacted product's BPX cases: the
preconditioner's atomics make two runs of the same cycle differ in the last bits by themselves."""
import os
import types

import numpy as np
import pytest

from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

MIB = 131072
CHUNK, FLOOR, FACTOR, CAP = "1", "0.125", "2", "2"
_ENV = ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB", "FEMO_D2H_CHUNK_MB", "FEMO_D2H_ON_DEMAND", "FEMO_D2H_PROMISE_OUTPUTS",
        "FEMO_RANGE_FLOOR_MB", "FEMO_RANGE_FACTOR", "FEMO_D2H_MAX_CHUNK_MB")
_MESHES, _HEAD, _TAIL, _PROBLEMS = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    pc = utils_hip.KSP_OPTIONS["pc"]
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    _PROBLEMS.clear(); _HEAD.clear(); _TAIL.clear(); _MESHES.clear()
    utils_hip.clear_workspaces()
    for k in _ENV:
        os.environ.pop(k, None)
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def _taper(chunk_h2d, chunk_d2h, floor=FLOOR, factor=FACTOR, cap=CAP):
    os.environ.update(FEMO_H2D_CHUNK_MB=chunk_h2d, FEMO_D2H_CHUNK_MB=chunk_d2h, FEMO_RANGE_FLOOR_MB=floor, FEMO_RANGE_FACTOR=factor,
                      FEMO_D2H_MAX_CHUNK_MB=cap)


def _plan(n, chunk_mb, taper, floor=FLOOR, factor=FACTOR, cap=CAP):
    from femo_amd import _lib
    e = lambda mb: int(float(mb) * MIB)
    return _lib.load().femo_range_plan_host(n, e(chunk_mb), taper, e(floor), int(factor), e(cap), None, 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mesh(name):
    if name not in _MESHES:
        from femo_amd.fea.mesh import Mesh, createUnitCubeMesh, createUnitSquareMesh
        if name == "square":
            m = createUnitSquareMesh(725)
        elif name == "small":
            m = createUnitCubeMesh(32)
        elif name == "odd":
            full = createUnitCubeMesh(56)
            m = Mesh(full.x, full.conn[:-1], full.n)
        elif name == "permuted":
            m = createUnitCubeMesh(56).permuted(seed=3)
        else:
            m = createUnitCubeMesh(56)
        _MESHES[name] = m
    return _MESHES[name]


def _head(ctx, name):
    """femo_newton_rhs_linear with f on its way: operator, a random state off the Dirichlet values, one f; the one-copy result."""
    if name not in _HEAD:
        from femo_amd import engine as E
        mesh = _mesh(name)
        dm = mesh.device(ctx)
        rng = np.random.default_rng(17)
        bd = fo.boundary_vertices_box(mesh.x)
        ds = E.DirichletSet(dm, bd, 0.3 + 0.1 * rng.standard_normal(len(bd)))
        U, F, B = E.Vec(ctx, mesh.n_vert).set(rng.standard_normal(mesh.n_vert)), E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_vert)
        F.set(np.zeros(mesh.n_cell))
        K, A = E.Mat(dm), E.Mat(dm)
        E.assemble_system(dm, 0, None, U, F, ds, K, A, None)
        c = types.SimpleNamespace(mesh=mesh, dm=dm, ds=ds, U=U, F=F, B=B, K=K, A=A, f=rng.standard_normal(mesh.n_cell))
        _taper("0", "0")
        c.one = _rhs(c)
        assert c.one.st["h2d_deferred"] == 1 and c.one.st["h2d_chunks"] == 1
        _HEAD[name] = c
    return _HEAD[name]


def _rhs(c):
    from femo_amd import engine as E
    f_host = E.pinned_array(c.f)
    E.host_stats(reset=True)
    before = c.dm.head_info()["streamed"]
    with E.deferred_uploads():
        c.F.set(f_host)
        E.newton_rhs_linear(c.K, c.F, c.U, c.ds, c.B)
    return types.SimpleNamespace(b=np.array(c.B.get()), st=E.host_stats(), streamed=c.dm.head_info()["streamed"] - before)


def _tail(ctx, name):
    """host += (dR/df)^T X into the pinned copy of a random explicit gradient G; the unchunked result."""
    if name not in _TAIL:
        from femo_amd import engine as E
        mesh = _mesh(name)
        dm = mesh.device(ctx)
        rng = np.random.default_rng(23)
        CV, X, G, Y = E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_vert), E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_cell)
        E.assemble_dRdf_cell(dm, 0, None, CV)
        X.set(rng.standard_normal(mesh.n_vert))
        G.set(rng.standard_normal(mesh.n_cell) * 1e-3)
        c = types.SimpleNamespace(mesh=mesh, dm=dm, CV=CV, X=X, G=G, Y=Y, n=mesh.n_cell)
        _taper("0", "0")
        c.one = _down(c)
        assert c.one.did == dict(streamed=0, ranges=0, plain=1)
        _TAIL[name] = c
    return _TAIL[name]


def _down(c):
    from femo_amd import engine as E
    w = E.writable(c.G.get(), announce=False)
    before = c.dm.tail_info()
    E.host_stats(reset=True)
    E.dRdf_cell_apply_T_add_to_host(c.dm, c.CV, c.X, c.Y, w, c.n)
    after = c.dm.tail_info()
    return types.SimpleNamespace(g=np.array(w, copy=True), st=E.host_stats(), did={k: after[k] - before[k] for k in after})


@pytest.mark.parametrize("name", ["cube", "odd", "square", "permuted"])
def test_tapered_head_is_bit_equal(ctx, name):
    c = _head(ctx, name)
    _taper(CHUNK, CHUNK)
    many = _rhs(c)
    want = _plan(c.mesh.n_cell, CHUNK, 1)
    print(f"{name}: {many.st['h2d_chunks']} copies (host plan {want}, equal pieces {_plan(c.mesh.n_cell, CHUNK, 0)}), "
          f"max |b - b0| {np.abs(many.b - c.one.b).max():.3e}")
    assert many.st["h2d_deferred"] == 1 and many.st["h2d_chunks"] == want and want > _plan(c.mesh.n_cell, CHUNK, 0) == 9
    assert many.streamed == 1 and c.one.streamed == 0
    assert np.array_equal(_bits(many.b), _bits(c.one.b))


@pytest.mark.parametrize("name", ["cube", "odd", "square", "permuted"])
def test_tapered_tail_is_bit_equal(ctx, name):
    c = _tail(ctx, name)
    _taper(CHUNK, CHUNK)
    many = _down(c)
    want = _plan(c.n, CHUNK, 2)
    print(f"{name}: {many.did} (host plan {want}), max |g - g0| {np.abs(many.g - c.one.g).max():.3e}")
    assert many.did == dict(streamed=1, ranges=want, plain=0) and 1 < want < 9
    assert many.st["d2h_device_sum"] == 1 and many.st["d2h_device_sum_bytes"] == 8 * c.n and many.st["d2h_async"] == 0
    assert np.array_equal(_bits(many.g), _bits(c.one.g))
    # no growth beyond the chunk, and a factor of 4: other plans, the same bits
    for cap, factor in ((CHUNK, FACTOR), (CAP, "4")):
        _taper(CHUNK, CHUNK, cap=cap, factor=factor)
        other = _down(c)
        assert other.did == dict(streamed=1, ranges=_plan(c.n, CHUNK, 2, cap=cap, factor=factor), plain=0)
        assert np.array_equal(_bits(other.g), _bits(c.one.g))


def test_default_floor_leaves_the_equal_pieces_of_small_chunks(ctx):
    """The library's default floor (8 MiB) is above these chunks: nine equal pieces either way, as before."""
    h, t = _head(ctx, "cube"), _tail(ctx, "cube")
    for k in ("FEMO_RANGE_FLOOR_MB", "FEMO_RANGE_FACTOR", "FEMO_D2H_MAX_CHUNK_MB"):
        os.environ.pop(k, None)
    os.environ.update(FEMO_H2D_CHUNK_MB=CHUNK, FEMO_D2H_CHUNK_MB=CHUNK)
    up, down = _rhs(h), _down(t)
    assert up.st["h2d_chunks"] == 9 and down.did == dict(streamed=1, ranges=9, plain=0)
    assert np.array_equal(_bits(up.b), _bits(h.one.b)) and np.array_equal(_bits(down.g), _bits(t.one.g))


def _bpx_cycle(p, f_host):
    from bench import one_cycle
    from femo_amd import engine as E
    E.host_stats(reset=True)
    before = p.dm.tail_info()
    g = one_cycle(p.sim, p.fea, f_host, E.pinned_full(p.mesh.n_vert, 0.0))
    after = p.dm.tail_info()
    return types.SimpleNamespace(u=np.array(E.host_wait(p.sim['u']), copy=True), g=np.array(E.host_wait(g), copy=True),
                                 J=float(np.asarray(p.sim['l2_functional']).ravel()[0]), st=E.host_stats(),
                                 did={k: after[k] - before[k] for k in after})


def test_bpx_cycle_over_tapered_ranges(ctx):
    from bench import build_problem, source_fields
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    utils_hip.KSP_OPTIONS["pc"] = "bpx"
    mesh = _mesh("small")
    sim, fea = build_problem(mesh, device=False)
    p = types.SimpleNamespace(mesh=mesh, sim=sim, fea=fea, dm=mesh.device(ctx))
    fs = source_fields(mesh, 2)
    _taper("0", "0")
    _bpx_cycle(p, E.pinned_array(fs[0]))                 # builds the lattice, warms the pool
    a, b = _bpx_cycle(p, E.pinned_array(fs[1])), _bpx_cycle(p, E.pinned_array(fs[1]))
    _taper("0.25", "0.25", floor="0.03125", cap="0.5")
    c = _bpx_cycle(p, E.pinned_array(fs[1]))
    utils_hip.KSP_OPTIONS["pc"] = "jacobi"
    assert a.did == dict(streamed=0, ranges=0, plain=1)
    assert c.did == dict(streamed=1, ranges=_plan(mesh.n_cell, "0.25", 2, floor="0.03125", cap="0.5"), plain=0) and c.did["ranges"] > 1
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    for what, x, y, z in (("u", c.u, a.u, b.u), ("dJ/df", c.g, a.g, b.g), ("J", np.array([c.J]), np.array([a.J]), np.array([b.J]))):
        plain, tapered = rel(z, y), rel(x, y)
        print(f"{what}: tapered - plain {tapered:.2e}, plain - plain {plain:.2e}")
        assert tapered <= 8 * max(plain, 2.3e-16), what
