"""The streamed tail of a cycle: dJ/df += (dR/df)^T psi into the pinned block that still mirrors the explicit dJ/df forms
product, sum and copy-out range by range (femo_dRdf_cell_apply_T_add_to_host, FEMO_D2H_CHUNK_MB).

Every case compares against THE SAME CALL under FEMO_D2H_CHUNK_MB=0 -- the product into a scratch vector followed by
femo_vec_add_to_host, the path of before -- with np.array_equal on uint64 views: the ranged kernel sums the vertices in the
same order, rounds the product and then the sum, so the gradient is the same bits and no tolerance is involved.  The arrays
are those of tests/test_gpu_streamed_head.py (n = 56 cube: 1,053,696 cells; 725^2 square: 1,051,250 cells); chunks of 1 MiB
cut them into 9 ranges.  What ran is asked of the library (DeviceMesh.tail_info, femo_mesh_tail_info of femo_hip_test.h).

The cycles run with the Jacobi-preconditioned CG, for the reason given in tests/test_gpu_streamed_head.py: two BPX cycles
differ in the last bits by themselves.  One case runs the BPX cycle that bench.py measures, n = 32, and holds it to the
distance of two unchunked runs."""
import os
import threading
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB_CHUNK = "1"                      # 131,072 entries per range: 9 ranges of either array
ODD_TAIL = "1.607421875"             # 823 * 256 entries: the 1,053,695 cells of the cube less one leave a last range of 255
_MESHES, _PROBLEMS, _ENGINE = {}, {}, {}
_ENV = ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB", "FEMO_D2H_CHUNK_MB", "FEMO_D2H_ON_DEMAND")


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    pc, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], "jacobi"
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    _PROBLEMS.clear(); _ENGINE.clear(); _MESHES.clear()
    utils_hip.clear_workspaces()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _mesh(name):
    if name in _MESHES:
        return _MESHES[name]
    from femo_amd.fea.mesh import Mesh, createUnitCubeMesh, createUnitSquareMesh
    if name == "square":
        m = createUnitSquareMesh(725)
    elif name == "small":
        m = createUnitCubeMesh(32)
    elif name == "odd":                                # the cube without its last cell: an odd number of cells
        full = createUnitCubeMesh(56)
        m = Mesh(full.x, full.conn[:-1], full.n)
    elif name == "permuted":
        m = createUnitCubeMesh(56).permuted(seed=3)    # random vertex numbering: the gathers of psi are scattered
    else:
        m = createUnitCubeMesh(56)
    _MESHES[name] = m
    return m


def _engine(ctx, name):
    """The entry point on its own: dR/df of the Poisson form, a random multiplier X, a random explicit gradient G."""
    if name not in _ENGINE:
        from femo_amd import engine as E
        mesh = _mesh(name)
        dm = mesh.device(ctx)
        rng = np.random.default_rng(23)
        CV, X, G, Y = E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_vert), E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_cell)
        E.assemble_dRdf_cell(dm, 0, None, CV)
        X.set(rng.standard_normal(mesh.n_vert))
        g = rng.standard_normal(mesh.n_cell) * 1e-3
        G.set(g)
        _ENGINE[name] = types.SimpleNamespace(mesh=mesh, dm=dm, CV=CV, X=X, G=G, Y=Y, g=g, n=mesh.n_cell, ref={})
    return _ENGINE[name]


def _tail(c, chunk, target="mirror", into=None):
    """host += (dR/df)^T X with host = a copy of G: (host, host statistics, what the call did).  target: 'mirror' (the pinned
    array of G.get()), 'pageable', 'plain' (pinned, filled by the caller: mirrors nothing); into: an array to mirror G into first."""
    from femo_amd import engine as E
    if into is not None:
        c.G.get(out=into)                                # a whole pooled block: recorded as the copy of G again
        w = into
    elif target == "mirror":
        w = E.writable(c.G.get(), announce=False)
    elif target == "pageable":
        w = np.array(c.g)
    else:
        w = E.pinned_empty(c.n)
        E.host_copy(w, c.g)
    os.environ["FEMO_D2H_CHUNK_MB"] = chunk
    before = c.dm.tail_info()
    E.host_stats(reset=True)
    syncs = E.host_syncs(reset=True)
    E.dRdf_cell_apply_T_add_to_host(c.dm, c.CV, c.X, c.Y, w, c.n)
    syncs = E.host_syncs()
    after = c.dm.tail_info()
    did = {k: after[k] - before[k] for k in after}
    return types.SimpleNamespace(w=w, g=np.array(w, copy=True), st=E.host_stats(), did=did, syncs=syncs)


def _reference(c):
    """The unchunked call, once per mesh."""
    if "one" not in c.ref:
        one = _tail(c, "0")
        assert one.did == dict(streamed=0, ranges=0, plain=1) and one.st["d2h_device_sum"] == 1
        # the sum itself, against NumPy: the same product and sum, each rounded once (the sum over the vertices in the kernel's order)
        conn = c.mesh.conn
        x = np.array(c.X.get())
        s = np.zeros(c.n)
        for a in range(conn.shape[1]):
            s = s + x[conn[:, a]]
        want = c.g + s * np.array(c.CV.get())
        assert _same_bits(one.g, want)
        c.ref["one"] = one
    return c.ref["one"]


def _streamed(ctx, name, chunk, ranges):
    c = _engine(ctx, name)
    one, many = _reference(c), _tail(_engine(ctx, name), chunk)
    print(f"{name}, chunk {chunk}: {many.did}, host waits {many.syncs} (unchunked {one.syncs}), max |g - g0| {np.abs(many.g - one.g).max():.3e}")
    assert many.did == dict(streamed=1, ranges=ranges, plain=0)
    assert many.st["d2h_device_sum"] == 1 and many.st["d2h_device_sum_bytes"] == 8 * c.n
    assert many.st["d2h_staged"] == 0 and many.st["d2h_pinned"] == 0 and many.st["d2h_async"] == 0
    assert many.syncs <= one.syncs
    assert _same_bits(many.g, one.g)
    return c, many


def test_cube_in_nine_ranges(ctx):
    c, _ = _streamed(ctx, "cube", MIB_CHUNK, 9)
    assert c.n == 1053696


def test_odd_cell_count_leaves_a_255_cell_last_range(ctx):
    c = _engine(ctx, "odd")
    assert c.n % 2 == 1 and c.n - 5 * 823 * 256 == 255
    _streamed(ctx, "odd", ODD_TAIL, 6)
    _streamed(ctx, "odd", MIB_CHUNK, 9)


def test_square_in_nine_ranges(ctx):
    c, _ = _streamed(ctx, "square", MIB_CHUNK, 9)           # the 2-D load_conn on offset pointers: 3 * c0 words
    assert c.mesh.tdim == 2


def test_random_numbering(ctx):
    _streamed(ctx, "permuted", MIB_CHUNK, 9)


def test_chunk_larger_than_the_array_is_one_range(ctx):
    _streamed(ctx, "cube", "16", 1)


def test_same_target_again_reuses_the_events(ctx):
    from femo_amd import engine as E
    c = _engine(ctx, "cube")
    one = _reference(c)
    first = _tail(c, MIB_CHUNK)
    assert first.did["ranges"] == 9 and _same_bits(first.g, one.g)
    # at once again: the target holds the sum now and mirrors nothing -- the product is added on the way out, as before
    again0 = _tail(c, "0")
    os.environ["FEMO_D2H_CHUNK_MB"] = "0"
    E.dRdf_cell_apply_T_add_to_host(c.dm, c.CV, c.X, c.Y, again0.w, c.n)
    os.environ["FEMO_D2H_CHUNK_MB"] = MIB_CHUNK
    before = c.dm.tail_info()
    E.dRdf_cell_apply_T_add_to_host(c.dm, c.CV, c.X, c.Y, first.w, c.n)
    assert c.dm.tail_info()["plain"] == before["plain"] + 1 and c.dm.tail_info()["streamed"] == before["streamed"]
    assert _same_bits(first.w, again0.w)
    # the same array made a mirror again: through the same events, then through fewer of them
    for chunk, ranges in ((MIB_CHUNK, 9), (MIB_CHUNK, 9), ("2", 5)):
        r = _tail(c, chunk, into=first.w)
        assert r.did == dict(streamed=1, ranges=ranges, plain=0) and _same_bits(r.g, one.g)


def test_pageable_target_takes_the_plain_path(ctx):
    c = _engine(ctx, "cube")
    one = _reference(c)
    page = _tail(c, MIB_CHUNK, target="pageable")
    assert page.did == dict(streamed=0, ranges=0, plain=1) and page.st["d2h_device_sum"] == 0 and page.st["d2h_staged"] == 1
    assert _same_bits(page.g, one.g) and _same_bits(page.g, _tail(c, "0", target="pageable").g)


def test_target_that_mirrors_nothing_takes_the_plain_path(ctx):
    c = _engine(ctx, "cube")
    one = _reference(c)
    plain = _tail(c, MIB_CHUNK, target="plain")
    assert plain.did == dict(streamed=0, ranges=0, plain=1) and plain.st["d2h_device_sum"] == 0
    assert _same_bits(plain.g, one.g) and _same_bits(plain.g, _tail(c, "0", target="plain").g)


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


def test_two_emulated_ranks_take_the_plain_path():
    """A partitioned mesh: the multiplier's ghosts are exchanged first and the product runs in one launch, as before."""
    from femo_amd import engine as E
    from femo_amd.dist import DistMesh
    from femo_amd.dist.partition import build_local_mesh, rcb_partition
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    world, n = 2, 8
    gmesh = createUnitCubeMesh(n, jitter=0.2)
    part = rcb_partition(gmesh.x, world)

    def rank_fn(rank, c):
        utils_hip.set_context(c, thread_local=True)
        try:
            L = build_local_mesh(gmesh.x, gmesh.conn, part, rank, world)
            mesh = DistMesh(L, gmesh.n_vert, gmesh.n_cell, bbox=(gmesh.x.min(axis=0), gmesh.x.max(axis=0)))
            dm = mesh.device(c)
            ncell = len(L.conn)
            rng = np.random.default_rng(5 + rank)
            CV, X, G, Y = E.Vec(c, ncell), E.Vec(c, dm.n_vert), E.Vec(c, ncell), E.Vec(c, ncell)
            E.assemble_dRdf_cell(dm, 0, None, CV)
            X.set(rng.standard_normal(dm.n_vert))
            g = rng.standard_normal(ncell)
            G.set(g)
            w = E.writable(G.get(), announce=False)
            E.dRdf_cell_apply_T_add_to_host(dm, CV, X, Y, w, ncell)
            y = np.array(E.dRdf_cell_apply(dm, CV, X, E.Vec(c, ncell), transpose=True).get())
            return dict(got=np.array(w, copy=True), want=g + y, tail=dm.tail_info())
        finally:
            utils_hip.set_context(None, thread_local=True)

    os.environ["FEMO_D2H_CHUNK_MB"] = "0.001"
    for r in _run_ranks(world, rank_fn):
        print("rank:", r["tail"], "max |g - want|", np.abs(r["got"] - r["want"]).max())
        assert r["tail"] == dict(streamed=0, ranges=0, plain=1)
        assert _same_bits(r["got"], r["want"])


def _problem(ctx, name):
    """The benchmark's problem on the mesh, warmed up like bench.py."""
    if name not in _PROBLEMS:
        from bench import build_problem, one_cycle, source_fields
        from femo_amd import engine as E
        mesh = _mesh(name)
        sim, fea = build_problem(mesh, device=False)
        fs = source_fields(mesh, 3)
        os.environ["FEMO_D2H_CHUNK_MB"] = "0"
        one_cycle(sim, fea, E.pinned_array(fs[0]), E.pinned_full(mesh.n_vert, 0.0))
        _PROBLEMS[name] = types.SimpleNamespace(mesh=mesh, sim=sim, fea=fea, fs=fs, dm=mesh.device(ctx))
    return _PROBLEMS[name]


def _cycle(p, f_host, chunk):
    """One benchmark cycle with f_host at the operator boundary: (u, J, dJ/df, host statistics, what the tail did)."""
    from bench import one_cycle
    from femo_amd import engine as E
    os.environ["FEMO_D2H_CHUNK_MB"] = chunk
    before = p.dm.tail_info()
    E.host_stats(reset=True)
    g = one_cycle(p.sim, p.fea, f_host, E.pinned_full(p.mesh.n_vert, 0.0))
    st, after = E.host_stats(), p.dm.tail_info()
    return types.SimpleNamespace(u=np.array(E.host_wait(p.sim['u']), copy=True), g=np.array(E.host_wait(g), copy=True),
                                 J=float(np.asarray(p.sim['l2_functional']).ravel()[0]), st=st,
                                 did={k: after[k] - before[k] for k in after})


def test_cycle_through_the_operator_surface(ctx):
    from femo_amd import engine as E
    p = _problem(ctx, "cube")
    a, b = _cycle(p, E.pinned_array(p.fs[1]), "0"), _cycle(p, E.pinned_array(p.fs[1]), MIB_CHUNK)
    print(f"cycle: {b.did}; max |u - u0| {np.abs(a.u - b.u).max():.3e}, max |g - g0| {np.abs(a.g - b.g).max():.3e}, J - J0 {b.J - a.J:.3e}")
    assert a.did == dict(streamed=0, ranges=0, plain=1) and b.did == dict(streamed=1, ranges=9, plain=0)
    assert a.st["d2h_device_sum"] == 1 and b.st["d2h_device_sum"] == 1
    assert _same_bits(a.u, b.u) and _same_bits(a.g, b.g) and _same_bits([a.J], [b.J])


def test_bpx_cycle_over_the_streamed_tail(ctx):
    """The cycle bench.py measures, n = 32: BPX-preconditioned CG.  Two runs of it differ in the last bits by themselves, so
    the chunked cycle is held to that self-distance: relative max-norm distance to an unchunked run within
    8 x max(distance of two unchunked runs, 2.3e-16), the rule of tests/test_gpu_pcg_ring.py for the same noise."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    p = _problem(ctx, "small")
    utils_hip.KSP_OPTIONS["pc"] = "bpx"
    try:
        _cycle(p, E.pinned_array(p.fs[1]), "0")          # (the first BPX cycle of this problem builds the lattice)
        a, b = _cycle(p, E.pinned_array(p.fs[1]), "0"), _cycle(p, E.pinned_array(p.fs[1]), "0")
        c = _cycle(p, E.pinned_array(p.fs[1]), "0.25")   # 32,768 entries per range: the 196,608 cells in 6 ranges
    finally:
        utils_hip.KSP_OPTIONS["pc"] = "jacobi"
    assert c.did == dict(streamed=1, ranges=6, plain=0) and b.did == dict(streamed=0, ranges=0, plain=1)
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    for what, x, y, z in (("u", a.u, b.u, c.u), ("dJ/df", a.g, b.g, c.g),
                          ("J", np.array([a.J]), np.array([b.J]), np.array([c.J]))):
        s0, d = rel(x, y), max(rel(z, x), rel(z, y))
        print(f"BPX cycle, {what}: unchunked against unchunked {s0:.3e}, chunked against unchunked {d:.3e}")
        assert d <= 8 * max(s0, 2.3e-16), what
