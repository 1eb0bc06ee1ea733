"""Results on demand (femo_vec_get_host_promised, engine.lazy_results(on_demand=True), engine.host_forget): the pinned array
of ``Vec.get`` is recorded as the copy of the vector and marked in flight, but nothing travels until somebody needs the
bytes or the vector is about to change.

Vectors of 1 M entries; every comparison is exact (a copy moves bits).  What travelled is read from engine.host_stats:
a promise that is kept shows up as one d2h_async copy of 8 n bytes, a promise that is dropped as nothing at all.  A copy-out
is promised from 1 MiB on (hostmem.cpp, PROMISE_MIN_BYTES); a smaller one leaves at once, as before.  The cycle at the end
is therefore the n = 56 cube of tests/test_gpu_streamed_tail.py (185,193 vertices: 1.48 MB of multiplier; at n = 32 it would
be 287 KB and travel), with the Jacobi-preconditioned CG (a function of its inputs, tests/test_gpu_streamed_head.py): the
multiplier of the adjoint solve stays on the device, n_vert * 8 bytes fewer leave, and u, J and dJ/df are the same bits as
under FEMO_D2H_ON_DEMAND=0."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 20
_ENV = ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB", "FEMO_D2H_CHUNK_MB", "FEMO_D2H_ON_DEMAND")


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    pc, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], "jacobi"
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    utils_hip.clear_workspaces()
    E.host_sync()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(31)
    return rng.standard_normal(N), rng.standard_normal(N)


def _promise(v):
    from femo_amd import engine as E
    with E.lazy_results(True, on_demand=True):
        return v.get()


def _d2h_bytes(st):
    return st["d2h_pinned_bytes"] + st["d2h_staged_bytes"] + st["d2h_async_bytes"] + st["d2h_device_sum_bytes"]


def _vec(ctx, values):
    from femo_amd import engine as E
    v = E.Vec(ctx, values.size).set(values)
    ctx.sync()
    E.host_stats(reset=True)
    return v


def test_promised_array_after_host_wait(ctx, data):
    from femo_amd import engine as E
    v = _vec(ctx, data[0])
    a = _promise(v)
    assert not a.flags.writeable and E.host_stats()["d2h_async"] == 0 and _d2h_bytes(E.host_stats()) == 0
    E.host_wait(a)
    st = E.host_stats()
    assert st["d2h_async"] == 1 and _d2h_bytes(st) == 8 * N
    assert np.array_equal(a, data[0])
    E.host_wait(a)                                       # kept once
    assert E.host_stats()["d2h_async"] == 1


def test_promised_array_after_host_sync(ctx, data):
    from femo_amd import engine as E
    v, w = _vec(ctx, data[0]), _vec(ctx, data[1])
    a, b = _promise(v), _promise(w)
    assert E.host_stats()["d2h_async"] == 0
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 2
    assert np.array_equal(a, data[0]) and np.array_equal(b, data[1])


def test_eager_under_the_switch(ctx, data):
    from femo_amd import engine as E
    v = _vec(ctx, data[0])
    os.environ["FEMO_D2H_ON_DEMAND"] = "0"
    try:
        a = _promise(v)
    finally:
        del os.environ["FEMO_D2H_ON_DEMAND"]
    assert E.host_stats()["d2h_async"] == 1              # left at once: femo_vec_get_host_async
    assert np.array_equal(E.host_wait(a), data[0])


def test_small_results_leave_at_once(ctx, data):
    """Below 1 MiB the copy is cheaper than a promise that might have to be kept in front of a writer: eager, as before."""
    from femo_amd import engine as E
    small = data[0][:(1 << 17) - 1]                      # one entry short of 1 MiB
    v = _vec(ctx, small)
    a = _promise(v)
    assert E.host_stats()["d2h_async"] == 1 and E.host_stats()["d2h_async_bytes"] == 8 * small.size
    v.fill(0.0)
    assert np.array_equal(E.host_wait(a), small)
    edge = data[0][:1 << 17]                             # 1 MiB exactly: promised
    w = _vec(ctx, edge)
    b = _promise(w)
    assert E.host_stats()["d2h_async"] == 0
    assert np.array_equal(E.host_wait(b), edge) and E.host_stats()["d2h_async"] == 1


def test_source_changes_after_the_promise(ctx, data):
    """Mutated, refilled or destroyed: the array holds what the vector held when it was promised."""
    from femo_amd import engine as E
    v = _vec(ctx, data[0])
    a = _promise(v)
    v.fill(3.0)                                          # a kernel that writes v: the old content leaves first
    assert E.host_stats()["d2h_async"] == 1
    b = _promise(v)
    v.set(data[1])                                       # an upload into v
    c = _promise(v)
    other = E.Vec(ctx, N).set(data[0])
    v.axpy(2.0, other)
    d = _promise(v)
    del v                                                # destroyed with a promise outstanding
    gc.collect()
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 4
    assert np.array_equal(a, data[0]) and np.array_equal(b, np.full(N, 3.0)) and np.array_equal(c, data[1])
    assert np.array_equal(d, data[1] + 2.0 * data[0])


def test_forgotten_block_delivers_nothing_to_its_next_owner(ctx, data):
    from femo_amd import engine as E
    gc.collect()
    E.host_trim()                                        # an empty pool: the block released below is the next one of its size
    v = _vec(ctx, data[0])
    a = _promise(v)
    addr = a.ctypes.data
    E.host_forget(a)
    del a
    gc.collect()
    b = E.pinned_empty(N)                                # the recycled block of this size
    assert b.ctypes.data == addr
    b[:] = 7.0
    E.host_touch(b)
    v.fill(1.0)                                          # a writer of the source: nothing is owed any more
    ctx.sync()
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 0 and _d2h_bytes(E.host_stats()) == 0
    assert np.array_equal(b, np.full(N, 7.0))
    # ... and a block released with its promise outstanding, not forgotten first
    c = _promise(v)
    addr = c.ctypes.data
    del c
    gc.collect()
    d = E.pinned_empty(N)
    assert d.ctypes.data == addr
    d[:] = 5.0
    E.host_touch(d)
    v.fill(2.0)
    ctx.sync()
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 0 and np.array_equal(d, np.full(N, 5.0))
    # the target of another copy-out: the earlier promise is dropped, the new content arrives
    e = _promise(v)
    w = E.writable(e, announce=False)
    other = E.Vec(ctx, N).set(data[1])
    E.host_stats(reset=True)
    other.get(out=w)
    st = E.host_stats()
    assert st["d2h_async"] == 0 and st["d2h_pinned"] == 1 and np.array_equal(w, data[1])


def test_unresolved_array_back_into_set_moves_no_bytes(ctx, data):
    from femo_amd import engine as E
    v = _vec(ctx, data[0])
    a = _promise(v)
    v.set(a)                                             # the vector it came from: nothing to do
    w = E.Vec(ctx, N).set(a)                             # another vector: a copy on the device
    st = E.host_stats()
    assert st["h2d_skipped"] == 1 and st["h2d_as_d2d"] == 1
    assert st["h2d_pinned_bytes"] == 0 and st["h2d_staged_bytes"] == 0 and _d2h_bytes(st) == 0 and st["d2h_async"] == 0
    E.host_forget(a)
    assert np.array_equal(w.get(), data[0]) and np.array_equal(v.get(), data[0])
    assert E.host_stats()["d2h_async"] == 0


def test_verifier_reads_the_promised_array(ctx, data):
    from femo_amd import engine as E
    v = _vec(ctx, data[0])
    a = _promise(v)
    os.environ["FEMO_HOST_VERIFY"] = "1"
    try:
        v.set(a)                                         # the verifier compares bytes: the promise is kept first
    finally:
        del os.environ["FEMO_HOST_VERIFY"]
    assert E.host_stats()["d2h_async"] == 1 and E.host_stats()["h2d_skipped"] == 1
    assert np.array_equal(E.host_wait(a), data[0])


def test_cycle_keeps_the_multiplier_on_the_device(ctx):
    from bench import build_problem, one_cycle, source_fields
    from femo_amd import engine as E
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(56)
    assert 8 * mesh.n_vert >= 1 << 20
    sim, fea = build_problem(mesh, device=False)
    fs = source_fields(mesh, 2)
    one_cycle(sim, fea, E.pinned_array(fs[0]), E.pinned_full(mesh.n_vert, 0.0))

    def cycle(on_demand):
        if not on_demand:
            os.environ["FEMO_D2H_ON_DEMAND"] = "0"
        try:
            E.host_stats(reset=True)
            g = one_cycle(sim, fea, E.pinned_array(fs[1]), E.pinned_full(mesh.n_vert, 0.0))
            st = E.host_stats()
        finally:
            os.environ.pop("FEMO_D2H_ON_DEMAND", None)
        bits = lambda x: np.array(E.host_wait(np.asarray(x)), copy=True).ravel().view(np.uint64)
        return bits(sim['u']), bits(g), bits(sim['l2_functional']), st

    u0, g0, J0, st0 = cycle(False)
    u1, g1, J1, st1 = cycle(True)
    print(f"D2H bytes per cycle: eager {_d2h_bytes(st0)}, on demand {_d2h_bytes(st1)}; n_vert {mesh.n_vert}")
    assert _d2h_bytes(st0) - _d2h_bytes(st1) == 8 * mesh.n_vert
    assert st0["d2h_async"] - st1["d2h_async"] == 1
    assert np.array_equal(u0, u1) and np.array_equal(g0, g1) and np.array_equal(J0, J1)
