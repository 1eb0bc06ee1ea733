"""The pool of pinned blocks in a steady cycle, and blocks released with a transfer in flight (csrc/hostmem.cpp).

femo_host_stats counts what a warmed-up cycle must not do: fresh hipHostMallocs (pool_fresh) and releases of blocks a DMA
still owns -- parked by femo_host_free (pool_free_deferred) and recycled by a later pool call once their event is complete, or
waited for by femo_host_unregister, which cannot park a caller's memory (pool_free_waited).  A release of a pool block returns
at once, and the block reaches no new owner before its last DMA is over -- the recycled-block cases of
tests/test_gpu_on_demand_copy.py, with a copy in flight instead of a promise.

The timing bound: 128 MiB take at least 2.3 ms at the link's 57 GB/s; a release that waited for the copy, enqueued
microseconds before, would take about that long, one that parks the block takes microseconds (11 us observed).  The bound is
1 ms, below half the copy's time."""
import gc
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 24                           # 128 MiB: a copy of 2.3 ms at the link's rate
_ENV = ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB", "FEMO_D2H_CHUNK_MB", "FEMO_D2H_ON_DEMAND", "FEMO_D2H_PROMISE_OUTPUTS",
        "FEMO_RANGE_FLOOR_MB", "FEMO_RANGE_FACTOR", "FEMO_D2H_MAX_CHUNK_MB")


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    pc = utils_hip.KSP_OPTIONS["pc"]
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    utils_hip.clear_workspaces()
    E.host_sync()
    gc.collect()
    E.host_trim()                                        # the 128 MiB blocks of this module
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def test_steady_cycles_allocate_nothing_and_wait_for_nothing(ctx):
    from bench import PC, build_problem, one_cycle, source_fields
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    utils_hip.KSP_OPTIONS["pc"] = PC
    mesh = createUnitCubeMesh(32)
    sim, fea = build_problem(mesh, device=False)
    f_pin = [E.pinned_array(f) for f in source_fields(mesh, 4)]
    u0 = E.pinned_full(mesh.n_vert, 0.0)
    g = None
    for k in range(2):
        g = one_cycle(sim, fea, f_pin[k], u0)            # held across the next cycle, as a driver holds its gradient
    E.host_stats(reset=True)
    for k in range(2, 5):
        g = one_cycle(sim, fea, f_pin[k % 4], u0)
    st = E.host_stats()
    print({k: st[k] for k in st if k.startswith("pool_")})
    assert st["pool_fresh"] == 0 and st["pool_fresh_us"] == 0
    assert st["pool_free_deferred"] == 0                 # no release of a block in flight: nothing a waiting free would wait for
    assert st["pool_free_waited"] == 0 and st["pool_free_waited_us"] == 0
    assert np.isfinite(np.asarray(E.host_wait(g))).all()


def test_release_with_a_copy_out_in_flight_returns_at_once(ctx):
    from femo_amd import engine as E
    gc.collect()
    E.host_sync()
    E.host_trim()                                        # an empty pool: what is released below is the only block of its size
    data = np.random.default_rng(41).standard_normal(N)
    v = E.Vec(ctx, N).set(data)
    ctx.sync()
    E.host_stats(reset=True)
    with E.lazy_results(True):
        a = v.get()                                      # the copy-out is enqueued; nobody waits for it
    addr = a.ctypes.data
    t0 = time.perf_counter()
    del a                                                # the only reference: femo_host_free runs here
    dt = (time.perf_counter() - t0) * 1e3
    b = E.pinned_empty(N)                                # the next owner of this size, microseconds later
    st = E.host_stats()
    print(f"release with the copy in flight: {dt:.3f} ms, {({k: st[k] for k in st if k.startswith('pool_')})}, "
          f"next owner got {'the same' if b.ctypes.data == addr else 'another'} block")
    assert st["d2h_async"] == 1 and st["pool_free_deferred"] == 1 and st["pool_free_waited"] == 0
    assert dt < 1.0                                      # returned without waiting for the 2.3 ms copy
    assert b.ctypes.data != addr and st["pool_fresh"] == 2   # the parked block is not handed on: a fresh one (a's was the first)
    b[:] = 7.0
    E.host_touch(b)
    ctx.sync()                                           # every copy enqueued so far has landed
    E.host_sync()
    assert np.array_equal(b, np.full(N, 7.0))            # no late DMA into the new owner's block
    fresh = E.host_stats()["pool_fresh"]
    c = E.pinned_empty(N)                                # the parked block, recycled now that its event is complete
    assert c.ctypes.data == addr and E.host_stats()["pool_fresh"] == fresh
    c[:] = 5.0
    E.host_touch(c)
    ctx.sync()
    assert np.array_equal(c, np.full(N, 5.0)) and np.array_equal(b, np.full(N, 7.0))
    assert np.array_equal(v.get(), data)


def test_release_with_an_upload_in_flight_still_delivers(ctx):
    """A deferred upload reads the block after the array is gone: the block is parked, not handed on, until the copy is over."""
    from femo_amd import engine as E
    gc.collect()
    E.host_sync()
    E.host_trim()                                        # an empty pool, as above
    data = np.random.default_rng(43).standard_normal(N)
    v = E.Vec(ctx, N).fill(0.0)
    ctx.sync()
    a = E.pinned_array(data)
    addr = a.ctypes.data
    E.host_stats(reset=True)
    with E.deferred_uploads():
        v.set(a)
        t0 = time.perf_counter()
        del a                                            # the only reference: femo_host_free runs here
        dt = (time.perf_counter() - t0) * 1e3
        b = E.pinned_empty(N)                            # must not be the block the DMA still reads
        st = E.host_stats()
        b[:] = -3.0
        E.host_touch(b)
    print(f"release with the upload in flight: {dt:.3f} ms, {({k: st[k] for k in st if k.startswith('pool_')})}")
    assert st["h2d_deferred"] == 1 and st["pool_free_deferred"] == 1 and st["pool_free_waited"] == 0 and dt < 1.0
    assert b.ctypes.data != addr and st["pool_fresh"] == 1
    assert np.array_equal(v.get(), data)


def test_unpinning_a_caller_array_in_flight_waits_and_is_counted(ctx):
    """Caller memory pinned in place cannot be parked -- its owner frees it next: femo_host_unregister waits for the copy,
    outside the pool's lock, and that wait is what pool_free_waited counts."""
    from femo_amd import engine as E
    data = np.random.default_rng(47).standard_normal(N)
    v = E.Vec(ctx, N).set(data)
    out = np.zeros(N)
    assert E.register(out)
    ctx.sync()
    E.host_stats(reset=True)
    E.check(E._lib.load().femo_vec_get_host_async(v.handle, out.ctypes.data, N))   # returns with the copy in flight
    E._forget_owner(id(out))                             # what NumPy's release of the array triggers: unpin the range
    st = E.host_stats()
    print({k: st[k] for k in st if k.startswith("pool_")})
    assert st["d2h_async"] == 1 and st["pool_free_waited"] == 1 and st["pool_free_waited_us"] > 0 and st["pool_free_deferred"] == 0
    assert not E.is_pinned(out) and np.array_equal(out, data)
