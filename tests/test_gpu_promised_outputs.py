"""The partials of an output operator as promised copy-outs (FEMO_PROMISE_OUTPUT, FEMO_D2H_PROMISE_OUTPUTS): in a reverse
sweep dJ/du goes straight back into the adjoint solve and the explicit dJ/df is overwritten by the streamed tail from the
device, so neither crosses the link -- but whoever reads one of them on the host gets the vector's content.

The cycles run with the Jacobi-preconditioned CG (a function of its inputs: tests/test_gpu_streamed_head.py), so a cycle with
and without the promises is compared bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 20
_ENV = ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB", "FEMO_D2H_CHUNK_MB", "FEMO_D2H_ON_DEMAND", "FEMO_D2H_PROMISE_OUTPUTS",
        "FEMO_RANGE_FLOOR_MB", "FEMO_RANGE_FACTOR", "FEMO_D2H_MAX_CHUNK_MB")
_CUBE = {}


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    pc, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], "jacobi"
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    _CUBE.clear()
    utils_hip.clear_workspaces()
    E.host_sync()
    for k in _ENV:
        os.environ.pop(k, None)
    for k, v in saved.items():
        if v is not None:
            os.environ[k] = v


def _d2h_bytes(st):
    return st["d2h_pinned_bytes"] + st["d2h_staged_bytes"] + st["d2h_async_bytes"] + st["d2h_device_sum_bytes"]


def _bits(x):
    from femo_amd import engine as E
    return np.array(E.host_wait(np.asarray(x)), copy=True).ravel().view(np.uint64)


def _problem(n):
    """bench.py's problem on the n-cube, one cycle run (the pool and the workspaces are warm)."""
    if n not in _CUBE:
        from bench import build_problem, one_cycle, source_fields
        from femo_amd import engine as E
        from femo_amd.fea.mesh import createUnitCubeMesh
        mesh = createUnitCubeMesh(n)
        sim, fea = build_problem(mesh, device=False)
        fs = source_fields(mesh, 2)
        one_cycle(sim, fea, E.pinned_array(fs[0]), E.pinned_full(mesh.n_vert, 0.0))
        _CUBE[n] = (mesh, sim, fea, fs)
    return _CUBE[n]


def _cycle(n, **env):
    from bench import one_cycle
    from femo_amd import engine as E
    mesh, sim, fea, fs = _problem(n)
    os.environ.update(env)
    try:
        E.host_stats(reset=True)
        g = one_cycle(sim, fea, E.pinned_array(fs[1]), E.pinned_full(mesh.n_vert, 0.0))
        st = E.host_stats()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return _bits(sim['u']), _bits(g), _bits(sim['l2_functional']), st


def test_cycle_keeps_the_outputs_partials_off_the_link(ctx):
    mesh = _problem(56)[0]
    assert 8 * mesh.n_vert >= 1 << 20
    u0, g0, J0, st0 = _cycle(56, FEMO_D2H_PROMISE_OUTPUTS="0")
    u1, g1, J1, st1 = _cycle(56)
    print(f"D2H bytes per cycle: eager {_d2h_bytes(st0)}, promised {_d2h_bytes(st1)}; n_cell {mesh.n_cell}, n_vert {mesh.n_vert}; "
          f"asynchronous copy-outs {st0['d2h_async']} / {st1['d2h_async']}")
    assert _d2h_bytes(st0) - _d2h_bytes(st1) == 8 * (mesh.n_cell + mesh.n_vert)
    assert st0["d2h_async"] - st1["d2h_async"] == 2          # nothing was sent for the tail's target block, nor for dJ/du
    assert st1["d2h_device_sum"] == 1 and st1["d2h_device_sum_bytes"] == 8 * mesh.n_cell
    assert np.array_equal(u0, u1) and np.array_equal(g0, g1) and np.array_equal(J0, J1)
    # the multiplier's switch does not govern them: without it exactly its 8 n_vert bytes more, as before
    u2, g2, J2, st2 = _cycle(56, FEMO_D2H_ON_DEMAND="0")
    assert _d2h_bytes(st2) - _d2h_bytes(st1) == 8 * mesh.n_vert and st2["d2h_async"] - st1["d2h_async"] == 1
    assert np.array_equal(u2, u1) and np.array_equal(g2, g1) and np.array_equal(J2, J1)


def test_small_cycle_promises_nothing(ctx):
    mesh = _problem(12)[0]
    assert 8 * mesh.n_cell < 1 << 20
    u0, g0, J0, st0 = _cycle(12, FEMO_D2H_PROMISE_OUTPUTS="0")
    u1, g1, J1, st1 = _cycle(12)
    assert _d2h_bytes(st0) == _d2h_bytes(st1) == 8 * (2 * mesh.n_cell + 3 * mesh.n_vert) and st0["d2h_async"] == st1["d2h_async"]
    assert np.array_equal(u0, u1) and np.array_equal(g0, g1) and np.array_equal(J0, J1)


def test_explicit_read_delivers_the_partials(ctx):
    """compute_derivatives on its own, then a reader on the host: one copy each, the content of the eager copies."""
    from femo_amd import engine as E
    from femo_amd.csdl_opt.output_model import OutputOperation
    mesh, sim, fea, fs = _problem(56)
    _cycle(56)
    op = next(op for _, op in sim.ops if isinstance(op, OutputOperation))
    inputs = {k: sim.values[k] for k in op.input_meta}
    os.environ["FEMO_D2H_PROMISE_OUTPUTS"] = "0"
    try:
        eager = {}
        op.compute_derivatives(inputs, eager)
        eager = {k: np.array(E.host_wait(v), copy=True) for k, v in eager.items()}
    finally:
        os.environ.pop("FEMO_D2H_PROMISE_OUTPUTS", None)
    os.environ["FEMO_D2H_ON_DEMAND"] = "0"                # (not their switch)
    try:
        E.host_stats(reset=True)
        lazy = {}
        op.compute_derivatives(inputs, lazy)
        assert E.host_stats()["d2h_async"] == 0 and _d2h_bytes(E.host_stats()) == 0
    finally:
        os.environ.pop("FEMO_D2H_ON_DEMAND", None)
    assert sorted(v.size for v in lazy.values()) == [mesh.n_vert, mesh.n_cell]
    sent = 0
    for key, v in lazy.items():
        assert not v.flags.writeable
        got = np.array(E.host_wait(v), copy=True)
        sent += 1
        st = E.host_stats()
        assert st["d2h_async"] == sent and np.array_equal(got.view(np.uint64), eager[key].view(np.uint64)), key
        E.host_wait(v)                                   # kept once
        assert E.host_stats()["d2h_async"] == sent
    assert _d2h_bytes(E.host_stats()) == 8 * (mesh.n_cell + mesh.n_vert)
    # ... and host_sync keeps them all
    lazy = {}
    E.host_stats(reset=True)
    op.compute_derivatives(inputs, lazy)
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 2
    for key, v in lazy.items():
        assert np.array_equal(np.asarray(v).view(np.uint64), eager[key].view(np.uint64)), key


def _promise_output(v):
    from femo_amd import engine as E
    with E.lazy_results(True, on_demand=True, outputs=True):
        return v.get()


def test_negated_promise_is_a_promise(ctx):
    """y = -x with x only promised (the reverse sweep's adjoint seed): nothing travels, handed to Vec.set it is a scale on the
    device, a reader gets -x with one copy, and forgotten it delivers nothing."""
    from femo_amd import engine as E
    rng = np.random.default_rng(5)
    data = rng.standard_normal(N)
    v = E.Vec(ctx, N).set(data)
    ctx.sync()
    E.host_stats(reset=True)
    x = _promise_output(v)
    y = E.pinned_empty(N)
    y[:] = 9.0
    E.host_touch(y)
    E.host_axpby(-1.0, x, 0.0, y)
    w = E.Vec(ctx, N).set(y)
    st = E.host_stats()
    assert st["d2h_async"] == 0 and _d2h_bytes(st) == 0 and st["h2d_as_d2d"] == 1 and st["h2d_pinned_bytes"] == 0
    assert np.array_equal(w.get(), -data)
    E.host_stats(reset=True)
    assert np.array_equal(E.host_wait(y), -data) and E.host_stats()["d2h_async"] == 1      # the reader: one copy, scaled behind it
    assert np.array_equal(E.host_wait(x), data) and E.host_stats()["d2h_async"] == 2
    # forgotten: a writer of the source owes nothing, and the block keeps what its owner writes
    x2 = _promise_output(v)
    E.host_axpby(-2.0, x2, 0.0, y)
    E.host_forget(y)
    E.host_forget(x2)
    y[:] = 4.0
    E.host_touch(y)
    E.host_stats(reset=True)
    v.fill(1.0)
    ctx.sync()
    E.host_sync()
    assert E.host_stats()["d2h_async"] == 0 and np.array_equal(y, np.full(N, 4.0))
    # a writer of the source in front of a reader: the scaled promise is kept with the old content
    v.set(data)
    x3 = _promise_output(v)
    E.host_axpby(0.5, x3, 0.0, y)
    v.fill(2.0)
    assert np.array_equal(E.host_wait(y), 0.5 * data) and np.array_equal(E.host_wait(x3), data)


def test_tail_target_drops_its_promise(ctx):
    """The streamed tail into a block that was only promised the explicit gradient: the sum is formed from the vector, the
    promise is dropped and nothing is sent for it; the same bits as into the eager copy."""
    from femo_amd import engine as E
    mesh = _problem(56)[0]
    dm = mesh.device(ctx)
    rng = np.random.default_rng(23)
    CV, X, G, Y = E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_vert), E.Vec(ctx, mesh.n_cell), E.Vec(ctx, mesh.n_cell)
    E.assemble_dRdf_cell(dm, 0, None, CV)
    X.set(rng.standard_normal(mesh.n_vert))
    g = rng.standard_normal(mesh.n_cell) * 1e-3
    os.environ["FEMO_D2H_CHUNK_MB"] = "1"
    try:
        out = []
        for promised in (False, True):
            G.set(g)
            w = E.writable(_promise_output(G) if promised else G.get(), announce=False)
            before = dm.tail_info()
            E.host_stats(reset=True)
            E.dRdf_cell_apply_T_add_to_host(dm, CV, X, Y, w, mesh.n_cell)
            G.fill(0.0)                                  # a writer of the source: no promise is left to keep
            ctx.sync()
            E.host_sync()
            st, after = E.host_stats(), dm.tail_info()
            assert after["streamed"] - before["streamed"] == 1 and after["plain"] == before["plain"]
            assert st["d2h_async"] == 0 and st["d2h_device_sum"] == 1 and _d2h_bytes(st) == 8 * mesh.n_cell
            out.append(np.array(w, copy=True))
    finally:
        os.environ.pop("FEMO_D2H_CHUNK_MB", None)
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)) and not np.array_equal(out[0], g)
    # the plain tail (product, then accumulate on the device) drops the promise as well, and the verifier keeps it
    for env, sent in (({"FEMO_D2H_CHUNK_MB": "0"}, 0), ({"FEMO_D2H_CHUNK_MB": "0", "FEMO_HOST_VERIFY": "1"}, 1),
                      ({"FEMO_D2H_CHUNK_MB": "1", "FEMO_HOST_VERIFY": "1"}, 1)):
        os.environ.update(env)
        try:
            G.set(g)
            w = E.writable(_promise_output(G), announce=False)
            E.host_stats(reset=True)
            E.dRdf_cell_apply_T_add_to_host(dm, CV, X, Y, w, mesh.n_cell)
            st = E.host_stats()
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert st["d2h_async"] == sent and st["d2h_device_sum"] == 1, env
        assert np.array_equal(np.array(w).view(np.uint64), out[0].view(np.uint64)), env
