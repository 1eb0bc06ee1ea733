"""The streamed head of a cycle: a deferred upload of f travels in chunks (FEMO_H2D_CHUNK_MB), and femo_newton_rhs_linear
forms the load vector and the first Newton right-hand side range by range, on the row blocks whose cells have landed.

Every case compares against THE SAME CALL under FEMO_H2D_CHUNK_MB=0 (one copy, the single-launch path) with
np.array_equal: the ranges run the same kernels on the same rows, so the Newton right-hand side, the state, the functional
and the gradient are the same bits and no tolerance is involved.  The f arrays reach the 8 MiB threshold of the deferred
upload (n = 56 cube: 1,053,696 cells; 725^2 square: 1,051,250 cells) and chunks of 1 MiB cut them into 9 copies.

The cycles run with the Jacobi-preconditioned CG.  The BPX preconditioner accumulates its brick restriction with fp64
atomics, so two runs of the SAME cycle differ in the last bits whatever the upload does (measured on the n = 32 cube, both
runs through the synchronous upload and the single launch: max |u - u'| 2.1e-17, |g - g'| 2.1e-24): a bit-for-bit comparison
says nothing there.  With Jacobi every reduction has a fixed order, the cycle is a function of its inputs, and state,
functional and gradient are the same bits exactly when everything the head hands on is.  One case runs the BPX cycle that
bench.py measures and holds it to the distance of two one-copy runs."""
import os
import types

import numpy as np
import pytest

from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

MIB_CHUNK = "1"                      # 131,072 entries per copy: 9 copies of either array
SHORT_TAIL = "4.009765625"           # 2053 * 256 entries: the square's 1,051,250 cells leave a last copy of 114
ODD_TAIL = "1.607421875"             # 823 * 256 entries: the 1,053,695 cells of the cube less one leave a last copy of 255
_MESHES, _PROBLEMS, _ENGINE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _environment(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    saved = {k: os.environ.pop(k, None) for k in ("FEMO_HOST_VERIFY", "FEMO_H2D_CHUNK_MB")}   # the verifier uploads synchronously
    pc, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], "jacobi"
    yield
    utils_hip.KSP_OPTIONS["pc"] = pc
    _PROBLEMS.clear(); _ENGINE.clear(); _MESHES.clear()
    utils_hip.clear_workspaces()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _mesh(name):
    if name in _MESHES:
        return _MESHES[name]
    from femo_amd.fea.mesh import createUnitCubeMesh, createUnitSquareMesh
    if name == "square":
        m = createUnitSquareMesh(725)
    elif name == "small":
        m = createUnitCubeMesh(32)                     # 196,608 cells: 1.5 MB, below the threshold
    elif name == "odd":                                # the cube without its last cell (every vertex keeps two cells or more):
        from femo_amd.fea.mesh import Mesh             # an odd number of cells, still above the threshold
        full = createUnitCubeMesh(56)
        m = Mesh(full.x, full.conn[:-1], full.n)
    elif name == "permuted":
        m = createUnitCubeMesh(56).permuted(seed=3)    # random vertex numbering, as it comes
    elif name == "morton":
        m = createUnitCubeMesh(56).permuted(seed=3).reordered()
    else:
        m = createUnitCubeMesh(56)
    _MESHES[name] = m
    return m


def _problem(ctx, name, pinned=True):
    """The benchmark's problem on the mesh, warmed up like bench.py (the second cycle on linearises under the upload)."""
    key = name if pinned else name + ":pageable"
    if key not in _PROBLEMS:
        from bench import build_problem, one_cycle, source_fields
        from femo_amd import engine as E
        mesh = _mesh(name)
        sim, fea = build_problem(mesh, device=False, pinned=pinned)
        if mesh.tdim == 3:
            fs = source_fields(mesh, 3)
        else:                                            # (bench.py's fields are three-dimensional)
            xc = mesh.centroids()
            fs = [np.sin(np.pi * xc[:, 0]) * np.sin(np.pi * xc[:, 1]) * (0.5 + 0.3 * np.cos((k + 1) * np.pi * xc[:, 0]) + 0.2 * xc[:, 1])
                  for k in range(3)]
        os.environ["FEMO_H2D_CHUNK_MB"] = "0"
        one_cycle(sim, fea, E.pinned_array(fs[0]), E.pinned_full(mesh.n_vert, 0.0))
        _PROBLEMS[key] = types.SimpleNamespace(mesh=mesh, sim=sim, fea=fea, fs=fs, dm=mesh.device(ctx))
    return _PROBLEMS[key]


def _cycle(p, f_host, chunk, u0=None):
    """One benchmark cycle with f_host at the operator boundary: (u, J, dJ/df, host statistics, head queries)."""
    from bench import one_cycle
    from femo_amd import engine as E
    os.environ["FEMO_H2D_CHUNK_MB"] = chunk
    E.host_stats(reset=True)
    g = one_cycle(p.sim, p.fea, f_host, E.pinned_full(p.mesh.n_vert, 0.0) if u0 is None else u0)
    st = E.host_stats()
    return types.SimpleNamespace(u=np.array(E.host_wait(p.sim['u']), copy=True), g=np.array(E.host_wait(g), copy=True),
                                 J=float(np.asarray(p.sim['l2_functional']).ravel()[0]), st=st, head=p.dm.head_info())


def _engine(ctx, name):
    """The entry point on its own: operator, a random state that is NOT on the Dirichlet set's values, non-zero values."""
    if name not in _ENGINE:
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
        _ENGINE[name] = types.SimpleNamespace(mesh=mesh, dm=dm, ds=ds, U=U, F=F, B=B, K=K, A=A,
                                              f=[rng.standard_normal(mesh.n_cell) for _ in range(2)])
    return _ENGINE[name]


def _rhs(c, f_host, chunk, bc=True):
    """femo_newton_rhs_linear with f_host on its way: (b, host statistics, head queries)."""
    from femo_amd import engine as E
    os.environ["FEMO_H2D_CHUNK_MB"] = chunk
    E.host_stats(reset=True)
    with E.deferred_uploads():
        c.F.set(f_host)
        E.newton_rhs_linear(c.K, c.F, c.U, c.ds if bc else None, c.B)
    return types.SimpleNamespace(b=np.array(c.B.get()), st=E.host_stats(), head=c.dm.head_info())


def _same_cycle(a, b, what):
    du, dg = np.abs(a.u - b.u).max(), np.abs(a.g - b.g).max()
    print(f"{what}: max |u - u0| {du:.3e}, max |g - g0| {dg:.3e}, J - J0 {a.J - b.J:.3e}")
    assert np.array_equal(a.u, b.u) and np.array_equal(a.g, b.g) and a.J == b.J, what


def _both(ctx, name, chunk=MIB_CHUNK):
    """Right-hand side and cycle of `name`, chunked against one copy; returns the chunked runs."""
    from femo_amd import engine as E
    p, c = _problem(ctx, name), _engine(ctx, name)
    one = _rhs(c, E.pinned_array(c.f[0]), "0")
    many = _rhs(c, E.pinned_array(c.f[0]), chunk)
    print(f"{name}: max |b - b0| {np.abs(many.b - one.b).max():.3e}; copies {many.st['h2d_chunks']} / {one.st['h2d_chunks']}, "
          f"row blocks {many.head['row_blocks']}, before the last range {many.head['blocks_early']}")
    assert one.st["h2d_deferred"] == 1 and one.st["h2d_chunks"] == 1 and one.head["streamed"] == many.head["streamed"] - 1
    assert np.array_equal(many.b, one.b)
    nobc0, nobc = _rhs(c, E.pinned_array(c.f[1]), "0", bc=False), _rhs(c, E.pinned_array(c.f[1]), chunk, bc=False)
    assert np.array_equal(nobc.b, nobc0.b)
    cyc0 = _cycle(p, E.pinned_array(p.fs[1]), "0")
    cyc = _cycle(p, E.pinned_array(p.fs[1]), chunk)
    assert cyc0.st["h2d_deferred"] >= 1 and cyc.head["streamed"] == cyc0.head["streamed"] + 1
    _same_cycle(cyc, cyc0, name)
    return many, cyc


def test_structured_cube(ctx):
    many, cyc = _both(ctx, "cube")
    assert many.st["h2d_chunks"] == 9 and cyc.st["h2d_chunks"] == 9
    for r in (many, cyc):                                # lexicographic: the rows follow the cells
        assert 2 * r.head["blocks_early"] >= r.head["row_blocks"]


def test_structured_square(ctx):
    many, cyc = _both(ctx, "square")
    assert many.st["h2d_chunks"] == 9
    assert 2 * many.head["blocks_early"] >= many.head["row_blocks"]


def test_random_numbering_degenerates_to_one_range(ctx):
    many, cyc = _both(ctx, "permuted")
    assert many.st["h2d_chunks"] == 9
    for r in (many, cyc):                                # every row block needs a cell near the end: correct, not faster
        assert r.head["row_blocks"] - r.head["blocks_early"] > 0.9 * r.head["row_blocks"]


def test_morton_numbering_streams_again(ctx):
    many, cyc = _both(ctx, "morton")
    assert many.st["h2d_chunks"] == 9
    assert 2 * many.head["blocks_early"] >= many.head["row_blocks"]


def test_chunk_larger_than_the_array_is_one_copy(ctx):
    from femo_amd import engine as E
    c, p = _engine(ctx, "cube"), _problem(ctx, "cube")
    one, big = _rhs(c, E.pinned_array(c.f[0]), "0"), _rhs(c, E.pinned_array(c.f[0]), "16")
    assert big.st["h2d_deferred"] == 1 and big.st["h2d_chunks"] == 1
    assert big.head["streamed"] == one.head["streamed"] and big.head["load_builds"] == one.head["load_builds"] + 1
    assert np.array_equal(big.b, one.b)
    cyc0, cyc = _cycle(p, E.pinned_array(p.fs[1]), "0"), _cycle(p, E.pinned_array(p.fs[1]), "16")
    assert cyc.st["h2d_chunks"] == cyc.st["h2d_deferred"] >= 1 and cyc.head["streamed"] == cyc0.head["streamed"]
    _same_cycle(cyc, cyc0, "one copy of 16 MiB")


def test_last_chunk_shorter_than_256_cells(ctx):
    c = _engine(ctx, "square")
    assert c.mesh.n_cell - 2 * 2053 * 256 == 114
    many, cyc = _both(ctx, "square", SHORT_TAIL)
    assert many.st["h2d_chunks"] == 3 and cyc.st["h2d_chunks"] == 3


def test_odd_number_of_cells_with_an_odd_last_chunk(ctx):
    """The lone last cell of k_cell_fvol's double2 stream, on the offset pointers of the last range: 1,053,695 cells, five
    copies of 210,688 and one of 255."""
    c = _engine(ctx, "odd")
    assert c.mesh.n_cell % 2 == 1 and c.mesh.n_cell * 8 >= 8 << 20 and c.mesh.n_cell - 5 * 823 * 256 == 255
    many, cyc = _both(ctx, "odd", ODD_TAIL)
    assert many.st["h2d_chunks"] == 6 and cyc.st["h2d_chunks"] == 6
    many, cyc = _both(ctx, "odd")                       # and with the odd cell at the end of a long last copy
    assert many.st["h2d_chunks"] == 9


def test_bpx_cycle_over_the_streamed_head(ctx):
    """The cycle bench.py measures: BPX-preconditioned CG.  Two runs of it differ in the last bits by themselves (fp64 atomics
    in the brick restriction), so the chunked cycle is held to that self-distance: relative max-norm distance to a one-copy
    run within 8 x max(distance of two one-copy runs, 2.3e-16) -- the rule of test_gpu_pcg_ring.py for the same noise (one
    rounding as the floor; DESIGN_LOG R13 records up to 5.3 between maxima of this noise over a handful of runs)."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    p = _problem(ctx, "cube")
    utils_hip.KSP_OPTIONS["pc"] = "bpx"
    try:
        _cycle(p, E.pinned_array(p.fs[1]), "0")          # (the first BPX cycle of this problem builds the lattice)
        a, b = _cycle(p, E.pinned_array(p.fs[1]), "0"), _cycle(p, E.pinned_array(p.fs[1]), "0")
        c = _cycle(p, E.pinned_array(p.fs[1]), MIB_CHUNK)
    finally:
        utils_hip.KSP_OPTIONS["pc"] = "jacobi"
    assert c.st["h2d_chunks"] == 9 and c.head["streamed"] == b.head["streamed"] + 1
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    for what, x, y, z in (("u", a.u, b.u, c.u), ("dJ/df", a.g, b.g, c.g),
                          ("J", np.array([a.J]), np.array([b.J]), np.array([c.J]))):
        s0, d = rel(x, y), max(rel(z, x), rel(z, y))
        print(f"BPX cycle, {what}: one copy against one copy {s0:.3e}, chunked against one copy {d:.3e}")
        assert d <= 8 * max(s0, 2.3e-16), what


def test_second_solve_with_the_same_f_finds_the_load_vector(ctx):
    from femo_amd import engine as E
    c, p = _engine(ctx, "cube"), _problem(ctx, "cube")
    first = _rhs(c, E.pinned_array(c.f[1]), MIB_CHUNK)
    E.newton_rhs_linear(c.K, c.F, c.U, c.ds, c.B)        # the same vector, untouched: complete and cached
    again = c.dm.head_info()
    assert again["load_builds"] == first.head["load_builds"] and again["streamed"] == first.head["streamed"]
    assert np.array_equal(np.array(c.B.get()), first.b)
    fpin = E.pinned_array(p.fs[2])                       # the cycle: the second hand-over of the block is elided, f keeps its generation
    a = _cycle(p, fpin, MIB_CHUNK)
    b = _cycle(p, fpin, MIB_CHUNK)
    assert b.st["h2d_deferred"] == 0 and b.head["load_builds"] == a.head["load_builds"] and b.head["streamed"] == a.head["streamed"]
    _same_cycle(b, a, "same f again")


def test_new_f_of_the_same_size_reuses_the_events(ctx):
    from femo_amd import engine as E
    c, p = _engine(ctx, "cube"), _problem(ctx, "cube")
    ref = [_rhs(c, E.pinned_array(f), "0").b for f in c.f]
    for k in (0, 1, 0):                                  # the same vector, upload after upload through the same events
        r = _rhs(c, E.pinned_array(c.f[k]), MIB_CHUNK)
        assert r.st["h2d_chunks"] == 9 and np.array_equal(r.b, ref[k])
    r = _rhs(c, E.pinned_array(c.f[1]), "2")             # fewer copies than there are events
    assert r.st["h2d_chunks"] == 5 and np.array_equal(r.b, ref[1])
    cyc0 = [_cycle(p, E.pinned_array(p.fs[k]), "0") for k in (1, 2)]
    for k, chunk, copies in ((0, MIB_CHUNK, 9), (1, MIB_CHUNK, 9), (0, "2", 5)):      # the cycle's own f vector likewise
        cyc = _cycle(p, E.pinned_array(p.fs[k + 1]), chunk)
        assert cyc.st["h2d_chunks"] == copies
        _same_cycle(cyc, cyc0[k], f"new f {k}, {copies} copies")


def test_nonzero_initial_state_with_a_dirichlet_set(ctx):
    """u = 1 (CSDL's default) against the benchmark's zero boundary values: the lifted rows K u' of the first right-hand
    side lie on both sides of every range boundary; the engine-level cases above use non-zero values on the set."""
    from femo_amd import engine as E
    p = _problem(ctx, "cube")
    ones = lambda: E.pinned_full(p.mesh.n_vert, 1.0)
    a, b = _cycle(p, E.pinned_array(p.fs[1]), "0", u0=ones()), _cycle(p, E.pinned_array(p.fs[1]), MIB_CHUNK, u0=ones())
    assert b.st["h2d_chunks"] == 9 and b.head["streamed"] == a.head["streamed"] + 1
    _same_cycle(b, a, "u0 = 1")


def test_pageable_and_small_inputs_take_the_synchronous_upload(ctx):
    from femo_amd import engine as E
    c = _engine(ctx, "cube")
    one = _rhs(c, E.pinned_array(c.f[0]), "0")
    page = _rhs(c, np.array(c.f[0]), MIB_CHUNK)          # pageable memory: through the staging ring, synchronous
    assert page.st["h2d_deferred"] == 0 and page.st["h2d_chunks"] == 0 and page.st["h2d_staged"] == 1
    assert page.head["streamed"] == one.head["streamed"] and np.array_equal(page.b, one.b)
    q = _problem(ctx, "cube", pinned=False)              # ... and the pageable driver's cycle
    a, b = _cycle(q, np.array(q.fs[1]), "0"), _cycle(q, np.array(q.fs[1]), MIB_CHUNK)
    assert b.st["h2d_deferred"] == 0 and b.st["h2d_chunks"] == 0 and b.head["streamed"] == a.head["streamed"]
    _same_cycle(b, a, "pageable f")
    s, cs = _problem(ctx, "small"), _engine(ctx, "small")
    r0, r1 = _rhs(cs, E.pinned_array(cs.f[0]), "0"), _rhs(cs, E.pinned_array(cs.f[0]), "0.25")
    assert r1.st["h2d_deferred"] == 0 and r1.st["h2d_chunks"] == 0 and r1.head["streamed"] == 0 and np.array_equal(r1.b, r0.b)
    a, b = _cycle(s, E.pinned_array(s.fs[1]), "0"), _cycle(s, E.pinned_array(s.fs[1]), "0.25")
    assert b.st["h2d_deferred"] == 0 and b.st["h2d_chunks"] == 0 and b.head["streamed"] == 0
    _same_cycle(b, a, "f below 8 MiB")
