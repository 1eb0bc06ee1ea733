"""The compacted copy of S A S (csrc/spmv.hip: k_scale_sell<true>, femo_launch_spmv, femo_mat_compact_settle).  The scaling
of a matrix also writes a copy in which every regular slice keeps only the slots that are not zero in all 64 rows, packed to
the front in their order; the products of the Krylov loops walk that copy.  A dead slot contributed acc += 0 * x and the live
ones keep their order, so for finite x every product is the full product bit for bit: each case compares, on uint64 views,
with the same call under FEMO_SPMV_COMPACT=0 on a fresh matrix, and asks the library (Mat.compact_info, femo_mat_compact_info
of femo_hip_test.h) what the build packed and which copy the products read.

On a structured simplicial grid the P1 stiffness couples a vertex with its axis neighbours only: of the 14 stored slots of a
cube's row (6 axis neighbours, 6 face diagonals, 2 body diagonals) 8 hold exact zeros, of the 6 of a square's row 2 do."""
import gc
import os

import numpy as np
import pytest

from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

EPS = 2.3e-16
DOTS = {"none": 0, "dax": 1, "dax_xx": 2, "dax_axax": 3}


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.delenv("FEMO_SPMV_COMPACT", raising=False)
    yield


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _x(n, seed=11):
    """Random without zeros."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    x[x == 0.0] = 1.0
    return x


def _stiffness(ctx, dm, mesh, seed=3):
    """K of the Poisson form, no Dirichlet set (every row keeps its couplings), in a fresh matrix."""
    from femo_amd import engine as E
    rng = np.random.default_rng(seed)
    K = E.Mat(dm)
    E.assemble_system(dm, 0, None, E.Vec(ctx, mesh.n_vert).set(np.zeros(mesh.n_vert)),
                      E.Vec(ctx, mesh.n_cell).set(1.0 + rng.random(mesh.n_cell)), None, K, None, None)
    return K


def _product(ctx, A, x, dots=0):
    from femo_amd import engine as E
    y = E.Vec(ctx, len(x))
    part = A.spmv_scaled(dots, E.Vec(ctx, len(x)).set(x), y)
    return y.get().copy(), part


def _plain(monkeypatch, fn):
    """fn() under FEMO_SPMV_COMPACT=0."""
    monkeypatch.setenv("FEMO_SPMV_COMPACT", "0")
    try:
        return fn()
    finally:
        monkeypatch.delenv("FEMO_SPMV_COMPACT", raising=False)


def _slices(dm):
    """The slices of the mesh from its pattern, by the rule of csrc/topology.cpp (step 3.5): (regular, pairs stored) each.  A
    full slice is regular when the union of its rows' column deltas is no larger than the longest row of the mesh and every
    row + delta is a vertex; it stores the union.  Every other slice stores its longest row.  Pairs: padded to even."""
    rowptr, col = dm.pattern_csr()
    n = dm.n_rows
    row = np.repeat(np.arange(n), np.diff(rowptr))
    d = col.astype(np.int64) - row
    longest = int(np.diff(rowptr).max()) - 1
    out = []
    for s in range(dm.info["n_slices"]):
        v0, v1 = 64 * s, 64 * s + 63
        lo, hi = rowptr[v0], rowptr[min(v1 + 1, n)]
        ds = np.unique(d[lo:hi][d[lo:hi] != 0])
        regular = v1 < n and 0 < len(ds) <= min(longest, 32) and v0 + ds[0] >= 0 and v1 + ds[-1] < dm.n_vert
        width = len(ds) if regular else int(np.diff(rowptr[v0:min(v1 + 1, n) + 1]).max()) - 1
        out.append((bool(regular), (width + 1) // 2))
    assert sum(r for r, _ in out) == dm.info["regular_slices"]
    return out


def _irregular_pairs(dm):
    return sum(p for r, p in _slices(dm) if not r)


@pytest.fixture(scope="module")
def cube8(ctx):
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(8)
    dm = mesh.device(ctx)
    # 12 slices: 2 .. 8 are regular; in 0, 1, 9 and 10 a completed column would leave the mesh, the last one is partial
    assert mesh.n_vert == 729 and dm.info["n_slices"] == 12 and dm.info["regular_slices"] == 7
    assert [r for r, _ in _slices(dm)] == [False] * 2 + [True] * 7 + [False] * 3
    return mesh, dm


# ---- case 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dots", list(DOTS))
def test_cube_keeps_three_pairs_and_every_variant_is_bit_equal(ctx, monkeypatch, cube8, dots):
    mesh, dm = cube8
    x = _x(mesh.n_vert)
    K = _stiffness(ctx, dm, mesh)
    y, part = _product(ctx, K, x, DOTS[dots])
    info = K.compact_info()
    y0, part0 = _plain(monkeypatch, lambda: _product(ctx, _stiffness(ctx, dm, mesh), x, DOTS[dots]))
    print(f"compact cube n=8 {dots}: {info}")
    assert info["valid"] == 1 and info["slices"] == 7
    assert info["live_pairs"] == 3 * 7 + _irregular_pairs(dm), info
    assert info["full_pairs"] == 7 * 7 + _irregular_pairs(dm), info
    assert info["products_compact"] == 1 and info["products_full"] == 0, info
    assert _same(y, y0)
    assert part.shape == part0.shape and part.shape[0] == {0: 0, 1: 1, 2: 2, 3: 2}[DOTS[dots]]
    assert _same(part, part0)


# ---- case 2 -----------------------------------------------------------------------------------------------------------
def test_square_keeps_two_pairs_of_three(ctx, monkeypatch):
    from femo_amd.fea.mesh import createUnitSquareMesh
    mesh = createUnitSquareMesh(32)
    dm = mesh.device(ctx)
    reg, ns = dm.info["regular_slices"], dm.info["n_slices"]
    assert mesh.n_vert == 1089 and 2 * reg >= ns
    x = _x(mesh.n_vert)
    K = _stiffness(ctx, dm, mesh)
    y, part = _product(ctx, K, x, 1)
    info = K.compact_info()
    y0, part0 = _plain(monkeypatch, lambda: _product(ctx, _stiffness(ctx, dm, mesh), x, 1))
    print(f"compact square n=32: {info}, regular {reg} of {ns}")
    # every regular slice stores 6 slots (3 pairs) and keeps +-1 and +-(n + 1): 2 pairs; the rest walks what it stores
    assert info["valid"] == 1 and info["slices"] == reg
    assert info["live_pairs"] == 2 * reg + _irregular_pairs(dm), info
    assert info["full_pairs"] == 3 * reg + _irregular_pairs(dm), info
    assert info["products_compact"] == 1
    assert _same(y, y0) and _same(part, part0)


# ---- case 3 -----------------------------------------------------------------------------------------------------------
def test_jittered_cube_has_nothing_dead_and_the_gate_switches_the_build_off(ctx, monkeypatch):
    from femo_amd import engine as E
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(12, jitter=0.2)
    dm = mesh.device(ctx)
    assert 2 * dm.info["regular_slices"] >= dm.info["n_slices"]
    x = _x(mesh.n_vert)
    K = _stiffness(ctx, dm, mesh)
    y, part = _product(ctx, K, x, 1)
    info = K.compact_info()
    y0, part0 = _plain(monkeypatch, lambda: _product(ctx, _stiffness(ctx, dm, mesh), x, 1))
    print(f"compact jittered n=12 before the solve: {info}")
    assert info["valid"] == 1 and info["live_pairs"] == info["full_pairs"] > 0, info
    assert info["products_compact"] == 1 and info["products_full"] == 0
    assert _same(y, y0) and _same(part, part0)
    # the end of the first solve looks at the counters: nothing dead, the handle stops building (K is singular: three
    # iterations are all this asks for)
    K.solve_cg(E.Vec(ctx, mesh.n_vert).set(x - x.mean()), E.Vec(ctx, mesh.n_vert), pc="jacobi", max_it=3)
    after = K.compact_info()
    assert after["valid"] == 0 and after["products_compact"] >= 2, after        # (the solve's own products still read the copy)
    n_compact, n_full = after["products_compact"], after["products_full"]
    y1, part1 = _product(ctx, K, x, 1)
    last = K.compact_info()
    print(f"compact jittered n=12 after the solve: {last}")
    assert last["valid"] == 0 and last["products_compact"] == n_compact and last["products_full"] == n_full + 1, last
    assert _same(y1, y0) and _same(part1, part0)
    # ... also after the next assembly into the same handle
    E.assemble_system(dm, 0, None, E.Vec(ctx, mesh.n_vert).set(np.zeros(mesh.n_vert)),
                      E.Vec(ctx, mesh.n_cell).set(1.0 + np.random.default_rng(3).random(mesh.n_cell)), None, K, None, None)
    y2, _ = _product(ctx, K, x, 1)
    again = K.compact_info()
    assert again["valid"] == 0 and again["products_compact"] == n_compact and again["products_full"] == n_full + 2, again
    assert _same(y2, y0)


# ---- cases 4 and 5: chosen values ---------------------------------------------------------------------------------------
def _chosen(rowptr, col, live_deltas, dead_rows=(), seed=5):
    """CSR values on the pattern: 4 on the diagonal, a random non-zero on the couplings whose column - row is in
    `live_deltas`, exact zeros elsewhere and in the rows `dead_rows`."""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    d = col.astype(np.int64) - row
    val = np.where(np.isin(d, list(live_deltas)), rng.uniform(0.5, 1.5, len(col)) * rng.choice([-1.0, 1.0], len(col)), 0.0)
    val[np.isin(row, list(dead_rows))] = 0.0
    val[d == 0] = 4.0
    return val, row, d


def _expected_live_pairs(val, row, d, slices):
    """What the packing must find: per regular slice the deltas with a non-zero in some row, padded to a pair (None: the
    slice is not regular and keeps what it stores)."""
    per_slice, total = [], 0
    for s, (regular, pairs) in enumerate(slices):
        here = (row >> 6 == s) & (d != 0) & (val != 0.0)
        per_slice.append((len(np.unique(d[here])) + 1) // 2 if regular else None)
        total += per_slice[-1] if regular else pairs
    return per_slice, total


def test_odd_live_count_and_a_slice_without_live_slots(ctx, monkeypatch, cube8):
    from femo_amd import engine as E
    mesh, dm = cube8
    rowptr, col, _ = _stiffness(ctx, dm, mesh).export_csr()
    val, row, d = _chosen(rowptr, col, (-81, -9, -1, 1, 9), dead_rows=range(192, 256))
    per_slice, want = _expected_live_pairs(val, row, d, _slices(dm))
    assert per_slice[3] == 0 and per_slice.count(3) == 6                    # none; five slots, the last pair half padding
    x = _x(mesh.n_vert)
    A = E.Mat(dm).import_csr(val)
    y, part = _product(ctx, A, x, 3)
    info = A.compact_info()
    y0, part0 = _plain(monkeypatch, lambda: _product(ctx, E.Mat(dm).import_csr(val), x, 3))
    print(f"compact chosen values: {info}, pairs per regular slice {per_slice}")
    assert info["valid"] == 1 and info["live_pairs"] == want and info["products_compact"] == 1, (info, want)
    assert _same(y, y0) and _same(part, part0)
    assert _same(y[192:256], x[192:256])                      # identity rows of the scaled operator: y = x
    assert not _same(y[:192], x[:192])


def test_a_slot_dead_in_one_assembly_is_live_in_the_next(ctx, monkeypatch, cube8):
    from femo_amd import engine as E
    mesh, dm = cube8
    rowptr, col, _ = _stiffness(ctx, dm, mesh).export_csr()
    slices = _slices(dm)
    val1, row, d = _chosen(rowptr, col, (-81, -9, -1, 1, 9), seed=5)
    val2, _, _ = _chosen(rowptr, col, (-81, -9, 1, 9, 10, 81, 91), seed=6)   # -1 dies; +81 and two diagonals come alive
    x = _x(mesh.n_vert)
    A = E.Mat(dm).import_csr(val1)
    y1, _ = _product(ctx, A, x, 1)
    info1 = A.compact_info()
    assert info1["live_pairs"] == _expected_live_pairs(val1, row, d, slices)[1], info1
    A.import_csr(val2)                                                        # the same handle
    y2, part2 = _product(ctx, A, x, 1)
    info2 = A.compact_info()
    print(f"compact staleness: first {info1}, second {info2}")
    assert info2["valid"] == 1 and info2["products_compact"] == 2 and info2["products_full"] == 0, info2
    assert info2["live_pairs"] == _expected_live_pairs(val2, row, d, slices)[1] != info1["live_pairs"], info2
    y1_0, _ = _plain(monkeypatch, lambda: _product(ctx, E.Mat(dm).import_csr(val1), x, 1))
    y2_0, part2_0 = _plain(monkeypatch, lambda: _product(ctx, E.Mat(dm).import_csr(val2), x, 1))
    assert _same(y1, y1_0)
    assert _same(y2, y2_0) and _same(part2, part2_0)
    assert not _same(y2, y1)


# ---- case 6 -----------------------------------------------------------------------------------------------------------
def test_not_built_without_regular_slices(ctx, monkeypatch):
    from femo_amd.fea.mesh import createUnitCubeMesh
    mesh = createUnitCubeMesh(8).permuted(seed=7)
    dm = mesh.device(ctx)
    assert dm.info["regular_slices"] == 0
    x = _x(mesh.n_vert)
    K = _stiffness(ctx, dm, mesh)
    y, part = _product(ctx, K, x, 1)
    info = K.compact_info()
    y0, part0 = _plain(monkeypatch, lambda: _product(ctx, _stiffness(ctx, dm, mesh), x, 1))
    assert info == dict(valid=0, slices=0, live_pairs=0, full_pairs=0, products_compact=0, products_full=1), info
    assert _same(y, y0) and _same(part, part0)


def test_not_built_on_two_emulated_ranks(monkeypatch):
    from femo_amd import engine as E
    from femo_amd.dist.partition import rcb_partition
    from tests.test_gpu_emulated_ranks import _local_problem, _reference, _run_ranks
    m = fo.unit_cube_mesh(12, 0.0)
    part = rcb_partition(m.x, 2)
    x_ref, _ = _reference(m)

    def rank_fn(rank, ctx):
        L, dm, A, b, _, _ = _local_problem(ctx, m, part, rank, 2)
        x = E.Vec(ctx, len(L.x))
        info = A.solve_cg(b, x, rtol=1e-14, pc="jacobi")
        return dict(gid=L.vert_global[:L.n_owned], x=x.get(L.n_owned), its=info.iterations, conv=info.converged, compact=A.compact_info())

    def solve():
        out = _run_ranks(2, rank_fn)
        x = np.zeros(m.n_vert)
        for r in out:
            x[r["gid"]] = r["x"]
        return x, out

    x_new, out = solve()
    x_plain, out_plain = _plain(monkeypatch, solve)
    for r, r0 in zip(out, out_plain):
        print(f"compact on two emulated ranks: {r['compact']}, iterations {r['its']} (plain {r0['its']})")
        assert r["conv"] == 1 and r["its"] == r0["its"]
        assert r["compact"]["valid"] == 0 and r["compact"]["products_compact"] == 0 and r["compact"]["slices"] == 0, r["compact"]
        assert r["compact"]["products_full"] >= r["its"], r["compact"]
    assert np.array_equal(x_new, x_plain)                     # the same launches in both runs
    assert np.abs(x_new - x_ref).max() / np.abs(x_ref).max() < 1e-10


# ---- case 7 -----------------------------------------------------------------------------------------------------------
def test_switched_off_nothing_is_built(ctx, monkeypatch, cube8):
    from femo_amd import engine as E
    mesh, dm = cube8
    monkeypatch.setenv("FEMO_SPMV_COMPACT", "0")
    bd = fo.boundary_vertices_box(mesh.x)
    A, b = E.Mat(dm), E.Vec(ctx, mesh.n_vert)
    E.assemble_system(dm, 0, None, E.Vec(ctx, mesh.n_vert).set(np.zeros(mesh.n_vert)), E.Vec(ctx, mesh.n_cell).set(np.ones(mesh.n_cell)),
                      E.DirichletSet(dm, bd, np.zeros(len(bd))), None, A, b)
    _product(ctx, A, _x(mesh.n_vert), 1)
    info = A.solve_cg(b, E.Vec(ctx, mesh.n_vert), rtol=1e-12, pc="jacobi")
    st = A.compact_info()
    assert info.converged == 1 and info.iterations > 0
    assert st["valid"] == 0 and st["slices"] == 0 and st["live_pairs"] == 0 and st["full_pairs"] == 0 and st["products_compact"] == 0, st
    assert st["products_full"] >= 1 + info.iterations, st


# ---- case 8: cycles through the operator surface --------------------------------------------------------------------------
def _cycles(ctx, n, pc, modes):
    """One benchmark cycle per entry of `modes` (True: compacted, False: FEMO_SPMV_COMPACT=0) on one problem, warmed up once:
    (u, dJ/df, J, iteration counts, products on the compacted copy during the cycle) each."""
    from bench import build_problem, one_cycle, source_fields
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    utils_hip.set_context(ctx)
    saved, utils_hip.KSP_OPTIONS["pc"] = utils_hip.KSP_OPTIONS["pc"], pc
    try:
        mesh = createUnitCubeMesh(n)
        sim, fea = build_problem(mesh, device=False)
        f = source_fields(mesh, 1)[0]
        dm = mesh.device(ctx)

        def on_copy():
            return sum(o.compact_info()["products_compact"] for o in gc.get_objects() if isinstance(o, E.Mat) and o.mesh is dm)

        os.environ["FEMO_SPMV_COMPACT"] = "0"
        one_cycle(sim, fea, f)
        out = []
        for compact in modes:
            if compact:
                os.environ.pop("FEMO_SPMV_COMPACT", None)
            else:
                os.environ["FEMO_SPMV_COMPACT"] = "0"
            del utils_hip.LAST_KSP_INFO[:]
            before = on_copy()
            g = np.array(E.host_wait(one_cycle(sim, fea, f)), copy=True)
            out.append((np.array(E.host_wait(sim['u']), copy=True), g, float(np.asarray(sim['l2_functional']).ravel()[0]),
                        [i["iterations"] for i in utils_hip.LAST_KSP_INFO], on_copy() - before))
        return out
    finally:
        os.environ.pop("FEMO_SPMV_COMPACT", None)
        utils_hip.KSP_OPTIONS["pc"] = saved
        utils_hip.clear_workspaces()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), np.finfo(float).tiny))


def test_bpx_cycle_within_the_noise_of_two_plain_runs(ctx):
    plain_a, plain_b, new = _cycles(ctx, 32, "bpx", (False, False, True))
    assert plain_a[4] == 0 and plain_b[4] == 0 and new[4] > sum(new[3]) // 2, (plain_a[4], plain_b[4], new[4], new[3])
    assert new[3] == plain_a[3] == plain_b[3] and sum(new[3]) > 20, (new[3], plain_a[3], plain_b[3])
    for k, name in enumerate(("u", "dJ/df", "J")):
        s0 = _rel(plain_a[k], plain_b[k])
        d = max(_rel(new[k], plain_a[k]), _rel(new[k], plain_b[k]))
        print(f"compact bpx cycle n=32 {name}: plain-plain {s0:.3e}, compact-plain {d:.3e}, bound {8.0 * max(s0, EPS):.3e}")
        assert d <= 8.0 * max(s0, EPS), (name, d, s0)


def test_jacobi_cycle_is_bit_equal(ctx):
    plain, new = _cycles(ctx, 12, "jacobi", (False, True))
    assert plain[4] == 0 and new[4] > sum(new[3]) // 2, (plain[4], new[4], new[3])
    assert new[3] == plain[3] and sum(new[3]) > 20
    assert _same(new[0], plain[0]) and _same(new[1], plain[1]) and new[2] == plain[2]
