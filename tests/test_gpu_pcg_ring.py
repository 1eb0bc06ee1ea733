"""Kept search directions in the one-rank merged BPX-PCG (csrc/solver.hip: ensure_ring, k_pcg_flush; csrc/bpx.hip: MergedCarry
without the x stream).  The loop leaves direction k in slot k % R of a ring and forms x^ = x^_0 + sum_k alpha_k p_k with one fma
per direction in the order of the iterations, when the ring is full and at the end of the solve -- the same additions in the same
order as the per-iteration update (FEMO_PCG_RING=0), which uses the same fma.  What is left between the two is the noise of the
loop itself: the brick restriction sums with atomics, so two runs of ONE loop differ in the last bits.

Per case: three solves with FEMO_PCG_RING=0 give s0, their largest pairwise max-norm distance relative to the largest entry;
every variant (unset -- the per-iteration update again on meshes this small: the default ring is for meshes of millions of
rows --, 32 slots, and 3 and 4 slots: several wraps per solve) must reproduce iteration count and convergence flag and lie
within 8 x max(s0, 2.3e-16) of each baseline solution (2.3e-16: one rounding; 8 x: DESIGN_LOG R13 records up to 5.3 between nine-pair and three-pair maxima of this noise).

After every solve the library is asked what ran (DeviceMesh.pcg_info, femo_mesh_pcg_info of femo_hip_test.h): the merged loop
(femo_pc_merged_ok), on exactly the slots the variant names, with at least one flush per wrap and one at the end.

Shapes on which the merged loop runs on one rank (DESIGN_LOG R13): jittered 32^3 (35,937 rows, odd: the lone last entry of the
carriers' pair loop; separable chain), 31^3 (32,768 rows, even), 64^2 (no chain), 64^3 (flattened chain)."""
import itertools

import numpy as np
import pytest

from oracle import femo_oracle as fo
from tests.test_gpu_bpx import _poisson_system

pytestmark = pytest.mark.gpu

RING_VARIANTS = (None, "32", "3", "4")
EPS = 2.3e-16


def _solve(monkeypatch, ctx, A, b, ring, x0=None, dm=None, **kw):
    from femo_amd import engine as E
    if ring is None:
        monkeypatch.delenv("FEMO_PCG_RING", raising=False)
    else:
        monkeypatch.setenv("FEMO_PCG_RING", ring)
    x = E.Vec(ctx, b.n)
    if x0 is not None:
        x.set(x0)
    info = A.solve_cg(b, x, pc="bpx", zero_guess=x0 is None, **kw)
    monkeypatch.delenv("FEMO_PCG_RING", raising=False)
    if dm is not None:
        # what ran, asked of the library: the merged loop, on the ring this variant names (these meshes lie far below the row
        # count from which the default keeps directions: unset is the per-iteration update here), flushed as often as it wraps
        st = dm.pcg_info()
        want = 0 if ring is None else int(ring)
        assert st["merged"] and st["ring_slots"] == want, (ring, st)
        if want == 0 or info.iterations == 0:
            assert st["flushes"] == 0, (ring, st)
        else:
            assert st["flushes"] >= 1 + (info.iterations - 1) // (want - 1), (ring, info.iterations, st)
    return x.get().copy(), info.iterations, info.converged


def _dist(a, b, scale):
    return np.abs(a - b).max() / scale


def _check_ring_against_update(monkeypatch, ctx, dm, A, b, label, x0=None, **kw):
    """Returns (baseline solutions, iterations) after asserting every ring variant against the per-iteration update."""
    assert dm.pcg_info()["merged"], label               # femo_pc_merged_ok: BPX-PCG solves on this mesh take the merged loop
    short = dm.pcg_info()["ring_short"]
    base = [_solve(monkeypatch, ctx, A, b, "0", x0, dm, **kw) for _ in range(3)]
    its, conv = base[0][1], base[0][2]
    assert all(r[1] == its and r[2] == conv for r in base), [(r[1], r[2]) for r in base]
    scale = max(np.abs(base[0][0]).max(), np.finfo(float).tiny)
    s0 = max(_dist(p[0], q[0], scale) for p, q in itertools.combinations(base, 2))
    bound = 8.0 * max(s0, EPS)
    for ring in RING_VARIANTS:
        xr, it_r, conv_r = _solve(monkeypatch, ctx, A, b, ring, x0, dm, **kw)
        d = max(_dist(xr, r[0], scale) for r in base)
        print(f"pcg_ring {label} ring={ring}: iterations {it_r} (baseline {its}), converged {conv_r}, s0 {s0:.3e}, distance {d:.3e}, bound {bound:.3e}")
        assert it_r == its and conv_r == conv, (label, ring, it_r, its, conv_r, conv)
        assert d <= bound, (label, ring, d, s0)
    assert dm.pcg_info()["ring_short"] == short         # no solve got fewer slots than it asked for
    return [r[0] for r in base], its, conv


@pytest.fixture(scope="module")
def cube32(ctx):
    m = fo.unit_cube_mesh(32, 0.2)
    assert m.n_vert == 35937
    return (m,) + _poisson_system(ctx, m, seed=7)


@pytest.mark.parametrize("d,n,jit,rows", [(3, 31, 0.0, 32768), (2, 64, 0.2, 4225), (3, 64, 0.1, 274625)])
def test_ring_is_the_per_iteration_update(ctx, monkeypatch, d, n, jit, rows):
    m = fo.unit_square_mesh(n, jit) if d == 2 else fo.unit_cube_mesh(n, jit)
    assert m.n_vert == rows
    dm, bc, A, b = _poisson_system(ctx, m, seed=n)
    _, its, conv = _check_ring_against_update(monkeypatch, ctx, dm, A, b, f"{d}-D n={n}", rtol=1e-12)
    assert conv == 1 and its > 8               # more than two wraps of the 3- and 4-slot rings


def test_ring_on_an_odd_row_count(ctx, monkeypatch, cube32):
    m, dm, bc, A, b = cube32
    _, its, conv = _check_ring_against_update(monkeypatch, ctx, dm, A, b, "3-D n=32", rtol=1e-12)
    assert conv == 1 and 20 <= its <= 40


def test_ring_with_a_guess_and_an_absolute_tolerance(ctx, monkeypatch, cube32):
    m, dm, bc, A, b = cube32
    from femo_amd import engine as E
    x = E.Vec(ctx, m.n_vert)
    full = A.solve_cg(b, x, rtol=1e-12, pc="bpx")
    assert full.converged == 1
    x0 = x.get() * (1.0 + 1e-3 * np.random.default_rng(1).standard_normal(m.n_vert))
    _, its, conv = _check_ring_against_update(monkeypatch, ctx, dm, A, b, "3-D n=32 guess+atol", x0=x0, rtol=1e-14, atol=1e-7 * full.rhs_norm)
    assert conv == 1 and 4 < its < full.iterations + 40


def test_ring_when_the_right_hand_side_is_below_atol(ctx, monkeypatch, cube32):
    m, dm, bc, A, b = cube32
    from femo_amd import engine as E
    x = E.Vec(ctx, m.n_vert)
    rhs_norm = A.solve_cg(b, x, rtol=1e-2, pc="bpx").rhs_norm
    base, its, conv = _check_ring_against_update(monkeypatch, ctx, dm, A, b, "3-D n=32 below atol", rtol=1e-12, atol=10.0 * rhs_norm)
    assert its == 0 and conv == 1
    # no iteration: x is the zero guess with the identity rows solved (boundary values), identical in every run
    bd = fo.boundary_vertices_box(m.x)
    inner = np.ones(m.n_vert, bool)
    inner[bd] = False
    assert np.all(base[0][inner] == 0.0) and np.abs(base[0][bd]).max() > 0.0
    for ring in RING_VARIANTS:
        xr, _, _ = _solve(monkeypatch, ctx, A, b, ring, dm=dm, rtol=1e-12, atol=10.0 * rhs_norm)
        assert np.array_equal(xr, base[0])


def test_ring_when_max_it_ends_the_solve(ctx, monkeypatch, cube32):
    m, dm, bc, A, b = cube32
    _, its, conv = _check_ring_against_update(monkeypatch, ctx, dm, A, b, "3-D n=32 max_it=5", rtol=1e-12, max_it=5)
    assert its == 5 and conv == 0
