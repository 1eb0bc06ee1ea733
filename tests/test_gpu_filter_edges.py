"""GPU tests of the device-built density filter (femo_filter_create: k_f_bin, k_scan, k_f_fill, k_f_sort_buckets, k_f_rows,
k_f_rowsum, k_f_weights, and k_f_apply) at the edges of its build, against the extended-precision brute force of
tests/filter_ref.py.

What the cases reach that the two mesh-centroid shapes of test_gpu_topopt.py do not: more grid cells than one scan chunk
(1024) with empty cells among them, the growth of the cell size (h *= 1.25) when the radius is tiny against the box, a single
cell with dense rows, a direction without extent, a box far from the origin and on its negative side, point counts at the
workgroup (256) and scan-chunk (1024) boundaries, n = 1, coincident points, and distances that equal the radius.

Bounds (eps = 2^-52, m_i = length of row i, W^ = the extended-precision weight; none of them is fitted to the kernels):

  entry    |W_ij - W^_ij| <= eps (4 + 6 m_i W^_ij)
           d_ij carries a few ulp (differences, squares, their sum, the root), r - d one more, the sequential row sum
           S_i up to m_i eps relative, the quotient one.  An entry with |d - r| <= 8 eps r (a *tie* of the reference) may be
           present on one side only and then counts as 0 there.
  row sum  |sum_j W_ij - 1| <= (m_i + 2) eps
  apply    |y_i - y^_i| <= eps (m_i sum_j |W^_ij x_j| + sum_j (4 + 6 m_i W^_ij) |x_j|): the sequential product sum, then
           the entry bound carried through; the same with W^T for the transposed product
  CSR x    the exported matrix times x, summed on the host, differs from apply's result by the first term at most
  W^T      equals W transposed bit for bit (d_ij = d_ji bit for bit, both divided by the same S), on the same pattern

The random cases assert that the reference has no tie at all, so their patterns must be equal outright."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import filter_ref as fref

pytestmark = pytest.mark.gpu

EPS = fref.EPS
LD = np.longdouble
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025)
CASES = (["cells2d", "cells3d", "capped", "onecell", "collinear", "coplanar", "shifted"]
         + ["sizes-%d" % n for n in SIZES] + ["lattice"])


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _case(name):
    """(coordinates, radius, random): fixed seeds; ``random`` cases must be free of ties."""
    rng = np.random.default_rng(11)
    if name == "cells2d":
        return rng.random((2000, 2)), 0.02, True
    if name == "cells3d":
        return rng.random((1500, 3)), 0.08, True
    if name == "capped":
        c = rng.random((300, 2))
        ang = rng.uniform(0.0, 2.0 * np.pi, 20)
        twins = c[rng.choice(300, 20, replace=False)] + 3e-4 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        return np.concatenate([c, twins]), 1e-3, True
    if name == "onecell":
        return rng.random((300, 3)), 2.0, True
    if name == "collinear":
        c = rng.random((500, 2))
        c[:, 1] = 0.375
        return c, 0.01, True
    if name == "coplanar":
        c = rng.random((500, 3))
        c[:, 2] = -0.625
        return c, 0.08, True
    if name == "shifted":
        return rng.random((600, 2)) * 3.0 + np.array([1e6, -2e6]), 0.3, True
    if name.startswith("sizes-"):
        n = int(name[6:])
        c = rng.random((n, 2))
        if n == 2:
            c[1] = c[0]                                     # the same point twice: d = 0 off the diagonal
        return c, float(np.sqrt(10.0 / (np.pi * n))), True
    if name == "lattice":
        gx, gy = np.meshgrid(np.arange(12) * 0.1, np.arange(9) * 0.1, indexing="ij")
        return np.stack([gx.ravel(), gy.ravel()], axis=1), 0.2, False
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The extended-precision filter of a case, computed once and shared (read-only) by everything that needs it."""
    c, r, _ = _case(name)
    R = fref.filter_matrix_ld(c, r)
    W = R.dense()
    W.flags.writeable = False
    m = np.array([len(j) for j in R.cols], dtype=np.int64)
    return R, W, m


def _export(F, transpose=False):
    rowptr, col, val = F.export_csr(transpose=transpose)
    return rowptr.copy(), col.copy(), val.copy()


def _ratio(err, bound):
    return float((err / bound).max())


def check_filter(name, n, rowptr, col, val, rowptrT, colT, valT, x, y, yT, y1):
    """Every assertion on one built filter; the device enters only through the arrays.  Returns the measured worst
    ratios of error to bound (printed by the test: run with -s to read them)."""
    R, Wref, m = _reference(name)
    random = _case(name)[2]
    nnz = int(rowptr[-1])
    # ---- pattern
    assert rowptr.shape == (n + 1,) and rowptr[0] == 0 and nnz == col.size == val.size
    assert np.all(np.diff(rowptr) >= 1)
    for i in range(n):
        row = col[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(row) > 0), "row %d not strictly ascending" % i
        assert row[0] >= 0 and row[-1] < n and i in row, "row %d: column out of range or diagonal missing" % i
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    P = np.zeros((n, n), bool)
    P[rows, col] = True
    Pref = Wref > 0
    for i in range(n):
        Pref[i, R.cols[i]] = True                            # a weight of exactly 0 (d == r) is still an entry
    differ = np.argwhere(P != Pref)
    if random:
        assert len(R.ties) == 0, "the seed produced a tie: choose another"
        assert np.array_equal(P, Pref)
    else:
        assert all((int(i), int(j)) in R.ties for i, j in differ)
        assert len(differ) <= len(R.ties)
    assert np.array_equal(P, P.T)
    # ---- values
    W = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    Wd = W.toarray()
    bound = EPS * (4.0 + 6.0 * m[:, None].astype(LD) * Wref)
    err = np.abs(Wd.astype(LD) - Wref)
    ratios = {"entry": _ratio(err, bound)}
    assert np.all(err <= bound), "entry error %.3g of its bound" % ratios["entry"]
    if name == "capped":
        single = np.nonzero(m == 1)[0]
        assert single.size > 0 and np.any(m == 2)
        assert np.all(Wd[single, single] == 1.0)             # a row of its diagonal alone: r / r
    # ---- rows sum to one
    rs = np.abs(Wd.astype(LD).sum(axis=1) - 1)
    ratios["rowsum"] = _ratio(rs, (m + 2) * EPS)
    assert np.all(rs <= (m + 2) * EPS)
    # ---- transpose, bit for bit
    assert np.array_equal(rowptrT, rowptr) and np.array_equal(colT, col)
    WT = sp.csr_matrix((valT, colT, rowptrT), shape=(n, n))
    assert np.array_equal(WT.toarray(), Wd.T)
    # ---- apply
    ax = np.abs(x).astype(LD)
    for tag, Wr, out, M in (("apply", Wref, y, W), ("applyT", Wref.T, yT, WT)):
        first = EPS * m * (np.abs(Wr) @ ax)
        b = first + EPS * ((4.0 + 6.0 * m[:, None].astype(LD) * Wr) * (P | Pref)) @ ax
        e = np.abs(out.astype(LD) - Wr @ x.astype(LD))
        ratios[tag] = _ratio(e, b)
        assert np.all(e <= b), "%s error %.3g of its bound" % (tag, ratios[tag])
        assert np.all(np.abs((M @ x).astype(LD) - out) <= first)          # exported CSR times x
    r1 = np.abs(y1.astype(LD) - 1)
    ratios["ones"] = _ratio(r1, (m + 2) * EPS)
    assert np.all(r1 <= (m + 2) * EPS)
    return ratios, len(R.ties), len(differ)


@pytest.mark.parametrize("name", CASES)
def test_filter_edge(gpu, name):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceFilter
    c, r, _ = _case(name)
    n = c.shape[0]
    F = DeviceFilter(gpu, c, r)
    rowptr, col, val = _export(F)
    rowptrT, colT, valT = _export(F, transpose=True)
    assert F.nnz == rowptr[-1]
    x = np.random.default_rng(12).standard_normal(n)
    vx, vy = Vec(gpu, n).set(x), Vec(gpu, n)
    y = np.array(F.apply(vx, vy).get())
    yT = np.array(F.apply(vx, vy, transpose=True).get())
    y1 = np.array(F.apply(Vec(gpu, n).fill(1.0), vy).get())
    ratios, ties, differ = check_filter(name, n, rowptr, col, val, rowptrT, colT, valT, x, y, yT, y1)
    print("filter edge %-10s n %4d nnz %6d ties %3d differing %3d  worst error / bound: %s"
          % (name, n, rowptr[-1], ties, differ, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    # determinism: the bucket fill uses atomics, the per-cell sort hides their order
    G = DeviceFilter(gpu, c, r)
    for a, b in zip(_export(G), (rowptr, col, val)):
        assert np.array_equal(a, b)


def test_nonfinite_coordinates_are_refused(gpu):
    """NaN in the first point, NaN further in, +-inf: an error that names the cause, before any device work (without the
    check the host loop over the cell size does not end on the first and the third, and the second gave its point an empty
    row and a filtered density of 0).  The context stays usable."""
    from femo_amd._lib import FemoError
    from femo_amd.fea.elasticity import DeviceFilter
    base = np.random.default_rng(13).random((64, 2))
    for idx, bad in (((0, 0), np.nan), ((0, 1), np.nan), ((40, 1), np.nan), ((17, 0), np.inf), ((63, 1), -np.inf)):
        c = base.copy()
        c[idx] = bad
        with pytest.raises(FemoError, match="finite"):
            DeviceFilter(gpu, c, 0.2)
    c3 = np.random.default_rng(14).random((30, 3))
    c3[29, 2] = np.nan
    with pytest.raises(FemoError, match="finite"):
        DeviceFilter(gpu, c3, 0.3)
    F = DeviceFilter(gpu, base, 0.2)
    rowptr, col, val = F.export_csr()
    R = fref.filter_matrix_ld(base, 0.2)
    assert not R.ties
    assert np.array_equal(col, np.concatenate(R.cols))
    m = np.repeat([len(j) for j in R.cols], [len(j) for j in R.cols])
    Wref = np.concatenate(R.weights)
    assert np.all(np.abs(val.astype(LD) - Wref) <= EPS * (4 + 6 * m * Wref))
