"""Rows of more than 14 off-diagonal entries on the GPU (meshes of tests/wide_meshes.py; their host topology is pinned
in tests/test_wide_rows_host.py): every row-length branch of the assembly dispatch, of the Dirichlet row mask, of the
SELL-64 product in its three slice classes, of the transposition map and of the CSR exports, plus the Krylov solves and the
elasticity blocks on such rows.  Each case asserts the ``max_rowlen`` / slice-class precondition that puts it on its side
of a threshold ("Row-length dispatch")."""
import numpy as np
import pytest

import wide_meshes as W
from oracle import femo_oracle as fo

pytestmark = pytest.mark.gpu

RTOL = 1e-12          # relative, max norm: the bar of the assembly comparisons of test_gpu_engine.py
CAPACITY = "exceeds the LDS strip capacity"


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def _cube6():
    m = fo.unit_cube_mesh(6)
    return m.x, m.conn


def _joined(k):
    return W.union(_cube6(), W.bipyramid(k), (3.0, 0.0, 0.0))


def _renumbered(xc, perm_of):
    x, conn = xc
    return W.renumber(x, conn, perm_of(len(x)))


# name -> construction.  fan<k>: 2-D, hub row of k entries; bip<k>: 3-D, hub row of k + 2 entries.
MESHES = {
    **{f"fan{k}": (lambda k=k: W.fan(k, 6)) for k in (8, 9, 16, 17, 40, 62, 63, 64, 65, 84, 85)},
    **{f"bip{k}": (lambda k=k: W.bipyramid(k)) for k in (13, 14, 30, 31, 60, 61, 62, 63)},
    "cube6_bip13": lambda: _joined(13), "cube6_bip14": lambda: _joined(14), "cube6_bip30": lambda: _joined(30),
    "cube5_8": lambda: W.cube5(8),
    "fan40x8_hub_first": lambda: W.fan(40, 8),
    "fan40x8_hub_middle": lambda: _renumbered(W.fan(40, 8), lambda n: W.move_vertex(n, 0, n // 2)),
    "fan40x8_hub_last": lambda: _renumbered(W.fan(40, 8), lambda n: W.move_vertex(n, 0, n - 1)),
    "fan40x8_random": lambda: _renumbered(W.fan(40, 8), lambda n: W.random_numbering(n, 5)),
    # seed 5, the numbering pinned in test_wide_rows_host.py, leaves the hub in a slice of 16-bit columns; seed 12 gives the hub
    # row itself a column more than 32767 away (asserted from the pattern in _product_preconditions)
    "fan40x900_random": lambda: _renumbered(W.fan(40, 900), lambda n: W.random_numbering(n, 12)),
    "fan40x900_rings": lambda: W.fan(40, 900),
    "strip32760": lambda: W.strip(32760, 4, 1),
    "strip32764": lambda: W.strip(32764, 4, 1),
}

# (mesh, max_rowlen): one case on each side of every threshold of femo_launch_system / femo_launch_residual / femo_bc_create
CASES_3D = [("cube6_bip13", 15), ("bip14", 16), ("cube6_bip14", 16), ("cube5_8", 18), ("bip30", 32), ("cube6_bip30", 32),
            ("bip31", 33), ("bip60", 62), ("bip61", 63), ("bip62", 64)]
CASES_2D = [("fan8", 8), ("fan9", 9), ("fan16", 16), ("fan17", 17), ("fan40", 40), ("fan62", 62), ("fan63", 63), ("fan84", 84)]
# the forms that accumulate in k_jacobian's strip: cap 32, 64, 64 entries per thread
CASES_STRIP = [("cube5_8", 18), ("bip31", 33), ("bip62", 64), ("fan17", 17), ("fan40", 40), ("fan64", 64)]

_CACHE = {}


class _Case:
    """Everything the tests of one mesh share, computed once and left unchanged."""

    def __init__(self, ctx, name):
        from femo_amd import engine as E
        self.name = name
        x, conn = MESHES[name]()
        self.om = om = fo.OMesh(x.shape[1], x, conn)
        self.n, self.nc, self.d = om.n_vert, om.n_cell, om.tdim
        self.dm = E.DeviceMesh(ctx, x, conn)
        self.info = self.dm.info
        rng = np.random.default_rng(11)
        self.u, self.f = rng.standard_normal(self.n), rng.standard_normal(self.nc)
        self.gvals = rng.standard_normal(self.n)                     # Dirichlet value of vertex v, whichever set holds it
        self.U, self.F = E.Vec(ctx, self.n).set(self.u), E.Vec(ctx, self.nc).set(self.f)
        self.bmask = fo.boundary_facets(om)
        on = np.zeros(self.n, bool)
        for k in range(self.d + 1):
            on[np.delete(conn, k, axis=1)[((self.bmask >> k) & 1) != 0].ravel()] = True
        self.boundary = np.nonzero(on)[0].astype(np.int32)
        self._K = None

    @property
    def K(self):
        if self._K is None:
            self._K = fo.stiffness(self.om)
        return self._K

    @property
    def hub(self):
        return int(np.argmax(np.diff(self.K.indptr)))

    def hub_neighbours(self):
        h = self.hub
        c = self.K.indices[self.K.indptr[h]:self.K.indptr[h + 1]]
        return c[c != h]                                             # sorted: position = bit of the hub's row mask

    def sets(self):
        """The three Dirichlet sets: the topological boundary; (i) the set also holds the hub's highest-numbered neighbours
        -- slots 32 ... of its row where it has that many, the upper half otherwise -- and, so that the mask has both kinds
        of bits, none of its other neighbours; (ii) the boundary and the hub itself."""
        nb = self.hub_neighbours()
        s0 = 32 if len(nb) > 32 else len(nb) // 2
        low, high = nb[:s0], nb[s0:]
        return {"boundary": self.boundary,
                "hub_high": np.union1d(np.setdiff1d(self.boundary, low), high).astype(np.int32),
                "hub": np.union1d(self.boundary, [self.hub]).astype(np.int32)}

    def slice_widths(self):
        """Stored entries per row of every slice, by the rules of the host topology: the union of the column offsets of a
        full slice where it is no larger than min(max_rowlen, 32) and stays inside the mesh (regular slice), the longest row
        otherwise; rounded up to a whole pair.  Checked against the library's own totals."""
        rp, col = self.K.indptr, self.K.indices
        rows = np.repeat(np.arange(self.n), np.diff(rp))
        off = col.astype(np.int64) - rows
        keep = off != 0
        rows, off = rows[keep], off[keep]
        ns = (self.n + 63) // 64
        rl = np.bincount(rows, minlength=ns * 64)
        dcap = min(self.info["max_rowlen"], 32)
        width, regular = np.zeros(ns, np.int64), 0
        for s in range(ns):
            w = rl[s * 64:(s + 1) * 64].max()
            if (s + 1) * 64 <= self.n:
                D = np.unique(off[(rows >= s * 64) & (rows < (s + 1) * 64)])
                if 0 < len(D) <= dcap and s * 64 + D[0] >= 0 and s * 64 + 63 + D[-1] < self.n:
                    w, regular = len(D), regular + 1
            width[s] = (w + 1) & ~1
        assert regular == self.info["regular_slices"] and 64 * width.sum() == self.info["sell_entries"]
        return width


def _case(ctx, name):
    if name not in _CACHE:
        _CACHE[name] = _Case(ctx, name)
    return _CACHE[name]


def _ds(E, c, dofs):
    return E.DirichletSet(c.dm, dofs, c.gvals[dofs])


# ----------------------------------------------------------------------------------------------- assembly dispatch ----
@pytest.mark.parametrize("name,rowlen", CASES_3D + CASES_2D)
def test_linear_jacobian(ctx, name, rowlen):
    """assemble_jacobian of the linear form: k_poisson_system_lds at every width, its LDS request beyond 64 KiB from 34
    (3-D) / 44 (2-D) entries, the 64-bit row mask up to 62 entries and the byte mask beyond."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    K = c.K
    rowptr, col = c.dm.pattern_csr()
    assert np.array_equal(rowptr, K.indptr) and np.array_equal(col, K.indices)
    J = E.Mat(c.dm)
    E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, J)
    Kg = J.to_scipy()
    assert np.array_equal(Kg.indices, K.indices)
    e = _rel(Kg.data, K.data)
    print(f"{name}: dR/du {e:.2e}")
    assert e < RTOL
    assert abs(Kg - Kg.T).max() == 0.0
    for label, dofs in c.sets().items():
        A = E.Mat(c.dm)
        E.assemble_jacobian(c.dm, 0, None, c.U, c.F, _ds(E, c, dofs), A)
        Ag, Ao = A.to_scipy(), fo.eliminate_bc(K, dofs)
        e = _rel(Ag.data, Ao.data)
        print(f"{name}: A, set {label} ({len(dofs)} dofs) {e:.2e}")
        assert np.array_equal(Ag.indices, Ao.indices) and e < RTOL
        assert abs(Ag - Ag.T).max() == 0.0


def test_hub_mask_bits_32_to_61(ctx):
    """The precondition of the row-mask cases, from the pattern: with set (i) the hub row of fan62 has exactly the bits
    32 ... 61 of its mask set, and the hub row of bip60 (62 entries) likewise."""
    for name in ("fan62", "bip60"):
        c = _case(ctx, name)
        nb, dofs = c.hub_neighbours(), c.sets()["hub_high"]
        assert len(nb) == 62 and c.hub not in dofs
        assert [k for k in range(62) if nb[k] in dofs] == list(range(32, 62))


@pytest.mark.parametrize("name,rowlen", CASES_3D + CASES_2D)
def test_linear_system_combinations(ctx, name, rowlen):
    """The three combinations the operators ask for -- A + rhs, dR/du + A, rhs only -- against the separate calls and the
    oracle: k_poisson_system_pipe<3, 14> / <3, 16> / <2, 8> up to 14 / 16 / 8 entries with a row mask, k_poisson_system_lds
    beyond."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    K = c.K
    R = fo.residual(c.om, c.u, c.f)
    J = E.Mat(c.dm)
    E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, J)
    Jd = J.to_scipy().data
    B = E.Vec(ctx, c.n)
    E.assemble_system(c.dm, 0, None, c.U, c.F, None, None, None, B)              # rhs only, no set: the residual
    assert _rel(B.get(), R) < RTOL
    for label, dofs in c.sets().items():
        ds = _ds(E, c, dofs)
        A = E.Mat(c.dm)
        E.assemble_jacobian(c.dm, 0, None, c.U, c.F, ds, A)
        Ad = A.to_scipy().data
        b_ref = fo.newton_rhs(K, R, c.u, dofs, c.gvals[dofs])
        A1, B1 = E.Mat(c.dm), E.Vec(ctx, c.n)
        E.assemble_system(c.dm, 0, None, c.U, c.F, ds, None, A1, B1)             # A + rhs
        e = (_rel(A1.to_scipy().data, Ad), _rel(B1.get(), b_ref))
        J2, A2 = E.Mat(c.dm), E.Mat(c.dm)
        E.assemble_system(c.dm, 0, None, c.U, c.F, ds, J2, A2, None)             # dR/du + A
        e += (_rel(J2.to_scipy().data, Jd), _rel(A2.to_scipy().data, Ad))
        B3 = E.Vec(ctx, c.n)
        E.assemble_system(c.dm, 0, None, c.U, c.F, ds, None, None, B3)           # rhs only
        e += (_rel(B3.get(), b_ref),)
        print(f"{name}, set {label}: " + " ".join(f"{v:.2e}" for v in e))
        assert max(e) < RTOL
        for M in (A1, J2, A2):
            Mg = M.to_scipy()
            assert abs(Mg - Mg.T).max() == 0.0
        assert _rel(A1.to_scipy().data, fo.eliminate_bc(K, dofs).data) < RTOL


@pytest.mark.parametrize("name,rowlen", CASES_3D + CASES_2D)
def test_linear_residual_and_right_hand_sides(ctx, name, rowlen):
    """assemble_residual (the pipelined kernel up to 16 / 8 entries, FEMO_ROW_WALK beyond), newton_rhs, newton_rhs_linear
    and bc_apply_rhs."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    K = c.K
    R_ref = fo.residual(c.om, c.u, c.f)
    R = E.Vec(ctx, c.n)
    E.assemble_residual(c.dm, 0, None, c.U, c.F, R)
    e = _rel(R.get(), R_ref)
    print(f"{name}: residual {e:.2e}")
    assert e < RTOL
    J = E.Mat(c.dm)
    E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, J)
    B = E.Vec(ctx, c.n)
    assert _rel(E.newton_rhs_linear(J, c.F, c.U, None, B).get(), R_ref) < RTOL
    for label, dofs in c.sets().items():
        ds = _ds(E, c, dofs)
        b_ref = fo.newton_rhs(K, R_ref, c.u, dofs, c.gvals[dofs])
        e = (_rel(E.newton_rhs(J, R, c.U, ds, B).get(), b_ref),)
        e += (_rel(E.newton_rhs_linear(J, c.F, c.U, ds, B).get(), b_ref),)
        B.set(R_ref)
        ref3 = R_ref.copy()
        ref3[dofs] = c.u[dofs] - c.gvals[dofs]
        e += (_rel(E.bc_apply_rhs(ds, c.U, B).get(), ref3),)
        print(f"{name}, set {label}: " + " ".join(f"{v:.2e}" for v in e))
        assert max(e) < RTOL


@pytest.mark.parametrize("facets", [False, True])
@pytest.mark.parametrize("name,rowlen", CASES_STRIP)
def test_nonlinear_form(ctx, name, rowlen, facets):
    """Nonlinear Poisson (pde = 1), with and without the Nitsche facets: k_jacobian with strips of 32 and 64 entries."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    cap = 16
    while cap < rowlen:
        cap *= 2
    assert cap == {17: 32, 18: 32, 33: 64, 40: 64, 64: 64}[rowlen]
    u = 0.7 * c.u
    uex = fo.u_exact_nl(c.om.x)
    bm = c.bmask if facets else np.zeros(c.nc, np.uint8)
    c.dm.set_boundary_facets(bm if facets else None)
    try:
        U, UEX = E.Vec(ctx, c.n).set(u), E.Vec(ctx, c.n).set(uex)
        beta = 10.0
        r_ref, J_ref = fo.nl_residual(c.om, u, c.f, uex, bm, beta), fo.nl_jacobian(c.om, u, bm, beta)
        R = E.assemble_residual(c.dm, 1, [beta], U, c.F, E.Vec(ctx, c.n), aux=UEX)
        J = E.assemble_jacobian(c.dm, 1, [beta], U, c.F, None, E.Mat(c.dm), aux=UEX)
        Jg = J.to_scipy()
        e = (_rel(R.get(), r_ref), _rel(Jg.data, J_ref.data))
        J2, B = E.Mat(c.dm), E.Vec(ctx, c.n)
        E.assemble_system(c.dm, 1, [beta], U, c.F, None, J2, None, B, aux=UEX)
        e += (_rel(B.get(), r_ref), _rel(J2.to_scipy().data, J_ref.data))
        # with a Dirichlet set that holds the hub's upper neighbours
        dofs = c.sets()["hub_high"]
        A = E.assemble_jacobian(c.dm, 1, [beta], U, c.F, _ds(E, c, dofs), E.Mat(c.dm), aux=UEX)
        e += (_rel(A.to_scipy().data, fo.eliminate_bc(J_ref, dofs).data),)
        print(f"{name}, facets {facets}: " + " ".join(f"{v:.2e}" for v in e))
        assert np.array_equal(Jg.indices, J_ref.indices) and max(e) < RTOL
    finally:
        c.dm.set_boundary_facets(None)


@pytest.mark.parametrize("name,rowlen", CASES_STRIP)
def test_mass_form(ctx, name, rowlen):
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    M = E.assemble_jacobian(c.dm, 2, None, None, None, None, E.Mat(c.dm))
    Mg, Mo = M.to_scipy(), fo.mass_matrix(c.om)
    e = _rel(Mg.data, Mo.data)
    print(f"{name}: mass {e:.2e}")
    assert np.array_equal(Mg.indices, Mo.indices) and e < RTOL
    Y = M.mult(c.U, E.Vec(ctx, c.n))
    assert _rel(Y.get(), Mo @ c.u) < RTOL


@pytest.mark.parametrize("name,rowlen", [("fan9", 9), ("fan40", 40), ("cube5_8", 18), ("bip62", 64)])
def test_residual_as_the_first_pass_over_a_mesh(ctx, name, rowlen):
    """FEMO_ROW_WALK reads the visit records that the matrix assemblies build on their first pass: a residual that comes first
    has to build them itself.  A mesh of its own, not the shared one, so that nothing has run on it."""
    from femo_amd import engine as E
    x, conn = MESHES[name]()
    om = fo.OMesh(x.shape[1], x, conn)
    dm = E.DeviceMesh(ctx, x, conn)
    assert dm.info["max_rowlen"] == rowlen and rowlen > (16 if om.tdim == 3 else 8)
    rng = np.random.default_rng(13)
    u, f = rng.standard_normal(om.n_vert), rng.standard_normal(om.n_cell)
    R = E.assemble_residual(dm, 0, None, E.Vec(ctx, om.n_vert).set(u), E.Vec(ctx, om.n_cell).set(f), E.Vec(ctx, om.n_vert))
    assert _rel(R.get(), fo.residual(om, u, f)) < RTOL


# -------------------------------------------------------------------------------------------------------- limits ----
def _all_assemblies_raise(ctx, c, pdes):
    from femo_amd import engine as E
    U, UEX = c.U, E.Vec(ctx, c.n).set(fo.u_exact_nl(c.om.x))
    for pde in pdes:
        J, B = E.Mat(c.dm), E.Vec(ctx, c.n)
        with pytest.raises(E.FemoError, match=CAPACITY):
            E.assemble_jacobian(c.dm, pde, [10.0], U, c.F, None, J, aux=UEX)
        with pytest.raises(E.FemoError, match=CAPACITY):
            E.assemble_system(c.dm, pde, [10.0], U, c.F, None, J, None, None if pde == 2 else B, aux=UEX)


@pytest.mark.parametrize("name,rowlen", [("bip63", 65), ("fan85", 85)])
def test_rows_beyond_the_capacity_are_refused(ctx, name, rowlen):
    """65 entries in 3-D, 85 in 2-D: no form assembles a matrix, the refusal is made on the host before any launch, and the
    context goes on working.  (The residuals keep no strip and have no such limit.)"""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    _all_assemblies_raise(ctx, c, (0, 1, 2))
    R = E.assemble_residual(c.dm, 0, None, c.U, c.F, E.Vec(ctx, c.n))
    assert _rel(R.get(), fo.residual(c.om, c.u, c.f)) < RTOL
    _a_small_mesh_still_assembles(ctx)


@pytest.mark.parametrize("name,rowlen", [("fan65", 65), ("fan84", 84)])
def test_strip_forms_stop_at_64_entries_in_2d(ctx, name, rowlen):
    """The 2-D row neighbourhood of the linear form fits in LDS up to 84 entries (test_linear_jacobian[fan84]); the strip of
    the nonlinear and mass forms holds 64 entries per thread in either dimension, the next size would be 256 KiB."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    assert c.info["max_rowlen"] == rowlen
    _all_assemblies_raise(ctx, c, (1, 2))
    J = E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, E.Mat(c.dm))
    assert _rel(J.to_scipy().data, c.K.data) < RTOL
    _a_small_mesh_still_assembles(ctx)


def _a_small_mesh_still_assembles(ctx):
    from femo_amd import engine as E
    m = fo.unit_cube_mesh(3, 0.2)
    dm = E.DeviceMesh(ctx, m.x, m.conn)
    J = E.assemble_jacobian(dm, 0, None, None, None, None, E.Mat(dm))
    assert _rel(J.to_scipy().data, fo.stiffness(m).data) < RTOL


# -------------------------------------------------------------------------------------------------- SELL product ----
PRODUCT_MESHES = ["cube5_8", "fan40x8_hub_first", "fan40x8_hub_middle", "fan40x8_hub_last", "fan40x8_random",
                  "fan40x900_random", "fan40x900_rings", "bip30", "bip31", "bip62", "bip61", "strip32760", "strip32764"]


def _product_preconditions(c):
    """What puts the mesh on its branch of the product, asserted from the pattern and the library's own counts."""
    info, name = c.info, c.name
    width = c.slice_widths()
    K = c.K
    rows = np.repeat(np.arange(c.n), np.diff(K.indptr))
    far = np.unique(rows[np.abs(K.indices.astype(np.int64) - rows) > 32767] // 64)        # slices of 32-bit columns
    hub_slice = c.hub // 64
    if name == "cube5_8":
        assert info["regular_slices"] == 7 and np.count_nonzero(width == 18) >= 7      # 9 pairs: one pass of the loop + 1
    if name.startswith("fan40x8"):
        assert info["regular_slices"] + info["short_slices"] == info["n_slices"] == 6      # every irregular slice is short
        assert (info["regular_slices"] == 0) == (name == "fan40x8_random")
        assert width[hub_slice] == 40         # wider than a regular slice can be: a short slice of 20 pairs, two passes + 4
        assert c.hub == {"first": 0, "middle": c.n // 2, "last": c.n - 1}.get(name.split("_")[-1], c.hub)
    if name == "fan40x8_hub_last":
        assert c.n % 64 == 1 and hub_slice == info["n_slices"] - 1                      # ragged last slice, the hub alone in it
    if name == "fan40x900_random":
        assert info["regular_slices"] == 0 and info["n_slices"] == 563 and info["short_slices"] == 563 - len(far) == 462
        assert np.abs(c.hub_neighbours().astype(np.int64) - c.hub).max() > 32767       # in the hub's own row
        assert hub_slice in far and width[hub_slice] == 40                              # the 32-bit class, 20 pairs
    if name == "fan40x900_rings":
        assert info["regular_slices"] == 560 and width[0] == 40 and len(far) == 0       # hub slice: 16-bit class
    if name in ("bip30", "bip31", "bip62", "bip61"):
        assert int(np.diff(K.indptr).max()) - 1 == {"bip30": 32, "bip31": 33, "bip62": 64, "bip61": 63}[name]
        assert info["regular_slices"] == 0 and info["short_slices"] == info["n_slices"]
    if name == "bip61":
        assert c.n == 64 and info["n_slices"] == 1
    if name == "bip62":
        assert c.n == 65 and info["n_slices"] == 2                                      # a second slice of one row
    if name == "strip32760":
        d = K.indices.astype(np.int64) - rows
        assert d.max() == 32767 and d.min() == -32767 and info["short_slices"] == info["n_slices"] == 1024
    if name == "strip32764":
        assert info["short_slices"] == 0 and info["regular_slices"] == 0 and len(far) == 1024
    return width


def _check_product(ctx, c, M, width, label):
    """mult and mult(transpose=True) against the product of the EXPORTED values in extended precision, row by row within
    (n_i + 2) 2^-53 (|A| |u|)_i, n_i the stored entries per row of the row's slice: n_i + 1 terms (the diagonal too) summed
    in sequence, each product and each sum rounded once."""
    from femo_amd import engine as E
    A = M.to_scipy()
    n_i = np.repeat(width, 64)[:c.n].astype(np.float64)
    ul = c.u.astype(np.longdouble)
    Y = E.Vec(ctx, c.n)
    for transpose in (False, True):
        At = A.T.tocsr() if transpose else A
        ref = np.zeros(c.n, np.longdouble)
        rows = np.repeat(np.arange(c.n), np.diff(At.indptr))
        np.add.at(ref, rows, At.data.astype(np.longdouble) * ul[At.indices])
        bound = (n_i + 2.0) * 2.0 ** -53 * (abs(At) @ np.abs(c.u))
        y = np.array(M.mult(c.U, Y, transpose=transpose).get())
        err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{c.name}, {label}{'^T' if transpose else ''}: largest error / bound {worst:.3f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("name", PRODUCT_MESHES)
def test_product(ctx, name):
    """The product on J of the nonlinear form (unsymmetric Nitsche: unsymmetric values, so a wrong transposition map shows)
    and on K of the linear form."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    width = _product_preconditions(c)
    K = E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, E.Mat(c.dm))
    _check_product(ctx, c, K, width, "K")
    c.dm.set_boundary_facets(c.bmask)
    try:
        U3, UEX = E.Vec(ctx, c.n).set(0.3 * c.u), E.Vec(ctx, c.n).set(fo.u_exact_nl(c.om.x))
        J = E.assemble_jacobian(c.dm, 1, [0.0, -1.0], U3, c.F, None, E.Mat(c.dm), aux=UEX)
    finally:
        c.dm.set_boundary_facets(None)
    Jg = J.to_scipy()
    assert abs(Jg - Jg.T).max() > 1e-3 * abs(Jg).max()
    _check_product(ctx, c, J, width, "J")


@pytest.mark.parametrize("name", PRODUCT_MESHES)
def test_newton_rhs_linear(ctx, name):
    """k_spmv_sell_rhs on the same meshes: the Newton right-hand side from the assembled operator against the oracle."""
    from femo_amd import engine as E
    c = _case(ctx, name)
    _product_preconditions(c)
    K = E.assemble_jacobian(c.dm, 0, None, c.U, c.F, None, E.Mat(c.dm))
    R_ref = fo.residual(c.om, c.u, c.f)
    B = E.Vec(ctx, c.n)
    e = (_rel(E.newton_rhs_linear(K, c.F, c.U, None, B).get(), R_ref),)
    # (on the strips every vertex is a boundary vertex: the third set leaves most rows to the product)
    for dofs in (c.sets()["boundary"], c.sets()["hub_high"], np.arange(0, c.n, 7, dtype=np.int32)):
        b_ref = fo.newton_rhs(c.K, R_ref, c.u, dofs, c.gvals[dofs])
        e += (_rel(E.newton_rhs_linear(K, c.F, c.U, _ds(E, c, dofs), B).get(), b_ref),)
    print(f"{name}: " + " ".join(f"{v:.2e}" for v in e))
    assert max(e) < RTOL


# -------------------------------------------------------------------------------------------------------- solves ----
SOLVE_MESHES = ["cube5_8", "fan40x8_random", "cube6_bip30"]


@pytest.mark.parametrize("name", SOLVE_MESHES)
def test_cg(ctx, name):
    """solve_cg on the eliminated operator (the fused dot products of the product, k_scale_sell on wide slices) with the bars
    of test_gpu_engine.py::test_cg_parity."""
    from femo_amd import engine as E
    import scipy.sparse.linalg as spla
    c = _case(ctx, name)
    if name == "cube5_8":
        assert c.info["regular_slices"] == 7 and c.info["max_rowlen"] == 18
    bd = c.boundary
    A = E.assemble_jacobian(c.dm, 0, None, None, None, E.DirichletSet(c.dm, bd, 0.0), E.Mat(c.dm))
    Ao = fo.eliminate_bc(c.K, bd)
    b = np.random.default_rng(3).standard_normal(c.n)
    B, X = E.Vec(ctx, c.n).set(b), E.Vec(ctx, c.n)
    info = A.solve_cg(B, X, rtol=1e-13)
    xo = spla.splu(Ao.tocsc()).solve(b)
    _, it_o, _ = fo.pcg_jacobi(Ao, b, rtol=1e-13)
    print(f"{name}: {info.iterations} iterations (oracle {it_o}), error {_rel(X.get(), xo):.2e}")
    assert info.converged == 1
    assert _rel(X.get(), xo) < 1e-10
    assert abs(info.iterations - it_o) <= max(2, it_o // 50)
    info2 = A.solve_cg(B, X, transpose=True, rtol=1e-13, zero_guess=False)
    assert info2.converged == 1 and info2.iterations <= 2
    Z = E.Vec(ctx, c.n)
    info3 = A.solve_cg(Z, X, rtol=1e-13)
    assert info3.iterations == 0 and np.all(X.get() == 0.0)


@pytest.mark.parametrize("name", SOLVE_MESHES)
def test_bicgstab(ctx, name):
    """solve_bicgstab, plain and transposed, on the nonlinear Jacobian with its Dirichlet set against LU, at the tolerance of
    test_gpu_nonlinear.py::test_bicgstab_matches_lu."""
    from femo_amd import engine as E
    import scipy.sparse.linalg as spla
    c = _case(ctx, name)
    u, uex = 0.3 * c.u, fo.u_exact_nl(c.om.x)
    c.dm.set_boundary_facets(c.bmask)
    try:
        U, UEX = E.Vec(ctx, c.n).set(u), E.Vec(ctx, c.n).set(uex)
        J = E.assemble_jacobian(c.dm, 1, [0.0, -1.0], U, c.F, E.DirichletSet(c.dm, c.boundary, 0.0), E.Mat(c.dm), aux=UEX)
    finally:
        c.dm.set_boundary_facets(None)
    Jo = fo.eliminate_bc(fo.nl_jacobian(c.om, u, c.bmask, 0.0, -1.0), c.boundary)
    assert _rel(J.to_scipy().data, Jo.data) < RTOL
    b = np.random.default_rng(9).standard_normal(c.n)
    B, X = E.Vec(ctx, c.n).set(b), E.Vec(ctx, c.n)
    info = J.solve_bicgstab(B, X, rtol=1e-13)
    assert info.converged == 1 and _rel(X.get(), spla.splu(Jo.tocsc()).solve(b)) < 1e-9
    info = J.solve_bicgstab(B, X, transpose=True, rtol=1e-13)
    assert info.converged == 1 and _rel(X.get(), spla.splu(Jo.T.tocsc()).solve(b)) < 1e-9


# ---------------------------------------------------------------------------------------------------- elasticity ----
@pytest.mark.parametrize("name", ["fan40", "cube5_8"])
def test_elasticity_blocks(ctx, name):
    """DeviceElasticity.assemble + export_csr (k_elast_export: structural zeros of completed regular slices below entry 32,
    none from entry 32 on) and apply, against tests/elasticity_ref.py at the bar of test_gpu_topopt.py::test_assembly_parity."""
    import elasticity_ref as ref
    from femo_amd.engine import Vec
    from femo_amd.fea import utils_hip
    from femo_amd.fea.elasticity import METHODS, DeviceElasticity
    from femo_amd.fea.mesh import Mesh
    utils_hip.set_context(ctx)
    c = _case(ctx, name)
    assert c.info["regular_slices"] > 0 and c.info["max_rowlen"] == {"fan40": 40, "cube5_8": 18}[name]
    mesh = Mesh(c.om.x, c.om.conn)
    rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
    dev = DeviceElasticity(ctx, mesh)
    dev.assemble(METHODS["SIMP"], Vec(ctx, mesh.n_cell).set(rho))
    K, Kr = dev.export_csr(), ref.stiffness(mesh.x, mesh.conn, rho, "SIMP")
    K.sort_indices(); Kr.sort_indices()
    assert K.nnz == c.info["nnz"] * c.d * c.d
    assert np.array_equal(K.indptr, Kr.indptr) and np.array_equal(K.indices, Kr.indices)
    assert abs(K - Kr).max() <= 1e-12 * abs(Kr).max()
    assert (K != K.T).nnz == 0
    xv = np.random.default_rng(8).standard_normal(dev.n_dof)
    y = dev.apply(Vec(ctx, dev.n_dof).set(xv), Vec(ctx, dev.n_dof))
    assert _rel(y.get(), Kr @ xv) <= 1e-12
