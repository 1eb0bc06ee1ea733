"""No output hides a non-finite state ("Non-finite inputs"): every entry point of the table below that returns a
scalar, a gradient or a field is called with one entry of one floating-point input vector at NaN, +Inf or -Inf, and the
result is held to the two-sided contract of tests/nonfinite.py against the float64 restatement evaluated on the same
poisoned input: never hides, does not spray, a finite restatement decides the value, the handle still works.  A call may
refuse instead (`project_von_mises` with the consistent mass raises "the von Mises stress to project is not finite": a CG
on such a right-hand side has nothing to converge to); the call after it must then work.

Rows: the elasticity handle (rect24x12: 576 cells = 2 blocks of 256 and a tail of 64; cube6j: 1296 cells = 5 blocks and a tail
of 16; 325 and 343 vertices: 2 vertex blocks), the projection (600 cells: 3 blocks), the shell (`scordelis_lo_mesh(12, 12)`:
288 cells = 1 block and a tail of 32).  Three poisoned positions per input: the first wave of the first block, an entry whose
cells lie in the last, partly filled block, the last entry.  Batched calls run with L = 3 and L = 5 (the dJ/du kernel's chunk
of 4 columns is crossed) and poison column 0, then column L - 1.

Documented skips, which stay skips: a column of weight 0 in the stress aggregate, a cell of weight 0 in `compliance_dx`, a
passive cell of the projection.  The products and the solves have their own NaN tests and are not in the table.

Rows that cannot meet the contract: none."""
import functools

import numpy as np
import pytest

import elast_buckle_ref as bk
import elast_eig_ref as er
import elast_body_ref as br
import elast_stress_multi_ref as mref
import elast_stress_ref as sref
import elasticity_ref as ref
import nonfinite as nf
import projection_ref as P
from oracle import shell_oracle as so

pytestmark = pytest.mark.gpu

MESHES = ["rect24x12", "cube6j"]
DENSITY = 1.3


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


@functools.lru_cache(maxsize=None)
def _mesh(name):
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh
    mesh = createRectangleMesh([0.0, 0.0], [2.0, 1.0], 24, 12) if name == "rect24x12" else createUnitCubeMesh(6, 0.2)
    assert (mesh.n_vert, mesh.n_cell) == ((325, 576) if name == "rect24x12" else (343, 1296))
    return mesh


_HANDLES = {}


def _device(ctx, name):
    from femo_amd.fea.elasticity import DeviceElasticity
    if name not in _HANDLES:
        _HANDLES[name] = DeviceElasticity(ctx, _mesh(name))
    return _HANDLES[name]


def _vec(ctx, a):
    from femo_amd.engine import Vec
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return Vec(ctx, a.size).set(a)


def _out(ctx, n):
    from femo_amd.engine import Vec
    return Vec(ctx, int(n))


def _get(v, shape=None):
    a = np.array(v.get())
    return a if shape is None else a.reshape(shape)


def _refused():
    from femo_amd._lib import FemoError
    return (FemoError, ValueError)


# ======================================================================================================= elasticity ====
# A row: name, L (the column counts it runs with; (1,) for an unbatched call), make(mesh, L) -> dict of arrays and
# parameters, poison: input name -> kind ("cell", "dof", "dofcols"), out: output name -> kind ("scalar", "colscalars",
# "cell", "compcell", "dof", "dofcols"), call(ctx, dev, A) and ref(mesh, A) -> dict of outputs.
def _state(mesh, L, seed):
    """L random columns (magnitudes 1 ... 1e-3), rho in U(1e-3, 1), m_l = 1 / max sigma_vm(u_l), weights in U(0.25, 2)."""
    return mref.random_columns(mesh.x, mesh.conn, L, seed=seed)


def _make_stress(mesh, L, p=8.0, q=0.5):
    U, rho, m, w = _state(mesh, L, 5)
    return dict(U=U, rho=rho, m=m, w=w, p=p, q=q, alpha=float(ref.cell_volumes(mesh.x, mesh.conn).sum()))


def _call_pnorm(ctx, dev, A):
    gu, gr = _out(ctx, A["U"].size), _out(ctx, A["rho"].size)
    J = dev.pnorm_stress(_vec(ctx, A["rho"]), _vec(ctx, A["U"]), A["m"][0], A["p"], A["q"], A["alpha"], grad_u=gu, grad_rho=gr)
    return dict(value=J, du=_get(gu), drho=_get(gr))


def _ref_pnorm(mesh, A):
    R = sref.pnorm_stress(mesh.x, mesh.conn, A["rho"], A["U"][0], A["m"][0], A["p"], A["q"], A["alpha"])
    return dict(value=R["value"], du=R["du"], drho=R["drho"])


def _call_pnorm_multi(ctx, dev, A):
    L = len(A["U"])
    gu, gr = _out(ctx, A["U"].size), _out(ctx, A["rho"].size)
    vals = dev.pnorm_stress_multi(L, _vec(ctx, A["rho"]), _vec(ctx, A["U"]), A["m"], A["p"], A["q"], A["alpha"], weights=A["w"],
                                  grad_u=gu, grad_rho=gr)
    return dict(values=np.array(vals), du=_get(gu, (L, -1)), drho=_get(gr))


def _ref_pnorm_multi(mesh, A):
    R = mref.pnorm_stress_multi(mesh.x, mesh.conn, A["rho"], A["U"], A["m"], A["p"], A["q"], A["alpha"], weights=A["w"])
    return dict(values=R["values"], du=R["du"], drho=R["drho"])


def _fields(mesh, A, q):
    return np.stack([sref.cell_field(mesh.x, mesh.conn, u, A["rho"], q) for u in A["U"]])


def _call_von_mises(ctx, dev, A):
    nc = A["rho"].size
    uv, rv = _vec(ctx, A["U"]), _vec(ctx, A["rho"])
    return dict(relaxed=_get(dev.von_mises(uv, _out(ctx, nc), rv, A["q"])), solid=_get(dev.von_mises(uv, _out(ctx, nc))))


def _ref_von_mises(mesh, A):
    return dict(relaxed=_fields(mesh, A, A["q"])[0], solid=_fields(mesh, A, 0.0)[0])


def _make_vm_multi(mesh, L, column=None):
    A = _make_stress(mesh, L)
    A.update(scales=np.random.default_rng(8).uniform(0.5, 2.0, L) / np.array([f.max() for f in _fields(mesh, A, A["q"])]),
             column=column)
    return A


def _call_vm_multi(ctx, dev, A):
    L, nc = len(A["U"]), A["rho"].size
    uv, rv = _vec(ctx, A["U"]), _vec(ctx, A["rho"])
    kw = dict(scales=A["scales"], column=A["column"])
    return dict(relaxed=_get(dev.von_mises_multi(L, uv, _out(ctx, nc), rv, A["q"], **kw)),
                solid=_get(dev.von_mises_multi(L, uv, _out(ctx, nc), **kw)))


def _ref_vm_multi(mesh, A):
    out = {}
    for key, q in (("relaxed", A["q"]), ("solid", 0.0)):
        F = _fields(mesh, A, q)
        out[key] = mref.envelope(F, A["scales"]) if A["column"] is None else A["scales"][A["column"]] * F[A["column"]]
    return out


def _make_drho(mesh, L, transpose):
    U, rho, _, _ = _state(mesh, L, 11)
    rng = np.random.default_rng(12)
    x = rng.standard_normal(U.shape) if transpose else rng.standard_normal(rho.size)
    return dict(U=U, rho=rho, x=x, transpose=transpose, K0=ref.element_matrices(mesh.x, mesh.conn))


def _call_drho(ctx, dev, A):
    from femo_amd.fea.elasticity import METHODS
    L, t = len(A["U"]), A["transpose"]
    y = _out(ctx, A["rho"].size if t else A["U"].size)
    args = (_vec(ctx, A["rho"]), _vec(ctx, A["U"]), _vec(ctx, A["x"]), y)
    if A.get("single"):
        dev.drho(METHODS["SIMP"], t, *args)
    else:
        dev.drho_multi(METHODS["SIMP"], t, L, *args)
    return dict(y=_get(y) if t else _get(y, (L, -1)))


def _ref_drho(mesh, A):
    x, conn = mesh.x, mesh.conn
    if A["transpose"]:
        return dict(y=sum(ref.compliance_gradient(x, conn, A["rho"], u, xl, "SIMP", K0=A["K0"]) for u, xl in zip(A["U"], A["x"])))
    return dict(y=np.stack([br.drho_forward(x, conn, A["rho"], u, A["x"], "SIMP", K0=A["K0"]) for u in A["U"]]))


def _make_drho_single(mesh, L, transpose):
    return dict(_make_drho(mesh, 1, transpose), single=True)


def _make_body(mesh, L, transpose):
    rng = np.random.default_rng(13)
    B = rng.uniform(0.2, 1.0, (L, mesh.tdim)) * np.where(rng.random((L, mesh.tdim)) < 0.5, -1.0, 1.0)
    x = rng.standard_normal((L, mesh.x.size)) if transpose else rng.uniform(0.1, 1.0, mesh.n_cell)
    return dict(B=B, x=x, transpose=transpose)


def _call_body(ctx, dev, A):
    L, t = len(A["B"]), A["transpose"]
    y = _out(ctx, dev.mesh.n_cell if t else L * dev.n_dof)
    dev.body_apply(L, A["B"], _vec(ctx, A["x"]), y, transpose=t, a=-1.5)
    return dict(y=_get(y) if t else _get(y, (L, -1)))


def _ref_body(mesh, A):
    if A["transpose"]:
        return dict(y=-1.5 * sum(br.body_drho_T(mesh.x, mesh.conn, xl, b) for xl, b in zip(A["x"], A["B"])))
    return dict(y=np.stack([-1.5 * br.body_load(mesh.x, mesh.conn, A["x"], b) for b in A["B"]]))


def _mass_terms(mesh, rho, u, law):
    """(n_cell, d + 1, d): density m'(rho_e) (M0_e u_e), component by component: M0_e = |T_e| S (x) I_d."""
    d = mesh.tdim
    S = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    ue = np.asarray(u).reshape(-1, d)[mesh.conn]
    return (DENSITY * er.mass_law_d(rho, law) * ref.cell_volumes(mesh.x, mesh.conn))[:, None, None] * np.einsum("ab,ebi->eai", S, ue)


def _make_mass_drho(mesh, L, transpose):
    U, rho, _, _ = _state(mesh, L, 14)
    rng = np.random.default_rng(15)
    x = rng.standard_normal(U.shape) if transpose else rng.standard_normal(rho.size)
    return dict(U=U, rho=rho, x=x, transpose=transpose, scales=-rng.uniform(0.5, 2.0, L), law="du_olhoff")


def _call_mass_drho(ctx, dev, A):
    L, t = len(A["U"]), A["transpose"]
    y = _out(ctx, A["rho"].size if t else A["U"].size)
    dev.mass_drho_multi(t, L, A["scales"], _vec(ctx, A["rho"]), _vec(ctx, A["U"]), _vec(ctx, A["x"]), y, density=DENSITY,
                        mass_law=A["law"])
    return dict(y=_get(y) if t else _get(y, (L, -1)))


def _ref_mass_drho(mesh, A):
    d = mesh.tdim
    T = [_mass_terms(mesh, A["rho"], u, A["law"]) for u in A["U"]]
    if A["transpose"]:
        return dict(y=sum(s * np.einsum("eai,eai->e", t, xl.reshape(-1, d)[mesh.conn]) for s, t, xl in zip(A["scales"], T, A["x"])))
    out = np.zeros((len(T), mesh.n_vert, d))
    for l, (s, t) in enumerate(zip(A["scales"], T)):
        np.add.at(out[l], mesh.conn, s * A["x"][:, None, None] * t)
    return dict(y=out.reshape(len(T), -1))


def _make_eig_drho(mesh, L):
    U, rho, _, _ = _state(mesh, L, 16)
    rng = np.random.default_rng(17)
    return dict(U=U / np.abs(U).max(axis=1, keepdims=True), rho=rho, lam=rng.uniform(0.5, 2.0, L), c=rng.standard_normal(L),
                K0=ref.element_matrices(mesh.x, mesh.conn), M0=er.element_mass_matrices(mesh.x, mesh.conn))


def _call_eig_drho(ctx, dev, A):
    from femo_amd.fea.elasticity import METHODS
    y = _out(ctx, A["rho"].size)
    dev.eig_drho(METHODS["RAMP"], len(A["U"]), _vec(ctx, A["rho"]), _vec(ctx, A["U"]), A["lam"], A["c"], y, density=DENSITY,
                 mass_law="du_olhoff")
    return dict(y=_get(y))


def _ref_eig_drho(mesh, A):
    return dict(y=er.eig_drho(mesh.x, mesh.conn, A["rho"], A["U"].T, A["lam"], A["c"], "RAMP", "du_olhoff", DENSITY, A["K0"], A["M0"]))


def _cell_stress(mesh, rho, u, method):
    """(n_cell, d, d): C(rho_e) (lam tr(eps) I + 2 mu eps), the trace added on the diagonal only (no 0 * tr off it)."""
    d = mesh.tdim
    lam, mu = ref.lame()
    g, _ = sref.cell_gradients(mesh.x, mesh.conn)
    G = np.einsum("ebi,ebk->eik", np.asarray(u).reshape(-1, d)[mesh.conn], g)
    sig = mu * (G + np.transpose(G, (0, 2, 1)))
    tr = np.trace(G, axis1=1, axis2=2)
    for i in range(d):
        sig[:, i, i] += lam * tr
    return ref.penal(rho, method)[:, None, None] * sig


def _make_geom(mesh, L):
    U, rho, _, _ = _state(mesh, 1, 18)
    return dict(U=U, rho=rho)


def _call_geom(ctx, dev, A):
    from femo_amd.fea.elasticity import METHODS
    k = dev.d * (dev.d + 1) // 2
    out = dev.geom_stress(METHODS["RAMP"], _vec(ctx, A["rho"]), _vec(ctx, A["U"]), _out(ctx, k * A["rho"].size))
    return dict(sigma=_get(out, (k, -1)))


def _ref_geom(mesh, A):
    return dict(sigma=bk.stress_components(_cell_stress(mesh, A["rho"], A["U"][0], "RAMP")))


def _make_buckle(mesh, L):
    Phi, rho, _, _ = _state(mesh, L, 19)
    rng = np.random.default_rng(20)
    return dict(U=Phi / np.abs(Phi).max(axis=1, keepdims=True), rho=rho, u=rng.standard_normal(mesh.x.size), w1=rng.standard_normal(L),
                w2=rng.standard_normal(L), K0=ref.element_matrices(mesh.x, mesh.conn))


def _call_buckle(ctx, dev, A):
    from femo_amd.fea.elasticity import METHODS
    L, m = len(A["U"]), METHODS["SIMP"]
    rv, pv = _vec(ctx, A["rho"]), _vec(ctx, A["U"])
    du = dev.buckle_du(m, L, rv, pv, A["w2"], _out(ctx, dev.n_dof))
    dr = dev.buckle_drho(m, L, rv, _vec(ctx, A["u"]), pv, A["w1"], A["w2"], _out(ctx, A["rho"].size))
    return dict(du=_get(du), drho=_get(dr))


def _ref_buckle(mesh, A):
    x, conn = mesh.x, mesh.conn
    return dict(du=bk.buckle_du(x, conn, A["rho"], A["U"].T, A["w2"], "SIMP"),
                drho=bk.buckle_drho(x, conn, A["rho"], A["u"], A["U"].T, A["w1"], A["w2"], "SIMP", K0=A["K0"]))


def _make_dots(mesh, L):
    rng = np.random.default_rng(21)
    return dict(U=rng.standard_normal((L, mesh.x.size)), f=rng.standard_normal(mesh.x.size))


def _call_dots(ctx, dev, A):
    return dict(dots=dev.newmark_dots(len(A["U"]), _vec(ctx, A["f"]), _vec(ctx, A["U"])))


def _ref_dots(mesh, A):
    return dict(dots=np.array([float(np.sum(A["f"] * u)) for u in A["U"]]))


def _row(name, L, make, call, restate, poison, out, **kw):
    return pytest.param(dict(name=name, L=L, make=make, call=call, ref=restate, poison=poison, out=out, **kw), id=name)


_STRESS_OUT = dict(value="scalar", du="dof", drho="cell")
ELAST_ROWS = [
    _row("pnorm_stress-p8-q0.5", (1,), _make_stress, _call_pnorm, _ref_pnorm, dict(U="dofcols", rho="cell"), _STRESS_OUT),
    _row("pnorm_stress-p1-q0", (1,), functools.partial(_make_stress, p=1.0, q=0.0), _call_pnorm, _ref_pnorm,
         dict(U="dofcols", rho="cell"), _STRESS_OUT),
    _row("pnorm_stress_multi", (3, 5), _make_stress, _call_pnorm_multi, _ref_pnorm_multi, dict(U="dofcols", rho="cell"),
         dict(values="colscalars", du="dofcols", drho="cell")),
    _row("von_mises", (1,), _make_stress, _call_von_mises, _ref_von_mises, dict(U="dofcols", rho="cell"),
         dict(relaxed="cell", solid="cell"), not_read=dict(solid=("rho",))),
    _row("von_mises_multi-envelope", (3, 5), _make_vm_multi, _call_vm_multi, _ref_vm_multi, dict(U="dofcols", rho="cell"),
         dict(relaxed="cell", solid="cell"), not_read=dict(solid=("rho",))),
    _row("von_mises_multi-column0", (3, 5), functools.partial(_make_vm_multi, column=0), _call_vm_multi, _ref_vm_multi,
         dict(U="dofcols", rho="cell"), dict(relaxed="cell", solid="cell"), not_read=dict(solid=("rho",)), column=0),
    _row("von_mises_multi-last-column", (3, 5), functools.partial(_make_vm_multi, column=-1), _call_vm_multi, _ref_vm_multi,
         dict(U="dofcols", rho="cell"), dict(relaxed="cell", solid="cell"), not_read=dict(solid=("rho",)), column=-1),
    _row("drho-T", (1,), functools.partial(_make_drho_single, transpose=True), _call_drho, _ref_drho,
         dict(U="dofcols", x="dofcols", rho="cell"), dict(y="cell")),
    _row("drho-N", (1,), functools.partial(_make_drho_single, transpose=False), _call_drho, _ref_drho,
         dict(U="dofcols", x="cell", rho="cell"), dict(y="dofcols")),
    _row("drho_multi-T", (3, 5), functools.partial(_make_drho, transpose=True), _call_drho, _ref_drho,
         dict(U="dofcols", x="dofcols", rho="cell"), dict(y="cell")),
    _row("drho_multi-N", (3, 5), functools.partial(_make_drho, transpose=False), _call_drho, _ref_drho,
         dict(U="dofcols", x="cell", rho="cell"), dict(y="dofcols")),
    _row("body_apply-N", (3,), functools.partial(_make_body, transpose=False), _call_body, _ref_body, dict(x="cell"), dict(y="dofcols")),
    _row("body_apply-T", (3,), functools.partial(_make_body, transpose=True), _call_body, _ref_body, dict(x="dofcols"), dict(y="cell")),
    _row("mass_drho_multi-T", (3, 5), functools.partial(_make_mass_drho, transpose=True), _call_mass_drho, _ref_mass_drho,
         dict(U="dofcols", x="dofcols", rho="cell"), dict(y="cell")),
    _row("mass_drho_multi-N", (3, 5), functools.partial(_make_mass_drho, transpose=False), _call_mass_drho, _ref_mass_drho,
         dict(U="dofcols", x="cell", rho="cell"), dict(y="dofcols")),
    _row("eig_drho", (3,), _make_eig_drho, _call_eig_drho, _ref_eig_drho, dict(U="dofcols", rho="cell"), dict(y="cell")),
    _row("geom_stress", (1,), _make_geom, _call_geom, _ref_geom, dict(U="dofcols", rho="cell"), dict(sigma="compcell")),
    _row("buckle_du-buckle_drho", (3,), _make_buckle, _call_buckle, _ref_buckle, dict(U="dofcols", u="dof", rho="cell"),
         dict(du="dof", drho="cell"), not_read=dict(du=("u",))),
    _row("newmark_dots", (9,), _make_dots, _call_dots, _ref_dots, dict(U="dofcols", f="dof"), dict(dots="colscalars")),
]


def _entries(mesh, kind, L):
    """(flat entry, cells that read it, its column or None) for the poisoned positions of an input of ``kind``."""
    d, conn = mesh.tdim, mesh.conn
    if kind == "cell":
        return [(c, nf.one_cell(mesh.n_cell, c), None) for c in nf.cell_positions(mesh.n_cell)]
    pos = nf.positions(conn, d)
    if kind == "dof":
        return [(e, nf.cells_of_vertex(conn, e // d), None) for e in pos]
    cols = (0,) if L == 1 else (0, L - 1)
    return [(col * mesh.x.size + e, nf.cells_of_vertex(conn, e // d), col) for col in cols for e in pos]


def _dependent(mesh, out_kind, shape, cells, col, row_column):
    """The entries of an output of ``out_kind`` that may change when an input read by ``cells`` (in column ``col``) does."""
    d = mesh.tdim
    dofs = nf.vertex_dofs(nf.entries_of_cells(mesh.conn, cells, mesh.n_vert), d)
    if out_kind == "scalar":
        return np.ones(shape, bool)
    if out_kind == "colscalars":
        m = np.ones(shape, bool) if col is None else np.zeros(shape, bool)
        if col is not None:
            m[col] = True
        return m
    if out_kind in ("cell", "compcell"):
        if row_column is not None and col is not None and col != row_column:
            return np.zeros(shape, bool)                     # the field of one column does not read the others
        return np.broadcast_to(cells, shape)
    if out_kind == "dof":
        return dofs
    return nf.in_column(dofs, shape[0], col)


def _run_row(ctx, row, mesh, dev, L, tol=None, decide_tol=1e-12):
    A = row["make"](mesh, L)
    if row.get("column") == -1:
        row = dict(row, column=L - 1)
        A["column"] = L - 1
    clean = row["call"](ctx, dev, A)
    base = row["ref"](mesh, A)
    for k, kind in row["out"].items():                       # the restatement is the reference on finite inputs to begin with
        err = np.abs(np.asarray(clean[k]) - np.asarray(base[k])).max()
        assert err <= 1e-11 * max(np.abs(np.asarray(base[k])).max(), 1e-300), (row["name"], k, err)
    msgs, n_calls = [], 0
    for name, kind in row["poison"].items():
        for entry, cells, col in _entries(mesh, kind, len(A[name]) if kind == "dofcols" else 1):
            for value in nf.VALUES:
                B = dict(A)
                B[name] = nf.poison(A[name], entry, value)
                got = row["call"](ctx, dev, B)
                with np.errstate(all="ignore"):
                    want = row["ref"](mesh, B)
                n_calls += 1
                for k, kind_out in row["out"].items():
                    shape = np.atleast_1d(np.asarray(clean[k])).shape
                    dep = _dependent(mesh, kind_out, shape, cells, col, row.get("column"))
                    if name in row.get("not_read", {}).get(k, ()):
                        dep = np.zeros(shape, bool)
                    msgs += nf.violations(got[k], want[k], clean[k], dep, tol=tol, decide_tol=decide_tol,
                                          label=f"{row['name']} L={L} {name}[{entry}]={value} -> {k}")
    again = row["call"](ctx, dev, A)                          # the handle still works: the clean bits again
    for k in row["out"]:
        assert np.array_equal(np.asarray(again[k]), np.asarray(clean[k])), (row["name"], k, "after the poisoned calls")
    print(f"{row['name']} L={L}: {n_calls} poisoned calls, {len(msgs)} violations")
    return msgs


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("row", ELAST_ROWS)
def test_elasticity(gpu, row, name):
    mesh, dev = _mesh(name), _device(gpu, name)
    msgs = []
    for L in row["L"]:
        msgs += _run_row(gpu, row, mesh, dev, L)
    assert not msgs, "\n".join(msgs[:20] + [f"... {len(msgs)} in all"])


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("L", [3, 5])
def test_weight_zero_column_stays_skipped(gpu, name, L):
    """The documented skip: a column of weight 0 takes no part in dJ/du (written as zeros) nor in dJ/drho, whatever its state
    holds; its own unweighted value J_l still shows the poison, and the other columns' values keep the clean bits."""
    mesh, dev = _mesh(name), _device(gpu, name)
    for col in (0, L - 1):
        A = _make_stress(mesh, L)
        A["w"] = A["w"].copy()
        A["w"][col] = 0.0
        clean = _call_pnorm_multi(gpu, dev, A)
        assert np.all(clean["du"][col] == 0.0)
        for entry, _, _ in [e for e in _entries(mesh, "dofcols", L) if e[2] == col]:
            for value in nf.VALUES:
                got = _call_pnorm_multi(gpu, dev, dict(A, U=nf.poison(A["U"], entry, value)))
                assert np.array_equal(got["du"], clean["du"]) and np.array_equal(got["drho"], clean["drho"]), (col, entry, value)
                assert not np.isfinite(got["values"][col])
                others = np.arange(L) != col
                assert np.array_equal(got["values"][others], clean["values"][others])


def test_mma_refuses_the_aggregate_of_a_poisoned_state(gpu):
    """End to end: J of `pnorm_stress` on a poisoned state is not finite, `DeviceMMA.update` refuses it as a constraint value,
    and the next clean update is step 1."""
    from femo_amd.opt import DeviceMMA
    mesh, dev = _mesh("rect24x12"), _device(gpu, "rect24x12")
    A = _make_stress(mesh, 1)
    n = mesh.n_cell
    opt = DeviceMMA(gpu, _vec(gpu, np.full(n, 1e-3)), _vec(gpu, np.ones(n)), 1)
    x, g = A["rho"], np.random.default_rng(3).standard_normal(n)
    good = _call_pnorm(gpu, dev, A)
    for value in nf.VALUES:
        bad = _call_pnorm(gpu, dev, dict(A, U=nf.poison(A["U"], nf.positions(mesh.conn, mesh.tdim)[1], value)))
        assert not np.isfinite(bad["value"])
        with pytest.raises(ValueError, match="the value of constraint 0 is not finite"):       # the value alone: a clean gradient
            opt.update(_vec(gpu, x), 1.0, _vec(gpu, g), [bad["value"] - 1.0], _vec(gpu, good["drho"]))
    info = opt.update(_vec(gpu, x), 1.0, _vec(gpu, g), [good["value"] - 1.0], _vec(gpu, good["drho"]))
    assert info["step"] == 1 and info["converged"] == 1


# ======================================================================================================= projection ====
N_PROJ, BETA_PROJ, ETA_PROJ = 600, 8.0, 0.4
SOLID, VOID = (256,), (255,)
PROJ_POSITIONS = (5, 556, N_PROJ - 1, SOLID[0])                  # first wave, the tail block, the last entry, a passive cell


def _proj_inputs():
    rng = np.random.default_rng(4)
    return dict(xt=rng.random(N_PROJ), v=rng.uniform(0.5, 1.5, N_PROJ), a=rng.standard_normal(N_PROJ),
                flag=P.flags(N_PROJ, SOLID, VOID))


def _only(j):
    return nf.one_cell(N_PROJ, j)


@pytest.mark.parametrize("beta", [0.0, BETA_PROJ])
def test_projection_fixed_threshold(gpu, beta):
    """rho = H(xt), J^T a and J d with a fixed threshold are entry by entry: only entry j moves, a passive cell does not even
    read its xt, tanh(+-Inf) = +-1 gives the finite values H = 1 or 0 and H_x = 0, and beta = 0 is the identity."""
    from femo_amd.fea.elasticity import DeviceProjection
    I = _proj_inputs()
    xt, v, a, flag = I["xt"], I["v"], I["a"], I["flag"]
    proj = DeviceProjection(gpu, N_PROJ, beta, ETA_PROJ, v, SOLID, VOID, 1e-4)

    def call(xt_, a_):
        d_xt, d_a = _vec(gpu, xt_), _vec(gpu, a_)
        d_rho = _out(gpu, N_PROJ)
        proj.forward(d_xt, d_rho)
        return dict(rho=_get(d_rho), reverse=_get(proj.reverse(d_xt, d_a, _out(gpu, N_PROJ))),
                    tangent=_get(proj.tangent(d_xt, d_a, _out(gpu, N_PROJ))))

    def restate(xt_, a_):
        return dict(rho=P.project(xt_, beta, ETA_PROJ, flag, 1e-4), reverse=P.jac_reverse(xt_, a_, beta, ETA_PROJ, flag)[0],
                    tangent=P.jac_forward(xt_, a_, beta, ETA_PROJ, flag)[0])

    clean = call(xt, a)
    msgs = []
    for j in PROJ_POSITIONS:
        for value in nf.VALUES:
            for which in ("xt", "a"):
                xt_, a_ = (nf.poison(xt, j, value), a) if which == "xt" else (xt, nf.poison(a, j, value))
                got = call(xt_, a_)
                with np.errstate(all="ignore"):
                    want = restate(xt_, a_)
                # the entry bounds of tests/projection_ref.py at the poisoned point, with the rounding of the product on top
                # (a non-finite a_j leaves no bound to speak of: the entry is not finite in the restatement, or an exact 0)
                with np.errstate(all="ignore"):
                    bx = np.abs(a_) * np.nan_to_num(P.bound_Hx(np.nan_to_num(xt_, posinf=1e300, neginf=-1e300), beta, ETA_PROJ))
                bx = np.nan_to_num(bx, nan=0.0, posinf=0.0) + P.EPS * np.abs(np.nan_to_num(want["reverse"], posinf=0.0, neginf=0.0))
                tols = dict(rho=np.full(N_PROJ, P.bound_H(beta, ETA_PROJ)), reverse=bx, tangent=bx)
                for k in ("rho", "reverse", "tangent"):
                    if which == "a" and k == "rho":
                        dep = np.zeros(N_PROJ, bool)
                    else:
                        dep = _only(j)
                    msgs += nf.violations(got[k], want[k], clean[k], dep, decide_tol=tols[k],
                                          label=f"projection beta={beta} {which}[{j}]={value} -> {k}")
                if flag[j] != 0:                              # the documented skip: a passive cell
                    assert np.array_equal(got["rho"], clean["rho"])
                    assert got["reverse"][j] == 0.0 and got["tangent"][j] == 0.0
    again = call(xt, a)
    assert all(np.array_equal(again[k], clean[k]) for k in clean)
    assert not msgs, "\n".join(msgs[:20] + [f"... {len(msgs)} in all"])


def test_projection_volume_threshold(gpu):
    """The volume-preserving threshold couples every cell through eta, so every active entry is in the dependent set.  The
    bisection's rule `g > 0 ? lo = mid : hi = mid` decides the same way on the device and in the restatement whatever g is, and
    a g that is NaN or -Inf at every step (xt_j = NaN, +Inf) ends at eta = 2^-54, a g = +Inf (xt_j = -Inf) at 1 - 2^-54: the
    density is H at that threshold to the entry bound, NaN in cell j only for xt_j = NaN.  The Jacobian products at the
    threshold of a clean forward call: a NaN reaches every active entry through the rank-one term."""
    from femo_amd.fea.elasticity import DeviceProjection
    I = _proj_inputs()
    xt, v, a, flag = I["xt"], I["v"], I["a"], I["flag"]
    act = flag == 0
    proj = DeviceProjection(gpu, N_PROJ, BETA_PROJ, "volume", v, SOLID, VOID, 1e-4)
    d_rho = _out(gpu, N_PROJ)
    info0 = proj.forward(_vec(gpu, xt), d_rho)
    rho0, eta0 = _get(d_rho), info0["eta"]
    msgs = []
    for j in PROJ_POSITIONS:
        for value in nf.VALUES:
            xt_ = nf.poison(xt, j, value)
            info = proj.forward(_vec(gpu, xt_), d_rho)
            got = _get(d_rho)
            if flag[j] != 0:                                  # a passive cell's xt is not read: the clean call again
                assert info["eta"] == eta0 and np.array_equal(got, rho0)
                continue
            with np.errstate(all="ignore"):
                eta = P.bisect_eta(xt_, v, BETA_PROJ, flag)
                want = P.project(xt_, BETA_PROJ, eta, flag, 1e-4)
            assert eta in (2.0 ** -54, 1.0 - 2.0 ** -54) and info["eta"] == eta, (j, value, info["eta"], eta)
            assert not np.isfinite(info["vol_in"])
            msgs += nf.violations(got, want, rho0, act, decide_tol=np.full(N_PROJ, P.bound_H(BETA_PROJ, eta)),
                                  label=f"projection volume xt[{j}]={value} -> rho")
            assert np.array_equal(got[~act], rho0[~act])
    # Jacobian products at the threshold of the clean call
    info = proj.forward(_vec(gpu, xt), d_rho)
    assert info["eta"] == eta0 and np.array_equal(_get(d_rho), rho0)
    d_xt, d_a = _vec(gpu, xt), _vec(gpu, a)
    clean = dict(reverse=_get(proj.reverse(d_xt, d_a, _out(gpu, N_PROJ))), tangent=_get(proj.tangent(d_xt, d_a, _out(gpu, N_PROJ))))
    for j in PROJ_POSITIONS:
        for value in nf.VALUES:
            for which in ("xt", "a"):
                xt_, a_ = (nf.poison(xt, j, value), a) if which == "xt" else (xt, nf.poison(a, j, value))
                d_xt, d_a = _vec(gpu, xt_), _vec(gpu, a_)
                got = dict(reverse=_get(proj.reverse(d_xt, d_a, _out(gpu, N_PROJ))), tangent=_get(proj.tangent(d_xt, d_a, _out(gpu, N_PROJ))))
                for k, fn in (("reverse", P.jac_reverse), ("tangent", P.jac_forward)):
                    with np.errstate(all="ignore"):
                        want = np.asarray(fn(xt_, a_, BETA_PROJ, eta0, flag, v, True)[0], dtype=float)
                        bound = P.volume_product_bounds(xt_, a_, BETA_PROJ, eta0, flag, v, k == "tangent")[0] if np.all(np.isfinite(want)) else 0.0
                    dep = np.zeros(N_PROJ, bool) if flag[j] != 0 else act
                    msgs += nf.violations(got[k], want, clean[k], dep, decide_tol=np.broadcast_to(bound, (N_PROJ,)),
                                          label=f"projection volume {which}[{j}]={value} -> {k}")
    assert not msgs, "\n".join(msgs[:20] + [f"... {len(msgs)} in all"])


def test_projection_grayness(gpu):
    """M_nd = 4 sum v rho (1 - rho) / sum v reads every cell, passive ones too: one non-finite density and it is not finite."""
    from femo_amd.fea.elasticity import DeviceProjection
    I = _proj_inputs()
    proj = DeviceProjection(gpu, N_PROJ, BETA_PROJ, ETA_PROJ, I["v"], SOLID, VOID, 1e-4)
    rho = I["xt"]
    clean = proj.grayness(_vec(gpu, rho))
    for j in PROJ_POSITIONS:
        for value in nf.VALUES:
            with np.errstate(all="ignore"):
                want = float(P.grayness(nf.poison(rho, j, value), I["v"]))
            got = proj.grayness(_vec(gpu, nf.poison(rho, j, value)))
            assert not np.isfinite(want) and not np.isfinite(got), (j, value, got, want)
    assert proj.grayness(_vec(gpu, rho)) == clean


# ============================================================================================================ shell ====
E_Y, NU_S, RHO_S = 4.32e8, 0.3, 2710.0
SHELL_TOL = 1e-12                                                  # the parity bar of the shell kernels (float atomics)


@functools.lru_cache(maxsize=None)
def _shell_space():
    pts, conn = so.scordelis_lo_mesh(12, 12)
    V = so.ShellSpace(pts, conn)
    assert V.conn.shape[0] == 288
    return pts, conn, V


_SHELL = {}


def _shell(ctx):
    from femo_amd.fea.shell import DeviceShell, ShellSpace
    if "dev" not in _SHELL:
        pts, conn, _ = _shell_space()
        _SHELL["dev"] = DeviceShell(ctx, ShellSpace(pts, conn))
    return _SHELL["dev"]


def _shell_inputs():
    _, _, V = _shell_space()
    rng = np.random.default_rng(7)
    h = 0.25 * (1.0 + 0.3 * rng.random(V.n_vert))
    w = 1e-3 * rng.standard_normal(V.n_dof)
    vm = so.von_mises_stress(V, w, h, E_Y, NU_S, 1.0)
    cw = (V.x[V.conn][:, :, 0].min(axis=1) >= 12.0).astype(float)             # a tagged region, like dx_2(10)
    assert 0 < cw.sum() < cw.size
    return dict(h=h, w=w, v=1e-3 * rng.standard_normal(V.n_dof), acc=rng.standard_normal(V.n_dof), dh=0.1 * h * rng.standard_normal(V.n_vert),
                f=rng.standard_normal(3 * V.n_vert), m=1.0 / vm.max(), cw=cw, alpha=float(V.frames()[3].sum()))


def _quad(V):
    e1, e2, e3, area, gl = V.frames()
    for lam, wq in zip(*so.QUAD_INPLANE):
        N, gN = so._p2(lam, gl)
        yield lam, wq * area, N, so._strain_operators(e1, e2, e3, gN, gl, lam)


def _scatter(n, index, values):
    out = np.zeros(n)
    np.add.at(out, np.asarray(index).ravel(), np.asarray(values).ravel())
    return out


def _sh_ref_vm_rhs(V, A, surface):
    vm = so.von_mises_stress(V, A["w"], A["h"], E_Y, NU_S, surface)
    lam, wq = np.asarray(so.QUAD_INPLANE[0]), np.asarray(so.QUAD_INPLANE[1])
    return _scatter(V.n_vert, V.conn, np.einsum("c,q,cq,qi->ci", V.frames()[3], wq, vm, lam))


def _shear_quad(V):
    e1, e2, e3, area, gl = V.frames()
    for lam, wq in zip(*so.QUAD_SHEAR):
        yield lam, wq * area * so.SHEAR_CORRECTION * E_Y / (2.0 * (1.0 + NU_S)), so._strain_operators(e1, e2, e3, so._p2(lam, gl)[1], gl, lam)[2]


def _sh_ref_dform(V, A):
    """1/2 v^T K(h) w and g_b = v^T (dK/dh_b) w from the strains of v and w at the quadrature points (the sums of
    oracle/shell_oracle.py::dform_dh and element_stiffness, strains first)."""
    C = so.plane_stress(E_Y, NU_S)
    hc, ve, we = A["h"][V.conn], A["v"][V.cell_dofs], A["w"][V.cell_dofs]
    en, g = 0.0, np.zeros((V.conn.shape[0], 3))
    for lam, wa, _, (Bm, Bb, _, Bd) in _quad(V):
        hq = hc @ lam
        mem = np.einsum("ci,ij,cj->c", np.einsum("cia,ca->ci", Bm, ve), C, np.einsum("cia,ca->ci", Bm, we))
        ben = np.einsum("ci,ij,cj->c", np.einsum("cia,ca->ci", Bb, ve), C, np.einsum("cia,ca->ci", Bb, we))
        dri = E_Y * np.einsum("ci,ci->c", np.einsum("cia,ca->ci", Bd, ve), np.einsum("cia,ca->ci", Bd, we))
        en += float((wa * (hq * mem + hq ** 3 * (ben / 12.0 + dri))).sum())
        g += (wa * (mem + hq * hq * (0.25 * ben + 3.0 * dri)))[:, None] * lam[None, :]
    for lam, wk, Bs in _shear_quad(V):
        sh = wk * np.einsum("ci,ci->c", np.einsum("cia,ca->ci", Bs, ve), np.einsum("cia,ca->ci", Bs, we))
        en += float(((hc @ lam) * sh).sum())
        g += sh[:, None] * lam[None, :]
    return dict(energy=0.5 * en, dh=_scatter(V.n_vert, V.conn, g))


def _sh_ref_dform_fwd(V, A):
    """(dK/dh [dh]) w: the section weights h, h^3 / 12, E h^3 and the shear's h differentiated in the direction dh."""
    C = so.plane_stress(E_Y, NU_S)
    hc, dc, we = A["h"][V.conn], A["dh"][V.conn], A["w"][V.cell_dofs]
    y = np.zeros((V.conn.shape[0], 27))
    for lam, wa, _, (Bm, Bb, _, Bd) in _quad(V):
        hq, dq = hc @ lam, dc @ lam
        y += np.einsum("cia,ci->ca", Bm, (wa * dq)[:, None] * np.einsum("ij,cj->ci", C, np.einsum("cjb,cb->cj", Bm, we)))
        y += np.einsum("cia,ci->ca", Bb, (wa * 0.25 * hq * hq * dq)[:, None] * np.einsum("ij,cj->ci", C, np.einsum("cjb,cb->cj", Bb, we)))
        y += np.einsum("cia,ci->ca", Bd, (wa * 3.0 * E_Y * hq * hq * dq)[:, None] * np.einsum("cib,cb->ci", Bd, we))
    for lam, wk, Bs in _shear_quad(V):
        y += np.einsum("cia,ci->ca", Bs, (wk * (dc @ lam))[:, None] * np.einsum("cib,cb->ci", Bs, we))
    return _scatter(V.n_dof, V.cell_dofs, y)


def _sh_ref_compliance(V, A, cells):
    """1/2 u^T M u and M u over the displacement dofs, which are all the compliance reads: the oracle's `compliance` takes the
    product with the whole state vector, rotations times zero included."""
    nu3 = 3 * V.n_unode
    g = so.compliance_du(V, A["w"], cells)
    return dict(J=0.5 * float(A["w"][:nu3] @ g[:nu3]), dw=g)


def _sh_ref_mass(V, A):
    area = V.frames()[3]
    return RHO_S * float((area * A["h"][V.conn].mean(axis=1)).sum()), _scatter(V.n_vert, V.conn, np.repeat(RHO_S * area / 3.0, 3))


def _sh_ref_hpower(V, A, coef, p):
    area = V.frames()[3]
    lam6, w6 = so.QUAD_INPLANE
    hq = A["h"][V.conn] @ lam6.T
    return (coef * float((area[:, None] * w6[None, :] * hq ** p).sum()),
            _scatter(V.n_vert, V.conn, coef * p * np.einsum("c,q,cq,qb->cb", area, w6, hq ** (p - 1.0), lam6)))


def _sh_ref_inertia_dh(V, A):
    """d/dh_b of lam^T M(h) acc: rho int phi_b (lam_u . acc_u + h^2 / 4 lam_theta . acc_theta)."""
    hc = A["h"][V.conn]
    lu, au = (A[k][V.cell_dofs[:, :18]].reshape(-1, 6, 3) for k in ("v", "acc"))
    lt, at = (A[k][V.cell_dofs[:, 18:]].reshape(-1, 3, 3) for k in ("v", "acc"))
    g = np.zeros((V.conn.shape[0], 3))
    for lam, wa, N, _ in _quad(V):
        hq = hc @ lam
        d = np.einsum("ci,ci->c", np.einsum("a,cai->ci", N, lu), np.einsum("a,cai->ci", N, au)) \
            + 0.25 * hq * hq * np.einsum("ci,ci->c", np.einsum("b,cbi->ci", lam, lt), np.einsum("b,cbi->ci", lam, at))
        g += (RHO_S * wa * d)[:, None] * lam[None, :]
    return _scatter(V.n_vert, V.conn, g)


def _sh_ref_load_T(V, A):
    le = A["v"][V.cell_dofs[:, :18]].reshape(-1, 6, 3)
    out = np.zeros((V.conn.shape[0], 3, 3))
    for lam, wa, N, _ in _quad(V):
        out += np.einsum("c,b,ci->cbi", wa, lam, np.einsum("a,cai->ci", N, le))
    return _scatter(3 * V.n_vert, 3 * V.conn[:, :, None] + np.arange(3), out)


# name -> (inputs that can be poisoned with their kind, outputs with their kind, call(ctx, dev, D) with D the device vectors
# of the inputs, restatement(V, A))
def _sh_compliance(ctx, dev, D):
    g = _out(ctx, dev.n_dof)
    return dict(J=dev.compliance(D["w"], grad=g), dw=_get(g))


def _sh_compliance_dx(ctx, dev, D):
    g = _out(ctx, dev.n_dof)
    return dict(J=dev.compliance_dx(D["w"], D["cw"], grad=g), dw=_get(g))


def _sh_pnorm(surface):
    def call(ctx, dev, D):
        gw, gh = _out(ctx, dev.n_dof).fill(0.0), _out(ctx, D["h"].n).fill(0.0)
        J = dev.pnorm_stress(E_Y, NU_S, D["h"], D["w"], D["_m"], 4.0, D["_alpha"], surface=surface, grad_w=gw, grad_h=gh)
        return dict(J=J, dw=_get(gw), dh=_get(gh))

    def restate(V, A):
        J, gw, gh = so.pnorm_stress(V, A["w"], A["h"], E_Y, NU_S, m=A["m"], rho=4.0, alpha=A["alpha"], surface=surface, grad=True)
        return dict(J=J, dw=gw, dh=gh)
    return call, restate


def _sh_vm_rhs(ctx, dev, D):
    b, ml = _out(ctx, D["h"].n), _out(ctx, D["h"].n)
    dev.vm_rhs(E_Y, NU_S, D["h"], D["w"], 1.0, b, ml)
    return dict(b=_get(b), lumped=_get(ml))


def _sh_project(lump):
    def call(ctx, dev, D):
        return dict(field=_get(dev.project_von_mises(E_Y, NU_S, D["h"], D["w"], 1.0, _out(ctx, D["h"].n), lump_mass=lump)))
    return call, lambda V, A: dict(field=so.project_von_mises(V, A["w"], A["h"], E_Y, NU_S, 1.0, lump_mass=lump))


def _sh_dform(ctx, dev, D):
    return dict(energy=dev.dform_dh(E_Y, NU_S, D["h"], D["v"], D["w"], energy=True),
                dh=_get(dev.dform_dh(E_Y, NU_S, D["h"], D["v"], D["w"], out=_out(ctx, D["h"].n))))


def _sh_dform_fwd(ctx, dev, D):
    return dict(y=_get(dev.dform_dh_fwd(E_Y, NU_S, D["h"], D["dh"], D["w"], _out(ctx, dev.n_dof))))


def _sh_mass(ctx, dev, D):
    g = _out(ctx, D["h"].n)
    return dict(J=dev.mass(RHO_S, D["h"], grad=g), dh=_get(g))


def _sh_reg(kind):
    def call(ctx, dev, D):
        g = _out(ctx, D["h"].n)
        return dict(J=dev.regularization(kind, D["h"], grad=g), dh=_get(g))

    def restate(V, A):
        J, g = so.regularization(V, A["h"], kind, grad=True)
        return dict(J=J, dh=g)
    return call, restate


def _sh_hpower(ctx, dev, D):
    g = _out(ctx, D["h"].n)
    return dict(J=dev.hpower(0.5e3, 3.0, D["h"], grad=g), dh=_get(g))


def _sh_inertia(ctx, dev, D):
    return dict(y=_get(dev.inertia_apply(RHO_S, D["h"], D["acc"], _out(ctx, dev.n_dof))),
                dh=_get(dev.inertia_dh(RHO_S, D["h"], D["v"], D["acc"], _out(ctx, D["h"].n))))


def _sh_load(ctx, dev, D):
    return dict(F=_get(dev.load(D["f"], _out(ctx, dev.n_dof))), FT=_get(dev.load_T(D["v"], _out(ctx, D["f"].n))))


def _pair(J_g):
    return dict(J=J_g[0], dh=J_g[1])


SHELL_ROWS = {
    "compliance": (dict(w="state"), dict(J="scalar", dw="state"), _sh_compliance, lambda V, A: _sh_ref_compliance(V, A, None)),
    "compliance_dx": (dict(w="state"), dict(J="scalar", dw="state"), _sh_compliance_dx,
                      lambda V, A: _sh_ref_compliance(V, A, np.flatnonzero(A["cw"]))),
    "pnorm_stress-top": (dict(w="state", h="vert"), dict(J="scalar", dw="state", dh="vert")) + _sh_pnorm(1.0),
    "pnorm_stress-mid": (dict(w="state", h="vert"), dict(J="scalar", dw="state", dh="vert")) + _sh_pnorm(0.0),
    "pnorm_stress-bottom": (dict(w="state", h="vert"), dict(J="scalar", dw="state", dh="vert")) + _sh_pnorm(-1.0),
    "vm_rhs": (dict(w="state", h="vert"), dict(b="vert", lumped="fixed"), _sh_vm_rhs,
               lambda V, A: dict(b=_sh_ref_vm_rhs(V, A, 1.0), lumped=_scatter(V.n_vert, V.conn, np.repeat(V.frames()[3] / 3.0, 3)))),
    "project_von_mises-lumped": (dict(w="state", h="vert"), dict(field="vert")) + _sh_project(True),
    "project_von_mises-consistent": (dict(w="state", h="vert"), dict(field="all")) + _sh_project(False),
    "dform_dh-energy": (dict(w="state", v="state", h="vert"), dict(energy="scalar", dh="vert"), _sh_dform,
                        _sh_ref_dform),
    "dform_dh_fwd": (dict(w="state", dh="vert", h="vert"), dict(y="state"), _sh_dform_fwd, lambda V, A: dict(y=_sh_ref_dform_fwd(V, A))),
    "mass": (dict(h="vert"), dict(J="scalar", dh="fixed"), _sh_mass, lambda V, A: _pair(_sh_ref_mass(V, A))),
    "regularization-H1": (dict(h="vert"), dict(J="scalar", dh="vert")) + _sh_reg("H1"),
    "regularization-L2H1": (dict(h="vert"), dict(J="scalar", dh="vert")) + _sh_reg("L2H1"),
    "regularization-L2": (dict(h="vert"), dict(J="scalar", dh="vert")) + _sh_reg("L2"),
    "hpower": (dict(h="vert"), dict(J="scalar", dh="vert"), _sh_hpower, lambda V, A: _pair(_sh_ref_hpower(V, A, 0.5e3, 3.0))),
    "inertia_apply-inertia_dh": (dict(acc="state", v="state", h="vert"), dict(y="state", dh="vert"), _sh_inertia,
                                 lambda V, A: dict(y=so.inertia_apply(V, A["h"], RHO_S, A["acc"]), dh=_sh_ref_inertia_dh(V, A))),
    "load-load_T": (dict(f="vert3", v="state"), dict(F="state", FT="vert3"), _sh_load,
                    lambda V, A: dict(F=so.load_vector(V, A["f"].reshape(-1, 3)), FT=_sh_ref_load_T(V, A))),
}
# what an output does not read at all: it keeps the clean result whatever that input holds
SHELL_NOT_READ = {("inertia_apply-inertia_dh", "y"): ("v",), ("load-load_T", "F"): ("v",), ("load-load_T", "FT"): ("f",)}


def _shell_entries(V, kind):
    """(flat entry, cells that read it) for the three poisoned positions of an input of ``kind``."""
    n_cell = V.conn.shape[0]
    tail = (n_cell - 1) // 256 * 256
    assert 0 < n_cell - tail < 256 and tail > 0
    c = tail + (n_cell - tail) // 2
    if kind == "state":
        ent = [3 * 3 + 0, int(V.cell_dofs[c][22]), V.n_dof - 1]                # a displacement, a rotation of the tail block, the last dof
        return [(e, nf.cells_of_entry(V.cell_dofs, e)) for e in ent]
    verts = [3, int(V.conn[c][1]), V.n_vert - 1]
    if kind == "vert":
        return [(v, nf.cells_of_vertex(V.conn, v)) for v in verts]
    return [(3 * v + k, nf.cells_of_vertex(V.conn, v)) for k, v in enumerate(verts)]


def _shell_dependent(V, kind, shape, cells):
    if kind in ("scalar", "all"):
        return np.ones(shape, bool)
    if kind == "fixed":
        return np.zeros(shape, bool)
    if kind == "state":
        return nf.entries_of_cells(V.cell_dofs, cells, V.n_dof)
    verts = nf.entries_of_cells(V.conn, cells, V.n_vert)
    return verts if kind == "vert" else np.repeat(verts, 3)


@pytest.mark.parametrize("name", list(SHELL_ROWS))
def test_shell(gpu, name):
    poisonable, outputs, call, restate = SHELL_ROWS[name]
    _, _, V = _shell_space()
    dev, A = _shell(gpu), _shell_inputs()

    def run(B):
        D = {k: _vec(gpu, B[k]) for k in ("h", "w", "v", "acc", "dh", "f", "cw")}
        D["_m"], D["_alpha"] = B["m"], B["alpha"]
        return call(gpu, dev, D)

    clean, base = run(A), restate(V, A)
    for k in outputs:
        err = np.abs(np.asarray(clean[k]) - np.asarray(base[k])).max()
        assert err <= 1e-10 * np.abs(np.asarray(base[k])).max(), (name, k, err)
    msgs, refused = [], 0
    for which, kind in poisonable.items():
        for entry, cells in _shell_entries(V, kind):
            if name == "compliance_dx" and not np.any(A["cw"][cells] != 0.0):
                continue                                      # (the documented skip has its own test below)
            for value in nf.VALUES:
                B = dict(A)
                B[which] = nf.poison(A[which], entry, value)
                try:
                    got = run(B)
                except _refused():
                    refused += 1                              # the call refuses: the clean call after it must work (below)
                    continue
                with np.errstate(all="ignore"):
                    want = restate(V, B)
                for k, kind_out in outputs.items():
                    shape = np.atleast_1d(np.asarray(clean[k])).shape
                    dep = _shell_dependent(V, kind_out, shape, cells)
                    if which in SHELL_NOT_READ.get((name, k), ()):
                        dep = np.zeros(shape, bool)
                    msgs += nf.violations(got[k], want[k], clean[k], dep, tol=SHELL_TOL, decide_tol=SHELL_TOL,
                                          label=f"shell {name} {which}[{entry}]={value} -> {k}")
    again = run(A)
    for k in outputs:
        assert np.abs(np.asarray(again[k]) - np.asarray(clean[k])).max() <= SHELL_TOL * np.abs(np.asarray(clean[k])).max(), (name, k)
    print(f"shell {name}: {refused} calls refused, {len(msgs)} violations")
    assert name != "project_von_mises-consistent" or refused > 0
    assert not msgs, "\n".join(msgs[:20] + [f"... {len(msgs)} in all"])


def test_shell_compliance_dx_skips_cells_of_weight_zero(gpu):
    """The documented skip: `compliance_dx` does not read the state of a cell whose weight is 0, so a poisoned dof that only
    such cells hold changes neither the value nor the gradient."""
    _, _, V = _shell_space()
    dev, A = _shell(gpu), _shell_inputs()
    outside = [d for d in range(0, V.n_dof, 97) if not np.any(A["cw"][nf.cells_of_entry(V.cell_dofs, d)] != 0.0)][:3]
    assert len(outside) == 3
    cw = _vec(gpu, A["cw"])
    g = _out(gpu, V.n_dof)
    J = dev.compliance_dx(_vec(gpu, A["w"]), cw, grad=g)
    g0 = _get(g)
    for d in outside:
        for value in nf.VALUES:
            Jp = dev.compliance_dx(_vec(gpu, nf.poison(A["w"], d, value)), cw, grad=g)
            assert np.isfinite(Jp) and abs(Jp - J) <= SHELL_TOL * abs(J)
            assert np.abs(_get(g) - g0).max() <= SHELL_TOL * np.abs(g0).max()
