"""Mirror of femo/fea/utils_dolfinx.py on the HIP engine.

Same function names, argument meaning and return conventions as the reference
(file:line cited per function); dolfinx/PETSc objects are replaced by the
handle classes of ``femo_amd.engine``.  Values may cross as NumPy arrays (the
CSDL convention) or as ``DeviceArray`` (stay in HBM).
"""
from __future__ import annotations

import os
import threading
from timeit import default_timer
from typing import List, Optional, Sequence

import numpy as np

from .. import _lib
from .. import engine as E
from ..engine import Context, DeviceArray, Vec
from .forms import (BackendForm, BeamResidual, DerivativeForm, FieldExpression, Form, FunctionExpr, GradientMagnitude,
                    L2TrackingFunctional, LinearFunctional, NonlinearPoissonResidual, PoissonResidual, PowerExpr, derivative)
from .function import Function, FunctionSpace, _VectorView
from .io import MeshTags, import_mesh, read_mesh, write_mesh_files
from .mesh import (BeamMesh, Mesh, createIntervalMesh, createRectangleMesh, createUnitCubeMesh, createUnitSquareMesh,
                   findNodeIndices, meshSize,
                   locate_dofs_geometrical)

DOLFIN_EPS = 3E-16

# ---------------------------------------------------------------- context ----
_CTX: Optional[Context] = None
_TLS = threading.local()          # per-thread override (rank emulation: one rank per host thread)


def get_context() -> Context:
    """One context (device + stream) per process: device = LOCAL_RANK (one
    process per GPU), replacing ``comm = MPI.COMM_WORLD`` (utils_dolfinx.py:32).
    A thread that called ``set_context(ctx, thread_local=True)`` sees its own."""
    global _CTX
    ctx = getattr(_TLS, "ctx", None)
    if ctx is not None:
        return ctx
    if _CTX is None:
        _CTX = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _CTX


def set_context(ctx: Optional[Context], thread_local: bool = False) -> None:
    global _CTX
    if thread_local:
        _TLS.ctx = ctx
    else:
        _CTX = ctx


# Linear-solver options: the analogue of the global PETSc options database the
# reference mutates (utils_dolfinx.py:393-403, 446).  CG + Jacobi replaces MUMPS.
# rtol acts on the Jacobi-preconditioned residual; the relative error of the
# solution is bounded by cond(D^-1 A) * rtol (cond ~ 0.4 n^2 on an n^d grid), and
# 1e-14 keeps states and sensitivities within 1e-10 of the LU oracle on every
# parity case (measured sweep: DESIGN.md section 6).
# pc: 'bpx' = Jacobi + auxiliary-lattice multilevel correction (csrc/bpx.hip) wherever the operator
# comes from a Poisson-type form, Jacobi elsewhere (mass matrix, beam); 'jacobi' = diagonal scaling only.
# rtol_bpx: BPX-CG stops on the residual in the norm of the preconditioner, sqrt(r^T M^-1 r) <= rtol_bpx sqrt(b^T M^-1 b);
# that ratio tracks the relative energy-norm error (measured: within 10 %) on every mesh size, whereas the error
# behind a given Jacobi-norm ratio grows like cond(D^-1 A) ~ n^2 -- 1e-14 there was what the 1e-10 parity bar needed
# on the 10 M-DOF cube and over-solved by ~12 of 42 iterations.  1e-11 leaves the state / sensitivity errors at
# 1e-12..1e-11 of their maxima (tests/test_gpu_fullsize.py, test_gpu_operators.py assert 1e-10).
KSP_OPTIONS = dict(rtol=1e-14, rtol_bpx=1e-11, atol=0.0, max_it=100000, check_every=32, pc='bpx')
_BPX_KINDS = (_lib.PDE_POISSON, _lib.PDE_NL_POISSON)
BPX_MAX_OCCUPANCY = 20.0      # Mesh.lattice_occupancy() above this: graded mesh, Jacobi does better
LAST_KSP_INFO: List[dict] = []   # appended by every linear solve (iteration counts for reports); callers
KSP_INFO_CAP = 1 << 16           # that need a complete record clear it first (bench.py); oldest entries go beyond the cap


# ------------------------------------------------------- array <-> function ----
def getFuncArray(v: Function, device: bool = False):
    """utils_dolfinx.py:155-159."""
    if device:
        return DeviceArray(v.vec)
    return v.vector.getArray()


def setFuncArray(v: Function, v_array) -> None:
    """utils_dolfinx.py:161-167."""
    if isinstance(v_array, DeviceArray):
        if v_array.vec is not v.vec:
            v.version += 1
            v.vec.copy_from(v_array.vec)
        return
    v.vector[:] = v_array
    v.vector.assemble()
    v.vector.ghostUpdate()


def update(v: Function, v_values) -> None:
    """utils_dolfinx.py:300-311: a length-1 value broadcasts via Vec.set."""
    if not isinstance(v_values, DeviceArray) and len(v_values) == 1 and v.function_space.dim != 1:
        v.vector.set(v_values)
    else:
        setFuncArray(v, v_values)


def createFunction(function: Function) -> Function:
    """utils_dolfinx.py:316-317."""
    return Function(function.function_space)


def computePartials(form: Form, function: Function) -> DerivativeForm:
    """utils_dolfinx.py:313-314."""
    return derivative(form, function)


# ------------------------------------------------------------ Dirichlet BCs ----
class DirichletBC:
    """dolfinx.fem.dirichletbc(value, dofs[, V]) [ext] (fea_dolfinx.py:169-176)."""

    def __init__(self, value, dofs, function_space: Optional[FunctionSpace] = None):
        if isinstance(dofs, (tuple, list)) and len(dofs) == 2 and not np.isscalar(dofs[0]):
            dofs = dofs[0]        # (V, V) locate returns a pair of identical arrays [ext]
        self.dofs = np.asarray(dofs, dtype=np.int32).ravel()
        self.value = value
        self.function_space = function_space

    def version(self):
        return (id(self.value), self.value.version) if isinstance(self.value, Function) else float(self.value)

    def values(self) -> np.ndarray:
        """Prescribed values on ``dofs``.  A Function value is re-read only after a
        host-side write to it (Function.version), not on every assembly."""
        if isinstance(self.value, Function):
            ver = self.value.version
            if getattr(self, "_cache_ver", None) != ver:
                self._cache = self.value.vector.getArray()[self.dofs]
                self._cache_ver = ver
            return self._cache
        return np.full(self.dofs.shape, float(self.value))


def dirichletbc(value, dofs, function_space=None) -> DirichletBC:
    return DirichletBC(value, dofs, function_space)


_BC_CACHE: dict = {}


def _dirichlet_set(mesh: Mesh, bcs: Sequence[DirichletBC]) -> Optional[E.DirichletSet]:
    """Merge a bc list into one device set (first bc wins on duplicates, as
    dolfinx applies them in order).  Cached per (mesh, list identity, value versions)."""
    if not bcs:
        return None
    key = (id(mesh), tuple(id(b) for b in bcs))
    ver = tuple(b.version() for b in bcs)
    hit = _BC_CACHE.get(key)
    if hit is not None and hit[1] == ver:
        return hit[0]
    vals = np.concatenate([b.values() for b in bcs])
    dofs = np.concatenate([b.dofs for b in bcs])
    _, first = np.unique(dofs, return_index=True)
    ds = E.DirichletSet(mesh.device(get_context()), dofs[first], vals[first])
    _BC_CACHE[key] = (ds, ver, bcs)
    return ds


# Device buffers that are re-used across calls (allocation and free of GB-sized
# buffers costs milliseconds and synchronises the stream): keyed by (mesh, role).
_WORK: dict = {}


def _work(mesh: Mesh, role: str, make):
    key = (id(mesh), role)
    w = _WORK.get(key)
    if w is None or w[0] is not mesh:
        w = (mesh, make())
        _WORK[key] = w
    return w[1]


def clear_workspaces() -> None:
    _WORK.clear()
    _BC_CACHE.clear()


def _shutdown() -> None:
    """Release device objects before the context (and before the HIP runtime's own
    static destructors run at interpreter exit)."""
    global _CTX
    import gc
    clear_workspaces()
    gc.collect()
    if _CTX is not None:
        try:
            _CTX.sync()
        except Exception:
            pass


import atexit  # noqa: E402

atexit.register(_shutdown)


# ------------------------------------------------------------------ matrices ----
class SparseMatrix:
    """PETSc Mat stand-in for N x N operators on the mesh pattern."""

    def __init__(self, mesh: Mesh, symmetric: bool = False):
        self.mesh = mesh
        self.dmesh = mesh.device(get_context())
        self.mat = E.Mat(self.dmesh)
        self.symmetric = symmetric
        self.pde_kind = None       # set by the assembly that fills the values

    def getSizes(self):
        return (self.dmesh.n_rows, self.dmesh.n_vert)

    @property
    def size(self):
        return self.getSizes()

    def mult(self, x: Vec, y: Vec) -> Vec:
        return self.mat.mult(x, y, transpose=False)

    def multTranspose(self, x: Vec, y: Vec) -> Vec:
        return self.mat.mult(x, y, transpose=not self.symmetric)

    def new_row_vec(self) -> Vec:
        return _work(self.mesh, "spmv_row", lambda: Vec(get_context(), self.dmesh.n_vert))

    def new_col_vec(self) -> Vec:
        return _work(self.mesh, "spmv_col", lambda: Vec(get_context(), self.dmesh.n_vert))

    def to_scipy(self):
        return self.mat.to_scipy()

    def getValuesCSR(self):
        rowptr, col, val = self.mat.export_csr()
        return rowptr, col, val


class CellMatrix:
    """dR/df for a DG0 argument: N x n_cell, stored cell-major (tdim+1 values per
    cell aligned with the connectivity), i.e. the CSC of the PETSc Mat the
    reference assembles at state_model.py:141."""

    def __init__(self, mesh: Mesh, uniform: bool = False):
        """``uniform``: every column has one value on all its rows (the Poisson-type residuals: -|T_c|/(d+1)); the matrix
        is then kept as n_cell values instead of (d+1) n_cell (round 3: a quarter of the bytes to fill and to apply)."""
        self.mesh = mesh
        self.dmesh = mesh.device(get_context())
        self.uniform = bool(uniform)
        self.vals = Vec(get_context(), mesh.n_cell * (1 if self.uniform else mesh.tdim + 1))

    def getSizes(self):
        return (self.dmesh.n_rows, self.mesh.n_cell)

    def mult(self, x: Vec, y: Vec) -> Vec:
        if self.uniform:
            return E.dRdf_cell_apply(self.dmesh, self.vals, x, y, transpose=False)
        return E.dRdf_apply(self.dmesh, self.vals, x, y, transpose=False)

    def multTranspose(self, x: Vec, y: Vec) -> Vec:
        if self.uniform:
            return E.dRdf_cell_apply(self.dmesh, self.vals, x, y, transpose=True)
        return E.dRdf_apply(self.dmesh, self.vals, x, y, transpose=True)

    def new_row_vec(self) -> Vec:
        return _work(self.mesh, "cellmat_row", lambda: Vec(get_context(), self.dmesh.n_vert))

    def new_col_vec(self) -> Vec:
        return _work(self.mesh, "cellmat_col", lambda: Vec(get_context(), self.mesh.n_cell))

    def to_scipy(self):
        import scipy.sparse as sp
        d1 = self.mesh.tdim + 1
        v = np.asarray(self.vals.get())
        if self.uniform:
            v = np.repeat(v, d1)
        rows = self.mesh.conn.ravel()
        cols = np.repeat(np.arange(self.mesh.n_cell), d1)
        A = sp.coo_matrix((v, (rows, cols)), shape=(self.mesh.n_vert, self.mesh.n_cell)).tocsr()
        A.sort_indices()
        return A


class TransposedMatrix:
    """Result of ``transpose(A)``: a view, no data is moved (utils_dolfinx.py:241-245)."""

    def __init__(self, A: SparseMatrix):
        self.A = A


def transpose(A: SparseMatrix) -> TransposedMatrix:
    return TransposedMatrix(A)


def convertToCOO(A):
    """utils_dolfinx.py:248-254."""
    return A.to_scipy().tocoo()


def convertToDense(A) -> np.ndarray:
    """utils_dolfinx.py:290-297 (debug only)."""
    return A.to_scipy().toarray()


# ------------------------------------------------------------------ assembly ----
def _mesh_of(form: Form) -> Mesh:
    base = form.form if isinstance(form, DerivativeForm) else form
    if isinstance(base, BackendForm):
        return base.mesh
    return base.functions()[0].function_space.mesh


_RESIDUALS = (PoissonResidual, NonlinearPoissonResidual, BeamResidual)


def _aux(res) -> Optional[Vec]:
    """Extra device field of a residual form + one-time mesh data it needs (exterior facets)."""
    if isinstance(res, NonlinearPoissonResidual):
        if res.weak_bc:
            mesh = res.u.function_space.mesh
            dm = mesh.device(get_context())
            if not getattr(dm, "_bfacets_set", False):
                dm.set_boundary_facets(mesh.boundary_facet_mask())
                dm._bfacets_set = True
            return res.u_exact.vec
    if isinstance(res, BeamResidual):
        return res.load.vec
    return None


def assembleScalar(c: Form) -> float:
    """utils_dolfinx.py:169-173; local value (all-reduced over ranks inside the engine)."""
    if isinstance(c, BackendForm):
        return c.assemble_scalar()
    if isinstance(c, L2TrackingFunctional):
        dm = _mesh_of(c).device(get_context())
        return E.functional_value(dm, c.functional_kind, c.params, c.u.vec, c.f.vec, c.u_exact.vec)
    if isinstance(c, LinearFunctional):
        n = c.arg.function_space.dim
        return c.coeff.vec.dot(c.arg.vec, n)
    raise NotImplementedError(f"assembleScalar: {type(c).__name__} is not in the form catalogue")


def _assemble_vector_dev(v: Form, out: Optional[Vec] = None) -> Vec:
    """Assembles into ``out`` or into a per-(mesh, form kind) buffer that the next
    assembly of the same kind overwrites (callers consume the result at once)."""
    if isinstance(v, BackendForm):
        return v.assemble_vector(out)
    if isinstance(v, DerivativeForm) and isinstance(v.form, BackendForm):
        return v.form.assemble_derivative(v.wrt, out)
    ctx = get_context()
    mesh = _mesh_of(v)
    dm = mesh.device(ctx)
    if isinstance(v, _RESIDUALS):
        out = out or _work(mesh, "vec_residual", lambda: Vec(ctx, dm.n_vert))
        return E.assemble_residual(dm, v.pde_kind, v.params, v.u.vec, v.f.vec, out, aux=_aux(v))
    if isinstance(v, DerivativeForm) and isinstance(v.form, L2TrackingFunctional):
        J = v.form
        if v.wrt is J.u:
            out = out or _work(mesh, "vec_dJdu", lambda: Vec(ctx, dm.n_vert))
            return E.functional_grad_u(dm, J.functional_kind, J.params, J.u.vec, J.f.vec, J.u_exact.vec, out)
        if v.wrt is J.f:
            out = out or _work(mesh, "vec_dJdf", lambda: Vec(ctx, mesh.n_cell))
            return E.functional_grad_f(dm, J.functional_kind, J.params, J.u.vec, J.f.vec, J.u_exact.vec, out)
    if isinstance(v, DerivativeForm) and isinstance(v.form, LinearFunctional):
        J = v.form
        n = v.wrt.function_space.dim
        out = out or _work(mesh, f"vec_lin_{n}", lambda: Vec(ctx, n))
        if v.wrt is J.arg:
            return out.copy_from(J.coeff.vec)
        return out.fill(0.0)
    raise NotImplementedError(f"assembleVector: {type(v).__name__} is not in the form catalogue")


def assembleVector(v: Form, device: bool = False):
    """utils_dolfinx.py:175-179; no BC treatment."""
    vec = _assemble_vector_dev(v)
    return DeviceArray(vec) if device else vec.get()


def assembleMatrix(M: Form, bcs: Sequence[DirichletBC] = (), out=None):
    """utils_dolfinx.py:181-187.  ``out`` lets callers re-use a matrix."""
    if isinstance(M, DerivativeForm) and isinstance(M.form, BackendForm):
        return M.form.partial_matrix(M.wrt, out)
    if not isinstance(M, DerivativeForm) or not isinstance(M.form, _RESIDUALS):
        raise NotImplementedError(f"assembleMatrix: {type(M).__name__} is not in the form catalogue")
    res = M.form
    mesh = _mesh_of(M)
    dm = mesh.device(get_context())
    if M.wrt is res.u:
        A = out if isinstance(out, SparseMatrix) else SparseMatrix(mesh, symmetric=res.is_symmetric)
        A.pde_kind = res.pde_kind
        E.assemble_jacobian(dm, res.pde_kind, res.params, res.u.vec, res.f.vec, _dirichlet_set(mesh, bcs), A.mat,
                            aux=_aux(res))
        return A
    if M.wrt is res.f:
        if bcs:
            raise NotImplementedError("dR/df with Dirichlet rows eliminated")
        uniform = res.pde_kind in (_lib.PDE_POISSON, _lib.PDE_NL_POISSON)
        D = out if isinstance(out, CellMatrix) and out.uniform == uniform else CellMatrix(mesh, uniform=uniform)
        if uniform:
            E.assemble_dRdf_cell(dm, res.pde_kind, res.params, D.vals)
        else:
            E.assemble_dRdf(dm, res.pde_kind, res.params, res.u.vec, res.f.vec, D.vals)
        return D
    raise NotImplementedError("derivative of the residual w.r.t. this Function")


def assembleSystem(J: Form, F: Form, bcs: Sequence[DirichletBC] = (), rhs: bool = True, out=None,
                   out_nobc=None):
    """utils_dolfinx.py:189-202: A with Dirichlet rows/cols eliminated (diag 1) and
    b = F - K[:,bc] g, b[bc] = g (apply_lifting + set_bc [ext]).  The operator
    layer passes ``rhs=False`` because it discards b (state_model.py:149), and
    ``out_nobc`` to get dR/du without BCs from the same pass over the mesh."""
    if isinstance(J, DerivativeForm) and isinstance(J.form, BackendForm) and J.wrt is J.form.u:
        return J.form.assemble_system(bcs, rhs, out, out_nobc)
    if not isinstance(J, DerivativeForm) or not isinstance(J.form, _RESIDUALS) or J.wrt is not J.form.u:
        raise NotImplementedError("assembleSystem: J must be derivative(residual, state)")
    res = J.form
    mesh = _mesh_of(J)
    dm = mesh.device(get_context())
    A = out if isinstance(out, SparseMatrix) else SparseMatrix(mesh, symmetric=res.is_symmetric)
    ds = _dirichlet_set(mesh, bcs)
    A.pde_kind = res.pde_kind
    if out_nobc is not None:
        out_nobc.pde_kind = res.pde_kind
    E.assemble_system(dm, res.pde_kind, res.params, res.u.vec, res.f.vec, ds,
                      out_nobc.mat if out_nobc is not None else None, A.mat, None, aux=_aux(res))
    if not rhs:
        return A, None
    b = _assemble_vector_dev(F).get()
    if ds is not None:
        K = out_nobc if out_nobc is not None else assembleMatrix(J)
        g = np.zeros(mesh.n_vert)
        g[ds.dofs] = ds.vals
        gv = Vec(get_context(), mesh.n_vert).set(g)
        Kg = Vec(get_context(), mesh.n_vert)
        K.mult(gv, Kg)
        b = b - Kg.get()
        b[ds.dofs] = ds.vals
    return A, b


def applyBC(res: Form, u: Function, bcs: Sequence[DirichletBC]) -> np.ndarray:
    """utils_dolfinx.py:266-273: the residual vector with Dirichlet lifting, b = F - K[:,bc] g, b[bc] = g
    (apply_lifting + set_bc [ext]), K = derivative(res, u)."""
    _, b = assembleSystem(derivative(res, u), res, bcs)
    return b


def assemble(f: Form, dim: int = 0, bcs: Sequence[DirichletBC] = (), device: bool = False):
    """utils_dolfinx.py:204-213."""
    if dim == 0:
        return assembleScalar(f)
    elif dim == 1:
        return assembleVector(f, device=device)
    elif dim == 2:
        M = assembleMatrix(f, bcs=bcs)
        return convertToDense(M)
    else:
        return TypeError("Invalid type for assembly.")


def assemble_partials(of=None, wrt=None, dim=1):
    """utils_dolfinx.py:216-222."""
    return assemble(derivative(of, wrt), dim=dim)


# --------------------------------------------------------------------- SpMV ----
def _as_vec(x) -> Vec:
    if isinstance(x, Function):
        return x.vec
    if isinstance(x, _VectorView):
        return x._fn.vec
    if isinstance(x, DeviceArray):
        return x.vec
    if isinstance(x, Vec):
        return x
    raise TypeError(f"expected a Function / vector, got {type(x).__name__}")


def computeMatVecProductFwd(A, x: Function, device: bool = False):
    """utils_dolfinx.py:256-264:  y = A x."""
    y = A.new_row_vec()
    A.mult(_as_vec(x), y)
    n = A.getSizes()[0]
    return DeviceArray(y, n) if device else y.get(n)


def computeMatVecProductBwd(A, R: Function, device: bool = False):
    """utils_dolfinx.py:275-287:  y = A^T R."""
    y = A.new_col_vec()
    A.multTranspose(_as_vec(R), y)
    n = A.getSizes()[1]
    return DeviceArray(y, n) if device else y.get(n)


def _add_product(target, A, x, transposed: bool):
    """target += A x (or A^T x) with NumPy's in-place semantics: the ``d_residuals[u] += ...`` /
    ``d_inputs[arg] += ...`` statements of state_model.py:176-200.  For a NumPy target the sum is
    formed while the product is copied out of the device (no second pass over the host array)."""
    y = A.new_col_vec() if transposed else A.new_row_vec()
    n = A.getSizes()[1 if transposed else 0]
    if (transposed and isinstance(A, CellMatrix) and A.uniform and isinstance(target, np.ndarray) and target.dtype == np.float64
            and target.flags.c_contiguous and target.flags.writeable and target.size == n):
        # the tail of a reverse sweep: product, sum and copy-out in one call, streamed where the sum is formed on the device
        return E.dRdf_cell_apply_T_add_to_host(A.dmesh, A.vals, _as_vec(x), y, target, n)
    (A.multTranspose if transposed else A.mult)(_as_vec(x), y)
    if isinstance(target, DeviceArray):
        target += DeviceArray(y, n)
        return target
    if (isinstance(target, np.ndarray) and target.dtype == np.float64 and target.flags.c_contiguous
            and target.flags.writeable and target.size == n):
        y.add_to_host(target, n)
        return target
    if isinstance(target, np.ndarray) and E.is_pinned(target):
        E.host_touch(target)                     # a NumPy write into a block that may be recorded as a mirror
    target += E.host_wait(y.get(n))
    return target


def addMatVecProductFwd(target, A, x):
    """target += A x  (utils_dolfinx.py:256-264 followed by the caller's ``+=``)."""
    return _add_product(target, A, x, False)


def addMatVecProductBwd(target, A, R):
    """target += A^T R  (utils_dolfinx.py:275-287 followed by the caller's ``+=``)."""
    return _add_product(target, A, R, True)


# ------------------------------------------------------------- linear solves ----
class KSP:
    """A configured Jacobi-CG solve on a fixed operator (PETSc KSP stand-in).
    ``solve(b, x)`` follows petsc4py's argument order (utils_dolfinx.py:493)."""

    def __init__(self, A, options: Optional[dict] = None):
        self.transposed = isinstance(A, TransposedMatrix)
        self.A = A.A if self.transposed else A
        self.options = dict(KSP_OPTIONS)
        if options:
            self.options.update(options)
        self.info = None

    def solve(self, b, x) -> None:
        """Symmetric operators: Jacobi-CG; otherwise BiCGSTAB on A or its explicit transpose."""
        if self.transposed and hasattr(self.A, "backend_solve_transpose"):    # an operator that is not symmetric solves A^T itself
            self.A.backend_solve_transpose(_as_vec(b), _as_vec(x), self.options)
            self.info = self.A.info
            return
        if hasattr(self.A, "backend_solve"):               # operators of a BackendForm bring their own solver
            self.A.backend_solve(_as_vec(b), _as_vec(x), self.options)
            self.info = self.A.info
            return
        o = self.options
        tr = self.transposed and not self.A.symmetric
        kw = dict(transpose=tr, rtol=o["rtol"], atol=o["atol"], max_it=o["max_it"], zero_guess=True,
                  check_every=o["check_every"])
        if self.A.symmetric:
            pc = o.get("pc", "jacobi")
            if pc == "bpx" and (self.A.pde_kind not in _BPX_KINDS
                                or self.A.mesh.lattice_occupancy() > BPX_MAX_OCCUPANCY):
                pc = "jacobi"
            if pc == "bpx":
                kw["rtol"] = o.get("rtol_bpx", o["rtol"])
                kw["atol_pc"] = o.get("atol_pc", 0.0)
            self.info = self.A.mat.solve_cg(_as_vec(b), _as_vec(x), pc=pc, **kw)
        else:
            self.info = self.A.mat.solve_bicgstab(_as_vec(b), _as_vec(x), **kw)
        LAST_KSP_INFO.append(dict(thread=threading.get_ident(), iterations=self.info.iterations, converged=self.info.converged,
                                  residual_norm=self.info.residual_norm, rhs_norm=self.info.rhs_norm,
                                  pc_residual_norm=self.info.pc_residual_norm, pc_rhs_norm=self.info.pc_rhs_norm,
                                  solve_ms=self.info.solve_ms, spmv_ms=self.info.spmv_ms,
                                  spmv_samples=self.info.spmv_samples, loop_allreduces=getattr(self.info, "loop_allreduces", 0)))
        if len(LAST_KSP_INFO) > KSP_INFO_CAP:
            del LAST_KSP_INFO[:-KSP_INFO_CAP // 2]
        if self.info.converged != 1:
            raise RuntimeError(f"{'CG' if self.A.symmetric else 'BiCGSTAB'} did not converge: {self.info.iterations} iterations, "
                               f"||r|| = {self.info.residual_norm:.3e}, ||b|| = {self.info.rhs_norm:.3e}")


def solveKSP_mumps(A, b, x, options: Optional[dict] = None) -> None:
    """utils_dolfinx.py:476-493: solve A x = b.  Name kept for drop-in; the factorisation
    is replaced by Jacobi-preconditioned CG on the device (BASELINE.json design)."""
    KSP(A, options).solve(b, x)


solveKSP = solveKSP_mumps   # utils_dolfinx.py:451-474 (ASM/GMRES variant) maps to the same solve


def setUpKSP_MUMPS(A, options: Optional[dict] = None) -> KSP:
    """utils_dolfinx.py:495-512: a reusable solver object for repeated right-hand sides."""
    return KSP(A, options)


# ---------------------------------------------------------- nonlinear solves ----
class cycle_linearisation:
    """``with cycle_linearisation(res, bcs, dRdu, A):`` a Newton solve of ``res`` with ``bcs`` inside the block runs on these
    matrices -- dR/du without and A with the Dirichlet set eliminated, assembled by the caller in THIS cycle -- instead of
    assembling its own (forms with constant partials only, `_NewtonBase.linear_reuse`).  Per thread, and gone with the block:
    a linearisation is never carried into a later solve."""

    def __init__(self, res: Form, bcs, K: "SparseMatrix", A: "SparseMatrix"):
        self.entry = (res, list(bcs), K, A)

    def __enter__(self):
        _TLS.linearisation = self.entry
        return self

    def __exit__(self, *exc):
        _TLS.linearisation = None
        return False


def _offered_linearisation(F: Form, bcs):
    entry = getattr(_TLS, "linearisation", None)
    if entry is None or entry[0] is not F or len(entry[1]) != len(bcs) or any(a is not b for a, b in zip(entry[1], bcs)):
        return None
    return entry[2], entry[3]


class _NewtonBase:
    def __init__(self, F: Form, w: Function, bcs, abs_tol, rel_tol, max_it, report, error_on_nonconvergence):
        if not isinstance(F, _RESIDUALS):
            raise NotImplementedError(f"nonlinear solve of {type(F).__name__}")
        self.F, self.w, self.bcs = F, w, list(bcs)
        self.atol, self.rtol, self.max_it = abs_tol, rel_tol, max_it
        self.report, self.error_on_nonconvergence = report, error_on_nonconvergence
        self.mesh = _mesh_of(F)
        self.iterations = 0
        self.residual_norms: List[float] = []
        self.ksp_iterations: List[int] = []
        self.stol = 0.0           # relative step tolerance (PETSc SNES only, see SNESSolver)

    # Newton corrections below the rounding error of the assembled residual are noise:
    # ||D^-1 (fl(F(u)) - F(u))||_2 ~ c eps ||u||_2 (measured c ~ 20 on the 10 M-DOF cube,
    # DESIGN.md section 6).  Linear solves stop there instead of iterating on round-off.
    NOISE_FACTOR = 64.0
    # Newton reads rho_0 of the next solve with its own reduction and skips a solve the solver would not iterate on (round 6;
    # False leaves the decision to the solver: tests compare the two)
    newton_probe = True
    # A form whose partials are constant (`constant_partials`: linear Poisson) has ONE operator per solve: dR/du and A are
    # assembled once, in one pass over the mesh -- or taken from the caller's linearisation of this cycle
    # (`cycle_linearisation`) -- and every right-hand side is a product with dR/du (engine.newton_rhs_linear) instead of another
    # pass.  Same iterations, same reductions, same rules.  False: a pass per residual, as for every other form (tests
    # compare the two)
    linear_reuse = True

    def solve(self, func: Function):
        """dolfinx.nls.petsc.NewtonSolver.solve [ext]: F; while not converged and
        it < max_it: J, solve J dx = b, x -= dx, F, convergence test on ||b||.
        F (with Dirichlet lifting) and J come from one fused pass over the mesh."""
        ctx = get_context()
        mesh, F = self.mesh, self.F
        dm = mesh.device(ctx)
        n = mesh.n_vert
        b = _work(mesh, "newton_b", lambda: Vec(ctx, n))
        dx = _work(mesh, "newton_dx", lambda: Vec(ctx, n))
        ds = _dirichlet_set(mesh, self.bcs)
        aux = _aux(F)
        reuse = self.linear_reuse and getattr(F, "constant_partials", False) and F.pde_kind == _lib.PDE_POISSON
        offered = _offered_linearisation(F, self.bcs) if reuse else None
        if offered is not None:
            K, A = offered
        else:
            A = _work(mesh, "newton_A", lambda: SparseMatrix(mesh, symmetric=F.is_symmetric))
            A.pde_kind = F.pde_kind
        if reuse:
            if offered is None:
                K = _work(mesh, "newton_K", lambda: SparseMatrix(mesh, symmetric=F.is_symmetric))
                K.pde_kind = F.pde_kind
                # the operator of this solve: needs neither f nor u, so it runs under an upload of f that is still in flight,
                # and so does S A S (one rank: as in the library's deferred pass, whether to scale early is not a decision
                # ranks may take differently)
                E.assemble_system(dm, F.pde_kind, F.params, F.u.vec, F.f.vec, ds, K.mat, A.mat, None, aux=aux)
                if ctx.nranks == 1 and A.symmetric and KSP_OPTIONS.get("pc") in ("bpx", "jacobi"):
                    A.mat.prescale()

            def residual_pass(with_matrix, flagged=False):
                E.newton_rhs_linear(K.mat, F.f.vec, F.u.vec, ds, b, flagged=flagged)
        else:
            def residual_pass(with_matrix, flagged=False):
                E.assemble_system(dm, F.pde_kind, F.params, F.u.vec, F.f.vec, ds, None, A.mat if with_matrix else None, b,
                                  aux=aux)
        # F (with Dirichlet lifting) and J at the current iterate, one pass over the mesh
        residual_pass(True)
        n_own = dm.n_rows          # dots run over owned rows (all-reduced across ranks in the library)
        r0 = r = float(np.sqrt(b.dot(b, n_own)))
        self.residual_norms = [r]
        converged = r < self.atol or (r0 > 0 and 1.0 < self.rtol)
        it = 0
        opts = dict(KSP_OPTIONS)
        z0 = None
        energy_scale = None
        eps = np.finfo(np.float64).eps
        bpx_energy = opts.get("pc") == "bpx" and A.pde_kind in _BPX_KINDS
        # Every scalar a Newton step looks at -- ||F||, ||u|| (noise floor of the next solve), ||dx|| (SNES step test),
        # u.Au (energy scale of the next solve's threshold) -- comes from ONE reduction and one host synchronisation
        # after the assembly pass (Vec.dots); rounds 1-3 drained the stream for each of them.
        unorm = uAu = None
        g2 = None
        rho_b = None               # rho_0 of the NEXT solve, when the last reduction carried it (round 6)
        # A pass that does not solve (below) leaves dx = 0 off the Dirichlet rows and b_i = u_i - g_i on them: once the state
        # carries its boundary values exactly, dx is all +0.0, the update writes back the u it read and the next right-hand side
        # is, bit for bit, the one in place.  The identity solve says so in a device-side flag, and the update and the product
        # behind it are handed that flag and leave early while it is down (LOG R18).  Every launch and every record stays; the
        # host never looks at the flag, and the library hands it on only while b provably is the right-hand side of this very
        # u.  One rank, linear form; FEMO_NEWTON_FLAG=0 (read here, once per solve): the plain launches.
        use_flag = (reuse and ctx.nranks == 1 and os.environ.get("FEMO_NEWTON_FLAG", "1") != "0" and E.has_newton_flag())
        while not converged and it < self.max_it:
            if it > 0:
                # (a NaN ||u|| gives no noise floor -- max() would drop it without a word -- and, below, no skip either: the
                # pass goes to the solver, whose own rule says -1 for the residual of such a state)
                noise = self.NOISE_FACTOR * eps * unorm
                opts["atol"] = max(KSP_OPTIONS["atol"], KSP_OPTIONS["rtol"] * z0, noise if noise == noise else 0.0)
                if bpx_energy:
                    # Later corrections are solved to the accuracy the first solve aims at, measured against the
                    # STATE: sqrt(r^T M^-1 r) ~ energy norm of the error, threshold rtol_bpx * sqrt(u^T A u) (interior
                    # rows).  From a good initial state (u = 0 in bench.py) the first solve already is that accurate
                    # and these solves stop before their first iteration; from u = 1 (CSDL's default) the first
                    # correction is O(1), 1e-11 of it is 1e-7 of the state, and the second Newton step does the rest.
                    # The threshold is a scale, not a result: when the correction just applied did not iterate (it was
                    # below the previous threshold, i.e. below rtol_bpx of the state in the energy norm) the state's
                    # energy is unchanged to that accuracy and the product A u (0.28 ms at C4) is not repeated.
                    if uAu is not None:
                        if g2 is None:
                            g2 = 0.0
                            if ds is not None:
                                # kept on the set (its dofs and values are fixed for its lifetime): the mask and the sum over
                                # 280 k boundary values cost 0.4 ms of idle device per cycle at C4 (round 5)
                                cached = getattr(ds, "_g2_own", None)
                                if cached is not None and cached[0] == n_own:
                                    g2 = cached[1]
                                else:
                                    own = ds.vals[ds.dofs < n_own]                  # identity rows: (A u)_i = u_i = g_i
                                    g2 = float(np.square(own).sum())    # not np.dot: the first BLAS call starts a pool of spinning
                                    #                                     threads (one per core) that eats the process's CPU quota
                                    if ctx.nranks > 1:
                                        g2 = float(ctx.allreduce_sum([g2])[0])       # every rank must use the same threshold
                                    ds._g2_own = (n_own, g2)
                        energy_scale = float(np.sqrt(max(uAu - g2, 0.0)))
                    opts["atol_pc"] = opts.get("rtol_bpx", 1e-11) * energy_scale
            # Round 6: the solver's own first decision -- "nothing to iterate on": rho_0 = b^T D^-1 b over the non-identity
            # rows is zero or not above atol^2 (k_pcg_setup / the classic loops) -- taken HERE from the number that came back
            # with this pass's reduction (Vec.dots_rhs), so that a pass whose correction is below the rounding error of the
            # assembled residual (Newton's passes 2 and 3 of a linear form) costs one small launch instead of a solver
            # set-up, a first application and a host round trip.  Same numbers, same rule, same result (identity rows solved,
            # zero elsewhere); the solve is still reported (0 iterations).
            # A rho_0 that is NaN is not "nothing to iterate on": the solver's rule reports it as converged = -1, so it is the
            # solver that gets it (the record of the path without the probe), never the identity solve's converged = 1.
            skip = (rho_b is not None and A.symmetric and not hasattr(A, "backend_solve")
                    and rho_b == rho_b and (it == 0 or unorm == unorm)
                    and (rho_b == 0.0 or not (np.sqrt(rho_b) > opts["atol"])))
            if skip:
                A.mat.identity_solve(b, dx, flagged=use_flag)
                ksp_its = 0
                LAST_KSP_INFO.append(dict(thread=threading.get_ident(), iterations=0, converged=1, residual_norm=float(np.sqrt(rho_b)),
                                          rhs_norm=float(np.sqrt(rho_b)), pc_residual_norm=0.0, pc_rhs_norm=0.0, solve_ms=0.0, spmv_ms=0.0,
                                          spmv_samples=0, loop_allreduces=0, skipped_by_newton=True))
            else:
                ksp = KSP(A, opts)
                ksp.solve(b, dx)
                if z0 is None:
                    z0 = ksp.info.rhs_norm
                ksp_its = ksp.info.iterations
            self.ksp_iterations.append(ksp_its)
            flagged = skip and use_flag
            func.vec.axpy(-1.0, dx, flagged=flagged)
            it += 1
            # next pass: residual for the convergence test and, in the same launch, the Jacobian the
            # next iteration will use.  After the last allowed iteration nothing consumes a Jacobian
            # (the reference assembles J only when it iterates again), so that pass is residual-only.
            residual_pass(it < self.max_it, flagged)
            pairs = [(b, b)]
            more = it < self.max_it
            want_energy = more and bpx_energy and (energy_scale is None or self.ksp_iterations[-1] > 0)
            if more or self.stol > 0.0:
                pairs.append((func.vec, func.vec))
            if self.stol > 0.0:
                pairs.append((dx, dx))
            if want_energy:
                Au = _work(mesh, "newton_Au", lambda: Vec(ctx, n))
                A.mult(func.vec, Au)
                pairs.append((func.vec, Au))
            # (with another solve to come and its operator just assembled: rho_0 of that solve rides in the same reduction)
            probe = more and F.is_symmetric and self.newton_probe
            if probe:
                vals = Vec.dots_rhs(pairs, n_own, A.mat, b)
                rho_b = vals.pop()
            else:
                vals = Vec.dots(pairs, n_own)
                rho_b = None
            r = float(np.sqrt(vals[0]))
            unorm = float(np.sqrt(vals[1])) if len(vals) > 1 else None
            step_small = self.stol > 0.0 and vals[2] < (self.stol ** 2) * vals[1]
            uAu = vals[-1] if want_energy else None
            self.residual_norms.append(r)
            converged = r < self.atol or (r0 > 0 and r / r0 < self.rtol) or step_small
            if self.report:
                print(f"Newton iteration {it}: r (abs) = {r:.6e} (tol = {self.atol:g}) "
                      f"r (rel) = {r / r0 if r0 > 0 else 0.0:.6e} (tol = {self.rtol:g})")
        self.iterations = it
        if not converged and self.error_on_nonconvergence:
            raise RuntimeError("Newton solver did not converge")
        return it, converged


class NewtonSolverHIP(_NewtonBase):
    pass


def NewtonSolver(F, w, bcs=[], abs_tol=1e-50, rel_tol=1e-30, max_it=3, initialize=False,
                 error_on_nonconvergence=False, report=False):
    """utils_dolfinx.py:419-449.  Tolerances as in the reference => always
    ``max_it`` iterations; non-convergence is silent."""
    if initialize is True:
        w.vector.set(0.1)                               # utils_dolfinx.py:433-435
    return NewtonSolverHIP(F, w, bcs, abs_tol, rel_tol, max_it, report, error_on_nonconvergence)


class SNESSolverHIP(_NewtonBase):
    def getConvergedReason(self):
        return 3 if self._converged else -5             # SNES_CONVERGED_FNORM_RELATIVE / DIVERGED_MAX_IT

    def solve(self, b_unused, x):
        func = self.w
        it, self._converged = super().solve(func)
        return it


def SNESSolver(F, w, bcs=[], abs_tol=1e-13, rel_tol=1e-13, max_it=100, report=False):
    """utils_dolfinx.py:376-416: newtonls, full step, atol = rtol = 1e-13, LU -> CG.  The
    reference leaves PETSc's step tolerance at its default (stol = 1e-8: converged when
    ||dx|| < stol ||x|| [ext]), which is what ends the iteration once ||F|| sits on round-off."""
    s = SNESSolverHIP(F, w, bcs, abs_tol, rel_tol, max_it, report, True)
    s.stol = 1e-8
    return s


def solveNonlinear(res, func, bc, solver, report, initialize):
    """utils_dolfinx.py:319-333."""
    start = default_timer()
    if isinstance(res, BackendForm):
        if initialize is True:
            func.vector.set(0.1)                           # utils_dolfinx.py:433-435
        res.solve_state(func, bc, report)
    elif solver == 'Newton':
        newton_solver = NewtonSolver(res, func, bc, initialize=initialize, report=report)
        newton_solver.solve(func)
    elif solver == 'SNES':
        snes_solver = SNESSolver(res, func, bc, report=report)
        snes_solver.solve(None, func.vector)
        if report is True:
            print("Converged reason:", snes_solver.getConvergedReason())
    else:
        raise ValueError(f"unknown PDE_SOLVER {solver!r}")
    stop = default_timer()
    if report is True:
        print("Solve nonlinear finished in ", stop - start, "seconds")


# ---------------------------------------------------------------- projection ----
def _cell_values(expr: FieldExpression, mesh: Mesh) -> Optional[Vec]:
    """DG0 values of a cell-wise constant expression, or None for a CG1 Function."""
    ctx = get_context()
    dm = mesh.device(ctx)
    if isinstance(expr, FunctionExpr):
        return expr.fn.vec if expr.fn.function_space.family == "DG" else None
    out = _work(mesh, "proj_cells", lambda: Vec(ctx, mesh.n_cell))
    if isinstance(expr, GradientMagnitude):
        return E.cell_expression(dm, 0, None, expr.fn.vec, out)
    if isinstance(expr, PowerExpr):
        return E.cell_expression(dm, 1, [expr.p], expr.fn.vec, out)
    raise NotImplementedError(f"project: {type(expr).__name__} is not in the form catalogue")


def project(v, target_func: Function, bcs=[], lump_mass=False):
    """utils_dolfinx.py:549-583: L2 projection onto the (CG1) space of ``target_func``.
    b_i = int v phi_i; lump_mass: x = b / (M 1); else solve M x = b (the reference uses PETSc's
    default KSP, rtol 1e-5 [ext]; here Jacobi-CG at the KSP_OPTIONS tolerance)."""
    if isinstance(v, BackendForm) and hasattr(v, "project_field"):
        if bcs:
            raise NotImplementedError("project with Dirichlet conditions")
        return v.project_field(target_func, lump_mass)
    if isinstance(v, Function):
        v = FunctionExpr(v)
    if not isinstance(v, FieldExpression):
        raise NotImplementedError(f"project: {type(v).__name__} is not in the form catalogue")
    if bcs:
        raise NotImplementedError("project with Dirichlet conditions")
    V = target_func.function_space
    if V.family != "CG":
        raise NotImplementedError("project onto a space other than CG1")
    mesh = V.mesh
    ctx = get_context()
    dm = mesh.device(ctx)
    n = mesh.n_vert
    b = _work(mesh, "proj_b", lambda: Vec(ctx, n))
    load = _work(mesh, "proj_load", lambda: CellMatrix(mesh))       # -(int_c phi_a) per (cell, a)
    E.assemble_dRdf(dm, _lib.PDE_POISSON, None, None, None, load.vals)
    cells = _cell_values(v, mesh)
    M = None
    if cells is not None:
        load.mult(cells, b)                                          # b = -(sum_c w_c |T_c|/(d+1))
        sign = -1.0
    else:
        M = _work(mesh, "proj_M", lambda: SparseMatrix(mesh, symmetric=True))
        M.pde_kind = _lib.PDE_MASS
        E.assemble_jacobian(dm, _lib.PDE_MASS, None, None, None, None, M.mat)
        M.mult(v.fn.vec, b)
        sign = 1.0
    if lump_mass:
        ones = _work(mesh, "proj_ones", lambda: Vec(ctx, mesh.n_cell)).fill(1.0)
        lumped = _work(mesh, "proj_lumped", lambda: Vec(ctx, n))
        load.mult(ones, lumped)                                      # -(M 1)
        E.pointwise_divide(target_func.vec, b, lumped, dm.n_rows)    # (sign b') / (-(M 1)) handled below
        if sign > 0:                                                 # b = +M v: flip (lumped carries a minus)
            tmp = _work(mesh, "proj_tmp", lambda: Vec(ctx, n)).fill(0.0)
            tmp.axpy(-1.0, target_func.vec)
            target_func.vec.copy_from(tmp)
    else:
        if M is None:
            M = _work(mesh, "proj_M", lambda: SparseMatrix(mesh, symmetric=True))
            M.pde_kind = _lib.PDE_MASS
        E.assemble_jacobian(dm, _lib.PDE_MASS, None, None, None, None, M.mat)
        if sign < 0:
            rhs = _work(mesh, "proj_tmp", lambda: Vec(ctx, n)).fill(0.0)
            rhs.axpy(-1.0, b)
        else:
            rhs = b
        KSP(M).solve(rhs, target_func.vec)
    target_func.version += 1


# --------------------------------------------------------------------- norms ----
def errorNorm(v: Function, v_ex: Function, norm: str = 'L2') -> float:
    """utils_dolfinx.py:225-238: sqrt(int (v - v_ex)^2 [+ |grad(v - v_ex)|^2 for 'H1']), exact for the
    P1 / DG0 functions of the engine (host-side, not on the hot path)."""
    if norm not in ('L2', 'H1'):
        raise NotImplementedError("errorNorm: norm must be 'L2' or 'H1'")
    mesh = v.function_space.mesh
    X = mesh.x[mesh.conn]
    E_ = X[:, 1:, :] - X[:, :1, :]
    vol = np.abs(np.linalg.det(E_)) / (2.0 if mesh.tdim == 2 else 6.0)
    d = mesh.tdim

    def nodal(fn):
        a = fn.vector.getArray()
        return a[mesh.conn] if fn.function_space.family == "CG" else np.repeat(a[:, None], d + 1, axis=1)

    e = nodal(v) - nodal(v_ex)
    s = e.sum(axis=1)
    val = (vol / ((d + 1) * (d + 2)) * ((e ** 2).sum(axis=1) + s ** 2)).sum()
    if norm == 'H1':
        # grad of the P1 interpolant of e per cell: solve E_^T-system for the gradient of the differences
        de = e[:, 1:] - e[:, :1]                                   # (n_cell, d)
        grad = np.linalg.solve(E_, de[:, :, None])[:, :, 0]        # rows of E_ are edge vectors: E_ grad = de
        val += (vol * (grad ** 2).sum(axis=1)).sum()
    return float(np.sqrt(val))
