"""Heat conduction with a penalised conductivity on the HIP engine: the second physics of the SIMP track, the heat-sink
problem, and the temperature of the thermoelastic chain rho -> T(rho) -> u(rho, T) -> J (kernels in csrc/conduction.hip;
tests/thermal_ref.py restates them).  The forms are ``BackendForm``s like those of fea/elasticity.py: `FEA.add_input /
add_state / add_output`, `StateOperation`, `OutputOperation` and `FEAModel` are used unchanged.  A thermal `FEA` whose state
is named ``temperature`` feeds an elastic `FEA` with an input of that name (`ThermalExpansion` of fea/elasticity.py) in one
`FEAModel(fea=[...])`: the reverse sweep then needs two adjoint solves, one per state.

  ConductionResidual   R(T; rho) = K_theta(rho) T - Q,  K_theta = sum_c k(rho_c) |T_c| grad phi_a . grad phi_b on the mesh's
                       scalar pattern, k(rho) = k_min + (k0 - k_min) C(rho) with C = rho^3 (SIMP) or rho / (1 + 8 (1 - rho))
                       (RAMP).  Q is the P1 load of a volumetric source (a number or a DG0 Function: q_c |T_c| / (d + 1) at
                       every vertex of c) plus a facet flux on ``ds`` lumped like the traction (|f| / d at every vertex of f);
                       it does not depend on rho.  dR/drho = k'(rho) |T_c| grad phi_v . grad T_c, matrix free, forward and
                       reverse one launch each.  Dirichlet values may be non-zero (a sink temperature): the right-hand side
                       is the lifting b = Q - K_theta g, b = g on the fixed set.  The state and adjoint solves are
                       `femo_solve_cg` to ``rtol`` (1e-13), Jacobi-scaled by default; ``preconditioner="multilevel"`` adds
                       the auxiliary-lattice BPX of csrc/bpx.hip with level weights theta / diag(P_l^T K_theta P_l) formed
                       on the device once per assembly (tests/cond_pc_ref.py restates them), whose iteration count does not
                       grow with the mesh; its stopping norm is that of the preconditioner, sqrt(r^T M^-1 r) <= rtol
                       sqrt(b^T M^-1 b).  A solve that does not converge raises
  ThermalCompliance    J = Q^T T, dJ/dT = Q, nothing with respect to rho

Out of scope: the lattice preconditioner as the default, a V-cycle or off-diagonal Galerkin operators on the lattices (the
weights are diagonals), convection (Robin) boundaries, design-dependent sources, temperature-dependent material data,
partitioned meshes.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .. import _lib
from .._lib import check
from ..engine import PC_KINDS, Vec, _ptr
from .elasticity import METHODS, PRECONDITIONERS, Measure, _ctx, _fixed_data, lumped_facet_measure, cell_volumes
from .forms import BackendForm
from .function import Function, FunctionSpace


class DeviceConduction:
    """femo_cond: K_theta(rho) and its eliminated form on the mesh's scalar pattern, the lifting, the PCG solve (Jacobi or the
    lattice preconditioner) and the two density products."""

    def __init__(self, ctx, mesh):
        self.ctx, self.lib, self.mesh = ctx, ctx.lib, mesh
        self.dm = mesh.device(ctx)
        h = _lib.H()
        check(self.lib.femo_cond_create(self.dm.handle, C.byref(h)))
        self.handle = h
        self.n_vert, self.n_cell = int(self.dm.n_vert), int(self.dm.n_cell)
        self.nnz = int(self.dm.info["nnz"])
        self._bc = None                     # the DirichletSet of the last assembly, kept alive with it
        self._rho = None                    # ... and its density: the lattice weights are formed from it at the first solve
        self._work = None

    def assemble(self, method: int, k0: float, k_min: float, rho: Vec, bc=None) -> None:
        """K_theta(rho), and with the `engine.DirichletSet` ``bc`` the eliminated matrix beside it (one launch)."""
        check(self.lib.femo_cond_assemble(self.handle, int(method), float(k0), float(k_min), rho.handle,
                                          None if bc is None else bc.handle))
        self._bc, self._rho = bc, rho

    def apply(self, x: Vec, y: Vec, eliminated: bool = False) -> Vec:
        check(self.lib.femo_cond_apply(self.handle, int(bool(eliminated)), x.handle, y.handle))
        return y

    def lift(self, q: Vec, b: Vec, g: Optional[Vec] = None) -> Vec:
        """b = g on the fixed set (0 without g), q - K_theta g elsewhere."""
        if g is not None and self._work is None:
            self._work = Vec(self.ctx, int(self.dm.n_rows))
        check(self.lib.femo_cond_lift(self.handle, q.handle, None if g is None else g.handle,
                                      None if g is None else self._work.handle, b.handle))
        return b

    def solve(self, b: Vec, x: Vec, rtol: float = 1e-13, atol: float = 0.0, max_it: int = 1_000_000, check_every: int = 8,
              zero_guess: bool = True, pc: str = "jacobi") -> "_lib.SolveInfo":
        """PCG; ``pc`` = "jacobi" or "multilevel" (the lattice preconditioner weighted with this operator's Galerkin
        diagonals; ``rtol`` is then relative in the norm of the preconditioner)."""
        if pc not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {pc!r} (jacobi or multilevel)")
        opts = _lib.SolverOpts(float(rtol), float(atol), int(max_it), int(bool(zero_guess)), int(check_every),
                               PC_KINDS["bpx" if pc == "multilevel" else "jacobi"], 0.0)
        info = _lib.SolveInfo()
        check(self.lib.femo_cond_solve(self.handle, b.handle, x.handle, C.byref(opts), C.byref(info)))
        return info

    def pc_apply(self, r: Vec, z: Vec) -> Vec:
        """z = M^-1 r with the lattice preconditioner of the current assembly, in unscaled variables."""
        check(self.lib.femo_cond_pc_apply(self.handle, r.handle, z.handle))
        return z

    def pc_info(self) -> dict:
        """Lattice levels, nodes per level (coarsest first) and how often the Galerkin diagonals were formed."""
        out = np.zeros(34, np.int64)
        check(self.lib.femo_cond_pc_info(self.handle, _ptr(out), len(out)))
        nl = int(out[0])
        return dict(levels=nl, builds=int(out[1]), nodes=[int(v) for v in out[2:2 + nl]])

    def pc_level_weights(self, level: int) -> np.ndarray:
        """C_level = keep theta / diag(P_l^T A P_l) of the current assembly."""
        nodes = self.pc_info()["nodes"]
        if not 0 <= level < len(nodes):
            raise ValueError(f"level {level} of {len(nodes)}")
        out = np.zeros(nodes[level])
        check(self.lib.femo_cond_pc_export_level(self.handle, int(level), _ptr(out)))
        return out

    def drho(self, method: int, k0: float, k_min: float, transpose: bool, rho: Vec, T: Vec, x: Vec, y: Vec, a: float = 1.0,
             accumulate: bool = False) -> Vec:
        """forward: y[n_vert] (+)= a sum_c k'(rho_c) x_c |T_c| grad phi_v . grad T_c; transposed: y[n_cell] (+)= a k'(rho_c)
        |T_c| grad x_c . grad T_c."""
        check(self.lib.femo_cond_drho(self.handle, int(method), float(k0), float(k_min), int(bool(transpose)), float(a),
                                      rho.handle, T.handle, x.handle, y.handle, int(bool(accumulate))))
        return y

    def export_csr(self, eliminated: bool = False):
        """scipy CSR of K_theta, or of the eliminated matrix."""
        import scipy.sparse as sp
        rowptr = np.zeros(int(self.dm.n_rows) + 1, np.int64)
        col = np.zeros(self.nnz, np.int32)
        val = np.zeros(self.nnz)
        check(self.lib.femo_cond_export_csr(self.handle, int(bool(eliminated)), _ptr(rowptr), _ptr(col), _ptr(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(int(self.dm.n_rows), self.n_vert))

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None) and getattr(self.dm, "handle", None):
                self.lib.femo_cond_destroy(h)
        except Exception:
            pass


def conduction_handle(mesh) -> DeviceConduction:
    """One handle per (mesh, context)."""
    ctx = _ctx()
    cache = mesh.__dict__.setdefault("_cond", {})
    h = cache.get(id(ctx))
    if h is None or h.ctx is not ctx:
        h = cache[id(ctx)] = DeviceConduction(ctx, mesh)
    return h


def _check_scalar_space(name: str, T: Function):
    Q = T.function_space
    if not isinstance(Q, FunctionSpace) or Q.family != "CG":
        raise NotImplementedError(f"{name} needs a FunctionSpace(mesh, ('CG', 1)) temperature")
    mesh = Q.mesh
    if getattr(mesh, "tdim", None) not in (2, 3) or mesh.conn.shape[1] != mesh.tdim + 1:
        raise NotImplementedError(f"{name} needs a 2-D or 3-D simplex Mesh")
    if getattr(mesh, "local", None) is not None and mesh.local.nranks > 1:
        raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
    return mesh


def heat_load(mesh, source=None, flux=None, ds: Optional[Measure] = None) -> np.ndarray:
    """Q on the host: q_c |T_c| / (d + 1) at every vertex of cell c for the source (a number or a DG0 Function) plus ``flux``
    times the lumped facet measure of ``ds``.  Neither may depend on the density."""
    d = mesh.tdim
    Q = np.zeros(mesh.n_vert)
    if source is not None:
        if isinstance(source, Function):
            if source.function_space.family != "DG" or source.function_space.mesh is not mesh:
                raise NotImplementedError("the heat source needs a number or a DG0 Function on the temperature's mesh")
            q = np.array(source.vector.getArray(), dtype=np.float64)
        else:
            q = np.full(mesh.n_cell, float(source))
        np.add.at(Q, mesh.conn.ravel(), np.repeat(q * cell_volumes(mesh) / (d + 1), d + 1))
    if flux is not None:
        if ds is None:
            ds = Measure("ds", domain=mesh)
        Q += float(flux) * lumped_facet_measure(mesh, ds.facets())
    return Q


class _HeatLoad:
    """Q of a form on the device, rebuilt when a source Function was written."""

    def __init__(self, name: str, mesh, source, flux, ds):
        if source is None and flux is None:
            raise ValueError(f"{name}: the load needs a source or a flux")
        if isinstance(source, Function):
            if source.function_space.family != "DG" or source.function_space.mesh is not mesh:
                raise NotImplementedError(f"{name}: the heat source needs a number or a DG0 Function on the temperature's mesh")
        elif source is not None:
            source = float(source)
        self.mesh, self.source, self.flux, self.ds = mesh, source, None if flux is None else float(flux), ds
        self.vec, self.key = None, None

    def get(self) -> Vec:
        key = (id(_ctx()), self.source.version if isinstance(self.source, Function) else None)
        if key != self.key:
            self.vec = Vec(_ctx(), self.mesh.n_vert).set(heat_load(self.mesh, self.source, self.flux, self.ds))
            self.key = key
        return self.vec


class ConductionMatrix:
    """dR/dT = K_theta(rho); with ``masked`` the eliminated matrix (identity rows / columns on the fixed vertices).
    `backend_solve` is the PCG of the form, with its preconditioner."""
    symmetric = True
    pde_kind = None

    def __init__(self, form: "ConductionResidual", masked: bool = False):
        self.form, self.masked, self.mesh = form, masked, form.mesh
        self._row = None
        self.info = None

    def getSizes(self):
        return (self.mesh.n_vert, self.mesh.n_vert)

    size = property(getSizes)

    def mult(self, x: Vec, y: Vec) -> Vec:
        dev = self.form.operator()
        return dev.apply(x, y, eliminated=self.masked and self.form._mask is not None)

    multTranspose = mult

    def new_row_vec(self) -> Vec:
        if self._row is None:
            self._row = Vec(_ctx(), self.mesh.n_vert)
        return self._row

    new_col_vec = new_row_vec

    def backend_solve(self, b: Vec, x: Vec, options: Optional[dict] = None) -> None:
        o = options or {}
        F = self.form
        info = F.operator().solve(b, x, rtol=o.get("cond_rtol", F.rtol), max_it=o.get("cond_max_it", 1_000_000),
                                  pc=F.preconditioner)
        self.info = F._record(info, "adjoint")

    def to_scipy(self):
        return self.form.operator().export_csr(eliminated=self.masked and self.form._mask is not None)


class _ConductionDrho:
    """dR/drho (n_vert x n_cell), matrix free: column c = k'(rho_c) |T_c| grad phi_v . grad T_c."""

    def __init__(self, form: "ConductionResidual"):
        self.form, self.mesh = form, form.mesh
        self._row = self._col = None

    def getSizes(self):
        return (self.mesh.n_vert, self.mesh.n_cell)

    def _apply(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        return F.device().drho(F.method_id, F.k0, F.k_min, transpose, F.rho.vec, F.u.vec, x, y)

    def mult(self, x: Vec, y: Vec) -> Vec:
        return self._apply(False, x, y)

    def multTranspose(self, x: Vec, y: Vec) -> Vec:
        return self._apply(True, x, y)

    def new_row_vec(self) -> Vec:
        if self._row is None:
            self._row = Vec(_ctx(), self.mesh.n_vert)
        return self._row

    def new_col_vec(self) -> Vec:
        if self._col is None:
            self._col = Vec(_ctx(), self.mesh.n_cell)
        return self._col


class ConductionResidual(BackendForm):
    """R(T; rho) = K_theta(rho) T - Q (see the module docstring).  ``source``: a number or a DG0 Function; ``flux``: a number on
    the facets of ``ds``.  ``rtol`` (1e-13, the stopping level of the PDE filter) is that of the state and adjoint solves,
    ``preconditioner`` ("jacobi", the default, or "multilevel": see the module docstring) theirs; ``last_info[kind]`` keeps the record of the last solve of each kind ("state", "adjoint").  Q is non-zero on the fixed
    vertices, and so is the multiplier of an output such as `ThermalCompliance`: the exact reduced gradient needs
    ``fea.consistent_bc_partials = True``, as for the body and thermal loads of the elasticity."""
    rank = 1
    is_linear = True
    is_symmetric = True
    constant_partials = False
    matrix_class = ConductionMatrix

    def __init__(self, T: Function, rho: Function, source=None, flux=None, ds: Optional[Measure] = None, k0: float = 1.0,
                 k_min: float = 0.0, method: str = "SIMP", preconditioner: str = "jacobi"):
        name = "ConductionResidual"
        mesh = _check_scalar_space(name, T)
        if rho.function_space.family != "DG" or rho.function_space.mesh is not mesh:
            raise NotImplementedError(f"{name} needs a DG0 density on the temperature's mesh")
        if method not in METHODS:
            raise ValueError(f"unknown penalisation method {method!r} (SIMP or RAMP)")
        if preconditioner not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {preconditioner!r} (jacobi or multilevel)")
        self.preconditioner = preconditioner
        k0, k_min = float(k0), float(k_min)
        if not (np.isfinite(k0) and np.isfinite(k_min) and 0.0 <= k_min < k0):
            raise ValueError(f"{name}: finite conductivities with 0 <= k_min < k0 are needed")
        self.u = self.T = T
        self.rho, self.mesh = rho, mesh
        self.k0, self.k_min, self.method, self.method_id = k0, k_min, method, METHODS[method]
        self._load = _HeatLoad(name, mesh, source, flux, ds)
        self.rtol = 1e-13
        self._mask = self._vals = None
        self._bc = None
        self._res = self._b = self._g = None
        self.last_info = {}

    def functions(self):
        return (self.u, self.rho)

    def device(self) -> DeviceConduction:
        return conduction_handle(self.mesh)

    def load(self) -> Vec:
        return self._load.get()

    def _set_bcs(self, bcs) -> None:
        mask, vals = _fixed_data(self.mesh.n_vert, bcs)
        if mask is None or not mask.any():
            self._mask = self._vals = self._bc = None
            return
        if self._mask is None or not np.array_equal(mask, self._mask) or not np.array_equal(vals, self._vals):
            from ..engine import DirichletSet
            dofs = np.nonzero(mask)[0].astype(np.int32)
            self._bc = DirichletSet(self.mesh.device(_ctx()), dofs, vals[dofs])
            self._mask, self._vals = mask, vals
            self._g = None

    def operator(self) -> DeviceConduction:
        """The handle with K_theta(rho) of the current density and this form's fixed set: reassembled when either changed."""
        dev = self.device()
        key = (self.rho.version, id(self.rho.vec), id(self._bc), self.method_id, self.k0, self.k_min, id(self))
        if getattr(dev, "_owner", None) != key:
            dev.assemble(self.method_id, self.k0, self.k_min, self.rho.vec, self._bc)
            dev._owner = key
        return dev

    def _record(self, info, kind: str):
        from .utils_hip import LAST_KSP_INFO
        self.last_info[kind] = dict(iterations=info.iterations, converged=info.converged, solve_ms=info.solve_ms,
                                    residual_norm=info.residual_norm, rhs_norm=info.rhs_norm,
                                    preconditioner=self.preconditioner)
        LAST_KSP_INFO.append(dict(self.last_info[kind], kind="conduction_" + kind))
        if info.converged != 1:
            raise RuntimeError(f"conduction PCG ({self.preconditioner}) did not converge ({kind}): {info.iterations} iterations, "
                               f"sqrt(r.D^-1 r) = {info.residual_norm:.3e} of {info.rhs_norm:.3e}")
        return info

    def new_matrix(self) -> ConductionMatrix:
        return self.matrix_class(self)

    def assemble_vector(self, out: Optional[Vec] = None) -> Vec:
        """K_theta(rho) T - Q"""
        if out is None:
            if self._res is None:
                self._res = Vec(_ctx(), self.mesh.n_vert)
            out = self._res
        self.operator().apply(self.u.vec, out)
        return out.axpy(-1.0, self.load())

    def partial_matrix(self, wrt: Function, out=None):
        if wrt is self.u:
            return out if isinstance(out, self.matrix_class) and not out.masked else self.matrix_class(self)
        if wrt is self.rho:
            return out if isinstance(out, _ConductionDrho) else _ConductionDrho(self)
        raise ValueError("the conduction residual does not depend on that Function")

    def assemble_system(self, bcs, rhs: bool, out, out_nobc):
        if rhs:
            raise NotImplementedError("assembleSystem(rhs=True) for the conduction form: use solveNonlinear / FEA.solve")
        self._set_bcs(bcs)
        self.operator()
        A = out if isinstance(out, self.matrix_class) else self.matrix_class(self)
        A.form, A.masked = self, True
        if isinstance(out_nobc, self.matrix_class):
            out_nobc.form, out_nobc.masked = self, False
        return A, None

    def _rhs(self, dev: DeviceConduction) -> Vec:
        """The lifting b = Q - K_theta g, b = g on the fixed set; Q itself without one."""
        Q = self.load()
        if self._mask is None:
            return Q
        if self._b is None:
            self._b = Vec(_ctx(), self.mesh.n_vert)
        g = None
        if np.any(self._vals[self._mask == 1] != 0.0):
            if self._g is None:
                self._g = Vec(_ctx(), self.mesh.n_vert).set(np.where(self._mask == 1, self._vals, 0.0))
            g = self._g
        return dev.lift(Q, self._b, g)

    def solve_state(self, func: Function, bcs, report: bool = False) -> None:
        """K_theta(rho) T = Q with the strongly imposed temperatures: one PCG solve (the form is linear)."""
        self._set_bcs(bcs)
        dev = self.operator()
        info = dev.solve(self._rhs(dev), func.vec, rtol=self.rtol, pc=self.preconditioner)
        func.version += 1
        self._record(info, "state")
        if report:
            print(f"conduction solve: {info.iterations} PCG iterations, {info.solve_ms:.1f} ms")


class ThermalCompliance(BackendForm):
    """J = Q^T T with the load Q of `ConductionResidual` (``source``, ``flux``, ``ds``): the thermal compliance of the
    heat-sink problem.  dJ/dT = Q; the form depends on T alone."""
    rank = 0

    def __init__(self, T: Function, source=None, flux=None, ds: Optional[Measure] = None):
        self.mesh = _check_scalar_space("ThermalCompliance", T)
        self.u = self.T = T
        self._load = _HeatLoad("ThermalCompliance", self.mesh, source, flux, ds)

    def functions(self):
        return (self.u,)

    def load(self) -> Vec:
        return self._load.get()

    def assemble_scalar(self) -> float:
        return self.load().dot(self.u.vec, self.mesh.n_vert)

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        out = self._gradient_buffer(wrt, out)
        return out.copy_from(self.load()) if wrt is self.u else out.fill(0.0)


def pdeRes_conduction(T, v, rho_e, source=None, flux=None, dss: Optional[Measure] = None, k0: float = 1.0, k_min: float = 0.0,
                      method: str = "SIMP", preconditioner: str = "jacobi") -> ConductionResidual:
    """The conduction residual in the style of `pdeRes`; ``v`` is implied by the catalogue."""
    return ConductionResidual(T, rho_e, source=source, flux=flux, ds=dss, k0=k0, k_min=k_min, method=method,
                              preconditioner=preconditioner)


def thermal_compliance(T, source=None, flux=None, dss: Optional[Measure] = None) -> ThermalCompliance:
    return ThermalCompliance(T, source=source, flux=flux, ds=dss)
