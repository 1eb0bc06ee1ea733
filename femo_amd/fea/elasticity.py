"""SIMP topology optimisation on the HIP engine: the linear-elasticity state, its loads and outputs, and the device
handles of the density filter (examples/beam_topo_opt/run_topo_opt_cantilever_beam.py; kernels in csrc/elasticity.hip,
product and PCG in csrc/elast_solve.hip, stress in csrc/elast_stress.hip, the displacement aggregate in csrc/elast_disp.hip, body loads in csrc/elast_body.hip, thermal loads in csrc/elast_thermal.hip, eigenfrequencies in csrc/elast_eig.hip,
buckling in csrc/elast_buckle.hip, the block iteration of both in csrc/elast_block.hip, the harmonic response in csrc/elast_harm.hip, its damped form in csrc/elast_damp.hip, the transient response in csrc/elast_transient.hip).  One load case is the L = 1 case of several:
each form is written once, and the MultiLoad... names adapt the constructor arguments and the presentation.

The forms are ``BackendForm``s, like the shell forms: `utils_hip.assemble*`, `solveNonlinear` and `KSP` hand them their
own assembly and solves, so `FEA.add_input / add_state / add_output`, `StateOperation`, `OutputOperation` and `FEAModel`
are used unchanged.

  ElasticityResidual   R(u; rho) = sum_e C(rho_e) int_e sigma_0(u) : eps(v) dx - int_ds(tag) t . v ds   (pdeRes, :85-101)
                       C = rho^3 (SIMP) or rho / (1 + 8 (1 - rho)) (RAMP); sigma_0 = lambda_0 tr(eps) I + 2 mu_0 eps with
                       lambda_0 = E nu / ((1 + nu)(1 - 2 nu)), mu_0 = E / (2 (1 + nu)) -- plane strain in 2-D
  Compliance           J = int_ds(tag) t . u ds = F^T u                                                 (compliance, :108-109)
  body forces          ``body_force`` / ``body_forces`` of the residuals and compliances: self-weight and inertial load cases
                       (gravity, pull-up, lateral manoeuvres).  b = mass density times acceleration, constant per load case;
                       the mass is linear in rho, so F(rho) = T + G_b rho with (G_b rho)[d v + i] = b_i sum_{e around v}
                       rho_e |T_e| / (d + 1).  R = K(rho) u - F(rho), dR/drho = C'(rho) K0 u - G_b, J = sum_l w_l F_l(rho) . u_l
                       with dJ/drho = G_{wB}^T u: one launch each for all load cases (csrc/elast_body.hip).  Not in the
                       reference's script.  RAMP is the usual stiffness law here (SIMP's rho^3 against the linear mass gives
                       large displacements at low density), and the exact reduced gradient needs
                       ``fea.consistent_bc_partials = True``: F(rho) is non-zero on clamped vertices
  thermal loads        ``thermal=ThermalExpansion(alpha, temperature, T_ref, scales)`` of the static residuals and compliances:
                       sigma = C(rho) (sigma_0(u) - beta_0 theta I) on the 3 x 3 tensor, beta_0 = (3 lambda_0 + 2 mu_0) alpha (the
                       same constant in plane strain and in 3-D), theta = T - T_ref a number or a CG1 Function.  The load is
                       F_th = s_l H(C(rho); theta), H(w; theta)[d v + i] = sum_{e around v} w_e beta_0 thetabar_e |T_e| d_i phi_v,
                       thetabar_e the cell mean (exact for P1): it scales with the stiffness law, not with the mass.  dR/drho
                       gains -s_l H(C'(rho) . ; theta), and with a temperature Function the form depends on (u, rho, T) with
                       dR/dT = -s_l H(C(rho); .): one operator, three contractions, one launch each for all load cases
                       (csrc/elast_thermal.hip).  The temperature may be the state of a `ConductionResidual` (fea/conduction.py)
                       in another FEA of the same FEAModel: the thermoelastic chain rho -> T -> u -> J, two adjoint solves.
                       F_th is non-zero on clamped vertices: the exact reduced gradient needs
                       ``fea.consistent_bc_partials = True``.  The thermal stress is hydrostatic on the 3 x 3 tensor, so the von
                       Mises outputs below are already the thermoelastic ones.  Not in the harmonic, damped, transient, eigen
                       and buckling forms (refused); one temperature for all load cases.  Not in the reference's script
  elastic supports     ``springs`` of the static residuals: K_s(rho) = K(rho) + diag(k), one stiffness k >= 0 per dof from
                       `point_springs` (a workpiece, an input or output port) and `facet_springs` (a Winkler foundation, lumped
                       like the traction).  The handle carries them into the product, block-Jacobi and the lattice blocks of
                       the multilevel preconditioner; they do not depend on rho.  Not in the reference's script
  ElasticityDisplacement  J = sum_l w_l l_l . u_l: the displacement of a port (`port_displacement`) or the mean displacement
                       of a boundary (`mean_displacement`); with two port springs the objective of a compliant mechanism
  ElasticityPnormDisplacement  J = (1/alpha) sum_v a_v (m |u_v|)^p over a vertex list, a tagged boundary or the whole mesh:
                       "no vertex of this region moves more than delta" as one smooth output (csrc/elast_disp.hip)
  averageFunc          (1/|Omega|) int rho dx as a LinearFunctional with the DG0 coefficient |T_e| / |Omega| (:103-106)
  ElasticityPnormStress  J = (1/alpha) sum_e |T_e| (m rho_e^q sigma_vm,e)^p, the aggregated von Mises stress of the solid
                       material: sigma_vm = sqrt(3/2 s : s), s the deviator of sigma_0(u) as a 3 x 3 tensor (plane strain in
                       2-D: sigma_zz = lambda_0 tr eps); rho^q sigma_vm is the qp-relaxed cell stress.  Not in the reference's
                       script: the solid counterpart of the shell's pnorm_stress (shell_pde.py:297-313)
  ElasticityVonMises   the cell field rho_e^q sigma_vm,e for `project` / FEA.add_field_output
  MultiLoadElasticityResidual, MultiLoadCompliance
                       L load cases on one K(rho): the state is a Function(LoadCaseSpace(V, L)), column l solves
                       K(rho) u_l = F_l, and J = sum_l w_l F_l . u_l.  Every solve of the cycle -- state, adjoint, forward
                       mode -- is one batched PCG over all columns (csrc/elast_solve.hip)
  MultiLoadPnormStress J = sum_l w_l J_l with one aggregate J_l = (1/alpha) sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p per
                       load case of a LoadCaseSpace state: the values, dJ/du (column l = w_l dJ_l/du_l) and dJ/drho of all
                       load cases in one pass over the mesh (csrc/elast_stress.hip).  Its adjoint is one batched PCG
                       whose right-hand sides are not loads: they are non-zero on the clamped dofs of every column
  MultiLoadVonMises    the cell field max_l s_l rho_e^q sigma_vm,e(u_l) (the envelope over the load cases), or that of one
                       load case, for `project` / FEA.add_field_output
  ElasticityEigenvalues  the lowest eigenpairs of K(rho) phi = lambda M(rho) phi on the free dofs, M = density sum_e m(rho_e)
                       M0_e the consistent P1 mass with m = rho or Du & Olhoff's C^1 cut-off below rho = 0.1: block inverse
                       iteration with Rayleigh-Ritz, every inner solve one batched PCG over the block (csrc/elast_block.hip),
                       warm-started from the previous modes.  Not in the reference's script
  EigenvalueAggregate  J = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p), a smooth stand-in for the fundamental eigenvalue that is
                       symmetric within a cluster, as a scalar output of the density alone: dJ/drho = sum_k c_k (C'(rho_e)
                       phi_k^T K0_e phi_k - lambda_k density m'(rho_e) phi_k^T M0_e phi_k) in one launch, no adjoint solve.
                       ``n_modes`` should not split a cluster of (nearly) equal eigenvalues
  ElasticityBuckling   the smallest positive load factors of (K(rho) + lambda K_G(u, rho)) phi = 0 on the free dofs for the
                       state u of an `ElasticityResidual`: K_G the geometric stiffness of the cell stress C(rho_e) sigma_0(u_e),
                       matrix free.  Solved as (-K_G) phi = mu K phi, mu = 1 / lambda, for the largest positive mu by the block
                       iteration of the eigenfrequencies on another pencil (csrc/elast_block.hip), on the residual's
                       own K.  Not in the reference's script
  BucklingAggregate    J = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p) of the load factors, the aggregate of `EigenvalueAggregate`, as a
                       scalar output of (u, rho): dJ/du and dJ/drho are one launch each, and the framework's adjoint solve
                       K w = dJ/du does the rest.  dJ/du is non-zero on clamped dofs: the exact reduced gradient needs
                       ``fea.consistent_bc_partials = True``
  HarmonicElasticityResidual  the undamped harmonic response (K(rho) - omega_l^2 M(rho)) u_l = F_l in real arithmetic: one
                       K, one consistent mass M (that of `ElasticityEigenvalues`, assembled once per density as a scalar matrix
                       on the pattern of K), one fixed set; column l of a Function(LoadCaseSpace(V, L)) carries its own
                       frequency omega_l and its own load -- a frequency sweep is one state.  State, adjoint and forward-mode
                       solves are each ONE batched preconditioned MINRES (csrc/elast_harm.hip): above the first resonance the
                       matrix is indefinite, where PCG breaks down.  Not in the reference's script
  DynamicCompliance    J = sum_l w_l |F_l . u_l| (Ma, Kikuchi & Cheng 1995; Olhoff & Du 2005), or sum_l w_l (F_l . u_l)^2, of a
                       harmonic state: the usual companion of an eigenfrequency constraint
  DampedHarmonicElasticityResidual, DampedDynamicCompliance
                       the damped response (K - omega_l^2 M + i (c_K,l K + c_M,l M)) u_l = F_l in complex arithmetic, c_K = eta +
                       omega beta, c_M = omega alpha for a structural loss factor eta and Rayleigh damping alpha M + beta K; the
                       state is a Function(LoadCaseSpace(V, 2L)) with Re u_l in column 2 l and Im u_l in column 2 l + 1.  State,
                       adjoint (conj(Z)) and forward-mode solves are each ONE batched preconditioned COCR (Sogabe & Zhang
                       2007; csrc/elast_damp.hip), which converges at a resonance, where the undamped MINRES does not, and
                       J = sum_l w_l |F_l . u_l| (or its square) of the complex compliance is finite and differentiable there
  TransientElasticityResidual, TransientCompliance
                       the time-domain response by Newmark(beta, gamma) with Rayleigh damping, as the two-step recurrence in the
                       displacements from rest; the state is a Function(TimeHistorySpace(V, N)) holding u_1 ... u_N, the whole
                       history one state of the operator surface.  The history solves a block lower-banded block-Toeplitz
                       system with symmetric blocks, so the adjoint is the SAME march run backwards: state, forward-mode and
                       adjoint solves are one device-resident loop (csrc/elast_transient.hip), each step one fused
                       right-hand-side launch and one PCG on K + sigma M.  J = sum_n w_n F . u_n (or its squared form)

P1 simplices only: the quadrilaterals of the reference's createRectangleMesh are split into triangles (fea/mesh.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .. import _lib
from .._lib import check
from ..engine import Vec, _ptr
from .forms import BackendForm, LinearFunctional
from .function import Function, FunctionSpace, LoadCaseSpace, TimeHistorySpace, VectorFunctionSpace
from .io import MeshTags

METHODS = {"SIMP": _lib.ELAST_SIMP, "RAMP": _lib.ELAST_RAMP}
MASS_LAWS = _lib.ELAST_MASS_LAWS          # "linear" (m = rho) | "du_olhoff" (C^1 cut-off below rho = 0.1)
PRECONDITIONERS = _lib.ELAST_PC           # "jacobi" (block diagonal) | "multilevel" (csrc/elast_pc.hip)


def _ctx():
    from .utils_hip import get_context
    return get_context()


def _n_values(who: str, what: str, values, n: int, noun: str = "load cases", scalar: bool = True, error=ValueError) -> np.ndarray:
    """``values`` as a float array of its own of length ``n``: one value per load case (column, mode), or with ``scalar`` one
    number for all of them."""
    a = np.array(values, dtype=np.float64).ravel()
    if scalar and a.size == 1 and np.ndim(values) == 0:
        a = np.full(n, float(a[0]))
    if a.size != n:
        raise error(f"{who}: {n} {noun} need as many {what}")
    return a


def _one_per_column(who: str, what: str, values, n_cols: int, noun: str = "columns") -> np.ndarray:
    """`_n_values` as the device calls want it: exactly one value per column (or mode), a FemoError otherwise."""
    return _n_values(who, what, values, n_cols, noun, scalar=False, error=_lib.FemoError)


def _f64(a: np.ndarray):
    return a.ctypes.data_as(_lib.c_f64p)


# ------------------------------------------------------------------------------------------------ device handles ----
class DeviceElasticity:
    """femo_elast: K(rho) as d x d blocks on the mesh's scalar pattern, its products, the traction load, dR/drho and PCG."""

    def __init__(self, ctx, mesh, E: float = 1.0, nu: float = 0.3):
        self.ctx, self.lib, self.mesh = ctx, ctx.lib, mesh
        self.dm = mesh.device(ctx)
        h = _lib.H()
        check(self.lib.femo_elast_create(self.dm.handle, float(E), float(nu), C.byref(h)))
        self.handle = h
        buf = (C.c_int64 * len(_lib.ELAST_INFO_KEYS))()
        check(self.lib.femo_elast_info(self.handle, buf))
        self.info = dict(zip(_lib.ELAST_INFO_KEYS, (int(v) for v in buf)))
        self.d, self.n_dof = self.info["dim"], self.info["n_dof"]
        self.fixed_key = None
        self.springs_key = None
        self.facets_key = None
        self.pc_plan = None                # set by pc_setup: dict(levels, bytes, nodes)
        self._rho = None

    def set_fixed(self, mask: Optional[np.ndarray]) -> None:
        if mask is None:
            check(self.lib.femo_elast_set_fixed(self.handle, None))
            self.fixed_key = None
            return
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.size == self.n_dof
        check(self.lib.femo_elast_set_fixed(self.handle, _ptr(m)))
        self.fixed_key = hash(m.tobytes())

    def set_springs(self, k: Optional[np.ndarray]) -> None:
        """Elastic supports: one stiffness >= 0 per dof (None or all zeros: none).  The operator is K(rho) + diag(k) from the
        next `assemble` on; until then products and solves are refused."""
        if k is None:
            check(self.lib.femo_elast_set_springs(self.handle, None))
            self.springs_key = None
        else:
            a = np.ascontiguousarray(k, dtype=np.float64).ravel()
            if a.size != self.n_dof:
                raise _lib.FemoError(f"set_springs: {self.n_dof} dofs need as many stiffnesses, got {a.size}")
            check(self.lib.femo_elast_set_springs(self.handle, _ptr(a)))
            self.springs_key = hash(a.tobytes()) if a.any() else None
        self._owner = None                 # whoever assembled last: K is gone

    def set_facets(self, facets: np.ndarray) -> None:
        f = np.ascontiguousarray(facets, dtype=np.int32).reshape(-1, self.d)
        key = hash(f.tobytes())
        if key != self.facets_key:
            check(self.lib.femo_elast_set_facets(self.handle, f.shape[0], _ptr(f)))
            self.facets_key = key

    def assemble(self, method: int, rho: Vec) -> None:
        check(self.lib.femo_elast_assemble(self.handle, int(method), rho.handle))
        self._rho = rho                    # the multilevel blocks are rebuilt from this vector on the next solve

    def apply(self, x: Vec, y: Vec, masked: bool = False, a: float = 1.0, b: float = 0.0, f: Optional[Vec] = None) -> Vec:
        """y = a K x + b f, or with A (identity rows / columns on the fixed dofs) when ``masked``."""
        check(self.lib.femo_elast_apply(self.handle, int(bool(masked)), float(a), x.handle, float(b),
                                        None if f is None else f.handle, y.handle))
        return y

    def load(self, t, out: Vec) -> Vec:
        tv = (C.c_double * 3)(*([float(v) for v in np.ravel(t)] + [0.0] * 3)[:3])
        check(self.lib.femo_elast_load(self.handle, tv, out.handle))
        return out

    def drho(self, method: int, transpose: bool, rho: Vec, u: Vec, x: Vec, y: Vec, accumulate: bool = False) -> Vec:
        check(self.lib.femo_elast_drho(self.handle, int(method), int(bool(transpose)), rho.handle, u.handle, x.handle,
                                       y.handle, int(bool(accumulate))))
        return y

    def pnorm_stress(self, rho: Vec, u: Vec, m: float, p: float, q: float, alpha: float, value: bool = True,
                     grad_u: Optional[Vec] = None, grad_rho: Optional[Vec] = None, accumulate: bool = False):
        """J = (1/alpha) sum_e |T_e| (m rho_e^q sigma_vm,e)^p (returned when ``value``), dJ/du into ``grad_u`` and dJ/drho
        into ``grad_rho`` (added onto them with ``accumulate``)."""
        val = C.c_double(0.0)
        check(self.lib.femo_elast_pnorm_stress(self.handle, rho.handle, u.handle, float(m), float(p), float(q), float(alpha),
                                               C.byref(val) if value else None, None if grad_u is None else grad_u.handle,
                                               None if grad_rho is None else grad_rho.handle, int(bool(accumulate))))
        return val.value if value else None

    def von_mises(self, u: Vec, out: Vec, rho: Optional[Vec] = None, q: float = 0.0) -> Vec:
        """out[n_cell] = rho_e^q sigma_vm,e; the solid stress (q = 0) needs no density."""
        check(self.lib.femo_elast_von_mises(self.handle, None if rho is None else rho.handle, u.handle, float(q), out.handle))
        return out

    def pc_setup(self, spacing_factor: float = 0.0) -> dict:
        """Lattice plan of the multilevel preconditioner (once per mesh); 0 selects the default spacing factor."""
        check(self.lib.femo_elast_pc_setup(self.handle, float(spacing_factor)))
        self.pc_plan = {k: v for k, v in self.pc_info().items() if k in ("levels", "bytes", "nodes")}
        return self.pc_plan

    def pc_info(self) -> dict:
        """levels, lattice bytes, block builds so far, device ms of the last block build, nodes per level."""
        buf = (C.c_int64 * _lib.ELAST_PC_INFO_COUNT)()
        check(self.lib.femo_elast_pc_info(self.handle, buf))
        nl = int(buf[0])
        return dict(levels=nl, bytes=int(buf[1]), builds=int(buf[2]), build_ms=int(buf[3]) * 1e-3,
                    nodes=[int(buf[4 + l]) for l in range(nl)])

    def pc_level(self, level: int) -> np.ndarray:
        """(nodes, d, d): the Galerkin blocks blockdiag(P_l^T A P_l) of lattice ``level``, before inversion."""
        nodes = self.pc_info()["nodes"][level]
        out = np.zeros((nodes, self.d, self.d))
        check(self.lib.femo_elast_pc_export_level(self.handle, int(level), _ptr(out)))
        return out

    def pc_apply(self, r: Vec, z: Vec) -> Vec:
        """z = M^-1 r with the multilevel preconditioner."""
        check(self.lib.femo_elast_pc_apply(self.handle, r.handle, z.handle))
        return z

    @staticmethod
    def _solver_opts(rtol, atol, max_it, check_every, zero_guess, pc) -> _lib.SolverOpts:
        if pc not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {pc!r} (jacobi or multilevel)")
        if check_every is None:
            check_every = 64 if pc == "jacobi" else 0
        return _lib.SolverOpts(rtol=float(rtol), atol=float(atol), max_it=int(max_it), zero_guess=int(bool(zero_guess)),
                               check_every=int(check_every), pc=PRECONDITIONERS[pc], atol_pc=0.0)

    def solve(self, b: Vec, x: Vec, rtol: float = 1e-15, atol: float = 0.0, max_it: int = 1_000_000,
              check_every: Optional[int] = None, zero_guess: bool = True, pc: str = "jacobi") -> _lib.SolveInfo:
        """PCG; ``pc`` = "jacobi" or "multilevel" (needs `pc_setup`).  Polls every 64 iterations with Jacobi, and every 8
        (the library's default) with the multilevel preconditioner, unless ``check_every`` says otherwise."""
        opts = self._solver_opts(rtol, atol, max_it, check_every, zero_guess, pc)
        info = _lib.SolveInfo()
        check(self.lib.femo_elast_solve(self.handle, b.handle, x.handle, C.byref(opts), C.byref(info)))
        return info

    # ---- several load cases in one vector: column l at l * n_dof (csrc/elast_solve.hip) ----
    def _cols(self, n_cols: int, *vecs: Vec, what: str = "load cases") -> int:
        """``n_cols`` as an int, once every vector given holds that many columns (``what``: what the error calls them)."""
        n_cols = int(n_cols)
        for v in vecs:
            if v is not None and v.n < n_cols * self.n_dof:
                raise _lib.FemoError(f"{n_cols} {what} need vectors of {n_cols * self.n_dof} entries, got {v.n}")
        return n_cols

    def apply_multi(self, n_cols: int, x: Vec, y: Vec, masked: bool = False, a: float = 1.0, b: float = 0.0,
                    f: Optional[Vec] = None) -> Vec:
        """y_l = a K x_l + b f_l (or with the masked A) for all ``n_cols`` columns in one launch."""
        check(self.lib.femo_elast_apply_multi(self.handle, int(bool(masked)), self._cols(n_cols, x, y, f), float(a), x.handle,
                                              float(b), None if f is None else f.handle, y.handle))
        return y

    def solve_multi(self, n_cols: int, b: Vec, x: Vec, rtol: float = 1e-15, atol: float = 0.0, max_it: int = 1_000_000,
                    check_every: Optional[int] = None, zero_guess: bool = True, pc: str = "jacobi") -> list:
        """`solve` for ``n_cols`` right-hand sides in one batched PCG; one `SolveInfo` per column (``solve_ms`` is that of the
        whole batched solve in each).  A column that has converged is frozen while the others go on."""
        opts = self._solver_opts(rtol, atol, max_it, check_every, zero_guess, pc)
        info = (_lib.SolveInfo * _lib.ELAST_MAX_COLS)()
        check(self.lib.femo_elast_solve_multi(self.handle, self._cols(n_cols, b, x), b.handle, x.handle, C.byref(opts), info))
        return [info[l] for l in range(int(n_cols))]

    def drho_multi(self, method: int, transpose: bool, n_cols: int, rho: Vec, u: Vec, x: Vec, y: Vec,
                   accumulate: bool = False) -> Vec:
        """transpose: y[n_cell] (+)= sum_l C'(rho) x_l^T K0 u_l; otherwise column l of y (+)= the forward product with u_l."""
        n_cols = self._cols(n_cols, u, x if transpose else y)
        check(self.lib.femo_elast_drho_multi(self.handle, int(method), int(bool(transpose)), n_cols, rho.handle, u.handle,
                                             x.handle, y.handle, int(bool(accumulate))))
        return y

    def body_apply(self, n_cols: int, b, x: Vec, y: Vec, transpose: bool = False, a: float = 1.0, base: Optional[Vec] = None,
                   zero_fixed: bool = False, accumulate: bool = False) -> Vec:
        """The body-load operator G_B of the ``n_cols`` body forces ``b`` (n_cols x d) in one launch (csrc/elast_body.hip):
        column l of y = [y if ``accumulate``, else ``base`` or 0] + a b_l sum_{c around v} x_c |T_c| / (d + 1) from the cell
        vector x, with 0 on the dofs of the fixed set when ``zero_fixed``; ``transpose``: y[n_cell] (+)= a G_B^T x from the
        n_cols columns of x."""
        bv = np.asarray(b, dtype=np.float64).reshape(-1, self.d) if np.size(b) else np.zeros((0, self.d))
        n_cols = self._cols(n_cols, x if transpose else y, base)
        if bv.shape[0] != n_cols:
            raise _lib.FemoError(f"body_apply: {n_cols} columns need as many body forces")
        b3 = np.zeros((max(n_cols, 1), 3))
        b3[:n_cols, :self.d] = bv
        check(self.lib.femo_elast_body_apply(self.handle, n_cols, b3.ctypes.data_as(_lib.c_f64p), int(bool(transpose)),
                                             float(a), x.handle, None if base is None else base.handle,
                                             int(bool(zero_fixed)), y.handle, int(bool(accumulate))))
        return y

    def thermal_apply(self, method: int, product: str, n_cols: int, scales, alpha: float, rho: Vec, temperature, y: Vec,
                      T_ref: float = 0.0, x: Optional[Vec] = None, a: float = 1.0, base: Optional[Vec] = None,
                      zero_fixed: bool = False, accumulate: bool = False) -> Vec:
        """The thermal-expansion operator H(w; theta)[d v + i] = sum_{c around v} w_c beta_0 thetabar_c |T_c| d_i phi_v^c in one
        launch for ``n_cols`` columns with the scales ``scales`` (csrc/elast_thermal.hip); beta_0 = (3 lambda_0 + 2 mu_0)
        ``alpha``, theta = ``temperature`` - ``T_ref`` with the temperature a Vec of nodal values or a number (uniform).
        ``product`` "N": column l of y = [y if ``accumulate``, else ``base`` or 0] + a s_l H(w; theta), w = C(rho), or
        C'(rho) x with the cell vector ``x``; 0 on the dofs of the fixed set when ``zero_fixed``.  "T_rho": y[n_cell] (+)= a
        C'(rho_c) beta_0 thetabar_c |T_c| sum_l s_l div(x_l)_c and "T_temp": y[n_vert] (+)= a sum_{c around v} C(rho_c) beta_0
        |T_c| / (d + 1) sum_l s_l div(x_l)_c from the n_cols columns of ``x``: the transposes in w and in theta."""
        if product not in _lib.ELAST_THERMAL_PRODUCTS:
            raise _lib.FemoError(f"thermal_apply: unknown product {product!r} (N, T_rho or T_temp)")
        fwd = product == "N"
        n_cols = self._cols(n_cols, y if fwd else x, base)
        s = np.ascontiguousarray(scales, dtype=np.float64).ravel()
        if s.size != n_cols:
            raise _lib.FemoError(f"thermal_apply: {n_cols} columns need as many scales")
        s8 = np.zeros(max(n_cols, 1))
        s8[:n_cols] = s
        uniform = not isinstance(temperature, Vec)
        check(self.lib.femo_elast_thermal_apply(self.handle, int(method), _lib.ELAST_THERMAL_PRODUCTS[product], n_cols,
                                                s8.ctypes.data_as(_lib.c_f64p), float(alpha), rho.handle,
                                                None if uniform else temperature.handle, float(temperature) if uniform else 0.0,
                                                float(T_ref), float(a), None if x is None else x.handle,
                                                None if base is None else base.handle, int(bool(zero_fixed)), y.handle,
                                                int(bool(accumulate))))
        return y

    # ---- eigenfrequencies: K phi = lambda M(rho) phi on the free dofs (csrc/elast_eig.hip, csrc/elast_block.hip) ----
    @staticmethod
    def _mass_law(mass_law: str) -> int:
        if mass_law not in MASS_LAWS:
            raise _lib.FemoError(f"unknown mass law {mass_law!r} (linear or du_olhoff)")
        return MASS_LAWS[mass_law]

    def mass_apply_multi(self, n_cols: int, rho: Vec, x: Vec, y: Vec, masked: bool = False, a: float = 1.0,
                         density: float = 1.0, mass_law: str = "linear") -> Vec:
        """y_l = a M(rho) x_l with the consistent P1 mass M = density sum_e m(rho_e) M0_e, matrix free, for all ``n_cols``
        columns in one launch; ``masked``: M_ff (fixed entries of x read as 0, exact zeros on the fixed dofs of y)."""
        check(self.lib.femo_elast_mass_apply_multi(self.handle, self._mass_law(mass_law), float(density), int(bool(masked)),
                                                   self._cols(n_cols, x, y), float(a), rho.handle, x.handle, y.handle))
        return y

    def block_gram(self, n_a: int, a: Vec, n_b: int, b: Vec) -> np.ndarray:
        """(n_a, n_b): G[i, j] = a_i . b_j, all pairs in one pass."""
        n_a, n_b = self._cols(n_a, a), self._cols(n_b, b)
        G = np.zeros(max(n_a, 1) * max(n_b, 1))
        check(self.lib.femo_elast_block_gram(self.handle, n_a, a.handle, n_b, b.handle, G.ctypes.data_as(_lib.c_f64p)))
        return G.reshape(n_a, n_b)

    def block_rotate(self, n_cols: int, Q, x: Vec, y: Vec) -> Vec:
        """y_j = sum_i x_i Q[i, j] for the ``n_cols`` columns; ``y`` may be ``x``."""
        n_cols = self._cols(n_cols, x, y)
        Qa = np.ascontiguousarray(Q, dtype=np.float64)
        if Qa.shape != (n_cols, n_cols):
            raise _lib.FemoError(f"block_rotate: {n_cols} columns need a {n_cols} x {n_cols} matrix")
        check(self.lib.femo_elast_block_rotate(self.handle, n_cols, Qa.ctypes.data_as(_lib.c_f64p), x.handle, y.handle))
        return y

    def eig_drho(self, method: int, n_modes: int, rho: Vec, phi: Vec, lam, c, y: Vec, density: float = 1.0,
                 mass_law: str = "linear", accumulate: bool = False) -> Vec:
        """y[n_cell] (+)= sum_k c_k [C'(rho) phi_k^T K0 phi_k - lam_k density m'(rho) phi_k^T M0 phi_k] in one launch: with
        M-orthonormal modes the bracket is d lambda_k / d rho."""
        n_modes = self._cols(n_modes, phi)
        lv, cv = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (lam, c))
        if lv.size != n_modes or cv.size != n_modes:
            raise _lib.FemoError(f"eig_drho: {n_modes} modes need as many eigenvalues and weights")
        check(self.lib.femo_elast_eig_drho(self.handle, int(method), self._mass_law(mass_law), float(density), n_modes,
                                           rho.handle, phi.handle, _f64(lv), _f64(cv), y.handle, int(bool(accumulate))))
        return y

    def eigs(self, n_modes: int, rho: Vec, X: Vec, block: Optional[int] = None, density: float = 1.0,
             mass_law: str = "linear", rtol: float = 1e-9, max_outer: int = 200, pcg_rtol: float = 1e-12,
             pcg_max_it: int = 0, pc: str = "jacobi"):
        """The ``n_modes`` lowest eigenpairs of the assembled K and M(rho) on the free dofs by block inverse iteration with
        Rayleigh-Ritz; every inner solve is one batched PCG over the ``block`` columns of ``X`` (the start block on entry,
        the M-orthonormal modes on return; the last block - n_modes columns are guard vectors).  Returns (lambda[block]
        ascending, info) with info = dict(outer_iterations, pcg_iterations, converged, residual, solve_ms)."""
        block = min(_lib.ELAST_MAX_COLS, int(n_modes) + 2) if block is None else block
        return self._block_solve(lambda *tail: self.lib.femo_elast_eigs(self.handle, self._mass_law(mass_law), float(density),
                                                                        rho.handle, *tail),
                                 n_modes, block, X, rtol, max_outer, pcg_rtol, pcg_max_it, pc)

    def _block_solve(self, call, n_modes: int, block: int, X: Vec, rtol: float, max_outer: int, pcg_rtol: float,
                     pcg_max_it: int, pc: str):
        """The marshalling of `eigs` and `buckle`: ``call(n_modes, block, X, opts, lambda, info)`` is the library's entry point
        behind its leading arguments.  Returns (lambda[block], info)."""
        if pc not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {pc!r} (jacobi or multilevel)")
        block = self._cols(int(block), X)
        opts = _lib.EigOpts(rtol=float(rtol), pcg_rtol=float(pcg_rtol), max_outer=int(max_outer), pcg_max_it=int(pcg_max_it),
                            pc=PRECONDITIONERS[pc], reserved=0)
        info = _lib.EigInfo()
        lam = np.zeros(_lib.ELAST_MAX_COLS)
        check(call(int(n_modes), block, X.handle, C.byref(opts), lam.ctypes.data_as(_lib.c_f64p), C.byref(info)))
        return lam[:block].copy(), dict(outer_iterations=info.outer_iterations, pcg_iterations=info.pcg_iterations,
                                        converged=info.converged, residual=np.array(info.residual[:block]),
                                        solve_ms=info.solve_ms, preconditioner=pc)

    # ---- buckling: (K + lambda K_G(u, rho)) phi = 0 on the free dofs (csrc/elast_buckle.hip) ----
    def geom_stress(self, method: int, rho: Vec, u: Vec, out: Optional[Vec] = None) -> Optional[Vec]:
        """Fills the handle's cell stress C(rho_e) sigma_0(u_e), which `geom_apply_multi` reads; with ``out`` a copy of it:
        d (d+1) / 2 components of n_cell entries, component-major (the diagonal first, then 01[, 02, 12])."""
        check(self.lib.femo_elast_geom_stress(self.handle, int(method), rho.handle, u.handle))
        if out is not None:
            check(self.lib.femo_elast_geom_stress_get(self.handle, out.handle))
        return out

    def geom_apply_multi(self, n_cols: int, x: Vec, y: Vec, masked: bool = False, a: float = 1.0) -> Vec:
        """y_l = a K_G x_l with the geometric stiffness of the last `geom_stress`, matrix free, for all ``n_cols`` columns in one
        launch; ``masked``: (K_G)_ff (fixed entries of x read as 0, exact zeros on the fixed dofs of y)."""
        check(self.lib.femo_elast_geom_apply_multi(self.handle, int(bool(masked)), self._cols(n_cols, x, y), float(a), x.handle,
                                                   y.handle))
        return y

    def buckle_du(self, method: int, n_modes: int, rho: Vec, phi: Vec, w, out: Vec) -> Vec:
        """out[(v, j)] = sum_{e around v} C(rho_e) |T_e| (Sigma_H g_v)_j with Sigma_H = lam0 tr(H) I + 2 mu0 H and
        H = sum_k w_k (grad phi_k)^T (grad phi_k), in one launch: with K-orthonormal modes and w_k = lambda_k^2 it is
        d lambda_k / du."""
        n_modes = self._cols(n_modes, phi)
        wv = _one_per_column("buckle_du", "weights", w, n_modes, "modes")
        check(self.lib.femo_elast_buckle_du(self.handle, int(method), n_modes, rho.handle, phi.handle, _f64(wv), out.handle))
        return out

    def buckle_drho(self, method: int, n_modes: int, rho: Vec, u: Vec, phi: Vec, w1, w2, y: Vec,
                    accumulate: bool = False) -> Vec:
        """y[n_cell] (+)= C'(rho_e) |T_e| sum_k [w1_k (lam0 (div phi_k)^2 + 2 mu0 eps(phi_k) : eps(phi_k)) + w2_k sigma_0(u_e) :
        H_e(phi_k)] in one launch: with K-orthonormal modes, w1_k = lambda_k and w2_k = lambda_k^2 it is d lambda_k / d rho at
        fixed u."""
        n_modes = self._cols(n_modes, phi)
        w1v, w2v = (_one_per_column("buckle_drho", "weights", w, n_modes, "modes") for w in (w1, w2))
        check(self.lib.femo_elast_buckle_drho(self.handle, int(method), n_modes, rho.handle, u.handle, phi.handle, _f64(w1v),
                                              _f64(w2v), y.handle, int(bool(accumulate))))
        return y

    def buckle(self, n_modes: int, rho: Vec, u: Vec, X: Vec, block: Optional[int] = None, method: int = _lib.ELAST_SIMP,
               rtol: float = 1e-9, max_outer: int = 400, pcg_rtol: float = 1e-12, pcg_max_it: int = 0, pc: str = "jacobi"):
        """The ``n_modes`` smallest positive load factors of (K + lambda K_G(u, rho)) phi = 0 on the free dofs, with the
        assembled K of the handle: the block iteration of `eigs` on (-K_G) phi = mu K phi for the largest positive
        mu = 1 / lambda, every inner solve one batched PCG over the ``block`` columns of ``X`` from a zero first guess (the
        start block on entry, the K-orthonormal modes in descending mu on return; the last block - n_modes columns are guard
        vectors).  The block converges to the largest |mu| of either sign: when it fills up with negative mu (buckling under
        the reversed load) before ``n_modes`` positive ones are found, the call fails -- raise ``block``.  Returns
        (lambda[block] = 1 / mu, info) with info as that of `eigs`; ``residual`` is |(-K_G) x - mu K x| / (mu |K x|)."""
        block = _lib.ELAST_MAX_COLS if block is None else block
        return self._block_solve(lambda *tail: self.lib.femo_elast_buckle(self.handle, int(method), rho.handle, u.handle, *tail),
                                 n_modes, block, X, rtol, max_outer, pcg_rtol, pcg_max_it, pc)

    # ---- harmonic response: (K - sigma_l M(rho)) u_l = F_l, sigma_l = omega_l^2 (csrc/elast_harm.hip) ----
    def mass_assemble(self, rho: Vec, density: float = 1.0, mass_law: str = "linear") -> None:
        """M(rho) = density sum_e m(rho_e) M0_e as a scalar matrix on the pattern of K (one double per entry, one per row);
        `dyn_apply_multi` and `dyn_solve_multi` read it."""
        check(self.lib.femo_elast_mass_assemble(self.handle, self._mass_law(mass_law), float(density), rho.handle))

    def dyn_apply_multi(self, n_cols: int, shifts, x: Vec, y: Vec, masked: bool = False, a: float = 1.0, b: float = 0.0,
                        f: Optional[Vec] = None) -> Vec:
        """y_l = a (K - shifts[l] M) x_l + b f_l with the assembled K and M in one pass over the pattern (or with identity rows
        and columns on the fixed dofs when ``masked``); shifts[l] = 0 gives the bits of `apply_multi`."""
        n_cols = self._cols(n_cols, x, y, f)
        sv = _one_per_column("dyn_apply_multi", "shifts", shifts, n_cols)
        check(self.lib.femo_elast_dyn_apply_multi(self.handle, int(bool(masked)), n_cols, _f64(sv), float(a), x.handle,
                                                  float(b), None if f is None else f.handle, y.handle))
        return y

    def dyn_solve_multi(self, n_cols: int, shifts, b: Vec, x: Vec, rtol: float = 1e-12, atol: float = 0.0,
                        max_it: int = 1_000_000, check_every: Optional[int] = None, zero_guess: bool = True,
                        pc: str = "jacobi") -> list:
        """(K - shifts[l] M) x_l = b_l for ``n_cols`` right-hand sides in one batched MINRES with the preconditioner of
        `solve_multi` (built from the unshifted K); one `SolveInfo` per column: ``converged`` 1, 0 (max_it) or -1 (a
        non-finite value), ``residual_norm`` the recurrence's estimate of sqrt(r . M^-1 r), ``rhs_norm`` that of the first
        residual.  A finished column is frozen while the others go on."""
        opts = self._solver_opts(rtol, atol, max_it, check_every, zero_guess, pc)
        n_cols = self._cols(n_cols, b, x)
        sv = _one_per_column("dyn_solve_multi", "shifts", shifts, n_cols)
        info = (_lib.SolveInfo * _lib.ELAST_MAX_COLS)()
        check(self.lib.femo_elast_dyn_solve_multi(self.handle, n_cols, _f64(sv), b.handle, x.handle, C.byref(opts), info))
        return [info[l] for l in range(n_cols)]

    # ---- damped harmonic response: Z_l = (K - sigma_l M) + i (ck_l K + cm_l M); complex column l = real columns 2 l, 2 l + 1
    # (csrc/elast_damp.hip) ----
    def _damping(self, who: str, n_cols: int, shifts, ck, cm, *vecs: Vec):
        n_cols = int(n_cols)
        if not 1 <= n_cols <= _lib.ELAST_MAX_COLS // 2:
            raise _lib.FemoError(f"{who}: {n_cols} complex columns (1 to {_lib.ELAST_MAX_COLS // 2})")
        self._cols(2 * n_cols, *vecs)
        arrays = [_one_per_column(who, what, v, n_cols) for what, v in (("shifts", shifts), ("ck", ck), ("cm", cm))]
        return n_cols, [_f64(a) for a in arrays], arrays

    def cdyn_apply_multi(self, n_cols: int, shifts, ck, cm, x: Vec, y: Vec, masked: bool = False, conj: bool = False,
                         a: float = 1.0, b: float = 0.0, f: Optional[Vec] = None) -> Vec:
        """y_l = a Z_l x_l + b f_l with Z_l = (K - shifts[l] M) + i (ck[l] K + cm[l] M) (conj(Z_l) with ``conj``) for ``n_cols``
        complex columns, Re in real column 2 l and Im in 2 l + 1, in one pass over the pattern; ck = cm = 0 gives the bits of
        `dyn_apply_multi` on both parts."""
        n_cols, ptrs, _keep = self._damping("cdyn_apply_multi", n_cols, shifts, ck, cm, x, y, f)
        check(self.lib.femo_elast_cdyn_apply_multi(self.handle, int(bool(masked)), int(bool(conj)), n_cols, *ptrs, float(a),
                                                   x.handle, float(b), None if f is None else f.handle, y.handle))
        return y

    def cdyn_solve_multi(self, n_cols: int, shifts, ck, cm, b: Vec, x: Vec, conj: bool = False, rtol: float = 1e-12,
                         atol: float = 0.0, max_it: int = 1_000_000, check_every: Optional[int] = None, zero_guess: bool = True,
                         pc: str = "jacobi") -> list:
        """Z_l x_l = b_l (conj(Z_l) with ``conj``) for ``n_cols`` complex right-hand sides in one batched preconditioned COCR
        with the preconditioner of `solve_multi` on both parts; one `SolveInfo` per complex column: ``converged`` 1, 0
        (max_it) or -1 (a non-finite value or a zero denominator), ``residual_norm`` = sqrt(Re(r^H M^-1 r)), ``rhs_norm`` that
        of the first residual.  A finished column is frozen while the others go on."""
        opts = self._solver_opts(rtol, atol, max_it, check_every, zero_guess, pc)
        n_cols, ptrs, _keep = self._damping("cdyn_solve_multi", n_cols, shifts, ck, cm, b, x)
        info = (_lib.SolveInfo * _lib.ELAST_MAX_COLS)()
        check(self.lib.femo_elast_cdyn_solve_multi(self.handle, int(bool(conj)), n_cols, *ptrs, b.handle, x.handle,
                                                   C.byref(opts), info))
        return [info[l] for l in range(n_cols)]

    def mass_drho_multi(self, transpose: bool, n_cols: int, scales, rho: Vec, u: Vec, x: Vec, y: Vec, density: float = 1.0,
                        mass_law: str = "linear", accumulate: bool = False) -> Vec:
        """transpose: y[n_cell] (+)= sum_l scales[l] density m'(rho) x_l^T M0 u_l; otherwise column l of y (+)= scales[l] times
        the forward product of the cell vector x with u_l.  With scales = -shifts and ``accumulate`` on top of `drho_multi` it
        is dR/drho of the harmonic residual."""
        n_cols = self._cols(n_cols, u, x if transpose else y)
        sv = _one_per_column("mass_drho_multi", "scales", scales, n_cols)
        check(self.lib.femo_elast_mass_drho_multi(self.handle, self._mass_law(mass_law), float(density), int(bool(transpose)),
                                                  n_cols, _f64(sv), rho.handle, u.handle, x.handle, y.handle,
                                                  int(bool(accumulate))))
        return y

    # ---- transient response: Newmark march on a history of n_steps columns, column t = u_{t+1} (csrc/elast_transient.hip) ----
    @staticmethod
    def _newmark(params) -> _lib.NewmarkParams:
        dt, beta, gamma, c_m, c_k = (float(v) for v in params)
        return _lib.NewmarkParams(dt=dt, beta=beta, gamma=gamma, c_m=c_m, c_k=c_k)

    def newmark_rhs(self, u: Vec, y: Vec, m0: float, k0: float, mm: float, km: float, rhs: Optional[Vec] = None,
                    cr: float = 1.0, crf: float = 1.0, masked: bool = False) -> Vec:
        """y = cr rhs - (m0 M + k0 K) u_n - (mm M + km K) u_{n-1} in one pass over the pattern; ``u`` holds u_n then u_{n-1}.
        ``masked``: fixed entries of u read as 0, a fixed row gives crf rhs."""
        check(self.lib.femo_elast_newmark_rhs(self.handle, int(bool(masked)), float(cr), float(crf), float(m0), float(k0),
                                              float(mm), float(km), None if rhs is None else rhs.handle, u.handle, y.handle))
        return y

    def newmark_march(self, params, n_steps: int, U: Vec, rhs: Optional[Vec] = None, F: Optional[Vec] = None, signal=None,
                      reverse: bool = False, extrapolate: bool = True, rtol: float = 1e-13, atol: float = 0.0,
                      max_it: int = 1_000_000, check_every: Optional[int] = None, pc: str = "jacobi"):
        """All ``n_steps`` steps of L U = B (L^T U = B with ``reverse``) in one call: B is the history ``rhs`` or comes from the
        load pattern ``F`` and the n_steps + 1 samples ``signal``.  ``params`` = (dt, beta, gamma, c_m, c_k).  Returns (one
        `SolveInfo` per step, the column the march stopped at or -1)."""
        n_steps = self._cols(n_steps, U, rhs, what="steps")
        opts = self._solver_opts(rtol, atol, max_it, check_every, False, pc)
        g = None
        if signal is not None:
            g = np.ascontiguousarray(signal, dtype=np.float64).ravel()
            if g.size != n_steps + 1:
                raise _lib.FemoError(f"newmark_march: {n_steps} steps need {n_steps + 1} samples of the signal, got {g.size}")
        info = (_lib.SolveInfo * n_steps)()
        stopped = C.c_int32(-1)
        par = self._newmark(params)
        check(self.lib.femo_elast_newmark_march(self.handle, C.byref(par), n_steps, int(bool(reverse)),
                                                None if rhs is None else rhs.handle, None if F is None else F.handle,
                                                None if g is None else g.ctypes.data_as(_lib.c_f64p), U.handle, C.byref(opts),
                                                int(bool(extrapolate)), info, C.byref(stopped)))
        return [info[t] for t in range(n_steps)], int(stopped.value)

    def newmark_apply(self, params, n_steps: int, X: Vec, Y: Vec, transpose: bool = False, masked: bool = False) -> Vec:
        """Y = L X, or L^T X, for a history; FEMO_ELAST_MAX_COLS time steps per launch."""
        par = self._newmark(params)
        check(self.lib.femo_elast_newmark_apply(self.handle, C.byref(par), self._cols(n_steps, X, Y, what="steps"),
                                                int(bool(transpose)), int(bool(masked)), X.handle, Y.handle))
        return Y

    def newmark_drho(self, params, method: int, transpose: bool, n_steps: int, rho: Vec, U: Vec, x: Vec, y: Vec,
                     density: float = 1.0, mass_law: str = "linear", accumulate: bool = False, first: int = 0,
                     count: Optional[int] = None) -> Vec:
        """dR/drho of the march's residual for the columns first ... first + count - 1 (all by default).  transpose:
        y[n_cell] (+)= sum_t (dR_t/drho)^T x_t; otherwise column t of y (+)= dR_t/drho x.  Windows of FEMO_ELAST_MAX_COLS columns
        in ascending order."""
        n_steps = self._cols(n_steps, U, x if transpose else y, what="steps")
        par = self._newmark(params)
        check(self.lib.femo_elast_newmark_drho(self.handle, C.byref(par), int(method), self._mass_law(mass_law), float(density),
                                               int(bool(transpose)), n_steps, int(first),
                                               n_steps - int(first) if count is None else int(count), rho.handle, U.handle,
                                               x.handle, y.handle, int(bool(accumulate))))
        return y

    def newmark_dots(self, n_steps: int, f: Vec, U: Vec) -> np.ndarray:
        """(n_steps,): f . U_t for every column, through the Gram kernel in windows."""
        out = np.zeros(self._cols(n_steps, U, what="steps"))
        check(self.lib.femo_elast_newmark_dots(self.handle, int(n_steps), f.handle, U.handle, _f64(out)))
        return out

    def newmark_outer(self, n_steps: int, a, f: Vec, Y: Vec) -> Vec:
        """Y_t = a[t] f for every column."""
        av = _one_per_column("newmark_outer", "coefficients", a, self._cols(n_steps, Y, what="steps"))
        check(self.lib.femo_elast_newmark_outer(self.handle, int(n_steps), _f64(av), f.handle, Y.handle))
        return Y

    def pnorm_stress_multi(self, n_cols: int, rho: Vec, u: Vec, m, p: float, q: float, alpha: float, weights=None,
                           value: bool = True, grad_u: Optional[Vec] = None, grad_rho: Optional[Vec] = None,
                           accumulate: bool = False):
        """J_l = (1/alpha) sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p for every column (the array of the ``n_cols`` unweighted
        values is returned when ``value``), column l of ``grad_u`` (+)= w_l dJ_l/du_l, ``grad_rho`` (+)= sum_l w_l dJ_l/drho.
        ``m``: a scalar or one scale per column; ``weights``: one per column, 1 without."""
        n_cols = self._cols(n_cols, u, grad_u)
        mv, wv, vals = self._scales_and_weights("pnorm_stress_multi", n_cols, m, weights)
        check(self.lib.femo_elast_pnorm_stress_multi(self.handle, n_cols, rho.handle, u.handle, _f64(mv),
                                                     None if wv is None else _f64(wv), float(p), float(q), float(alpha),
                                                     _f64(vals) if value else None, None if grad_u is None else grad_u.handle,
                                                     None if grad_rho is None else grad_rho.handle, int(bool(accumulate))))
        return vals[:n_cols] if value else None

    @staticmethod
    def _scales_and_weights(who: str, n_cols: int, m, weights):
        """The scales ``m`` (a scalar or one per column) and the weights (one per column, or None) of an aggregate as arrays,
        and the array its ``n_cols`` values are written to."""
        mv = np.ascontiguousarray(m, dtype=np.float64).ravel()
        if np.ndim(m) == 0:
            mv = np.full(max(n_cols, 0), float(m))
        wv = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ravel()
        if mv.size != n_cols or (wv is not None and wv.size != n_cols):
            raise _lib.FemoError(f"{who}: {n_cols} columns need as many scales and weights")
        return mv, wv, np.zeros(max(n_cols, 1))

    def pnorm_disp_multi(self, n_cols: int, u: Vec, a: Vec, m, p: float, alpha: float = 0.0, weights=None, value: bool = True,
                         grad_u: Optional[Vec] = None, accumulate: bool = False):
        """J_l = (1/alpha) sum_v a_v (m_l |u_{l,v}|)^p with the nodal weights ``a`` (n_vert, >= 0) for every column (the array
        of the ``n_cols`` unweighted values is returned when ``value``), column l of ``grad_u`` (+)= w_l dJ_l/du_l.
        ``alpha`` <= 0: sum_v a_v.  ``m``: a scalar or one scale per column; ``weights``: one per column, 1 without."""
        n_cols = self._cols(n_cols, u, grad_u)
        mv, wv, vals = self._scales_and_weights("pnorm_disp_multi", n_cols, m, weights)
        check(self.lib.femo_elast_pnorm_disp_multi(self.handle, n_cols, u.handle, a.handle, _f64(mv),
                                                   None if wv is None else _f64(wv), float(p), float(alpha),
                                                   _f64(vals) if value else None, None if grad_u is None else grad_u.handle,
                                                   int(bool(accumulate))))
        return vals[:n_cols] if value else None

    def von_mises_multi(self, n_cols: int, u: Vec, out: Vec, rho: Optional[Vec] = None, q: float = 0.0, scales=None,
                        column: Optional[int] = None) -> Vec:
        """out[n_cell] = max_l s_l rho_e^q sigma_vm,e(u_l), or s_column rho_e^q sigma_vm,e(u_column) with ``column``."""
        n_cols = self._cols(n_cols, u)
        sv = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64).ravel()
        if sv is not None and sv.size != n_cols:
            raise _lib.FemoError(f"von_mises_multi: {n_cols} columns need as many scales")
        check(self.lib.femo_elast_von_mises_multi(self.handle, n_cols, None if rho is None else rho.handle, u.handle,
                                                  None if sv is None else _f64(sv), float(q),
                                                  -1 if column is None else int(column), out.handle))
        return out

    def export_csr(self):
        """K as a SciPy CSR matrix of size n_dof (host copy; tests and debugging)."""
        import scipy.sparse as sp
        nr, nnz, d = self.mesh.n_vert, self.info["nnz"], self.d
        rowptr = np.zeros(nr + 1, np.int64)
        col = np.zeros(nnz, np.int32)
        val = np.zeros(nnz * d * d)
        check(self.lib.femo_elast_export_csr(self.handle, _ptr(rowptr), _ptr(col), _ptr(val)))
        return sp.bsr_matrix((val.reshape(nnz, d, d), col, rowptr), shape=(nr * d, nr * d)).tocsr()

    def bench_spmv(self, x: Vec, y: Vec, reps: int = 20) -> float:
        ms = C.c_double(0.0)
        check(self.lib.femo_elast_bench_spmv(self.handle, x.handle, y.handle, int(reps), C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None) and getattr(self.dm, "handle", None):
                self.lib.femo_elast_destroy(h)
        except Exception:
            pass


def elasticity_handle(mesh, E: float = 1.0, nu: float = 0.3) -> DeviceElasticity:
    """One handle per (mesh, context, E, nu)."""
    ctx = _ctx()
    cache = mesh.__dict__.setdefault("_elast", {})
    key = (id(ctx), float(E), float(nu))
    h = cache.get(key)
    if h is None or h.ctx is not ctx:
        h = cache[key] = DeviceElasticity(ctx, mesh, E, nu)
    return h


class DeviceFilter:
    """femo_filter: W_ij = (r - d_ij) / sum_k (r - d_ik) over d_ij <= r, and W^T, built on the device
    (GeneralFilterOperation.compute_weight_mat, pre_processor/general_filter_model.py)."""

    def __init__(self, ctx, coordinates: np.ndarray, radius: float):
        self.ctx, self.lib = ctx, ctx.lib
        x = np.ascontiguousarray(coordinates, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] not in (2, 3):
            raise ValueError("filter coordinates must be an (n, 2) or (n, 3) array")
        self.n, self.dim, self.radius = x.shape[0], x.shape[1], float(radius)
        h = _lib.H()
        check(self.lib.femo_filter_create(ctx.handle, self.dim, self.n, _ptr(x), self.radius, C.byref(h)))
        self.handle = h
        nnz = C.c_int64(0)
        check(self.lib.femo_filter_nnz(self.handle, C.byref(nnz)))
        self.nnz = int(nnz.value)

    def apply(self, x: Vec, y: Vec, transpose: bool = False) -> Vec:
        check(self.lib.femo_filter_apply(self.handle, int(bool(transpose)), x.handle, y.handle))
        return y

    def export_csr(self, transpose: bool = False):
        """(rowptr, col, val) of W (or W^T), rows sorted by column."""
        rowptr = np.zeros(self.n + 1, np.int64)
        col = np.zeros(self.nnz, np.int32)
        val = np.zeros(self.nnz)
        check(self.lib.femo_filter_export_csr(self.handle, int(bool(transpose)), _ptr(rowptr), _ptr(col), _ptr(val)))
        return rowptr, col, val

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None):
                self.lib.femo_filter_destroy(h)
        except Exception:
            pass


class DevicePdeFilter:
    """femo_pde_filter (csrc/pde_filter.hip): the Helmholtz filter W = V^-1 T^T A^-1 T, A = rt^2 L + M, rt = r / (2 sqrt 3), on
    ``mesh`` (a fea mesh); ``mass`` is ``"lumped"`` (default: no undershoot on meshes without obtuse cells) or
    ``"consistent"``.  One scalar operator on the mesh pattern whatever the radius; ``apply`` is one Jacobi-PCG solve to
    ``rtol`` from the zero guess -- with ``warm_start`` from the nodal field of the last forward application.  ``last_info`` is
    the solve record of the last application (iterations, converged, residual_norm, rhs_norm, solve_ms, ...)."""

    MASS = {"lumped": 1, "consistent": 0}

    def __init__(self, ctx, mesh, radius: float, mass: str = "lumped", rtol: float = 1e-13, warm_start: bool = False):
        if mass not in self.MASS:
            raise ValueError(f"pde filter: mass = {mass!r}, must be 'lumped' or 'consistent'")
        self.ctx, self.lib, self.mesh = ctx, ctx.lib, mesh
        self.dm = mesh.device(ctx)
        self.n, self.radius, self.mass = int(self.dm.n_cell), float(radius), mass
        self.rtol, self.warm_start = float(rtol), bool(warm_start)
        h = _lib.H()
        _check_rc2(self.lib.femo_pde_filter_create(self.dm.handle, self.radius, self.MASS[mass], C.byref(h)))
        self.handle = h
        _check_rc2(self.lib.femo_pde_filter_set(self.handle, self.rtol, int(self.warm_start)))
        self.nnz = int(self.dm.info["nnz"])
        self.last_info = None

    def apply(self, x: Vec, y: Vec, transpose: bool = False) -> Vec:
        info = _lib.SolveInfo()
        try:
            _check_rc2(self.lib.femo_pde_filter_apply(self.handle, int(bool(transpose)), x.handle, y.handle, None, C.byref(info)))
        finally:
            self.last_info = {k: getattr(info, k) for k, _ in _lib.SolveInfo._fields_}
        return y

    def export_csr(self):
        """(rowptr, col, val) of A on the mesh pattern, rows sorted by column."""
        rowptr = np.zeros(self.dm.n_rows + 1, np.int64)
        col = np.zeros(self.nnz, np.int32)
        val = np.zeros(self.nnz)
        check(self.lib.femo_pde_filter_export_csr(self.handle, _ptr(rowptr), _ptr(col), _ptr(val)))
        return rowptr, col, val

    @property
    def bytes(self) -> int:
        """Device bytes the handle holds now (the scaled copy of A appears with the first solve)."""
        b = C.c_int64(0)
        check(self.lib.femo_pde_filter_bytes(self.handle, C.byref(b)))
        return int(b.value)

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None) and getattr(self.dm, "handle", None):
                self.lib.femo_pde_filter_destroy(h)
        except Exception:
            pass


def check_projection_params(n: int, beta, eta, volumes=None, solid=(), void=(), void_value: float = 1e-4):
    """Validates the parameters of the projection without a device and returns them as
    (beta, eta, mode, volumes or None, solid, void, void_value); ``eta`` is a float in [0, 1] or ``"volume"``."""
    n = int(n)
    if n < 1:
        raise ValueError(f"projection: n = {n}, need at least one cell")
    beta = float(beta)
    if not (np.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"projection: beta = {beta}, must be finite and >= 0")
    if isinstance(eta, str):
        if eta != "volume":
            raise ValueError(f"projection: eta = {eta!r}, must be a number in [0, 1] or 'volume'")
        mode, eta = _lib.PROJECT_VOLUME, 0.5
    else:
        mode, eta = _lib.PROJECT_FIXED, float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"projection: eta = {eta}, must lie in [0, 1]")
    void_value = float(void_value)
    if not 0.0 < void_value <= 1.0:
        raise ValueError(f"projection: void_value = {void_value}, must lie in (0, 1]")
    sets = []
    for name, idx in (("solid", solid), ("void", void)):
        raw = np.asarray(() if idx is None else idx).ravel()
        if raw.size and not np.issubdtype(raw.dtype, np.integer):
            raise ValueError(f"projection: {name} must hold integer cell indices")
        a = np.ascontiguousarray(raw, dtype=np.int64)
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError(f"projection: a {name} cell lies outside 0..{n - 1}")
        sets.append(a)
    if np.intersect1d(sets[0], sets[1]).size:
        raise ValueError("projection: a cell is both solid and void")
    if volumes is not None:
        volumes = np.ascontiguousarray(volumes, dtype=np.float64).ravel()
        if volumes.size != n:
            raise ValueError(f"projection: {volumes.size} volumes for n = {n}")
        if not (np.all(np.isfinite(volumes)) and np.all(volumes > 0.0)):
            raise ValueError("projection: the volumes must be positive and finite")
    if mode == _lib.PROJECT_VOLUME and np.union1d(sets[0], sets[1]).size >= n:
        raise ValueError("projection: the volume-preserving threshold needs an active cell")
    return beta, eta, mode, volumes, sets[0], sets[1], void_value


def _check_rc2(rc: int) -> None:
    """The library's error path; an input it refused (rc 2) is a ValueError."""
    if rc == 0:
        return
    msg = _lib.load().femo_last_error()
    msg = msg.decode() if msg else f"libfemo_hip error {rc}"
    if rc == 2:
        raise ValueError(msg)
    raise _lib.FemoError(msg)


class DeviceProjection:
    """femo_project (csrc/project.hip): rho = H(xt; beta, eta) on the active cells, 1 on ``solid``, ``void_value`` on ``void``;
    ``eta`` a number in [0, 1] or ``"volume"`` (the volume-preserving threshold, 53 bisection steps on the device)."""

    def __init__(self, ctx, n: int, beta: float = 0.0, eta=0.5, volumes=None, solid=(), void=(), void_value: float = 1e-4):
        self.ctx, self.lib = ctx, ctx.lib
        self.n = int(n)
        beta, eta_, mode, v, s, w, vv = check_projection_params(n, beta, eta, volumes, solid, void, void_value)
        self._beta, self._eta = beta, ("volume" if mode == _lib.PROJECT_VOLUME else eta_)
        self.n_passive = int(s.size + w.size)
        h = _lib.H()
        _check_rc2(self.lib.femo_project_create(ctx.handle, self.n, None if v is None else _ptr(v), s.size, _ptr(s) if s.size else None,
                                                w.size, _ptr(w) if w.size else None, vv, beta, eta_, mode, C.byref(h)))
        self.handle = h

    @property
    def beta(self) -> float:
        return self._beta

    @property
    def eta(self):
        return self._eta

    def set(self, beta=None, eta=None) -> None:
        beta = self._beta if beta is None else beta
        eta = self._eta if eta is None else eta
        volume = isinstance(eta, str)
        if volume and eta != "volume":
            raise ValueError(f"projection: eta = {eta!r}, must be a number in [0, 1] or 'volume'")
        _check_rc2(self.lib.femo_project_set(self.handle, float(beta), 0.5 if volume else float(eta),
                                             _lib.PROJECT_VOLUME if volume else _lib.PROJECT_FIXED))
        self._beta, self._eta = float(beta), (eta if volume else float(eta))

    @staticmethod
    def _info(info: "_lib.ProjectInfo") -> dict:
        return {k: getattr(info, k) for k, _ in _lib.ProjectInfo._fields_ if k != "reserved"}

    def forward(self, xt: Vec, rho: Vec, info: bool = True) -> Optional[dict]:
        rec = _lib.ProjectInfo()
        _check_rc2(self.lib.femo_project_forward(self.handle, xt.handle, rho.handle, C.byref(rec) if info else None))
        return self._info(rec) if info else None

    def filter_forward(self, filt, x: Vec, xt: Vec, rho: Vec, info: bool = True) -> Optional[dict]:
        """xt = W x and rho = P(xt) with a DeviceFilter (fixed threshold: one launch) or a DevicePdeFilter (load, solve, and
        one launch for the cell means and the projection)."""
        rec = _lib.ProjectInfo()
        entry = self.lib.femo_pde_filter_project if isinstance(filt, DevicePdeFilter) else self.lib.femo_filter_project
        _check_rc2(entry(filt.handle, self.handle, x.handle, xt.handle, rho.handle, C.byref(rec) if info else None))
        return self._info(rec) if info else None

    def reverse(self, xt: Vec, a: Vec, out: Vec) -> Vec:
        _check_rc2(self.lib.femo_project_reverse(self.handle, xt.handle, a.handle, out.handle))
        return out

    def tangent(self, xt: Vec, d: Vec, out: Vec) -> Vec:
        _check_rc2(self.lib.femo_project_tangent(self.handle, xt.handle, d.handle, out.handle))
        return out

    def grayness(self, rho: Vec) -> float:
        m = C.c_double(0.0)
        _check_rc2(self.lib.femo_project_grayness(self.handle, rho.handle, C.byref(m)))
        return float(m.value)

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None):
                self.lib.femo_project_destroy(h)
        except Exception:
            pass


# ----------------------------------------------------------------------------------------- boundary data / UFL ----
class Constant:
    """dolfinx.fem.Constant(mesh, value) [ext]: a spatially constant scalar or vector (run_topo_opt_cantilever_beam.py:73)."""

    def __init__(self, mesh, value):
        self.mesh = mesh
        self.value = np.array(value, dtype=np.float64)

    def __array__(self, dtype=None, copy=None):
        return self.value if dtype is None else self.value.astype(dtype)


def meshtags(mesh, dim: int, entities, values) -> MeshTags:
    """dolfinx.mesh.meshtags [ext]: entities (as returned by locate_entities_boundary, one row of vertices each) with
    integer tags (run_topo_opt_cantilever_beam.py:46-47)."""
    ents = np.asarray(entities, dtype=np.int32).reshape(len(np.atleast_1d(values)), -1)
    if ents.size and ents.shape[1] != dim + 1:
        raise ValueError(f"entities of dimension {dim} have {dim + 1} vertices")
    return MeshTags(dim, ents, np.atleast_1d(values))


class Measure:
    """ufl.Measure('ds', domain=mesh, subdomain_data=tags) [ext]; ``ds_(100)`` selects the facets tagged 100
    (run_topo_opt_cantilever_beam.py:51-52).  Without subdomain data (or tag) it is the whole exterior boundary."""

    def __init__(self, integral_type: str = "ds", domain=None, subdomain_data: Optional[MeshTags] = None,
                 metadata=None, subdomain_id=None):
        if integral_type != "ds":
            raise NotImplementedError("Measure: only exterior facet integrals ('ds') are in the catalogue")
        self.integral_type, self.mesh, self.subdomain_data = integral_type, domain, subdomain_data
        self.metadata, self.subdomain_id = metadata, subdomain_id

    def __call__(self, subdomain_id) -> "Measure":
        return Measure(self.integral_type, self.mesh, self.subdomain_data, self.metadata, subdomain_id)

    def facets(self) -> np.ndarray:
        """(n, tdim) vertex ids of the facets the measure integrates over."""
        tags = self.subdomain_data
        if tags is not None and self.subdomain_id is not None:
            return tags.entities[tags.find(self.subdomain_id)]
        from .mesh import locate_entities_boundary
        return locate_entities_boundary(self.mesh, self.mesh.tdim - 1, lambda x: np.ones(x.shape[1], dtype=bool))


def _traction(t, mesh) -> Optional[np.ndarray]:
    """None: no traction (a load case that carries a body force alone)."""
    if t is None:
        return None
    tv = np.ravel(np.asarray(t.value if isinstance(t, Constant) else t, dtype=np.float64))
    if tv.size != mesh.tdim:
        raise ValueError(f"the traction needs {mesh.tdim} components")
    return tv


def _body_forces(name: str, body_forces, n_cases: int, mesh) -> Optional[np.ndarray]:
    """(n_cases, tdim) body forces, a None entry being the zero vector; None when there is no body force at all."""
    if body_forces is None:
        return None
    body_forces = list(body_forces)
    if len(body_forces) != n_cases:
        raise ValueError(f"{name}: {n_cases} load cases need as many body forces")
    if all(b is None for b in body_forces):
        return None
    B = np.zeros((n_cases, mesh.tdim))
    for l, b in enumerate(body_forces):
        if b is None:
            continue
        bv = np.ravel(np.asarray(b.value if isinstance(b, Constant) else b, dtype=np.float64))
        if bv.size != mesh.tdim:
            raise ValueError(f"{name}: the body force needs {mesh.tdim} components")
        B[l] = bv
    return B


class ThermalExpansion:
    """The thermal strain alpha (T - T_ref) I of the static residuals and compliances (``thermal=``): ``alpha`` the linear
    expansion coefficient, ``temperature`` a number (uniform) or a Function(FunctionSpace(mesh, ("CG", 1))) -- an input of
    the form then, e.g. the state of a `ConductionResidual`'s FEA --, ``scales`` one factor per load case (default 1 for
    every case; 0 switches a case off).  One temperature serves all load cases."""

    def __init__(self, alpha: float, temperature, T_ref: float = 0.0, scales=None):
        self.alpha, self.T_ref = float(alpha), float(T_ref)
        if not (np.isfinite(self.alpha) and np.isfinite(self.T_ref)):
            raise ValueError("ThermalExpansion: alpha and T_ref must be finite")
        if isinstance(temperature, Function):
            Q = temperature.function_space
            if not isinstance(Q, FunctionSpace) or Q.family != "CG":
                raise NotImplementedError("ThermalExpansion: the temperature needs a FunctionSpace(mesh, ('CG', 1))")
            self.temperature = temperature
        else:
            self.temperature = float(temperature)
        self.scales = None if scales is None else np.array(scales, dtype=np.float64).ravel()
        if self.scales is not None and not np.all(np.isfinite(self.scales)):
            raise ValueError("ThermalExpansion: the scales must be finite")

    @property
    def function(self) -> Optional[Function]:
        """The temperature Function, or None for a uniform temperature."""
        return self.temperature if isinstance(self.temperature, Function) else None


class _ThermalTerm:
    """A `ThermalExpansion` bound to a form: its density, stiffness law and handle (E, nu), and the scales of the form's
    load cases (the weights of a compliance folded in).  The three products of csrc/elast_thermal.hip for that form."""

    def __init__(self, name: str, thermal: ThermalExpansion, mesh, rho: Function, n_cases: int, E: float, nu: float,
                 method_id: int, weights=None):
        if not isinstance(thermal, ThermalExpansion):
            raise TypeError(f"{name}: thermal= takes a ThermalExpansion")
        T = thermal.function
        if T is not None and T.function_space.mesh is not mesh:
            raise NotImplementedError(f"{name}: the temperature needs a CG1 space on the state's mesh")
        s = np.ones(n_cases) if thermal.scales is None else thermal.scales
        if s.size != n_cases:
            raise ValueError(f"{name}: {n_cases} load cases need as many thermal scales")
        self.thermal, self.mesh, self.rho, self.method_id = thermal, mesh, rho, method_id
        self.E, self.nu, self.n_cases = float(E), float(nu), n_cases
        self.scales = s.copy() if weights is None else s * np.asarray(weights, dtype=np.float64)

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def key(self) -> tuple:
        T = self.thermal.function
        return (None, self.thermal.temperature) if T is None else (T.version, id(T.vec))

    def _temperature(self):
        T = self.thermal.function
        return self.thermal.temperature if T is None else T.vec

    def load(self, y: Vec, **kw) -> Vec:
        """y_l = [...] + a s_l H(C(rho); theta)"""
        th = self.thermal
        return self.device().thermal_apply(self.method_id, "N", self.n_cases, self.scales, th.alpha, self.rho.vec,
                                           self._temperature(), y, T_ref=th.T_ref, **kw)

    def drho(self, transpose: bool, x: Vec, y: Vec, a: float, accumulate: bool = True) -> Vec:
        """forward: y_l (+)= a s_l H(C'(rho) x; theta); transposed: y[n_cell] (+)= a sum_l s_l (T_rho product of x_l)"""
        th = self.thermal
        return self.device().thermal_apply(self.method_id, "T_rho" if transpose else "N", self.n_cases, self.scales, th.alpha,
                                           self.rho.vec, self._temperature(), y, T_ref=th.T_ref, x=x, a=a, accumulate=accumulate)

    def dtemp(self, transpose: bool, x: Vec, y: Vec, a: float, accumulate: bool = False) -> Vec:
        """forward: y_l (+)= a s_l H(C(rho); x) for the nodal field x; transposed: y[n_vert] (+)= a sum_l s_l (T_T product of x_l)"""
        dev = self.device()
        if transpose:
            return dev.thermal_apply(self.method_id, "T_temp", self.n_cases, self.scales, self.thermal.alpha, self.rho.vec, 0.0, y,
                                     x=x, a=a, accumulate=accumulate)
        return dev.thermal_apply(self.method_id, "N", self.n_cases, self.scales, self.thermal.alpha, self.rho.vec, x, y, a=a,
                                 accumulate=accumulate)


def _facets_of(measures, tractions) -> list:
    """The tagged facets of every load case that has a traction (None for the others: they need none)."""
    return [None if t is None else ds.facets() for ds, t in zip(measures, tractions)]


def _load_vec(mesh, facets: np.ndarray, t: np.ndarray) -> Vec:
    """F = int_ds t . v ds on the device, cached per (facets, t)."""
    cache = mesh.__dict__.setdefault("_elast_loads", {})
    key = (id(_ctx()), hash(np.ascontiguousarray(facets, dtype=np.int32).tobytes()), tuple(t))
    F = cache.get(key)
    if F is None:
        dev = elasticity_handle(mesh)
        F = Vec(_ctx(), mesh.tdim * mesh.n_vert)
        dev.set_facets(facets)
        dev.load(t, F)
        cache[key] = F
    return F


def _check_springs(name: str, springs, n_dof: int) -> Optional[np.ndarray]:
    """The per-dof stiffnesses as a contiguous float array, or None for none (None, or all zeros)."""
    if springs is None:
        return None
    k = np.ascontiguousarray(springs, dtype=np.float64).ravel()
    if k.size != n_dof:
        raise ValueError(f"{name}: {n_dof} dofs need as many spring stiffnesses, got {k.size}")
    if not (np.all(np.isfinite(k)) and np.all(k >= 0.0)):
        raise ValueError(f"{name}: spring stiffnesses must be finite and >= 0")
    return k.copy() if k.any() else None


def _one_space(name: str, V) -> VectorFunctionSpace:
    """The space of one displacement field: V itself, or the base of a LoadCaseSpace."""
    V = V.base if isinstance(V, LoadCaseSpace) else V
    if not isinstance(V, VectorFunctionSpace):
        raise NotImplementedError(f"{name} needs a VectorFunctionSpace(mesh, ('CG', 1))")
    return V


def facet_measures(mesh, facets: np.ndarray) -> np.ndarray:
    """|f| of every facet (rows of tdim vertex ids): edge lengths in 2-D, triangle areas in 3-D."""
    f = np.asarray(facets, dtype=np.int64).reshape(-1, mesh.tdim)
    p = mesh.x[f][:, :, :mesh.tdim]
    if mesh.tdim == 2:
        return np.linalg.norm(p[:, 1] - p[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def lumped_facet_measure(mesh, facets: np.ndarray) -> np.ndarray:
    """(n_vert,) sum_{f around v} |f| / d: the lumping of the traction load (femo_elast_load)."""
    f = np.asarray(facets, dtype=np.int64).reshape(-1, mesh.tdim)
    out = np.zeros(mesh.n_vert)
    np.add.at(out, f.ravel(), np.repeat(facet_measures(mesh, f) / mesh.tdim, mesh.tdim))
    return out


def lumped_cell_volume(mesh) -> np.ndarray:
    """(n_vert,) sum_{e around v} |T_e| / (d + 1)."""
    out = np.zeros(mesh.n_vert)
    np.add.at(out, mesh.conn.ravel(), np.repeat(cell_volumes(mesh) / (mesh.tdim + 1), mesh.tdim + 1))
    return out


def point_springs(V, dofs, k) -> np.ndarray:
    """Per-dof stiffnesses of springs ``k`` (a scalar or one per entry) on the dofs ``dofs`` of V (a workpiece, an input or
    output port); repeated dofs add up, and so do the arrays of several supports."""
    V = _one_space("point_springs", V)
    dofs = np.atleast_1d(np.asarray(dofs, dtype=np.int64)).ravel()
    kv = np.broadcast_to(np.asarray(k, dtype=np.float64), dofs.shape)
    if dofs.size and (dofs.min() < 0 or dofs.max() >= V.dim):
        raise ValueError(f"point_springs: dof out of range (0 to {V.dim - 1})")
    if not (np.all(np.isfinite(kv)) and np.all(kv >= 0.0)):
        raise ValueError("point_springs: spring stiffnesses must be finite and >= 0")
    out = np.zeros(V.dim)
    np.add.at(out, dofs, kv)
    return out


def facet_springs(V, ds: "Measure", kappa) -> np.ndarray:
    """Per-dof stiffnesses of a Winkler foundation of stiffness per area ``kappa`` (a scalar or a d-vector) on the facets of
    ``ds``, lumped like the traction load: k_{v,i} = kappa_i sum_{f around v} |f| / d."""
    V = _one_space("facet_springs", V)
    d = V.mesh.tdim
    kap = np.asarray(kappa, dtype=np.float64).ravel()
    kap = np.full(d, kap[0]) if kap.size == 1 else kap
    if kap.size != d or not (np.all(np.isfinite(kap)) and np.all(kap >= 0.0)):
        raise ValueError(f"facet_springs: kappa is a scalar or {d} components, finite and >= 0")
    return (lumped_facet_measure(V.mesh, ds.facets())[:, None] * kap[None, :]).ravel()


def port_displacement(V, dofs, coeffs=1.0) -> np.ndarray:
    """The vector l of a point output u_out = l . u: ``coeffs`` (a scalar or one per entry) on the dofs ``dofs`` of V."""
    V = _one_space("port_displacement", V)
    dofs = np.atleast_1d(np.asarray(dofs, dtype=np.int64)).ravel()
    cv = np.broadcast_to(np.asarray(coeffs, dtype=np.float64), dofs.shape)
    if dofs.size == 0 or dofs.min() < 0 or dofs.max() >= V.dim:
        raise ValueError(f"port_displacement: needs dofs in 0 to {V.dim - 1}")
    out = np.zeros(V.dim)
    np.add.at(out, dofs, cv)
    return out


def mean_displacement(V, direction, ds: "Measure") -> np.ndarray:
    """The vector l of the mean displacement of the facets of ``ds`` along ``direction``: the traction load of ``direction``
    (femo_elast_load) over |Gamma|."""
    V = _one_space("mean_displacement", V)
    t = _traction(direction, V.mesh)
    w = lumped_facet_measure(V.mesh, ds.facets())
    if not w.sum() > 0.0:
        raise ValueError("mean_displacement: the measure has no facets")
    return (w[:, None] * t[None, :]).ravel() / w.sum()


def _owned_stiffness(owner, mask: Optional[np.ndarray]) -> DeviceElasticity:
    """The handle of ``owner`` (its ``device()``, ``rho``, ``method_id``, ``preconditioner``) with K(rho) of the current density
    and the fixed set ``mask``, and with the owner's elastic supports (its ``springs``, none without the attribute):
    reassembled when the density (its version or its vector), the fixed set, the springs, the method or the owner changed
    since the last assembly on this handle."""
    dev = owner.device()
    want = None if mask is None else hash(mask.tobytes())
    if dev.fixed_key != want:
        dev.set_fixed(mask)
    springs = getattr(owner, "springs", None)     # the handle is shared per mesh: an owner without springs clears them
    if dev.springs_key != (None if springs is None else hash(springs.tobytes())):
        dev.set_springs(springs)
    key = (owner.rho.version, id(owner.rho.vec), dev.fixed_key, dev.springs_key, owner.method_id, id(owner))
    if getattr(dev, "_owner", None) != key:
        dev.assemble(owner.method_id, owner.rho.vec)
        dev._owner = key
    if owner.preconditioner == "multilevel" and dev.pc_plan is None:
        dev.pc_setup()
    return dev


def _reciprocal_power_mean(lam: np.ndarray, p: float):
    """J = ((1/n) sum_k lambda_k^-p)^(-1/p) of positive values and c_k = dJ/dlambda_k = (1/n) lambda_k^(-p-1) J^(p+1)."""
    lam = np.asarray(lam, dtype=np.float64)
    lo = lam.min()
    J = lo * np.mean((lam / lo) ** -p) ** (-1.0 / p)
    return J, (lam / J) ** (-p - 1.0) / lam.size


def _fixed_data(n_dof: int, bcs):
    """(mask, values) of a bc list (first bc wins on duplicates); (None, None) without bcs."""
    if not bcs:
        return None, None
    mask = np.zeros(n_dof, dtype=np.uint8)
    vals = np.zeros(n_dof)
    for bc in reversed(list(bcs)):
        mask[bc.dofs] = 1
        vals[bc.dofs] = np.asarray(bc.values(), dtype=np.float64)
    return mask, vals


def _mask_host(S, mask: Optional[np.ndarray], identity: bool = True):
    """The host copy of a masked operator: ``S`` with zero rows and columns on the fixed dofs of ``mask`` and, with
    ``identity``, ones on their diagonal; ``S`` itself without a mask."""
    if mask is None:
        return S
    import scipy.sparse as sp
    free = sp.diags((mask == 0).astype(np.float64))
    S = free @ S @ free
    return (S + sp.diags(mask.astype(np.float64)) if identity else S).tocsr()


# ------------------------------------------------------------------------------------------------------ operators ----
class ElasticityMatrix:
    """dR/du = K(rho) on every column; with ``masked`` the A of state_model.py:149 (identity rows / columns on the fixed
    dofs).  One `mult` is one batched product, one `backend_solve` one batched PCG over all columns."""
    symmetric = True
    pde_kind = None

    def __init__(self, form: "ElasticityResidual", masked: bool = False):
        self.form, self.masked, self.mesh = form, masked, form.mesh
        self._row = None
        self.info = None

    def getSizes(self):
        n = self.form.n_cases * self.form.n_dof
        return (n, n)

    size = property(getSizes)

    def mult(self, x: Vec, y: Vec) -> Vec:
        dev = self.form.stiffness()
        return dev.apply_multi(self.form.n_cases, x, y, masked=self.masked and dev.fixed_key is not None)

    multTranspose = mult

    def new_row_vec(self) -> Vec:
        if self._row is None:
            self._row = Vec(_ctx(), self.getSizes()[0])
        return self._row

    new_col_vec = new_row_vec

    def backend_solve(self, b: Vec, x: Vec, options: Optional[dict] = None) -> None:
        self.info = self.form._matrix_solve(b, x, "adjoint", options)

    def _host_mask(self) -> Optional[np.ndarray]:
        """The fixed set a host copy of this matrix carries: the form's when ``masked``."""
        return self.form._mask if self.masked else None

    def to_scipy(self):
        import scipy.sparse as sp
        K = _mask_host(self.form.stiffness().export_csr(), self._host_mask())
        return K if self.form.n_cases == 1 else sp.block_diag([K] * self.form.n_cases, format="csr")


class MultiLoadElasticityMatrix(ElasticityMatrix):
    """`ElasticityMatrix` of a `MultiLoadElasticityResidual`."""


class _UnsymmetricMatrix(ElasticityMatrix):
    """A dR/du that is not symmetric: the transposed product and the transposed solve are calls of their own.  A subclass
    gives ``_apply(flag, x, y)`` and ``_solve(flag, kind, b, x, options)``, ``flag`` False for the matrix (`mult`, and
    `backend_solve`: the forward mode) and True for its transpose (`multTranspose`, and `backend_solve_transpose`: the
    adjoint); `_solve` leaves what the form's `_record` returns in ``info``."""
    symmetric = False

    def mult(self, x: Vec, y: Vec) -> Vec:
        return self._apply(False, x, y)

    def multTranspose(self, x: Vec, y: Vec) -> Vec:
        return self._apply(True, x, y)

    def backend_solve(self, b: Vec, x: Vec, options: Optional[dict] = None) -> None:
        self._solve(False, "forward", b, x, options)

    def backend_solve_transpose(self, b: Vec, x: Vec, options: Optional[dict] = None) -> None:
        self._solve(True, "adjoint", b, x, options)


class _MatrixFree:
    """A partial of a residual that is never formed, (n_cases n_dof) x the mesh's ``cols`` ("n_cell" or "n_vert"): `mult` and
    `multTranspose` are the subclass's ``_product(transpose, x, y)``."""

    def __init__(self, form: "ElasticityResidual"):
        self.form, self.mesh = form, form.mesh
        self._row = self._col = None

    def getSizes(self):
        return (self.form.n_cases * self.form.n_dof, getattr(self.mesh, self.cols))

    def mult(self, x: Vec, y: Vec) -> Vec:
        return self._product(False, x, y)

    def multTranspose(self, x: Vec, y: Vec) -> Vec:
        return self._product(True, x, y)

    def new_row_vec(self) -> Vec:
        if self._row is None:
            self._row = Vec(_ctx(), self.getSizes()[0])
        return self._row

    def new_col_vec(self) -> Vec:
        if self._col is None:
            self._col = Vec(_ctx(), self.getSizes()[1])
        return self._col


class _ElasticityDrho(_MatrixFree):
    """dR/drho ((n_cases n_dof) x n_cell), matrix free: block l of column e = C'(rho_e) K0_e u_{l,e}, minus the body-load
    operator G_B of a form with body forces and minus s_l H(C'(rho) . ; theta) of a form with a thermal load (F depends on
    the density there), added onto the stiffness term."""
    cols = "n_cell"

    def _product(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        F.device().drho_multi(F.method_id, transpose, F.n_cases, F.rho.vec, F.u.vec, x, y)
        if F.body is not None:
            F.device().body_apply(F.n_cases, F.body, x, y, transpose=transpose, a=-1.0, accumulate=True)
        if F.thermal is not None:
            F.thermal.drho(transpose, x, y, a=-1.0)
        return y


class _ElasticityDtemp(_MatrixFree):
    """dR/dT ((n_cases n_dof) x n_vert) of a form whose thermal load reads a temperature Function, matrix free: block l =
    -s_l H(C(rho); .), the thermal load as a linear map of the nodal temperatures (csrc/elast_thermal.hip)."""
    cols = "n_vert"

    def _product(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        return self.form.thermal.dtemp(transpose, x, y, a=-1.0)


# ---------------------------------------------------------------------------------------------------------- forms ----
def _loads_vec(mesh, facets_list, tractions, weights=None) -> Optional[Vec]:
    """Column l = w_l F_l (w = 1 without weights).  One unweighted column is the load of `_load_vec` itself; several are
    placed through the host once and cached.  A load case without a traction (None) is a zero column; None when no load
    case has one."""
    if all(t is None for t in tractions):
        return None
    if len(tractions) == 1 and weights is None:
        return _load_vec(mesh, facets_list[0], tractions[0])
    cache = mesh.__dict__.setdefault("_elast_multi_loads", {})
    w = np.ones(len(tractions)) if weights is None else np.asarray(weights, dtype=np.float64)
    key = (id(_ctx()), tuple(None if f is None else hash(np.ascontiguousarray(f, dtype=np.int32).tobytes()) for f in facets_list),
           tuple(None if t is None else tuple(t) for t in tractions), tuple(w))
    F = cache.get(key)
    if F is None:
        n = mesh.tdim * mesh.n_vert
        cols = [np.zeros(n) if tractions[l] is None else
                w[l] * np.array(_load_vec(mesh, facets_list[l], tractions[l]).get(), dtype=np.float64)
                for l in range(len(tractions))]
        F = cache[key] = Vec(_ctx(), len(cols) * n).set(np.concatenate(cols))
    return F


class _BodyLoad:
    """The total load T + G_B rho of a form with body forces, in a Vec of the form's own: rebuilt by one G_B launch whenever
    the density (its version or its vector) or the traction columns changed.  ``B``: (n_cases, tdim), weights included.
    With ``thermal`` (a `_ThermalTerm`) the total is T + G_B rho + s_l H(C(rho); theta), the thermal load one launch of its
    own onto the first (``B`` may then be None: that launch alone), rebuilt when the temperature changed as well."""

    def __init__(self, mesh, rho: Function, B: Optional[np.ndarray], thermal: Optional["_ThermalTerm"] = None):
        self.mesh, self.rho, self.B, self.thermal = mesh, rho, B, thermal
        self.vec = None
        self.key = None

    def total(self, dev: "DeviceElasticity", traction: Optional[Vec], zero_fixed: bool = False) -> Vec:
        key = (self.rho.version, id(self.rho.vec), id(traction), dev.fixed_key if zero_fixed else None)
        if self.thermal is not None:
            key += self.thermal.key()
        if key != self.key:
            L = self.B.shape[0] if self.B is not None else self.thermal.n_cases
            if self.vec is None:
                self.vec = Vec(_ctx(), L * dev.n_dof)
            if self.B is not None:
                dev.body_apply(L, self.B, self.rho.vec, self.vec, base=traction, zero_fixed=zero_fixed)
            if self.thermal is not None:
                self.thermal.load(self.vec, base=None if self.B is not None else traction, zero_fixed=zero_fixed,
                                  accumulate=self.B is not None)
            self.key = key
        return self.vec


def _multi_arguments(name: str, u: Function, tractions, measures, body_forces=None, thermal=None):
    V = u.function_space
    if not isinstance(V, LoadCaseSpace):
        raise NotImplementedError(f"{name} needs a Function(LoadCaseSpace(V, n_cases)) state")
    if getattr(V.mesh, "local", None) is not None and V.mesh.local.nranks > 1:
        raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
    tractions = list(tractions)
    measures = [None] * len(tractions) if measures is None else list(measures)
    if len(tractions) != V.n_cases or len(measures) != V.n_cases:
        raise ValueError(f"{name}: {V.n_cases} load cases need as many tractions and measures")
    if any(t is None for t in tractions) and _body_forces(name, body_forces, V.n_cases, V.mesh) is None and thermal is None:
        raise ValueError(f"{name}: a load case without a traction needs a body force")
    ts = [_traction(t, V.mesh) for t in tractions]
    dss = [ds if ds is not None else Measure("ds", domain=V.mesh) for ds in measures]
    return V, ts, dss, _body_forces(name, body_forces, V.n_cases, V.mesh)


class ElasticityResidual(BackendForm):
    """R(u; rho) = K_s(rho) u - F(rho), K_s = K(rho) + diag(springs) with the elastic supports ``springs`` (one stiffness >= 0
    per dof, from `point_springs` / `facet_springs`; None: K itself; they do not depend on rho, so dR/drho is unchanged), and
    F = the tagged traction ``ds`` (see the module docstring) plus the nodal forces ``point_load`` (one value per dof, the
    input force of a mechanism's port; ``traction`` may then be None) plus, with
    ``body_force`` b (mass density times acceleration, constant), the self-weight G_b rho: rho_e |T_e| b / (d + 1) at every
    vertex of cell e.  ``traction`` may be None with a body force.  ``n_cases`` columns (one here), ``n_dof`` dofs per
    column; every product and solve is the batched one over all columns.

    With a body force `load` is the total F(rho), rebuilt in one launch when the density changes, and dR/drho gains
    -G_b.  RAMP is the usual stiffness law with self-weight: SIMP's rho^3 against the linear mass gives large displacements
    at low density.  F(rho) is non-zero on clamped vertices, so the adjoint is non-zero on fixed dofs: the exact reduced
    gradient needs ``fea.consistent_bc_partials = True``, as for `MultiLoadPnormStress`.

    With ``thermal`` (a `ThermalExpansion`) F gains the thermal expansion load s_l H(C(rho); theta) (module docstring): `load`
    is rebuilt when the density or the temperature changed, dR/drho gains -s_l H(C'(rho) . ; theta), and with a temperature
    Function T the form depends on (u, rho, T), `partial_matrix(T)` being the matrix-free -s_l H(C(rho); .).  ``traction`` may
    be None with a thermal load.  It is non-zero on clamped vertices as well: ``consistent_bc_partials`` as above."""
    rank = 1
    is_linear = True
    is_symmetric = True
    constant_partials = False
    matrix_class = ElasticityMatrix
    max_it = 1_000_000            # the bound on the iterations of a solve (assign to an instance to change it)

    def __init__(self, u: Function, rho: Function, traction, ds: Optional[Measure] = None, E: float = 1.0,
                 nu: float = 0.3, method: str = "SIMP", preconditioner: str = "jacobi", body_force=None, springs=None,
                 point_load=None, thermal: Optional[ThermalExpansion] = None):
        V = u.function_space
        if not isinstance(V, VectorFunctionSpace):
            raise NotImplementedError("ElasticityResidual needs a VectorFunctionSpace(mesh, ('CG', 1)) state")
        self.t = _traction(traction, V.mesh)
        self.ds = ds if ds is not None else Measure("ds", domain=V.mesh)
        body = _body_forces("ElasticityResidual", None if body_force is None else [body_force], 1, V.mesh)
        if point_load is not None:
            point_load = np.ascontiguousarray(point_load, dtype=np.float64).ravel().copy()
            if point_load.size != V.dim or not np.all(np.isfinite(point_load)):
                raise ValueError(f"ElasticityResidual: the point load needs {V.dim} finite entries")
        if self.t is None and body is None and point_load is None and thermal is None:
            raise ValueError("ElasticityResidual: without a traction the load needs a body force, a point load or a thermal load")
        self._setup(u, rho, V, 1, [self.t], [self.ds], E, nu, method, preconditioner, body, springs, thermal)
        self.point_load = point_load

    def _setup(self, u, rho, V, n_cases, tractions, measures, E, nu, method, preconditioner, body=None, springs=None,
               thermal=None) -> None:
        """``V``: the space of one column (the numbering of the bcs and of the springs); ``body``: (n_cases, tdim) body forces
        or None; ``springs``: one stiffness per dof of V or None; ``thermal``: a `ThermalExpansion` or None."""
        if rho.function_space.family != "DG" or rho.function_space.mesh is not V.mesh:
            raise NotImplementedError(f"{type(self).__name__} needs a DG0 density on the state's mesh")
        if method not in METHODS:
            raise ValueError(f"unknown penalisation method {method!r} (SIMP or RAMP)")
        if preconditioner not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {preconditioner!r} (jacobi or multilevel)")
        self.preconditioner = preconditioner
        self.u, self.rho, self.mesh = u, rho, V.mesh
        self.E, self.nu, self.method, self.method_id = float(E), float(nu), method, METHODS[method]
        self.n_cases, self.n_dof = n_cases, V.dim
        self.tractions, self.measures = tractions, measures
        self.body = body
        self.springs = _check_springs(type(self).__name__, springs, V.dim)
        self.point_load, self._point_vec = None, None
        self.thermal = None if thermal is None else _ThermalTerm(type(self).__name__, thermal, V.mesh, rho, n_cases, E, nu,
                                                                  self.method_id)
        self._body_load = self._body_rhs = None
        if body is not None or thermal is not None:
            self._body_load, self._body_rhs = (_BodyLoad(V.mesh, rho, body, self.thermal),
                                               _BodyLoad(V.mesh, rho, body, self.thermal))
        self.rtol = 1e-15
        self._key = None
        self._mask = None
        self._vals = None
        self._res = None
        self._rhs_cache = None
        self.last_info = {}

    def functions(self):
        T = None if self.thermal is None else self.thermal.thermal.function
        return (self.u, self.rho) if T is None else (self.u, self.rho, T)

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def _traction_load(self) -> Optional[Vec]:
        """The part of the load that does not depend on the density: the tractions plus the nodal forces ``point_load``."""
        T = _loads_vec(self.mesh, _facets_of(self.measures, self.tractions), self.tractions)
        if self.point_load is None:
            return T
        if self._point_vec is None or self._point_vec[0] is not T:
            host = self.point_load if T is None else np.array(T.get(), dtype=np.float64) + self.point_load
            self._point_vec = (T, Vec(_ctx(), host.size).set(host))
        return self._point_vec[1]

    def load(self) -> Vec:
        """Column l: the total load F_l(rho)."""
        T = self._traction_load()
        return T if self._body_load is None else self._body_load.total(self.device(), T)

    def _set_bcs(self, bcs) -> None:
        mask, self._vals = _fixed_data(self.n_dof, bcs)
        self._mask = mask

    def stiffness(self) -> DeviceElasticity:
        """The handle with K(rho) of the current density and this form's fixed set: reassembled when either changed."""
        return _owned_stiffness(self, self._mask)

    def _record(self, infos, kind: str):
        """Keeps the record of a solve (``infos``: one per column) and raises when it did not converge; returns what
        the matrix shows as its ``info``.  One column, one flat record; several columns: `MultiLoadElasticityResidual`."""
        from .utils_hip import LAST_KSP_INFO
        info = infos[0]
        self.last_info[kind] = dict(iterations=info.iterations, converged=info.converged, solve_ms=info.solve_ms,
                                    residual_norm=info.residual_norm, rhs_norm=info.rhs_norm,
                                    preconditioner=self.preconditioner)
        LAST_KSP_INFO.append(dict(self.last_info[kind], kind="elasticity_" + kind))
        if info.converged != 1:
            raise RuntimeError(f"elasticity PCG did not converge ({kind}): {info.iterations} iterations, "
                               f"sqrt(r.M^-1 r) = {info.residual_norm:.3e} of {info.rhs_norm:.3e}")
        return info

    def _report(self, infos) -> str:
        return f"elasticity solve: {infos[0].iterations} PCG iterations, {infos[0].solve_ms:.1f} ms"

    def new_matrix(self) -> ElasticityMatrix:
        return self.matrix_class(self)

    def _residual_buffer(self, out: Optional[Vec], n: Optional[int] = None) -> Vec:
        """``out``, or without one the form's own residual vector, allocated on first use (``n`` entries, all columns by
        default)."""
        if out is None:
            if self._res is None:
                self._res = Vec(_ctx(), self.n_cases * self.n_dof if n is None else n)
            out = self._res
        return out

    def assemble_vector(self, out: Optional[Vec] = None) -> Vec:
        """Column l: K u_l - F_l; one launch for all columns (femo_elast_apply_multi)."""
        out = self._residual_buffer(out)
        return self.stiffness().apply_multi(self.n_cases, self.u.vec, out, a=1.0, b=-1.0, f=self.load())

    def partial_matrix(self, wrt: Function, out=None):
        if wrt is self.u:
            return out if isinstance(out, self.matrix_class) and not out.masked else self.matrix_class(self)
        if wrt is self.rho:
            return out if isinstance(out, _ElasticityDrho) else _ElasticityDrho(self)
        if self.thermal is not None and wrt is self.thermal.thermal.function:
            return out if isinstance(out, _ElasticityDtemp) else _ElasticityDtemp(self)
        raise ValueError("the elasticity residual does not depend on that Function")

    def assemble_system(self, bcs, rhs: bool, out, out_nobc):
        if rhs:
            raise NotImplementedError("assembleSystem(rhs=True) for the elasticity form: use solveNonlinear / FEA.solve")
        self._set_bcs(bcs)
        self.stiffness()
        A = out if isinstance(out, self.matrix_class) else self.matrix_class(self)
        A.form, A.masked = self, True
        if isinstance(out_nobc, self.matrix_class):
            out_nobc.form, out_nobc.masked = self, False
        return A, None

    def _rhs(self, dev: DeviceElasticity) -> Vec:
        """Column l: F_l with the Dirichlet lifting, b_l = F_l - K g, b_l = g on the fixed dofs (the same fixed set and
        the same values for every column).  With body forces and homogeneous values it is built on the device in the launch
        that forms the body load (the traction columns as its base, zeros on the fixed dofs), once per density."""
        if self._mask is None:
            return self.load()
        fixed = self._mask == 1
        nonzero = bool(np.any(self._vals[fixed] != 0.0))
        if self._body_rhs is not None and not nonzero:
            return self._body_rhs.total(dev, self._traction_load(), zero_fixed=True)
        F = self.load()
        key = (id(F), hash(self._mask.tobytes()))
        if not nonzero and self._rhs_cache is not None and self._rhs_cache[0] == key:
            return self._rhs_cache[1]
        ctx, L, n = _ctx(), self.n_cases, self.n_dof
        if nonzero:
            g = Vec(ctx, L * n).set(np.tile(np.where(fixed, self._vals, 0.0), L))
            b = Vec(ctx, L * n)
            dev.apply_multi(L, g, b, a=-1.0, b=1.0, f=F)            # F_l - K g
            bh = np.array(b.get()).reshape(L, n)
        else:
            bh = np.array(F.get()).reshape(L, n)
        bh[:, fixed] = self._vals[fixed]
        bv = Vec(ctx, L * n).set(bh.ravel())
        if not nonzero:
            self._rhs_cache = (key, bv)
        return bv

    def _operator(self) -> DeviceElasticity:
        """The handle with everything this form's products and solves read: K(rho) here, M(rho) as well under `_MassCarrying`."""
        return self.stiffness()

    def _solve_columns(self, dev: DeviceElasticity, b: Vec, x: Vec, transpose: bool, **opts) -> list:
        """This form's batched solve for all columns on the handle of `_operator` (``transpose``: with the transposed
        matrix, which is the matrix itself here): K(rho) x_l = b_l, one PCG."""
        return dev.solve_multi(self.n_cases, b, x, pc=self.preconditioner, **opts)

    def _matrix_solve(self, b: Vec, x: Vec, kind: str, options: Optional[dict], transpose: bool = False):
        """`backend_solve` of this form's matrix: the solve under the caller's options, recorded as ``kind``."""
        o = options or {}
        infos = self._solve_columns(self._operator(), b, x, transpose, rtol=o.get("elast_rtol", self.rtol),
                                    max_it=o.get("elast_max_it", self.max_it))
        return self._record(infos, kind)

    def solve_state(self, func: Function, bcs, report: bool = False) -> None:
        """The state of every column with the strongly imposed dofs: ONE batched solve (the form is linear)."""
        self._set_bcs(bcs)
        dev = self._operator()
        infos = self._solve_columns(dev, self._rhs(dev), func.vec, False, rtol=self.rtol, max_it=self.max_it)
        func.version += 1
        self._record(infos, "state")
        if report:
            print(self._report(infos))


class MultiLoadElasticityResidual(ElasticityResidual):
    """Column l of the residual is K(rho) u_l - F_l, with F_l the traction ``tractions[l]`` on ``measures[l]`` plus, with
    ``body_forces`` (one per load case, None = none), the inertial load G_{b_l} rho of `ElasticityResidual` -- gravity, a
    pull-up, a lateral manoeuvre; a load case with a body force may have None as its traction: L load cases
    on one stiffness matrix, one fixed set and one preconditioner.  ``u`` is a Function(LoadCaseSpace(V, L)).  The state
    solve, the adjoint solve (`apply_inverse_jacobian`) and the forward-mode solve are each ONE batched PCG over all columns
    (`DeviceElasticity.solve_multi`): a converged column is frozen while the others iterate.

    Boundary conditions are given in the numbering of the base space V, exactly as for `ElasticityResidual`
    (``fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), ...)], V)``), and hold for every column: the same fixed set,
    the same values, and the lifting b_l = F_l - K g.

    Out of scope: supports that differ between the load cases; partitioned meshes.  The stress outputs of a multi-column
    state are `MultiLoadPnormStress` / `MultiLoadVonMises`.  ``last_info[kind]`` keeps, per kind of solve ("state",
    "adjoint"), the record of the last batched solve with one entry per column under ``columns``; ``solve_counts[kind]``
    counts the batched solves."""
    matrix_class = MultiLoadElasticityMatrix

    def __init__(self, u: Function, rho: Function, tractions, measures=None, E: float = 1.0, nu: float = 0.3,
                 method: str = "SIMP", preconditioner: str = "jacobi", body_forces=None, springs=None,
                 thermal: Optional[ThermalExpansion] = None):
        V, ts, dss, body = _multi_arguments("MultiLoadElasticityResidual", u, tractions, measures, body_forces, thermal)
        self._setup(u, rho, V.base, V.n_cases, ts, dss, E, nu, method, preconditioner, body, springs, thermal)
        self.solve_counts = {"state": 0, "adjoint": 0}

    # How the column-wise solves of this form and of its subclasses are recorded and reported; a subclass changes the data.
    _title, _solver = "elasticity", "PCG"                       # "<title> <solver> did not converge", "<title> solve, ..."
    _kind = "elasticity_multiload_"                             # + the kind of solve: ``kind`` of the LAST_KSP_INFO record
    _residual = "sqrt(r.M^-1 r)"                                # what the solver's residual_norm measures
    _column, _plural = "load case", "load cases"                # what a column is called in the error and in the report
    _count = "n_cases"                                          # the attribute with the number of columns solved for
    _per_column = {}                                            # attribute -> its name in the error: arrays with one value per
    #                                                             column, copied into the record; the error gives the value of
    #                                                             the column that failed

    def _record(self, infos, kind: str):
        """`ElasticityResidual._record` for a column-wise solve: one entry per column under ``columns``, the solve counted in
        ``solve_counts[kind]``; raises on the first column that did not converge and returns ``infos``."""
        from .utils_hip import LAST_KSP_INFO
        n = getattr(self, self._count)
        cols = [dict(iterations=i.iterations, converged=i.converged, residual_norm=i.residual_norm, rhs_norm=i.rhs_norm)
                for i in infos]
        self.solve_counts[kind] = self.solve_counts.get(kind, 0) + 1
        self.last_info[kind] = dict(columns=cols, n_cases=n, iterations=[c["iterations"] for c in cols],
                                    converged=[c["converged"] for c in cols], solve_ms=infos[0].solve_ms,
                                    preconditioner=self.preconditioner,
                                    **{k: getattr(self, k).copy() for k in self._per_column})
        LAST_KSP_INFO.append(dict(self.last_info[kind], kind=self._kind + kind))
        for l, c in enumerate(cols):
            if c["converged"] != 1:
                its = "".join(f", {name} = {getattr(self, k)[l]:.6g}" for k, name in self._per_column.items())
                raise RuntimeError(f"{self._title} {self._solver} did not converge ({kind}, {self._column} {l} of {n}{its}): "
                                   f"{c['iterations']} iterations, {self._residual} = {c['residual_norm']:.3e} of "
                                   f"{c['rhs_norm']:.3e}")
        return infos

    def _report(self, infos) -> str:
        return (f"{self._title} solve, {getattr(self, self._count)} {self._plural}: {[i.iterations for i in infos]} "
                f"{self._solver} iterations, {infos[0].solve_ms:.1f} ms")


class Compliance(BackendForm):
    """J = int_ds t . u ds = F^T u (compliance, run_topo_opt_cantilever_beam.py:108-109); over several columns
    J = sum_l w_l F_l . u_l.  With ``body_force`` the load is the total F(rho) = T + G_b rho of `ElasticityResidual`: the
    density ``rho`` is then required, the form depends on (u, rho), and dJ/drho = G_{wB}^T u (one launch).  With ``thermal``
    (a `ThermalExpansion`; ``rho`` required, ``E``, ``nu`` and ``method`` those of the residual) the load carries s_l H(C(rho);
    theta) as well: the work of the total load, with dJ/drho += sum_l w_l s_l (T_rho product of u_l) and, for a temperature
    Function T (an argument of the form then), dJ/dT = sum_l w_l s_l (T_T product of u_l), one launch each."""
    rank = 0

    def __init__(self, u: Function, traction, ds: Optional[Measure] = None, body_force=None, rho: Optional[Function] = None,
                 thermal: Optional[ThermalExpansion] = None, E: float = 1.0, nu: float = 0.3, method: str = "SIMP"):
        if not isinstance(u.function_space, VectorFunctionSpace):
            raise NotImplementedError("Compliance needs a VectorFunctionSpace(mesh, ('CG', 1)) state")
        self.u, self.mesh = u, u.function_space.mesh
        self.t = _traction(traction, self.mesh)
        self.ds = ds if ds is not None else Measure("ds", domain=self.mesh)
        self.tractions, self.measures, self.weights = [self.t], [self.ds], None
        self._set_body("Compliance", _body_forces("Compliance", None if body_force is None else [body_force], 1, self.mesh), rho,
                       thermal, E, nu, method)

    def _set_body(self, name: str, body: Optional[np.ndarray], rho: Optional[Function], thermal=None, E: float = 1.0,
                  nu: float = 0.3, method: str = "SIMP") -> None:
        """``body``: (n_cases, tdim) or None; kept with the weights folded in (column l = w_l b_l), as are the scales of
        ``thermal``."""
        if body is None and thermal is None and any(t is None for t in self.tractions):
            raise ValueError(f"{name}: a load case without a traction needs a body force")
        if body is not None or thermal is not None:
            if rho is None:
                raise ValueError(f"{name}: the load of a body force or a thermal expansion depends on the density: pass rho")
            if rho.function_space.family != "DG" or rho.function_space.mesh is not self.mesh:
                raise NotImplementedError(f"{name} needs a DG0 density on the state's mesh")
            if body is not None and self.weights is not None:
                body = body * np.asarray(self.weights, dtype=np.float64)[:, None]
        self.thermal = None
        if thermal is not None:
            if method not in METHODS:
                raise ValueError(f"unknown penalisation method {method!r} (SIMP or RAMP)")
            self.thermal = _ThermalTerm(name, thermal, self.mesh, rho, len(self.tractions), E, nu, METHODS[method], self.weights)
        self.body, self.rho = body, rho if (body is not None or thermal is not None) else None
        self._body_load = None if self.rho is None else _BodyLoad(self.mesh, rho, body, self.thermal)

    def functions(self):
        if self.rho is None:
            return (self.u,)
        T = None if self.thermal is None else self.thermal.thermal.function
        return (self.u, self.rho) if T is None else (self.u, self.rho, T)

    def load(self) -> Vec:
        """Column l = w_l F_l, the total load with body forces and the thermal load."""
        T = _loads_vec(self.mesh, _facets_of(self.measures, self.tractions), self.tractions, self.weights)
        return T if self._body_load is None else self._body_load.total(elasticity_handle(self.mesh), T)

    def assemble_scalar(self) -> float:
        return self.load().dot(self.u.vec, self.u.function_space.dim)

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        out = self._gradient_buffer(wrt, out)
        if wrt is self.u:
            return out.copy_from(self.load())
        if self.rho is not None and wrt is self.rho:
            if self.body is not None:
                elasticity_handle(self.mesh).body_apply(self.body.shape[0], self.body, self.u.vec, out, transpose=True)
            if self.thermal is not None:
                self.thermal.drho(True, self.u.vec, out, a=1.0, accumulate=self.body is not None)
            return out
        if self.thermal is not None and wrt is self.thermal.thermal.function:
            return self.thermal.dtemp(True, self.u.vec, out, a=1.0)
        return out.fill(0.0)


class MultiLoadCompliance(Compliance):
    """J = sum_l w_l F_l . u_l over the load cases of a Function(LoadCaseSpace(V, L)) (w = 1 without ``weights``); with
    ``body_forces`` and ``thermal`` (and the density ``rho``) F_l is the total load of `MultiLoadElasticityResidual`."""

    def __init__(self, u: Function, tractions, measures=None, weights=None, body_forces=None, rho: Optional[Function] = None,
                 thermal: Optional[ThermalExpansion] = None, E: float = 1.0, nu: float = 0.3, method: str = "SIMP"):
        V, self.tractions, self.measures, body = _multi_arguments("MultiLoadCompliance", u, tractions, measures, body_forces,
                                                                  thermal)
        self.u, self.mesh = u, V.mesh
        self.weights = np.ones(V.n_cases) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
        if self.weights.size != V.n_cases:
            raise ValueError(f"MultiLoadCompliance: {V.n_cases} load cases need as many weights")
        self._set_body("MultiLoadCompliance", body, rho, thermal, E, nu, method)


class _StateOutput(BackendForm):
    """A scalar output of the state ``u`` alone: its partial in ``u`` is the subclass's ``_state_gradient(out)``, that in any
    other Function zero."""
    rank = 0

    def functions(self):
        return (self.u,)

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        out = self._gradient_buffer(wrt, out)
        return self._state_gradient(out) if wrt is self.u else out.fill(0.0)


class ElasticityDisplacement(_StateOutput):
    """J = sum_l w_l l_l . u_l for host vectors l_l in the numbering of the base space (`port_displacement`,
    `mean_displacement`): the displacement of a port, the mean displacement of a boundary.  dJ/du = w l: `Compliance` with
    another vector.  ``ell``: one vector (used for every column) or one per column."""

    def __init__(self, u: Function, ell, weights=None):
        V = u.function_space
        base = _one_space("ElasticityDisplacement", V)
        L = V.n_cases if isinstance(V, LoadCaseSpace) else 1
        ell = np.asarray(ell, dtype=np.float64)
        if ell.ndim == 1:
            ell = np.tile(ell, (L, 1))
        if ell.shape != (L, base.dim):
            raise ValueError(f"ElasticityDisplacement: {L} columns need vectors of {base.dim} entries")
        if not np.all(np.isfinite(ell)):
            raise ValueError("ElasticityDisplacement: the vectors must be finite")
        self.weights = np.ones(L) if weights is None else _n_values("ElasticityDisplacement", "weights", weights, L)
        self.u, self.mesh, self.n_cases, self.ell = u, V.mesh, L, ell
        self._vec = None

    def load(self) -> Vec:
        """Column l = w_l l_l on the device (uploaded once)."""
        if self._vec is None:
            self._vec = Vec(_ctx(), self.ell.size).set((self.weights[:, None] * self.ell).ravel())
        return self._vec

    def values(self) -> np.ndarray:
        """The unweighted l_l . u_l of the current state (host)."""
        return np.einsum("ln,ln->l", self.ell, np.asarray(self.u.vec.get(), dtype=np.float64).reshape(self.n_cases, -1))

    def assemble_scalar(self) -> float:
        return self.load().dot(self.u.vec, self.u.function_space.dim)

    def _state_gradient(self, out: Vec) -> Vec:
        return out.copy_from(self.load())


class ElasticityPnormDisplacement(_StateOutput):
    """J = sum_l w_l J_l, J_l = (1/alpha) sum_v a_v (m |u_{l,v}|)^p with alpha = sum_v a_v: the aggregated nodal displacement
    of a region, the smooth form of "no vertex of this region moves more than delta" (`max_estimate` <= delta).  ``region``:
    a vertex index array (a_v = 1), a ``ds(tag)`` (a_v = the lumped facet measure) or None (all vertices with their lumped
    cell volume).  On a plain state or a LoadCaseSpace state; value and dJ/du are one pass over the vertices for all columns
    (`DeviceElasticity.pnorm_disp_multi`, csrc/elast_disp.hip).  dJ/du is non-zero on clamped dofs of the region: the exact
    reduced gradient needs ``fea.consistent_bc_partials = True``."""

    def __init__(self, u: Function, region=None, m=1.0, p: float = 8.0, weights=None, E: float = 1.0, nu: float = 0.3):
        V = u.function_space
        base = _one_space("ElasticityPnormDisplacement", V)
        mesh = base.mesh
        L = V.n_cases if isinstance(V, LoadCaseSpace) else 1
        if region is None:
            a = lumped_cell_volume(mesh)
        elif isinstance(region, Measure):
            a = lumped_facet_measure(mesh, region.facets())
        else:
            idx = np.unique(np.asarray(region, dtype=np.int64).ravel())
            if idx.size == 0 or idx.min() < 0 or idx.max() >= mesh.n_vert:
                raise ValueError(f"ElasticityPnormDisplacement: the region needs vertices in 0 to {mesh.n_vert - 1}")
            a = np.zeros(mesh.n_vert)
            a[idx] = 1.0
        if not a.sum() > 0.0:
            raise ValueError("ElasticityPnormDisplacement: the region is empty")
        self.m = _n_values("ElasticityPnormDisplacement", "scales m", m, L)
        self.weights = np.ones(L) if weights is None else _n_values("ElasticityPnormDisplacement", "weights", weights, L)
        if not (np.all(self.m > 0.0) and np.all(np.isfinite(self.m)) and p >= 1.0 and np.isfinite(p)):
            raise ValueError("the displacement aggregate needs m > 0 and a finite p >= 1")
        if not np.all(self.weights >= 0.0):
            raise ValueError("the displacement aggregate needs weights >= 0")
        self.u, self.mesh, self.n_cases, self.a, self.p = u, mesh, L, a, float(p)
        self.alpha = float(a.sum())
        self.E, self.nu = float(E), float(nu)
        self._a_vec = None
        self._values = None

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def _call(self, **kw):
        if self._a_vec is None:
            self._a_vec = Vec(_ctx(), self.a.size).set(self.a)
        return self.device().pnorm_disp_multi(self.n_cases, self.u.vec, self._a_vec, self.m, self.p, self.alpha,
                                              weights=self.weights, **kw)

    def values(self) -> Optional[np.ndarray]:
        """The J_l of the last `assemble_scalar` (unweighted), or None before the first."""
        return None if self._values is None else self._values.copy()

    def max_estimate(self) -> np.ndarray:
        """J_l^(1/p) / m_l per column, from the current state: the p-mean of |u_v| over the region, which tends to the
        maximum from below as p grows."""
        return self._call() ** (1.0 / self.p) / self.m

    def assemble_scalar(self) -> float:
        self._values = self._call()
        return float(self.weights @ self._values)

    def _state_gradient(self, out: Vec) -> Vec:
        self._call(value=False, grad_u=out)
        return out


def cell_volumes(mesh) -> np.ndarray:
    """|T_e| of every simplex."""
    p = mesh.x[mesh.conn]
    J = p[:, 1:, :] - p[:, :1, :]
    fact = 2.0 if mesh.tdim == 2 else 6.0
    return np.abs(np.linalg.det(J)) / fact


def _check_stress_spaces(name: str, u: Function, rho: Optional[Function]) -> None:
    if isinstance(u.function_space, LoadCaseSpace):
        raise NotImplementedError(f"{name} needs a VectorFunctionSpace(mesh, ('CG', 1)) state; for the load cases of a "
                                  "LoadCaseSpace use MultiLoadPnormStress / MultiLoadVonMises")
    if not isinstance(u.function_space, VectorFunctionSpace):
        raise NotImplementedError(f"{name} needs a VectorFunctionSpace(mesh, ('CG', 1)) state")
    if rho is not None and (rho.function_space.family != "DG" or rho.function_space.mesh is not u.function_space.mesh):
        raise NotImplementedError(f"{name} needs a DG0 density on the state's mesh")


def _check_multi_stress_spaces(name: str, u: Function, rho: Optional[Function]) -> LoadCaseSpace:
    V = u.function_space
    if not isinstance(V, LoadCaseSpace):
        raise NotImplementedError(f"{name} needs a Function(LoadCaseSpace(V, n_cases)) state")
    if getattr(V.mesh, "local", None) is not None and V.mesh.local.nranks > 1:
        raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
    if rho is not None and (rho.function_space.family != "DG" or rho.function_space.mesh is not V.mesh):
        raise NotImplementedError(f"{name} needs a DG0 density on the state's mesh")
    return V


class ElasticityPnormStress(BackendForm):
    """J = (1/alpha) sum_e |T_e| (m rho_e^q sigma_vm,e)^p with the solid-material von Mises stress (module docstring);
    alpha = |Omega| unless given.  dJ/du is not a multiple of the load: its adjoint solve is a solve of its own.  Over
    several columns J = sum_l w_l J_l; value, dJ/du (column l = w_l dJ_l/du_l) and dJ/drho each take one pass over the mesh
    for all of them (`DeviceElasticity.pnorm_stress_multi`).  ``m`` is a float here and may be assigned to.  With a thermal
    load (`ThermalExpansion`) the stress gains -C beta_0 theta I, hydrostatic on the 3 x 3 tensor in plane strain too: its
    deviator, and with it sigma_vm, is unchanged, so this output is the thermoelastic one as it stands."""
    rank = 0

    def __init__(self, u: Function, rho: Function, E: float = 1.0, nu: float = 0.3, m: float = 1.0, p: float = 8.0,
                 q: float = 0.5, alpha: Optional[float] = None):
        _check_stress_spaces("ElasticityPnormStress", u, rho)
        self._setup(u, rho, u.function_space.mesh, 1, m, np.ones(1), E, nu, p, q, alpha)
        self.m = float(m)

    def _setup(self, u, rho, mesh, n_cases, m, weights, E, nu, p, q, alpha) -> None:
        if not (np.all(np.asarray(m) > 0.0) and p >= 1.0 and q >= 0.0) or (alpha is not None and not alpha > 0.0):
            raise ValueError("the stress aggregate needs m > 0, p >= 1, q >= 0 and alpha > 0")
        if not np.all(weights >= 0.0):
            raise ValueError("the stress aggregate needs weights >= 0")
        self.u, self.rho, self.mesh, self.n_cases = u, rho, mesh, n_cases
        self.m, self.weights = m, weights
        self.E, self.nu, self.p, self.q = float(E), float(nu), float(p), float(q)
        self.alpha = float(cell_volumes(self.mesh).sum() if alpha is None else alpha)
        self._values = None

    def functions(self):
        return (self.u, self.rho)

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def _call(self, **kw):
        return self.device().pnorm_stress_multi(self.n_cases, self.rho.vec, self.u.vec, self.m, self.p, self.q, self.alpha,
                                                weights=self.weights, **kw)

    def values(self) -> Optional[np.ndarray]:
        """The J_l of the last `assemble_scalar` (unweighted), or None before the first."""
        return None if self._values is None else self._values.copy()

    def assemble_scalar(self) -> float:
        self._values = self._call()
        return float(self.weights @ self._values)

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        out = self._gradient_buffer(wrt, out)
        if wrt is self.u:
            self._call(value=False, grad_u=out)
        elif wrt is self.rho:
            self._call(value=False, grad_rho=out)
        else:
            out.fill(0.0)
        return out


class MultiLoadPnormStress(ElasticityPnormStress):
    """J = sum_l w_l J_l, J_l = (1/alpha) sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p, over the load cases of a
    Function(LoadCaseSpace(V, L)): the worst stress over all load cases as one p-norm constraint.  ``m``: a scalar or one
    scale per load case (the loads differ in magnitude); ``weights`` >= 0, 1 without; p, q, alpha shared, alpha = |Omega|
    unless given.  dJ/du is non-zero on the clamped dofs of every column: the exact reduced gradient needs
    ``fea.consistent_bc_partials``."""

    def __init__(self, u: Function, rho: Function, E: float = 1.0, nu: float = 0.3, m=1.0, p: float = 8.0, q: float = 0.5,
                 alpha: Optional[float] = None, weights=None):
        V = _check_multi_stress_spaces("MultiLoadPnormStress", u, rho)
        m = _n_values("MultiLoadPnormStress", "scales m", m, V.n_cases)
        weights = np.ones(V.n_cases) if weights is None else _n_values("MultiLoadPnormStress", "weights", weights, V.n_cases)
        self._setup(u, rho, V.mesh, V.n_cases, m, weights, E, nu, p, q, alpha)

    def set_scales_from_state(self) -> np.ndarray:
        """m_l = 1 / max_e rho_e^q sigma_vm,e(u_l) from the current state and density, so that the terms of every aggregate
        are O(1).  A load case without stress keeps its scale."""
        cells = Vec(_ctx(), self.mesh.n_cell)
        for l in range(self.n_cases):
            peak = float(np.max(self.device().von_mises_multi(self.n_cases, self.u.vec, cells, self.rho.vec, self.q,
                                                              column=l).get()))
            if peak > 0.0:
                self.m[l] = 1.0 / peak
        return self.m.copy()


class ElasticityVonMises(BackendForm):
    """The cell field rho_e^q sigma_vm,e (q = 0: the stress of the solid material, no density needed); over several columns
    max_l s_l rho_e^q sigma_vm,e(u_l), or the field of one of them.  `project` hands the projection over: onto a DG0 target
    the cell values themselves, onto CG1 the L2 projection of a cell-wise constant.  The thermal stress of a `ThermalExpansion`
    is hydrostatic (see `ElasticityPnormStress`): the field of a thermoelastic state needs no change."""
    rank = 0

    def __init__(self, u: Function, rho: Optional[Function] = None, E: float = 1.0, nu: float = 0.3, q: float = 0.0):
        _check_stress_spaces("ElasticityVonMises", u, rho)
        self._setup(u, rho, u.function_space.mesh, 1, None, None, E, nu, q)

    def _setup(self, u, rho, mesh, n_cases, scales, load_case, E, nu, q) -> None:
        if not q >= 0.0 or (q > 0.0 and rho is None):
            raise ValueError("the relaxed von Mises stress needs q >= 0, and the density when q > 0")
        self.u, self.rho, self.mesh, self.n_cases = u, rho, mesh, n_cases
        self.scales, self.load_case = scales, load_case
        self.E, self.nu, self.q = float(E), float(nu), float(q)
        self._cells = None

    def functions(self):
        return (self.u,) if self.rho is None else (self.u, self.rho)

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def _field(self, out: Vec) -> Vec:
        return self.device().von_mises_multi(self.n_cases, self.u.vec, out, None if self.rho is None else self.rho.vec, self.q,
                                             scales=self.scales, column=self.load_case)

    def project_field(self, target: Function, lump_mass: bool = False) -> Function:
        V = target.function_space
        if V.mesh is not self.mesh or isinstance(V, (VectorFunctionSpace, LoadCaseSpace)) or V.family not in ("DG", "CG"):
            raise NotImplementedError("the von Mises stress is projected onto the DG0 or the CG1 space of the state's mesh")
        if V.family == "DG":
            self._field(target.vec)
            target.version += 1
            return target
        if self._cells is None:
            self._cells = Function(FunctionSpace(self.mesh, ("DG", 0)))
        self._field(self._cells.vec)
        self._cells.version += 1
        from .utils_hip import project
        project(self._cells, target, lump_mass=lump_mass)           # the cell-constant path PowerExpr takes
        return target


class MultiLoadVonMises(ElasticityVonMises):
    """The cell field max_l s_l rho_e^q sigma_vm,e(u_l) over the load cases of a Function(LoadCaseSpace(V, L)) -- the envelope
    -- or, with ``load_case``, s_l rho_e^q sigma_vm,e(u_l) of that load case alone.  ``scales`` > 0: one per load case, 1
    without.  Projected onto DG0 and CG1 as `ElasticityVonMises` is."""

    def __init__(self, u: Function, rho: Optional[Function] = None, E: float = 1.0, nu: float = 0.3, q: float = 0.0,
                 scales=None, load_case: Optional[int] = None):
        V = _check_multi_stress_spaces("MultiLoadVonMises", u, rho)
        if load_case is not None and not 0 <= int(load_case) < V.n_cases:
            raise ValueError(f"MultiLoadVonMises: load case {load_case} of {V.n_cases}")
        scales = None if scales is None else _n_values("MultiLoadVonMises", "scales", scales, V.n_cases)
        if scales is not None and not np.all(scales > 0.0):
            raise ValueError("MultiLoadVonMises needs scales > 0")
        self._setup(u, rho, V.mesh, V.n_cases, scales, None if load_case is None else int(load_case), E, nu, q)


class _BlockModes:
    """What `ElasticityEigenvalues` and `ElasticityBuckling` share: a block of modes solved by the block iteration of
    csrc/elast_block.hip, re-solved only when the key of its inputs changed, from the previous modes (a seeded random block
    the first time).  A subclass names its values (``_values_name``: the key of them in ``last_info``), its record in
    LAST_KSP_INFO (``_kind``) and its solve in the error text (``_solve_name``)."""

    @staticmethod
    def _check_block(name: str, n_modes: int, block: int):
        if not 1 <= n_modes <= block <= _lib.ELAST_MAX_COLS:
            raise ValueError(f"{name}: {n_modes} modes in a block of {block} (1 <= n_modes <= block <= {_lib.ELAST_MAX_COLS})")

    def _setup_block(self, V: VectorFunctionSpace, n_modes: int, block: int, rtol: float, max_outer: int, seed: int):
        self.n_modes, self.block, self.n_dof = n_modes, block, V.dim
        self.rtol, self.pcg_rtol, self.max_outer, self.seed = float(rtol), 1e-12, max_outer, int(seed)
        self.modes = Function(LoadCaseSpace(V, block))
        self._lam = None
        self._key = None
        self._started = False
        self.last_info = {}

    def _solved_values(self, mask: np.ndarray, key: tuple, handle, solve) -> np.ndarray:
        """The first n_modes values: cached while ``key`` and the fixed set ``mask`` stand, otherwise ``solve(handle())``, the
        device call on the handle with K assembled, from the previous modes."""
        key += (hash(mask.tobytes()),)
        if key == self._key:
            return self._lam[:self.n_modes].copy()
        from .utils_hip import LAST_KSP_INFO
        dev = handle()
        if not self._started:                                          # afterwards: the previous modes
            free = mask == 0
            X = np.zeros((self.block, self.n_dof))
            X[:, free] = np.random.default_rng(self.seed).standard_normal((int(free.sum()), self.block)).T
            self.modes.vector[:] = X.ravel()
            self._started = True
        lam, info = solve(dev)
        self.modes.version += 1
        self.last_info = dict(info, **{self._values_name: lam.copy()}, n_modes=self.n_modes, block=self.block)
        LAST_KSP_INFO.append(dict(self.last_info, kind=self._kind))
        if info["converged"] != 1:
            raise RuntimeError(f"elasticity {self._solve_name} solve did not converge: {info['outer_iterations']} outer steps, "
                               f"residuals {info['residual'][:self.n_modes]} above {self.rtol:.1e}")
        self._lam, self._key = lam, key
        return lam[:self.n_modes].copy()


class ElasticityEigenvalues(_BlockModes):
    """The ``n_modes`` lowest eigenpairs of K(rho) phi = lambda M(rho) phi with the supports ``bcs`` (homogeneous; at least
    one: a free-free structure needs a shift, which is out of scope), by `DeviceElasticity.eigs` in a block of ``block``
    columns (the block - n_modes last ones are guard vectors).  M is the consistent P1 mass, density ``density`` times
    m(rho): ``mass_law`` "linear" or "du_olhoff".

    ``modes`` is a Function(LoadCaseSpace(V, block)): M-orthonormal, zeros on the fixed dofs, the entry of largest
    magnitude of each column positive.  `eigenvalues` re-solves only when the density (its version or its vector) or the
    fixed set changed, from the previous modes (a seeded random block the first time).  K is reassembled the way
    `ElasticityResidual.stiffness` does it, on the same handle and with the same ownership key, so a static residual on the
    same mesh keeps working beside it.  ``last_info`` keeps the record of the last solve; a solve that does not converge
    raises.

    Out of scope: partitioned meshes, lumped non-structural masses.  Buckling load factors are `ElasticityBuckling`."""

    def __init__(self, rho: Function, V: VectorFunctionSpace, bcs, n_modes: int, block: Optional[int] = None, E: float = 1.0,
                 nu: float = 0.3, method: str = "SIMP", density: float = 1.0, mass_law: str = "linear",
                 preconditioner: str = "jacobi", rtol: float = 1e-9, seed: int = 0):
        name = type(self).__name__
        if isinstance(V, LoadCaseSpace) or not isinstance(V, VectorFunctionSpace):
            raise NotImplementedError(f"{name} needs the VectorFunctionSpace(mesh, ('CG', 1)) of one displacement field")
        if getattr(V.mesh, "local", None) is not None and V.mesh.local.nranks > 1:
            raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
        if rho.function_space.family != "DG" or rho.function_space.mesh is not V.mesh:
            raise NotImplementedError(f"{name} needs a DG0 density on the mesh of V")
        if method not in METHODS:
            raise ValueError(f"unknown penalisation method {method!r} (SIMP or RAMP)")
        if mass_law not in MASS_LAWS:
            raise ValueError(f"unknown mass law {mass_law!r} (linear or du_olhoff)")
        if preconditioner not in PRECONDITIONERS:
            raise ValueError(f"unknown preconditioner {preconditioner!r} (jacobi or multilevel)")
        n_modes = int(n_modes)
        block = min(_lib.ELAST_MAX_COLS, n_modes + 2) if block is None else int(block)
        self._check_block(name, n_modes, block)
        mask, vals = _fixed_data(V.dim, bcs)
        if mask is None or not mask.any():
            raise NotImplementedError(f"{name}: without supports K is singular (free-free structures need a shift)")
        if np.any(vals != 0.0):
            raise NotImplementedError(f"{name}: the supports of an eigenproblem are homogeneous")
        self.rho, self.V, self.mesh, self._mask = rho, V, V.mesh, mask
        self.E, self.nu, self.method, self.method_id = float(E), float(nu), method, METHODS[method]
        self.density, self.mass_law, self.preconditioner = float(density), mass_law, preconditioner
        self._setup_block(V, n_modes, block, rtol, 200, seed)

    _values_name, _kind, _solve_name = "eigenvalues", "elasticity_eigs", "eigen"

    def device(self) -> DeviceElasticity:
        return elasticity_handle(self.mesh, self.E, self.nu)

    def stiffness(self) -> DeviceElasticity:
        """`ElasticityResidual.stiffness`: the handle with K(rho) of the current density and this object's fixed set."""
        return _owned_stiffness(self, self._mask)

    def eigenvalues(self) -> np.ndarray:
        """lambda_0 <= ... <= lambda_{n_modes-1} of the current density."""
        return self._solved_values(
            self._mask, (self.rho.version, id(self.rho.vec)), self.stiffness,
            lambda dev: dev.eigs(self.n_modes, self.rho.vec, self.modes.vec, block=self.block, density=self.density,
                                 mass_law=self.mass_law, rtol=self.rtol, max_outer=self.max_outer, pcg_rtol=self.pcg_rtol,
                                 pc=self.preconditioner))


class EigenvalueAggregate(BackendForm):
    """J = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p), p >= 1, over the ``n_modes`` lowest eigenvalues of an
    `ElasticityEigenvalues`: a smooth stand-in for lambda_1 (lambda_1 <= J <= n^(1/p) lambda_1, so J >= c bounds lambda_1
    from below by c n^(-1/p)) that is symmetric in the eigenvalues, so it is differentiable where the modes of a cluster swap -- provided
    the cluster lies inside: ``n_modes`` should not split a group of (nearly) equal eigenvalues, since the derivative of a
    single eigenvalue inside a cluster does not exist.  A rank-0 output of the density alone: no state, no adjoint solve.
    dJ/drho is one launch, sum_k c_k dlambda_k/drho with c_k = (1/n) lambda_k^(-p-1) J^(p+1)."""
    rank = 0

    def __init__(self, eigen: ElasticityEigenvalues, p: float = 8.0):
        if not isinstance(eigen, ElasticityEigenvalues):
            raise NotImplementedError("EigenvalueAggregate needs an ElasticityEigenvalues")
        if not p >= 1.0:
            raise ValueError("EigenvalueAggregate needs p >= 1")
        self.eigen, self.rho, self.mesh, self.p = eigen, eigen.rho, eigen.mesh, float(p)
        self._grad_rho = None                      # one buffer of n_cell entries whatever the argument, not `_gradient_buffer`

    def functions(self):
        return (self.rho,)

    def _value(self):
        lam = self.eigen.eigenvalues()
        return _reciprocal_power_mean(lam, self.p)[0], lam

    def assemble_scalar(self) -> float:
        return float(self._value()[0])

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        if out is None:
            if self._grad_rho is None:
                self._grad_rho = Vec(_ctx(), self.mesh.n_cell)
            out = self._grad_rho
        if wrt is not self.rho:
            return out.fill(0.0)
        lam = self.eigen.eigenvalues()
        c = _reciprocal_power_mean(lam, self.p)[1]
        g = self.eigen
        return g.device().eig_drho(g.method_id, g.n_modes, self.rho.vec, g.modes.vec, lam, c, out, density=g.density,
                                   mass_law=g.mass_law)


class ElasticityBuckling(_BlockModes):
    """The ``n_modes`` smallest positive load factors lambda of (K(rho) + lambda K_G(u, rho)) phi = 0 on the free dofs, for the
    state u of ``residual``, an `ElasticityResidual` of one load case: the load lambda F is the linearised buckling load.
    K_G is the geometric stiffness of the cell stress sigma_e = C(rho_e) sigma_0(u_e) with the residual's own stiffness law,
    K_G,e[(a,i),(b,j)] = delta_ij |T_e| g_a . sigma_e g_b.  Density, state, method, E, nu, preconditioner and the fixed set
    are the residual's; K comes from ``residual.stiffness()``, so it is not assembled again and the handle stays the
    residual's (the state must have been solved: before that the residual has no fixed set, and `load_factors` raises).

    Solved by `DeviceElasticity.buckle` in a block of ``block`` columns (all FEMO_ELAST_MAX_COLS unless given: the spectra
    of (-K_G, K) are dense, and 5 columns take 2-3 times the outer steps of 8).  ``modes`` is a Function(LoadCaseSpace(V,
    block)): K-orthonormal, zeros on the fixed dofs, the entry of largest magnitude of each column positive.  `load_factors`
    re-solves only when the density or the state (their versions or vectors) or the fixed set changed, from the previous
    modes (a seeded random block the first time).  ``last_info`` keeps the record of the last solve; a solve that does not
    converge raises.

    Limitation: the block converges to the modes of largest |1 / lambda| of EITHER sign, and a negative lambda is buckling
    under the reversed load.  A load whose negative spectrum dominates (a member in tension) fills the block with those
    before ``n_modes`` positive factors are found; the solve then fails and says so: raise ``block``.

    Out of scope: a stress interpolation of its own or a cut-off against low-density pseudo-modes (the stress carries the
    stiffness law C), several load cases or supports that differ per case, shifted or sign-selective iterations for loads
    whose negative spectrum dominates, partitioned meshes, inhomogeneous supports, nonlinear pre-buckling."""

    def __init__(self, residual: "ElasticityResidual", n_modes: int, block: Optional[int] = None, rtol: float = 1e-9,
                 seed: int = 0):
        name = type(self).__name__
        if not isinstance(residual, ElasticityResidual):
            raise NotImplementedError(f"{name} needs the ElasticityResidual whose state carries the load")
        if isinstance(residual, MultiLoadElasticityResidual) or residual.n_cases != 1:
            raise NotImplementedError(f"{name}: several load cases are out of scope (one ElasticityResidual, one load)")
        if residual.thermal is not None:                              # the pre-stress would need -C beta_0 theta I as well
            raise NotImplementedError(f"{name}: thermal loads are out of scope")
        if getattr(residual.mesh, "local", None) is not None and residual.mesh.local.nranks > 1:
            raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
        n_modes = int(n_modes)
        block = _lib.ELAST_MAX_COLS if block is None else int(block)
        self._check_block(name, n_modes, block)
        self.residual, self.u, self.rho, self.mesh = residual, residual.u, residual.rho, residual.mesh
        self._setup_block(residual.u.function_space, n_modes, block, rtol, 400, seed)

    _values_name, _kind, _solve_name = "load_factors", "elasticity_buckling", "buckling"

    def device(self) -> DeviceElasticity:
        return self.residual.device()

    def _fixed_mask(self) -> np.ndarray:
        R = self.residual
        if R._mask is None or not R._mask.any():
            raise RuntimeError(f"{type(self).__name__}: the residual has no fixed set yet -- solve the state first (the supports "
                               "reach the residual with the solve, and without supports K is singular)")
        if np.any(R._vals[R._mask == 1] != 0.0):
            raise NotImplementedError(f"{type(self).__name__}: inhomogeneous supports are out of scope")
        return R._mask

    def load_factors(self) -> np.ndarray:
        """0 < lambda_0 <= ... <= lambda_{n_modes-1} of the current density and state."""
        R = self.residual                                              # its K and ownership key: no assembly of our own
        return self._solved_values(
            self._fixed_mask(), (self.rho.version, id(self.rho.vec), self.u.version, id(self.u.vec)), R.stiffness,
            lambda dev: dev.buckle(self.n_modes, self.rho.vec, self.u.vec, self.modes.vec, block=self.block, method=R.method_id,
                                   rtol=self.rtol, max_outer=self.max_outer, pcg_rtol=self.pcg_rtol, pc=R.preconditioner))


class BucklingAggregate(BackendForm):
    """J = ((1/n) sum_{k<n} lambda_k^-p)^(-1/p), p >= 1, over the ``n_modes`` smallest positive load factors of an
    `ElasticityBuckling`: the aggregate of `EigenvalueAggregate` (lambda_1 <= J <= n^(1/p) lambda_1, symmetric within a
    cluster, so ``n_modes`` should not split one).  A rank-0 output of (u, rho).  With K-orthonormal modes and
    c_k = dJ/dlambda_k,

      dJ/drho_e = sum_k c_k lambda_k C'(rho_e) [phi_k,e^T K0_e phi_k,e + lambda_k |T_e| sigma_0(u_e) : H_e(phi_k)]
      dJ/du_(b,j) = sum_k c_k lambda_k^2 sum_{e around b} C(rho_e) |T_e| (Sigma_H,e(phi_k) g_b)_j

    with H = (grad phi)^T (grad phi) and Sigma_H = lambda_0 tr(H) I + 2 mu_0 H: one launch each.  The framework's adjoint
    solves K w = dJ/du and applies dR/drho^T (the body-load term included).  dJ/du is non-zero on clamped dofs: the exact
    reduced gradient needs ``fea.consistent_bc_partials = True``, as for `ElasticityPnormStress`."""
    rank = 0

    def __init__(self, buckling: ElasticityBuckling, p: float = 8.0):
        if not isinstance(buckling, ElasticityBuckling):
            raise NotImplementedError("BucklingAggregate needs an ElasticityBuckling")
        if not p >= 1.0:
            raise ValueError("BucklingAggregate needs p >= 1")
        self.buckling, self.u, self.rho, self.mesh, self.p = buckling, buckling.u, buckling.rho, buckling.mesh, float(p)

    def functions(self):
        return (self.u, self.rho)

    def assemble_scalar(self) -> float:
        return float(_reciprocal_power_mean(self.buckling.load_factors(), self.p)[0])

    def assemble_derivative(self, wrt: Function, out: Optional[Vec] = None) -> Vec:
        out = self._gradient_buffer(wrt, out)
        if wrt is not self.u and wrt is not self.rho:
            return out.fill(0.0)
        b = self.buckling
        lam = b.load_factors()
        c = _reciprocal_power_mean(lam, self.p)[1]
        dev, method = b.device(), b.residual.method_id
        if wrt is self.u:
            return dev.buckle_du(method, b.n_modes, self.rho.vec, b.modes.vec, c * lam * lam, out)
        return dev.buckle_drho(method, b.n_modes, self.rho.vec, self.u.vec, b.modes.vec, c * lam, c * lam * lam, out)


# ------------------------------------------------------------------------------------------- harmonic response ----
def _host_mass(mesh, rho: np.ndarray, mass_law: str, density: float):
    """M(rho) as a SciPy CSR matrix (host copy; tests and debugging)."""
    import scipy.sparse as sp
    d, nv = mesh.tdim, mesh.tdim + 1
    m = rho if mass_law == "linear" else np.where(rho >= 0.1, rho, 6e5 * rho ** 6 - 5e6 * rho ** 7)
    w = density * m * cell_volumes(mesh) / ((d + 1) * (d + 2))
    S = (np.ones((nv, nv)) + np.eye(nv))[None, :, :] * w[:, None, None]
    Ms = sp.csr_matrix((S.ravel(), (np.repeat(mesh.conn, nv, axis=1).ravel(), np.tile(mesh.conn, (1, nv)).ravel())),
                       shape=(mesh.n_vert, mesh.n_vert))
    return sp.kron(Ms, sp.identity(d), format="csr")


class HarmonicElasticityMatrix(MultiLoadElasticityMatrix):
    """dR/du of a `HarmonicElasticityResidual`: K(rho) - omega_l^2 M(rho) on column l, symmetric; with ``masked`` identity
    rows / columns on the fixed dofs.  One `mult` is one fused product over all columns, one `backend_solve` one batched
    MINRES."""

    def mult(self, x: Vec, y: Vec) -> Vec:
        F = self.form
        dev = F.dynamic()
        return dev.dyn_apply_multi(F.n_cases, F.shifts, x, y, masked=self.masked and dev.fixed_key is not None)

    multTranspose = mult

    def to_scipy(self):
        import scipy.sparse as sp
        F = self.form
        K = F.dynamic().export_csr()
        M = _host_mass(F.mesh, np.array(F.rho.vec.get(), dtype=np.float64), F.mass_law, F.density)
        return sp.block_diag([_mask_host((K - sg * M).tocsr(), self._host_mask()) for sg in F.shifts], format="csr")


class _HarmonicDrho(_ElasticityDrho):
    """dR/drho of a `HarmonicElasticityResidual`: block l of column e = C'(rho_e) K0_e u_{l,e} - omega_l^2 density m'(rho_e)
    M0_e u_{l,e}; the mass term is one launch for all columns, added onto the stiffness term."""

    def _product(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        super()._product(transpose, x, y)
        return F.device().mass_drho_multi(transpose, F.n_cases, -F.shifts, F.rho.vec, F.u.vec, x, y, density=F.density,
                                          mass_law=F.mass_law, accumulate=True)


class _MassCarrying:
    """What the residuals with a mass matrix share, mixed in ahead of their static base: M(rho) beside K(rho) on the handle,
    the ``density`` / ``mass_law`` arguments and their solver's tolerance, and what none of them takes: body forces, thermal
    loads, inhomogeneous supports."""

    @staticmethod
    def _refuse_loads(name: str, body, thermal) -> None:
        if body is not None:
            raise NotImplementedError(f"{name}: body forces are out of scope")
        if thermal is not None:
            raise NotImplementedError(f"{name}: thermal loads are out of scope")

    @staticmethod
    def _check_mass(name: str, density: float, mass_law: str) -> None:
        if mass_law not in MASS_LAWS:
            raise ValueError(f"unknown mass law {mass_law!r} (linear or du_olhoff)")
        if not (np.isfinite(density) and density >= 0.0):
            raise ValueError(f"{name}: the mass density must be finite and >= 0")

    def _set_mass(self, density: float, mass_law: str, rtol: float) -> None:
        """After `_setup`: the checked mass arguments, and the tolerance of this form's solver in place of the PCG's 1e-15."""
        self.density, self.mass_law = float(density), mass_law
        self.rtol = rtol

    def _set_bcs(self, bcs) -> None:
        super()._set_bcs(bcs)
        if self._mask is not None and np.any(self._vals[self._mask == 1] != 0.0):
            raise NotImplementedError(f"{self._supports_name}: inhomogeneous supports are out of scope")

    def dynamic(self) -> DeviceElasticity:
        """`stiffness()` with M(rho) of the current density as well: reassembled when the density (its version or its
        vector), the mass density or the mass law changed since the last mass assembly on this handle."""
        dev = self.stiffness()
        key = (self.rho.version, id(self.rho.vec), self.density, self.mass_law)
        if getattr(dev, "_mass_owner", None) != key:
            dev.mass_assemble(self.rho.vec, density=self.density, mass_law=self.mass_law)
            dev._mass_owner = key
        return dev

    _operator = dynamic


class HarmonicElasticityResidual(_MassCarrying, MultiLoadElasticityResidual):
    """Column l of the residual is (K(rho) - omega_l^2 M(rho)) u_l - F_l: the undamped response to the time-harmonic load
    F_l cos(omega_l t), in real arithmetic.  ``u`` is a Function(LoadCaseSpace(V, L)); ``omegas``: one angular frequency
    >= 0 per column (a frequency sweep under one load repeats the traction); M = ``density`` sum_e m(rho_e) M0_e is the
    consistent P1 mass of `ElasticityEigenvalues` with ``mass_law`` "linear" or "du_olhoff".  One K, one M, one fixed set
    and one preconditioner (block-Jacobi or multilevel, of the unshifted K) serve all columns.

    A `MultiLoadElasticityResidual` in everything else: the state solve, the adjoint solve and the forward-mode solve are
    each ONE batched MINRES (`DeviceElasticity.dyn_solve_multi`) -- K - omega^2 M is indefinite above the first resonance,
    where PCG breaks down -- and dR/drho = C'(rho) K0 u - omega^2 density m'(rho) M0 u.  M is reassembled only when the density
    (its version or its vector), ``density`` or ``mass_law`` changed.  ``rtol`` is 1e-12, not the 1e-15 of the PCG forms:
    MINRES stops on a recurrence estimate of the residual, which parts from the true residual near eps cond; ``max_it``
    bounds the iterations of a solve.  A column that does not converge raises, naming the column and its omega.  Close to a resonance the iteration count grows and
    the response is large: keep the frequencies away from the eigenfrequencies of the design (`ElasticityEigenvalues`).

    Damping: `DampedHarmonicElasticityResidual`.  Out of scope: shifted or deflated preconditioners, frequency-band integrals,
    viscous dampers at points, body forces, inhomogeneous supports, partitioned meshes."""
    matrix_class = HarmonicElasticityMatrix
    _supports_name = "HarmonicElasticityResidual"
    _title, _solver, _kind, _residual = "harmonic elasticity", "MINRES", "elasticity_harmonic_", "estimated sqrt(r.M^-1 r)"
    _column, _plural, _per_column = "column", "frequencies", {"omegas": "omega"}

    def __init__(self, u: Function, rho: Function, tractions, measures=None, omegas=None, density: float = 1.0,
                 mass_law: str = "linear", E: float = 1.0, nu: float = 0.3, method: str = "SIMP",
                 preconditioner: str = "jacobi", body_forces=None, thermal=None):
        name = "HarmonicElasticityResidual"
        self._refuse_loads(name, body_forces, thermal)
        if any(t is None for t in list(tractions)):
            raise ValueError(f"{name}: every column needs a traction (body forces are out of scope)")
        V, ts, dss, _ = _multi_arguments(name, u, tractions, measures)
        om = self._check_omegas(name, omegas, V.n_cases)
        self._check_mass(name, density, mass_law)
        self._setup(u, rho, V.base, V.n_cases, ts, dss, E, nu, method, preconditioner, None)
        self.omegas, self.shifts = om, om * om
        self._set_mass(density, mass_law, rtol=1e-12)
        self.solve_counts = {"state": 0, "adjoint": 0}

    @staticmethod
    def _check_omegas(name: str, omegas, n: int) -> np.ndarray:
        if omegas is None:
            raise ValueError(f"{name}: one angular frequency per column (omegas)")
        om = _n_values(name, "frequencies omega", omegas, n)
        if not np.all(np.isfinite(om)) or np.any(om < 0.0):
            raise ValueError(f"{name}: the frequencies omega must be finite and >= 0")
        return om

    def assemble_vector(self, out: Optional[Vec] = None) -> Vec:
        """Column l: (K - omega_l^2 M) u_l - F_l; one launch for all columns (femo_elast_dyn_apply_multi)."""
        out = self._residual_buffer(out)
        return self.dynamic().dyn_apply_multi(self.n_cases, self.shifts, self.u.vec, out, a=1.0, b=-1.0, f=self.load())

    def partial_matrix(self, wrt: Function, out=None):
        if wrt is self.rho:
            return out if isinstance(out, _HarmonicDrho) else _HarmonicDrho(self)
        return super().partial_matrix(wrt, out)

    def _solve_columns(self, dev: DeviceElasticity, b: Vec, x: Vec, transpose: bool, **opts) -> list:
        """(K - omega_l^2 M) x_l = b_l for every column: ONE batched MINRES (the matrix is symmetric)."""
        return dev.dyn_solve_multi(self.n_cases, self.shifts, b, x, pc=self.preconditioner, **opts)


class DynamicCompliance(_StateOutput):
    """J = sum_l w_l |c_l|, or sum_l w_l c_l^2 with ``squared``, over the columns of a harmonic state, c_l = F_l . u_l the
    dynamic compliance of column l (w = 1 without ``weights``).  Below the first resonance c_l > 0; above it the response
    may be in antiphase with the load and c_l < 0, hence the absolute value (Ma, Kikuchi & Cheng 1995) or the square, which
    is smooth where c_l changes sign.  dJ/du_l = w_l sgn(c_l) F_l, or 2 w_l c_l F_l; the form has no partial in the density --
    the framework's adjoint solve (one batched MINRES) and dR/drho of `HarmonicElasticityResidual` give the total."""

    def __init__(self, u: Function, tractions, measures=None, weights=None, squared: bool = False):
        name = "DynamicCompliance"
        if any(t is None for t in list(tractions)):
            raise ValueError(f"{name}: every column needs a traction")
        V, self.tractions, self.measures, _ = _multi_arguments(name, u, tractions, measures)
        self.u, self.mesh, self.n_cases = u, V.mesh, V.n_cases
        self.weights = np.ones(V.n_cases) if weights is None else _n_values(name, "weights", weights, V.n_cases)
        self.squared = bool(squared)

    def load(self) -> Vec:
        """Column l = F_l, unweighted."""
        return _loads_vec(self.mesh, _facets_of(self.measures, self.tractions), self.tractions)

    def responses(self) -> np.ndarray:
        """c_l = F_l . u_l of the current state, all columns in one pass."""
        L = self.n_cases
        return np.diag(elasticity_handle(self.mesh).block_gram(L, self.load(), L, self.u.vec)).copy()

    def assemble_scalar(self) -> float:
        c = self.responses()
        return float(self.weights @ (c * c if self.squared else np.abs(c)))

    def _state_gradient(self, out: Vec) -> Vec:
        c = self.responses()
        coef = self.weights * (2.0 * c if self.squared else np.sign(c))
        return elasticity_handle(self.mesh).block_rotate(self.n_cases, np.diag(coef), self.load(), out)


# ------------------------------------------------------------------------------------ damped harmonic response ----
class DampedHarmonicElasticityMatrix(_UnsymmetricMatrix, MultiLoadElasticityMatrix):
    """dR/du of a `DampedHarmonicElasticityResidual` as the real operator on the 2L columns: [[A_l, -B_l], [B_l, A_l]] on
    the pair (2 l, 2 l + 1), A = K - omega^2 M, B = c_K K + c_M M -- not symmetric.  `mult` is Z, `multTranspose` conj(Z) (the
    transpose of the real operator); `backend_solve` is one batched COCR with Z (forward mode), `backend_solve_transpose`
    one with conj(Z) (the adjoint)."""

    def _apply(self, conj: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        dev = F.dynamic()
        return dev.cdyn_apply_multi(F.n_freq, F.shifts, F.ck, F.cm, x, y, conj=conj,
                                    masked=self.masked and dev.fixed_key is not None)

    def _solve(self, conj: bool, kind: str, b: Vec, x: Vec, options: Optional[dict]) -> None:
        self.info = self.form._matrix_solve(b, x, kind, options, transpose=conj)

    def to_scipy(self):
        import scipy.sparse as sp
        F = self.form
        K = F.dynamic().export_csr()
        M = _host_mass(F.mesh, np.array(F.rho.vec.get(), dtype=np.float64), F.mass_law, F.density)
        blocks, mask = [], self._host_mask()
        for sg, ck, cm in zip(F.shifts, F.ck, F.cm):
            A = _mask_host((K - sg * M).tocsr(), mask)
            B = _mask_host((ck * K + cm * M).tocsr(), mask, identity=False)
            blocks.append(sp.bmat([[A, -B], [B, A]], format="csr"))
        return sp.block_diag(blocks, format="csr")


class _DampedHarmonicDrho(_ElasticityDrho):
    """dR/drho of a `DampedHarmonicElasticityResidual`, matrix free: block l of column e is C'(rho_e) K0_e u_{l,e} (1 + i c_K)
    - density m'(rho_e) M0_e u_{l,e} (omega_l^2 - i c_M), split into its parts.  The stiffness and the mass launches of the
    undamped form on two rotated copies of the state: (1 + i c_K) u and (omega^2 - i c_M) u."""

    def __init__(self, form):
        super().__init__(form)
        self._uk = self._um = None
        self._key = None

    def _states(self):
        F = self.form
        key = (F.u.version, id(F.u.vec), tuple(F.shifts), tuple(F.ck), tuple(F.cm))
        if key != self._key:
            n2 = F.n_cases
            if self._uk is None:
                self._uk, self._um = Vec(_ctx(), n2 * F.n_dof), Vec(_ctx(), n2 * F.n_dof)
            QK, QM = np.zeros((n2, n2)), np.zeros((n2, n2))
            for l in range(F.n_freq):
                r, i = 2 * l, 2 * l + 1
                QK[r, r] = QK[i, i] = 1.0
                QK[i, r], QK[r, i] = -F.ck[l], F.ck[l]
                QM[r, r] = QM[i, i] = F.shifts[l]
                QM[i, r], QM[r, i] = F.cm[l], -F.cm[l]
            dev = F.device()
            dev.block_rotate(n2, QK, F.u.vec, self._uk)
            dev.block_rotate(n2, QM, F.u.vec, self._um)
            self._key = key
        return self._uk, self._um

    def _product(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        uk, um = self._states()
        dev = F.device()
        dev.drho_multi(F.method_id, transpose, F.n_cases, F.rho.vec, uk, x, y)
        return dev.mass_drho_multi(transpose, F.n_cases, -np.ones(F.n_cases), F.rho.vec, um, x, y, density=F.density,
                                   mass_law=F.mass_law, accumulate=True)


def _damped_arguments(name: str, u: Function, tractions, measures):
    """(V, L, tractions, measures) of a state of 2L real columns, the lists interleaved with None for the imaginary columns:
    the load of column 2 l is F_l, that of column 2 l + 1 zero."""
    V = u.function_space
    if not isinstance(V, LoadCaseSpace):
        raise NotImplementedError(f"{name} needs a Function(LoadCaseSpace(V, 2 n_frequencies)) state")
    if getattr(V.mesh, "local", None) is not None and V.mesh.local.nranks > 1:
        raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
    if V.n_cases % 2:
        raise ValueError(f"{name}: the state needs an even number of columns (Re and Im of every frequency), got {V.n_cases}")
    L = V.n_cases // 2
    if L > _lib.ELAST_MAX_COLS // 2:
        raise ValueError(f"{name}: {L} frequencies ({_lib.ELAST_MAX_COLS // 2} at the most)")
    tractions = list(tractions)
    measures = [None] * len(tractions) if measures is None else list(measures)
    if len(tractions) != L or len(measures) != L:
        raise ValueError(f"{name}: {L} frequencies need as many tractions and measures")
    if any(t is None for t in tractions):
        raise ValueError(f"{name}: every frequency needs a traction (body forces are out of scope)")
    ts, dss = [], []
    for t, ds in zip(tractions, measures):
        ds = ds if ds is not None else Measure("ds", domain=V.mesh)
        ts += [_traction(t, V.mesh), None]
        dss += [ds, ds]
    return V, L, ts, dss


class DampedHarmonicElasticityResidual(HarmonicElasticityResidual):
    """The damped harmonic response Z_l u_l = F_l in complex arithmetic,

        Z_l = K(rho) - omega_l^2 M(rho) + i (c_K,l K(rho) + c_M,l M(rho)),   c_K = loss_factor + omega beta,   c_M = omega alpha,

    with a structural ``loss_factor`` eta and Rayleigh damping ``rayleigh`` = (alpha, beta), C = alpha M + beta K.  ``u`` is a
    Function(LoadCaseSpace(V, 2L)): column 2 l is Re u_l, column 2 l + 1 is Im u_l; ``tractions``, ``measures`` and ``omegas``
    are per frequency, L <= 4 of them.  The residual is Z_l u_l - F_l split into its parts (the load is real).  K, M, the fixed
    set, the preconditioner, the load caches and the recording are those of `HarmonicElasticityResidual`.

    With damping the response is bounded at every frequency, and J of `DampedDynamicCompliance` is finite and differentiable
    across the resonances that an optimiser moves through the excitation frequencies.  The state solve, the forward-mode
    solve and the adjoint solve are each ONE batched preconditioned COCR (`DeviceElasticity.cdyn_solve_multi`; Sogabe &
    Zhang 2007), the adjoint with conj(Z), the transpose of the real operator: `KSP.solve` hands a transposed solve to
    `backend_solve_transpose`.  (A cached solver object of ``fea.linear_problem = True`` solves with the matrix itself and is
    not for this form.)  ``solve_counts`` has "state", "adjoint" and "forward".  dR/drho is matrix free, composed of the
    launches of the undamped form on two rotated copies of the state.

    Out of scope: frequency-band integrals, shifted preconditioners, viscous dampers at points, body forces, inhomogeneous
    supports, partitioned meshes."""
    matrix_class = DampedHarmonicElasticityMatrix
    is_symmetric = False
    _title, _solver, _kind = "damped harmonic elasticity", "COCR", "elasticity_damped_harmonic_"
    _residual, _count = "sqrt(Re(r^H M^-1 r))", "n_freq"

    def __init__(self, u: Function, rho: Function, tractions, measures=None, omegas=None, loss_factor: float = 0.0,
                 rayleigh=(0.0, 0.0), density: float = 1.0, mass_law: str = "linear", E: float = 1.0, nu: float = 0.3,
                 method: str = "SIMP", preconditioner: str = "jacobi", body_forces=None, thermal=None):
        name = "DampedHarmonicElasticityResidual"
        self._refuse_loads(name, body_forces, thermal)
        V, L, ts, dss = _damped_arguments(name, u, tractions, measures)
        om = self._check_omegas(name, omegas, L)
        damping = np.array([float(loss_factor)] + [float(v) for v in np.ravel(rayleigh)])
        if damping.size != 3 or not np.all(np.isfinite(damping)) or np.any(damping < 0.0):
            raise ValueError(f"{name}: the damping (loss_factor, rayleigh = (alpha, beta)) must be finite and >= 0")
        self._check_mass(name, density, mass_law)
        self._setup(u, rho, V.base, 2 * L, ts, dss, E, nu, method, preconditioner, None)
        self.n_freq = L
        self.loss_factor, self.rayleigh = float(damping[0]), (float(damping[1]), float(damping[2]))
        self.omegas = om
        self._set_mass(density, mass_law, rtol=1e-12)
        self.solve_counts = {"state": 0, "adjoint": 0, "forward": 0}

    @property
    def omegas(self) -> np.ndarray:
        return self._omegas

    @omegas.setter
    def omegas(self, om) -> None:
        """The shifts and the damping coefficients follow the frequencies."""
        self._omegas = np.array(om, dtype=np.float64)
        self.shifts = self._omegas * self._omegas
        self.ck = self.loss_factor + self._omegas * self.rayleigh[1]
        self.cm = self._omegas * self.rayleigh[0]

    def assemble_vector(self, out: Optional[Vec] = None) -> Vec:
        """Columns 2 l, 2 l + 1: Re and Im of Z_l u_l - F_l; one launch (femo_elast_cdyn_apply_multi)."""
        out = self._residual_buffer(out)
        return self.dynamic().cdyn_apply_multi(self.n_freq, self.shifts, self.ck, self.cm, self.u.vec, out, a=1.0, b=-1.0,
                                               f=self.load())

    def partial_matrix(self, wrt: Function, out=None):
        if wrt is self.rho:
            return out if isinstance(out, _DampedHarmonicDrho) else _DampedHarmonicDrho(self)
        return MultiLoadElasticityResidual.partial_matrix(self, wrt, out)

    def _solve_columns(self, dev: DeviceElasticity, b: Vec, x: Vec, transpose: bool, **opts) -> list:
        """Z_l x_l = b_l for every frequency, or with ``transpose`` conj(Z_l) x_l = b_l: ONE batched COCR."""
        return dev.cdyn_solve_multi(self.n_freq, self.shifts, self.ck, self.cm, b, x, conj=transpose, pc=self.preconditioner,
                                    **opts)


class DampedDynamicCompliance(_StateOutput):
    """J = sum_l w_l |c_l|, or sum_l w_l |c_l|^2 with ``squared``, over the frequencies of a damped harmonic state, c_l =
    F_l . u_l the complex dynamic compliance (unconjugated; the load is real).  dJ/du: the real column of frequency l is
    w_l (Re c_l / |c_l|) F_l and the imaginary one w_l (Im c_l / |c_l|) F_l; 2 w_l Re c_l F_l and 2 w_l Im c_l F_l for the square.
    No partial in the density: the adjoint solve (one batched COCR with conj(Z)) and dR/drho of
    `DampedHarmonicElasticityResidual` give the total,
    dJ/drho = sum_l w_l Re(conj(c_l) / |c_l| dc_l/drho), dc_l/drho_e = -u_e^T [C'(rho_e) K0_e (1 + i c_K) - density m'(rho_e) M0_e
    (omega_l^2 - i c_M)] u_e."""

    def __init__(self, u: Function, tractions, measures=None, weights=None, squared: bool = False):
        name = "DampedDynamicCompliance"
        V, L, self.tractions, self.measures = _damped_arguments(name, u, tractions, measures)
        self.u, self.mesh, self.n_cases, self.n_freq = u, V.mesh, V.n_cases, L
        self.weights = np.ones(L) if weights is None else _n_values(name, "weights", weights, L)
        self.squared = bool(squared)

    def load(self) -> Vec:
        """Column 2 l = F_l, unweighted; column 2 l + 1 = 0."""
        return _loads_vec(self.mesh, _facets_of(self.measures, self.tractions), self.tractions)

    def responses(self) -> np.ndarray:
        """The complex c_l = F_l . u_l of the current state, all frequencies in one pass."""
        n2 = self.n_cases
        G = elasticity_handle(self.mesh).block_gram(n2, self.load(), n2, self.u.vec)
        r = 2 * np.arange(self.n_freq)
        return G[r, r] + 1j * G[r, r + 1]

    def assemble_scalar(self) -> float:
        a = np.abs(self.responses())
        return float(self.weights @ (a * a if self.squared else a))

    def _state_gradient(self, out: Vec) -> Vec:
        c = self.responses()
        a = np.abs(c)
        coef = self.weights * (2.0 * c if self.squared else np.where(a > 0.0, c / np.where(a > 0.0, a, 1.0), 0.0))
        Q = np.zeros((self.n_cases, self.n_cases))
        r = 2 * np.arange(self.n_freq)
        Q[r, r], Q[r, r + 1] = coef.real, coef.imag
        return elasticity_handle(self.mesh).block_rotate(self.n_cases, Q, self.load(), out)


# ------------------------------------------------------------------------------------------ transient response ----
class TransientElasticityMatrix(_UnsymmetricMatrix):
    """dR/dU of a `TransientElasticityResidual`: the block lower-banded, block-Toeplitz L of the Newmark recurrence on the
    history -- not symmetric, but with symmetric blocks, so `backend_solve_transpose` (the adjoint) is the march of
    `backend_solve` (forward mode) run from the last step to the first.  With ``masked`` the diagonal blocks carry identity
    rows / columns on the fixed dofs and the sub-diagonal blocks zero ones.  `mult` / `multTranspose` are the banded product,
    8 time steps per launch."""

    def getSizes(self):
        n = self.form.n_steps * self.form.n_dof
        return (n, n)

    size = property(getSizes)

    def _apply(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        dev = F.dynamic()
        return dev.newmark_apply(F.params, F.n_steps, x, y, transpose=transpose,
                                 masked=self.masked and dev.fixed_key is not None)

    def _solve(self, reverse: bool, kind: str, b: Vec, x: Vec, options: Optional[dict]) -> None:
        o = options or {}
        F = self.form
        infos, stopped = F.dynamic().newmark_march(F.params, F.n_steps, x, rhs=b, reverse=reverse, extrapolate=F.extrapolate,
                                                   rtol=o.get("elast_rtol", F.rtol), max_it=o.get("elast_max_it", F.max_it),
                                                   pc=F.preconditioner)
        self.info = F._record((infos, stopped), kind)

    def to_scipy(self):
        import scipy.sparse as sp
        F = self.form
        K = F.dynamic().export_csr()
        M = _host_mass(F.mesh, np.array(F.rho.vec.get(), dtype=np.float64), F.mass_law, F.density)
        A = [_mask_host((m * M + k * K).tocsr(), self._host_mask(), identity=j == 0)        # ones on the diagonal blocks only
             for j, (m, k) in enumerate(zip(F.blocks["m"], F.blocks["k"]))]
        N = F.n_steps
        sub = lambda k: sp.csr_matrix((np.ones(max(N - k, 0)), (np.arange(k, N), np.arange(0, max(N - k, 0)))), shape=(N, N))
        return (sp.kron(sp.identity(N), A[0]) + sp.kron(sub(1), A[1]) + sp.kron(sub(2), A[2])).tocsr()


class _TransientDrho(_ElasticityDrho):
    """dR/drho of a `TransientElasticityResidual` ((n_steps n_dof) x n_cell), matrix free: block t of column e is C'(rho_e) K0_e
    uK_t,e + density m'(rho_e) M0_e uM_t,e with the banded combinations uK_t = sum_j k_j u_{t+j}, uM_t = sum_j m_j u_{t+j}; the
    existing batched products in windows of 8 time steps, in ascending order."""

    def getSizes(self):
        return (self.form.n_steps * self.form.n_dof, self.mesh.n_cell)

    def _product(self, transpose: bool, x: Vec, y: Vec) -> Vec:
        F = self.form
        return F.device().newmark_drho(F.params, F.method_id, transpose, F.n_steps, F.rho.vec, F.u.vec, x, y, density=F.density,
                                       mass_law=F.mass_law)


def _transient_space(name: str, u: Function) -> TimeHistorySpace:
    V = u.function_space
    if not isinstance(V, TimeHistorySpace):
        raise NotImplementedError(f"{name} needs a Function(TimeHistorySpace(V, n_steps)) state")
    if getattr(V.mesh, "local", None) is not None and V.mesh.local.nranks > 1:
        raise NotImplementedError(f"{name}: partitioned meshes are out of scope")
    return V


class TransientElasticityResidual(_MassCarrying, ElasticityResidual):
    """The time-domain response M u'' + C u' + K(rho) u = g(t) F from rest, C = c_m M + c_k K (``rayleigh`` = (c_m, c_k)), by
    Newmark(``beta``, ``gamma``) with the step ``dt``, written as its two-step recurrence in the displacements:

        A1 u_{n+1} + A0 u_n + A- u_{n-1} = dt^2 (beta g_{n+1} + b0 g_n + b- g_{n-1}) F,   A_j = m_j M + k_j K,   n = 0 ... N - 1

    (the scalars in csrc/elast_transient.hip; u_0 = u_-1 = 0, g_-1 = 0).  ``u`` is a Function(TimeHistorySpace(V, N)) holding
    u_1 ... u_N; ``traction`` on ``ds`` is the one spatial load pattern F, ``signal`` the N + 1 samples g_0 ... g_N of its time
    signal; M = ``density`` sum_e m(rho_e) M0_e as for `HarmonicElasticityResidual`, reassembled under the same rule.

    The residual of the whole history is R = L U - B with L block lower-banded and block-Toeplitz with symmetric blocks:
    L^T is the same march on the time-reversed sequence.  The state solve, the forward-mode solve (`backend_solve` of
    `new_matrix()`) and the adjoint solve (`backend_solve_transpose`) are ONE device-resident loop
    (`DeviceElasticity.newmark_march`): per step one fused right-hand-side launch and one PCG on K + (m1 / k1) M with the
    block-Jacobi (diagonal blocks of K + (m1 / k1) M) or multilevel preconditioner, from the extrapolated first guess
    2 u_n - u_{n-1} (``extrapolate``, on by default).  The guess buys accuracy, not speed: the PCG stops relative to the residual
    of its first guess, so a better guess lowers the level it stops at and leaves the iteration count where it was (measured:
    1-6 % more iterations, a lower error).  A step that does not converge raises, naming the step.

    Refused: beta <= 0, gamma < 1/2, partitioned meshes, inhomogeneous supports, body forces, n_steps < 1,
    len(signal) != n_steps + 1, non-finite inputs.  Out of scope: several load patterns in one march, non-zero initial
    conditions, checkpointing, HHT-alpha and generalised-alpha, point dampers."""
    matrix_class = TransientElasticityMatrix
    is_symmetric = False
    _supports_name = "TransientElasticityResidual"

    def __init__(self, u: Function, rho: Function, traction, ds: Optional[Measure] = None, signal=None, dt: float = None,
                 beta: float = 0.25, gamma: float = 0.5, rayleigh=(0.0, 0.0), density: float = 1.0, mass_law: str = "linear",
                 E: float = 1.0, nu: float = 0.3, method: str = "SIMP", preconditioner: str = "jacobi", body_force=None,
                 thermal=None):
        name = "TransientElasticityResidual"
        self._refuse_loads(name, body_force, thermal)
        V = _transient_space(name, u)
        if traction is None:
            raise ValueError(f"{name}: the load pattern needs a traction (body forces are out of scope)")
        self.t = _traction(traction, V.mesh)
        self.ds = ds if ds is not None else Measure("ds", domain=V.mesh)
        if signal is None:
            raise ValueError(f"{name}: the time signal needs n_steps + 1 samples (signal)")
        g = np.array(signal, dtype=np.float64).ravel()
        if g.size != V.n_steps + 1:
            raise ValueError(f"{name}: {V.n_steps} steps need {V.n_steps + 1} samples of the signal, got {g.size}")
        if not np.all(np.isfinite(g)):
            raise ValueError(f"{name}: the signal must be finite")
        if dt is None or not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"{name}: the time step dt must be finite and > 0")
        if not (np.isfinite(beta) and beta > 0.0):
            raise ValueError(f"{name}: beta must be finite and > 0 (the step matrix must be positive definite)")
        if not (np.isfinite(gamma) and gamma >= 0.5):
            raise ValueError(f"{name}: gamma must be finite and >= 1/2")
        ray = np.array(rayleigh, dtype=np.float64).ravel()
        if ray.size != 2 or not np.all(np.isfinite(ray)) or np.any(ray < 0.0):
            raise ValueError(f"{name}: rayleigh = (c_m, c_k) must be two finite values >= 0")
        self._check_mass(name, density, mass_law)
        self._setup(u, rho, V.base, 1, [self.t], [self.ds], E, nu, method, preconditioner, None)
        self.n_steps, self.signal = V.n_steps, g
        self.dt, self.beta, self.gamma, self.rayleigh = float(dt), float(beta), float(gamma), (float(ray[0]), float(ray[1]))
        self.params = (self.dt, self.beta, self.gamma, self.rayleigh[0], self.rayleigh[1])
        dt2 = self.dt * self.dt
        b0, bm = 0.5 + self.gamma - 2.0 * self.beta, 0.5 - self.gamma + self.beta
        cm, ck = self.rayleigh
        self.blocks = dict(m=(1.0 + self.gamma * self.dt * cm, -2.0 + (1.0 - 2.0 * self.gamma) * self.dt * cm,
                              1.0 - (1.0 - self.gamma) * self.dt * cm),
                           k=(self.gamma * self.dt * ck + self.beta * dt2, (1.0 - 2.0 * self.gamma) * self.dt * ck + b0 * dt2,
                              -(1.0 - self.gamma) * self.dt * ck + bm * dt2), b0=b0, bm=bm)
        self._set_mass(density, mass_law, rtol=1e-13)
        self.extrapolate = True
        self.solve_counts = {"state": 0, "adjoint": 0, "forward": 0}
        self._B = None

    def signal_coefficients(self) -> np.ndarray:
        """(n_steps,): dt^2 (beta g_{t+1} + b0 g_t + b- g_{t-1}), the factor of F in the right-hand side of step t."""
        g = self.signal
        gm = np.concatenate([[0.0], g[:-2]])
        return self.dt ** 2 * (self.beta * g[1:] + self.blocks["b0"] * g[:-1] + self.blocks["bm"] * gm)

    def assemble_vector(self, out: Optional[Vec] = None) -> Vec:
        """R = L U - B of the whole history, without any Dirichlet treatment: the banded product and one launch for B."""
        n = self.n_steps * self.n_dof
        out = self._residual_buffer(out, n)
        dev = self.dynamic()
        if self._B is None:
            self._B = Vec(_ctx(), n)
        dev.newmark_outer(self.n_steps, self.signal_coefficients(), self.load(), self._B)
        dev.newmark_apply(self.params, self.n_steps, self.u.vec, out)
        return out.axpy(-1.0, self._B)

    def partial_matrix(self, wrt: Function, out=None):
        if wrt is self.rho:
            return out if isinstance(out, _TransientDrho) else _TransientDrho(self)
        return super().partial_matrix(wrt, out)

    def solve_state(self, func: Function, bcs, report: bool = False) -> None:
        """The whole history in one call: N steps on the device, each one fused right-hand side and one PCG."""
        self._set_bcs(bcs)
        dev = self.dynamic()
        out = dev.newmark_march(self.params, self.n_steps, func.vec, F=self.load(), signal=self.signal,
                                extrapolate=self.extrapolate, rtol=self.rtol, max_it=self.max_it, pc=self.preconditioner)
        func.version += 1
        self._record(out, "state")
        if report:
            print(self._report(out))

    def _record(self, out, kind: str):
        """`ElasticityResidual._record` for a march: ``out`` = (one record per step, the step it stopped at or -1)."""
        from .utils_hip import LAST_KSP_INFO
        infos, stopped = out
        taken = [i for i in infos if i.iterations > 0 or i.converged != 0]
        self.solve_counts[kind] = self.solve_counts.get(kind, 0) + 1
        self.last_info[kind] = dict(n_steps=self.n_steps, iterations=[i.iterations for i in infos],
                                    converged=[i.converged for i in infos], stopped_at=stopped,
                                    solve_ms=float(sum(i.solve_ms for i in taken)), preconditioner=self.preconditioner)
        LAST_KSP_INFO.append(dict(self.last_info[kind], kind="elasticity_transient_" + kind))
        if stopped >= 0:
            i = infos[stopped]
            raise RuntimeError(f"transient elasticity PCG did not converge ({kind}, step {stopped} of {self.n_steps}): "
                               f"{i.iterations} iterations, sqrt(r.M^-1 r) = {i.residual_norm:.3e} of {i.rhs_norm:.3e}; the later "
                               f"steps were not taken")
        return infos

    def _report(self, out) -> str:
        infos = out[0]
        its = [i.iterations for i in infos]
        return (f"transient elasticity march, {self.n_steps} steps: {sum(its)} PCG iterations ({min(its)} to {max(its)} per step), "
                f"{sum(i.solve_ms for i in infos):.1f} ms in the solves")


class TransientCompliance(_StateOutput):
    """J = sum_n w_n c_n, or sum_n w_n c_n^2 with ``squared``, over the steps of a transient state, c_n = F . u_n the work of
    the load pattern on step n (n = 1 ... N).  Without ``weights`` they are ``dt`` each -- the rectangle rule of int F . u dt --
    and ``dt``, the time step of the residual, must be given: the state's space does not know it.  dJ/du_n = w_n F or 2 w_n c_n F; the form has no partial in the density -- the reversed
    march of `TransientElasticityResidual` and its dR/drho give the total."""

    def __init__(self, u: Function, traction, ds: Optional[Measure] = None, weights=None, squared: bool = False,
                 dt: Optional[float] = None):
        name = "TransientCompliance"
        V = _transient_space(name, u)
        if traction is None:
            raise ValueError(f"{name}: the load pattern needs a traction")
        self.t = _traction(traction, V.mesh)
        self.ds = ds if ds is not None else Measure("ds", domain=V.mesh)
        self.u, self.mesh, self.n_steps = u, V.mesh, V.n_steps
        if weights is None:
            if dt is None or not (np.isfinite(dt) and dt > 0.0):
                raise ValueError(f"{name}: without weights the default w_n = dt needs the time step dt")
            self.weights = np.full(V.n_steps, float(dt))
        else:
            self.weights = np.array(weights, dtype=np.float64).ravel()
            if self.weights.size != V.n_steps or not np.all(np.isfinite(self.weights)):
                raise ValueError(f"{name}: {V.n_steps} steps need as many finite weights")
        self.squared = bool(squared)

    def load(self) -> Vec:
        return _load_vec(self.mesh, self.ds.facets(), self.t)

    def responses(self) -> np.ndarray:
        """c_n = F . u_n of the current history, through the Gram kernel in windows of 8 steps."""
        return elasticity_handle(self.mesh).newmark_dots(self.n_steps, self.load(), self.u.vec)

    def assemble_scalar(self) -> float:
        c = self.responses()
        return float(self.weights @ (c * c if self.squared else c))

    def _state_gradient(self, out: Vec) -> Vec:
        coef = self.weights * (2.0 * self.responses() if self.squared else 1.0)
        return elasticity_handle(self.mesh).newmark_outer(self.n_steps, coef, self.load(), out)


def averageFunc(func: Function) -> LinearFunctional:
    """(1/|Omega|) int func dx for a DG0 Function (averageFunc, run_topo_opt_cantilever_beam.py:103-106)."""
    V = func.function_space
    if V.family != "DG":
        raise NotImplementedError("averageFunc needs a DG0 Function")
    vol = cell_volumes(V.mesh)
    coeff = Function(FunctionSpace(V.mesh, ("DG", 0)))
    coeff.vector[:] = vol / vol.sum()
    return LinearFunctional(coeff, func)


# ---------------------------------------------------------------------------- builders of the run script (:85-109) ----
def pdeRes(u, v, rho_e, f, E: float = 1.0, dss: Optional[Measure] = None, method: str = "SIMP",
           preconditioner: str = "jacobi", body_force=None, springs=None, point_load=None,
           thermal: Optional[ThermalExpansion] = None) -> ElasticityResidual:
    """run_topo_opt_cantilever_beam.py:85-101 (nu = 0.3 as there); ``v`` is implied by the catalogue.  ``body_force``: the
    self-weight rho b dx (not in the reference's script); ``f`` may then be None.  ``springs``: elastic supports, one
    stiffness per dof (`point_springs`, `facet_springs`), and ``point_load``: nodal forces, one value per dof (a port's input
    force, built like `port_displacement`); neither is in the reference's script.  ``thermal``: the thermal expansion load
    of a `ThermalExpansion`; ``f`` may then be None."""
    return ElasticityResidual(u, rho_e, f, dss, E=E, nu=0.3, method=method, preconditioner=preconditioner,
                              body_force=body_force, springs=springs, point_load=point_load, thermal=thermal)


def compliance(u, f, dss: Optional[Measure] = None, body_force=None, rho_e=None, thermal: Optional[ThermalExpansion] = None,
               E: float = 1.0, method: str = "SIMP") -> Compliance:
    """run_topo_opt_cantilever_beam.py:108-109; with ``body_force`` or ``thermal`` (and the density ``rho_e``) the work of the
    total load; ``E`` and ``method`` are those of `pdeRes` (read by the thermal load alone)."""
    return Compliance(u, f, dss, body_force=body_force, rho=rho_e, thermal=thermal, E=E, nu=0.3, method=method)


def pdeRes_multiload(u, v, rho_e, fs, dss_list=None, E: float = 1.0, method: str = "SIMP",
                     preconditioner: str = "jacobi", body_forces=None, springs=None,
                     thermal: Optional[ThermalExpansion] = None) -> MultiLoadElasticityResidual:
    """`pdeRes` for the load cases ``fs[l]`` on ``dss_list[l]`` with the body forces ``body_forces[l]`` (None = none) and
    the elastic supports ``springs`` (the same for every load case) and the thermal load ``thermal`` (one temperature, one
    scale per load case); ``u`` is a Function(LoadCaseSpace(V, len(fs)))."""
    return MultiLoadElasticityResidual(u, rho_e, fs, dss_list, E=E, nu=0.3, method=method, preconditioner=preconditioner,
                                       body_forces=body_forces, springs=springs, thermal=thermal)


def displacement(u, ell, weights=None) -> ElasticityDisplacement:
    """sum_l w_l l_l . u_l as a scalar output (`port_displacement`, `mean_displacement` build l)."""
    return ElasticityDisplacement(u, ell, weights=weights)


def pnorm_displacement(u, region=None, m=1.0, p: float = 8.0, weights=None) -> ElasticityPnormDisplacement:
    """The aggregated nodal displacement of a region as a scalar output."""
    return ElasticityPnormDisplacement(u, region, m=m, p=p, weights=weights)


def compliance_multiload(u, fs, dss_list=None, weights=None, body_forces=None, rho_e=None,
                         thermal: Optional[ThermalExpansion] = None, E: float = 1.0, method: str = "SIMP") -> MultiLoadCompliance:
    """sum_l w_l F_l . u_l with F_l = int_ds(l) f_l . v ds + the body load of ``body_forces[l]`` + the thermal load of
    ``thermal`` (either needs ``rho_e``; ``E`` and ``method`` as for `compliance`)"""
    return MultiLoadCompliance(u, fs, dss_list, weights, body_forces=body_forces, rho=rho_e, thermal=thermal, E=E, nu=0.3,
                               method=method)


def pdeRes_harmonic(u, v, rho_e, fs, dss_list=None, omegas=None, density: float = 1.0, mass_law: str = "linear", E: float = 1.0,
                    method: str = "SIMP", preconditioner: str = "jacobi") -> HarmonicElasticityResidual:
    """`pdeRes_multiload` for the harmonic loads ``fs[l]`` cos(omegas[l] t) on ``dss_list[l]`` (nu = 0.3 as there); ``u`` is a
    Function(LoadCaseSpace(V, len(fs)))."""
    return HarmonicElasticityResidual(u, rho_e, fs, dss_list, omegas=omegas, density=density, mass_law=mass_law, E=E, nu=0.3,
                                      method=method, preconditioner=preconditioner)


def dynamic_compliance(u, fs, dss_list=None, weights=None, squared: bool = False) -> DynamicCompliance:
    """sum_l w_l |F_l . u_l| (or its squared form) of a harmonic state as a scalar output."""
    return DynamicCompliance(u, fs, dss_list, weights=weights, squared=squared)


def pdeRes_harmonic_damped(u, v, rho_e, fs, dss_list=None, omegas=None, loss_factor: float = 0.0, rayleigh=(0.0, 0.0),
                           density: float = 1.0, mass_law: str = "linear", E: float = 1.0, method: str = "SIMP",
                           preconditioner: str = "jacobi") -> DampedHarmonicElasticityResidual:
    """`pdeRes_harmonic` with a structural loss factor and Rayleigh damping (alpha, beta); ``u`` is a
    Function(LoadCaseSpace(V, 2 len(fs))): Re and Im of every frequency."""
    return DampedHarmonicElasticityResidual(u, rho_e, fs, dss_list, omegas=omegas, loss_factor=loss_factor, rayleigh=rayleigh,
                                            density=density, mass_law=mass_law, E=E, nu=0.3, method=method,
                                            preconditioner=preconditioner)


def dynamic_compliance_damped(u, fs, dss_list=None, weights=None, squared: bool = False) -> DampedDynamicCompliance:
    """sum_l w_l |F_l . u_l| (or its squared form) of a damped harmonic state, c_l complex, as a scalar output."""
    return DampedDynamicCompliance(u, fs, dss_list, weights=weights, squared=squared)


def pdeRes_transient(u, v, rho_e, f, dss: Optional[Measure] = None, signal=None, dt: float = None, beta: float = 0.25,
                     gamma: float = 0.5, rayleigh=(0.0, 0.0), density: float = 1.0, mass_law: str = "linear", E: float = 1.0,
                     method: str = "SIMP", preconditioner: str = "jacobi") -> TransientElasticityResidual:
    """`pdeRes` in the time domain: the Newmark march under the load pattern ``f`` on ``dss`` with the time signal ``signal``
    (nu = 0.3 as there); ``u`` is a Function(TimeHistorySpace(V, len(signal) - 1))."""
    return TransientElasticityResidual(u, rho_e, f, dss, signal=signal, dt=dt, beta=beta, gamma=gamma, rayleigh=rayleigh,
                                       density=density, mass_law=mass_law, E=E, nu=0.3, method=method,
                                       preconditioner=preconditioner)


def transient_compliance(u, f, dss: Optional[Measure] = None, weights=None, squared: bool = False,
                         dt: Optional[float] = None) -> TransientCompliance:
    """sum_n w_n F . u_n (or its squared form) of a transient state as a scalar output; without ``weights`` w_n = ``dt``, the
    time step given to `pdeRes_transient`."""
    return TransientCompliance(u, f, dss, weights=weights, squared=squared, dt=dt)


def pnorm_stress(u, rho_e, E: float = 1.0, nu: float = 0.3, m: float = 1.0, p: float = 8.0, q: float = 0.5,
                 alpha: Optional[float] = None) -> ElasticityPnormStress:
    """The aggregated von Mises stress as a scalar output, named after the shell's builder (shell_pde.py:297-313)."""
    return ElasticityPnormStress(u, rho_e, E=E, nu=nu, m=m, p=p, q=q, alpha=alpha)


def von_Mises_stress(u, rho_e=None, E: float = 1.0, nu: float = 0.3, q: float = 0.0) -> ElasticityVonMises:
    """The (relaxed) von Mises stress as a field output."""
    return ElasticityVonMises(u, rho_e, E=E, nu=nu, q=q)


def pnorm_stress_multiload(u, rho_e, E: float = 1.0, nu: float = 0.3, m=1.0, p: float = 8.0, q: float = 0.5,
                           alpha: Optional[float] = None, weights=None) -> MultiLoadPnormStress:
    """`pnorm_stress` over the load cases of a Function(LoadCaseSpace(V, L)): sum_l w_l J_l with one scale m_l per load case."""
    return MultiLoadPnormStress(u, rho_e, E=E, nu=nu, m=m, p=p, q=q, alpha=alpha, weights=weights)


def von_Mises_stress_multiload(u, rho_e=None, E: float = 1.0, nu: float = 0.3, q: float = 0.0, scales=None,
                               load_case: Optional[int] = None) -> MultiLoadVonMises:
    """The envelope of the (relaxed) von Mises stress over the load cases, or the field of one load case, as a field output."""
    return MultiLoadVonMises(u, rho_e, E=E, nu=nu, q=q, scales=scales, load_case=load_case)


def eigenvalue_aggregate(rho_e, V, bcs, n_modes: int = 3, p: float = 8.0, block: Optional[int] = None, E: float = 1.0,
                         nu: float = 0.3, method: str = "SIMP", density: float = 1.0, mass_law: str = "linear",
                         preconditioner: str = "jacobi", rtol: float = 1e-9, seed: int = 0) -> EigenvalueAggregate:
    """The smooth lower bound of the fundamental eigenvalue as a scalar output of the density:
    ``fea.add_output(name, 'scalar', eigenvalue_aggregate(rho_e, V, bcs, n_modes=3), ['density'])``."""
    return EigenvalueAggregate(ElasticityEigenvalues(rho_e, V, bcs, n_modes, block=block, E=E, nu=nu, method=method,
                                                     density=density, mass_law=mass_law, preconditioner=preconditioner,
                                                     rtol=rtol, seed=seed), p=p)


def buckling_aggregate(residual: ElasticityResidual, n_modes: int = 2, p: float = 8.0, block: Optional[int] = None,
                       rtol: float = 1e-9, seed: int = 0) -> BucklingAggregate:
    """The smooth lower bound of the critical buckling load factor of the state of ``residual`` as a scalar output:
    ``fea.add_output('buckling', 'scalar', buckling_aggregate(res), ['u', 'density'])`` with
    ``fea.consistent_bc_partials = True``."""
    return BucklingAggregate(ElasticityBuckling(residual, n_modes, block=block, rtol=rtol, seed=seed), p=p)
