"""Method of Moving Asymptotes on the device: ``DeviceMMA`` binds the handle of csrc/mma.hip (include/femo_hip.h states the
formulation), ``MMA`` drives a ``CSDLProblem`` with it -- ``Simulator.run``, one ``compute_totals`` per output, one update.

``BetaContinuation`` is the continuation schedule on the sharpness of the Heaviside projection
(csdl_opt/filter_model.py: ProjectedFilterOperation, csrc/project.hip), which is also where passive cells enter the loop: the
projection fixes their density and zeroes their Jacobian rows, while ``CSDLProblem`` and the handle still refuse xmax = xmin.

Out of scope: GCMMA's inner conservative loop, equality constraints, several design-variable vectors, more than 8 rows,
partitioned meshes, continuation on the SIMP exponent or the filter radius, an OC update."""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict, List, Optional

import numpy as np

from .. import _lib
from ..engine import DeviceArray, Vec
from .problem import CSDLProblem

MAX_M = _lib.MMA_MAX_M
_GET = dict(L=0, U=1, alfa=2, beta=3, p=4, q=5, b=6, bsum=7, xsi=8, eta=9)


def _check(rc: int) -> None:
    """The library's error path; an input it refused (rc 2) is a ValueError."""
    if rc == 0:
        return
    msg = _lib.load().femo_last_error()
    msg = msg.decode() if msg else f"libfemo_hip error {rc}"
    if rc == 2:
        raise ValueError(msg)
    raise _lib.FemoError(msg)


def _check_params(m: int, move: float, sub_tol: float) -> None:
    if not 0 <= int(m) <= MAX_M:
        raise ValueError(f"MMA: {m} constraint rows, supported: 0 to {MAX_M}")
    if not (np.isfinite(move) and move > 0.0):
        raise ValueError(f"MMA: move = {move}, must be positive")
    if not 0.0 < sub_tol <= 1.0:
        raise ValueError(f"MMA: sub_tol = {sub_tol}, must lie in (0, 1]")


def _info(info: _lib.MmaInfo, m: int) -> Dict:
    out = {k: getattr(info, k) for k, _ in _lib.MmaInfo._fields_ if k not in ("lam", "y")}
    out["lam"] = np.array(info.lam[:m])
    out["y"] = np.array(info.y[:m])
    return out


class DeviceMMA:
    """n variables in the box [xmin, xmax] (device vectors, copied), m rows f_i(x) <= 0."""

    def __init__(self, ctx, xmin: Vec, xmax: Vec, m: int, move: float = 0.5, sub_tol: float = 1e-7, c=1000.0, d=1.0,
                 n: Optional[int] = None):
        _check_params(m, move, sub_tol)
        self.ctx, self.lib = ctx, ctx.lib
        self.n, self.m = int(xmin.n if n is None else n), int(m)
        par = _lib.MmaParams(move=float(move), sub_tol=float(sub_tol))
        cc, dd = np.broadcast_to(np.asarray(c, float), (self.m,)), np.broadcast_to(np.asarray(d, float), (self.m,))
        for i in range(MAX_M):
            par.c[i], par.d[i] = (cc[i], dd[i]) if i < self.m else (1000.0, 1.0)
        h = _lib.H()
        _check(self.lib.femo_mma_create(ctx.handle, self.n, self.m, xmin.handle, xmax.handle, C.byref(par), C.byref(h)))
        self.handle = h

    def update(self, x: Vec, f0: float, df0: Vec, f=(), df: Optional[Vec] = None) -> Dict:
        """x <- x^{k+1} in place.  f: the m row values; df: their gradients, m stacked columns of n entries."""
        fv = np.ascontiguousarray(np.asarray(f, dtype=np.float64).ravel())
        if fv.size != self.m or (self.m > 0 and df is None):
            raise ValueError(f"MMA: {self.m} rows need {self.m} values and their gradients")
        info = _lib.MmaInfo()
        _check(self.lib.femo_mma_update(self.handle, x.handle, float(f0), df0.handle, fv.ctypes.data_as(_lib.c_f64p),
                                        df.handle if self.m > 0 else None, C.byref(info)))
        return _info(info, self.m)

    def reset(self) -> None:
        _check(self.lib.femo_mma_reset(self.handle))

    def get(self, what: str, i: int = 0) -> np.ndarray:
        """L, U, alfa, beta, p (row i), q (row i), b, bsum, xsi, eta of the last step (include/femo_hip_test.h; tests)."""
        out = np.empty(self.m if what in ("b", "bsum") else self.n)
        _check(self.lib.femo_mma_get(self.handle, _GET[what], int(i), C.c_void_p(out.ctypes.data)))
        return out

    def solve_subproblem(self, L, U, alfa, beta, p, q, b):
        """One subproblem from host arrays (include/femo_hip_test.h; tests): x and a record like mma_ref.subsolve's."""
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (L, U, alfa, beta, p, q, b)]
        assert a[4].shape == a[5].shape == (self.m + 1, self.n) and a[6].size == self.m
        x, xsi, eta, small = np.empty(self.n), np.empty(self.n), np.empty(self.n), np.empty(4 * max(self.m, 1))
        info = _lib.MmaInfo()
        ptr = [C.c_void_p(v.ctypes.data) for v in a + [x, xsi, eta, small]]
        _check(self.lib.femo_mma_solve_subproblem(self.handle, *ptr, C.byref(info)))
        m = self.m
        rec = _info(info, m)
        rec.update(y=small[:m], lam=small[m:2 * m], mu=small[2 * m:3 * m], s=small[3 * m:4 * m], xsi=xsi, eta=eta,
                   newton=rec["newton_steps"])
        return x, rec

    def __del__(self):
        try:
            h, self.handle = getattr(self, "handle", None), None
            if h and getattr(self.ctx, "handle", None):
                self.lib.femo_mma_destroy(h)
        except Exception:
            pass


class BetaContinuation:
    """Continuation on the projection's sharpness: stage s runs with ``op.beta = betas[s]`` and ends after ``every`` design
    steps, or earlier when the driver's ``tol > 0`` and the step's max_dx_rel <= tol.  At a stage's end ``op.beta`` takes the
    next value and the driver restarts the asymptote history (``handle.reset()``); the loop may stop on ``tol`` only in the
    last stage.  ``op`` is anything with a settable ``beta`` (a ProjectedFilterOperation)."""

    def __init__(self, op, betas, every: int):
        self.op = op
        self.betas = [float(b) for b in betas]
        self.every = int(every)
        if not self.betas or any(not (np.isfinite(b) and b >= 0.0) for b in self.betas):
            raise ValueError(f"BetaContinuation: betas = {betas}, need at least one finite value >= 0")
        if self.every < 1:
            raise ValueError(f"BetaContinuation: every = {every}, must be at least 1")
        self.stage, self.steps_in_stage = 0, 0

    @property
    def last_stage(self) -> bool:
        return self.stage == len(self.betas) - 1

    def start(self) -> None:
        self.stage, self.steps_in_stage = 0, 0
        self.op.beta = self.betas[0]

    def after_step(self, max_dx_rel: float, tol: float) -> str:
        """Called once per design step: ``'stop'`` (tol met in the last stage), ``'advance'`` (beta took its next value: the
        caller resets the optimiser's history) or ``'go'``."""
        self.steps_in_stage += 1
        small = tol > 0.0 and max_dx_rel <= tol
        if self.last_stage:
            return 'stop' if small else 'go'
        if small or self.steps_in_stage >= self.every:
            self.stage += 1
            self.steps_in_stage = 0
            self.op.beta = self.betas[self.stage]
            return 'advance'
        return 'go'


class MMA:
    """Minimise the problem's objective under its rows with the device-resident MMA update.

    The objective is ``scaler * J``; with ``normalize`` (the default) it is divided by ``|scaler * J(x^1)|``, because the
    subproblem's constants c_i = 1000 presume an objective of order one -- an objective of order 1e4 would make violating
    a constraint cheaper than it should be.  Each step runs ``sim.run()``, one ``sim.compute_totals`` for the objective and
    one per constrained output, and one update; with ``Simulator(device=True)`` the design and the gradients stay in HBM
    (only function values and the sums of the subproblem's m x m system cross the link), in host mode they are uploaded.
    Stops after ``max_iter`` steps or when max_j |x^{k+1} - x^k| / range_j <= tol.  ``results`` holds the history.
    ``continuation`` (a BetaContinuation) runs its schedule inside the loop: ``results['beta']``, ``['eta']`` and
    ``['grayness']`` then hold the projection's sharpness, threshold and M_nd of the design each step was taken from,
    ``results['reset']`` the steps (from 1) that began with a fresh asymptote history."""

    def __init__(self, prob: CSDLProblem, max_iter: int = 100, move: float = 0.5, tol: float = 1e-3, sub_tol: float = 1e-7,
                 normalize: bool = True, c: float = 1000.0, d: float = 1.0,
                 continuation: Optional[BetaContinuation] = None):
        if not isinstance(prob, CSDLProblem):
            raise ValueError("MMA needs a CSDLProblem")
        _check_params(prob.m, move, sub_tol)
        if int(max_iter) < 1:
            raise ValueError(f"MMA: max_iter = {max_iter}")
        self.prob, self.max_iter, self.move, self.tol, self.sub_tol = prob, int(max_iter), float(move), float(tol), float(sub_tol)
        self.normalize, self.c, self.d = bool(normalize), c, d
        if continuation is not None and not isinstance(continuation, BetaContinuation):
            raise ValueError("MMA: continuation must be a BetaContinuation")
        self.continuation = continuation
        self.results: Dict[str, List] = {}
        self.handle: Optional[DeviceMMA] = None
        self.callback = None          # called as callback(x, f0, df0, f, df) with the update's arguments just before it

    def setup(self) -> "MMA":
        """Create the device handle (uploads the two bound vectors, once); ``solve`` does it if need be."""
        from ..fea.utils_hip import get_context
        if self.handle is None:
            ctx, prob = get_context(), self.prob
            self.handle = DeviceMMA(ctx, Vec(ctx, prob.n).set(prob.xmin), Vec(ctx, prob.n).set(prob.xmax), prob.m, self.move,
                                    self.sub_tol, self.c, self.d)
        return self

    def solve(self) -> Dict[str, List]:
        from ..fea.utils_hip import get_context
        prob, sim = self.prob, self.prob.simulator
        ctx = get_context()
        n, m, dv = prob.n, prob.m, prob.dv_name
        device = bool(getattr(sim, "device", False))
        self.setup().handle.reset()
        x = Vec(ctx, n)
        if device:
            x.copy_from(sim.device_value(dv).vec)
            sim[dv] = DeviceArray(x, n)                  # the simulator reads the vector the update writes
        else:
            x.set(np.asarray(sim[dv], dtype=np.float64))
        df0, df = Vec(ctx, n), (Vec(ctx, m * n) if m > 0 else None)
        cols = [Vec(ctx, n, device_ptr=df.device_ptr + 8 * i * n) for i in range(m)]
        names = list(dict.fromkeys(r.name for r in prob.rows))
        res = self.results = dict(objective=[], constraints=[], max_dx=[], inner=[], halvings=[], stages=[], converged=[],
                                  update_ms=[], cycle_ms=[])
        cont = self.continuation
        if cont is not None:
            res.update(beta=[], eta=[], grayness=[], reset=[1])
            cont.start()
        scale0 = None
        for step in range(1, self.max_iter + 1):
            t0 = time.perf_counter()
            sim.run()
            J = prob.objective_scaler * float(np.asarray(sim[prob.objective]).ravel()[0])
            if scale0 is None:
                if self.normalize and (J == 0.0 or not np.isfinite(J)):
                    raise ValueError(f"MMA: the objective is {J} at the start design and cannot be normalised")
                scale0 = 1.0 / abs(J) if self.normalize else 1.0
            self._column(df0, sim.compute_totals(prob.objective, dv), prob.objective_scaler * scale0)
            val = {k: float(np.asarray(sim[k]).ravel()[0]) for k in names}
            grad = {k: sim.compute_totals(k, dv) for k in names}
            f = [r.sign * r.scaler * (val[r.name] - r.bound) for r in prob.rows]
            for r, col in zip(prob.rows, cols):
                self._column(col, grad[r.name], r.sign * r.scaler)
            ctx.sync()
            t1 = tc = time.perf_counter()
            if self.callback is not None:
                self.callback(x, J * scale0, df0, f, df)
                ctx.sync()
                t1 = time.perf_counter()
            info = self.handle.update(x, J * scale0, df0, f, df)
            if not device:
                sim[dv] = x.get()
            t2 = time.perf_counter()
            res["objective"].append(J); res["constraints"].append(f); res["max_dx"].append(info["max_dx"])
            res["inner"].append(info["newton_steps"]); res["halvings"].append(info["halvings"]); res["stages"].append(info["stages"])
            res["converged"].append(info["converged"])
            res["update_ms"].append((t2 - t1) * 1e3); res["cycle_ms"].append((tc - t0) * 1e3)
            if cont is not None:
                last = getattr(cont.op, "last", None) or {}
                res["beta"].append(cont.betas[cont.stage]); res["eta"].append(last.get("eta", float("nan")))
                res["grayness"].append(cont.op.grayness() if hasattr(cont.op, "grayness") else float("nan"))
                what = cont.after_step(info["max_dx_rel"], self.tol)
                if what == 'stop':
                    break
                if what == 'advance' and step < self.max_iter:
                    self.handle.reset()
                    res["reset"].append(step + 1)
            elif info["max_dx_rel"] <= self.tol:
                break
        self.x = x
        return res

    @staticmethod
    def _column(col: Vec, g, a: float) -> None:
        """col = a * g, g a DeviceArray (stays on the device) or a host array (uploaded)."""
        if isinstance(g, DeviceArray):
            col.fill(0.0)
            col.axpy(a, g.vec)
        else:
            col.set(a * np.asarray(g, dtype=np.float64).ravel())

    def print_results(self) -> None:
        r = self.results
        if not r or not r["objective"]:
            print("MMA: no step taken")
            return
        k = len(r["objective"])
        print(f"MMA {self.prob.problem_name}: {k} steps, objective {r['objective'][0]:.6g} -> {r['objective'][-1]:.6g}, "
              f"rows at the last step {['%.3e' % v for v in r['constraints'][-1]]}, last max|dx| {r['max_dx'][-1]:.3e}, "
              f"{sum(r['inner'])} Newton steps, update {np.mean(r['update_ms']):.2f} ms / cycle {np.mean(r['cycle_ms']):.2f} ms per step, "
              f"{'all subproblems converged' if all(c == 1 for c in r['converged']) else 'a subproblem hit a cap'}")
