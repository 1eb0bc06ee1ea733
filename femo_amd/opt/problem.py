"""``CSDLProblem``: what ``Model.add_design_variable`` / ``add_constraint`` / ``add_objective`` recorded, read into the shape
an optimiser works on -- one design vector in a box, an objective, rows ``g_i(x) <= 0``.  Stands in for modopt.CSDLProblem
(run_topo_opt_cantilever_beam.py).  Nothing here touches the device."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np


class Row(NamedTuple):
    """One inequality row  sign * scaler * (g - bound) <= 0  of the output ``name``."""
    name: str
    sign: float
    bound: float
    scaler: float


def _scaler(v) -> float:
    s = 1.0 if v is None else float(v)
    if not np.isfinite(s) or s <= 0.0:
        raise ValueError(f"scaler = {v!r}: a positive finite number is needed")
    return s


class CSDLProblem:
    def __init__(self, problem_name: str = "problem", simulator=None):
        if simulator is None:
            raise ValueError("CSDLProblem needs the simulator")
        self.problem_name = problem_name
        self.simulator = simulator
        model = simulator.model
        dvs = getattr(model, "design_variables", {})
        if len(dvs) != 1:
            raise ValueError(f"MMA works on exactly one design-variable vector, the model has {len(dvs)}: {sorted(dvs)} "
                             "(several vectors are out of scope)")
        (self.dv_name, dv), = dvs.items()
        var = model.variables.get(self.dv_name) if hasattr(model, "variables") else None
        if var is None:
            raise ValueError(f"design variable {self.dv_name!r} is not an input of the model")
        self.n = int(np.prod(var.shape))
        self.dv_scaler = _scaler(dv.get("scaler"))
        if self.dv_scaler != 1.0:
            raise ValueError("a scaler on the design variable is not supported: scale the bounds instead")
        self.xmin = self._bound(dv.get("lower"), "lower")
        self.xmax = self._bound(dv.get("upper"), "upper")
        if np.any(self.xmax <= self.xmin):
            raise ValueError(f"design variable {self.dv_name!r}: upper <= lower in {int(np.sum(self.xmax <= self.xmin))} entries "
                             "(passive regions are out of scope)")
        obj = getattr(model, "objective", None)
        if not obj:
            raise ValueError("the model has no objective")
        self.objective = obj["name"]
        self.objective_scaler = _scaler(obj.get("scaler"))
        self.rows: List[Row] = []
        for name, c in getattr(model, "constraints", {}).items():
            if c.get("equals") is not None:
                raise ValueError(f"constraint {name!r}: equality constraints are out of scope for MMA")
            s = _scaler(c.get("scaler"))
            lower, upper = c.get("lower"), c.get("upper")
            if lower is None and upper is None:
                raise ValueError(f"constraint {name!r} has neither lower nor upper")
            for b, sign in ((upper, 1.0), (lower, -1.0)):
                if b is None:
                    continue
                if np.size(b) != 1 or not np.isfinite(float(np.asarray(b).ravel()[0])):
                    raise ValueError(f"constraint {name!r}: the bound {b!r} must be one finite number")
                self.rows.append(Row(name, sign, float(np.asarray(b).ravel()[0]), s))
        self.m = len(self.rows)

    def _bound(self, v, which: str) -> np.ndarray:
        if v is None:
            raise ValueError(f"design variable {self.dv_name!r} has no {which} bound: MMA needs a box")
        a = np.asarray(v, dtype=np.float64)
        if a.size not in (1, self.n):
            raise ValueError(f"design variable {self.dv_name!r}: {which} has {a.size} entries, expected 1 or {self.n}")
        a = np.broadcast_to(a.ravel(), (self.n,)).astype(np.float64).copy() if a.size == 1 else a.ravel().copy()
        if not np.all(np.isfinite(a)):
            raise ValueError(f"design variable {self.dv_name!r}: {which} is not finite everywhere: MMA needs a box")
        return a
