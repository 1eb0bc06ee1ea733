"""The optimiser side of the reference's drivers (``from modopt import CSDLProblem, SLSQP``), on the device:

    from femo_amd.opt import CSDLProblem, MMA
    prob = CSDLProblem(problem_name='beam_topo_opt', simulator=sim)
    optimizer = MMA(prob, max_iter=100, move=0.5, tol=1e-3, sub_tol=1e-7, normalize=True)
    optimizer.solve(); optimizer.print_results()

``MMA`` is the Method of Moving Asymptotes (include/femo_hip.h; csrc/mma.hip), ``DeviceMMA`` the bare handle,
``BetaContinuation`` the schedule on the Heaviside projection's sharpness (``MMA(..., continuation=...)``)."""
from .mma import MMA, BetaContinuation, DeviceMMA
from .problem import CSDLProblem

__all__ = ["CSDLProblem", "MMA", "DeviceMMA", "BetaContinuation"]
