"""The reference's cantilever driver to its end (examples/beam_topo_opt/run_topo_opt_cantilever_beam.py): the SIMP design
loop with the device-resident MMA update in the place of modopt's SLSQP / SNOPT.

  python scripts/run_topopt.py --nelx 640 --nely 320 --pc multilevel --device --iters 20
  python scripts/run_topopt.py --n3 48 --pc multilevel --device --iters 20 --host-update
  ... --stress        a second constraint: the p-norm von Mises stress at most 0.9 times its value at the start design
  ... --host          Simulator(device=False): NumPy arrays at the operator boundary, uploaded for the update
  ... --host-update   also run the NumPy restatement's update (tests/mma_ref.py) on the same data, step by step
  ... --betas 1,2,4,8 --every 5   Heaviside projection between filter and state (ProjectedFilterModel) with continuation on
                      its sharpness: --every design steps per value (BetaContinuation); without --betas: today's model
  ... --eta 0.5|volume            the projection's threshold: a number in [0, 1] or the volume-preserving one
  ... --solid-frame W             a passive solid strip of W cells along the loaded edge (needs --betas; --betas 0 projects nothing else)
  ... --problem inverter [--kin 0.1 --kout 0.1 --volume 0.3 --move 0.2]   the half model of the force inverter on the 2 x 1
                      rectangle: input spring and unit input force at the top-left corner, output spring and the objective
                      u_out (port_displacement) at the top-right corner, a roller on the top (symmetry) edge, a clamp on
                      x = 0, y <= 0.1; minimises u_out under avg_density <= volume from x = volume
  ... --problem heatsink [--volume 0.3 --move 0.2]   the heat-sink problem on the 2 x 1 rectangle: uniform heating, a sink T = 0
                      over the middle fifth of the left edge, conductivity k_min + (1 - k_min) rho^3 with k_min = 1e-3
                      (ConductionResidual); minimises the thermal compliance under avg_density <= volume from x = volume;
                      --pc multilevel: the conduction solves with the lattice preconditioner weighted by K_theta's diagonals
  ... --filter helmholtz        the Helmholtz PDE filter (HelmholtzFilterModel, or ProjectedFilterModel(filter="helmholtz") with
                      --betas) in the neighbour list's place: one scalar solve per product, memory independent of the radius

Minimises the compliance under avg_density <= 0.40 from x = 0.4 (--problem cantilever, the default).  Prints one JSON line
(with --problem inverter also u_out per step and final_u_out): per step the objective, the
constraint values and the inner (Newton) iterations; the ms of the MMA update against the ms of the design cycle (the first
step is the warm-up and left out of the statistics: median, minimum, maximum over the others); the bytes a Newton step moves
by the count of DESIGN.md section 10 and the GB/s that gives; with --host-update the restatement's ms beside the device's,
alternating with it step by step, and the largest difference between the two updates.  Writes the final filtered density
to --out (XDMF).  With --betas the line also holds beta, eta and the grayness M_nd per step, the ms the projection takes per
step (its operation's own timers: compute, both products, synchronised) and its share of the cycle, and the ms of the 53-step
bisection alone (a volume-mode forward call minus a fixed-mode one on the final design, median of 10)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args):
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel, HelmholtzFilterModel, ProjectedFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, VectorFunctionSpace,
                                      createRectangleMesh, createUnitCubeMesh, locate_dofs_geometrical,
                                      locate_entities_boundary, meshSize, meshtags)
    if args.n3:
        mesh = createUnitCubeMesh(args.n3)
        marker = lambda x: np.logical_and(np.isclose(x[0], 1.0), x[2] < 0.25)
        t = (0.0, 0.0, -1.0)
    else:
        LX, LY = 160.0, 80.0
        mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), args.nelx, args.nely)
        marker = lambda x: np.logical_and(abs(x[1] - LY / 2) < LY / args.nely + 3e-6, abs(x[0] - LX) < 3e-6)
        t = (0.0, -0.25)
    d = mesh.tdim
    facets = locate_entities_boundary(mesh, d - 1, marker)
    ds_ = Measure("ds", domain=mesh, subdomain_data=meshtags(mesh, d - 1, facets, np.full(len(facets), 100, dtype=np.int32)))
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(V)
    f = Constant(mesh, t)
    res = pdeRes(u, None, rho, f, dss=ds_(100), preconditioner=args.pc)
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    fea.add_output(name="avg_density", type="scalar", form=averageFunc(rho), arguments=["density"])
    fea.add_output(name="compliance", type="scalar", form=compliance(u, f, dss=ds_(100)), arguments=["displacements"])
    stress = None
    if args.stress:
        from femo_amd.fea.elasticity import pnorm_stress
        stress = pnorm_stress(u, rho, p=8.0, q=0.5)
        fea.add_output(name="stress", type="scalar", form=stress, arguments=["displacements", "density"])
        fea.consistent_bc_partials = True
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0.0, atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    betas = getattr(args, "betas", None)
    helmholtz = getattr(args, "filter", "neighbours") == "helmholtz"
    if betas:
        from femo_amd.fea.elasticity import cell_volumes
        frame, solid = int(getattr(args, "solid_frame", 0) or 0), None
        if frame > 0:
            if args.n3:
                raise SystemExit("--solid-frame is for the rectangle")
            solid = np.nonzero(mesh.centroids()[:, 0] >= LX - frame * LX / args.nelx - 1e-9)[0]
        eta = getattr(args, "eta", "0.5")
        which = dict(filter="helmholtz", mesh=mesh) if helmholtz else dict(coordinates=Q.tabulate_dof_coordinates())
        filt = ProjectedFilterModel(nel=mesh.n_cell, h_avg=(h.max() + h.min()) / 2, projection_beta=betas[0],
                                    eta=eta if eta == "volume" else float(eta), volumes=cell_volumes(mesh), solid=solid, **which)
        args.projection = filt
    elif helmholtz:
        filt = HelmholtzFilterModel(mesh=mesh, beta=2.0, h_avg=(h.max() + h.min()) / 2)
    else:
        filt = GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2)
    model.add(filt, name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.full(mesh.n_cell, 0.4))
    model.add_design_variable("density_unfiltered", upper=1.0, lower=1e-4)
    model.add_objective("compliance")
    model.add_constraint("avg_density", upper=0.40)
    sim = Simulator(model, device=args.device)
    return sim, model, mesh, stress


def build_inverter(args):
    """The compliant-mechanism problem: elastic supports at the two ports and a displacement output as the objective."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Function, FunctionSpace, VectorFunctionSpace, createRectangleMesh, displacement,
                                      locate_dofs_geometrical, meshSize, point_springs, port_displacement)
    if args.n3:
        raise SystemExit("--problem inverter is for the rectangle")
    LX, LY = 2.0, 1.0
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), args.nelx, args.nely)
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ("DG", 0)), VectorFunctionSpace(mesh, ("CG", 1))
    rho, u = Function(Q), Function(V)
    corner = lambda cx: int(np.nonzero(np.isclose(mesh.x[:, 0], cx) & np.isclose(mesh.x[:, 1], LY))[0][0])
    dof_in, dof_out = 2 * corner(0.0), 2 * corner(LX)
    springs = point_springs(V, [dof_in, dof_out], [args.kin, args.kout])
    res = pdeRes(u, None, rho, None, preconditioner=args.pc, springs=springs, point_load=port_displacement(V, [dof_in]))
    fea.add_input("density", rho)
    fea.add_state(name="displacements", function=u, residual_form=res, arguments=["density"])
    fea.add_output(name="avg_density", type="scalar", form=averageFunc(rho), arguments=["density"])
    fea.add_output(name="u_out", type="scalar", form=displacement(u, port_displacement(V, [dof_out])), arguments=["displacements"])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.logical_and(np.isclose(x[0], 0.0), x[1] <= 0.1 * LY + 1e-9)),
                            locate_dofs_geometrical(V.sub(1), lambda x: np.isclose(x[1], LY))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.full(mesh.n_cell, args.volume))
    model.add_design_variable("density_unfiltered", upper=1.0, lower=1e-3)
    model.add_objective("u_out")
    model.add_constraint("avg_density", upper=args.volume)
    return Simulator(model, device=args.device), model, mesh, None


def build_heatsink(args):
    """The heat-sink problem: uniform heating of the 2 x 1 rectangle, a sink T = 0 over the middle fifth of the left edge,
    conductivity k_min + (1 - k_min) rho^3 with k_min = 1e-3; minimises the thermal compliance Q^T T under
    avg_density <= volume from x = volume."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc
    from femo_amd.fea.fea_hip import (FEA, Function, FunctionSpace, createRectangleMesh, locate_dofs_geometrical, meshSize,
                                      pdeRes_conduction, thermal_compliance)
    if args.n3:
        raise SystemExit("--problem heatsink is for the rectangle")
    LX, LY = 2.0, 1.0
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([LX, LY]), args.nelx, args.nely)
    fea = FEA(mesh)
    fea.REPORT = False
    fea.consistent_bc_partials = True          # the load Q is non-zero on the sink, and so is the multiplier
    Q, P = FunctionSpace(mesh, ("DG", 0)), FunctionSpace(mesh, ("CG", 1))
    rho, T = Function(Q), Function(P)
    res = pdeRes_conduction(T, None, rho, source=1.0, k0=1.0, k_min=1e-3, preconditioner=args.pc)
    fea.add_input("density", rho)
    fea.add_state(name="temperature", function=T, residual_form=res, arguments=["density"])
    fea.add_output(name="avg_density", type="scalar", form=averageFunc(rho), arguments=["density"])
    fea.add_output(name="thermal_compliance", type="scalar", form=thermal_compliance(T, source=1.0), arguments=["temperature"])
    Tbc = Function(P)
    Tbc.vector.set(0.0)
    sink = lambda x: np.logical_and(np.isclose(x[0], 0.0), abs(x[1] - LY / 2) <= 0.1 * LY + 1e-9)
    fea.add_strong_bc(Tbc, [locate_dofs_geometrical((P, P), sink)], P)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=(h.max() + h.min()) / 2),
              name="general_filter_model")
    model.create_input("density_unfiltered", shape=mesh.n_cell, val=np.full(mesh.n_cell, args.volume))
    model.add_design_variable("density_unfiltered", upper=1.0, lower=1e-3)
    model.add_objective("thermal_compliance")
    model.add_constraint("avg_density", upper=args.volume)
    return Simulator(model, device=args.device), model, mesh, None


def newton_step_bytes(n, m):
    """Bytes one Newton step without halvings moves ("Optimiser"): the three reading passes and the
    commit each read x, xi, eta, L, U, alpha, beta and p, q of the m + 1 functions; the commit writes x, xi, eta."""
    return (4 * (7 + 2 * (m + 1)) + 3) * 8 * n


def stats(v):
    v = np.asarray(v[1:] if len(v) > 1 else v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nelx", type=int, default=80)
    ap.add_argument("--nely", type=int, default=40)
    ap.add_argument("--n3", type=int, default=0)
    ap.add_argument("--pc", choices=("jacobi", "multilevel"), default="jacobi")
    ap.add_argument("--iters", type=int, default=20)
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--device", dest="device", action="store_true", default=True)
    mode.add_argument("--host", dest="device", action="store_false")
    ap.add_argument("--stress", action="store_true")
    ap.add_argument("--host-update", action="store_true")
    ap.add_argument("--betas", type=lambda t: [float(b) for b in t.split(",")], default=None)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--eta", default="0.5")
    ap.add_argument("--solid-frame", type=int, default=0)
    ap.add_argument("--filter", choices=("neighbours", "helmholtz"), default="neighbours",
                    help="the explicit neighbour list (default) or the Helmholtz PDE filter (memory independent of the radius)")
    ap.add_argument("--out", default=os.path.join("topopt_out", "density.xdmf"))
    ap.add_argument("--problem", choices=("cantilever", "inverter", "heatsink"), default="cantilever")
    ap.add_argument("--kin", type=float, default=0.1, help="inverter: the input spring")
    ap.add_argument("--kout", type=float, default=0.1, help="inverter: the output (workpiece) spring")
    ap.add_argument("--volume", type=float, default=0.3, help="inverter, heatsink: the volume bound and the start density")
    ap.add_argument("--move", type=float, default=None, help="the move limit of MMA (cantilever 0.5, inverter and heatsink 0.2)")
    args = ap.parse_args()
    inverter, heatsink = args.problem == "inverter", args.problem == "heatsink"
    if (inverter or heatsink) and (args.stress or args.betas or args.filter != "neighbours"):
        raise SystemExit(f"--problem {args.problem} runs the plain neighbour filter without --stress")
    if args.solid_frame and not args.betas:
        raise SystemExit("--solid-frame needs --betas (passive cells go through the projection)")
    from femo_amd import _lib
    from femo_amd.engine import Context, Vec
    from femo_amd.fea import utils_hip
    from femo_amd.fea.io import XDMFRecorder
    from femo_amd.opt import MMA, BetaContinuation, CSDLProblem
    if _lib.device_count() < 1:
        raise SystemExit("run_topopt needs a HIP device")
    ctx = Context(0)
    utils_hip.set_context(ctx)
    sim, model, mesh, stress = build_inverter(args) if inverter else build_heatsink(args) if heatsink else build(args)
    utils_hip.LAST_KSP_INFO.clear()          # a complete record of this run's solves
    n = mesh.n_cell
    if stress is not None:
        # the aggregate's scale from the start design, and its bound: 0.9 times its value there
        sim.run()
        cells = Vec(ctx, n)
        stress.m = 1.0 / float(np.max(stress.device().von_mises(stress.u.vec, cells, stress.rho.vec, stress.q).get()))
        sim.run()
        model.add_constraint("stress", upper=0.9 * float(np.asarray(sim["stress"]).ravel()[0]))
    prob = CSDLProblem(problem_name="beam_topo_opt", simulator=sim)
    op = args.projection.operation if args.betas else None
    cont = BetaContinuation(op, args.betas, args.every) if args.betas else None
    move = args.move if args.move is not None else (0.2 if inverter or heatsink else 0.5)
    optimizer = MMA(prob, max_iter=args.iters, move=move, tol=0.0, sub_tol=1e-7, normalize=True, continuation=cont).setup()
    host = dict(ms=[], dx=[], newton=[])
    proj_ms = []
    if op is not None:
        op.sync_timers = True

        def on_projection(*_):                 # once per step, after run() and the totals: what the operation took since the last call
            total = op.time_ms["compute"] + op.time_ms["jacvec"]
            proj_ms.append(total - sum(proj_ms))
        optimizer.callback = on_projection
    if args.host_update:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mma_ref
        ref = mma_ref.MMA(prob.xmin, prob.xmax, prob.m)
        pending = []

        def on_update(x, f0, df0, f, df):
            xh, g0 = np.array(x.get()), np.array(df0.get())
            g = np.array(df.get()).reshape(prob.m, n) if prob.m else np.zeros((0, n))
            t0 = time.perf_counter()
            xn = ref.update(xh, g0, f, g)
            host["ms"].append((time.perf_counter() - t0) * 1e3)
            host["newton"].append(ref.last["rec"]["newton"])
            # the restatement keeps its own history; it is handed the device's iterate every step, so that both update the same data
            pending.append((x, xn))
            if op is not None:
                on_projection()
        optimizer.callback = on_update
    res = optimizer.solve()
    if args.host_update:
        # the device's x^{k+1} is the next step's x^k: compare the last pair (the earlier ones were overwritten in place)
        x, xn = pending[-1]
        host["dx"] = float(np.abs(np.array(x.get()) - xn).max())
    optimizer.print_results()
    sim.run()
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rec = XDMFRecorder(args.out)
    rec.write_mesh(mesh)
    rho = np.array(np.asarray(sim["density"]), dtype=np.float64)
    rec.write_function(types.SimpleNamespace(vector=types.SimpleNamespace(getArray=lambda: rho), name="density"), t=len(res["objective"]))
    upd, cyc = stats(res["update_ms"]), stats(res["cycle_ms"])
    inner = res["inner"][1:] if len(res["inner"]) > 1 else res["inner"]
    trials = np.add(res["inner"], res["halvings"]) + np.asarray(res["stages"])
    passes = 3 * np.asarray(res["inner"]) + trials                      # assemble, stepmax, commit + every trial
    step_bytes = newton_step_bytes(n, prob.m)
    update_bytes = passes * (7 + 2 * (prob.m + 1)) * 8 * n + 3 * 8 * n * np.asarray(res["inner"])
    gbps = update_bytes / (np.asarray(res["update_ms"]) * 1e-3) / 1e9
    out = dict(metric="topopt_mma", mesh=(f"cube n={args.n3}" if args.n3 else f"rect {args.nelx}x{args.nely}"), n_cell=n,
               m=prob.m, pc=args.pc, device=bool(args.device), steps=len(res["objective"]), objective=res["objective"],
               constraints=res["constraints"], inner=res["inner"], halvings=res["halvings"], converged=res["converged"],
               max_dx=res["max_dx"], update_ms=upd, cycle_ms=cyc, update_share=upd["median"] / (upd["median"] + cyc["median"]),
               newton_per_update=float(np.mean(inner)), newton_step_bytes=step_bytes,
               update_GBps=stats(list(gbps)), density_file=args.out,
               avg_density=float(np.asarray(sim["avg_density"]).ravel()[0]))
    if inverter:
        # state and adjoint PCG of every design cycle, in the order they ran
        pcg_log = [r for r in utils_hip.LAST_KSP_INFO if str(r.get("kind", "")).startswith("elasticity_")]
        out.update(metric="topopt_mma_inverter", u_out=res["objective"], final_u_out=float(np.asarray(sim["u_out"]).ravel()[0]),
                   kin=args.kin, kout=args.kout, volume=args.volume, move=move,
                   pcg_iterations=[[r["kind"].split("_")[-1], r["iterations"]] for r in pcg_log])
    elif heatsink:
        # state and adjoint PCG of every design cycle (--pc: Jacobi or the lattice preconditioner), in the order they ran
        pcg_log = [r for r in utils_hip.LAST_KSP_INFO if str(r.get("kind", "")).startswith("conduction_")]
        out.update(metric="topopt_mma_heatsink", final_thermal_compliance=float(np.asarray(sim["thermal_compliance"]).ravel()[0]),
                   volume=args.volume, move=move, k_min=1e-3,
                   pcg_iterations=[[r["kind"].split("_")[-1], r["iterations"]] for r in pcg_log])
    else:
        out["final_compliance"] = float(np.asarray(sim["compliance"]).ravel()[0])
    if op is not None:
        pm = stats(proj_ms)
        compute_ms, products_ms = op.time_ms["compute"], op.time_ms["jacvec"]       # of the loop: taken before the calls below
        xt, r1 = op._xt, Vec(ctx, n)
        calls = {}
        for eta in ("volume", 0.5):
            op.projection.set(eta=eta)
            op.projection.forward(xt, r1)
            calls[eta] = float(np.median([op.projection.forward(xt, r1)["ms"] for _ in range(10)]))
        op.eta = args.eta if args.eta == "volume" else float(args.eta)
        steps = max(len(proj_ms), 1)
        out.update(beta=res["beta"], eta=res["eta"], grayness=res["grayness"], reset=res["reset"], projection_ms=pm,
                   projection_compute_ms_mean=compute_ms / max(op.time_ms["calls"], 1), projection_products_ms_mean=products_ms / steps,
                   projection_share=pm["median"] / (upd["median"] + cyc["median"]), bisection_ms=calls["volume"] - calls[0.5],
                   forward_volume_ms=calls["volume"], forward_fixed_ms=calls[0.5])
    if args.host_update:
        out.update(host_update_ms=stats(host["ms"]), host_newton=host["newton"], host_vs_device_last_dx=host["dx"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
