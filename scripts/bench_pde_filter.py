"""The two density filters side by side on one mesh and radius, in one process: build time, bytes held, one W x and one
W^T y, PCG iterations of the Helmholtz solves, and the SIMP cycle (filter -> state -> compliance -> adjoint -> W^T) with
each filter.  Legs alternate after a warm-up; every time is a median with its min and max.  Prints one JSON line.

  python scripts/bench_pde_filter.py --nelx 640 --nely 320 --radius-h 2
  python scripts/bench_pde_filter.py --n3 48 --radius-h 4

The neighbour list's size is computed before it is built (n_cell times the cells in a ball of radius r: 2 pi (r/h)^2 in
the rectangle's two triangles per square, 6 (4/3) pi (r/h)^3 in the cube's six tetrahedra per box; 20 B per pair).  A leg
that would take more than a quarter of the device's free memory is skipped and reported as such.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise SystemExit("hipMemGetInfo failed")
    return int(free.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nelx", type=int, default=80)
    ap.add_argument("--nely", type=int, default=40)
    ap.add_argument("--n3", type=int, default=0)
    ap.add_argument("--radius-h", type=float, default=2.0)
    ap.add_argument("--h", choices=("avg", "edge"), default="avg",
                    help="the h of --radius-h: the mean cell size (h.max + h.min) / 2 the models use, or the box edge")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--no-cycle", action="store_true")
    args = ap.parse_args()
    from femo_amd import _lib
    from femo_amd.engine import Context, Vec
    from femo_amd.fea import utils_hip
    from femo_amd.fea.elasticity import DeviceFilter, DevicePdeFilter
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh, meshSize
    if _lib.device_count() < 1:
        raise SystemExit("bench_pde_filter needs a HIP device")
    ctx = Context(0)
    utils_hip.set_context(ctx)
    mesh = createUnitCubeMesh(args.n3) if args.n3 else createRectangleMesh(np.array([0.0, 0.0]), np.array([160.0, 80.0]), args.nelx, args.nely)
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    edge = 1.0 / args.n3 if args.n3 else 160.0 / args.nelx
    r = args.radius_h * (edge if args.h == "edge" else h_avg)
    n = mesh.n_cell
    # the neighbour list before it is built (the formula counts in box edges)
    per_cell = 6 * (4.0 / 3.0) * np.pi * (r / edge) ** 3 if args.n3 else 2 * np.pi * (r / edge) ** 2
    est_bytes = 20.0 * per_cell * n
    free = free_bytes()
    out = dict(metric="pde_filter", mesh=(f"cube n={args.n3}" if args.n3 else f"rect {args.nelx}x{args.nely}"), n_cell=n,
               n_vert=mesh.n_vert, radius_h=args.radius_h, h=args.h, radius=r, h_avg=h_avg, edge=edge, neighbours_estimated_bytes=est_bytes,
               device_free_bytes=free, reps=args.reps)
    legs = {}
    ctx.sync()
    t0 = time.perf_counter()
    legs["helmholtz"] = DevicePdeFilter(ctx, mesh, r)
    ctx.sync()
    out["helmholtz_build_ms"] = (time.perf_counter() - t0) * 1e3
    if est_bytes > free / 4:
        out["neighbours"] = "skipped: the list would exceed a quarter of the free device memory"
    else:
        c = mesh.centroids()
        ctx.sync()
        t0 = time.perf_counter()
        legs["neighbours"] = DeviceFilter(ctx, c, r)
        ctx.sync()
        out["neighbours_build_ms"] = (time.perf_counter() - t0) * 1e3
        out["neighbours_nnz"] = legs["neighbours"].nnz
        out["neighbours_bytes"] = 20 * legs["neighbours"].nnz + 8 * (n + 1)
    x = Vec(ctx, n).set(np.random.default_rng(0).uniform(0.0, 1.0, n))
    y = Vec(ctx, n)
    times = {(k, t): [] for k in legs for t in (False, True)}
    iters = {}
    for rep in range(args.reps + 1):                                # rep 0: warm-up (the scaled copy of A appears here)
        for t in (False, True):
            for k, f in legs.items():
                ctx.sync()
                t0 = time.perf_counter()
                f.apply(x, y, transpose=t)
                ctx.sync()
                if rep:
                    times[(k, t)].append((time.perf_counter() - t0) * 1e3)
                if k == "helmholtz":
                    iters["WT" if t else "W"] = f.last_info["iterations"]
    for (k, t), v in times.items():
        out[f"{k}_{'WT' if t else 'W'}_ms"] = stats(v)
    out["helmholtz_iterations"] = iters
    out["helmholtz_bytes"] = legs["helmholtz"].bytes
    out["helmholtz_solve_ms_last"] = legs["helmholtz"].last_info["solve_ms"]
    del legs, x, y
    if not args.no_cycle:
        spec = importlib.util.spec_from_file_location("bench_topopt", os.path.join(ROOT, "scripts", "bench_topopt.py"))
        bt = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bt)
        sims = {}
        for k in ("neighbours", "helmholtz"):
            if k == "neighbours" and "neighbours_nnz" not in out:
                continue
            a = argparse.Namespace(n3=args.n3, nelx=args.nelx, nely=args.nely, pc="jacobi", stress=False, filter=k, radius_h=r / h_avg)
            sims[k] = bt.build(a)[0]
        x0 = {k: np.array(s["density_unfiltered"]) for k, s in sims.items()}
        cyc = {k: [] for k in sims}
        for c in range(args.cycles + 1):
            for k, s in sims.items():
                s["density_unfiltered"] = x0[k] * (1.0 - 1e-3 * c)
                ctx.sync()
                t0 = time.perf_counter()
                s.run()
                np.asarray(s.compute_totals("compliance", "density_unfiltered"))
                ctx.sync()
                if c:
                    cyc[k].append((time.perf_counter() - t0) * 1e3)
        for k, v in cyc.items():
            out[f"{k}_cycle_ms"] = stats(v)
            out[f"{k}_compliance"] = float(sims[k]["compliance"][0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
