#!/usr/bin/env python3
"""Benchmark of femo's hot path on MI355X: DOFs/s of one assemble + adjoint-solve cycle.

One *step* = one full cycle of SURVEY.md section 8(d) through the operator surface
(FEAModel / StateOperation / OutputOperation):

    set f -> solve_residual_equations (Newton x3: assemble R, dR/du, A; CG)
          -> OutputOperation.compute (J) -> compute_totals:
             OutputOperation.compute_derivatives (dJ/du, dJ/df)
             StateOperation.compute_derivatives (dR/du, dR/df, A)
             apply_inverse_jacobian 'rev' (transposed CG solve)
             compute_jacvec_product 'rev' (dR/df^T lambda)   -> dJ/df

Every step gets a different synthetic source f_k and a cold start u = 0, so no
result of a previous step can be reused.  ``value`` is the SURVEY.md 8(d) metric:
NumPy arrays at the operator boundary, host-to-device and device-to-host traffic
inside the timed region.  ``device_resident`` is the same cycle with inputs and
outputs kept in HBM (round 1's headline), ``pageable_boundary`` the cycle with a
driver that keeps every array in pageable memory.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline line (``value``, ``ms_per_step`` and what the
timed steps themselves counted); ``--dump-outputs DIR`` also writes what the last timed step returned.  Everything else --
the device-resident, pageable and u = 1 legs, the SpMV roofline, PCIe rates, the self-check, configs 2 / 5 / 3, the
scaling models and the CPU baselines -- runs only with ``--full``, where the ``--no-*`` switches select among them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# before anything in this process can initialise the HIP runtime (torch's control plane included): a context's compute, copy
# and exchange streams -- and RCCL's -- must not share hardware queues (femo_amd/_lib.py, DESIGN_LOG.md R6.6)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

METRIC = "DOFs/sec assemble+adjoint-solve, 10M-DOF Poisson, 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s measured copy)
ALPHA = 1e-6                   # run_poisson_opt.py:112
PC = "bpx"                     # set from --pc in main()


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--mesh-n", dest="n", type=int, default=215, help="cube resolution (215 -> 10,077,696 DOFs)")
    p.add_argument("--jitter", type=float, default=0.0,
                   help="interior vertex jitter in units of h (SURVEY.md 8(d): 0.2); default: structured grid")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-n", type=int, default=0, help="cube resolution of the CPU baseline (0: the benchmark's own size, one cycle)")
    p.add_argument("--permute", action="store_true",
                   help="random vertex numbering: no regular SELL slices, scattered gathers (the unstructured-mesh rate)")
    p.add_argument("--no-pcie", action="store_true")
    p.add_argument("--no-configs", action="store_true", help="skip the legs for BASELINE configs 2, 5 and 3 (reported under 'configs') and the scaling model")
    p.add_argument("--scaling-model", action="store_true", help="only with --no-configs: still run the 8-rank block leg ('scaling_model')")
    p.add_argument("--no-check", action="store_true", help="skip the self-check of the timed configuration against the DST-exact cycle")
    p.add_argument("--reorder", action="store_true",
                   help="Mesh.reordered(): what import_mesh does to a mesh it reads (Morton curve unless the numbering is already structured)")
    p.add_argument("--force-morton", action="store_true", help="with --reorder: renumber along the Morton curve regardless")
    p.add_argument("--pc", choices=("bpx", "jacobi"), default="bpx",
                   help="CG preconditioner: bpx = Jacobi + auxiliary-lattice multilevel correction (default)")
    p.add_argument("--full", action="store_true",
                   help="everything besides the headline: device-resident / pageable / u = 1 legs, SpMV roofline, PCIe rates, "
                        "self-check, configs 2 / 5 / 3, scaling models and CPU baselines (the --no-* switches select among them)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step returned (dJ/df, u, J) as DIR/<name>.npy in float64; arrays of more than "
                        f"{DUMP_MAX_ENTRIES} entries as a fixed seeded sample of that many (N = 1 only)")
    return p.parse_args()


DUMP_MAX_ENTRIES = 3_000_000       # per array: dJ/df and u at most 24 MB each in float64, 48 MB in all
DUMP_SEED = 20240807


def dump_outputs(directory: str, arrays: dict) -> dict:
    """``DIR/<name>.npy`` (float64) for every array; one of more than DUMP_MAX_ENTRIES entries is replaced by its values at
    ``np.unique(default_rng(DUMP_SEED).integers(0, size, DUMP_MAX_ENTRIES))`` -- the same sorted indices on every run of
    the same size, so two builds can be compared entry for entry.  Returns {name: entries written}."""
    os.makedirs(directory, exist_ok=True)
    out = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.size > DUMP_MAX_ENTRIES:
            a = a[np.unique(np.random.default_rng(DUMP_SEED).integers(0, a.size, DUMP_MAX_ENTRIES))]
        np.save(os.path.join(directory, f"{name}.npy"), a)
        out[name] = int(a.size)
    return out


def spmv_algorithmic_bytes(nnz: int, n: int) -> int:
    """B_A = nnz*12 + (N+1)*4 + 2N*8 (CSR values+columns, row pointer, x, y)."""
    return nnz * 12 + (n + 1) * 4 + 2 * n * 8


def stored_bytes(info: dict, n: int) -> int:
    """Bytes the SELL SpMV actually has to move: values of every padded entry, column
    indices of the irregular slices only, per-slice deltas, diagonal, x and y."""
    ns = max(info["n_slices"], 1)
    frac_short = info.get("short_slices", 0) / ns                       # 16-bit column deltas
    frac_general = 1.0 - info["regular_slices"] / ns - frac_short       # 32-bit column indices
    return int(info["sell_entries"] * 8 + info["sell_entries"] * (4 * frac_general + 2 * frac_short)
               + info["n_slices"] * (8 + 4 * info["max_rowlen"]) + 3 * n * 8)


def source_fields(mesh, count: int, seed: int = 20240807):
    """f_k = f*(centroid) * (0.5 + smooth seeded modulation): K+W different inputs."""
    xc = mesh.centroids()
    # On the un-jittered grid a centroid coordinate is a multiple of h / 4, so every sine / cosine below takes one of
    # 4 n + 1 values per axis: tabulate them and gather (set-up of the harness: 8.4 s of NumPy transcendentals at C4
    # otherwise, VERDICT round 2 housekeeping).  Same values bit for bit: the table entries are evaluated by the same
    # NumPy calls on the same arguments.
    n4 = 4 * int(getattr(mesh, "n", 0) or 0)
    idx = None
    if n4 > 0:
        idx = np.rint(xc * n4).astype(np.int32)
        if np.abs(xc - idx / n4).max() > 1e-12:
            idx = None                                   # jittered or foreign mesh: evaluate point by point
    grid = np.arange(n4 + 1) / n4 if idx is not None else None

    def fun(f, arg_scale, axis):
        if idx is None:
            return f(arg_scale * xc[:, axis])
        return f(arg_scale * grid)[idx[:, axis]]

    base = fun(np.sin, np.pi, 0) * fun(np.sin, np.pi, 1)
    if xc.shape[1] == 3:
        base = base * fun(np.sin, np.pi, 2)
    base /= (1.0 + ALPHA * 4.0 * np.pi ** 4)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = rng.uniform(0.2, 0.8, size=3)
        k = rng.integers(1, 4, size=3)
        mod = 0.5 + a[0] * fun(np.cos, np.pi * k[0], 0) * a[1] * fun(np.cos, np.pi * k[1], 1) \
            + a[2] * xc[:, 2]
        out.append(base * mod)
    return out


def build_problem(mesh, device: bool, pinned: bool = True):
    """The set-up of examples/poisson_opt/run_poisson_opt.py:95-179 on the HIP mirror (3-D)."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Function, FunctionSpace, TestFunction, locate_dofs_geometrical,
                                      outputForm, pdeRes)
    d = mesh.tdim
    fea = FEA(mesh)
    fea.REPORT = False
    Vf, Vu = FunctionSpace(mesh, ('DG', 0)), FunctionSpace(mesh, ('CG', 1))
    f_fn, u_fn = Function(Vf), Function(Vu)
    v = TestFunction(Vu)

    class Expression_u:
        def eval(self, x):
            return np.prod(np.sin(np.pi * x[:d]), axis=0) / (d * np.pi ** 2)

    u_ex = fea.add_exact_solution(Expression_u, Vu)
    ubc = Function(Vu)
    ubc.vector.set(0.0)
    locs = []
    for k in range(d):
        locs.append(locate_dofs_geometrical((Vu, Vu), lambda x, k=k: np.isclose(x[k], 0., atol=1e-6)))
        locs.append(locate_dofs_geometrical((Vu, Vu), lambda x, k=k: np.isclose(x[k], 1., atol=1e-6)))
    fea.add_strong_bc(ubc, locs, Vu)
    fea.add_input('f', f_fn)
    fea.add_state(name='u', function=u_fn, residual_form=pdeRes(u_fn, v, f_fn), arguments=['f'])
    fea.add_output(name='l2_functional', type='scalar', form=outputForm(u_fn, f_fn, u_ex, ALPHA),
                   arguments=['f', 'u'])
    fea.PDE_SOLVER = 'Newton'
    model = FEAModel(fea=[fea])
    model.create_input('f', shape=fea.inputs_dict['f']['shape'], val=0.086)
    model.add_design_variable('f')
    model.add_objective('l2_functional', scaler=1e5)
    return Simulator(model, device=device, pinned=pinned), fea


def one_cycle(sim, fea, f_value, u0=None):
    """One step: new source in, cold start (nothing carried over), forward run, reverse sweep.
    Host mode: ``f_value`` / ``u0`` are NumPy arrays and the gradient comes back as one."""
    sim['f'] = f_value
    fea.states_dict['u']['function'].vector.set(0.0)
    if sim.device:
        sim.values['u'].vec.fill(0.0)
    else:
        sim['u'] = u0 if u0 is not None else np.zeros(fea.states_dict['u']['shape'])
    sim.run()
    return sim.compute_totals('l2_functional', 'f')


def usable_cores() -> int:
    """Cores this process may actually use: min(affinity, cgroup v2 cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


_CANON: dict = {}


def _canonical_mesh(n: int, jitter: float):
    """The oracle's own mesh generator (lexicographic numbering), shared by the checker and the CPU baseline."""
    from oracle import femo_oracle as fo
    key = (n, jitter)
    if key not in _CANON:
        _CANON.clear()
        _CANON[key] = fo.unit_cube_mesh(n, jitter=jitter)
    return _CANON[key]


def cpu_baseline(args, gpu_counts, n_dof_gpu, n_cell_gpu, nnz_gpu):
    """The same cycle on the host cores with the C/OpenMP oracle port: ONE cycle at the benchmark's own
    size by default (about 10 s of CPU work with BPX-CG), so nothing is extrapolated.  ``--cpu-n`` selects a
    smaller cube; the figure is then scaled by cells / nnz and says so."""
    from oracle import c_port
    c_port.use_native()            # the port compiled for THIS box's CPU when gcc is here (the shipped .so is x86-64-v3)
    from oracle import femo_oracle as fo
    n = args.cpu_n if args.cpu_n else args.n
    m = _canonical_mesh(n, args.jitter)
    f = source_fields(_Centroid(m), 1)[0]
    bd = fo.boundary_vertices_box(m.x)
    threads = usable_cores()
    out = c_port.poisson_cycle(3, m.x, m.conn, f, fo.u_target(m.x), bd, ALPHA, rtol=1e-14, threads=threads, pc=PC)
    T = out["times"]
    t_sample = T["cycle"]
    its = f"{out['it_fwd']}+{out['it_adj']}"
    head = (f"oracle/femo_oracle_c.c (C/OpenMP restatement, not FEniCSx): one whole cycle with the same {PC.upper()}-CG and the "
            f"same Newton noise-floor rule on the n={n} cube ({m.n_vert} DOFs), {t_sample:.2f} s, CG its {its}; "
            f"the GPU run's CG its were {gpu_counts}")
    if n == args.n:
        return {"value": m.n_vert / t_sample, "unit": "DOFs/s", "cores": int(out["threads"]), "kind": "port",
                "sample": head + "; measured at the benchmark's size, nothing scaled",
                "split_s": {k: round(v, 3) for k, v in T.items()}}
    # a smaller sample scaled to the benchmark mesh: assembly-like phases by cell count, CG by nnz x
    # iteration count (BPX counts do not grow with the mesh; Jacobi-CG counts grow in proportion to n)
    it_main = out["it_fwd"][0] + out["it_adj"]
    t_cg = T["cg_fwd"] + T["cg_adj"]
    per_it_per_nnz = t_cg / max(it_main, 1) / out["nnz"]
    t_other = t_sample - t_cg
    it_scaled = it_main * (args.n / n if PC == "jacobi" else 1.0)
    t_scaled = t_other * (n_cell_gpu / m.n_cell) + per_it_per_nnz * nnz_gpu * it_scaled
    return {"value": n_dof_gpu / t_scaled, "unit": "DOFs/s", "cores": int(out["threads"]), "kind": "port",
            "sample": head + f"; scaled to n={args.n} by cell count (assembly, {t_other:.2f} s) and nnz x {it_scaled:.0f} iterations"}


def dst_reference_cycle(n: int, k: int, count: int):
    """(u, dJ/df) of the structured n-cube for source field ``k`` of ``source_fields(..., count)``, both solves by the sine
    transform (oracle/c_port.py::poisson_cycle_dst): the checker of the N > 1 run, computed on rank 0 outside the timed region
    (`femo_amd/dist` calls back into the harness for it: the package itself never touches ``oracle/``)."""
    from oracle import c_port
    c_port.use_native()            # the port compiled for THIS box's CPU when gcc is here (the shipped .so is x86-64-v3)
    from oracle import femo_oracle as fo
    canon = _canonical_mesh(n, 0.0)
    fg = source_fields(_Centroid(canon), count)[k]
    ref = c_port.poisson_cycle_dst(n, 3, canon.x, canon.conn, fg, fo.u_target(canon.x), fo.boundary_vertices_box(canon.x), ALPHA,
                                   threads=usable_cores())
    return ref["u"], ref["grad"]


def self_check(args, mesh, f, u, J, grad):
    """The checker of the timed configuration (outside the timed region; part of the CPU leg like ``cpu_baseline``, the
    only other place that touches ``oracle/``): state, functional and total gradient of one more cycle of the SAME
    operator stack -- BPX-CG at KSP_OPTIONS['rtol_bpx'], Newton's noise rule, pinned host arrays -- against values
    that involve no iterative solver.  Structured cube: both solves by the type-I sine transform
    (oracle/c_port.py::poisson_cycle_dst, exact to round-off at any size); the vertex / cell numbering of permuted or
    reordered meshes is mapped back through the coordinates.  Jittered cube: no closed form exists, the C port's
    cycle with a 100x tighter CG tolerance stands in and ``kind`` says so.
    Reference algebra: femo/csdl_opt/state_model.py:87-115, 202-218."""
    from oracle import c_port
    c_port.use_native()            # the port compiled for THIS box's CPU when gcc is here (the shipped .so is x86-64-v3)
    from oracle import femo_oracle as fo
    n, d = args.n, mesh.tdim
    t0 = time.perf_counter()
    canon = _canonical_mesh(n, args.jitter)
    bd = fo.boundary_vertices_box(canon.x)
    # canonical (lexicographic) index of every vertex / cell of the benchmark's mesh, from the un-jittered lattice
    # position (jitter moves interior vertices by < h/2, so rounding recovers it) and the cell's vertex set
    if not (args.permute or args.reorder):
        vmap, cmap = None, None                      # generated in canonical numbering
    else:
        iv = np.rint(mesh.x * n).astype(np.int64)
        vmap = (iv[:, 2] * (n + 1) + iv[:, 1]) * (n + 1) + iv[:, 0]
        def cell_keys(conn, vm):
            s = np.sort(vm[conn] if vm is not None else conn.astype(np.int64), axis=1)
            order = np.lexsort((s[:, 3], s[:, 2], s[:, 1], s[:, 0]))
            return order
        oc, ob = cell_keys(canon.conn, None), cell_keys(mesh.conn, vmap)
        cmap = np.empty(mesh.n_cell, np.int64)
        cmap[ob] = oc                                # cell c of the benchmark mesh = canonical cell cmap[c]
    f_c = np.empty(canon.n_cell)
    if cmap is None:
        f_c[:] = f
    else:
        f_c[cmap] = f
    if args.jitter:
        ref = c_port.poisson_cycle(d, canon.x, canon.conn, f_c, fo.u_target(canon.x), bd, ALPHA, threads=usable_cores(),
                                   pc="bpx", rtol_bpx=1e-13)
        kind = "C port of the same cycle with BPX-CG at rtol 1e-13 (jittered mesh: no exact discrete solution)"
    else:
        ref = c_port.poisson_cycle_dst(n, d, canon.x, canon.conn, f_c, fo.u_target(canon.x), bd, ALPHA,
                                       threads=usable_cores())
        kind = "DST-exact discrete state and multiplier (oracle/c_port.py::poisson_cycle_dst), no iterative solve"
    u_ref = ref["u"] if vmap is None else ref["u"][vmap]
    g_ref = ref["grad"] if cmap is None else ref["grad"][cmap]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    return _judge({"u_rel_err": rel(np.asarray(u), u_ref), "grad_rel_err": rel(np.asarray(grad), g_ref),
                   "J_rel_err": float(abs(float(J) - float(ref["J"])) / abs(float(ref["J"]))),
                   "tolerance": 1e-10, "norm": "max-norm relative to the largest entry", "against": kind,
                   "seconds": time.perf_counter() - t0}, [("u_rel_err", "tolerance"), ("grad_rel_err", "tolerance"), ("J_rel_err", "tolerance")])


class _Centroid:
    def __init__(self, m):
        self._m = m

    def centroids(self):
        return self._m.x[self._m.conn].mean(axis=1)


# ---------------------------------------------------------------------------------------------------------------
# The other single-GPU configurations of BASELINE.json, timed after the headline leg and reported under "configs"
# (configs 2, 3 and 5 had builder-run numbers only).  Each record: ms_per_cycle, dofs_per_s,
# iteration counts, the roofline of its dominant kernel (HIP events inside its own loop) and a CPU baseline at a
# stated size (nothing scaled).
# ---------------------------------------------------------------------------------------------------------------
def whole_cycle_roofline(dim: int, N: int, Nc: int, nnz: int, its, ms_host: float, ms_dev: float) -> dict:
    """SURVEY.md section 8(d) cycle bytes, B = B_R #res + B_J #jac + B_F + (it_fwd + it_adj) B_it + B_A + (dR/df^T), with the
    passes and CG counts of THIS run, over the measured cycle time: the whole path against the HBM roofline, not only its
    best kernel.  Per-kernel formulae as in the survey (every array once per pass): B_R = Nc (4(d+1)+8) + N (8d+16),
    B_J = 4(d+1) Nc + 8d N + 8 nnz, B_F = Nc (4(d+1)+8(d+1)) + 8d N, B_A = 12 nnz + 4(N+1) + 16 N, B_it = B_A + 80 N (the
    fused lower bound).  Passes: Newton assembles F and A three times and F once more (#res = 4, #jac = 3),
    compute_derivatives assembles dR/du and A (#jac += 2) and dR/df (B_F), dJ/du is one product with the mass matrix (B_A),
    dR/df^T lambda streams the cell values once more (B_F)."""
    d = dim
    B_R = Nc * (4 * (d + 1) + 8) + N * (8 * d + 16)
    B_J = 4 * (d + 1) * Nc + 8 * d * N + 8 * nnz
    B_F = Nc * (4 * (d + 1) + 8 * (d + 1)) + 8 * d * N
    B_A = 12 * nnz + 4 * (N + 1) + 16 * N
    B_it = B_A + 80 * N
    n_it = int(sum(its)) if its else 0
    B = 4 * B_R + 5 * B_J + 2 * B_F + n_it * B_it + B_A
    out = {"bytes_per_cycle": int(B), "cg_iterations": n_it,
           "formula": "4 B_R + 5 B_J + 2 B_F + its * (B_A + 80 N) + B_A  (SURVEY.md section 8(d); PCIe bytes are not HBM bytes and are not in it)",
           "ms_per_cycle_host_boundary": ms_host, "achieved_GBs_host_boundary": B / (ms_host * 1e-3) / 1e9 if ms_host else None,
           "frac_host_boundary": B / (ms_host * 1e-3) / 1e9 / HBM_PEAK_GBS if ms_host else None}
    if ms_dev:
        out.update({"ms_per_cycle_device_resident": ms_dev, "frac_device_resident": B / (ms_dev * 1e-3) / 1e9 / HBM_PEAK_GBS})
    return out


def _judge(check: dict, pairs) -> dict:
    """`passed` for a check record: every (value key, tolerance key) pair must hold (the records listed
    values and tolerances but nothing computed a verdict).  main() flags the line and stderr when one fails."""
    ok = True
    for vk, tk in pairs:
        v, t = check.get(vk), check.get(tk)
        ok = ok and v is not None and t is not None and v == v and v <= t
    check["passed"] = bool(ok)
    return check


_PMC_FILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "pmc_traffic.json")


def _pmc_lookup(key: str):
    """(bytes per launch, file, build the pass was collected from) out of the newest committed hardware-counter pass that
    holds exactly this kernel at exactly this size (profiles/rNN_pmc_traffic.json, scripts/collect_profiles_r05.sh), or
    (None, None, None).  ADVICE round 4: the line says which pass -- and which build -- the stored figure comes from; it is
    divided by THIS run's measured time."""
    if not key:
        return None, None, None
    for name in _PMC_FILES:
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", name)))
        except Exception:
            continue
        if d.get(key) is not None:
            return d[key], name, d.get("collected_at_commit", "not recorded (before round 5)")
    return None, None, None


def _pmc_traffic(key: str):
    return _pmc_lookup(key)[0]


def _roofline(kernel: str, bytes_per_launch: int, ms: float, samples: int, note: str = "", stored: int = 0, traffic_key: str = "") -> dict:
    """One byte convention for every configuration (round 6): `achieved` / `frac` are PHYSICAL --
    the bytes the kernel really moves per launch (the PMC pass of this kernel at this size where one is committed, else the
    bytes of the stored format; `physical_bytes_source` says which) over the launch time measured in THIS run, against the
    8 TB/s peak.  `achieved_algorithmic` / `frac_algorithmic` price the same time with the ALGORITHMIC bytes of SURVEY.md
    8(d) (the CSR formula; for the shell the block format is the algorithm's own): a CSR-equivalent rate -- it says how fast
    a plain CSR kernel would have to stream to finish in the same time, and it exceeds the physical rate by the factor the
    compressed format saves (`format_compression`)."""
    ok = bool(ms and ms == ms and ms > 0)
    alg = bytes_per_launch / (ms * 1e-3) / 1e9 if ok else None
    stored = int(stored or bytes_per_launch)
    traffic, pmc_file, pmc_commit = _pmc_lookup(traffic_key)
    phys = traffic if traffic else stored
    ach = phys / (ms * 1e-3) / 1e9 if ok else None
    return {"bound": "hbm", "kernel": kernel, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS if ach else None, "traffic": traffic,
            "physical_bytes_per_launch": phys,
            "physical_bytes_source": f"PMC (2*FETCH_SIZE + WRITE_SIZE, profiles/{pmc_file}, collected at commit {pmc_commit})" if traffic else "stored bytes of the format the kernel reads",
            "achieved_algorithmic": alg, "frac_algorithmic": alg / HBM_PEAK_GBS if alg else None,
            "algorithmic_bytes_per_launch": int(bytes_per_launch), "stored_bytes_per_launch": stored,
            "format_compression": bytes_per_launch / phys if phys else None,
            "frac_algorithmic_note": "CSR-equivalent rate over the HBM peak, not a hardware fraction: the kernel moves format_compression x fewer bytes than the "
                                     "SURVEY.md 8(d) formula counts (and an operator that fits the 256 MB Infinity Cache is not read from HBM at all)",
            "frac_physical": ach / HBM_PEAK_GBS if ach else None,          # (rounds 2-5 name of `frac`; kept for readers of old lines)
            "avg_launch_ms": ms, "launches_timed": samples,
            "timed": "single launches inside the timed solver loops (HIP events on the library's stream)" + (("; " + note) if note else "")}


def _spmv_in_loop(infos):
    solves = [i for i in infos if i["spmv_samples"] > 0]
    n = sum(i["spmv_samples"] for i in solves)
    return (sum(i["spmv_ms"] for i in solves) / n if n else float("nan")), n


def _prime_pool(sim, names=("f", "u")):
    """The pinned pool sized before a leg's timed cycles, as in the headline leg: with asynchronous results two generations
    of result blocks are alive at a time, and a first-time hipHostMalloc would land in the timed region.  The recycled blocks
    of the leg before (other sizes) are released first."""
    from femo_amd import engine as E
    E.host_trim()
    n_f, n_u = (int(np.size(sim[k])) for k in names)
    prime = [E.pinned_empty(n_f) for _ in range(4)] + [E.pinned_empty(n_u) for _ in range(8)]
    del prime


def bench_config2(ctx, steps: int) -> dict:
    """BASELINE config 2: 3-D linear Poisson, n = 100 cube (1,030,301 DOFs), the same operator cycle as the headline."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    n = 100
    mesh = createUnitCubeMesh(n)
    sim, fea = build_problem(mesh, device=False)
    dm = mesh.device(ctx)
    fs = [E.pinned_array(f) for f in source_fields(mesh, 3)]
    u0 = E.pinned_full(mesh.n_vert, 0.0)
    _prime_pool(sim)                                                  # after the inputs took their blocks (see bench_unstructured)
    g = None
    for k in range(10):                                               # a 9 ms cycle: ten of them until the clocks have settled
        g = one_cycle(sim, fea, fs[k % 3], u0)
    ctx.sync()
    del utils_hip.LAST_KSP_INFO[:]
    E.host_syncs(reset=True)
    ms, g = _timed_cycles(ctx, lambda k: one_cycle(sim, fea, fs[k % 3], u0), steps, 0)
    host_syncs = (E.host_syncs() - 1) / steps
    infos = list(utils_hip.LAST_KSP_INFO)
    per = len(infos) // steps
    spmv_ms, ns = _spmv_in_loop(infos)
    nnz = dm.info["nnz"]
    from oracle import c_port
    c_port.use_native()            # the port compiled for THIS box's CPU when gcc is here (the shipped .so is x86-64-v3)
    from oracle import femo_oracle as fo
    om = _canonical_mesh(n, 0.0)
    bd = fo.boundary_vertices_box(om.x)
    f0 = source_fields(mesh, 1)[0]
    cpu = c_port.poisson_cycle(3, om.x, om.conn, f0, fo.u_target(om.x), bd, ALPHA, threads=usable_cores(), pc="bpx")
    ref = c_port.poisson_cycle_dst(n, 3, om.x, om.conn, np.asarray(fs[(steps - 1) % 3]), fo.u_target(om.x), bd, ALPHA)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    rec = {"workload": f"3-D linear Poisson, unit cube n={n}: {mesh.n_vert} DOFs, nnz {nnz}; the headline's operator cycle (host boundary, BPX-CG)",
           "n_dof": mesh.n_vert, "steps": steps, "ms_per_cycle": ms, "dofs_per_s": mesh.n_vert / (ms * 1e-3),
           "cg_iterations_per_cycle": [i["iterations"] for i in infos[:per]], "host_syncs_per_cycle": host_syncs,
           "roofline": _roofline("k_spmv_sell<1,true>", spmv_algorithmic_bytes(nnz, mesh.n_vert), spmv_ms, ns,
                                 "the matrix of this size (~140 MB stored) sits in the 256 MB Infinity Cache: an HBM fraction means little here",
                                 stored=stored_bytes(dm.info, mesh.n_vert), traffic_key="spmv_n100"),
           "check": _judge({"u_rel_err": rel(np.asarray(sim['u']), ref["u"]), "grad_rel_err": rel(np.asarray(E.host_wait(g)), ref["grad"]),
                            "against": "DST-exact cycle (oracle/c_port.py::poisson_cycle_dst)", "tolerance": 1e-10},
                           [("u_rel_err", "tolerance"), ("grad_rel_err", "tolerance")]),
           "cpu_baseline": {"value": om.n_vert / cpu["times"]["cycle"], "unit": "DOFs/s", "cores": int(cpu["threads"]), "kind": "port",
                            "sample": f"oracle/femo_oracle_c.c, one whole cycle at n={n} (this configuration's own size), "
                                      f"{cpu['times']['cycle']:.2f} s, CG its {cpu['it_fwd']}+{cpu['it_adj']}; nothing scaled"}}
    utils_hip.clear_workspaces()
    return rec


def bench_unstructured(ctx, n: int, steps: int = 3) -> dict:
    """The headline's cycle on the SAME cube with the numbering a foreign mesh has: vertices and
    cells renumbered at random (`Mesh.permuted`), then `Mesh.reordered()` -- what `import_mesh` does to a mesh it reads
    (Morton curve).  No lexicographic x-lines, hence no index-free "regular" SELL slices: the SpMV fetches its column
    indices and gathers through the caches.  Host boundary, same tolerances, same check (DST-exact cycle, vertex / cell
    numbering mapped back through the coordinates)."""
    import types
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    t0 = time.perf_counter()
    mesh = createUnitCubeMesh(n).permuted(seed=20240807).reordered()
    sim, fea = build_problem(mesh, device=False)
    dm = mesh.device(ctx)
    f_host = source_fields(mesh, 3)
    fs = [E.pinned_array(f) for f in f_host]
    u0 = E.pinned_full(mesh.n_vert, 0.0)
    _prime_pool(sim)             # AFTER the inputs took their blocks: the result generations must not meet an empty pool (a first
    #                              hipHostMalloc of 477 MB costs 60-90 ms and would land in the three timed cycles)
    setup_s = time.perf_counter() - t0
    for k in range(3):
        one_cycle(sim, fea, fs[k], u0)
    ctx.sync()
    del utils_hip.LAST_KSP_INFO[:]
    ms, g = _timed_cycles(ctx, lambda k: one_cycle(sim, fea, fs[k % 3], u0), steps, 0)
    infos = list(utils_hip.LAST_KSP_INFO)
    per = len(infos) // steps
    spmv_ms, ns = _spmv_in_loop(infos)
    nnz = dm.info["nnz"]
    kc = (steps - 1) % 3
    args = types.SimpleNamespace(n=n, jitter=0.0, permute=True, reorder=True)
    check = self_check(args, mesh, f_host[kc], np.array(sim['u'], copy=True), float(np.asarray(sim['l2_functional']).ravel()[0]),
                       np.array(E.host_wait(g), copy=True))
    rec = {"workload": f"the headline's cycle on the n={n} cube with random vertex / cell numbering renumbered by Mesh.reordered() (Morton curve), "
                       f"{mesh.n_vert} DOFs: the rate of an imported unstructured mesh; host boundary",
           "n_dof": mesh.n_vert, "steps": steps, "ms_per_cycle": ms, "dofs_per_s": mesh.n_vert / (ms * 1e-3), "setup_s": setup_s,
           "cg_iterations_per_cycle": [i["iterations"] for i in infos[:per]], "cg_ms_per_cycle": sum(i["solve_ms"] for i in infos) / steps,
           "sell_slices": dm.info["n_slices"], "regular_slices": dm.info["regular_slices"], "short_slices": dm.info.get("short_slices", 0),
           "roofline": _roofline("k_spmv_sell<1,true>", spmv_algorithmic_bytes(nnz, mesh.n_vert), spmv_ms, ns,
                                 "general slices: 16- or 32-bit column indices are fetched, x is gathered through L2 / Infinity Cache",
                                 stored=stored_bytes(dm.info, mesh.n_vert), traffic_key=f"spmv_n{n}_permuted_reordered"),
           "check": check}
    sim = fea = fs = u0 = g = None
    utils_hip.clear_workspaces()
    mesh._device = None
    return rec


def fenicsx_probe() -> dict:
    """is the reference's own stack on this box?  (Expected: no -- SURVEY.md section 8(c).)"""
    missing = []
    for name in ("dolfinx", "petsc4py", "ufl", "mpi4py"):
        try:
            __import__(name)
        except Exception as e:                                   # noqa: BLE001
            missing.append(f"{name}: {type(e).__name__}")
    return {"present": not missing, "detail": "importable" if not missing else "; ".join(missing),
            "consequence": "the CPU legs below are the in-repo restatement (oracle/), labelled kind 'port' / 'direct' -- not FEniCSx" if missing
                           else "dolfinx is importable: a FEniCSx CPU leg could be run on this box (not implemented: never observed)"}


def cpu_direct_legs(cube_n: int = 28) -> list:
    """the reference-FAITHFUL direct cycle on the host -- what femo does with MUMPS, restated
    with SciPy's SuperLU (oracle/femo_oracle.py::reference_cycle): Newton's three passes each assemble and FACTORISE
    (utils_dolfinx.py:419-449), the adjoint builds the transpose and factorises once more (fea_dolfinx.py:208-222 ->
    utils_dolfinx.py:476-493, 241-245).  Config 1 (64 x 64 square) and the largest cube whose cycle stays inside the time
    bound of this leg: sparse LU of a 3-D P1 operator fills as N^(4/3) and costs N^2 flops (10 s at 15.6 k DOFs, 57 s at 36 k,
    336 s at 69 k in the build container) -- the reason the 10 M-DOF configuration cannot be timed this way at all."""
    from oracle import femo_oracle as fo
    out = []
    for label, d, n in (("C1", 2, 64), ("cube", 3, cube_n)):
        m = fo.unit_square_mesh(n) if d == 2 else fo.unit_cube_mesh(n)
        bd = fo.boundary_vertices_box(m.x)
        f = fo.f_star(fo.centroids(m))
        t0 = time.perf_counter()
        fo.reference_cycle(m, f, fo.u_target(m.x), bd, np.zeros(len(bd)))
        t = time.perf_counter() - t0
        out.append({"config": label, "workload": f"{d}-D linear Poisson, n={n}: {m.n_vert} DOFs", "n_dof": int(m.n_vert), "seconds": t,
                    "value": m.n_vert / t, "unit": "DOFs/s", "cores": 1, "kind": "direct",
                    "sample": "oracle/femo_oracle.py::reference_cycle: NumPy assembly + scipy.sparse.linalg.splu, 3 factorisations (Newton) + 1 of the "
                              "transpose (adjoint), one core (SuperLU is serial; the reference's MUMPS is not installable here); measured at this size, nothing scaled"})
    return out


def _rss_mb() -> float:
    try:
        with open("/proc/self/statm") as fh:
            return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 1e6
    except Exception:
        return 0.0


def bench_distributed(args, rank: int, world: int, local_rank: int):
    """bench.py for N > 1: the 10 M-DOF mesh is partitioned over the ranks (strong scaling).
    Returns the result line on rank 0 (None elsewhere); bench.py prints it.  A rank that fails takes the job
    down instead of leaving the others in a barrier."""
    from femo_amd.dist import TorchControl
    from femo_amd.engine import Context
    from femo_amd.fea import utils_hip
    control = TorchControl(rank, world)
    try:
        ctx = Context(local_rank)
        utils_hip.set_context(ctx)
        control.init_comm(ctx)
        result = run_distributed_bench(args, ctx, control)
        control.barrier()
        return result
    except BaseException:                        # noqa: BLE001
        import sys
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)                              # torchrun tears the other ranks down


def run_distributed_bench(args, ctx, control, cpu_baseline: bool = True):
    """One rank's part of the N > 1 benchmark: rank-local mesh, the operator stack on it, the timed cycles,
    the JSON line on rank 0.  ``ctx`` already has its communicator (RCCL or emulated)."""
    import sys
    B = sys.modules[__name__]                                  # (moved out of femo_amd/dist: the package must not import its harness)
    from femo_amd.dist import local_unit_mesh, _grid
    from femo_amd.engine import Vec, host_wait as E_host_wait, pinned_array
    from femo_amd.fea import utils_hip

    rank, world = control.rank, control.world
    utils_hip.KSP_OPTIONS["pc"] = B.PC = getattr(args, "pc", "bpx")
    t0 = time.perf_counter()
    rss0 = _rss_mb()
    mesh = local_unit_mesh(args.n, 3, rank, world, jitter=getattr(args, "jitter", 0.0))
    mesh._occupancy = float(control.allreduce([mesh.lattice_occupancy()], "max")[0])    # one choice of preconditioner for all
    n_dof, n_cell_g = mesh.n_vert_global, mesh.n_cell_global
    # like N = 1: NumPy arrays at the operator boundary, every rank holding its own share of f, u and dJ/df in
    # pinned host memory (a distributed driver; each GPU has its own PCIe link)
    sim, fea = B.build_problem(mesh, device=False)
    dm = mesh.device(ctx)
    K, W = args.steps, args.warmup
    f_host = [pinned_array(f) for f in B.source_fields(mesh, min(K + W, 4))]
    from femo_amd.engine import pinned_full
    u0 = pinned_full(mesh.n_vert, 0.0)
    setup_s = time.perf_counter() - t0
    rss_setup = _rss_mb() - rss0

    # pinned pool sized during set-up (see bench.py: two generations of result blocks are alive at a time)
    from femo_amd.engine import pinned_empty
    n_f, n_u = int(np.size(sim['f'])), int(np.size(sim['u']))          # sizes of the arrays that cross the boundary
    prime = [pinned_empty(n_f) for _ in range(4)] + [pinned_empty(n_u) for _ in range(8)]
    del prime
    g = None
    for w in range(W):
        g = B.one_cycle(sim, fea, f_host[w % len(f_host)], u0)
    ctx.sync()
    control.barrier()
    if rank == 0:
        del utils_hip.LAST_KSP_INFO[:]
    control.barrier()
    ctx.comm_stats(reset=True)
    t0 = time.perf_counter()
    for k in range(K):
        g = B.one_cycle(sim, fea, f_host[(W + k) % len(f_host)], u0)   # the gradient is the caller's: held until replaced
    ctx.sync()
    control.barrier()
    elapsed = float(control.allreduce([time.perf_counter() - t0], "max")[0])
    comm = ctx.comm_stats()
    ms_per_step = elapsed / max(K, 1) * 1e3

    import threading
    me = threading.get_ident()                               # emulated ranks are threads sharing the module's log
    infos = [i for i in utils_hip.LAST_KSP_INFO if i.get("thread") == me]
    per = len(infos) // K if K else 0
    its_per_step = [i["iterations"] for i in infos[:per]]
    cg_ms = sum(i["solve_ms"] for i in infos) / max(K, 1)
    full = bool(getattr(args, "full", False))                # the SpMV roofline, the self-check and the CPU baseline: --full
    achieved = spmv_ms = float("nan")
    if full:
        A_mat = [w[1] for k, w in utils_hip._WORK.items() if k[1] == "newton_A" and w[0] is mesh][0].mat
        xv = Vec(ctx, mesh.n_vert).set(np.random.default_rng(rank).standard_normal(mesh.n_vert))
        yv = Vec(ctx, mesh.n_vert)
        control.barrier()
        spmv_ms = min(A_mat.bench_spmv(xv, yv, 50) for _ in range(3))      # local rows only, no halo: the kernel's own rate
    local_nnz = dm.info["nnz"]
    B_A = B.spmv_algorithmic_bytes(local_nnz, mesh.n_owned)
    if full:
        achieved = B_A / (spmv_ms * 1e-3) / 1e9
    L = mesh.local
    lat = dm.pc_info()
    hd = dm.halo_direct_info()
    # bytes a rank moves per CG iteration besides its HBM traffic: ghost values in and out, the lattice all-reduce
    halo_out, halo_in = int(L.send_ptr[-1]) * 8, int(L.recv_ptr[-1]) * 8
    stats = control.gather([mesh.n_owned, mesh.n_vert - mesh.n_owned, len(L.nbr), halo_out, halo_in, achieved, spmv_ms,
                            B.stored_bytes(dm.info, mesh.n_owned), rss_setup, setup_s])
    # ---- self-check of the partitioned run (outside the timed region): one more cycle; rank 0 computes the DST-exact
    # cycle of the WHOLE mesh (oracle/c_port.py::poisson_cycle_dst, no iterative solve), every rank compares the entries
    # it owns, the largest error over the ranks goes into the record.  Structured cube only.
    check = None
    if full and not getattr(args, "no_check", False) and not getattr(args, "jitter", 0.0):
        kc = (W + K) % len(f_host)
        g_chk = np.array(E_host_wait(B.one_cycle(sim, fea, f_host[kc], u0)), copy=True)
        u_chk = np.array(sim['u'], copy=True)
        n_cell_g = mesh.n_cell_global
        ref_u = ref_g = None
        if rank == 0:
            ref_u, ref_g = B.dst_reference_cycle(args.n, kc, min(K + W, 4))     # the checker lives with the harness, not in the package
        ref_u = control.broadcast(ref_u, n_dof)
        ref_g = control.broadcast(ref_g, n_cell_g)
        own_v, own_c = L.vert_global[:L.n_owned], L.cell_global[L.cell_owned]
        eu = float(np.abs(u_chk[:L.n_owned] - ref_u[own_v]).max()) if L.n_owned else 0.0
        eg = float(np.abs(g_chk[L.cell_owned] - ref_g[own_c]).max()) if own_c.size else 0.0
        errs = control.allreduce([eu, eg], "max")
        check = _judge({"u_rel_err": float(errs[0] / np.abs(ref_u).max()), "grad_rel_err": float(errs[1] / np.abs(ref_g).max()),
                        "tolerance": 1e-10, "norm": "max over all ranks' owned entries, relative to the largest entry",
                        "against": "DST-exact cycle of the whole mesh on rank 0 (oracle/c_port.py::poisson_cycle_dst)"},
                       [("u_rel_err", "tolerance"), ("grad_rel_err", "tolerance")])
        del ref_u, ref_g
    if rank != 0:
        return None
    result = {
        "metric": B.METRIC, "value": n_dof / (ms_per_step * 1e-3), "unit": "DOFs/s",
        "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {
            "workload": (f"3-D linear Poisson, P1 tets, unit cube n={args.n}: {n_dof} DOFs, {n_cell_g} cells, "
                         f"{world}-way block partition {'x'.join(str(g) for g in _grid(world))} (rank-local mesh generation), "
                         f"ghost-DOF halo ({'device-initiated: stores into the neighbours hipIpc-mapped inboxes + counters' if hd['enabled'] else 'ncclSend/Recv'}) "
                         f"+ RCCL all-reduce {B.PC.upper()}-CG; same cycle as N=1, every rank with "
                         f"NumPy arrays of its share of f, u and dJ/df at the operator boundary"),
            "boundary": "host (per rank: NumPy in pinned blocks; H2D + D2H inside the timed region)",
            "preconditioner": B.PC, "pc_lattice": lat,
            "n": args.n, "n_dof": n_dof, "n_cell": n_cell_g, "parallelism": f"block{world}",
            "owned_per_rank": [int(s[0]) for s in stats], "ghosts_per_rank": [int(s[1]) for s in stats],
            "neighbours_per_rank": [int(s[2]) for s in stats],
            "halo_bytes_sent_per_exchange_per_rank": [int(s[3]) for s in stats],
            "halo_bytes_received_per_exchange_per_rank": [int(s[4]) for s in stats],
            # counted on rank 0 over the timed cycles (femo_comm_stats); the merged loop issues one all-reduce and one
            # halo exchange per ENQUEUED iteration (batches: a few iterations behind the converged one are enqueued too)
            "allreduce_per_cg_iteration": (sum(i.get("loop_allreduces", 0) for i in infos) / max(sum(i["iterations"] for i in infos), 1)),
            "collectives_per_step_rank0": {k: v / max(K, 1) for k, v in comm.items()},
            "ghost_refresh_rank0": hd,          # {enabled, exchanges, consumer time-outs, producer workgroups} of the device-initiated plan (all zero: ncclSend/Recv)
            "allreduce_payload": "ONE ncclAllReduce per iteration: h on the lattice nodes SEVERAL ranks touch of the three brick-filled levels (L, L-1, L-2; sparse lists), "
                                 "level L-3 dense (restricted from the rank's partial sums before the exchange), 7 scalars (p.q, r.q, q.q, r.r, 3 single-rank lattice sums)",
            "linear_solves_per_step": per, "cg_iterations_per_step": its_per_step, "cg_ms_per_step": cg_ms,
            "non_cg_ms_per_step": ms_per_step - cg_ms,
            "setup_s_per_rank": [float(s[9]) for s in stats], "setup_rss_mb_per_rank": [float(s[8]) for s in stats],
        },
    }
    if full:
        result["roofline"] = {
            "bound": "hbm", "achieved": float(stats[0][7]) / (float(stats[0][6]) * 1e-3) / 1e9, "peak": B.HBM_PEAK_GBS, "unit": "GB/s",
            "frac": float(stats[0][7]) / (float(stats[0][6]) * 1e-3) / 1e9 / B.HBM_PEAK_GBS, "traffic": None,
            "achieved_algorithmic": float(stats[0][5]), "frac_algorithmic": float(stats[0][5]) / B.HBM_PEAK_GBS,
            "frac_physical": float(stats[0][7]) / (float(stats[0][6]) * 1e-3) / 1e9 / B.HBM_PEAK_GBS,
            "physical_bytes_per_launch": float(stats[0][7]),
            "physical_bytes_source": "stored bytes of the SELL format (no PMC pass at N > 1)",
            "kernel": "k_spmv_sell<1,true> on rank 0's local rows (per GPU), 150 back-to-back launches",
            "algorithmic_bytes_per_launch": B_A, "avg_launch_ms": float(stats[0][6]), "launches_timed": 150,
            "achieved_per_rank": [float(s[5]) for s in stats],
        }
    if check is not None:
        result["check"] = check
    if full and cpu_baseline and not getattr(args, "no_cpu_baseline", False):
        counts = its_per_step if its_per_step else [0]
        n = args.n
        nnz = n_dof + 2 * (3 * n * (n + 1) ** 2 + 3 * n * n * (n + 1) + n ** 3)
        result["cpu_baseline"] = B.cpu_baseline(args, counts, n_dof, n_cell_g, nnz)
    return result


def _block_leg(ctx, mesh, steps: int) -> dict:
    """The headline's operator cycle on one block mesh (host boundary): ms per cycle, CG counts, wall time per iteration."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    sim, fea = build_problem(mesh, device=False)
    dm = mesh.device(ctx)
    fs = [E.pinned_array(f) for f in source_fields(mesh, 3)]
    u0 = E.pinned_full(mesh.n_vert, 0.0)
    _prime_pool(sim)                                                  # after the inputs took their blocks (see bench_unstructured)
    for k in range(3):
        one_cycle(sim, fea, fs[k], u0)
    ctx.sync()
    del utils_hip.LAST_KSP_INFO[:]
    ctx.comm_stats(reset=True)
    E.host_syncs(reset=True)
    ms, _ = _timed_cycles(ctx, lambda k: one_cycle(sim, fea, fs[k % 3], u0), steps, 0)
    host_syncs = (E.host_syncs() - 1) / steps
    comm = ctx.comm_stats()
    infos = list(utils_hip.LAST_KSP_INFO)
    per = len(infos) // steps
    its = [i["iterations"] for i in infos[:per]]
    solves = [i for i in infos if i["iterations"] > 0]
    n_it = max(sum(i["iterations"] for i in solves), 1)
    us_per_it = 1e3 * sum(i["solve_ms"] for i in solves) / n_it
    spmv_ms, ns = _spmv_in_loop(infos)
    cg_ms = sum(i["solve_ms"] for i in infos) / steps
    lat = dm.pc_info()
    out = {"n_vert": int(mesh.n_vert), "ms_per_cycle": ms, "cg_iterations_per_cycle": its, "cg_ms_per_cycle": cg_ms,
           "non_cg_ms_per_cycle": ms - cg_ms, "us_per_cg_iteration_wall": us_per_it, "spmv_us": spmv_ms * 1e3 if ns else None,
           "host_syncs_per_cycle": host_syncs, "halo": dm.halo_direct_info() if hasattr(dm, "halo_direct_info") else None,
           "pc_lattice": lat,
           "collectives_per_cycle": {k: v / steps for k, v in comm.items()},
           "allreduce_per_cg_iteration": sum(i.get("loop_allreduces", 0) for i in infos) / n_it,
           "allreduce_doubles_per_call_in_loop": None}
    loop_calls = sum(i.get("loop_allreduces", 0) for i in infos)
    if loop_calls:
        # the loop's all-reduces dominate the count; the handful outside it (Newton's norms, J) carry <= 8 doubles each
        out["allreduce_doubles_per_call_in_loop"] = comm["allreduce_doubles"] / max(comm["allreduce_calls"], 1)
    utils_hip.clear_workspaces()
    return out


def bench_scaling_model(ctx, n_global: int, steps: int, headline_ms: float, headline_split: dict, one_rank_leg: bool = True,
                        global_its=None, model_rank: int = 2) -> dict:
    """What one rank of the 8-GPU run does, measured on THIS GPU (VERDICT rounds 3 and 4: "prove the budget on one GPU").

    Round 5: the leg runs the N-RANK CODE PATH.  A second context on the same device gets a *model communicator*
    (femo_comm_model, include/femo_hip_test.h): it is rank 0 of 8, so the library takes every partitioned-mesh branch -- the
    rank-local mesh of `bench.py --gpus 8` (femo_amd/dist/structured.py: the 108^3 block + one layer of ghost cells, the
    halo plan towards its 7 neighbours), the split interior / boundary SpMV with the halo pack on the communication stream,
    the pack kernel of the merged BPX-PCG loop, the sparse lattice lists, the whole mesh's lattice -- while every collective
    completes at once without moving a byte.  Everything a rank does per iteration is therefore inside the measured time
    EXCEPT the time on the wire; the projection adds an assumed latency for the one all-reduce and for the part of the halo
    exchange the interior SpMV does not cover, and says so.  (The numbers the leg computes are those of the block with zero
    ghost values, not of the global problem; the emulated-rank tests and `bench.py --gpus N` check the real thing.)
    `one_rank_loop_on_block` repeats round 4's measurement (the block as a mesh of its own through the one-rank loop)."""
    from femo_amd.dist import local_unit_mesh
    from femo_amd.engine import Context
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh
    nb = (n_global + 1) // 2
    n_dof_global = (n_global + 1) ** 3
    # (1) round 4's leg: the block alone, one-rank loop, whole-mesh lattice
    one = None
    if one_rank_leg:
        mesh1 = createUnitCubeMesh(nb)
        mesh1.x *= nb / n_global                                      # the block [0, nb h]^3 of the n-cube
        if hasattr(mesh1, "n"):
            mesh1.n = 0                                               # source_fields: evaluate point by point
        mesh1.device(ctx).set_global(np.zeros(3), np.ones(3), n_dof_global)
        one = _block_leg(ctx, mesh1, max(steps // 2, 3))
        mesh1._device = None
        del mesh1
    # (2) the N-rank path under the model communicator
    # rank 2 of the 1 x 2 x 4 pencils: one cut y-face and two cut z-faces, the largest halo of the eight
    ctx8 = Context(ctx.device if hasattr(ctx, "device") else 0)
    ctx8.comm_model(model_rank, 8)
    utils_hip.set_context(ctx8)
    try:
        mesh8 = local_unit_mesh(n_global, 3, model_rank, 8)
        leg = _block_leg(ctx8, mesh8, steps)
        L = mesh8.local
        halo = {"neighbours": int(len(L.nbr)), "ghosts": int(mesh8.n_vert - mesh8.n_owned),
                "bytes_sent_per_exchange": int(L.send_ptr[-1]) * 8, "bytes_received_per_exchange": int(L.recv_ptr[-1]) * 8}
        n_owned = int(mesh8.n_owned)
        mesh8._device = None
        del mesh8
    finally:
        utils_hip.set_context(ctx)
    ms_measured, us_per_it, its_model = leg["ms_per_cycle"], leg["us_per_cg_iteration_wall"], sum(leg["cg_iterations_per_cycle"])
    # The block with zero ghost values is a different (harder) problem than the global one: its CG counts are not those of a
    # rank of the real job, which runs the GLOBAL iteration (the emulated 8-rank run at this size reproduces the one-GPU counts
    # exactly, profiles/r04_emulated_8ranks_n215.json).  The cycle a real rank runs = this leg's work outside the loops + the
    # global iteration counts at this leg's measured cost per iteration.
    its_total = int(sum(global_its)) if global_its else its_model
    ms = leg["non_cg_ms_per_cycle"] + its_total * us_per_it * 1e-3
    ar_doubles = leg["allreduce_doubles_per_call_in_loop"]
    proj = {}
    # What of the ghost refresh stays exposed on the wire.  ncclSend/Recv-shaped path (round 5): +10 us per iteration, as
    # before.  Device-initiated path (round 6): the stores into the neighbours' inboxes are issued by the FIRST workgroups of
    # the prolongation launch and consumed by the waves of the boundary slices at the END of the next product -- the bulk of
    # the prolongation and the interior slices (>= 14 + 27 us on this block, see the timeline in profiles/) lie in between,
    # against ~117 KB per neighbour over a dedicated xGMI link (~2.5 us at 50 GB/s + a few us of latency): priced at 0.
    direct = bool((leg.get("halo") or {}).get("enabled"))
    halo_exposed_us = 0.0 if direct else 10.0
    for lat_us in (15.0, 30.0, 60.0):
        t_it = us_per_it + lat_us + halo_exposed_us       # + one all-reduce on the wire + the exposed part of one halo exchange
        cyc = ms + its_total * (t_it - us_per_it) * 1e-3
        proj[f"allreduce_{int(lat_us)}us"] = {"us_per_iteration": t_it, "ms_per_cycle": cyc, "speedup_vs_1gpu": headline_ms / cyc}
    return {"what": f"rank {model_rank} of the 1x2x4 partition of the headline mesh, run alone on this GPU through the N-rank code path (model communicator: "
                    "collectives counted, nothing on the wire), whole-mesh lattice",
            "block": f"{nb}^3 cells, {n_owned} owned DOFs + {halo['ghosts']} ghosts (1/8 of {n_dof_global} + interface)", "halo": halo,
            "pc_lattice": leg["pc_lattice"],
            "ms_per_cycle_block": ms, "ms_per_cycle_block_how": "non-CG time of the leg + the GLOBAL CG counts x the leg's measured wall time per iteration",
            "cg_iterations_global": list(global_its) if global_its else None,
            "ms_per_cycle_measured_on_the_model_problem": ms_measured,
            "cg_iterations_per_cycle": leg["cg_iterations_per_cycle"], "cg_ms_per_cycle": leg["cg_ms_per_cycle"],
            "non_cg_ms_per_cycle": leg["non_cg_ms_per_cycle"],
            "us_per_cg_iteration_wall": us_per_it, "spmv_us": leg["spmv_us"], "host_syncs_per_cycle": leg["host_syncs_per_cycle"],
            "ghost_refresh": ("device-initiated (stores into the neighbours' inboxes + counters, include/femo_hip.h ABI 9; here against the rank's own scratch: "
                              "loopback of the model communicator)" if (leg.get("halo") or {}).get("enabled") else "ncclSend/ncclRecv-shaped (comm stream + events)"),
            "ghost_refresh_info": leg.get("halo"),
            "launches_per_cg_iteration": {"one_rank": 5, "n_ranks": 6 if direct else 8,
                                          "kernels": ("device-initiated ghost refresh (round 6), ONE stream: SpMV (interior slices, then the slices with ghost columns: their waves wait "
                                                      "for the neighbours' counters and read the inbox), brick restriction of q, pack (shared lattice nodes of three levels + R h_T + 7 "
                                                      "scalars), [ncclAllReduce], coarse lattice + vector updates, fine lattice (own tiles), mesh prolongation (send vertices first: stores "
                                                      "into the neighbours' inboxes + counter bumps)") if direct else
                                                     ("SpMV over the interior slices, [halo event], SpMV over the boundary slices, brick restriction of q, pack, [ncclAllReduce], coarse lattice "
                                                      "+ vector updates, fine lattice, mesh prolongation on the send vertices, [ncclSend/Recv on the comm stream], mesh prolongation")},
            "collectives_per_cg_iteration": {"allreduce": leg["allreduce_per_cg_iteration"], "halo_exchange": 1,
                                             "allreduce_doubles": ar_doubles,
                                             "round4_allreduce_doubles": 138000,
                                             "counted_by": "femo_comm_stats on the model communicator (this leg), on emulated ranks (tests/test_gpu_emulated_ranks.py) and in the bench.py --gpus N record"},
            "collectives_per_cycle": leg["collectives_per_cycle"],
            "one_rank_loop_on_block": None if one is None else {k: one[k] for k in ("n_vert", "ms_per_cycle", "cg_iterations_per_cycle", "us_per_cg_iteration_wall", "spmv_us", "non_cg_ms_per_cycle")},
            "headline_1gpu_ms": headline_ms,
            "ideal_speedup_without_communication": headline_ms / ms,
            "projection": proj,
            "halo_exposed_us_assumed": halo_exposed_us,
            "assumptions": "each rank has its own PCIe link (the block's transfers are inside ms_per_cycle_block); per iteration the stated all-reduce "
                           "latency (the pack launch and the host enqueue of the collectives are measured, the wire is not) and halo_exposed_us_assumed of ghost "
                           "refresh not hidden (0 with the device-initiated refresh: its stores have the bulk of the prolongation and the interior slices "
                           "of the product, > 40 us, to cross a dedicated link; 10 with ncclSend/Recv); the collectives outside the CG loops (a dozen scalar "
                           "all-reduces and halo refreshes per cycle) are not priced; no multi-GPU box was available: wire latencies are assumptions, "
                           "everything else is measured"}


def build_problem_nl(mesh, device: bool = False):
    """examples/nonlinear_poisson_opt/run_nonlinear_poisson_opt.py:147-232 on the HIP mirror (symmetric Nitsche, SNES)."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import FEA, Function, FunctionSpace, TestFunction
    from femo_amd.fea.nonlinear_poisson import outputForm as outputFormNL, pdeRes as pdeResNL
    fea = FEA(mesh)
    fea.REPORT = False
    Vf, Vu = FunctionSpace(mesh, ('DG', 0)), FunctionSpace(mesh, ('CG', 1))
    f_fn, u_fn = Function(Vf), Function(Vu)
    u_ex = Function(Vu)
    u_ex.interpolate(lambda x: np.sin(2 * np.pi * x[0]) * np.sin(np.pi * x[1]))
    fea.add_input('f', f_fn)
    fea.add_state(name='u', function=u_fn, residual_form=pdeResNL(u_fn, TestFunction(Vu), f_fn, u_exact=u_ex, weak_bc=True, sym=True),
                  arguments=['f'])
    fea.add_output(name='l2_functional', type='scalar', form=outputFormNL(u_fn, f_fn, u_ex), arguments=['f', 'u'])
    fea.PDE_SOLVER = 'SNES'
    model = FEAModel(fea=[fea])
    model.create_input('f', shape=fea.inputs_dict['f']['shape'], val=0.1)
    return Simulator(model, device=device), fea


def bench_scaling_model_c5(ctx, steps: int, one_gpu: dict, n: int = 2236, world: int = 4, model_rank: int = 1) -> dict:
    """BASELINE config 5 is a 4-GPU configuration: what ONE of its four ranks does, measured on this GPU like `scaling_model`
    (model communicator, N-rank code path, nothing on the wire): rank 1 of the 1 x 4 slabs of the n x n square (two cut faces),
    the whole mesh's 2-D lattice, the nonlinear Poisson + Nitsche cycle of `configs.c5_nl`.  The projection uses the one-GPU
    leg's Newton / CG counts (a rank of the real job runs the global iteration: tests/test_gpu_emulated_ranks.py::
    test_nonlinear_cycle_on_four_emulated_ranks) at this leg's measured cost per iteration."""
    from femo_amd import engine as E
    from femo_amd.dist import local_unit_mesh
    from femo_amd.engine import Context
    from femo_amd.fea import utils_hip
    ctx4 = Context(ctx.device if hasattr(ctx, "device") else 0)
    ctx4.comm_model(model_rank, world)
    utils_hip.set_context(ctx4)
    try:
        mesh = local_unit_mesh(n, 2, model_rank, world)
        sim, fea = build_problem_nl(mesh)
        dm = mesh.device(ctx4)
        xc = mesh.centroids()
        fs = [E.pinned_array(0.1 * (1.0 + 0.2 * np.sin(np.pi * (k + 1) * xc[:, 0]) * xc[:, 1])) for k in range(3)]
        u1 = E.pinned_full(mesh.n_vert, 1.0)
        _prime_pool(sim)
        ufn = fea.states_dict['u']['function']

        def cycle(k):
            sim['f'] = fs[k % 3]
            ufn.vector.set(1.0)
            sim['u'] = u1
            sim.run()
            return sim.compute_totals('l2_functional', 'f')

        for k in range(2):
            cycle(k)
        ctx4.sync()
        del utils_hip.LAST_KSP_INFO[:]
        ctx4.comm_stats(reset=True)
        ms_model, _ = _timed_cycles(ctx4, cycle, steps, 0)
        comm = ctx4.comm_stats()
        infos = list(utils_hip.LAST_KSP_INFO)
        per = len(infos) // steps
        its_model = [i["iterations"] for i in infos[:per]]
        solves = [i for i in infos if i["iterations"] > 0]
        n_it = max(sum(i["iterations"] for i in solves), 1)
        us_per_it = 1e3 * sum(i["solve_ms"] for i in solves) / n_it
        non_cg = ms_model - sum(i["solve_ms"] for i in infos) / steps
        lat = dm.pc_info()
        L = mesh.local
        hd = dm.halo_direct_info()
        halo = {"neighbours": int(len(L.nbr)), "ghosts": int(mesh.n_vert - mesh.n_owned), "bytes_sent_per_exchange": int(L.send_ptr[-1]) * 8,
                "device_initiated": bool(hd["enabled"]), "consumer_timeouts": hd["timeouts"]}
        n_owned = int(mesh.n_owned)
        utils_hip.clear_workspaces()
        mesh._device = None
    finally:
        utils_hip.set_context(ctx)
    its_global = list(one_gpu.get("cg_iterations_per_cycle") or [])
    n_global = int(sum(its_global)) if its_global else n_it // max(steps, 1)
    ms = non_cg + n_global * us_per_it * 1e-3
    proj = {}
    halo_exposed_us = 0.0 if halo["device_initiated"] else 10.0        # as in scaling_model
    for lat_us in (15.0, 30.0, 60.0):
        cyc = ms + n_global * (lat_us + halo_exposed_us) * 1e-3
        proj[f"allreduce_{int(lat_us)}us"] = {"ms_per_cycle": cyc, "speedup_vs_1gpu": one_gpu["ms_per_cycle"] / cyc}
    return {"what": f"rank {model_rank} of the 1x{world} slabs of the n = {n} square (BASELINE config 5: 4 GPUs), run alone on this GPU through the N-rank code path "
                    "(model communicator), whole-mesh 2-D lattice", "owned_dofs": n_owned, "halo": halo, "pc_lattice": lat,
            "ms_per_cycle_block": ms, "ms_per_cycle_block_how": "non-CG time of the leg + the one-GPU leg's CG counts x this leg's measured wall time per iteration",
            "ms_per_cycle_measured_on_the_model_problem": ms_model, "cg_iterations_model_problem": its_model, "cg_iterations_global": its_global,
            "us_per_cg_iteration_wall": us_per_it, "non_cg_ms_per_cycle": non_cg,
            "coarse_lattice_kernel": "2-D: the single-workgroup kernel of the merged loop keeps every level below T-1 in LDS (k_lattice_coarse_m, the same launch as in 3-D); "
                                     "its cost is inside us_per_cg_iteration_wall",
            "collectives_per_cycle": {k: v / steps for k, v in comm.items()},
            "one_gpu_ms_per_cycle": one_gpu["ms_per_cycle"], "ideal_speedup_without_communication": one_gpu["ms_per_cycle"] / ms,
            "projection": proj,
            "halo_exposed_us_assumed": halo_exposed_us,
            "assumptions": "as scaling_model: the stated all-reduce latency and halo_exposed_us_assumed of exposed ghost refresh per iteration; collectives outside the CG loops not priced"}


def bench_config5(ctx, steps: int, n: int = 2236) -> dict:
    """BASELINE config 5 on one GPU: -div grad u + u^3 = f with symmetric Nitsche terms on the n x n square
    (n = 2236: 5,004,169 DOFs), SNES (Jacobian reassembled every Newton iteration) + adjoint-of-Newton gradient, NumPy
    arrays at the operator boundary, cold start from CSDL's default state u = 1 in every cycle."""
    from femo_amd import engine as E
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitSquareMesh
    mesh = createUnitSquareMesh(n)
    sim, fea = build_problem_nl(mesh)
    dm = mesh.device(ctx)
    xc = mesh.centroids()
    fs = [E.pinned_array(0.1 * (1.0 + 0.2 * np.sin(np.pi * (k + 1) * xc[:, 0]) * xc[:, 1])) for k in range(3)]   # run_nonlinear...:230-232: f = 0.1
    u1 = E.pinned_full(mesh.n_vert, 1.0)
    _prime_pool(sim)
    ufn = fea.states_dict['u']['function']

    def cycle(k):
        sim['f'] = fs[k % 3]
        ufn.vector.set(1.0)
        sim['u'] = u1
        sim.run()
        return sim.compute_totals('l2_functional', 'f')

    for k in range(2):
        cycle(k)
    ctx.sync()
    del utils_hip.LAST_KSP_INFO[:]
    ms, g = _timed_cycles(ctx, cycle, steps, 0)
    infos = list(utils_hip.LAST_KSP_INFO)
    per = len(infos) // steps
    spmv_ms, ns = _spmv_in_loop(infos)
    nnz = dm.info["nnz"]
    J = float(np.asarray(sim['l2_functional']).ravel()[0])
    # ---- self-check of this configuration (outside the timed region; the properties of
    # tests/test_gpu_round2.py::test_config5_full_size_properties): stationarity of the returned state, the adjoint total
    # against a directional central difference of J, the adjoint identity on the Jacobian of the converged state
    f0 = np.asarray(fs[(steps - 1) % 3])
    g_last = np.array(E.host_wait(g), copy=True)
    res_form = fea.states_dict['u']['residual_form']
    r_state = np.asarray(E.host_wait(utils_hip.assembleVector(res_form)))
    u_state = np.asarray(sim['u'])
    stationarity = float(np.abs(r_state).max() / max(1.0, np.abs(u_state).max()))
    d = np.cos(3.0 * xc[:, 0]) * np.sin(2.0 * xc[:, 1]) + 0.3
    Jd = []
    for sgn in (+1.0, -1.0):
        sim['f'] = f0 + sgn * 1e-3 * d
        ufn.vector.set(1.0)
        sim['u'] = u1
        sim.run()
        Jd.append(float(np.asarray(sim['l2_functional']).ravel()[0]))
    fd, an = (Jd[0] - Jd[1]) / 2e-3, float(g_last @ d)
    sim['f'] = f0
    ufn.vector.set(1.0)
    sim['u'] = u1
    sim.run()
    op = [o for _, o in sim.ops if hasattr(o, 'apply_inverse_jacobian')][0]
    op.compute_derivatives({'f': sim.values['f']}, {'u': sim.values['u']}, {})
    rng = np.random.default_rng(1)
    N = mesh.n_vert
    bv, cv = E.Vec(ctx, N).set(rng.standard_normal(N)), E.Vec(ctx, N).set(rng.standard_normal(N))
    xb, xcv = E.Vec(ctx, N), E.Vec(ctx, N)
    op.A.mat.solve_cg(bv, xb, rtol=1e-12, pc="bpx")
    op.A.mat.solve_cg(cv, xcv, rtol=1e-12, pc="bpx")
    lhs, rhs = xb.dot(cv), bv.dot(xcv)
    check = {"stationarity_residual_over_state": stationarity, "stationarity_tolerance": 1e-9,
             "gradient_vs_central_difference_rel": float(abs(an - fd) / abs(fd)), "gradient_tolerance": 5e-5,
             "adjoint_identity_rel": float(abs(lhs - rhs) / abs(lhs)), "adjoint_identity_tolerance": 1e-9,
             "against": "properties of the configuration itself (no closed form for the nonlinear problem): R(u) = 0 at the returned state, "
                        "dJ/df . d against (J(f + eps d) - J(f - eps d)) / 2 eps, <A^-1 b, c> = <b, A^-T c> on the converged Jacobian"}
    _judge(check, [("stationarity_residual_over_state", "stationarity_tolerance"), ("gradient_vs_central_difference_rel", "gradient_tolerance"),
                   ("adjoint_identity_rel", "adjoint_identity_tolerance")])
    del bv, cv, xb, xcv
    # CPU (round 5; VERDICT round 4, missing #2): the C/OpenMP port's cycle -- the same algorithm (SNES, Jacobian reassembled every
    # Newton step, BPX-preconditioned CG with the engine's stopping rules, adjoint solve) at THIS configuration's own size on all
    # host cores (oracle/c_port.py::nl_cycle).  Rounds 1-4 timed the NumPy / SuperLU oracle on one core at 148 k DOFs.
    from oracle import c_port
    c_port.use_native()            # the port compiled for THIS box's CPU when gcc is here (the shipped .so is x86-64-v3)
    from oracle import femo_oracle as fo
    x_h, conn_h = np.ascontiguousarray(mesh.x), np.ascontiguousarray(mesh.conn)
    bmask = np.ascontiguousarray(mesh.boundary_facet_mask(), dtype=np.uint8)
    c_port.lib().oc_set_num_threads(usable_cores())
    t0 = time.perf_counter()
    out = c_port.nl_cycle(2, x_h, conn_h, np.asarray(fs[0]), fo.u_exact_nl(x_h), bmask, fo.ALPHA_NL)
    t_cpu = out["times"]["cycle"]
    # the port is a checker too: state and gradient of the GPU's cycle for the same f (outside the timed region)
    sim['f'] = fs[0]
    ufn.vector.set(1.0)
    sim['u'] = u1
    sim.run()
    g_chk = np.array(E.host_wait(sim.compute_totals('l2_functional', 'f')), copy=True)
    relx = lambda a, b: float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())
    check["u_vs_c_port_rel"] = relx(sim['u'], out["u"])
    check["grad_vs_c_port_rel"] = relx(g_chk, out["grad"])
    check["c_port_tolerance"] = 1e-8
    check["c_port_note"] = ("two independent iterative solves of the same discrete problem (the port's CG stops at 1e-11 in the preconditioner's "
                            "norm as well): agreement to solver accuracy, not to round-off")
    _judge(check, [("stationarity_residual_over_state", "stationarity_tolerance"), ("gradient_vs_central_difference_rel", "gradient_tolerance"),
                   ("adjoint_identity_rel", "adjoint_identity_tolerance"), ("u_vs_c_port_rel", "c_port_tolerance"), ("grad_vs_c_port_rel", "c_port_tolerance")])
    del g_chk
    rec = {"workload": f"nonlinear Poisson + symmetric Nitsche, unit square n={n}: {mesh.n_vert} DOFs, nnz {nnz}; SNES from u = 1, "
                       "J, dJ/du, dJ/df, dR/du, dR/df, A, transposed solve, dR/df^T lambda; host boundary",
           "n_dof": mesh.n_vert, "steps": steps, "ms_per_cycle": ms, "dofs_per_s": mesh.n_vert / (ms * 1e-3),
           "newton_linear_solves_per_cycle": per - 1, "cg_iterations_per_cycle": [i["iterations"] for i in infos[:per]],
           "J": J, "roofline": _roofline("k_spmv_sell<1,true>", spmv_algorithmic_bytes(nnz, mesh.n_vert), spmv_ms, ns,
                                         stored=stored_bytes(dm.info, mesh.n_vert), traffic_key=f"spmv_sq{n}"),
           "check": check,
           "cpu_baseline": {"value": mesh.n_vert / t_cpu, "unit": "DOFs/s", "cores": int(out["threads"]), "kind": "port",
                            "sample": f"oracle/femo_oracle_c.c + oracle/c_port.py::nl_cycle: one whole cycle at n={n} (this configuration's own size, "
                                      f"{mesh.n_vert} DOFs), {out['newton_its']} Newton steps, CG its {out['it_fwd']} + {out['it_adj']}, {t_cpu:.1f} s on "
                                      f"{out['threads']} cores; nothing scaled"}}
    utils_hip.clear_workspaces()
    return rec


def bench_config3(ctx, steps: int, n: int = 362, cpu_n: int = 64) -> dict:
    """BASELINE config 3: Reissner-Mindlin shell (CG2^3 x CG1^3), Scordelis-Lo roof n x n x 2 triangles (n = 362:
    1.97 M dofs): assemble K(h), solve K w = F, compliance + dJ/dw, adjoint solve, thickness sensitivity dJ/dh."""
    from femo_amd import engine as E
    from femo_amd.fea.mesh import createCylindricalRoofMesh, roof_quarter_model_dofs
    from femo_amd.fea.shell import ShellProblem
    Lr = 25.0
    E.host_trim()
    pts, conn = createCylindricalRoofMesh(n, n, L=Lr)
    t0 = time.perf_counter()
    from femo_amd.fea.shell import ShellSpace
    S = ShellSpace(pts, conn)
    prob = ShellProblem(pts, conn, 4.32e8, 0.0, fixed_dofs=roof_quarter_model_dofs(S, Lr), ctx=ctx)
    prob.dev.enable_lattice_pc()
    setup_s = time.perf_counter() - t0
    vx = S.x
    prob.set_load([0.0, 0.0, -90.0])
    free = ~prob.fixed.astype(bool)
    fixed_idx = np.flatnonzero(~free)                  # the imposed dofs (a few thousand of 1.97 M): indexed, not masked, inside the cycle
    its, spmv_ms, spmv_n = [], 0.0, 0

    def cycle(k):
        nonlocal spmv_ms, spmv_n
        prob.set_thickness(0.25 * (1.0 + 0.02 * np.cos(2 * np.pi * (k + 1) * vx[:, 0] / Lr)))     # a new K every cycle
        w = prob.solve(rtol=1e-10)
        i1 = prob.last_info
        J, dJdw = prob.compliance(grad=True)
        dJdw[fixed_idx] = 0.0
        lam = prob.solve_adjoint(dJdw, rtol=1e-10)
        i2 = prob.last_info
        g = -prob.dRdh_T(lam)
        its.append([int(i1.iterations), int(i2.iterations)])
        spmv_ms += i1.spmv_ms + i2.spmv_ms
        spmv_n += i1.spmv_samples + i2.spmv_samples
        return w, J, g

    cycle(0)
    ctx.sync()
    its.clear(); spmv_ms = 0.0; spmv_n = 0
    t0 = time.perf_counter()
    for k in range(steps):
        w, J, g = cycle(k + 1)
    ctx.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    tip = int(np.argmin(np.abs(vx[:, 0]) + np.abs(vx[:, 1] - vx[:, 1].max())))
    # block-SELL bytes of the operator product: 9 values + 1 column index per 3 x 3 block, x and y once
    nblk = int(prob.dev.nnz) // 9
    b_spmv = nblk * (72 + 4) + 2 * 8 * int(S.n_dof)
    # ---- self-check (outside the timed region): residual of the returned state on the free dofs over the scale of the
    # load, the adjoint identity <w, c> = <F, mu> with mu = K^-1 c (one more solve), the tip deflection against the one
    # shell number the reference tree holds (run_shape_opt_roof.py:224; the thickness of the timed cycles varies by 2 %)
    w_h = np.asarray(w)
    r_all = prob.residual(w_h)
    r_free, reaction = r_all[free], float(np.abs(r_all[~free]).max())         # the reactions on the imposed dofs: the scale of the forces
    Fh = np.array(prob.F.get()); Fh[~free] = 0.0
    rng = np.random.default_rng(5)
    cvec = rng.standard_normal(S.n_dof); cvec[~free] = 0.0
    mu = prob.solve_adjoint(cvec, rtol=1e-10)
    lhs, rhs = float(w_h @ cvec), float(Fh @ mu)
    tip_w = float(S.vertex_displacement(w_h)[tip, 2])
    # (round 5: 1e-8, was 1e-7 -- the observed 2-3e-10 leave more than a decade; eps * cond(K) of the thin shell is what stands between these and 1e-10)
    check = {"free_dof_residual_over_reactions": float(np.abs(r_free).max() / reaction), "residual_tolerance": 1e-8,
             "adjoint_identity_rel": float(abs(lhs - rhs) / abs(lhs)), "adjoint_identity_tolerance": 1e-8,
             "tip_deflection_rel_to_reference": float(abs(tip_w + 0.3024) / 0.3024), "tip_tolerance": 0.01,
             "lattice_spaces": "Hermite-type" if prob.dev.pc_state()["hermite_in_use"] else "trilinear",    # the device's state, not the request
             "against": "properties of the configuration itself: K w = F on the free dofs (against the reaction forces on the imposed ones), <w, c> = <F, K^-1 c>, Scordelis-Lo tip deflection -0.3024 "
                        "(tolerances follow eps * cond(K) ~ 1e-8 of a thin shell, DESIGN.md section 8)"}
    _judge(check, [("free_dof_residual_over_reactions", "residual_tolerance"), ("adjoint_identity_rel", "adjoint_identity_tolerance"),
                   ("tip_deflection_rel_to_reference", "tip_tolerance")])
    # CPU: the oracle's direct-solver cycle (the reference factorises: 3 Newton steps + 1 adjoint factorisation)
    from oracle import shell_oracle as so
    t0 = time.perf_counter()
    cpu = so.reference_cycle(cpu_n)
    t_cpu = time.perf_counter() - t0
    return {"workload": f"Reissner-Mindlin shell, Scordelis-Lo roof {n} x {n} x 2 triangles: {S.n_dof} dofs, nnz {int(prob.dev.nnz)}; assemble K(h), "
                        "PCG solve, compliance + dJ/dw, adjoint PCG solve, dJ/dh; NumPy arrays in and out",
            "n_dof": int(S.n_dof), "steps": steps, "ms_per_cycle": ms, "dofs_per_s": S.n_dof / (ms * 1e-3), "setup_s": setup_s,
            "cg_iterations_per_cycle": its[-1], "tip_deflection": tip_w, "tip_reference": -0.3024,
            "roofline": _roofline("k_bsell_spmv", b_spmv, spmv_ms / max(spmv_n, 1), spmv_n,
                                  "bytes in the block-SELL format the kernel reads (8.44 B per scalar entry), not scalar-CSR bytes: the "
                                  "algorithmic and the stored count coincide", stored=b_spmv, traffic_key="bsell_spmv_n362" if n == 362 else ""),
            "check": check,
            "cpu_baseline": {"value": cpu["n_dof"] / t_cpu, "unit": "DOFs/s", "cores": 1, "kind": "port",
                             "sample": f"oracle/shell_oracle.py::reference_cycle (NumPy assembly, SciPy SuperLU: 3 Newton factorisations + 1 for the "
                                       f"adjoint, as the reference's MUMPS path does) on the {cpu_n} x {cpu_n} roof, {cpu['n_dof']} dofs, {t_cpu:.1f} s; "
                                       "measured at that size, nothing scaled.  The size is set by the time bound of the baseline leg, not by memory: "
                                       "the cycle factorises four times with SuperLU (COLAMD; MMD orderings are slower on this matrix) -- 20 s at n = 48, "
                                       "47 s at n = 64, 216 s at n = 96 (140 k dofs) in the build container; the reference's MUMPS is not installable here"}}


def _relaunch_multi_gpu(args) -> int:
    """``python bench.py --gpus N`` without a launcher: start the N ranks as a child torchrun job
    (before anything here touches the GPU) and pass its output and exit code on."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd).returncode


def main():
    global PC
    args = parse()
    PC = args.pc
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_relaunch_multi_gpu(args))
    # several ranks on one node share its cores (and the container's CPU quota): the library's host thread pool
    # would otherwise start min(cores, 16) threads in EVERY rank
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    if local_world > 1 and "FEMO_HOST_THREADS" not in os.environ:
        os.environ["FEMO_HOST_THREADS"] = str(max(1, min(16, usable_cores() // local_world)))
    from femo_amd.dist import _quiet_stdout
    with _quiet_stdout():                       # library banners go to stderr: stdout carries ONE JSON line
        result = _run(args)
    if result is not None:
        # every check record of the line carries `passed`; one verdict for the line, and a failing check is said aloud
        # (a plain run checks nothing -- the checks are part of --full -- and claims no verdict)
        failed, checked = [], []

        def walk(o, path):
            if isinstance(o, dict):
                if "passed" in o:
                    checked.append(path)
                    if o["passed"] is False:
                        failed.append(path)
                for k, v in o.items():
                    walk(v, f"{path}.{k}" if path else k)
        walk(result, "")
        if args.full or checked:
            result["checks_passed"] = not failed
        if failed:
            print(f"bench.py: CHECK FAILED in {failed}: the numbers of this line are not validated", file=sys.stderr, flush=True)
        print(json.dumps(result), flush=True)


def _timed_cycles(ctx, run_one, K, W):
    for w in range(W):
        run_one(w)
    ctx.sync()
    t0 = time.perf_counter()
    g = None
    for k in range(K):
        g = run_one(W + k)
    ctx.sync()
    return (time.perf_counter() - t0) / max(K, 1) * 1e3, g


def _run(args):
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dump_outputs and args.steps < 1:
        raise SystemExit("bench: --dump-outputs writes the last timed step's outputs and needs --steps >= 1")
    if world > 1 or os.environ.get("FEMO_BENCH_FORCE_DIST", "0") not in ("", "0"):   # the env switch runs the N>1 code path on one rank (tests)
        if args.dump_outputs:
            raise SystemExit("bench: --dump-outputs is implemented for the N = 1 path only (each rank holds a share of the arrays)")
        return bench_distributed(args, rank, world, local_rank)

    from femo_amd import engine as E
    from femo_amd.engine import Context, DeviceArray, Vec
    from femo_amd.fea import utils_hip
    from femo_amd.fea.mesh import createUnitCubeMesh

    ctx = Context(local_rank)
    utils_hip.set_context(ctx)
    utils_hip.KSP_OPTIONS["pc"] = PC
    t0 = time.perf_counter()
    mesh = createUnitCubeMesh(args.n, jitter=args.jitter)
    if args.permute:
        mesh = mesh.permuted(seed=20240807)
    if args.reorder:
        mesh = mesh.reordered(force=args.force_morton)
    sim, fea = build_problem(mesh, device=False)
    dm = mesh.device(ctx)
    n_dof, nnz = mesh.n_vert, dm.info["nnz"]
    K, W = args.steps, args.warmup
    f_host = source_fields(mesh, min(K + W, 4))
    # inputs "already on host" (SURVEY.md section 8(d)): NumPy arrays in pinned memory, as a driver that
    # allocates its variables through femo_host_alloc holds them
    f_pin = [E.pinned_array(f) for f in f_host]
    u0 = E.pinned_full(n_dof, 0.0)          # the cold-start state: a constant the library knows as such (device fill, no upload)
    setup_s = time.perf_counter() - t0

    # ---- headline: host arrays in, host arrays out ------------------------------------------------
    def host_cycle(k):
        return one_cycle(sim, fea, f_pin[k % len(f_pin)], u0)

    # The pinned pool is sized during set-up, like a backend that allocates its variable storage up front: with
    # asynchronous results two generations of result blocks are alive at a time, and a first-time hipHostMalloc of a
    # 477 MB block costs 60-90 ms -- with a single warm-up step (the default) that would land in the timed region.
    prime = [E.pinned_empty(int(np.size(sim['f']))) for _ in range(4)] + [E.pinned_empty(int(np.size(sim['u']))) for _ in range(8)]
    del prime
    g = None
    for w in range(W):
        g = host_cycle(w)          # held across the next cycle like in the timed loop
    ctx.sync()
    del utils_hip.LAST_KSP_INFO[:]
    E.host_stats(reset=True)
    E.host_syncs(reset=True)
    ms_per_step, g = _timed_cycles(ctx, lambda k: host_cycle(W + k), K, 0)   # never the source of the step before
    host_syncs = (E.host_syncs() - 1) / max(K, 1)                            # (- the ctx.sync() that ends the timed region)
    if not isinstance(g, np.ndarray) and K:
        raise SystemExit("bench: the host-boundary cycle must return a NumPy gradient")
    infos = list(utils_hip.LAST_KSP_INFO)
    xfer = E.host_stats()
    if args.dump_outputs:
        # what the caller of the last timed step holds: the gradient it returned, the state and the functional
        dump_outputs(args.dump_outputs, {"dJ_df": E.host_wait(g), "u": sim['u'], "J": sim['l2_functional']})

    per = len(infos) // K if K else 0                      # linear solves per step: Newton's three + the adjoint
    its_per_step = [i["iterations"] for i in infos[:per]]
    cg_ms = sum(i["solve_ms"] for i in infos) / max(K, 1)
    adj_ms = sum(i["solve_ms"] for k, i in enumerate(infos) if per and k % per == per - 1) / max(K, 1)
    fwd_ms = cg_ms - adj_ms
    solves = [i for i in infos if i["spmv_samples"] > 0]
    spmv_in_cg_ms = (sum(i["spmv_ms"] for i in solves) / sum(i["spmv_samples"] for i in solves)) if solves else float("nan")
    n_in_cg = sum(i["spmv_samples"] for i in solves)
    h2d_bytes = (xfer["h2d_pinned_bytes"] + xfer["h2d_staged_bytes"]) / max(K, 1)
    d2h_bytes = (xfer["d2h_pinned_bytes"] + xfer["d2h_staged_bytes"] + xfer["d2h_async_bytes"]
                 + xfer["d2h_device_sum_bytes"]) / max(K, 1)

    # ---- the headline record: everything in it comes from the timed steps ----------------------------
    result = {
        "metric": METRIC, "value": n_dof / (ms_per_step * 1e-3), "unit": "DOFs/s",
        "n_gpus": 1, "steps": K, "warmup": W, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {
            "workload": (f"3-D linear Poisson, P1 tets, unit cube n={args.n}: {n_dof} DOFs, {mesh.n_cell} cells, "
                         f"nnz {nnz}; per step, NumPy arrays at the operator boundary (f in; u, J, dJ/df out): "
                         f"Newton x3 (assemble R, dR/du, A; {PC.upper()}-CG) + J + dJ/du, dJ/df + "
                         f"dR/du, dR/df, A + transposed {PC.upper()}-CG + dR/df^T lambda; "
                         + ("CG stops on sqrt(r.M^-1 r) <= 1e-11 sqrt(b.M^-1 b) (energy-equivalent norm)" if PC == "bpx" else
                            "CG stops on sqrt(r.D^-1 r) <= 1e-14 sqrt(b.D^-1 b)") + "; cold start"),
            "boundary": "host (NumPy in pinned blocks of femo_host_alloc; H2D + D2H inside the timed region)",
            "preconditioner": PC, "pc_lattice": dm.pc_info(),
            "n": args.n, "jitter": args.jitter, "permuted": bool(args.permute), "reordered": bool(args.reorder),
            "n_dof": n_dof, "n_cell": mesh.n_cell, "nnz": nnz,
            "sell_slices": dm.info["n_slices"], "regular_slices": dm.info["regular_slices"], "short_slices": dm.info.get("short_slices", 0),
            "linear_solves_per_step": per, "cg_iterations_per_step": its_per_step, "cg_ms_per_step": cg_ms,
            "non_cg_ms_per_step": ms_per_step - cg_ms, "setup_s": setup_s,
            # blocking waits of the host on the device inside the library per cycle (femo_host_sync_stats): each is an idle
            # device for one host round trip (20-50 us) -- what the cycles of small meshes / of one rank of eight are made of
            "host_syncs_per_step": host_syncs,
            "pcie": {"h2d_bytes_per_step": h2d_bytes, "d2h_bytes_per_step": d2h_bytes,
                     "d2h_async_bytes_per_step": xfer["d2h_async_bytes"] / max(K, 1),
                     "d2h_device_sum_bytes_per_step": xfer["d2h_device_sum_bytes"] / max(K, 1),
                     "uploads_elided_per_step": (xfer["h2d_skipped"] + xfer["h2d_as_d2d"]) / max(K, 1),
                     "upload_bytes_elided_per_step": (xfer["h2d_skipped_bytes"] + xfer["h2d_as_d2d_bytes"]) / max(K, 1),
                     "host_threads": E._lib.load().femo_host_threads()},
        },
    }
    if not args.full:
        return result

    # ---- --full: the same cycle with inputs and outputs resident in HBM (no host boundary) ----------
    sim_d, fea_d = build_problem(mesh, device=True)
    f_dev = [DeviceArray(Vec(ctx, mesh.n_cell).set(f)) for f in f_pin]
    Kd = min(K, 5) if K else 0
    dev_ms, _ = _timed_cycles(ctx, lambda k: one_cycle(sim_d, fea_d, f_dev[k % len(f_dev)]), Kd, 1)
    del sim_d, fea_d, f_dev

    # ---- dominant kernel: the CG's SpMV (+ fused p.Ap), HIP events on the library's stream ---------
    from femo_amd.fea.utils_hip import _WORK
    A_mat = [w[1] for k, w in _WORK.items() if k[1] == "newton_A"][0].mat
    xv, yv = Vec(ctx, n_dof).set(np.random.default_rng(0).standard_normal(n_dof)), Vec(ctx, n_dof)
    spmv_loop_ms = min(A_mat.bench_spmv(xv, yv, 50) for _ in range(3))
    del xv, yv
    # `achieved` uses the launches inside the timed PCG loops (single launches between other kernels);
    # back-to-back launches run a few per cent faster (part of the matrix stays in the Infinity Cache)
    spmv_avg_ms = spmv_in_cg_ms if n_in_cg else spmv_loop_ms
    B_A = spmv_algorithmic_bytes(nnz, n_dof)
    achieved = B_A / (spmv_avg_ms * 1e-3) / 1e9
    traffic, pmc_file, pmc_commit = (None, None, None)
    if not (args.reorder and not args.permute):
        traffic, pmc_file, pmc_commit = _pmc_lookup(f"spmv_n{args.n}" + ("_permuted" if args.permute and not args.reorder else ""))
    stored = stored_bytes(dm.info, n_dof)
    physical = traffic if traffic else stored

    # PCIe rate of the box: one pinned 477 MB array each way
    probe = Vec(ctx, mesh.n_cell)
    t0 = time.perf_counter(); probe.set(f_host[0]); t_pg = time.perf_counter() - t0
    t0 = time.perf_counter(); probe.set(f_pin[-1]); t_up = time.perf_counter() - t0
    out = E.pinned_empty(mesh.n_cell)
    t0 = time.perf_counter(); probe.get(out=out); t_dn = time.perf_counter() - t0
    del probe, out
    nbytes = mesh.n_cell * 8

    # SURVEY.md section 8(d) split: Newton's linear solves / the transposed (adjoint) solve /
    # host<->device traffic and host-side passes / the rest (assembly, functional, dR/df^T lambda)
    result["config"]["split_ms_per_step"] = {"forward_solves": fwd_ms, "adjoint_solve": adj_ms,
                                             "h2d_d2h": ms_per_step - dev_ms,       # the part of the transfers NOT hidden behind kernels
                                             "assembly_outputs": dev_ms - cg_ms}
    result["config"]["pcie"].update({"h2d_pinned_GBs": nbytes / t_up / 1e9, "d2h_pinned_GBs": nbytes / t_dn / 1e9,
                                     "h2d_pageable_staged_GBs": nbytes / t_pg / 1e9})
    result["device_resident"] = {"value": n_dof / (dev_ms * 1e-3) if dev_ms else None, "unit": "DOFs/s", "ms_per_step": dev_ms,
                                 "steps": Kd, "note": "same cycle with DeviceArray inputs/outputs (no PCIe); round 1's headline"}
    result["roofline"] = {
        # round 6: `achieved` / `frac` are PHYSICAL -- the bytes the kernel really moves (PMC pass of
        # this kernel at this size, else the stored format's bytes) over the launch time measured in this run; the SURVEY
        # 8(d) CSR bytes over the same time are the CSR-equivalent rate `achieved_algorithmic` / `frac_algorithmic`
        "bound": "hbm", "achieved": physical / (spmv_avg_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": physical / (spmv_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
        "physical_bytes_per_launch": physical,
        "physical_bytes_source": f"PMC (2*FETCH_SIZE + WRITE_SIZE, profiles/{pmc_file}, collected at commit {pmc_commit})" if traffic else "stored bytes of the SELL format",
        "achieved_algorithmic": achieved, "frac_algorithmic": achieved / HBM_PEAK_GBS,
        "format_compression": B_A / physical,
        "frac_algorithmic_note": "CSR-equivalent rate: SURVEY.md 8(d) bytes (12 B per entry + 20 B per row) over the measured launch time; the regular-slice SELL format "
                                 "fetches no column indices and stores no unit diagonal, so the kernel moves format_compression x fewer bytes than the formula counts",
        "frac_physical": physical / (spmv_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "kernel": "k_spmv_sell<1,true> (SELL-64 SpMV + fused p.Ap, one launch per CG iteration)",
        "algorithmic_bytes_per_launch": B_A, "avg_launch_ms": spmv_avg_ms, "launches_timed": n_in_cg,
        "timed": "single launches inside the timed PCG loops (HIP events on the library's stream)",
        "avg_launch_ms_back_to_back": spmv_loop_ms, "back_to_back_launches_timed": 150,
        "stored_bytes_per_launch": stored,
        "whole_cycle": whole_cycle_roofline(mesh.tdim, n_dof, mesh.n_cell, nnz, its_per_step, ms_per_step, dev_ms),
    }
    # What of the transfers the operator protocol leaves exposed whatever the library does: the gradient is the last thing a
    # cycle produces and must be on the host when the cycle ends (nothing is left to compute under its way down); f must be
    # on the device before the load vector can be formed (only the f-independent half of the first pass runs under its way up).
    result["config"]["pcie"]["gradient_d2h_ms"] = t_dn * 1e3
    result["config"]["pcie"]["f_h2d_ms"] = t_up * 1e3
    result["config"]["pcie"]["pcie_floor_ms"] = t_dn * 1e3
    result["config"]["pcie"]["pcie_floor_note"] = ("the gradient's D2H at this box's pinned rate: the strict floor of split_ms_per_step.h2d_d2h under the operator "
                                                   "protocol; the rest of that entry is the part of f's upload (f_h2d_ms) that the f-independent kernels of the first pass do not cover")

    if not args.no_pcie:
        # a backend that keeps every array in its own pageable memory (copies results out, hands pageable inputs in)
        # ... with persistent storage, like a backend that preallocates its variable vectors: the engine pins such an
        # array in place the second time it sees it (engine._note_caller_array), so from the third cycle on every
        # transfer is one DMA; nothing is ever elided (the owner may write its arrays at any time).  The driver's
        # input array is its own too: f is copied into it at the start of every cycle.
        sim_p, fea_p = build_problem(mesh, device=False, pinned=False)
        f_own = np.empty(mesh.n_cell)
        u0_own = np.zeros(n_dof)
        for w in range(3):
            np.copyto(f_own, f_host[w % len(f_host)])
            one_cycle(sim_p, fea_p, f_own, u0_own)
        ctx.sync()
        E.host_stats(reset=True)
        Kp = 3
        t0 = time.perf_counter()
        for k in range(Kp):
            E.host_copy(f_own, f_host[(k + 1) % len(f_host)])
            one_cycle(sim_p, fea_p, f_own, u0_own)
        ctx.sync()
        t_h = (time.perf_counter() - t0) / Kp
        xp = E.host_stats()
        result["pageable_boundary"] = {"value": n_dof / t_h, "unit": "DOFs/s", "ms_per_step": t_h * 1e3, "steps": Kp,
                                       "h2d_pinned_per_step": xp["h2d_pinned"] / Kp, "h2d_staged_per_step": xp["h2d_staged"] / Kp,
                                       "h2d_elided_per_step": (xp["h2d_skipped"] + xp["h2d_as_d2d"]) / Kp,
                                       "note": "pageable NumPy arrays owned by the driver (preallocated variable storage) on both sides of "
                                               "every operator call; pinned in place by the engine on second sight, so transfers are DMAs; "
                                               "no upload is elided for caller-owned memory"}
        del sim_p, fea_p, f_own, u0_own
    if not args.no_pcie:
        # the same cycle from CSDL's default state value u = 1 instead of u = 0 ("the bench starts from
        # u = 0; from u = 1 the second Newton solve does real work"): a constant block like u0, a few cycles
        u1 = E.pinned_full(n_dof, 1.0)

        def ones_cycle(k):
            sim['f'] = f_pin[k % len(f_pin)]
            fea.states_dict['u']['function'].vector.set(1.0)
            sim['u'] = u1
            sim.run()
            return sim.compute_totals('l2_functional', 'f')

        ones_cycle(0)
        ctx.sync()
        del utils_hip.LAST_KSP_INFO[:]
        Ku = 3
        t0 = time.perf_counter()
        for k in range(Ku):
            ones_cycle(k + 1)
        ctx.sync()
        t_u1 = (time.perf_counter() - t0) / Ku
        its_u1 = [i["iterations"] for i in utils_hip.LAST_KSP_INFO[:len(utils_hip.LAST_KSP_INFO) // Ku]]
        result["csdl_default_start"] = {"value": n_dof / t_u1, "unit": "DOFs/s", "ms_per_step": t_u1 * 1e3, "steps": Ku,
                                        "cg_iterations_per_step": its_u1,
                                        "note": "cold start from u = 1 (python_csdl_backend's default state value) instead of u = 0"}
    if not args.no_check:
        # one more cycle of the timed stack, outside the timed region, compared with solver-free values
        kc = (W + K) % len(f_pin)
        g_chk = np.array(E.host_wait(host_cycle(kc)), copy=True)
        result["check"] = self_check(args, mesh, f_host[kc], np.array(sim['u'], copy=True),
                                     float(np.asarray(sim['l2_functional']).ravel()[0]), g_chk)
        del g_chk
    if not args.no_configs and not (args.permute or args.reorder or args.jitter) and args.n == 215:
        sim = fea = f_pin = u0 = g = dm = A_mat = None       # release the 10 M-DOF problem (host blocks, 20 GB of HBM) before the other meshes are built
        utils_hip.clear_workspaces()
        mesh._device = None
        import gc
        gc.collect()
        result["scaling_model"] = bench_scaling_model(ctx, args.n, 10, ms_per_step, result["config"]["split_ms_per_step"], global_its=its_per_step)
        result["configs"] = {"c2": bench_config2(ctx, 40), "c5_nl": bench_config5(ctx, 5), "c3_shell": bench_config3(ctx, 3)}
        try:
            result["unstructured"] = bench_unstructured(ctx, args.n, 3)
        except Exception as e:                                   # noqa: BLE001 - a leg of the report, never the headline
            result["unstructured"] = {"error": repr(e)}
        try:
            result["scaling_model_c5"] = bench_scaling_model_c5(ctx, 4, result["configs"]["c5_nl"])
        except Exception as e:                                   # noqa: BLE001 - a leg of the report, never the headline
            result["scaling_model_c5"] = {"error": repr(e)}
    if args.no_configs and args.scaling_model:
        sim = fea = f_pin = u0 = g = None
        utils_hip.clear_workspaces()
        result["scaling_model"] = bench_scaling_model(ctx, args.n, 10, ms_per_step, result["config"]["split_ms_per_step"], global_its=its_per_step)
    if not args.no_cpu_baseline:
        counts = its_per_step if its_per_step else [0]
        result["cpu_baseline"] = cpu_baseline(args, counts, n_dof, mesh.n_cell, nnz)
        # step 1 (is FEniCSx here?) and step 2a (the reference-faithful direct cycle where it fits)
        result["cpu_baseline"]["fenicsx_probe"] = fenicsx_probe()
        if args.n == 215 and not args.no_configs:
            try:
                result["cpu_baseline"]["direct"] = cpu_direct_legs()
            except Exception as e:                               # noqa: BLE001
                result["cpu_baseline"]["direct"] = {"error": repr(e)}
    return result


if __name__ == "__main__":
    main()
