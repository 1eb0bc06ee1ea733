"""The two solves and the D2H copies of every cycle out of a rocprofv3 --kernel-trace --memory-copy-trace CSV run of
bench.py --gpus 1: per cycle the spans of the forward and the adjoint loop and every D2H copy above 0.2 ms, t = 0 at the start
of f's upload; then, over all cycles, the gap from the end of the forward loop to the start of the first D2H copy behind it
(u's copy-out) against its median -- a cycle in which the host is late shows there.
usage: cycle_d2h.py DIR [CYCLE]      (CYCLE: list that cycle's copies; without it only the table over all cycles)"""
import csv, glob, os, statistics, sys
d = sys.argv[1]
detail = int(sys.argv[2]) if len(sys.argv) > 2 else None
ker, cp = [], []
for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        ker.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]))
for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        cp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")))
ker.sort(); cp.sort()
LOOP = ("k_spmv_sell<1, true", "k_pcg_xr", "k_restrict_bricks", "k_lattice_coarse", "k_lattice_prolong3", "k_prolong_mesh", "k_pcg_")
loop = [x for x in ker if any(x[2].startswith(p) for p in LOOP)]
# f's upload: H2D copies above 0.2 ms; pieces less than 5 ms apart are one upload
starts = []
for s, e, n in cp:
    if "HOST_TO_DEVICE" in n and e - s > 200_000:
        if not starts or s - starts[-1][1] > 5_000_000:
            starts.append([s, e])
        else:
            starts[-1][1] = e
gaps = []
for c in range(len(starts) - 1):
    t0, t1 = starts[c][0], starts[c + 1][0]
    runs = []                                            # loop kernels less than 1 ms apart are one solve's loop
    for s, e, n in loop:
        if t0 <= s < t1:
            if runs and s - runs[-1][1] < 1_000_000:
                runs[-1][1] = e
            else:
                runs.append([s, e])
    runs = [r for r in runs if r[1] - r[0] > 1_000_000]
    if len(runs) < 2:
        continue
    fwd, adj = runs[0], runs[-1]
    d2h = [x for x in cp if "DEVICE_TO_HOST" in x[2] and t0 <= x[0] < t1 and x[1] - x[0] > 200_000]
    after = [x for x in d2h if x[0] >= fwd[1]]
    gap = (after[0][0] - fwd[1]) / 1e3 if after else float("nan")
    mid = [x for x in d2h if fwd[1] <= x[0] < adj[1]]
    gaps.append((c, gap, (adj[0] - fwd[1]) / 1e3, (t1 - t0) / 1e3, len(mid), sum(x[1] - x[0] for x in mid) / 1e3))
    if detail == c:
        print(f"cycle {c}: {(t1 - t0) / 1e3:.0f} us to the next upload; forward loop {(fwd[0] - t0) / 1e3:.0f}..{(fwd[1] - t0) / 1e3:.0f}, "
              f"adjoint loop {(adj[0] - t0) / 1e3:.0f}..{(adj[1] - t0) / 1e3:.0f}")
        prev = None
        for s, e, n in d2h:
            tail = f"   {(s - prev) / 1e3:7.0f} us after the copy before" if prev is not None else ""
            print(f"  D2H {(s - t0) / 1e3:9.0f} .. {(e - t0) / 1e3:9.0f}  ({(e - s) / 1e3:7.0f} us){tail}")
            prev = e
if gaps:
    med = statistics.median(g[1] for g in gaps)
    print(f"{len(gaps)} cycles; forward loop's end to u's copy-out: median {med:.0f} us")
    print("cycle   to_copy_out_us   between_loops_us   cycle_us   D2H copies between the solves (count, us)")
    for c, gap, between, cyc, nmid, usmid in gaps:
        flag = "   <-- above 2 x median" if gap > 2 * med else ""
        print(f"{c:5d}   {gap:14.0f}   {between:16.0f}   {cyc:8.0f}   {nmid:3d} {usmid:8.0f}{flag}")
