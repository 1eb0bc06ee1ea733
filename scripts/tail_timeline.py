"""Per-cycle timeline of the tail of a cycle -- from the last loop kernel of the adjoint solve to the end of the last D2H
copy -- out of a rocprofv3 --kernel-trace --memory-copy-trace CSV run of bench.py --gpus 1.
usage: tail_timeline.py DIR CYCLE"""
import csv, glob, os, sys
d, cyc = sys.argv[1], int(sys.argv[2])
ev = []
for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]))
for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "COPY " + r.get("Direction", "").replace("MEMORY_COPY_", "") + " stream " + str(r.get("Stream_Id", "?"))))
ev.sort()
LOOP = ("k_spmv_sell<1, true", "k_pcg_xr", "k_restrict_bricks", "k_lattice_coarse", "k_lattice_prolong3", "k_prolong_mesh", "k_pcg_", "k_spmv_sell<4")
# the tail's product: k_dRdf_cell_apply_T (one launch) or its ranged variant (one per range); launches less than 20 ms apart are one cycle's
prod = [x for x in ev if x[2].startswith("k_dRdf_cell_apply_T")]
groups = []
for x in prod:
    if groups and x[0] - groups[-1][-1][1] < 20_000_000:
        groups[-1].append(x)
    else:
        groups.append([x])
g = groups[cyc]
t_prod = g[0][0]
loops = [x for x in ev if x[1] <= t_prod and any(x[2].startswith(p) for p in LOOP)]
t0 = loops[-1][1]                                        # end of the adjoint solve's last loop kernel
nxt = [x[0] for x in ev if x[0] > t_prod and x[2].startswith("COPY") and "HOST_TO_DEVICE" in x[2] and x[1] - x[0] > 200_000]
t_next = nxt[0] if nxt else ev[-1][1] + 1                # the next cycle's upload of f
d2h = [x for x in ev if x[2].startswith("COPY") and "DEVICE_TO_HOST" in x[2] and t0 - 1_000_000 < x[0] < t_next and x[1] > t0]
t_end = max(x[1] for x in d2h)
print(f"tail of cycle {cyc}: t = 0 at the end of the adjoint solve's last loop kernel ({loops[-1][2][:40]}); {len(g)} product launch(es)")
for s, e, n in ev:
    if e < t0 or s > t_end:
        continue
    if any(n.startswith(p) for p in LOOP) and s < t0:
        continue
    is_copy = n.startswith("COPY")
    print(f"t={(s - t0) / 1e3:9.1f} .. {(e - t0) / 1e3:9.1f}  {(e - s) / 1e3:8.1f} us  {'    ' if is_copy else ''}{n[:80]}")
big = [x for x in d2h if x[0] >= t_prod]                  # the gradient's copies: D2H copies that start after the first product launch
psi = [x for x in d2h if x[0] < t_prod]
if big:
    print(f"first gradient byte leaves {(big[0][0] - t0) / 1e3:.1f} us after the solve; {len(big)} gradient copy(ies), the last ends at {(big[-1][1] - t0) / 1e3:.1f} us")
for s, e, n in psi:
    ov = min(e, t_end) - max(s, big[0][0]) if big else 0
    print(f"copy in flight before the product: {n}  {(s - t0) / 1e3:.1f} .. {(e - t0) / 1e3:.1f} us; overlaps the gradient's copies for {max(ov, 0) / 1e3:.1f} us")
print(f"tail total: {(t_end - t0) / 1e3:.1f} us")
