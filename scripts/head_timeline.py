"""Per-cycle timeline around the upload of f from a rocprofv3 --kernel-trace --memory-copy-trace CSV run.
usage: head_timeline.py DIR CYCLE"""
import csv, glob, os, sys
d, cyc = sys.argv[1], int(sys.argv[2])
ev = []
for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], 0))
for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        big = "HOST_TO_DEVICE" in r.get("Direction", "") and (e - s) > 200_000     # a piece of f: > 0.2 ms at PCIe rate
        ev.append((s, e, "COPY " + r.get("Direction", "") + " " + str(r.get("Bytes", r.get("Size", ""))), 1 if big else 0))
ev.sort()
h2d = [x for x in ev if x[2].startswith("COPY") and "HOST_TO_DEVICE" in x[2]]
groups = []                                              # uploads of f: a long piece starts one, every H2D copy that begins
for x in h2d:                                            # within 0.3 ms of its last end belongs to it (the short last piece too)
    if groups and x[0] - groups[-1][-1][1] < 300_000:
        groups[-1].append(x)
    elif x[3]:
        groups.append([x])
groups = [g for g in groups if sum(e - s for s, e, _, _ in g) > 5_000_000]    # 5 ms of copying or more in all
g = groups[cyc]
t0, t_last = g[0][0], g[-1][1]
print(f"upload of f: {len(g)} piece(s), {(t_last - t0) / 1e3:.1f} us from the first piece's start to the last piece's end; t = 0 at its start")
LOOP = ("k_spmv_sell<1, true", "k_pcg_xr", "k_restrict_bricks", "k_lattice_coarse", "k_lattice_prolong3", "k_prolong_mesh", "k_pcg_", "k_spmv_sell<4")
first_loop = None
kern = [x for x in ev if not x[2].startswith("COPY")]
prev_end = None
for s, e, n, b in ev:
    if s < t0 - 200_000 or s > t_last + 1_500_000:
        continue
    is_copy = n.startswith("COPY")
    if not is_copy and any(n.startswith(x) for x in LOOP):
        if first_loop is None:
            first_loop = s
            print(f"t={(s - t0) / 1e3:9.1f}  first loop kernel {n[:50]}: {(s - t_last) / 1e3:.1f} us after the last piece of f")
        continue
    gap = "" if is_copy or prev_end is None else f"gap {(s - prev_end) / 1e3:7.1f}"
    print(f"t={(s - t0) / 1e3:9.1f}  {gap:12s} {(e - s) / 1e3:8.1f} us  {'    ' if is_copy else ''}{n[:80]}")
    if not is_copy:
        prev_end = e if prev_end is None else max(prev_end, e)
if first_loop is None:
    print("no loop kernel within 1.5 ms of the upload")
