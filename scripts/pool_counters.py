"""The pinned pool's bookkeeping per cycle of bench.py's headline workload (host arrays in, host arrays out): one JSON line
per step with the wall time and what femo_host_stats counted in it -- fresh hipHostMallocs and their time, frees of blocks in flight
(parked and handed to a later pool call: what a waiting femo_host_free would have waited for), unpinnings that waited for a DMA, D2H bytes and asynchronous
copy-outs.  A steady cycle shows zeros in the first three.
usage: pool_counters.py [N [STEPS [WARMUP]]]        (default 215 12 3; set-up as in bench.py, BPX-PCG)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from femo_amd import engine as E  # noqa: E402
from femo_amd.fea import utils_hip  # noqa: E402
from femo_amd.fea.mesh import createUnitCubeMesh  # noqa: E402

n, steps, warmup = (int(a) for a in (sys.argv[1:4] + ["215", "12", "3"][len(sys.argv) - 1:]))
ctx = E.Context(0)
utils_hip.set_context(ctx)
utils_hip.KSP_OPTIONS["pc"] = bench.PC
mesh = createUnitCubeMesh(n)
sim, fea = bench.build_problem(mesh, device=False)
f_pin = [E.pinned_array(f) for f in bench.source_fields(mesh, 4)]
u0 = E.pinned_full(mesh.n_vert, 0.0)
prime = [E.pinned_empty(int(np.size(sim['f']))) for _ in range(4)] + [E.pinned_empty(int(np.size(sim['u']))) for _ in range(8)]
del prime
KEYS = ("pool_fresh", "pool_fresh_us", "pool_free_deferred", "pool_free_waited", "pool_free_waited_us", "d2h_async")
g = None
for k in range(warmup + steps):
    if k == warmup:
        ctx.sync()
    E.host_stats(reset=True)
    t0 = time.perf_counter()
    g = bench.one_cycle(sim, fea, f_pin[k % len(f_pin)], u0)   # the gradient of the step before is held until here
    ms = (time.perf_counter() - t0) * 1e3
    st = E.host_stats()
    rec = {"step": k - warmup, "host_ms": round(ms, 3)}
    rec.update({key: st[key] for key in KEYS if key in st})
    rec["d2h_bytes"] = st["d2h_pinned_bytes"] + st["d2h_staged_bytes"] + st["d2h_async_bytes"] + st["d2h_device_sum_bytes"]
    print(json.dumps(rec), flush=True)
ctx.sync()
