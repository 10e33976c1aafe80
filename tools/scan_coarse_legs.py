"""bench.py's config-2 step with a chosen value of ctx option scan_coarse, in a fresh process: ms per step over 20 steps after 5 warm-up steps (as the plain
benchmark command), the per-kernel HIP-event averages, which form of the image scan ran (the profile notes), and what the one-time build costs: both build
kernels' device time and the wall time of the step that pays them (allocations, the two waits and the histogram copy are the rest of that step).
   python tools/scan_coarse_legs.py <scan_coarse value> [rows] [mod1m | dense]
mod1m (default): the benchmark's column, h mod 1e6, `x > 899999`.  dense: the worst case — Int64 values in [-50, 50) with I32_MIN and I32_MAX present
(shift 16), `x > 7`: half the rows share the constant's bucket, so scan_coarse = 2 refines every one of them and scan_coarse = 1 must refuse."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

opt = int(sys.argv[1])
rows = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000_000
column = sys.argv[3] if len(sys.argv) > 3 else "mod1m"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
import dfdb  # noqa: E402

st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = dfdb.Context(0, stream=st.cuda_stream)
ctx.set_option("scan_coarse", opt)
if column == "dense":
    import numpy as np
    x = np.random.default_rng(1).integers(-50, 50, rows).astype(np.int64)
    x[0], x[-1] = -(1 << 31), (1 << 31) - 1
    t = dfdb.DFTable.from_columns({"x": x}, block_size=65536, ctx=ctx)
    thr = 7
    del x
else:
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, rows)
    thr = 899_999
q = t[("x", lambda x: x > thr), dfdb.ALL]._query()
cnt = torch.zeros(1, dtype=torch.int64, device=dev)
ctx.profile(True)
torch.cuda.synchronize(); t0 = time.perf_counter()
nsel = q.count()                                       # first execution: always the flat scan
torch.cuda.synchronize(); first_ms = (time.perf_counter() - t0) * 1e3
out = torch.empty(max(nsel, 1), dtype=torch.int64, device=dev)


def step():
    q.reset()
    q.indices_device(out.data_ptr(), nsel)
    q.count_device(cnt.data_ptr())


torch.cuda.synchronize(); t0 = time.perf_counter()
step()                                                 # second execution: builds the image and, unless scan_coarse = 0, the coarse copy
torch.cuda.synchronize(); second_ms = (time.perf_counter() - t0) * 1e3
torch.cuda.synchronize(); t0 = time.perf_counter()
step()
torch.cuda.synchronize(); third_ms = (time.perf_counter() - t0) * 1e3
build = ctx.profile_get("scan_image.build")
cbuild = ctx.profile_get("scan_image.coarse_build")
ctx.profile(False)
for _ in range(5):
    step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20):
    step()
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / 20 * 1e3
ctx.profile(True)
for _ in range(20):
    step()
torch.cuda.synchronize()
prof = {k: ctx.profile_get(k) for k in ("scan_cmp", "scan_image", "scan_counts", "compact_indices")}
notes = {k: ctx.profile_get("scan_image." + k)[0] for k in ("coarse", "coarse_exact", "coarse_dense", "int32", "uint32")}
ctx.profile(False)
print(json.dumps({"scan_coarse": opt, "column": column, "rows": rows, "ms_per_step": ms, "selected": nsel, "count": int(cnt.item()),
                  "first_execution_ms": first_ms, "second_step_wall_ms": second_ms, "third_step_wall_ms": third_ms,
                  "build_launches": build[0], "build_kernel_ms": build[1], "coarse_build_launches": cbuild[0], "coarse_build_kernel_ms": cbuild[1],
                  "image_bytes": ctx.profile_get("scan_image_bytes")[0], "notes_of_20_steps": notes,
                  "kernels_avg_ms": {k: (v[1] / v[0] if v[0] else None) for k, v in prof.items()}, "resident": t.resident_bytes("x")}))
