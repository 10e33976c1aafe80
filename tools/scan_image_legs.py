"""bench.py's config-2 step with a chosen value of ctx option scan_image, in a fresh process: ms per step over 20 steps after 5 warm-up steps (as the plain
benchmark command), and — for scan_image = 1 — what the one-time build costs: the build kernel's device time and the wall time of the step that pays it.
   python tools/scan_image_legs.py <scan_image value> [rows]"""
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
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
import dfdb  # noqa: E402

st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = dfdb.Context(0, stream=st.cuda_stream)
ctx.set_option("scan_image", opt)
t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, rows)
q = t[("x", lambda x: x > 899_999), dfdb.ALL]._query()
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
step()                                                 # second execution: under scan_image = 1 this one builds the image
torch.cuda.synchronize(); second_ms = (time.perf_counter() - t0) * 1e3
torch.cuda.synchronize(); t0 = time.perf_counter()
step()
torch.cuda.synchronize(); third_ms = (time.perf_counter() - t0) * 1e3
build = ctx.profile_get("scan_image.build")
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
ctx.profile(False)
print(json.dumps({"scan_image": opt, "rows": rows, "ms_per_step": ms, "selected": nsel, "count": int(cnt.item()),
                  "first_execution_ms": first_ms, "second_step_wall_ms": second_ms, "third_step_wall_ms": third_ms,
                  "build_launches": build[0], "build_kernel_ms": build[1], "image_bytes": ctx.profile_get("scan_image_bytes")[0],
                  "kernels_avg_ms": {k: (v[1] / v[0] if v[0] else None) for k, v in prof.items()}, "resident": t.resident_bytes("x")}))
