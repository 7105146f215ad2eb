"""Sum the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of tools/bench_clip_u8.py per preprocessing route:
device-only microseconds per call of ClipHIP.preprocess_u8 and of the route through the fp32 image.
usage: python tools/kernel_stats_by_route.py KERNEL_STATS_CSV"""
import csv
import sys

# the table and vertical kernels serve both routes: their mean time per call (over both routes' calls) counts once for each
SHARED = ("clip_ragged_coeffs_kernel", "clip_resize_v_norm_kernel")
NEW = ("clip_u8canvas_resize_h_kernel",) + SHARED
OLD = ("u8canvas_to_f32chw_pad_kernel", "clip_ragged_to_u8_kernel", "clip_ragged_resize_h_kernel") + SHARED
rows = list(csv.DictReader(open(sys.argv[1])))
calls = {}
for name, keys in (("preprocess_u8", NEW), ("via_fp32_image", OLD)):
    total = 0.0
    for r in rows:
        if any(k in r["Name"] for k in keys):
            n, ns = int(r["Calls"]), float(r["TotalDurationNs"])
            total += ns / n
            print(f"{name:16s} {ns / n / 1e3:9.2f} us/call x {n:5d}  {r['Name'][:90]}")
    calls[name] = total / 1e3
print({k: round(v, 2) for k, v in calls.items()}, "ratio old/new", round(calls["via_fp32_image"] / calls["preprocess_u8"], 2))
