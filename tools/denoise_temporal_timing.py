#!/usr/bin/env python3
"""Times rptr_hip_denoise_temporal beside rptr_hip_denoise on a configs[1] frame: the 1000 x 500 height field, 1920 x 1080, 4 spp, the
diffuse variant, reprojection_mode 1, a yaw of 0.002 rad per frame (the fly-through's step).

Three frames are rendered with a temporal call each, so the last frame has a motion AOV and a history. On that frame, in this order:
  1. --warmup + --repeats temporal calls with reset_history = 1 (rp_k_denoise_temporal without history),
  2. --warmup + --repeats temporal calls with history (each reads what the previous call left; the taps lie where the frame's motion
     AOV points),
  3. --warmup + --repeats rptr_hip_denoise calls (rp_k_denoise_prepare),
each between two HIP events on the backend's stream (a torch stream the handle shares). Prints one JSON line with the median and the
least milliseconds of a whole call (5 iterations unless --iterations says otherwise).

Kernel times come from a kernel trace of this program, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/denoise_temporal_timing.py
    python tools/denoise_temporal_timing.py --summarize <dir>/.../*_kernel_trace.csv
--summarize reads the trace's dispatches in start order and prints the median and least microseconds of rp_k_denoise_temporal without
history (the first --warmup + --repeats dispatches after the three of the set-up, warm-up dropped), with history (the next ones) and of
rp_k_denoise_prepare (its last --repeats dispatches), with the bytes per pixel each figure amounts to at 4 TB/s for comparison.
"""
import argparse
import csv
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SETUP_FRAMES = 3


def yawed(abi, cam, k, rate=0.002):
    d = [float(v) for v in cam.dir[:]]
    u = [float(v) for v in cam.up[:]]
    r = [d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]]
    rl = math.sqrt(sum(x * x for x in r))
    a = rate * k
    nd = [math.cos(a) * d[i] + math.sin(a) * r[i] / rl for i in range(3)]
    nl = math.sqrt(sum(x * x for x in nd))
    c = abi.Camera()
    c.pos[:] = cam.pos[:]
    c.dir[:] = [x / nl for x in nd]
    c.up[:] = cam.up[:]
    c.fovy = cam.fovy
    return c


def summarize(path, warmup, repeats, width, height):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("KernelName") or ""
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name))
    rows.sort()
    temporal = [d for _, d, n in rows if "rp_k_denoise_temporal" in n]
    prepare = [d for _, d, n in rows if "rp_k_denoise_prepare" in n]
    per = warmup + repeats
    if len(temporal) != SETUP_FRAMES + 2 * per or len(prepare) != per:
        raise SystemExit("the trace holds %d rp_k_denoise_temporal and %d rp_k_denoise_prepare dispatches, expected %d and %d: was it made "
                         "with the same --warmup / --repeats?" % (len(temporal), len(prepare), SETUP_FRAMES + 2 * per, per))
    groups = {"rp_k_denoise_temporal_without_history": temporal[SETUP_FRAMES + warmup:SETUP_FRAMES + per],
              "rp_k_denoise_temporal_with_history": temporal[SETUP_FRAMES + per + warmup:],
              "rp_k_denoise_prepare": prepare[warmup:]}
    npix = width * height
    out = {"tool": "denoise_temporal_timing --summarize", "width": width, "height": height, "dispatches_each": repeats}
    for name, ns in groups.items():
        med = statistics.median(ns)
        out[name] = {"median_us": round(med / 1e3, 2), "min_us": round(min(ns) / 1e3, 2),
                     "bytes_per_pixel_at_4TBps": round(med * 1e-9 * 4e12 / npix, 1)}
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=str, default="1000x500")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--summarize", type=str, default=None, metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.warmup, args.repeats, args.width, args.height)
    import torch
    from realtimepathtracingresearchframework_amd import abi, backend, scenes
    nx, nz = (int(v) for v in args.grid.split("x"))
    scene = scenes.grid(nx, nz)
    cam = scene.camera_params()
    stream = torch.cuda.Stream()
    result = {"tool": "denoise_temporal_timing", "width": args.width, "height": args.height, "spp": args.spp, "grid": args.grid,
              "iterations": args.iterations, "repeats": args.repeats, "warmup": args.warmup}
    with torch.cuda.stream(stream):
        r = backend.RenderHip(stream=stream.cuda_stream)
        r.initialize(args.width, args.height)
        r.set_scene(scene)
        r.params.reprojection_mode = 1
        for k in range(SETUP_FRAMES):
            r.render(backend.RenderConfiguration(yawed(abi, cam, k), active_variant=abi.VARIANT_SIMPLE, reset_accumulation=k == 0), spp=args.spp)
            r.denoise_temporal(iterations=args.iterations)
        calls = (("temporal_without_history", lambda: r.denoise_temporal(iterations=args.iterations, reset_history=1)),
                 ("temporal_with_history", lambda: r.denoise_temporal(iterations=args.iterations)),
                 ("spatial", lambda: r.denoise(iterations=args.iterations)))
        for name, call in calls:
            times = []
            for k in range(args.warmup + args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                if k >= args.warmup:
                    times.append(a.elapsed_time(b))
            result[name] = {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4)}
            if name == "temporal_with_history":
                n = r.readback_denoise_history()[..., 3]
                result["history"] = {"surface_pixels": int((n > 0).sum()), "with_history": int((n > 1).sum()), "pixels": int(n.size)}
        r.close()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
