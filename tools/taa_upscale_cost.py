#!/usr/bin/env python3
"""Cost of rptr_hip_taa_upscale on configs[1] (the 1000 x 500 height field, 4 spp, the diffuse variant, a slow pan in reprojection_mode 2):

  * rendered at 960 x 540 and upscaled to 1920 x 1080, and rendered at 1920 x 1080 and upscaled to 3840 x 2160: milliseconds per call
    between two HIP events on the backend's stream (a torch stream the handle shares), with history (rp_k_taa_upscale) and without
    (reset_history = 1: rp_k_upscale_replicate), the median and the least of --repeats calls after --warmup;
  * for comparison one in-frame rp_k_taa pass at 1920 x 1080, the display pixel count of the first case: the median resolve_time_ms of
    the same frames with option "taa" = 1 less that with "taa" = 0 (stage timing 2: events on the resolve launches themselves).

Prints one JSON line. The calls of one case repeat on the same finished frame: each reads the previous call's output as its history.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def panned(abi, cam, k, rate=0.003):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=str, default="1000x500")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12, help="frames of the rp_k_taa comparison")
    args = ap.parse_args()
    import torch
    from realtimepathtracingresearchframework_amd import abi, backend, scenes
    nx, nz = (int(v) for v in args.grid.split("x"))
    scene = scenes.grid(nx, nz)
    cam = scene.camera_params()
    cfg = lambda k: backend.RenderConfiguration(panned(abi, cam, k), active_variant=abi.VARIANT_SIMPLE, reset_accumulation=k == 0)
    result = {"tool": "taa_upscale_cost", "grid": args.grid, "spp": args.spp, "repeats": args.repeats, "warmup": args.warmup, "upscale": {}}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for W, H in ((960, 540), (1920, 1080)):
            r = backend.RenderHip(stream=stream.cuda_stream)
            r.initialize(W, H)
            r.set_scene(scene)
            r.params.reprojection_mode = 2
            for k in range(3):   # a history and a moving view
                r.render(cfg(k), spp=args.spp)
                r.taa_upscale()
            case = {}
            for name, reset in (("with_history", 0), ("replicate", 1)):
                times = []
                for k in range(args.warmup + args.repeats):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    r.taa_upscale(reset_history=reset)
                    b.record(stream)
                    b.synchronize()
                    if k >= args.warmup:
                        times.append(a.elapsed_time(b))
                case[name + "_median_ms"] = round(statistics.median(times), 4)
                case[name + "_min_ms"] = round(min(times), 4)
            img = r.readback_upscaled()
            case["display"] = [int(img.shape[1]), int(img.shape[0])]
            result["upscale"]["%dx%d" % (W, H)] = case
            r.close()
        # one rp_k_taa pass at 1920 x 1080: the resolve stage with and without it
        resolve = {}
        for taa in (0, 1):
            r = backend.RenderHip(stream=stream.cuda_stream, options={"taa": taa})
            r.initialize(1920, 1080)
            r.set_scene(scene)
            r.params.reprojection_mode = 2
            r.set_stage_timing(2)
            times = []
            for k in range(args.frames):
                r.render(cfg(k), spp=args.spp)
                if k >= 2:   # (frame 0 resets and runs no pass)
                    times.append(float(r.stats().raw.resolve_time_ms))
            resolve[taa] = statistics.median(times)
            r.close()
        result["rp_k_taa_1920x1080_ms"] = round(resolve[1] - resolve[0], 4)
        result["resolve_ms_taa_off_on"] = [round(resolve[0], 4), round(resolve[1], 4)]
    up = result["upscale"]["960x540"]["with_history_median_ms"]
    result["ratio_to_rp_k_taa_at_1920x1080"] = round(up / result["rp_k_taa_1920x1080_ms"], 3) if result["rp_k_taa_1920x1080_ms"] > 0 else None
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
