#!/usr/bin/env python3
"""Times rptr_hip_denoise on a configs[1] frame: the 1000 x 500 height field, 1920 x 1080, 4 spp, the diffuse variant.

For 1..5 iterations: the median wall-clock milliseconds of one denoise call between two synchronisations of the backend's stream
(a torch stream the handle shares), over --repeats calls. Prints one JSON line. Under `rocprofv3 --kernel-trace --stats -- python
tools/denoise_timing.py` the kernel trace gives the per-pass times (rp_k_denoise_pass<1>, <2>, <0> = spacings 4, 8, 16 in launch
order); profiles/denoise_notes.md records such a run.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=str, default="1000x500")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from realtimepathtracingresearchframework_amd import abi, backend, scenes
    nx, nz = (int(v) for v in args.grid.split("x"))
    scene = scenes.grid(nx, nz)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = backend.RenderHip(stream=stream.cuda_stream)
        r.initialize(args.width, args.height)
        r.set_scene(scene)
        r.render(backend.RenderConfiguration(scene.camera_params(), active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True), spp=args.spp)
        result = {"tool": "denoise_timing", "width": args.width, "height": args.height, "spp": args.spp, "grid": args.grid, "repeats": args.repeats,
                  "median_ms": {}, "min_ms": {}}
        for it in range(1, 6):
            times = []
            for k in range(args.warmup + args.repeats):
                stream.synchronize()
                t0 = time.perf_counter()
                r.denoise(iterations=it)
                stream.synchronize()
                if k >= args.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            result["median_ms"][str(it)] = round(statistics.median(times), 4)
            result["min_ms"][str(it)] = round(min(times), 4)
        img = r.readback_denoised_f32()
        result["finite"] = bool(abs(float(img[..., :3].mean())) < float("inf"))
        r.close()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
