#!/usr/bin/env python3
"""Times rptr_hip_auto_exposure on a configs[1] frame: the 1000 x 500 height field, 1920 x 1080, 4 spp, the diffuse variant -- and on a
worst-case uniform frame, the same scene with the camera pitched up into the sky.

Per view: the median microseconds of one call for mode 0, mode 1 on the frame (source 0) and mode 1 on the denoised image (source 1),
each between two events on the backend's stream (a torch stream the handle shares), over --repeats calls after --warmup. Then rp_k_meter
alone on each view's float image and on a synthetic image of one value, plain (what the library launches) and with the wave-combine
step (tests/device_probes/exposure_probe.hip instantiates both; --no-probe skips this). Prints one JSON line. Every view runs
rptr_hip_denoise once, so under `rocprofv3 --kernel-trace --stats -- python tools/auto_exposure_timing.py` the kernel trace holds
rp_k_denoise_finish, a pass of rp_k_expose's shape, next to the three kernels;
profiles/auto_exposure_notes.md records such a run.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SKY = (0.0, 0.8, -0.6)  # pitched up 53 degrees: no ground in view


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=str, default="1000x500")
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-probe", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from realtimepathtracingresearchframework_amd import abi, backend, scenes
    nx, nz = (int(v) for v in args.grid.split("x"))
    scene = scenes.grid(nx, nz)
    result = {"tool": "auto_exposure_timing", "width": args.width, "height": args.height, "spp": args.spp, "grid": args.grid, "repeats": args.repeats, "views": {}}
    stream = torch.cuda.Stream()
    frames = {}
    with torch.cuda.stream(stream):
        r = backend.RenderHip(stream=stream.cuda_stream)
        r.initialize(args.width, args.height)
        r.set_scene(scene)
        for view in ("configs1", "sky"):
            cam = scene.camera_params()
            if view == "sky":
                cam.dir[:] = SKY
            r.render(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True), spp=args.spp)
            r.denoise(iterations=1)
            out = {}
            for name, fields in (("mode0", dict(mode=0)), ("mode1_source0", dict(mode=1, dt=1 / 60)), ("mode1_source1", dict(mode=1, source=1, dt=1 / 60))):
                pairs = []
                for k in range(args.warmup + args.repeats):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    r.auto_exposure(tone_mapping_mode=1, **fields)
                    b.record(stream)
                    if k >= args.warmup:
                        pairs.append((a, b))
                stream.synchronize()
                us = [a.elapsed_time(b) * 1e3 for a, b in pairs]
                out[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2)}
            st = r.readback_exposure_state()
            out["ev"] = round(float(st.ev), 4)
            out["bins_used"] = int(np.count_nonzero(np.array(st.histogram[:])))
            out["counted"] = int(st.counted)
            result["views"][view] = out
            img = np.zeros((args.height, args.width, 4), np.float32)
            r.readback_framebuffer(img)
            frames[view] = img
        blocks = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        r.close()
    if not args.no_probe:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from device_probes import exposure as probe
        result["meter_blocks"] = blocks
        flat = np.empty((args.height, args.width, 4), np.float32)  # one value everywhere: all 64 lanes of every wave hold the same bin
        flat[...] = (0.25, 0.5, 0.125, 1.0)
        frames["flat"] = flat
        result["views"]["flat"] = {}
        for view, img in frames.items():
            result["views"][view]["meter_combine_us"] = round(probe.time_meter(img, blocks, True, args.warmup, args.repeats), 2)
            result["views"][view]["meter_plain_us"] = round(probe.time_meter(img, blocks, False, args.warmup, args.repeats), 2)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
