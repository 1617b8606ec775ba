#!/usr/bin/env python3
"""What an occlusion-query run costs next to the closest-hit query of the same rays: the configs[1] scene (1M-triangle grid), the 1920x1080
pixel-centre camera rays as queries. Median of device runs of rptr_hip_trace_occlusion_device, each ended by a synchronous call on the
backend's stream, and of rptr_hip_trace_device on the same queries and the same handle, the two alternating in one loop; the cost of the
ending call alone is measured the same way and subtracted. Then the same pair for shadow probes: rays towards the sun from the camera
rays' first hits (the origins a host asks about; pixels that see the sky keep their camera ray), and -- the literal twin of the first
measurement -- from the camera rays' own origin. Prints one JSON line.
The library under test is RPTR_HIP_LIB's (a build with -DRP_OCCLUSION_COMMIT=1 measures the other way of committing the bits).

    python tools/occlusion_queries_timing.py [--reps 15] [--width 1920 --height 1080] [--alpha-cutoff 0.5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from realtimepathtracingresearchframework_amd import abi, backend, scenes  # noqa: E402
from radiance_queries_timing import camera_rays  # noqa: E402  (the pixel-centre rays of the pinhole camera)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--alpha-cutoff", type=float, default=None, help="ask for the cutout rule (the scene has no alpha-tested material: the opaque kernel runs)")
    a = ap.parse_args()
    W, H = a.width, a.height
    s = scenes.grid_1m()
    cam = s.camera_params()
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    q = camera_rays(cam, W, H)
    n = len(q)
    dq, dr = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    nw = (n + 31) // 32
    dbits = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbits), nw * 4) == 0 and hip.hipMemset(dbits, 0, nw * 4) == 0
    one = np.zeros((1, 8), np.float32)
    one[0, 6], one[0, 7] = 1.0, 1.0

    def sync_only():
        r.render_ray_queries(one)  # (synchronous on the backend's stream: waits for what was queued there)

    def occlusion():
        r.render_occlusion_queries_device(n, alpha_cutoff=a.alpha_cutoff, device_bits=dbits.value)
        sync_only()

    def closest():
        r.trace_device(dq, n, dr)
        sync_only()

    def measure(queries):
        assert hip.hipMemcpy(dq, queries.ctypes.data_as(C.c_void_p), queries.nbytes, 1) == 0
        runs = (("occlusion_ms", occlusion), ("closest_ms", closest), ("sync_only_ms", sync_only))
        for _ in range(3):
            for _, fn in runs:
                fn()
        t = {name: [] for name, _ in runs}
        for _ in range(a.reps):  # alternating: both see the same clocks and the same neighbours
            for name, fn in runs:
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        out = {name: round(statistics.median(v), 4) for name, v in t.items()}
        out["occlusion_device_ms"] = round(out["occlusion_ms"] - out["sync_only_ms"], 4)
        out["closest_device_ms"] = round(out["closest_ms"] - out["sync_only_ms"], 4)
        out["occlusion_range_ms"] = [round(min(t["occlusion_ms"]), 4), round(max(t["occlusion_ms"]), 4)]
        out["closest_range_ms"] = [round(min(t["closest_ms"]), 4), round(max(t["closest_ms"]), 4)]
        words = np.zeros(nw, np.uint32)
        assert hip.hipMemcpy(words.ctypes.data_as(C.c_void_p), dbits, words.nbytes, 2) == 0
        res = np.zeros((n, 4), np.float32)
        assert hip.hipMemcpy(res.ctypes.data_as(C.c_void_p), dr, res.nbytes, 2) == 0
        out["occluded"] = int(backend.RenderHip.unpack_occlusion_bits(words, n).sum())
        out["closest_hits"] = int((res.view(np.int32)[:, 3] >= 0).sum())
        return out

    out = {"camera": measure(q)}
    # shadow probes: towards the sun from where the camera rays land (a little off the surface, along the probe)
    sun = np.asarray(s.config.sun_dir, np.float64)
    sun = (sun / np.linalg.norm(sun)).astype(np.float32)
    hits = r.render_surface_queries(q, cam, variant=abi.VARIANT_SIMPLE)
    landed = hits["t"] > 0
    probes = q.copy()
    probes[landed, 0:3] = hits["position"][landed] + np.float32(1e-3) * sun
    probes[landed, 4:7] = sun
    out["sun_from_hits"] = measure(probes)
    out["sun_from_hits"]["probes"] = int(landed.sum())
    eye = q.copy()
    eye[:, 4:7] = sun
    out["sun_from_eye"] = measure(eye)
    out.update(width=W, height=H, queries=n, reps=a.reps, alpha_cutoff=a.alpha_cutoff, bytes_per_query_in=32, bytes_per_query_out_occlusion=0.125,
               bytes_per_query_out_closest=16, library=os.environ.get("RPTR_HIP_LIB", "the package's"))
    hip.hipFree(dbits)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
