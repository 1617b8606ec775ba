#!/usr/bin/env python3
"""What a surface-query run costs next to the closest-hit query of the same rays: the configs[1] scene (1M-triangle grid, diffuse BSDF),
the 1920x1080 pixel-centre camera rays as queries, in the backend's query buffer. Median of device runs of rptr_hip_trace_surface_device,
each ended by a synchronous call on the backend's stream, and of rptr_hip_trace_device on the same queries and the same handle, the two
alternating in one loop; the cost of the ending call alone is measured the same way and subtracted. Prints one JSON line.
--case textured: the textured test scene with the glTF program (the decode kernel's instantiation with texture code).

    python tools/surface_queries_timing.py [--case c2|textured] [--reps 15] [--width 1920 --height 1080]
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
    ap.add_argument("--case", choices=["c2", "textured"], default="c2")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    W, H = a.width, a.height
    s = scenes.grid_1m() if a.case == "c2" else scenes.textured_test(nx=256, nz=256)
    variant = abi.VARIANT_SIMPLE if a.case == "c2" else abi.VARIANT_GLTF
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
    hip.hipFree.argtypes = [C.c_void_p]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    dout = C.c_void_p()
    assert hip.hipMalloc(C.byref(dout), n * abi.SURFACE_HIT_DTYPE.itemsize) == 0
    one = np.zeros((1, 8), np.float32)
    one[0, 6], one[0, 7] = 1.0, 1.0

    def sync_only():
        r.render_ray_queries(one)  # (synchronous on the backend's stream: waits for what was queued there)

    def surface():
        r.render_surface_queries_device(n, cam, variant=variant, device_results=dout.value)
        sync_only()

    def closest():
        r.trace_device(dq, n, dr)
        sync_only()

    runs = (("surface_ms", surface), ("closest_ms", closest), ("sync_only_ms", sync_only))
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
    out["surface_device_ms"] = round(out["surface_ms"] - out["sync_only_ms"], 4)
    out["closest_device_ms"] = round(out["closest_ms"] - out["sync_only_ms"], 4)
    out["surface_range_ms"] = [round(min(t["surface_ms"]), 4), round(max(t["surface_ms"]), 4)]
    out["closest_range_ms"] = [round(min(t["closest_ms"]), 4), round(max(t["closest_ms"]), 4)]
    res = np.zeros(n, abi.SURFACE_HIT_DTYPE)
    assert hip.hipMemcpy(res.ctypes.data_as(C.c_void_p), dout, res.nbytes, 2) == 0
    out.update(case=a.case, width=W, height=H, queries=n, reps=a.reps, hits=int((res["t"] > 0).sum()), bytes_per_query_in=32, bytes_per_query_out=96)
    hip.hipFree(dout)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
