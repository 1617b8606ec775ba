#!/usr/bin/env python3
"""What rptr_hip_object_motion costs, and what its tracking adds to an update + refit.

pass: at 1920x1080, after a frame whose objects moved -- configs[1] (the 1M-triangle grid, its one instance moving) or the C4 forest (every
tree moving) -- the median of `reps` calls, each ended by reading "object_motion_pixels" (which waits for the backend's stream), next to
rptr_hip_trace_surface_device on the pixel-centre rays of the same camera in the backend's query buffer, ended the same way; the two and
the ending call alone alternate in one loop, the ending call is subtracted. The pass recomputes from the hit, so it is repeated on one frame.
refit: ms per update_instances + rptr_hip_refit (all trees of a forest drifting, as tools/bench_instances.py moves them) on two handles of
one process, tracking on and off, alternating frame by frame. A handle with tracking off takes the code path of a library without the
feature plus one untaken branch per update. Prints one JSON line.

    python tools/object_motion_cost.py --case c2|forest [--reps 15]
    python tools/object_motion_cost.py --case refit --size c4|small [--frames 20]
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
from radiance_queries_timing import camera_rays  # noqa: E402
from bench_instances import SIZES  # noqa: E402


def movable(s):
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    return s


def pass_cost(a):
    W, H = a.width, a.height
    if a.case == "c2":
        s = movable(scenes.grid_1m())
        n_move = 1
    else:
        s = movable(scenes.forest(name="forest-c4", **SIZES["c4"]))
        n_move = len(s.instances) - 1  # (the ground stays)
    x0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances[:n_move]])
    x1 = x0.copy()
    x1[:, :, 3] += np.array([0.3, 0.0, 0.2], np.float32)
    cam = s.camera_params()
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    if a.case == "c2":
        r.set_tlas_policy(abi.TLAS_REFIT)  # (one record: there is no top level to rebuild)
    r.track_object_motion()
    cfg = backend.RenderConfiguration(cam, active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True)
    r.render(cfg, spp=1)
    r.update_instances(0, x1)
    r.refit()
    r.render(cfg, spp=1)
    q = camera_rays(cam, W, H)
    n = len(q)
    dq, _ = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    dout = C.c_void_p()
    assert hip.hipMalloc(C.byref(dout), n * abi.SURFACE_HIT_DTYPE.itemsize) == 0
    pixels = []

    def sync_only():
        r.get_option("object_motion_pixels")

    def motion():
        pixels.append(r.object_motion())

    def surface():
        r.render_surface_queries_device(n, cam, variant=abi.VARIANT_SIMPLE, device_results=dout.value)
        sync_only()

    runs = (("pass_ms", motion), ("surface_ms", surface), ("sync_only_ms", sync_only))
    for _ in range(3):
        for _, fn in runs:
            fn()
    t = {name: [] for name, _ in runs}
    for _ in range(a.reps):
        for name, fn in runs:
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    out = {name: round(statistics.median(v), 4) for name, v in t.items()}
    out["pass_device_ms"] = round(out["pass_ms"] - out["sync_only_ms"], 4)
    out["surface_device_ms"] = round(out["surface_ms"] - out["sync_only_ms"], 4)
    out["pass_range_ms"] = [round(min(t["pass_ms"]), 4), round(max(t["pass_ms"]), 4)]
    out["surface_range_ms"] = [round(min(t["surface_ms"]), 4), round(max(t["surface_ms"]), 4)]
    assert len(set(pixels)) == 1
    out.update(case=a.case, width=W, height=H, reps=a.reps, instances_moved=n_move, pixels_rewritten=int(pixels[0]))
    hip.hipFree(dout)
    r.close()
    print(json.dumps(out))


def refit_cost(a):
    s = movable(scenes.forest(name="forest-" + a.size, **SIZES[a.size]))
    n = len(s.instances) - 1
    x0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances[:n]])
    x1 = x0.copy()
    x1[:, :, 3] = x0[np.random.default_rng(1).permutation(n)][:, :, 3]
    frames = a.frames
    path = [((1 - np.float32(k / frames)) * x0 + np.float32(k / frames) * x1).astype(np.float32) for k in range(1, frames + 1)]
    cam = s.camera_params()
    cfg = backend.RenderConfiguration(cam, active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True)
    handles = {}
    for name in ("off", "on"):
        r = backend.RenderHip()
        r.initialize(640, 360)
        r.set_scene(s)
        if name == "on":
            r.track_object_motion()
        r.render(cfg, spp=1)
        handles[name] = r
    ms = {"off": [], "on": []}
    for xf in path:
        for name, r in handles.items():
            t0 = time.perf_counter()
            r.update_instances(0, xf)
            r.refit()
            r.get_option("instance_updates_rejected")  # waits for the backend's stream
            ms[name].append((time.perf_counter() - t0) * 1e3)
            r.render(cfg, spp=1)  # (a submission: the next update is the first of its interval and takes the snapshot)
    out = dict(case="refit", size=a.size, instances=len(s.instances), frames=frames)
    for name in ms:
        v = sorted(ms[name][1:])  # (the first rebuild allocates its work space)
        out["update_refit_ms_median_tracking_" + name] = round(v[len(v) // 2], 4)
        out["update_refit_ms_range_tracking_" + name] = [round(v[0], 4), round(v[-1], 4)]
    for r in handles.values():
        r.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c2", "forest", "refit"], default="c2")
    ap.add_argument("--size", choices=sorted(SIZES), default="c4")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    refit_cost(a) if a.case == "refit" else pass_cost(a)


if __name__ == "__main__":
    main()
