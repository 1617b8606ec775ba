#!/usr/bin/env python3
"""What a radiance-query run costs next to the frame that does the same work: the configs[1] scene (1M-triangle grid, diffuse BSDF, sun +
sky), 1920x1080, 4 samples; the queries are the camera's pixel-centre rays. Median of synchronous calls of
RenderHip.render_radiance_queries (host arrays: upload, run, read-back) and of its device twin over the backend's buffers (the run alone),
against rptr_hip_render of the same camera on the same handle in the same process. Prints one JSON line.
--case textured: the textured test scene with the glTF program instead (the query shade kernels of that combination are compiled for three
waves per SIMD where the frame's run with four and a few spilled words: kernels.h rp_shade_query_waves).

    python tools/radiance_queries_timing.py [--case c2|textured] [--reps 15] [--width 1920 --height 1080 --spp 4]
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
from realtimepathtracingresearchframework_amd import abi, backend, scenes  # noqa: E402


def camera_rays(cam, W, H):
    """pixel-centre rays of the pinhole camera (host_frame.inl compute_view), float32"""
    pos, d, up = (np.asarray(list(v), np.float32) for v in (cam.pos, cam.dir, cam.up))
    plane_y = np.float32(2.0 * np.tan(0.5 * cam.fovy * np.pi / 180.0))
    du = np.cross(d, up)
    du = du / np.linalg.norm(du) * plane_y * np.float32(W / H)
    dv = np.cross(du, d)
    dv = -dv / np.linalg.norm(dv) * plane_y
    tl = d - 0.5 * du - 0.5 * dv
    x = (np.arange(W, dtype=np.float32) + 0.5) / W
    y = (np.arange(H, dtype=np.float32) + 0.5) / H
    dirs = x[None, :, None] * du + y[:, None, None] * dv + tl
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    q = np.zeros((W * H, 8), np.float32)
    q[:, 0:3], q[:, 4:7], q[:, 7] = pos, dirs.reshape(-1, 3), 2e32
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c2", "textured"], default="c2")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    W, H, spp = a.width, a.height, a.spp
    s = scenes.grid_1m() if a.case == "c2" else scenes.textured_test(nx=256, nz=256)
    variant = abi.VARIANT_SIMPLE if a.case == "c2" else abi.VARIANT_GLTF
    cam = s.camera_params()
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    r.set_stage_timing(0)
    q = camera_rays(cam, W, H)
    n = len(q)
    dq, dr = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    cfg = backend.RenderConfiguration(cam, active_variant=variant, reset_accumulation=True)
    one = np.zeros((1, 8), np.float32)
    one[0, 6], one[0, 7] = 1.0, 1.0

    def frame():
        r.render(cfg, spp=spp)

    def queries_device():
        r.render_radiance_queries_device(n, cam, variant=variant, spp=spp)
        r.render_ray_queries(one)  # (synchronous on the backend's stream: waits for the run)

    def sync_only():
        r.render_ray_queries(one)

    res = np.zeros((n, 4), np.float32)

    def queries_host():
        r.render_radiance_queries(q, cam, variant=variant, spp=spp, results=res)

    out = {}
    for name, fn in (("frame_ms", frame), ("queries_device_ms", queries_device), ("sync_only_ms", sync_only), ("queries_host_ms", queries_host)):
        for _ in range(3):
            fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(statistics.median(t), 4)
    out["queries_device_ms"] = round(out["queries_device_ms"] - out["sync_only_ms"], 4)
    out["ratio_device_run_to_frame"] = round(out["queries_device_ms"] / out["frame_ms"], 4)
    st = r.radiance_query_stats().raw
    out.update(case=a.case, width=W, height=H, spp=spp, queries=n, reps=a.reps, rays_closest=int(st.rays_closest), rays_shadow=int(st.rays_shadow), frame_rays_closest=int(r.stats().raw.rays_closest))
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
