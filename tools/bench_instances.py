#!/usr/bin/env python
"""Cost and quality of moving instances: ms per rptr_hip_refit under RPTR_TLAS_REBUILD and RPTR_TLAS_REFIT, ms of a fresh set_scene of
the moved scene (the only way to move an instance without rptr_hip_update_instances), and closest-hit node visits per ray of the three
trees after k frames of motion. scenes.forest at two sizes: BASELINE's C4 (10 meshes x 10 000 triangles, 1000 instances) and a small
one. Every instance has RPTR_MESH_INSTANCES_MOVE and moves each frame (a drift towards a permuted position: after k frames every tree
stands where another stood).

  python tools/bench_instances.py            # both sizes: one child process per size, chained, each under its own time limit
  python tools/bench_instances.py --size small|c4   # one size in this process; prints one JSON line

One GPU process at a time: the parent never opens the GPU, it starts `timeout -k 10 <s> python tools/bench_instances.py --size ...`
per size, chained with && (a size that fails ends the run)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"small": dict(n_meshes=4, tris_per_tree=300, n_instances=200), "c4": dict(n_meshes=10, tris_per_tree=10000, n_instances=1000)}
LIMIT_S = {"small": 240, "c4": 900}


def run_size(size, frames, W, H):
    import copy
    import numpy as np
    from realtimepathtracingresearchframework_amd import abi, backend, scenes
    s = scenes.forest(name="forest-" + size, **SIZES[size])
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    n = len(s.instances) - 1  # (the ground stays)
    x0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances[:n]])
    x1 = x0.copy()
    x1[:, :, 3] = x0[np.random.default_rng(1).permutation(n)][:, :, 3]
    path = [((1 - np.float32(k / frames)) * x0 + np.float32(k / frames) * x1).astype(np.float32) if k < frames else x1 for k in range(1, frames + 1)]
    moved = copy.copy(s)
    moved.instances = [copy.copy(i) for i in s.instances]
    for k in range(n):
        moved.instances[k].transform = x1[k].reshape(3, 4).copy()
    ONE_RAY = np.array([[0, 1000, 0, 0, 0, -1, 0, 1e20]], np.float32)  # origin, pad, direction, t_max
    out = {"size": size, "instances": len(s.instances), "instanced_triangles": int(s.num_instanced_tris()), "frames": frames}

    def visits(r):
        cfg = backend.RenderConfiguration(moved.camera_params(), active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True)
        st = r.render(cfg, spp=1, count_traversal=True)
        return st.raw.nodes_closest / max(1, st.raw.rays_closest)

    for name, policy in (("rebuild", abi.TLAS_REBUILD), ("refit", abi.TLAS_REFIT)):
        r = backend.RenderHip()
        r.initialize(W, H)
        r.set_scene(s)
        r.set_tlas_policy(policy)
        r.render_ray_queries(ONE_RAY)  # (query buffers exist: the synchronisation below is a one-ray query)
        ms = []
        for xf in path:
            r.update_instances(0, xf)          # (synchronous upload: not part of the refit's time)
            t0 = time.perf_counter()
            r.refit()
            r.render_ray_queries(ONE_RAY)  # waits for the backend's stream
            ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        r.render_ray_queries(ONE_RAY)
        sync_ms = (time.perf_counter() - t0) * 1e3
        ms = sorted(ms[1:])                    # (the first rebuild allocates its work space)
        out[name + "_refit_ms_median"] = ms[len(ms) // 2] - sync_ms
        out[name + "_refit_ms_min"] = ms[0] - sync_ms
        out["sync_query_ms"] = sync_ms
        out[name + "_records"] = int((r.export_bvh()[2].view(np.int32).reshape(-1, 32)[:, 12] >= 0).sum())
        out[name + "_visits_per_ray"] = visits(r)
        out[name + "_tlas_rebuilds"] = r.tlas_rebuild_count()
        r.close()
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        r.set_scene(moved)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["set_scene_ms_min"] = min(ms)
    out["fresh_visits_per_ray"] = visits(r)
    r.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    a = ap.parse_args()
    if a.size:
        run_size(a.size, a.frames, a.width, a.height)
        return 0
    steps = ["timeout -k 10 %d %s %s --size %s --frames %d --width %d --height %d" % (LIMIT_S[k], sys.executable, os.path.abspath(__file__), k, a.frames, a.width, a.height)
             for k in ("small", "c4")]
    return subprocess.call(" && ".join(steps), shell=True, cwd=ROOT)


if __name__ == "__main__":
    sys.exit(main())
