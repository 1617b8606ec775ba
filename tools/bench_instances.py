#!/usr/bin/env python
"""Cost and quality of moving instances: ms per rptr_hip_refit under RPTR_TLAS_REBUILD and RPTR_TLAS_REFIT, ms of a fresh set_scene of
the moved scene (the only way to move an instance without rptr_hip_update_instances), and closest-hit node visits per ray of the three
trees after k frames of motion. scenes.forest at two sizes: BASELINE's C4 (10 meshes x 10 000 triangles, 1000 instances) and a small
one. Every instance has RPTR_MESH_INSTANCES_MOVE and moves each frame (a drift towards a permuted position: after k frames every tree
stands where another stood).

  python tools/bench_instances.py            # both sizes: one child process per size, chained, each under its own time limit
  python tools/bench_instances.py --size small|c4   # one size in this process; prints one JSON line
  python tools/bench_instances.py --emissive [--size small|c4]   # the moving-lights leg (run_emissive), one JSON line. The host prepares
                                                     # the lights in Python: seconds for the small forest, far longer for C4's 10^6 emitters

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


def emissive_forest(size, emission):
    """the forest of `size` with tree mesh 0 given materials of its own, emitting `emission` (0: the same scene, dark), every mesh movable"""
    import copy
    import numpy as np
    from realtimepathtracingresearchframework_amd import abi, scenes
    s = scenes.forest(name="forest-%s-emissive" % size, **SIZES[size])
    base = len(s.materials)
    for k in range(2):  # (a tree's triangles use materials offset + 0 / + 1)
        m = copy.deepcopy(s.materials[k])
        m.emission_intensity = emission
        s.materials.append(m)
    s.pmeshes[0].material_offsets = np.array([base], np.int32)
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    s.prepare_lights()
    return s


def run_emissive(size, frames, W, H):
    """--emissive: what re-placing the lights costs a refit. ms per rptr_hip_refit (RPTR_TLAS_REBUILD) of the forest with one tree mesh
    emissive and its light sources registered, of the same scene with the emission zeroed (no lights, nothing registered), and ms of a
    fresh set_scene of the moved emissive scene -- the only remedy without rptr_hip_set_light_sources."""
    import copy
    import numpy as np
    from realtimepathtracingresearchframework_amd import backend, lights
    ONE_RAY = np.array([[0, 1000, 0, 0, 0, -1, 0, 1e20]], np.float32)
    out = {"size": size, "leg": "emissive", "frames": frames}
    lit = None
    for name, emission in (("emissive", 4.0), ("dark", 0.0)):
        s = emissive_forest(size, emission)
        n = len(s.instances) - 1  # (the ground stays)
        x0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances[:n]])
        x1 = x0.copy()
        x1[:, :, 3] = x0[np.random.default_rng(1).permutation(n)][:, :, 3]
        path = [((1 - np.float32(k / frames)) * x0 + np.float32(k / frames) * x1).astype(np.float32) if k < frames else x1 for k in range(1, frames + 1)]
        r = backend.RenderHip()
        r.initialize(W, H)
        r.set_scene(s)
        if emission > 0:
            lit = s
            r.set_light_sources(s)
            out["lights"] = len(s.lights)
            out["instances"] = len(s.instances)
        else:
            assert len(s.lights) == 0
        r.render_ray_queries(ONE_RAY)
        ms = []
        for xf in path:
            r.update_instances(0, xf)
            t0 = time.perf_counter()
            r.refit()
            r.render_ray_queries(ONE_RAY)  # waits for the backend's stream
            ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        r.render_ray_queries(ONE_RAY)
        sync_ms = (time.perf_counter() - t0) * 1e3
        ms = sorted(ms[1:])                # (the first rebuild allocates its work space)
        out[name + "_refit_ms_median"] = ms[len(ms) // 2] - sync_ms
        out[name + "_refit_ms_min"] = ms[0] - sync_ms
        out[name + "_refit_ms_max"] = ms[-1] - sync_ms
        if emission > 0:  # the lights are where the rule puts them, and a fresh set_scene of that scene is what the refit replaces
            moved = copy.copy(s)
            moved.instances = [copy.copy(i) for i in s.instances]
            for k in range(n):
                moved.instances[k].transform = x1[k].reshape(3, 4).copy()
            xf_all = np.stack([np.asarray(i.transform, np.float32) for i in moved.instances])
            moved.lights = s.lights.copy()
            moved.lights[:, :3] = lights.place_light_sources(s.light_sources, xf_all)
            out["lights_match_the_rule"] = bool(np.array_equal(r.readback_lights().view(np.uint32), moved.lights.view(np.uint32)))
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                r.set_scene(moved)
                ms.append((time.perf_counter() - t0) * 1e3)
            out["set_scene_ms_min"] = min(ms)
        r.close()
    assert lit is not None
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES))
    ap.add_argument("--emissive", action="store_true", help="the moving-lights leg (one size, default small): refit with re-placed lights against the same scene dark")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    a = ap.parse_args()
    if a.emissive:
        run_emissive(a.size or "small", a.frames, a.width, a.height)
        return 0
    if a.size:
        run_size(a.size, a.frames, a.width, a.height)
        return 0
    steps = ["timeout -k 10 %d %s %s --size %s --frames %d --width %d --height %d" % (LIMIT_S[k], sys.executable, os.path.abspath(__file__), k, a.frames, a.width, a.height)
             for k in ("small", "c4")]
    return subprocess.call(" && ".join(steps), shell=True, cwd=ROOT)


if __name__ == "__main__":
    sys.exit(main())
