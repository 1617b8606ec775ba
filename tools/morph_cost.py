#!/usr/bin/env python3
"""What morph targets on the device cost next to uploading finished vertices, on configs[5]'s mesh: scenes.grid(1000, 500) as a dynamic mesh
(1 M triangles, 3 M unrolled vertices) with 8 dense targets and 48 sparse ones of about 2 % of the vertices each (contiguous runs of
unrolled vertices: a patch of the surface), with and without the 64-bone chain of tools/skin_cost.py bound as well.

Two roads to the same shape, alternating in one run, each timed with events on the backend's stream (which the calls are ordered on):
  (a) update_vertices of the numpy-morphed array (36 MB from pageable host memory; the numpy arithmetic itself is NOT in the time), refit
  (b) update_morph_weights (56 floats; with the rig also update_bones, 64 x 48 bytes) + skin + refit
and rp_k_morph alone -- skin() between two events, once per pair and as a run of back-to-back calls -- as bytes per second over the bytes
it moves: per vertex 8 of offsets (two dwords, one of them shared with the neighbour: counted as 4) + 12 rest position + 4 rest normal
word in and 12 + 4 out (with the rig 16 of skin record more), per entry 32 (two float4) + 4 of weight (a cache hit: not counted),
against the float4-copy figure of the microarchitecture guide (6.29 TB/s). Weight sets keep every target non-zero, so every entry is
fetched AND applied. Before timing, the device's result is compared with tests/morph_ref.py bit for bit at this size. Prints one JSON line.

    python tools/morph_cost.py [--nx 1000 --nz 500] [--dense 8 --sparse 48] [--bones 64] [--reps 12]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import morph_ref as MR  # noqa: E402
import skin_ref as S  # noqa: E402
from skin_cost import chain_pose  # noqa: E402
from realtimepathtracingresearchframework_amd import backend, scenes  # noqa: E402

COPY_TBS = 6.29  # MI355X float4 copy, measured (microarchitecture guide)


def make_targets(n, dense, sparse, share, size, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    k = max(1, int(n * share))
    for t in range(dense + sparse):
        v = np.arange(n, dtype=np.uint32) if t < dense else (np.arange(k, dtype=np.uint32) + np.uint32(rng.integers(0, n - k + 1)))
        out.append((v, (rng.uniform(-0.002, 0.002, (len(v), 3)) * size).astype(np.float32), rng.uniform(-0.2, 0.2, (len(v), 3)).astype(np.float32)))
    return out


def weight_set(n_targets, k):
    """every target non-zero, one negative and one above 1"""
    w = (0.1 + 0.05 * np.sin(0.7 * np.arange(n_targets) + k)).astype(np.float32)
    w[k % n_targets] = -0.3
    w[(k + 3) % n_targets] = 1.2
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--nz", type=int, default=500)
    ap.add_argument("--dense", type=int, default=8)
    ap.add_argument("--sparse", type=int, default=48)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--burst", type=int, default=50)
    a = ap.parse_args()
    s = scenes.grid(a.nx, a.nz, deform_t=0.0)
    g = s.geometries[0]
    rest = scenes.dequantize_positions(g.qpos, g.scaling, g.offset)
    words = (np.asarray(g.qnrm_uv, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    n = len(rest)
    targets = make_targets(n, a.dense, a.sparse, a.share, float((rest.max(axis=0) - rest.min(axis=0)).max()))
    n_entries = sum(len(t[0]) for t in targets)
    weights = [weight_set(len(targets), k) for k in range(4)]
    transposed = MR.transpose(targets, n)
    bones, skin_weights = S.chain_rig(rest, a.bones)
    poses = [chain_pose(a.bones, 0.1 * k) for k in range(4)]

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = dict(triangles=n // 3, vertices=n, targets=len(targets), entries=n_entries, entries_per_vertex=round(n_entries / n, 3), reps=a.reps)
    for rigged in (False, True):
        tag = "morph_skin" if rigged else "morph"
        shaped = [MR.morph(rest, words, targets, weights[k], skin=(bones, skin_weights, poses[k]) if rigged else None, transposed=transposed) for k in range(4)]
        rv = backend.RenderHip(stream=stream.cuda_stream)
        rv.initialize(1920, 1080)
        rv.set_scene(s)
        rm = backend.RenderHip(stream=stream.cuda_stream)
        rm.initialize(1920, 1080)
        rm.set_scene(s)
        if rigged:
            rm.set_skin(0, bones, skin_weights)
        rm.set_morph_targets(0, targets)

        def stage(k):
            rm.update_morph_weights(0, 0, weights[k % 4])
            if rigged:
                rm.update_bones(0, poses[k % 4])

        stage(1)
        rm.skin()
        xyz, got_words = rm.readback_skinned(0)
        exact = bool(np.array_equal(xyz.view(np.uint32), shaped[1][0].view(np.uint32)) and np.array_equal(got_words, shaped[1][1]))
        assert exact, "rp_k_morph differs from tests/morph_ref.py"
        rm.refit()

        def road_vertices(k):
            rv.update_vertices(0, shaped[k % 4][0])
            rv.refit()

        def road_weights(k):
            stage(k)
            rm.skin()
            rm.refit()

        ms = {"vertices": [], "weights": [], "kernel_only": []}
        for k in range(a.reps + 2):
            tv = timed(lambda: road_vertices(k))
            tw = timed(lambda: road_weights(k))
            stage(k + 1)
            tk = timed(rm.skin)
            rm.refit()
            if k >= 2:  # (two warm-up rounds: code objects, first refits)
                ms["vertices"].append(tv)
                ms["weights"].append(tw)
                ms["kernel_only"].append(tk)

        def burst():
            for _ in range(a.burst):
                rm.skin()
        burst_ms = sorted(timed(burst) / a.burst for _ in range(5))
        rm.refit()
        bytes_moved = n * (4 + 12 + 4 + 12 + 4 + (16 if rigged else 0)) + n_entries * 32
        res = dict(exact_against_reference=exact, bytes_moved=bytes_moved)
        for name, v in ms.items():
            res[name + "_ms_median"] = round(statistics.median(v), 4)
            res[name + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        res["kernel_burst_ms_median"] = round(burst_ms[2], 4)
        res["kernel_burst_ms_range"] = [round(burst_ms[0], 4), round(burst_ms[-1], 4)]
        for key in ("kernel_only_ms_median", "kernel_burst_ms_median"):
            tbs = bytes_moved / (res[key] * 1e-3) / 1e12
            res[key.replace("_ms_median", "_tb_per_s")] = round(tbs, 3)
            res[key.replace("_ms_median", "_share_of_float4_copy")] = round(tbs / COPY_TBS, 3)
        res["speedup_weights_over_vertices"] = round(res["vertices_ms_median"] / res["weights_ms_median"], 2)
        out[tag] = res
        rv.close()
        rm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
