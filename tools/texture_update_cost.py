#!/usr/bin/env python3
"""What a dynamic texture costs (GPU): new level-0 texels from a device buffer and the mip chain made on the device
(rptr_hip_update_texture_device with RPTR_TEXTURE_GENERATE_MIPS, csrc/texture_mips.h), on a 2048 x 2048 sRGB texture and a 4096 x 4096
linear one that replace textures of scenes.textured_test(). (tools/texture_cost.py is about something else: what textured materials
cost a frame.)

Timed with events on the backend's stream, which the calls are ordered on, alternating in one run:
  (a) update_texture(device tensor, generate_mips=True)      the copy and one launch per level
  (b) update_texture(device tensor, generate_mips=False)     the copy alone
  (c) update_texture(None)                                   the chain alone
and, as wall time, the only way there was before: a fresh set_scene of the same scene with a host-made chain (scenes.generate_mips is
not counted; the scene's BVHs are tiny here -- README.md "Moving instances" has what they cost on a real scene).
Bytes moved by the chain: every level is read once and every level but the first written once, 4 bytes a texel; the copy reads and
writes level 0. Against the float4-copy figure of the microarchitecture guide (6.29 TB/s). The device's chain is compared with
scenes.generate_mips byte for byte first. Prints one JSON line per texture.

    python tools/texture_update_cost.py [--reps 12]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from realtimepathtracingresearchframework_amd import backend, scenes  # noqa: E402

COPY_TBS = 6.29  # MI355X float4 copy, measured (microarchitecture guide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    table = backend.srgb_decode_table()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for index, size, srgb in ((0, 2048, True), (1, 4096, False)):
        rng = np.random.default_rng(size)
        texels = [rng.integers(0, 256, (size, size, 4)).astype(np.uint8) for _ in range(2)]
        scene = copy.copy(scenes.textured_test())
        scene.textures = list(scene.textures)
        scene.textures[index] = scenes.Texture(rgba=texels[0], srgb=srgb)
        r = backend.RenderHip(stream=stream.cuda_stream)
        r.initialize(256, 256)
        r.set_scene(scene)
        dev = [torch.from_numpy(t).cuda() for t in texels]
        torch.cuda.synchronize()
        r.update_texture(index, dev[1])
        want = scenes.generate_mips(texels[1], srgb, table)
        exact = all(np.array_equal(r.readback_texture(index, l + 1), lv) for l, lv in enumerate(want))
        assert exact and r.texture_levels(index) == len(want) + 1, "the device's chain differs from scenes.generate_mips"
        ms = {"copy_and_chain": [], "copy_only": [], "chain_only": []}
        for k in range(a.reps + 2):
            t0 = timed(lambda: r.update_texture(index, dev[k & 1]))
            t1 = timed(lambda: r.update_texture(index, dev[k & 1], generate_mips=False))
            t2 = timed(lambda: r.update_texture(index, None))
            if k >= 2:  # (two warm-up rounds: code objects, the one allocation)
                ms["copy_and_chain"].append(t0)
                ms["copy_only"].append(t1)
                ms["chain_only"].append(t2)
        r.close()
        fresh = copy.copy(scene)
        fresh.textures = list(scene.textures)
        fresh.textures[index] = scenes.Texture(rgba=texels[1], srgb=srgb, mips=want)
        fresh.desc()  # (the packing of the levels into one buffer is the host's preparation, not the call)
        r = backend.RenderHip(stream=stream.cuda_stream)
        r.initialize(256, 256)
        r.set_scene(fresh)
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r.set_scene(fresh)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t) * 1e3)
        r.close()
        level_texels = [size * size] + [lv.shape[0] * lv.shape[1] for lv in want]
        chain_bytes = 4 * (sum(level_texels[:-1]) + sum(level_texels[1:]))
        copy_bytes = 8 * size * size
        out = dict(texture="%d x %d %s" % (size, size, "sRGB" if srgb else "linear"), levels=len(level_texels), reps=a.reps, exact_against_generate_mips=exact,
                   chain_bytes=chain_bytes, copy_bytes=copy_bytes)
        for name, v in ms.items():
            out[name + "_ms_median"] = round(statistics.median(v), 4)
            out[name + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        for name, nbytes in (("chain_only", chain_bytes), ("copy_only", copy_bytes), ("copy_and_chain", chain_bytes + copy_bytes)):
            tbs = nbytes / (out[name + "_ms_median"] * 1e-3) / 1e12
            out[name + "_tb_per_s"] = round(tbs, 3)
            out[name + "_share_of_float4_copy"] = round(tbs / COPY_TBS, 3)
        out["fresh_set_scene_wall_ms_median"] = round(statistics.median(walls), 3)
        out["fresh_set_scene_wall_ms_range"] = [round(min(walls), 3), round(max(walls), 3)]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
