"""bin/rptr_hip --skin <file> --bones <file> (host/rptr_cli.cpp): frame k of a run stages the bones of the file's frame k mod frames, skins
mesh 0 on the device and refits before it renders. The images of a three-frame profiling run over a two-frame bones file, and the image
sets of a data-capture run (one per frame of the file), equal the Python mirror driven with the same matrices, byte for byte. (The
refusals need no device: tests/test_skin_cpu.py.)"""
import struct
import subprocess

import numpy as np
import pytest

import skin_ref as S
from common import random_transforms
from host_tools import build_host_tool, read_exr, read_png
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _files(tmp_path):
    """a dumped dynamic grid, its skin file (a 4-bone chain) and a bones file of two gentle poses: the chain's bones a little away from
    identity, so that the mesh stays in front of the scene's camera"""
    s = scenes.grid(24, 12, deform_t=0.0)
    path = str(tmp_path / "grid.rpsc")
    s.dump(path)
    g = s.geometries[0]
    bones, weights = S.chain_rig(scenes.dequantize_positions(g.qpos, g.scaling, g.offset), 4)
    frames = np.tile(scenes.IDENTITY, (2, 4, 1, 1)).astype(np.float32)
    for f in range(2):
        frames[f] += np.float32(0.08) * (random_transforms(4, 50 + f, spread=20.0) - scenes.IDENTITY)
    skin_file, bones_file = str(tmp_path / "skin.bin"), str(tmp_path / "bones.bin")
    np.ascontiguousarray(np.concatenate([bones, weights], axis=1)).tofile(skin_file)
    with open(bones_file, "wb") as f:
        f.write(struct.pack("<II", 2, 4) + np.ascontiguousarray(frames).tobytes())
    return s, path, bones, weights, frames, ["--skin", skin_file, "--bones", bones_file]


def _mirror(s, bones, weights):
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    r.set_skin(0, bones, weights)
    return r


def _posed_frame(r, s, M):
    r.update_bones(0, M)
    r.skin()
    r.refit()
    r.render(backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)


def test_skinned_profiling_run_writes_the_mirrors_images(tmp_path):
    exe = build_host_tool("rptr_cli")
    s, path, bones, weights, frames, flags = _files(tmp_path)
    n = 3
    prefix = str(tmp_path / "sk")
    run = subprocess.run([exe, path, "--img", str(W), str(H), "--batch-spp", "1", "--synchronous", "--png", "--profiling-fps", "1", "--profiling-count", str(n),
                          "--profiling", prefix, "--profiling-img", prefix] + flags, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [line.split(",") for line in open(prefix + ".csv").read().strip().split("\n")[1:]]
    assert [int(v[2]) for v in rows] == [1] * n                                       # every frame starts a new accumulation
    r = _mirror(s, bones, weights)
    want = []
    for k in range(n):
        _posed_frame(r, s, frames[k % 2])
        fb = np.zeros((H, W, 4), np.uint8)
        assert r.readback_framebuffer(fb) == W * H * 4
        want.append(fb)
    r.close()
    assert not np.array_equal(want[0], want[1])                                       # the poses differ ...
    for k in range(n):
        got = read_png("%s_%04d.png" % (prefix, k + 1))
        assert got.shape == (H, W, 4)
        assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))


def test_skinned_data_capture_stores_one_image_set_per_pose(tmp_path):
    exe = build_host_tool("rptr_cli")
    s, path, bones, weights, frames, flags = _files(tmp_path)
    prefix = str(tmp_path / "cap")
    run = subprocess.run([exe, path, "--img", str(W), str(H), "--data-capture", prefix, "--data-capture-spp", "1"] + flags, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    r = _mirror(s, bones, weights)
    normals = []
    for k in range(2):
        _posed_frame(r, s, frames[k])
        rgba = np.zeros((H, W, 4), np.float32)
        assert r.readback_framebuffer(rgba) == W * H * 4
        assert np.array_equal(read_exr("%s_%04d_rgba.exr" % (prefix, k + 1)).view(np.uint32), rgba.view(np.uint32)), k
        half = np.zeros((H, W, 4), np.float16)
        assert r.readback_aov(1, half) == W * H * 4
        got = read_exr("%s_%04d_normal_depth.exr" % (prefix, k + 1))
        assert got.dtype == np.uint16 and np.array_equal(got, half.view(np.uint16)), k
        normals.append(got)
    r.close()
    assert not np.array_equal(normals[0], normals[1])
