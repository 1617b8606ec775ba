"""bin/rptr_hip --morph <file> --morph-weights <file> (host/rptr_cli.cpp) on a small written .vks whose mesh is dynamic: frame k of a run
stages the weights of the file's frame k mod frames, runs the deformers on the device and refits before it renders. The images of a
three-frame profiling run over a two-frame weights file, and the image sets of a data-capture run (one per frame of the file), equal the
Python mirror driven with the same weights, byte for byte -- alone and with --skin --bones beside them. (The refusals need no device:
tests/test_morph_cpu.py.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import morph_ref as MR
import skin_ref as S
from common import random_transforms
from host_tools import build_host_tool, read_exr, read_png
from realtimepathtracingresearchframework_amd import abi, backend, scenes, vks

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _files(tmp_path):
    """a written .vks of one grid whose material's extended name flags the mesh dynamic, a morph file of three targets (dense, a patch, an
    empty one), a weights file of two frames, and a skin and a bones file for the combined run"""
    path = str(tmp_path / "grid.vks")
    grid = scenes.grid(24, 12)
    grid.pmeshes[0] = scenes.ParameterizedMesh(mesh=0, material_offsets=np.array([0], np.int32))  # one material: the loader flags only such meshes
    names = vks.write_vks(path, grid)
    tex_dir = vks.texture_dir(path)
    os.makedirs(tex_dir, exist_ok=True)
    with open(tex_dir + names[0] + "_Ex.txt", "w") as f:
        f.write(names[0] + "_SHADERMESH_morph")
    s = vks.read_vks(path)
    assert int(s.meshes[0].dynamic) & abi.MESH_DYNAMIC and s.meshes[0].first_geometry == 0
    g = s.geometries[0]
    P = scenes.dequantize_positions(g.qpos, g.scaling, g.offset)
    n = len(P)
    size = float((P.max(axis=0) - P.min(axis=0)).max())
    rng = np.random.default_rng(12)
    patch = rng.permutation(n)[:n // 10].astype(np.uint32)
    targets = [(rng.permutation(n).astype(np.uint32), (rng.uniform(-0.02, 0.02, (n, 3)) * size).astype(np.float32), rng.uniform(-0.6, 0.6, (n, 3)).astype(np.float32)),
               (patch, (rng.uniform(-0.03, 0.03, (len(patch), 3)) * size).astype(np.float32), rng.uniform(-0.6, 0.6, (len(patch), 3)).astype(np.float32)),
               (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32), None)]
    weights = np.array([[0.8, -0.5, 0.3], [0.2, 1.4, 0.0]], np.float32)
    morph_file, weights_file = str(tmp_path / "morph.bin"), str(tmp_path / "weights.bin")
    with open(morph_file, "wb") as f:
        f.write(MR.morph_file(targets))
    with open(weights_file, "wb") as f:
        f.write(MR.weights_file(weights))
    bones, skin_weights = S.chain_rig(P, 4)
    bone_frames = np.tile(scenes.IDENTITY, (2, 4, 1, 1)).astype(np.float32)
    for k in range(2):
        bone_frames[k] += np.float32(0.08) * (random_transforms(4, 60 + k, spread=20.0) - scenes.IDENTITY)
    skin_file, bones_file = str(tmp_path / "skin.bin"), str(tmp_path / "bones.bin")
    np.ascontiguousarray(np.concatenate([bones, skin_weights], axis=1)).tofile(skin_file)
    with open(bones_file, "wb") as f:
        f.write(struct.pack("<II", 2, 4) + np.ascontiguousarray(bone_frames).tobytes())
    return dict(scene=s, path=path, targets=targets, weights=weights, bones=bones, skin_weights=skin_weights, bone_frames=bone_frames,
                morph_flags=["--morph", morph_file, "--morph-weights", weights_file], skin_flags=["--skin", skin_file, "--bones", bones_file])


def _mirror(f, skinned):
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(f["scene"])
    if skinned:
        r.set_skin(0, f["bones"], f["skin_weights"])
    r.set_morph_targets(0, f["targets"])
    return r


def _shaped_frame(r, f, k, skinned):
    if skinned:
        r.update_bones(0, f["bone_frames"][k % 2])
    r.update_morph_weights(0, 0, f["weights"][k % 2])
    r.skin()
    r.refit()
    r.render(backend.RenderConfiguration(f["scene"].camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)


@pytest.mark.parametrize("skinned", [False, True])
def test_morphed_profiling_run_writes_the_mirrors_images(tmp_path, skinned):
    exe = build_host_tool("rptr_cli")
    f = _files(tmp_path)
    n = 3
    prefix = str(tmp_path / "mo")
    run = subprocess.run([exe, f["path"], "--img", str(W), str(H), "--batch-spp", "1", "--synchronous", "--png", "--profiling-fps", "1", "--profiling-count", str(n),
                          "--profiling", prefix, "--profiling-img", prefix] + f["morph_flags"] + (f["skin_flags"] if skinned else []), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [line.split(",") for line in open(prefix + ".csv").read().strip().split("\n")[1:]]
    assert [int(v[2]) for v in rows] == [1] * n                                       # every frame starts a new accumulation
    r = _mirror(f, skinned)
    want = []
    for k in range(n):
        _shaped_frame(r, f, k, skinned)
        fb = np.zeros((H, W, 4), np.uint8)
        assert r.readback_framebuffer(fb) == W * H * 4
        want.append(fb)
    r.close()
    assert not np.array_equal(want[0], want[1])                                       # the shapes differ ...
    for k in range(n):
        got = read_png("%s_%04d.png" % (prefix, k + 1))
        assert got.shape == (H, W, 4)
        assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))


def test_morphed_data_capture_stores_one_image_set_per_weight_frame(tmp_path):
    exe = build_host_tool("rptr_cli")
    f = _files(tmp_path)
    prefix = str(tmp_path / "cap")
    run = subprocess.run([exe, f["path"], "--img", str(W), str(H), "--data-capture", prefix, "--data-capture-spp", "1"] + f["morph_flags"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    r = _mirror(f, False)
    normals = []
    for k in range(2):
        _shaped_frame(r, f, k, False)
        rgba = np.zeros((H, W, 4), np.float32)
        assert r.readback_framebuffer(rgba) == W * H * 4
        assert np.array_equal(read_exr("%s_%04d_rgba.exr" % (prefix, k + 1)).view(np.uint32), rgba.view(np.uint32)), k
        half = np.zeros((H, W, 4), np.float16)
        assert r.readback_aov(1, half) == W * H * 4
        got = read_exr("%s_%04d_normal_depth.exr" % (prefix, k + 1))
        assert got.dtype == np.uint16 and np.array_equal(got, half.view(np.uint16)), k
        normals.append(got)
    r.close()
    assert not os.path.exists("%s_0003_rgba.exr" % prefix)
    assert not np.array_equal(normals[0], normals[1])
