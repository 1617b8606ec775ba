"""Skinned meshes without a device: the restated arithmetic (tests/skin_ref.py) against plain linear algebra, the test rig, and the refusals
of bin/rptr_hip --skin / --bones (exit code 2 before a device is touched).

Normal words are compared to within ONE step per component: the restatement evaluates cof(A) n in float32, the yardstick
inverse-transpose(A) n in float64; both go through quantize.h's truncation to 1 / 32768 steps, so a float32 error of ~1e-7 can move a
component across one truncation boundary and never across two."""
import struct
import subprocess

import numpy as np

import skin_ref as S
from common import random_transforms
from host_tools import build_host_tool
from realtimepathtracingresearchframework_amd import abi, scenes

f32 = np.float32


def _points(n=200, seed=1):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-3, 3, (n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pos, scenes.quantize_normals(nrm.astype(f32))


def _single_bone(n, bone):
    bones = np.zeros((n, 4), np.uint16)
    weights = np.zeros((n, 4), np.uint16)
    bones[:, 0] = bone
    weights[:, 0] = 65535
    return bones, weights


def _word_steps(a, b):
    """largest difference of the two 16-bit components of oct-encoded normal words"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    dx = np.abs((a & 0xFFFF).astype(np.int64) - (b & 0xFFFF).astype(np.int64))
    dy = np.abs((a >> 16).astype(np.int64) - (b >> 16).astype(np.int64))
    return int(max(dx.max(), dy.max()))


def _inverse_transpose_words(M, words):
    n = S.dequantize_normals(words).astype(np.float64)
    q = n @ np.linalg.inv(M[:, :3].astype(np.float64))           # rows: (A^-T n)^T = n^T A^-1
    return scenes.quantize_normals(q.astype(f32)), q


def test_one_bone_with_full_weight_is_the_plain_transform():
    pos, words = _points()
    M = random_transforms(3, 11)                                  # rotation x non-uniform scale + translation
    bones, weights = _single_bone(len(pos), 2)
    got, gw, rejected = S.skin(pos, words, bones, weights, M)
    m = M[2]
    want = np.stack([(m[r, 0] * pos[:, 0] + m[r, 1] * pos[:, 1]) + (m[r, 2] * pos[:, 2] + m[r, 3]) for r in range(3)], axis=1)
    assert want.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and not rejected.any()
    ww, q = _inverse_transpose_words(m, words)
    assert _word_steps(gw, ww) <= 1
    d = S.dequantize_normals(gw).astype(np.float64)
    assert ((d * q).sum(axis=1) / np.linalg.norm(q, axis=1) > 0.9999).all()
    assert not np.array_equal(gw, words)                          # (the non-uniform scale turned the normals)


def test_a_mirroring_bone_flips_the_cofactor_normal_back():
    pos, words = _points(seed=2)
    m = random_transforms(1, 12)[0]
    m[:, 0] = -m[:, 0]                                            # mirrored: det < 0
    assert np.linalg.det(m[:, :3].astype(np.float64)) < 0
    bones, weights = _single_bone(len(pos), 0)
    _, gw, _ = S.skin(pos, words, bones, weights, m[None])
    ww, q = _inverse_transpose_words(m, words)
    assert _word_steps(gw, ww) <= 1
    # ... and without the flip the words would be those of the opposite normals
    raw = S.posed_normals(S.blend(bones, weights, m[None]), words)
    assert ((raw.astype(np.float64) * q).sum(axis=1) > 0).all()   # (posed_normals already negated cof(A) n)
    B = S.blend(bones, weights, m[None])
    cof = np.stack([S.cross(B[:, 1, :3], B[:, 2, :3]), S.cross(B[:, 2, :3], B[:, 0, :3]), S.cross(B[:, 0, :3], B[:, 1, :3])], axis=1)
    unflipped = np.einsum("nrc,nc->nr", cof.astype(np.float64), S.dequantize_normals(words).astype(np.float64))
    assert ((unflipped * q).sum(axis=1) < 0).all()


def test_rejected_vertices_keep_what_they_had():
    pos, words = _points(n=12, seed=3)
    M = random_transforms(2, 13)
    M[1, 1, 2] = np.nan
    bones, weights = _single_bone(len(pos), 0)
    bones[::3, 1] = 1                                             # a zero weight's bone is still read: 0 * NaN = NaN
    got, gw, rejected = S.skin(pos, words, bones, weights, M)
    assert rejected.tolist() == [k % 3 == 0 for k in range(len(pos))]
    assert np.array_equal(got[rejected].view(np.uint32), pos[rejected].view(np.uint32)) and np.array_equal(gw[rejected], words[rejected])
    assert not np.array_equal(got[~rejected], pos[~rejected])


def test_chain_rig_weights_sum_to_65535():
    s = scenes.grid(7, 5, deform_t=0.0)
    P = scenes.dequantize_positions(s.geometries[0].qpos, s.geometries[0].scaling, s.geometries[0].offset)
    for n_bones in (1, 2, 5, 64):
        bones, weights = S.chain_rig(P, n_bones)
        assert bones.shape == weights.shape == (len(P), 4) and bones.dtype == weights.dtype == np.uint16
        assert (weights.astype(np.int64).sum(axis=1) == 65535).all() and int(bones.max()) <= n_bones - 1
    bones, weights = S.chain_rig(P, 5)
    assert len(np.unique(bones[:, 0])) == 4 and ((weights[:, 0] > 0) & (weights[:, 1] > 0)).any()
    # identity bones give the rest pose back to rounding only: the weights are rounded quotients
    got, _, _ = S.skin(P, None, bones, weights, np.tile(scenes.IDENTITY, (5, 1, 1)))
    assert np.abs(got.astype(np.float64) - P).max() <= 4 * 2.0 ** -24 * np.abs(P).max()


def test_cli_refuses_bad_skin_arguments_before_touching_a_device(tmp_path):
    exe = build_host_tool("rptr_cli")
    dyn, static = scenes.grid(7, 5, deform_t=0.0), scenes.grid(7, 5)
    dyn_path, static_path = str(tmp_path / "dyn.rpsc"), str(tmp_path / "static.rpsc")
    dyn.dump(dyn_path)
    static.dump(static_path)
    assert dyn.meshes[0].dynamic & (abi.MESH_DYNAMIC | abi.MESH_SUBTLY_DYNAMIC)
    n = 3 * dyn.geometries[0].num_tris
    skin, bones = str(tmp_path / "skin.bin"), str(tmp_path / "bones.bin")
    b, w = S.chain_rig(scenes.dequantize_positions(dyn.geometries[0].qpos, dyn.geometries[0].scaling, dyn.geometries[0].offset), 5)
    np.concatenate([b, w], axis=1).tofile(skin)
    with open(bones, "wb") as f:
        f.write(struct.pack("<II", 2, 5) + np.tile(scenes.IDENTITY, (10, 1, 1)).astype(f32).tobytes())
    short_skin, short_bones = str(tmp_path / "short_skin.bin"), str(tmp_path / "short_bones.bin")
    np.concatenate([b, w], axis=1)[:n - 1].tofile(short_skin)
    with open(short_bones, "wb") as f:
        f.write(struct.pack("<II", 2, 5) + np.tile(scenes.IDENTITY, (9, 1, 1)).astype(f32).tobytes())
    prof = ["--profiling", str(tmp_path / "p")]
    cases = [([dyn_path] + prof + ["--skin", skin], "go together"),
             ([dyn_path] + prof + ["--bones", bones], "go together"),
             ([dyn_path, "--data-capture", str(tmp_path / "c"), "--skin", skin], "go together"),
             ([dyn_path] + prof + ["--skin", skin, "--bones", bones, "--animate-wave", "0.5", "0.4"], "--animate-wave"),
             ([dyn_path, "--validation", str(tmp_path / "v"), "--skin", skin, "--bones", bones], "validation"),
             ([static_path] + prof + ["--skin", skin, "--bones", bones], "dynamic"),
             ([dyn_path] + prof + ["--skin", short_skin, "--bones", bones], "unrolled vertices"),
             ([dyn_path] + prof + ["--skin", skin, "--bones", short_bones], "float32"),
             ([dyn_path] + prof + ["--skin", str(tmp_path / "missing.bin"), "--bones", bones], "unrolled vertices")]
    for args, text in cases:
        p = subprocess.run([exe] + args, capture_output=True, text=True)
        assert p.returncode == 2 and ("--skin" in p.stderr or "--bones" in p.stderr) and text in p.stderr, (args, p.returncode, p.stderr)
