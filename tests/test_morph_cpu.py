"""Morph targets without a device: the restated arithmetic (tests/morph_ref.py) against plain float64 algebra, its transposition, the
ABI record, and the refusals of bin/rptr_hip --morph / --morph-weights (exit code 2 before a device is touched)."""
import ctypes as C
import struct
import subprocess

import numpy as np

import morph_ref as MR
import skin_ref as S
from common import random_transforms
from host_tools import build_host_tool
from realtimepathtracingresearchframework_amd import abi, backend, scenes

f32 = np.float32
U = 2.0 ** -24                                                    # unit roundoff of binary32


def _points(n=200, seed=1):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-3, 3, (n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pos, scenes.quantize_normals(nrm.astype(f32))


def _targets(n, seed=2, sizes=(None, 40, 1, 0, 25)):
    """sparse targets over n vertices: None = dense; vertices in random order, each at most once per target"""
    rng = np.random.default_rng(seed)
    out = []
    for k in sizes:
        v = rng.permutation(n)[:n if k is None else k].astype(np.uint32)
        out.append((v, rng.uniform(-1, 1, (len(v), 3)).astype(f32), rng.uniform(-0.5, 0.5, (len(v), 3)).astype(f32)))
    return out


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_zero_weights_give_the_rest_pose_bit_for_bit():
    pos, words = _points()
    targets = _targets(len(pos))
    got, gw, rejected = MR.morph(pos, words, targets, np.zeros(len(targets), f32))
    assert np.array_equal(_bits(got), _bits(pos)) and np.array_equal(gw, words) and not rejected.any()
    got, gw, _ = MR.morph(pos, None, targets, np.zeros(len(targets), f32))
    assert np.array_equal(_bits(got), _bits(pos)) and gw is None
    # -0.0 is zero too: the entry is skipped, not added (x + -0.0 * d could turn a -0.0 coordinate into +0.0)
    pos[3] = -0.0
    got, _, _ = MR.morph(pos, words, targets, np.full(len(targets), -0.0, f32))
    assert np.array_equal(_bits(got), _bits(pos))


def test_zero_weights_under_a_skin_are_the_skin_alone():
    pos, words = _points(seed=5)
    targets = _targets(len(pos))
    bones, weights = S.chain_rig(pos, 4)
    M = random_transforms(4, 21)
    M[2, :, 0] = -M[2, :, 0]
    want = S.skin(pos, words, bones, weights, M)
    got = MR.morph(pos, words, targets, np.zeros(len(targets), f32), skin=(bones, weights, M))
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    moved = MR.morph(pos, words, targets, np.array([0.5, 0, 0, 0, 0], f32), skin=(bones, weights, M))
    assert not np.array_equal(_bits(moved[0]), _bits(want[0])) and not np.array_equal(moved[1], want[1])


def test_one_target_at_weight_one_adds_its_deltas_exactly():
    """multiples of 1/8 below 8 on both sides: every product and sum is exact in binary32"""
    rng = np.random.default_rng(7)
    n = 60
    pos = (rng.integers(-64, 64, (n, 3)) / 8.0).astype(f32)
    v = rng.permutation(n)[:25].astype(np.uint32)
    d = (rng.integers(-64, 64, (25, 3)) / 8.0).astype(f32)
    other = (np.arange(n, dtype=np.uint32), np.ones((n, 3), f32), None)
    got, gw, _ = MR.morph(pos, None, [other, (v, d, None)], np.array([0.0, 1.0], f32))
    want = pos.copy()
    want[v] += d
    assert np.array_equal(_bits(got), _bits(want)) and gw is None
    untouched = np.setdiff1d(np.arange(n), v)
    assert np.array_equal(_bits(got[untouched]), _bits(pos[untouched]))


def test_the_restatement_agrees_with_float64_algebra():
    """Per vertex at most K entries are applied; each adds one rounded product (relative error U) and one rounded sum (relative error U
    of the partial sum). With M = |rest| + sum |w| |d| bounding every partial sum and every product, the float32 result differs from the
    exact one by at most K (U M + U M) (1 + U)^(2 K) <= 2 K U M (1 + 4 K U); the inputs are float32 values, exact in float64."""
    pos, words = _points(n=300, seed=3)
    targets = _targets(len(pos), seed=4, sizes=(None, 80, 1, 0, 50, None))
    w = np.array([0.75, -0.4, 1.0, 0.3, 1.6, 0.2], f32)
    p, nrm, applied = MR.morphed_rest(pos, words, targets, w)
    n0 = S.dequantize_normals(words).astype(np.float64)
    exact_p, exact_n = pos.astype(np.float64), n0.copy()
    mag_p, mag_n = np.abs(exact_p), np.abs(n0)
    count = np.zeros(len(pos), np.int64)
    for (v, dp, dn), wt in zip(targets, w.astype(np.float64)):
        exact_p[v] += wt * dp.astype(np.float64)
        exact_n[v] += wt * dn.astype(np.float64)
        mag_p[v] += abs(wt) * np.abs(dp.astype(np.float64))
        mag_n[v] += abs(wt) * np.abs(dn.astype(np.float64))
        count[v] += 1
    K = int(count.max())
    assert 4 <= K <= 5 and count.min() == 2 and applied.all()
    bound = 2 * K * U * (1 + 4 * K * U)
    assert (np.abs(p.astype(np.float64) - exact_p) <= bound * mag_p).all()
    assert (np.abs(nrm.astype(np.float64) - exact_n) <= bound * mag_n).all()
    assert np.abs(p.astype(np.float64) - pos).max() > 0.5                         # (and the targets did move the mesh)


def test_the_order_of_a_targets_deltas_changes_nothing():
    pos, words = _points(seed=6)
    targets = _targets(len(pos), seed=8)
    w = np.array([0.3, 1.2, -0.7, 0.9, 0.5], f32)
    want = MR.morph(pos, words, targets, w)
    rng = np.random.default_rng(9)
    shuffled = []
    for v, dp, dn in targets:
        o = rng.permutation(len(v))
        shuffled.append((v[o], dp[o], dn[o]))
    got = MR.morph(pos, words, shuffled, w)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    a, b = MR.transpose(targets, len(pos)), MR.transpose(shuffled, len(pos))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    offsets, target = a[0], a[1]
    assert offsets[0] == 0 and offsets[-1] == sum(len(t[0]) for t in targets)
    for i in range(len(pos)):                                                     # ascending target index within every vertex
        assert (np.diff(target[offsets[i]:offsets[i + 1]]) > 0).all()


def test_the_run_fixture_can_see_an_order_error():
    """the fixture of tests/test_gpu_morph.py section 9 (runs of 0 ... 13 and 40 entries on a four-entry fetch): the restatement with
    every vertex's entries applied in reverse, and with its entries 4 ... applied before its entries 0-3, gives other position bits for
    at least half of the vertices that have five entries or more -- a kernel that walked a run or its trips in another order could not
    pass the bit-for-bit comparison. Vertices of up to four entries are one trip: the swap leaves them alone."""
    P, words = MR.grid_rest_pose()
    n = len(P)
    targets = MR.run_targets(P)
    assert len(targets) == abi.MAX_MORPH_TARGETS and n == 210
    sets = MR.run_weight_sets(targets, n)
    w = sets["mixed"][0]
    tr = MR.transpose(targets, n)
    count = np.diff(tr[0])
    want = MR.morph(P, words, targets, w, transposed=tr)
    assert not want[2].any()
    long = count >= 5
    assert long.sum() > 100
    for kind in ("reversed", "trips-swapped"):
        got = MR.morph(P, words, targets, w, transposed=MR.reordered(tr, kind))
        changed = (_bits(got[0]) != _bits(want[0])).any(axis=1)
        print("%s: position bits change for %.3f of the vertices with five entries or more" % (kind, changed[long].mean()))
        assert changed[long].mean() >= 0.5, (kind, changed[long].mean())
        if kind == "trips-swapped":
            assert not changed[count <= 4].any()
    # the weight sets say what they claim, and the special cases leave their mark on the reference: a word that is re-quantised,
    # one rejected vertex
    offsets, target = tr[0], tr[1]
    for name, zeroed in (("first-four-zero", [0, 1, 2, 3]), ("entry-3-zero", [3]), ("entry-4-zero", [4])):
        wk, v = sets[name]
        assert count[v] >= 5 and np.array_equal(np.nonzero(wk[target[offsets[v]:offsets[v + 1]]] == 0)[0], zeroed)
    wk, v = sets["first-four-zero"]
    got = MR.morph(P, words, targets, wk, transposed=tr)
    assert got[1][v] != words[v] and not np.array_equal(_bits(got[0][v]), _bits(P[v]))
    wk, v = sets["nan"]
    rejected = MR.morph(P, words, targets, wk, transposed=tr)[2]
    assert rejected.sum() == 1 and rejected[v]
    k = int(np.nonzero(np.isnan(wk[target[offsets[v]:offsets[v + 1]]]))[0][0])
    assert 4 <= k < 8


def test_abi_records():
    assert C.sizeof(abi.MorphDelta) == 32 and np.dtype(abi.MORPH_DELTA_DTYPE).itemsize == 32
    assert C.sizeof(abi.MorphTargetDesc) == 16 and abi.MAX_MORPH_TARGETS == 1024
    assert abi.MorphDelta.dpos.offset == 4 and abi.MorphDelta.dnrm.offset == 16 and getattr(abi.MorphDelta, "_pad").offset == 28
    rec = backend.RenderHip.morph_deltas([5, 2], [[1, 2, 3], [4, 5, 6]], None)
    assert rec.tobytes() == struct.pack("<I6fI", 5, 1, 2, 3, 0, 0, 0, 0) + struct.pack("<I6fI", 2, 4, 5, 6, 0, 0, 0, 0)
    for name in ("rptr_hip_set_morph_targets", "rptr_hip_update_morph_weights", "rptr_hip_update_morph_weights_device"):
        assert name in abi.EXPORTED_SYMBOLS


def test_cli_refuses_bad_morph_arguments_before_touching_a_device(tmp_path):
    exe = build_host_tool("rptr_cli")
    dyn, static = scenes.grid(7, 5, deform_t=0.0), scenes.grid(7, 5)
    dyn_path, static_path = str(tmp_path / "dyn.rpsc"), str(tmp_path / "static.rpsc")
    dyn.dump(dyn_path)
    static.dump(static_path)
    n = 3 * dyn.geometries[0].num_tris
    targets = _targets(n, sizes=(None, 20, 0))

    def write(name, data):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        return path

    morph = write("morph.bin", MR.morph_file(targets))
    weights = write("weights.bin", MR.weights_file(np.full((2, 3), 0.5)))
    short_morph = write("short_morph.bin", MR.morph_file(targets)[:-1])
    beyond = [targets[0], (np.array([n], np.uint32), np.ones((1, 3), f32), None), targets[2]]
    beyond_morph = write("beyond_morph.bin", MR.morph_file(beyond))
    short_weights = write("short_weights.bin", MR.weights_file(np.full((2, 3), 0.5))[:-4])
    four_weights = write("four_weights.bin", MR.weights_file(np.full((2, 4), 0.5)))
    prof = ["--profiling", str(tmp_path / "p")]
    both = ["--morph", morph, "--morph-weights", weights]
    cases = [([dyn_path] + prof + ["--morph", morph], "go together"),
             ([dyn_path] + prof + ["--morph-weights", weights], "go together"),
             ([dyn_path, "--data-capture", str(tmp_path / "c"), "--morph", morph], "go together"),
             ([dyn_path] + prof + both + ["--animate-wave", "0.5", "0.4"], "--animate-wave"),
             ([dyn_path, "--validation", str(tmp_path / "v")] + both, "validation"),
             ([static_path] + prof + both, "dynamic"),
             ([dyn_path] + prof + ["--morph", short_morph, "--morph-weights", weights], "unrolled vertices"),
             ([dyn_path] + prof + ["--morph", beyond_morph, "--morph-weights", weights], "unrolled vertices"),
             ([dyn_path] + prof + ["--morph", str(tmp_path / "missing.bin"), "--morph-weights", weights], "unrolled vertices"),
             ([dyn_path] + prof + ["--morph", morph, "--morph-weights", short_weights], "float32"),
             ([dyn_path] + prof + ["--morph", morph, "--morph-weights", four_weights], "4 targets")]
    for args, text in cases:
        p = subprocess.run([exe] + args, capture_output=True, text=True)
        assert p.returncode == 2 and "--morph" in p.stderr and text in p.stderr, (args, p.returncode, p.stderr)
