"""Recomputed normals without a device: the restated arithmetic (tests/normals_ref.py) on shapes whose answers are exact, the grouping
(transpose, ascending member order, the FLAT sentinel, the flip flag, the keep-previous-word rule), the welding helper in Python and in
C++ (host/normal_groups.hpp, as a stand-alone program under AddressSanitizer and UBSan), and the ABI's declarations."""
import os
import re
import subprocess

import numpy as np

import normals_ref as NR
from host_tools import ROOT, build_host_tool
from realtimepathtracingresearchframework_amd import abi, backend, scenes

f32 = np.float32
FLAT = NR.FLAT


def _word(x, y, z):
    return int(scenes.quantize_normals(np.array([[x, y, z]], f32))[0])


def _flat_grid(nx=4, ny=3):
    """an indexed grid in the plane z = 0, wound counter-clockwise seen from +z"""
    X, Y = np.meshgrid(np.arange(nx + 1, dtype=f32) * f32(0.75), np.arange(ny + 1, dtype=f32) * f32(1.25), indexing="ij")
    V = np.stack([X, Y, np.zeros_like(X)], axis=-1).reshape(-1, 3)
    idx = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
            idx += [[a, b, c], [a, c, d]]
    return NR.unroll(V, idx)


def test_a_flat_grid_points_along_z_and_flips():
    P, groups = _flat_grid()
    prev = np.full(len(P), 0x12345678, np.uint32)
    words, kept = NR.recompute(P, groups, prev)
    assert not kept.any() and (words == _word(0, 0, 1)).all()
    words, kept = NR.recompute(P, groups, prev, flip=True)
    assert not kept.any() and (words == _word(0, 0, -1)).all()
    assert _word(0, 0, 1) != _word(0, 0, -1)


def test_a_cube_of_flat_corners_has_axis_normals():
    quads = []          # (corners counter-clockwise seen from outside, outward axis)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0.0, 1.0):
            c = np.zeros((4, 3), f32)
            c[:, axis] = side
            c[:, u] = (0, 1, 1, 0)
            c[:, v] = (0, 0, 1, 1)
            if side == 0.0:
                c = c[::-1]
            n = np.zeros(3, f32)
            n[axis] = 1.0 if side else -1.0
            quads.append((c, n))
    P = np.concatenate([np.stack([c[0], c[1], c[2], c[0], c[2], c[3]]) for c, _ in quads])
    words, kept = NR.recompute(P, np.full(len(P), FLAT, np.uint32), np.zeros(len(P), np.uint32))
    assert len(P) == 36 and not kept.any()
    for k, (_, n) in enumerate(quads):
        assert (words[6 * k:6 * k + 6] == _word(*n)).all(), (k, n)
    assert len(set(words.tolist())) == 6


def _octahedron():
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    idx = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                tri = [sx, sy, sz]
                if (sx == 1) ^ (sy == 3) ^ (sz == 5):      # an odd number of mirrored axes turns the winding round
                    tri = [sx, sz, sy]
                idx.append(tri)
    return V, np.array(idx)


def test_a_welded_octahedron_has_axis_normals():
    V, idx = _octahedron()
    P, groups = NR.unroll(V, idx)
    f = NR.face_normals(P)
    assert (np.abs(f) == 1).all() and (np.einsum("ij,ij->i", f, P.reshape(-1, 3, 3).sum(axis=1)) > 0).all()      # (±1, ±1, ±1), outward
    sums = NR.group_sums(P, groups)
    words, kept = NR.recompute(P, groups, np.zeros(len(P), np.uint32))
    assert not kept.any()
    for corner, vertex in enumerate(groups):
        assert np.array_equal(sums[corner], 4 * V[vertex])                                # the four face normals sum exactly
        assert words[corner] == _word(*V[vertex])


def test_the_sum_runs_left_to_right_in_ascending_member_order():
    P, groups = NR.order_sensitive_fan()
    f = NR.face_normals(P)
    assert np.array_equal(f, np.array([[0, 0, 2.0 ** 24], [1, 0, 1], [0, 0, -2.0 ** 24]], f32))
    stated = (f[0] + f[1]) + f[2]
    other = (f[0] + f[2]) + f[1]
    assert np.array_equal(stated, np.array([1, 0, 0], f32)) and np.array_equal(other, np.array([1, 0, 1], f32))
    assert _word(*stated) != _word(*other)
    words, kept = NR.recompute(P, groups, np.zeros(9, np.uint32))
    assert not kept.any()
    assert (words[[0, 3, 6]] == _word(1, 0, 0)).all()
    assert words[1] == words[2] == _word(0, 0, 1) and words[4] == words[5] == _word(1, 0, 1) and words[7] == words[8] == _word(0, 0, -1)


def test_transpose_sentinel_and_first_occurrence_numbering():
    groups = np.array([9, FLAT, 4, 4, 9, FLAT, 9, 0xFFFFFFFE, 4], np.uint32)
    assert NR.dense_groups(groups).tolist() == [0, 1, 2, 2, 0, 3, 0, 4, 2]
    offsets, members = NR.transpose(groups)
    assert offsets.tolist() == [0, 3, 4, 7, 8, 9]
    assert members.tolist() == [0, 4, 6, 1, 2, 3, 8, 5, 7]
    lists = [members[offsets[g]:offsets[g + 1]] for g in range(5)]
    assert all((np.diff(m) > 0).all() for m in lists)                                     # ascending within every group
    assert sorted(members.tolist()) == list(range(9))                                     # every corner exactly once


def test_a_triangle_with_two_corners_in_one_group_contributes_twice():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 3], [1, 0, 0]], f32)       # f = (0, 0, 1) and (0, 3, 0)
    groups = np.array([5, 5, FLAT, 5, FLAT, FLAT], np.uint32)
    sums = NR.group_sums(P, groups)
    assert np.array_equal(sums[0], np.array([0, 3, 2], f32)) and np.array_equal(sums[1], sums[0]) and np.array_equal(sums[3], sums[0])
    assert np.array_equal(sums[2], np.array([0, 0, 1], f32)) and np.array_equal(sums[4], np.array([0, 3, 0], f32))


def test_unusable_sums_keep_the_previous_word():
    huge = f32(3e38)
    P = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0],                                         # zero area, alone in group 1
                  [0, 0, 0], [1, 0, 0], [0, 1, 0],                                         # a live triangle ...
                  [0, 0, 0], [0, 0, 0], [0, 0, 0],                                         # ... that shares group 2 with a zero-area one
                  [0, 0, 0], [np.nan, 0, 0], [0, 1, 0],                                    # a NaN coordinate: group 3
                  [0, 0, 0], [huge, 0, 0], [0, huge, 0],                                   # an overflowing product: FLAT corners
                  [0, 0, 0], [np.inf, 0, 0], [0, 1, 0]], f32)                              # an infinite coordinate
    groups = np.array([1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, FLAT, FLAT, FLAT, 4, 4, 4], np.uint32)
    prev = np.arange(100, 118, dtype=np.uint32)
    words, kept = NR.recompute(P, groups, prev)
    assert kept.tolist() == [True] * 3 + [False] * 6 + [True] * 9
    assert np.array_equal(words[kept], prev[kept]) and (words[3:9] == _word(0, 0, 1)).all()


# ------------------------------------------------------------------ the welding helper
def _two_quads(hard):
    """two quads that share the edge x = 1: with equal normals along it (smooth) or with each quad's own (hard)"""
    q0 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 1, 0], [0, 1, 0]], f32)
    q1 = np.array([[1, 0, 0], [2, 0, 1], [2, 1, 1], [1, 0, 0], [2, 1, 1], [1, 1, 0]], f32)
    n0, n1 = np.array([0, 0, 1], f32), np.array([-1, 0, 1], f32)
    N = np.concatenate([np.tile(n0, (6, 1)), np.tile(n1, (6, 1))])
    P = np.concatenate([q0, q1])
    if not hard:
        on_edge = P[:, 0] == 1
        N[on_edge] = n0 + n1
    return P, scenes.quantize_normals(N)


def test_the_python_helper_welds_smooth_vertices_and_keeps_hard_edges():
    P, words = _two_quads(hard=False)
    g = scenes.normal_groups(P, words)
    assert g.dtype == np.uint32 and g.tolist() == [0, 1, 2, 0, 2, 3, 1, 4, 5, 1, 5, 2]     # numbered by first occurrence; the edge welds
    P, words = _two_quads(hard=True)
    g = scenes.normal_groups(P, words)
    assert g.tolist() == [0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7]                             # the edge's corners stay apart
    # bitwise: 0.0 and -0.0 are different corners
    P2 = np.array([[0.0, 0, 0], [-0.0, 0, 0], [0.0, 0, 0]], f32)
    assert scenes.normal_groups(P2, np.zeros(3, np.uint32)).tolist() == [0, 1, 0]


def _tool_groups(tmp_path, name, P, words):
    exe = build_host_tool("normal_groups_tool", link_library=False, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    with open(src, "wb") as f:
        f.write(np.uint32(len(words)).tobytes() + np.ascontiguousarray(P, f32).tobytes() + np.ascontiguousarray(words, np.uint32).tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
    return np.fromfile(dst, np.uint32)


def test_the_cpp_helper_gives_the_same_array(tmp_path):
    for hard in (False, True):
        P, words = _two_quads(hard)
        assert np.array_equal(_tool_groups(tmp_path, "quads%d" % hard, P, words), scenes.normal_groups(P, words))
    geo = scenes.grid(7, 5, deform_t=0.0).geometries[0]
    P = scenes.dequantize_positions(geo.qpos, geo.scaling, geo.offset)
    words = (np.asarray(geo.qnrm_uv, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    P[11, 2] = -0.0
    P[17] = (np.nan, 1, 2)
    P[140] = P[17]                                                  # the same NaN bits: one group, as in Python
    words[140] = words[17]
    want = scenes.normal_groups(P, words)
    assert 40 < len(set(want.tolist())) < len(want) and want[140] == want[17]
    assert np.array_equal(_tool_groups(tmp_path, "grid", P, words), want)
    assert np.array_equal(_tool_groups(tmp_path, "empty", np.zeros((0, 3), f32), np.zeros(0, np.uint32)), np.zeros(0, np.uint32))
    exe = build_host_tool("normal_groups_tool", link_library=False, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    short = tmp_path / "short.in"
    short.write_bytes(np.uint32(5).tobytes() + b"\0" * 10)
    p = subprocess.run([exe, str(short), str(tmp_path / "short.out")], capture_output=True, text=True)
    assert p.returncode == 2 and "does not hold" in p.stderr


def test_the_welded_grid_has_the_valences_of_an_indexed_grid():
    geo = scenes.grid(5, 4, deform_t=0.0).geometries[0]
    P = scenes.dequantize_positions(geo.qpos, geo.scaling, geo.offset)
    words = (np.asarray(geo.qnrm_uv, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    g = scenes.normal_groups(P, words)
    assert len(g) == 120 and g.max() + 1 == 30                                            # 6 x 5 grid points
    assert set(np.bincount(g).tolist()) == {1, 2, 3, 6}


# ------------------------------------------------------------------ declarations
def test_the_abi_declares_the_calls_and_restates_the_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    assert re.search(r"^#define RPTR_NORMAL_GROUP_FLAT 0xFFFFFFFFu$", hdr, re.M) and abi.NORMAL_GROUP_FLAT == 0xFFFFFFFF
    assert re.search(r"^#define RPTR_NORMALS_FLIP 1u\b", hdr, re.M) and abi.NORMALS_FLIP == 1
    assert "int rptr_hip_set_normal_groups(rptr_hip_t *h, uint32_t geometry, const uint32_t *group, uint32_t num_vertices, uint32_t flags);" in hdr
    assert "int rptr_hip_recompute_normals(rptr_hip_t *h);" in hdr
    for text in ("e1 = p1 - p0,  e2 = p2 - p0", "e1.y*e2.z - e1.z*e2.y", "n = f(c_0 / 3)", "angle weighting is out of scope", "keeps its previous word"):
        assert text in hdr, text
    L = backend.load_library()
    for name, nargs in (("rptr_hip_set_normal_groups", 5), ("rptr_hip_recompute_normals", 1)):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert "#define RPTR_HIP_ABI_VERSION 5" in hdr and L.rptr_hip_abi_version() == 5       # the ABI version stays
    assert L.rptr_hip_option_count() == 22                                                # no counter, no option came with it
    for method in ("set_normal_groups", "recompute_normals"):
        assert callable(getattr(backend.RenderHip, method))
