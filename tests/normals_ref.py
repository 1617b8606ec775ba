"""The arithmetic of csrc/normals.h in numpy float32, operation by operation (include/rptr_hip.h "recomputed normals"): every product,
difference and sum is rounded to binary32 on its own, in the kernels' order, so the results are compared bit for bit.

    triangle t, corners p0 p1 p2 = positions[3t .. 3t+2]:  e1 = p1 - p0,  e2 = p2 - p0
      f = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x)
    group with members c_0 < c_1 < ...:  n = f(c_0 / 3);  n = n + f(c_k / 3), k = 1, 2, ... (left to right); FLAT corner i: n = f(i / 3)
    flip: n = -n;  word = scenes.quantize_normals(n) unless n is not finite or all zero (the corner keeps its previous word)

Arrays stay float32 throughout (numpy rounds every elementwise operation of two float32 operands to float32)."""
import numpy as np

from realtimepathtracingresearchframework_amd import abi, scenes

f32 = np.float32
FLAT = abi.NORMAL_GROUP_FLAT


def face_normals(positions):
    """(t, 3) float32: the area-weighted face normal of every triangle of unrolled positions (3 t, 3)"""
    p = np.asarray(positions, f32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        a = np.stack([e1[:, 1] * e2[:, 2], e1[:, 2] * e2[:, 0], e1[:, 0] * e2[:, 1]], axis=1)
        b = np.stack([e1[:, 2] * e2[:, 1], e1[:, 0] * e2[:, 2], e1[:, 1] * e2[:, 0]], axis=1)
        f = a - b
    assert f.dtype == f32
    return f


def dense_groups(groups):
    """the labels renumbered densely by first occurrence, every FLAT corner a group of its own -> (n,) int64"""
    out = np.empty(len(groups), np.int64)
    ids = {}
    count = 0
    for v, label in enumerate(np.asarray(groups, np.uint32).tolist()):
        if label == FLAT:
            out[v] = count
            count += 1
            continue
        if label not in ids:
            ids[label] = count
            count += 1
        out[v] = ids[label]
    return out


def transpose(groups):
    """-> (offsets (g + 1,), members (n,)): the per-group lists of member corners, every list in ascending unrolled vertex index"""
    dense = dense_groups(groups)
    n_groups = int(dense.max()) + 1 if len(dense) else 0
    members = np.argsort(dense, kind="stable")          # (stable: corners of one group stay in ascending order)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(dense, minlength=n_groups))])
    return offsets.astype(np.int64), members.astype(np.int64)


def group_sums(positions, groups):
    """(n, 3) float32: per corner the sum of its group's face normals, first member first, the others added left to right"""
    f = face_normals(positions)
    offsets, members = transpose(groups)
    first, sizes = offsets[:-1], np.diff(offsets)
    assert (sizes > 0).all()
    s = f[members[first] // 3].copy()                   # n = f(c_0 / 3) of every group ...
    with np.errstate(all="ignore"):
        for k in range(1, int(sizes.max()) if len(sizes) else 0):
            sel = sizes > k                             # ... then, for all groups at once, their k-th member: each group's own order is kept
            s[sel] = s[sel] + f[members[first[sel] + k] // 3]
    assert s.dtype == f32
    n = np.zeros((len(members), 3), f32)
    n[members] = np.repeat(s, sizes, axis=0)
    return n


def recompute(positions, groups, prev_words, flip=False):
    """-> (normal words (n,) uint32, kept (n,) bool): what rptr_hip_recompute_normals leaves in the geometry's array of normal words.
    prev_words: what a corner whose sum is not finite or all zero keeps"""
    n = group_sums(positions, groups)
    if flip:
        n = -n
    prev_words = np.asarray(prev_words, np.uint32)
    keep = ~np.isfinite(n).all(axis=1) | (n == 0).all(axis=1)
    with np.errstate(all="ignore"):
        words = scenes.quantize_normals(np.where(keep[:, None], f32(1.0), n).astype(f32))
    return np.where(keep, prev_words, words).astype(np.uint32), keep


def unroll(vertices, indices):
    """an indexed mesh as the library wants it: (positions (3 t, 3) float32, groups (3 t,) uint32 = the index buffer)"""
    idx = np.asarray(indices, np.int64).reshape(-1)
    return np.ascontiguousarray(np.asarray(vertices, f32)[idx]), idx.astype(np.uint32)


def order_sensitive_fan():
    """three triangles that share the origin as corner 0, with face normals (0, 0, 2^24), (1, 0, 1), (0, 0, -2^24): left to right the 1 in z
    is rounded away, (0 + 2^24 + 1) - 2^24 = 0 in binary32, and the normal is +x; any order that cancels the large terms first gives
    (1, 0, 1). -> (positions, groups: the three origin corners are one group, all others FLAT)"""
    P = np.array([[0, 0, 0], [4096, 0, 0], [0, 4096, 0],
                  [0, 0, 0], [0, 1, 0], [-1, 0, 1],
                  [0, 0, 0], [0, 4096, 0], [4096, 0, 0]], f32)
    groups = np.full(9, FLAT, np.uint32)
    groups[[0, 3, 6]] = 77
    return P, groups
