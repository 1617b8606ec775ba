"""The arithmetic of csrc/morph.h rp_k_morph in numpy float32, operation by operation (include/rptr_hip.h "morph targets"): every product
and sum is rounded to binary32 on its own, in the kernel's order, so the results are compared bit for bit.

    p = rest_pos[i];  n = dequantize_normal(rest_word[i])
    for each entry (t, dpos, dnrm) of vertex i, in ascending target index:  w = weight[t];  w == 0: skipped
        p[c] = p[c] + w * dpos[c];  n[c] = n[c] + w * dnrm[c]
    no skin: p' = p, q = n; no entry applied: the word is rest_word[i] itself
    skin:    B = blend, p' = (B0 x + B1 y) + (B2 z + B3), q = cof(A) n, negated when det A < 0   (tests/skin_ref.py)
    word = scenes.quantize_normals(q) unless q is not finite or all zero (the previous word stays)

It also restates the transposition the library does once per binding: a per-vertex list of entries sorted by (vertex, target). A target is
(vertex uint32[k], dpos float32[k, 3], dnrm float32[k, 3] or None), the form backend.RenderHip.set_morph_targets takes."""
import struct

import numpy as np

import skin_ref as S
from realtimepathtracingresearchframework_amd import backend, scenes

f32 = np.float32


def transpose(targets, n):
    """-> (offsets (n + 1,) int64, target (E,) int64, dpos (E, 3) float32, dnrm (E, 3) float32): the entries of vertex i are rows
    offsets[i] .. offsets[i + 1], in ascending target index"""
    vertex = np.concatenate([np.asarray(t[0], np.int64).reshape(-1) for t in targets] + [np.zeros(0, np.int64)])
    target = np.concatenate([np.full(len(np.asarray(t[0]).reshape(-1)), k, np.int64) for k, t in enumerate(targets)] + [np.zeros(0, np.int64)])
    dpos = np.concatenate([np.asarray(t[1], f32).reshape(-1, 3) for t in targets] + [np.zeros((0, 3), f32)])
    dnrm = np.concatenate([(np.zeros((len(np.asarray(t[0]).reshape(-1)), 3), f32) if t[2] is None else np.asarray(t[2], f32).reshape(-1, 3)) for t in targets]
                          + [np.zeros((0, 3), f32)])
    assert len(vertex) == 0 or (vertex.min() >= 0 and vertex.max() < n)
    assert len(np.unique(vertex * len(targets) + target)) == len(vertex), "a vertex appears twice within one target"
    order = np.lexsort((target, vertex))
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(vertex, minlength=n), out=offsets[1:])
    return offsets, target[order], dpos[order], dnrm[order]


def morphed_rest(rest_pos, rest_words, targets, weights, transposed=None):
    """-> (p (n, 3) float32, normals (n, 3) float32 or None, applied (n,) bool): the rest pose after the entries, before any skin.
    transposed: transpose(targets, n), for callers that morph the same targets more than once"""
    p = np.array(rest_pos, f32).reshape(-1, 3)
    n = len(p)
    nrm = None if rest_words is None else S.dequantize_normals(rest_words).copy()
    weights = np.asarray(weights, f32).reshape(-1)
    assert len(weights) == len(targets)
    offsets, target, dpos, dnrm = transpose(targets, n) if transposed is None else transposed
    count = offsets[1:] - offsets[:-1]
    applied = np.zeros(n, bool)
    for k in range(int(count.max()) if n else 0):                  # the k-th entry of every vertex that has one
        v = np.nonzero(count > k)[0]
        e = offsets[v] + k
        w = weights[target[e]]
        use = w != 0                                               # (NaN != 0: a NaN weight is applied, and rejected by its result)
        v, e, w = v[use], e[use], w[use, None]
        p[v] = p[v] + w * dpos[e]
        if nrm is not None:
            nrm[v] = nrm[v] + w * dnrm[e]
        applied[v] = True
    assert p.dtype == f32 and (nrm is None or nrm.dtype == f32)
    return p, nrm, applied


def morph(rest_pos, rest_words, targets, weights, skin=None, prev_pos=None, prev_words=None, transposed=None):
    """-> (positions (n, 3) float32, normal words (n,) uint32 or None, rejected (n,) bool). skin: None or (bones (n, 4), weights (n, 4),
    M (B, 3, 4)). prev_*: what a rejected vertex keeps (default: the rest pose, which is what the arrays hold before the first call)"""
    rest_pos = np.asarray(rest_pos, f32).reshape(-1, 3)
    prev_pos = rest_pos if prev_pos is None else np.asarray(prev_pos, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p, nrm, applied = morphed_rest(rest_pos, rest_words, targets, weights, transposed)
        if skin is not None:
            B = S.blend(*skin)
            x, y, z = p[:, 0, None], p[:, 1, None], p[:, 2, None]
            p = (B[:, :, 0] * x + B[:, :, 1] * y) + (B[:, :, 2] * z + B[:, :, 3])
            assert p.dtype == f32
        rejected = ~np.isfinite(p).all(axis=1)
        pos = np.where(rejected[:, None], prev_pos, p).astype(f32)
        if rest_words is None:
            return pos, None, rejected
        rest_words = np.asarray(rest_words, np.uint32)
        prev_words = rest_words if prev_words is None else np.asarray(prev_words, np.uint32)
        if skin is not None:
            A0, A1, A2 = B[:, 0, :3], B[:, 1, :3], B[:, 2, :3]
            C0, C1, C2 = S.cross(A1, A2), S.cross(A2, A0), S.cross(A0, A1)
            q = np.stack([S.dot(C0, nrm), S.dot(C1, nrm), S.dot(C2, nrm)], axis=1)
            q = np.where((S.dot(A0, C0) < 0)[:, None], -q, q)
        else:
            q = nrm
        assert q.dtype == f32
        keep = rejected | ~np.isfinite(q).all(axis=1) | (q == 0).all(axis=1)
        words = np.where(keep, prev_words, scenes.quantize_normals(np.where(keep[:, None], f32(1.0), q).astype(f32)))
        if skin is None:
            words = np.where(~applied & ~rejected, rest_words, words)  # untouched: the rest word itself, nothing is re-quantised
    return pos, words.astype(np.uint32), rejected


# ---- the files bin/rptr_hip --morph / --morph-weights reads (host/rptr_cli.cpp)
def morph_file(targets):
    """the file bin/rptr_hip --morph reads: uint32 targets, then per target uint32 deltas and that many RptrMorphDelta records"""
    out = struct.pack("<I", len(targets))
    for t in targets:
        rec = backend.RenderHip.morph_deltas(*t)
        out += struct.pack("<I", len(rec)) + rec.tobytes()
    return out


def weights_file(frames):
    frames = np.ascontiguousarray(frames, f32)
    return struct.pack("<II", frames.shape[0], frames.shape[1]) + frames.tobytes()
