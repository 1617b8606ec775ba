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


# ---- runs of entries across rp_k_morph's four-entry fetch (RP_MORPH_CHUNK): the fixture of tests/test_gpu_morph.py section 9, and the
# reorderings tests/test_morph_cpu.py uses to show that the fixture can see an order error
RUN_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13)   # under a chunk, a full chunk, one and two chunks with every remainder, three chunks + 1
LONG_RUN = 40                                       # ten trips


def grid_rest_pose(nx=7, nz=5):
    """(positions, normal words) of geometry 0 of scenes.grid(nx, nz, deform_t=0.0) as set_scene uploads them"""
    geo = scenes.grid(nx, nz, deform_t=0.0).geometries[0]
    return scenes.dequantize_positions(geo.qpos, geo.scaling, geo.offset), (np.asarray(geo.qnrm_uv, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def run_targets(P, n_targets=1024, seed=11):
    """n_targets sparse targets over the vertices P such that vertex v has RUN_LENGTHS[v % 11] entries and the middle vertex LONG_RUN, on
    target indices drawn from all of 0 .. n_targets - 1 (the last one is used). Every delta component is uniform(-1, 1) * 2^uniform(-6, 6),
    positions times 1/64 of the mesh's extent: partial sums of very different magnitude, so the order of a run's sum shows in its bits."""
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    rng = np.random.default_rng(seed)
    size = float((P.max(axis=0) - P.min(axis=0)).max())
    count = np.array([RUN_LENGTHS[v % len(RUN_LENGTHS)] for v in range(n)], np.int64)
    count[n // 2] = LONG_RUN
    listed = [[] for _ in range(n_targets)]
    for v in rng.permutation(n).tolist():                           # (a target lists its vertices in random order)
        if v == n // 2:
            ts = np.concatenate([rng.choice(n_targets - 1, LONG_RUN - 1, replace=False), [n_targets - 1]])
        else:
            ts = rng.choice(n_targets, count[v], replace=False)
        for t in ts.tolist():
            listed[t].append(v)
    out = []
    for t in range(n_targets):
        v = np.array(listed[t], np.uint32)
        mag = lambda: rng.uniform(-1, 1, (len(v), 3)) * 2.0 ** rng.uniform(-6, 6, (len(v), 3))
        out.append((v, (mag() * (size / 64)).astype(f32), (mag() / 8).astype(f32)))
    counts = np.bincount(np.concatenate([t[0] for t in out]).astype(np.int64), minlength=n)
    assert set(counts.tolist()) == set(RUN_LENGTHS) | {LONG_RUN} and (counts == LONG_RUN).sum() == 1 and len(out[n_targets - 1][0]) > 0
    return out


def run_weight_sets(targets, n, seed=12):
    """-> {name: (weights (len(targets),) float32, the vertex the set is about or None)}: uniform(-1.5, 1.5), none zero ("mixed"), and
    the same with the special cases of the entry loop put on the boundaries of its four-entry trips:
      first-four-zero  entries 0-3 of a vertex of 5 entries have weight 0, entry 4 has not: `applied` is set in the second trip only
      entry-3-zero     only entry 3 of a vertex of 9 entries: the last lane of a full first trip is skipped
      entry-4-zero     only entry 4 of a vertex of 13 entries: the first lane of the second trip is skipped
      zero             every weight
      nan              a NaN on an entry of the second trip (positions 4-7) of a vertex, on a target no other vertex is listed in"""
    offsets, target, _, _ = transpose(targets, n)
    count = np.diff(offsets)
    uses = np.bincount(target, minlength=len(targets))
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.5, 1.5, len(targets)).astype(f32)
    assert (base != 0).all()
    entries = lambda v: target[offsets[v]:offsets[v + 1]]
    sets = {"mixed": (base, None), "zero": (np.zeros(len(targets), f32), None)}
    for name, length, zeroed in (("first-four-zero", 5, [0, 1, 2, 3]), ("entry-3-zero", 9, [3]), ("entry-4-zero", 13, [4])):
        v = int(np.nonzero(count == length)[0][0])
        w = base.copy()
        w[entries(v)[zeroed]] = 0
        z = w[entries(v)] == 0
        assert np.array_equal(np.nonzero(z)[0], zeroed), name
        sets[name] = (w, v)
    lone = [(v, k) for v in np.nonzero(count > 4)[0].tolist() for k in range(4, min(int(count[v]), 8)) if uses[entries(v)[k]] == 1]
    assert lone
    v, k = lone[0]
    w = base.copy()
    w[entries(v)[k]] = np.nan
    sets["nan"] = (w, v)
    return sets


def reordered(transposed, kind):
    """transpose()'s arrays with every vertex's entries "reversed", or with its entries 4 ... in front of its entries 0-3 ("trips-swapped"):
    what a kernel would sum that walked a run backwards, or took its trips in the wrong order"""
    offsets, target, dpos, dnrm = transposed
    perm = np.arange(len(target))
    for v in range(len(offsets) - 1):
        a, b = int(offsets[v]), int(offsets[v + 1])
        if kind == "reversed":
            perm[a:b] = np.arange(a, b)[::-1]
        else:
            assert kind == "trips-swapped"
            perm[a:b] = np.concatenate([np.arange(min(a + 4, b), b), np.arange(a, min(a + 4, b))])
    return offsets, target[perm], dpos[perm], dnrm[perm]


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
