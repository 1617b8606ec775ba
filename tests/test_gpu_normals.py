"""Recomputed normals on the GPU (csrc/normals.h; rptr_hip_set_normal_groups / recompute_normals / readback_skinned) against
tests/normals_ref.py.

Every comparison is exact: the kernels and the restatement perform the same IEEE binary32 operations in the same order (the library is
built without contraction; a group's face normals are summed left to right in ascending unrolled vertex index on both sides).

Shapes. The bit-for-bit cases use one geometry of 87 triangles = 261 unrolled vertices (one full 256-lane block plus a remainder): a
wave-deformed 5 x 4-quad grid welded by index, two of its quads cut along the other diagonal (valences 1 to 7), a fan of 9 triangles round a hub, 37 loose
triangles whose corners are labelled into groups of 1, 2, 3, 4, 5, 7 and 8 members (every remainder of the four-wide fetch loop) with
several FLAT corners, and one triangle with two corners in one group; and one geometry of 70 triangles with a single hub group of 70
members. The renderer cases use test_gpu_skin's scene (scenes.grid(7, 5) as a dynamic mesh) at 32 x 32, 1 spp."""
import copy
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import normals_ref as NR
import skin_ref as S
import test_gpu_skin as TS
from common import config, float_bits, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

W = H = 32
f32 = np.float32
FLAT = NR.FLAT


# ------------------------------------------------------------------ shapes
def _soup_scene(P, seed=3):
    """one dynamic mesh of the unrolled triangles P with random unit normals: the words set_scene uploads are the 'previous' words"""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(len(P), 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    s = scenes.Scene(name="normals-soup")
    m = scenes._add_mesh(s, np.asarray(P, f32).reshape(-1, 3, 3), normals=N.astype(f32), dynamic=abi.MESH_DYNAMIC)
    s.pmeshes.append(scenes.ParameterizedMesh(mesh=m, material_offsets=np.array([0], np.int32)))
    s.instances.append(scenes.Instance(transform=scenes.IDENTITY.copy(), pmesh=0))
    s.materials = [abi.make_material((0.7, 0.7, 0.7), roughness=0.5)]
    s.camera = dict(eye=(0, 12, 40), center=(0, 0, 0), up=(0, 1, 0), fov=65.0)
    s.config = scenes.SceneConfig(**scenes.SKY_CONFIGS["default"])
    s.sky_key = "default"
    s.prepare_lights()
    return s


def _mixed_shape(seed=21):
    """-> (positions (261, 3) float32, groups (261,) uint32)"""
    rng = np.random.default_rng(seed)
    # the grid: 6 x 5 points under a wave, two quads cut along the other diagonal -> valences 1 to 7
    X, Z = np.meshgrid(np.arange(6, dtype=np.float64) * 1.5, np.arange(5, dtype=np.float64) * 1.25, indexing="ij")
    Y = 0.8 * np.sin(0.9 * X + 0.3) + 0.5 * np.cos(1.1 * Z)
    V = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(f32)
    idx = []
    for i in range(5):
        for j in range(4):
            a, b, c, d = i * 5 + j, i * 5 + j + 1, (i + 1) * 5 + j + 1, (i + 1) * 5 + j
            idx += [[a, b, d], [b, c, d]] if i == 2 and j < 2 else [[a, b, c], [a, c, d]]
    grid_p, grid_g = NR.unroll(V, idx)
    assert set(np.bincount(grid_g).tolist()) >= {1, 2, 3, 4, 5, 6} and len(grid_p) == 120
    grid_g = grid_g.copy()
    grid_g[[9, 10, 11, 51, 52, 53, 25]] = FLAT                       # two whole triangles and one lone corner
    # the fan: 9 triangles round a hub (label 1000), neighbouring rim corners welded in pairs (labels 1001 ...)
    rim = np.stack([10 + 2 * np.cos(np.arange(9) * 0.7), 1 + 0.3 * np.arange(9), 2 * np.sin(np.arange(9) * 0.7)], axis=1)
    hub = np.array([10, 2.5, 0.0])
    fan_p = np.concatenate([np.stack([hub, rim[k], rim[(k + 1) % 9]]) for k in range(9)]).astype(f32)
    fan_g = np.concatenate([[1000, 1001 + k, 1001 + (k + 1) % 9] for k in range(9)]).astype(np.uint32)
    # 38 loose triangles; their 114 corners labelled into groups of 8, 7, 5, 4, 3 (2000 ...), FLAT corners and single labels
    loose_p = (rng.uniform(-6, 6, (38, 1, 3)) + rng.uniform(-1.5, 1.5, (38, 3, 3))).reshape(-1, 3).astype(f32)
    loose_g = (3000 + np.arange(114)).astype(np.uint32)              # singles: every label once
    order = rng.permutation(np.arange(3, 114))                       # (corners 0, 1, 2: the triangle with two corners in one group)
    at = 0
    for label, size in ((2000, 8), (2001, 7), (2002, 3), (2003, 4), (2004, 3), (2005, 7), (2006, 8)):
        loose_g[order[at:at + size]] = label
        at += size
    loose_g[order[at:at + 12]] = FLAT
    loose_g[[0, 1]] = 2002                                            # ... the group of 3 becomes one of 5, two of them in triangle 0
    P = np.concatenate([grid_p, fan_p, loose_p])
    G = np.concatenate([grid_g, fan_g, loose_g])
    assert len(P) == 261 and len(P) // 3 == 87
    sizes = set(np.bincount(NR.dense_groups(G)).tolist())
    assert sizes >= {1, 2, 3, 4, 5, 6, 7, 8, 9}, sizes
    return P, G


def _hub_shape(seed=22):
    """70 triangles whose first corners are one group of 70 members (more than a wave's worth); the others FLAT or single"""
    rng = np.random.default_rng(seed)
    P = (rng.uniform(-4, 4, (70, 1, 3)) + rng.uniform(-1, 1, (70, 3, 3))).reshape(-1, 3).astype(f32)
    P[0::3] = (0.5, 0.25, -0.75)
    G = (100 + np.arange(210)).astype(np.uint32)
    G[0::3] = 7
    G[1::6] = FLAT
    return P, G


@pytest.fixture(scope="module")
def mixed():
    P, G = _mixed_shape()
    scene = _soup_scene(P)
    prev = TS._rest(scene, 0)[1]
    return scene, P, G, prev


def _recomputed(r, P, refit=True):
    r.update_vertices(0, P)
    r.recompute_normals()
    if refit:
        r.refit()
    return r.readback_skinned(0)


def _assert_words(got, want, what=""):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s normal words differ at %s" % (what, bad[:8])


# ------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("flip", [False, True])
def test_words_equal_the_reference_bit_for_bit(mixed, flip):
    scene, P, G, prev = mixed
    want, kept = NR.recompute(P, G, prev, flip=flip)
    assert not kept.any() and not np.array_equal(want, prev)
    r = renderer(scene, W, H)
    r.set_normal_groups(0, G, flip=flip)
    xyz, words = _recomputed(r, P)
    assert np.array_equal(float_bits(xyz), float_bits(P))
    _assert_words(words, want)
    if not flip:                                                    # a second call on other positions: nothing of the first survives
        P2 = (P * f32(1.25) + P[:, [1, 2, 0]] * f32(0.5)).astype(f32)
        want2, kept2 = NR.recompute(P2, G, want)
        assert not kept2.any() and not np.array_equal(want2, want)
        _assert_words(_recomputed(r, P2)[1], want2, "second")
    r.close()


@pytest.mark.parametrize("flip", [False, True])
def test_a_hub_of_seventy_members(flip):
    P, G = _hub_shape()
    scene = _soup_scene(P)
    prev = TS._rest(scene, 0)[1]
    want, kept = NR.recompute(P, G, prev, flip=flip)
    assert not kept.any() and np.bincount(NR.dense_groups(G)).max() == 70
    r = renderer(scene, W, H)
    r.set_normal_groups(0, G, flip=flip)
    _assert_words(_recomputed(r, P)[1], want)
    r.close()


def test_the_sum_runs_in_ascending_member_order_on_the_device():
    P, G = NR.order_sensitive_fan()
    scene = _soup_scene(P)
    want, kept = NR.recompute(P, G, TS._rest(scene, 0)[1])
    assert not kept.any() and (want[[0, 3, 6]] == scenes.quantize_normals(np.array([[1, 0, 0]], f32))[0]).all()
    r = renderer(scene, W, H)
    r.set_normal_groups(0, G)
    _assert_words(_recomputed(r, P)[1], want)
    r.close()


# ------------------------------------------------------------------ 2. the keep-previous-word rule
def test_zero_area_triangles_and_a_nan_keep_the_words_of_their_groups_only(mixed):
    """read-backs only after the NaN: the poisoned positions are never refitted, traced or rendered, and finite ones are written before
    the handle closes"""
    scene, P, G, prev = mixed
    r = renderer(scene, W, H)
    r.set_normal_groups(0, G)
    first, _ = NR.recompute(P, G, prev)
    _assert_words(_recomputed(r, P)[1], first)
    # (a) a zero-area triangle inside live groups: grid triangle 0 collapses onto its first corner, in place
    Pa = P.copy()
    Pa[1], Pa[2] = Pa[0], Pa[0]
    wa, kept = NR.recompute(Pa, G, first)
    assert (NR.face_normals(Pa)[0] == 0).all() and not kept.any() and not np.array_equal(wa, first)
    _assert_words(_recomputed(r, Pa)[1], wa, "(a)")
    # (b) a group of only zero-area triangles: the 8 members of label 2000 (and the other corners of their triangles) collapse
    Pb = P.copy()
    tris = np.unique(np.nonzero(G == 2000)[0] // 3)
    for t in tris:
        Pb[3 * t + 1], Pb[3 * t + 2] = Pb[3 * t], Pb[3 * t]
    wb, kept = NR.recompute(Pb, G, wa)
    assert kept[G == 2000].all() and kept.sum() >= 8 and not kept.all()
    got = _recomputed(r, Pb)[1]
    _assert_words(got, wb, "(b)")
    assert np.array_equal(got[kept], wa[kept]) and not np.array_equal(got[~kept], wa[~kept])
    # (c) one NaN coordinate in fan triangle 2 (unrolled vertex 127): exactly the groups that touch that triangle keep their words
    Pc = (P * f32(0.5)).astype(f32)
    Pc[127, 1] = np.nan
    wc, kept = NR.recompute(Pc, G, wb)
    dense = NR.dense_groups(G)
    touched = np.isin(dense, dense[126:129])
    assert np.array_equal(kept, touched) and 9 + 2 + 2 == kept.sum()            # the hub's nine corners and two rim pairs
    got = _recomputed(r, Pc, refit=False)[1]
    _assert_words(got, wc, "(c)")
    assert np.array_equal(got[kept], wb[kept]) and (got[~kept] != wb[~kept]).any()
    _recomputed(r, P)                                                            # finite again before anything else happens
    r.close()


# ------------------------------------------------------------------ 3. through the renderer
def _wave(P):
    """a deformation that is a function of the rest position: welded corners stay together"""
    D = np.asarray(P, np.float64).copy()
    D[:, 1] += 2.5 * np.sin(0.35 * D[:, 0] + 1.0) + 1.5 * np.cos(0.5 * D[:, 2])
    return D.astype(f32)


def _deformed_scene(scene, D0, words=None, grid=None):
    """the scene whose geometry 0 holds the positions D0 quantised on `grid` = (base, extent) (default: D0's own bounds) and, if given,
    these normal words -> (scene, the float positions set_scene makes of them, grid)"""
    if grid is None:
        lo, hi = D0.min(axis=0).astype(f32), D0.max(axis=0).astype(f32)
        extent = (hi - lo).astype(f32)
        grid = (lo, np.where(extent > 0, extent, f32(1e-3)).astype(f32))
    lo, extent = grid
    g = dataclasses.replace(scene.geometries[0], qpos=scenes.quantize_positions(D0, extent, lo), scaling=scenes.dequantization_scaling(extent),
                            offset=scenes.dequantization_offset(lo, extent))
    s = copy.copy(scene)
    s.geometries = [g] + list(scene.geometries[1:])
    if words is not None:
        s = TS._with_normal_words(s, words)
    return s, scenes.dequantize_positions(g.qpos, g.scaling, g.offset), grid


@pytest.fixture(scope="module")
def waved():
    scene = TS._scene()
    P, rest_words = TS._rest(scene, 0)
    groups = scenes.normal_groups(P, rest_words)
    assert groups.max() + 1 == 8 * 6
    _, D, grid = _deformed_scene(scene, _wave(P))                    # the wave, on the quantisation grid of the scene that will hold it
    words, kept = NR.recompute(D, groups, rest_words)
    assert not kept.any() and (words != rest_words).mean() > 0.9
    fresh, D2, _ = _deformed_scene(scene, D, words, grid)
    assert np.array_equal(float_bits(D2), float_bits(D))              # (a grid point is the centre of its cell: quantising it gives it back)
    pose = types.SimpleNamespace(pos=[D, TS._rest(scene, 1)[0]])
    return scene, groups, D, words, fresh, TS._looking_at(scene, pose)


def _frame(r, scene, cam, fif):
    cfg = config(scene, abi.VARIANT_GLTF, reset=True, camera=cam)
    if fif > 1:
        r.wait(r.render_async(cfg, spp=1))
    else:
        r.render(cfg, spp=1)
    return read_frame(r, W, H)


@pytest.mark.parametrize("rebuild,fif", [(False, 1), (True, 1), (False, 2)])
def test_update_recompute_refit_equals_a_fresh_scene_of_the_deformed_mesh(waved, rebuild, fif):
    """A: the rest scene, update_vertices + recompute_normals + refit. B: a fresh set_scene of the deformed mesh whose uploaded normal
    words are the reference's. C: as A without recompute_normals. Normal + depth AOV and frame: A == B bit for bit, C != B."""
    scene, groups, D, words, fresh, cam = waved
    a = renderer(scene, W, H, frames_in_flight=fif)
    b = renderer(fresh, W, H, frames_in_flight=fif)
    c = renderer(scene, W, H, frames_in_flight=fif)
    if rebuild:
        for r in (a, b, c):
            r.set_bvh_policy(force_bvh_rebuild=True)
    a.set_normal_groups(0, groups)
    # two frames in flight: an earlier frame (A, C: of the rest pose) is still in flight while the update is staged, and every handle
    # has rendered the same number of frames when the compared one starts (a frame's samples depend on how many came before it)
    pending = [r.render_async(config(s, abi.VARIANT_GLTF, reset=True, camera=cam), spp=1) for r, s in ((a, scene), (b, fresh), (c, scene))] if fif > 1 else []
    a.update_vertices(0, D)
    a.recompute_normals()
    a.refit()
    c.update_vertices(0, D)
    c.refit()
    for r, ticket in zip((a, b, c), pending):
        r.wait(ticket)
    fa, fb, fc = (_frame(r, s, cam, fif) for r, s in ((a, scene), (b, fresh), (c, scene)))
    _assert_words(a.readback_skinned(0)[1], words)
    print("rebuild %d, frames in flight %d: normal + depth differs from the un-recomputed run in %d of %d values" %
          (rebuild, fif, int((fb[3].view(np.uint16) != fc[3].view(np.uint16)).sum()), fb[3].size))
    assert np.array_equal(fa[3].view(np.uint16), fb[3].view(np.uint16)), "normal + depth AOV"
    assert same_images(fa, fb)
    assert not np.array_equal(fc[3].view(np.uint16), fb[3].view(np.uint16))      # the scene is sensitive: without the call the normals are the rest pose's
    assert not np.array_equal(fc[0].view(np.uint32), fb[0].view(np.uint32))
    if rebuild:
        assert a.bvh_rebuild_count() >= 1
    for r in (a, b, c):
        r.close()


# ------------------------------------------------------------------ 4. composition with the deformers
def test_recomputed_words_replace_the_skinners(waved):
    scene, groups = waved[0], waved[1]
    P, rest_words = TS._rest(scene, 0)
    n = len(P)
    bones, weights = np.zeros((n, 4), np.uint16), np.zeros((n, 4), np.uint16)
    weights[:, 0] = 65535
    ang = 0.7
    M = np.array([[[np.cos(ang), -np.sin(ang), 0, 0.5], [np.sin(ang), np.cos(ang), 0, -1.0], [0, 0, 1, 2.0]]], f32)
    r = renderer(scene, W, H)
    r.set_skin(0, bones, weights)
    r.set_normal_groups(0, groups)
    r.update_bones(0, M)
    r.skin()
    pos, skinned_words, rejected = S.skin(P, rest_words, bones, weights, M)
    xyz, got = r.readback_skinned(0)
    assert not rejected.any() and np.array_equal(float_bits(xyz), float_bits(pos))
    _assert_words(got, skinned_words, "skinned")
    r.recompute_normals()
    r.refit()
    xyz, got = r.readback_skinned(0)
    want, kept = NR.recompute(xyz, groups, skinned_words)
    assert not kept.any() and not np.array_equal(want, skinned_words)
    _assert_words(got, want, "recomputed")
    r.close()


def test_a_morph_target_without_normal_deltas_gets_normals_and_unbinding_keeps_them(waved):
    scene, groups = waved[0], waved[1]
    P, rest_words = TS._rest(scene, 0)
    n = len(P)
    dpos = (_wave(P) - P).astype(f32)
    r = renderer(scene, W, H)
    r.set_morph_targets(0, [(np.arange(n, dtype=np.uint32), dpos, None)])
    r.set_normal_groups(0, groups)
    r.update_morph_weights(0, 0, np.ones(1, f32))
    r.skin()
    xyz, morphed_words = r.readback_skinned(0)
    assert np.array_equal(float_bits(xyz), float_bits(P + dpos))
    r.recompute_normals()
    r.refit()
    xyz, got = r.readback_skinned(0)
    want, kept = NR.recompute(xyz, groups, morphed_words)
    assert not kept.any() and (want != morphed_words).mean() > 0.9        # zero dnrm left the rest normals: the hole this closes
    _assert_words(got, want, "recomputed")
    # unbinding keeps the last words (the morph binding still lets them be read), and nothing is left to recompute
    r.set_normal_groups(0, None)
    _assert_words(r.readback_skinned(0)[1], want, "after unbinding")
    with pytest.raises(backend.BackendError) as e:
        r.recompute_normals()
    assert e.value.code == abi.RPTR_E_INVALID and "no geometry is bound" in str(e.value)
    r.close()


# ------------------------------------------------------------------ 5. the error convention
def test_refusals(mixed):
    scene, P, G, prev = mixed
    L = backend.load_library()
    vp = C.c_void_p
    assert L.rptr_hip_set_normal_groups(None, 0, G.ctypes.data_as(vp), len(G), 0) == abi.RPTR_E_INVALID
    assert L.rptr_hip_recompute_normals(None) == abi.RPTR_E_INVALID
    r = backend.RenderHip()
    r.initialize(W, H)

    def refused(call, *text):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == abi.RPTR_E_INVALID, str(e.value)
        for t in text:
            assert t in str(e.value), str(e.value)

    refused(lambda: r.set_normal_groups(0, G), "before set_scene")
    refused(r.recompute_normals, "before set_scene")
    static = scenes.grid(7, 5)
    r.set_scene(static)
    refused(lambda: r.set_normal_groups(0, np.zeros(210, np.uint32)), "geometry 0", "dynamic")
    two = TS._scene()                                                # geometry 1: a dynamic mesh without normals
    r.set_scene(two)
    refused(lambda: r.set_normal_groups(1, np.zeros(36, np.uint32)), "geometry 1", "no normals")
    refused(lambda: r.set_normal_groups(2, np.zeros(36, np.uint32)), "geometry 2", "dynamic")      # no such geometry
    r.set_scene(scene)
    refused(r.recompute_normals, "no geometry is bound")
    refused(lambda: r.readback_skinned(0), "no normal groups")
    refused(lambda: r.set_normal_groups(0, G[:-1]), "261", "260")
    refused(lambda: r._check(L.rptr_hip_set_normal_groups(r._h, 0, G.ctypes.data_as(vp), len(G), 6)), "flag bits", "0x6")
    assert L.rptr_hip_set_normal_groups(r._h, 0, None, 261, 0) == abi.RPTR_E_INVALID
    assert L.rptr_hip_set_normal_groups(r._h, 0, G.ctypes.data_as(vp), 0, 0) == abi.RPTR_E_INVALID
    refused(r.recompute_normals, "no geometry is bound")            # none of the refused calls bound anything
    # a binding, then every refusal again: the binding still works
    r.set_normal_groups(0, G)
    want, _ = NR.recompute(P, G, prev)
    _assert_words(_recomputed(r, P)[1], want)
    refused(lambda: r.set_normal_groups(0, G[:-1]), "261", "260")
    refused(lambda: r._check(L.rptr_hip_set_normal_groups(r._h, 0, G.ctypes.data_as(vp), len(G), 2)), "flag bits")
    refused(lambda: r.set_normal_groups(5, G), "dynamic")
    P2 = (P * f32(0.5) + P[:, [2, 0, 1]]).astype(f32)
    want2, kept = NR.recompute(P2, G, want)
    assert not kept.any() and not np.array_equal(want2, want)
    _assert_words(_recomputed(r, P2)[1], want2, "after the refused calls")
    refused(lambda: r.readback_skinned(0, num_vertices=260), "261")
    # unbinding; a new set_scene drops a binding
    r.set_normal_groups(0, None)
    refused(r.recompute_normals, "no geometry is bound")
    r.set_normal_groups(0, G)
    r.set_scene(scene)
    refused(r.recompute_normals, "no geometry is bound")
    r.close()


# ------------------------------------------------------------------ 6. nothing bound, nothing new
def test_a_handle_that_never_recomputes_renders_what_it_did(waved):
    """the same positions through update_vertices + refit on a handle that binds normal groups and never recomputes, and on one that
    never heard of them: the same frame and AOV images, byte for byte"""
    scene, groups, D, words, fresh, cam = waved
    a, b = renderer(scene, W, H), renderer(scene, W, H)
    a.set_normal_groups(0, groups)
    for r in (a, b):
        r.update_vertices(0, D)
        r.refit()
    fa, fb = _frame(a, scene, cam, 1), _frame(b, scene, cam, 1)
    assert same_images(fa, fb)
    _assert_words(a.readback_skinned(0)[1], TS._rest(scene, 0)[1], "uploaded")
    a.close()
    b.close()
