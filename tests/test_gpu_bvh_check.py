"""Every tree the device builds, rebuilds or refits, exported and put through the exact checker of tests/bvh_check.py: containment with
zero tolerance against the vertices, the encoder's origin / exponent restated on the exact bounds (a stale box fails even when it is
larger), tightness, every triangle and record exactly once, instance boxes restated in float32 and bounded in float64, the stack.

What other tests already compare (a fresh set_scene, the oracle, brute force) is not repeated here; the renderers are 64 x 48 and render
no frame except in the scene-copy test.

Loops and adversarial vertices. The vertex sets of `_adversarial` reach the device builders only through update_vertices + refit, i.e.
the refit kernels and -- under force_bvh_rebuild -- the LBVH path (csrc/lbvh.h driven by host_scene.inl lbvh_front_half / lbvh_rebuild).
That path has no host loop at all beside the fixed RP_REFIT_LEVELS launches; its device loops run over integer keys (the Karras searches
double / halve a range inside [0, n), the depth walk follows parent links of a tree of at most 64 levels) and the radix sort makes a fixed
number of passes over 64-bit keys: every iteration count is bounded by the input size or the key width, none by a floating-point
comparison (NaN or huge coordinates only change which cell a key names). The one host loop that waits on device results is PLOC's
clustering loop (host_bvh.inl device_build_tree): it ends when the cluster count stops falling and reports an error instead of going
on, and it only ever sees the quantised vertices of set_scene, never these sets.

Stack. For a tree whose topology the host made (refits, moved instances) the bound is what rptr_hip_build_bvh_host reports for the scene,
as in test_gpu_instances.py::test_stack_bound_of_set_scene_covers_the_rebuilt_top_level. For a bottom-level tree made on the device (PLOC
at set_scene, LBVH at a rebuild) the library reports no bound of its own: set_scene holds the tree it got against the traversal stack's
capacity, RP_LDS_STACK + RPTR_BVH_STACK_DEPTH entries, and that capacity is the bound here."""
import numpy as np
import pytest

import bvh_check as B
from common import movable_two_level, random_transforms, renderer
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48
STACK_CAPACITY = 20 + 128   # csrc/dtraverse.h RP_LDS_STACK + include/rptr_bvh.h RPTR_BVH_STACK_DEPTH


def _check(r, scene, what, **kw):
    rep = B.check_bvh(*r.export_bvh(), scene, **kw)
    print("%s: %d nodes reached (%d not), levels %s / top %d, worst slack %.6f steps, instance overhang %.3f of its bound, stack %d of %s" % (
        what, rep["nodes_reached"], rep["unreached_nodes"], rep["levels"], rep["tlas_levels"], rep["worst_slack_steps"], rep["worst_instance_overhang"],
        rep["stack_entries"], rep["stack_bound"]))
    return rep


def _forest(tris_per_tree=300):
    return scenes.forest(n_meshes=3, tris_per_tree=tris_per_tree, n_instances=25, name="f")


# ------------------------------------------------------------------ the device PLOC build (csrc/ploc.h)
PLOC_SCENES = {
    "grid96x48-two_level": (lambda: scenes.grid(96, 48, with_emitters=True), "0"),
    "forest600-two_level": (lambda: _forest(600), "0"),
    "forest600-flat": (lambda: _forest(600), "1"),
    "soup5-two_level": (lambda: scenes.soup(5), "0"),
    "soup5-flat": (lambda: scenes.soup(5), "1"),
    "soup6-two_level": (lambda: scenes.soup(6), "0"),
    "soup6-flat": (lambda: scenes.soup(6), "1"),
}


@pytest.mark.parametrize("top", ["64", "16"])
@pytest.mark.parametrize("name", list(PLOC_SCENES))
def test_device_ploc_build_passes_the_exact_checker(name, top, monkeypatch):
    scene_fn, flatten = PLOC_SCENES[name]
    s = scene_fn()
    monkeypatch.setenv("RPTR_FLATTEN", flatten)
    monkeypatch.setenv("RPTR_BVH_BUILDER", "device")
    monkeypatch.setenv("RPTR_PLOC_TOP", top)
    r = renderer(s, W, H)
    assert r.bvh_build_info()[0]          # built on the device: no silent fall-back to the host builder passes as the device build
    _check(r, s, "PLOC %s top %s" % (name, top), stack_bound=STACK_CAPACITY)
    r.close()


# ------------------------------------------------------------------ refit and device rebuild of a deformed mesh
# refit_mesh_levels (csrc/host_scene.inl) refits the depths 0 .. 5 of a dynamic mesh's tree in the one block of rp_k_refit_top and every
# deeper level with a launch of rp_k_refit_level: a tree of 6 levels takes the one-block kernel alone, one of 7 takes both. The host
# builds grid(48, 24) with 6 levels and grid(50, 25) -- the smallest 2 : 1 grid for which it does -- with 7, as grid(96, 48).
GRIDS = [(48, 24, 6), (50, 25, 7), (96, 48, 7)]


def _dyn_grid(nx, nz):
    return scenes.grid(nx, nz, deform_t=0.0, name="dyn-grid")


def _deformations(nx, nz):
    """t = 0.3, 0.65, back to 0.0, then the whole mesh shrunk to half its size: boxes must shrink with it"""
    for t in (0.3, 0.65, 0.0):
        yield "t=%.2f" % t, scenes.grid_positions(nx, nz, t)
    yield "shrunk", (scenes.grid_positions(nx, nz, 0.0) * np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("nx,nz,levels", GRIDS)
def test_refit_of_a_deformed_grid(nx, nz, levels):
    """levels 6: rp_k_refit_top alone; levels 7: rp_k_refit_level for the deepest level, then rp_k_refit_top"""
    s = _dyn_grid(nx, nz)
    need = backend.build_bvh_host(s)[3]
    r = renderer(s, W, H)
    rep = _check(r, s, "grid %dx%d as built" % (nx, nz), stack_bound=need)
    assert list(rep["levels"].values()) == [levels]
    for what, P in _deformations(nx, nz):
        r.update_vertices(0, P)
        r.refit()
        _check(r, s, "grid %dx%d refit %s" % (nx, nz, what), positions={0: P}, stack_bound=need)
    assert r.bvh_rebuild_count() == 0
    r.close()


def _adversarial(P):
    """vertex sets a correct builder handles (every magnitude within 2^-40 .. 2^40, so every product of two extents is a normal, finite
    float), at the edges of the encoder: P is (3 n, 3) float32"""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P) // 3
    out = {}
    out["translated"] = (P + np.array([1e6, -3e5, 7e6], np.float32)).astype(np.float32)
    flat = P.copy()
    flat[:, 1] = np.float32(0.375)
    out["flat"] = flat
    out["point"] = np.broadcast_to(P[7], P.shape).astype(np.float32).copy()
    unit = (P / np.abs(P).max()).astype(np.float32)                                  # coordinates in [-1, 1]
    k = np.round(np.linspace(-24, 40, n)).astype(np.int32)                              # per triangle: 2^-24 .. 2^40 (its extents: from about 2^-40)
    out["binades"] = np.ldexp(unit.reshape(n, 3, 3), k[:, None, None]).astype(np.float32).reshape(-1, 3)
    zero = (P - P.mean(axis=0).astype(np.float32)).astype(np.float32)                   # straddles the origin
    zero[np.abs(zero) < np.float32(0.05) * np.abs(zero).max(axis=0)] = np.float32(-0.0)
    zero[::5, 1] = np.float32(-0.0)
    out["negative_zero"] = zero
    for v in out.values():
        t = v.reshape(n, 3, 3)
        ext = (t.max(axis=1) - t.min(axis=1)).astype(np.float64)
        assert v.dtype == np.float32 and np.isfinite(v).all() and np.abs(v).max() <= 2.0 ** 40 and (ext[ext > 0] >= 2.0 ** -60).all()
    assert np.signbit(out["negative_zero"]).any() and (out["negative_zero"] > 0).any() and (out["negative_zero"] < 0).any()
    return out


ADVERSARIAL = ["translated", "flat", "point", "binades", "negative_zero"]


def _dyn_soup():
    s = scenes.soup(3)
    s.meshes[0].dynamic = True
    return s


def _adversarial_case(mesh, case, rebuild):
    s = _dyn_grid(50, 25) if mesh == "grid" else _dyn_soup()
    g = s.geometries[0]
    P = _adversarial(scenes.dequantize_positions(g.qpos, g.scaling, g.offset))[case]
    r = renderer(s, W, H)
    if rebuild:
        r.set_bvh_policy(force_bvh_rebuild=True)
    r.update_vertices(0, P)
    r.refit()
    assert r.bvh_rebuild_count() == (1 if rebuild else 0)
    rep = _check(r, s, "%s %s %s" % (mesh, case, "rebuild" if rebuild else "refit"), positions={0: P}, rebuilt=rebuild,
                 stack_bound=STACK_CAPACITY if rebuild else backend.build_bvh_host(s)[3])
    r.close()
    return rep


@pytest.mark.parametrize("case", ADVERSARIAL)
@pytest.mark.parametrize("mesh", ["grid", "soup"])
def test_refit_on_adversarial_vertices(mesh, case):
    """grid(50, 25): both refit kernels (see GRIDS); soup(3) with its first mesh dynamic and instanced three times: the one-block kernel"""
    _adversarial_case(mesh, case, rebuild=False)


@pytest.mark.parametrize("case", ADVERSARIAL)
@pytest.mark.parametrize("mesh", ["grid", "soup"])
def test_device_rebuild_on_adversarial_vertices(mesh, case):
    """the same sets through rptr_hip_set_bvh_policy(force_bvh_rebuild = 1): the LBVH build of csrc/lbvh.h, boxes from the refit that ends it"""
    _adversarial_case(mesh, case, rebuild=True)


@pytest.mark.parametrize("nx,nz", [(50, 25), (96, 48)])
def test_device_rebuild_of_a_deformed_grid_and_rebuilds_alternating_with_refits(nx, nz):
    s = _dyn_grid(nx, nz)
    r = renderer(s, W, H)
    r.set_bvh_policy(force_bvh_rebuild=True)
    for what, P in _deformations(nx, nz):
        r.update_vertices(0, P)
        r.refit()
        _check(r, s, "grid %dx%d rebuild %s" % (nx, nz, what), positions={0: P}, rebuilt=True, stack_bound=STACK_CAPACITY)
    assert r.bvh_rebuild_count() == 4
    # a refit on the topology the last rebuild made (its level lists live on the device), a rebuild, a refit again
    for k, (force, t) in enumerate([(False, 0.4), (True, 0.8), (False, 0.1)]):
        r.set_bvh_policy(force_bvh_rebuild=force)
        P = scenes.grid_positions(nx, nz, t)
        r.update_vertices(0, P)
        r.refit()
        _check(r, s, "grid %dx%d %s t=%.1f" % (nx, nz, "rebuild" if force else "refit after a rebuild", t), positions={0: P}, rebuilt=True,
               stack_bound=STACK_CAPACITY)
    assert r.bvh_rebuild_count() == 5
    r.close()


# ------------------------------------------------------------------ moving instances (csrc/tlas_build.h)
def _moves(xf0, rng):
    """(name, transforms) over the instances whose set_scene transforms are xf0 (n, 3, 4)"""
    n = len(xf0)
    perm = xf0.copy()
    perm[:, :, 3] = xf0[rng.permutation(n), :, 3]
    yield "positions permuted", perm
    shear = xf0.copy()
    S = np.array([[1.7, 0.4, 0.0], [0.0, 0.6, -0.3], [0.2, 0.0, 1.1]], np.float32)
    shear[:, :, :3] = np.einsum("ij,njk->nik", S, xf0[:, :, :3]).astype(np.float32)
    yield "non-uniform scale with shear", shear
    mirror = xf0.copy()
    mirror[:, :, 0] = -mirror[:, :, 0]
    yield "mirrored", mirror
    for sc in (1e-3, 1e3):
        scaled = xf0.copy()
        scaled[:, :, :3] *= np.float32(sc)
        yield "scaled by %g" % sc, scaled
    far = xf0.copy()
    far[:, :, 3] += np.array([1e6, 0.0, -1e6], np.float32)
    yield "translated to 1e6", far
    same = xf0.copy()
    same[:] = xf0[0]
    yield "all coincident", same


@pytest.mark.parametrize("policy", [abi.TLAS_REBUILD, abi.TLAS_REFIT])
@pytest.mark.parametrize("layout", ["two_level", "partially_flattened"])
def test_moved_instances_of_the_forest(layout, policy, monkeypatch):
    """two_level: every mesh's instances may move, 101 re-braided records over 13 sub-roots. partially_flattened: the instances of mesh 1
    move and keep their records, everything else is one world-space tree behind an identity record."""
    s = _forest()
    if layout == "two_level":
        for m in s.meshes:
            m.dynamic = abi.MESH_INSTANCES_MOVE
        movers = list(range(len(s.instances)))
    else:
        monkeypatch.setenv("RPTR_FLATTEN", "-1")
        s.meshes[1].dynamic = abi.MESH_INSTANCES_MOVE
        movers = [i for i, inst in enumerate(s.instances) if s.pmeshes[inst.pmesh].mesh == 1]
    need = backend.build_bvh_host(s)[3]
    r = renderer(s, W, H)
    r.set_tlas_policy(policy)
    rep = _check(r, s, "%s as built" % layout, stack_bound=need)
    assert rep["top_records"] == (101 if layout == "two_level" else 1 + len(movers))
    xf0 = np.stack([np.asarray(s.instances[i].transform, np.float32) for i in movers])
    rebuilds = 0
    for what, xf in _moves(xf0, np.random.default_rng(3)):
        for k, i in enumerate(movers):       # (the movers of the partially flattened forest are not consecutive)
            r.update_instances(i, xf[k:k + 1])
        r.refit()
        rebuilds += 1 if policy == abi.TLAS_REBUILD else 0
        assert r.tlas_rebuild_count() == rebuilds
        _check(r, s, "%s policy %d %s" % (layout, policy, what), transforms={i: xf[k] for k, i in enumerate(movers)}, stack_bound=need)
    r.close()


@pytest.mark.parametrize("policy", [abi.TLAS_REBUILD, abi.TLAS_REFIT])
def test_moved_instance_of_a_single_instance_scene(policy):
    s = scenes.grid(16, 8)
    s.meshes[0].dynamic = abi.MESH_INSTANCES_MOVE
    need = backend.build_bvh_host(s)[3]
    r = renderer(s, W, H)
    r.set_tlas_policy(policy)
    M = np.array([[0.0, -1.5, 0.2, 3.0], [0.8, 0.0, 0.0, -2.0], [0.0, 0.1, 1.1, 7.0]], np.float32)
    r.update_instances(0, M[None])
    r.refit()
    rep = _check(r, s, "single instance policy %d" % policy, transforms={0: M}, stack_bound=need)
    assert rep["top_records"] == 1 and rep["tlas_nodes"] == 1
    r.close()


def test_instances_moved_from_a_device_buffer():
    import torch
    s = _forest()
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    need = backend.build_bvh_host(s)[3]
    r = renderer(s, W, H)
    xf0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances])
    what, xf = list(_moves(xf0, np.random.default_rng(5)))[1]
    buf = torch.from_numpy(np.ascontiguousarray(xf.reshape(-1, 12))).cuda()
    torch.cuda.synchronize()
    r.update_instances_device(0, buf.data_ptr(), len(xf))
    r.refit()
    assert r.get_option("instance_updates_rejected") == 0 and r.tlas_rebuild_count() == 1
    _check(r, s, "device source, %s" % what, transforms=xf, stack_bound=need)
    r.close()


@pytest.mark.parametrize("rebuild", [False, True])
def test_a_deformed_mesh_and_moved_instances_in_one_refit(rebuild):
    s = _forest()
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    s.meshes[0].dynamic = abi.MESH_DYNAMIC | abi.MESH_INSTANCES_MOVE
    need = backend.build_bvh_host(s)[3]
    r = renderer(s, W, H)
    r.set_bvh_policy(force_bvh_rebuild=rebuild)
    g = s.geometries[s.meshes[0].first_geometry]
    P = (scenes.dequantize_positions(g.qpos, g.scaling, g.offset) * np.float32(1.2) + np.array([0.1, 0.2, -0.1], np.float32)).astype(np.float32)
    xf0 = np.stack([np.asarray(i.transform, np.float32) for i in s.instances])
    what, xf = list(_moves(xf0, np.random.default_rng(9)))[0]
    r.update_vertices(s.meshes[0].first_geometry, P)
    r.update_instances(0, xf)
    r.refit()
    assert r.bvh_rebuild_count() == (1 if rebuild else 0) and r.tlas_rebuild_count() == 1
    _check(r, s, "deformed and moved (%s)" % ("rebuild" if rebuild else "refit"), positions={s.meshes[0].first_geometry: P}, transforms=xf, rebuilt=rebuild,
           stack_bound=STACK_CAPACITY if rebuild else need)
    r.close()


# ------------------------------------------------------------------ scene copies
def test_scene_copies_after_a_refit_render_the_checked_tree():
    """frames_in_flight = 3 on the scene of test_gpu_scene_copies.py (a deforming, moving mesh: every frame context keeps its own triangles,
    records and top level). rptr_hip_export_bvh reads the master copy; the contexts' copies cannot be exported one by one. So: the export
    after update + refit passes the checker, and one frozen frame on each of the three contexts -- each brought up to date on its own
    copy when its frame is submitted -- gives the bits of the frame a one-context handle renders from the master copy that was checked
    (whose export is the same tree, bit for bit)."""
    s = movable_two_level()
    s.meshes[0].dynamic = abi.MESH_DYNAMIC | abi.MESH_INSTANCES_MOVE
    g = s.geometries[0]
    P = (scenes.dequantize_positions(g.qpos, g.scaling, g.offset) * np.float32(1.2) + np.array([0.1, 0.2, -0.1], np.float32)).astype(np.float32)
    xf = random_transforms(len(s.instances), 70)
    cfg = backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_SIMPLE, reset_accumulation=True, freeze_frame=True)
    images, exports = [], []
    for fif in (3, 1):
        r = backend.RenderHip(frames_in_flight=fif)
        r.initialize(W, H)
        r.set_scene(s)
        r.update_vertices(0, P)
        r.update_instances(0, xf)
        r.refit()
        exports.append([a.copy() for a in r.export_bvh()])
        _check(r, s, "scene copies, %d frame contexts" % fif, positions={0: P}, transforms=xf, stack_bound=backend.build_bvh_host(s)[3])
        for _ in range(fif):
            r.wait(r.render_async(cfg, spp=1))
            img = np.zeros((H, W, 4), np.float32)
            assert r.readback_framebuffer(img) == W * H * 4
            images.append(img)
        r.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*exports))
    assert all(np.array_equal(images[0].view(np.uint32), im.view(np.uint32)) for im in images[1:]) and images[0][..., :3].std() > 0.01
