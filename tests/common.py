"""Shared helpers of the tests: renderer handles, configurations, read-backs, cameras, transforms and query rays. The helpers that build
random data are pinned by the tests that use them: the same arguments must keep giving the same arrays."""
import copy
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from realtimepathtracingresearchframework_amd import abi, backend, scenes

RMSE_TOL = 1e-3  # north_star: validation image error < 1e-3 RMSE at fixed seed/spp


def renderer(scene, W, H, **kw):
    """an initialized RenderHip(**kw) of W x H with the scene set"""
    r = backend.RenderHip(**kw)
    r.initialize(W, H)
    r.set_scene(scene)
    return r


def one_grid_elements(per_cu=8):
    """how many elements one launch of a grid-stride kernel covers before any lane takes a second trip: csrc/host_state.h grid_for caps
    the grid at per_cu * num_cus blocks of 256, and num_cus is the device's multiProcessorCount (rptr_hip.hip). Tests that mean to
    cross the cap size their shapes from this value."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu * 256


def config(scene, variant=abi.VARIANT_GLTF, reset=True, camera=None, freeze_frame=False):
    return backend.RenderConfiguration(camera or scene.camera_params(), active_variant=variant, reset_accumulation=reset, freeze_frame=freeze_frame)


def float_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def read_frame(r, W, H, aovs=True):
    """(accum, fb, albedo + roughness, normal + depth, motion + jitter) of the frame the read-backs return; aovs=False: the first two"""
    acc = np.zeros((H, W, 4), np.float32)
    fb = np.zeros((H, W, 4), np.uint8)
    assert r.readback_framebuffer(acc) == W * H * 4 and r.readback_framebuffer(fb) == W * H * 4
    if not aovs:
        return acc, fb
    aov = [np.zeros((H, W, 4), np.float16) for _ in range(3)]
    for k in range(3):
        assert r.readback_aov(k, aov[k]) == W * H * 4
    return acc, fb, aov[0], aov[1], aov[2]


def same_images(a, b):
    """two tuples of images, byte for byte"""
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def raw_stats(r):
    st = abi.Stats()
    assert r._L.rptr_hip_stats(r._h, C.byref(st)) == 0
    return st


def aov_close(a, b, what):
    """float16 images with the same finite / non-finite pattern (more than 99.95 % of the values) and values within 2^-9 max(|ref|, 2^-5),
    two half ulps (more than 99.9 % of them): the floats behind them differ by libm ulps between host and device, an RGBA16F store
    rounds them"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    fa, fb = np.isfinite(a32), np.isfinite(b32)
    same_pattern = float((fa == fb).mean())
    both = fa & fb
    err = np.abs(a32[both] - b32[both])
    tol = 2.0 ** -9 * np.maximum(np.abs(b32[both]), 2.0 ** -5)
    inside = float((err <= tol).mean())
    print("%s: finite pattern equal %.6f, inside the bound %.6f, worst error %.3e" % (what, same_pattern, inside, float(err.max())))
    assert same_pattern > 0.9995, what
    assert inside > 0.999, (what, float(err.max()))


def panned_camera(cam, k, rate):
    """the view yawed by rate * k radians about its up axis"""
    d = np.array(cam.dir[:], np.float64)
    u = np.array(cam.up[:], np.float64)
    r = np.cross(d, u)
    r /= np.linalg.norm(r)
    a = rate * k
    nd = math.cos(a) * d + math.sin(a) * r
    nd /= np.linalg.norm(nd)
    c = abi.Camera()
    c.pos[:] = cam.pos[:]
    c.dir[:] = [float(v) for v in nd]
    c.up[:] = cam.up[:]
    c.fovy = cam.fovy
    return c


def fly_camera(cam, k):
    """frame k of --fly-through (host/rptr_cli.cpp fly_camera, bench.py's path): yawed by 0.002 rad x s about the up axis from 2 cm x s
    further to the right, s = k mod 64 - 32; evaluated in double, rounded to float once"""
    s = k % 64 - 32
    a = 0.002 * s
    d = [float(v) for v in cam.dir[:]]
    u = [float(v) for v in cam.up[:]]
    r = [d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]]
    rl = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    r = [x / rl for x in r]
    nd = [math.cos(a) * d[i] + math.sin(a) * r[i] for i in range(3)]
    nl = math.sqrt(nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2])
    c = abi.Camera()
    c.pos[:] = [float(np.float32(float(cam.pos[i]) + 0.02 * s * r[i])) for i in range(3)]
    c.dir[:] = [float(np.float32(nd[i] / nl)) for i in range(3)]
    c.up[:] = cam.up[:]
    c.fovy = cam.fovy
    return c


def random_transforms(n, seed, spread=4.0):
    """rotation x NON-uniform scale + translation, float32 (n, 3, 4)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        ang = rng.uniform(0, 2 * np.pi)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        out[i, :, :3] = R @ np.diag(rng.uniform(0.5, 1.7, size=3))
        out[i, :, 3] = rng.uniform(-spread, spread, size=3)
    return out


def scene_transforms(s):
    return np.stack([np.asarray(i.transform, np.float32).reshape(3, 4) for i in s.instances])


def with_transforms(scene, xf, first=0):
    """a copy of the scene whose instances first, first + 1, ... have the transforms xf"""
    s = copy.copy(scene)
    s.instances = [copy.copy(i) for i in scene.instances]
    for k, m in enumerate(xf):
        s.instances[first + k].transform = np.asarray(m, np.float32).reshape(3, 4).copy()
    return s


def movable_two_level(n_inst=12, move_bit=True):
    """two_level_test without its emissive material (instances of an emissive mesh cannot move), every mesh MESH_INSTANCES_MOVE"""
    s = scenes.two_level_test(n_inst=n_inst)
    s.materials[3] = abi.make_material((1, 1, 1), roughness=0.4)
    s.prepare_lights()
    if move_bit:
        for m in s.meshes:
            m.dynamic = abi.MESH_INSTANCES_MOVE
    return s


def probe_queries(n, seed=3, spread=0.8, centre=(0.0, 1.0, 0.0), short=False):
    """random rays from inside the scene; short: every second one ends after 0.2 ... 3 units"""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 8), np.float32)
    q[:, 0:3] = rng.uniform(-spread, spread, (n, 3)).astype(np.float32) + np.float32(centre)
    d = rng.normal(size=(n, 3))
    q[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    q[:, 7] = 1e20
    if short:
        q[1::2, 7] = rng.uniform(0.2, 3.0, len(q[1::2])).astype(np.float32)
    return q


def synthetic_frame(H=32, W=48, amplitude=0.35):
    """albedo checker x smooth irradiance + deterministic hash noise on the irradiance -> (noisy accum, albedo, nd, clean rgb)"""
    ys, xs = np.mgrid[0:H, 0:W]
    checker = ((xs // 6 + ys // 6) & 1).astype(np.float32)
    albedo = np.stack([np.float32(0.2) + np.float32(0.6) * checker, np.float32(0.7) - np.float32(0.4) * checker, np.full((H, W), np.float32(0.5))], -1).astype(np.float16)
    irr = (np.float32(0.6) + np.float32(0.3) * np.sin(xs / np.float32(9.0)) * np.cos(ys / np.float32(7.0))).astype(np.float32)
    clean = albedo.astype(np.float32) * irr[..., None]
    hsh = (xs.astype(np.uint64) * 73856093) ^ (ys.astype(np.uint64) * 19349663)
    noise = np.empty((H, W, 3), np.float32)
    for ch in range(3):
        v = (hsh + np.uint64(ch * 83492791)) * np.uint64(2654435761) % np.uint64(1 << 32)
        v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
        noise[..., ch] = (v % np.uint64(65536)).astype(np.float32) / np.float32(65536) - np.float32(0.5)
    accum = np.empty((H, W, 4), np.float32)
    accum[..., :3] = albedo.astype(np.float32) * (irr[..., None] + np.float32(amplitude) * noise)
    accum[..., 3] = 1.0
    alb = np.concatenate([albedo, np.ones((H, W, 1), np.float16)], -1)
    nd = np.empty((H, W, 4), np.float16)
    nd[..., :3] = (0.0, 0.0, 1.0)
    nd[..., 3] = (np.float32(5.0) + xs * np.float32(0.02)).astype(np.float16)
    return accum, alb, nd, clean


def rel_excess(got, lo, hi):
    """how far a binary32 result lies outside the float64 band [lo, hi], relative to the band's larger end (0 inside)"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.maximum(lo - got, got - hi)
        return np.where(d > 0, d / np.maximum(np.maximum(np.abs(lo), np.abs(hi)), 1e-30), 0.0)


def gpu_render(scene, W, H, spp, variant, rank=0, world=1, stripe_rows=32, count=False, params=None, lighting=None, reset=True,
               renderer=None, keep=False, options=None):
    r = renderer or backend.RenderHip(rank=rank, world_size=world, stripe_rows=stripe_rows, options=options)
    if renderer is None:
        r.initialize(W, H)
        r.set_scene(scene)
    if params is not None:
        r.params = params
    if lighting is not None:
        r.lighting_params = lighting
    cfg = backend.RenderConfiguration(scene.camera_params(), active_variant=variant, reset_accumulation=reset)
    st = r.render(cfg, spp=spp, count_traversal=count)
    img = np.zeros((H, W, 4), dtype=np.float32)
    assert r.readback_framebuffer(img) == W * H * 4
    if keep or renderer is not None:
        return img, st, r
    r.close()
    return img, st, None


def image_error(a, b):
    """RMSE over RGB of the pixels finite in both, plus NaN-mask agreement."""
    fa, fb = np.isfinite(a[..., :3]).all(axis=2), np.isfinite(b[..., :3]).all(axis=2)
    both = fa & fb
    d = (a[..., :3] - b[..., :3])[both]
    rmse = float(np.sqrt(np.mean(d.astype(np.float64) ** 2))) if d.size else 0.0
    return rmse, bool(np.array_equal(fa, fb)), float(np.abs(d).max()) if d.size else 0.0


def random_queries(rng, n, lo, hi, t_max=1e20):
    q = np.zeros((n, 8), np.float32)
    q[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q[:, 4:7] = d
    q[:, 7] = t_max
    return q


def assert_ray_visit_parity(r, osc, W, H, spp, variant, max_rays=1 << 21):
    """Every ray of an oracle render (closest-hit AND occlusion rays, with their real intervals) is replayed through the
    device traversal: results and per-ray node / triangle visit counts must equal the oracle walking the exported tree.
    (Counts of a whole GPU render can differ from the oracle's by a few visits: libm differences of an ulp in a sampled
    direction change that ray's walk. Ray by ray on identical inputs the walk is exact.)"""
    osc.import_bvh(*r.export_bvh())
    _, st, rays = osc.render_logged(W, H, spp, max_rays, variant=variant, bvh_mode=O.BVH_IMPORTED, count=True)
    assert len(rays) == st.rays_closest + st.rays_shadow
    total = np.zeros(2, np.uint64)
    for any_hit in (False, True):
        sel = rays[rays[:, 8] == (1.0 if any_hit else 0.0)]
        q = np.zeros((len(sel), 8), np.float32)
        q[:, 0:3], q[:, 4:7], q[:, 7] = sel[:, 0:3], sel[:, 4:7], sel[:, 7]
        res, vis = r.trace_counted(q, tmin=sel[:, 3], any_hit=any_hit)
        tuv, ids, rv = osc.trace_ex_counts(sel[:, 0:3], sel[:, 4:7], sel[:, 3], sel[:, 7], any_hit=any_hit)
        assert np.array_equal(vis, rv), "%d of %d %s rays walk differently" % ((vis != rv).any(axis=1).sum(), len(sel),
                                                                             "occlusion" if any_hit else "closest-hit")
        if any_hit:
            assert np.array_equal(res[:, 0] != 0, ids[:, 0] != 0)
        else:
            hit = ids[:, 0] >= 0
            assert np.array_equal(res[:, 0] >= 0, hit)
            assert np.array_equal(res[hit, 0:2].view(np.uint32), tuv[hit, 1:3].view(np.uint32))
            assert np.array_equal(res[hit, 3].view(np.int32), ids[hit, 2])
        total += vis.sum(axis=0, dtype=np.uint64)
    assert int(total[0]) == st.nodes_closest + st.nodes_shadow and int(total[1]) == st.tris_closest + st.tris_shadow
    return st
