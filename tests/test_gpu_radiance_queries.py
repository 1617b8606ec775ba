"""Ray queries that return path-traced radiance (rptr_hip_trace_radiance*, RenderHip.render_radiance_queries): the path pipeline on the
rays of a query buffer. Against the oracle the queries ARE the camera rays of a frame (the oracle has no query entry); everything else
holds bit for bit by construction."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from common import RMSE_TOL, float_bits, image_error, probe_queries, renderer
from realtimepathtracingresearchframework_amd import abi, backend, pointsets, scenes

pytestmark = pytest.mark.gpu


def _primary_rays(osc, s, W, H, sample, **kw):
    """the camera rays of sample `sample` as the oracle itself makes them: a single-threaded render walks the pixels row by row and logs
    every ray; the primaries are the closest-hit records that start at the camera with t_min == 0, in pixel order"""
    ref, ost, rays = osc.render_logged(W, H, 1, 1 << 22, sample_begin=sample, accum=np.zeros((H, W, 4), np.float32), **kw)
    cam = np.asarray(list(s.camera_params().pos), np.float32)
    prim = rays[(rays[:, 8] == 0.0) & (rays[:, 3] == 0.0) & (rays[:, 0:3] == cam).all(axis=1)]
    assert len(prim) == W * H, "the ray log holds %d primaries for %d pixels" % (len(prim), W * H)
    q = np.zeros((W * H, 8), np.float32)
    q[:, 0:3], q[:, 4:7], q[:, 7] = prim[:, 0:3], prim[:, 4:7], np.float32(2e32)
    return q, ref, ost


def _check_against_frame(r, osc, s, W, H, variant, sample, **kw):
    q, ref, ost = _primary_rays(osc, s, W, H, sample, variant=variant, **kw)
    res = r.render_radiance_queries(q, s.camera_params(), variant=variant, spp=1, first_sample=sample, results=np.zeros((W * H, 4), np.float32))
    img = res.reshape(H, W, 4)
    rmse, same, worst = image_error(img, ref)
    st = r.radiance_query_stats().raw
    print("sample %d: rmse %.3e worst %.3e rays %d/%d shadow %d/%d" % (sample, rmse, worst, st.rays_closest, ost.rays_closest, st.rays_shadow, ost.rays_shadow))
    assert same and rmse < RMSE_TOL
    assert np.array_equal(img[..., 3], ref[..., 3])
    assert abs(int(st.rays_closest) - int(ost.rays_closest)) <= max(4, 1e-3 * ost.rays_closest)
    assert abs(int(st.rays_shadow) - int(ost.rays_shadow)) <= max(4, 1e-3 * ost.rays_shadow)


CASES = [("cornell32", abi.VARIANT_GLTF, 96, 72), ("two_level_test", abi.VARIANT_GLTF, 96, 72), ("grid_emitters", abi.VARIANT_SIMPLE, 100, 60),
         ("textured_test", abi.VARIANT_GLTF, 160, 120), ("alpha_test", abi.VARIANT_GLTF, 160, 120)]


def _scene(name):
    return scenes.grid(120, 60, with_emitters=True) if name == "grid_emitters" else getattr(scenes, name)()


@pytest.mark.parametrize("name,variant,W,H", CASES)
def test_camera_ray_queries_give_the_oracle_frame(name, variant, W, H):
    """1 + 2: queries that are the camera rays of sample 0 (fresh handle) and of sample 3 (first_sample = 3, zeroed results) give the
    oracle's frame of that sample: image, NaN mask, alpha, ray counts"""
    s = _scene(name)
    r = renderer(s, W, H)
    osc = O.OracleScene(s)
    kw = {}
    if name == "alpha_test":  # (the alpha tests depend on the order candidates turn up in: the oracle walks the device's tree)
        osc.import_bvh(*r.export_bvh())
        kw["bvh_mode"] = O.BVH_IMPORTED
    _check_against_frame(r, osc, s, W, H, variant, 0, **kw)
    _check_against_frame(r, osc, s, W, H, variant, 3, **kw)
    r.close()


@pytest.mark.parametrize("rng_variant", [abi.RNG_VARIANT_BN, abi.RNG_VARIANT_SOBOL, abi.RNG_VARIANT_Z_SBL])
def test_camera_ray_queries_with_table_point_sets(rng_variant):
    """10: the same with every table point set (wider than one 256-pixel Sobol' tile, not a multiple of 8)"""
    s = scenes.cornell32()
    W, H = 300, 140
    table = pointsets.default_table(rng_variant, seed=5)
    r = renderer(s, W, H)
    r.set_rng_variant(rng_variant, table)
    osc = O.OracleScene(s)
    osc.set_rng_variant(rng_variant, table)
    _check_against_frame(r, osc, s, W, H, abi.VARIANT_GLTF, 0)
    _check_against_frame(r, osc, s, W, H, abi.VARIANT_GLTF, 3)
    r.close()


def test_samples_split_over_calls_and_query_prefixes_are_bit_identical():
    """3 + 4: one call of 4 samples == four calls of one sample on the same buffer; the first m results of an n-query run == an m-query run"""
    s = scenes.cornell32()
    W, H = 64, 48
    r = renderer(s, W, H)
    cam = s.camera_params()
    q = probe_queries(5000)
    once = r.render_radiance_queries(q, cam, spp=4)
    assert np.isfinite(once).all() and once[:, :3].max() > 0
    buf = np.full((len(q), 4), 7.0, np.float32)
    for k in range(4):
        r.render_radiance_queries(q, cam, spp=1, first_sample=k, results=buf)
    assert np.array_equal(float_bits(once), float_bits(buf))
    m = 1237  # not a multiple of 64
    part = r.render_radiance_queries(q[:m], cam, spp=4)
    assert np.array_equal(float_bits(once[:m]), float_bits(part))
    # and the samples matter
    assert not np.array_equal(float_bits(once), float_bits(r.render_radiance_queries(q, cam, spp=1)))
    r.close()


def test_slicing_of_queries_and_samples_does_not_show(monkeypatch):
    """5: n = 3 W H + 17 queries on a W x H handle (four slices) == the same on a W x 4H handle (one slice); RPTR_MAX_BATCH_SPP=2 at 5
    samples (three batches) == the default slots"""
    s = scenes.two_level_test()
    W, H = 72, 40
    cam = s.camera_params()
    q = probe_queries(3 * W * H + 17, seed=9)
    r = renderer(s, W, H)
    a = r.render_radiance_queries(q, cam, spp=5)
    r.close()
    r = renderer(s, W, 4 * H)
    b = r.render_radiance_queries(q, cam, spp=5)
    r.close()
    assert np.array_equal(float_bits(a), float_bits(b))
    monkeypatch.setenv("RPTR_MAX_BATCH_SPP", "2")
    r = renderer(s, W, H)
    assert r.get_option("sample_slots") == 2
    c = r.render_radiance_queries(q, cam, spp=5)
    r.close()
    assert np.array_equal(float_bits(a), float_bits(c))


@pytest.mark.parametrize("rng_variant", [abi.RNG_VARIANT_BN, abi.RNG_VARIANT_SOBOL, abi.RNG_VARIANT_Z_SBL])
def test_slicing_does_not_show_with_table_point_sets(rng_variant):
    """5 with the table point sets: on the later slices the virtual pixel row lies beyond the frame's height, and the sets make their
    sample ids, scrambles and tile positions from that pixel; wider than one 256-pixel Sobol' tile"""
    s = scenes.cornell32()
    W, H = 264, 24
    cam = s.camera_params()
    table = pointsets.default_table(rng_variant, seed=5)
    q = probe_queries(3 * W * H + 17, seed=13)
    out = []
    for h in (H, 4 * H):
        r = renderer(s, W, h)
        r.set_rng_variant(rng_variant, table)
        out.append(r.render_radiance_queries(q, cam, spp=3))
        r.close()
    assert np.isfinite(out[0]).all() and np.array_equal(float_bits(out[0]), float_bits(out[1]))
    r = renderer(s, W, H)  # and the point set matters
    u = r.render_radiance_queries(q, cam, spp=3)
    r.close()
    assert not np.array_equal(float_bits(u), float_bits(out[0]))


def test_tail_hand_over_does_not_show():
    """6: the late bounces in the tail kernel from bounce 1 / 2, or not at all: same bits"""
    s = scenes.cornell32()
    cam = s.camera_params()
    q = probe_queries(20000, seed=5)
    out = []
    for tail in (0, 1, 2):
        r = renderer(s, 128, 96, options={"tail_bounce": tail})
        out.append(r.render_radiance_queries(q, cam, spp=2))
        r.close()
    assert np.array_equal(float_bits(out[0]), float_bits(out[1])) and np.array_equal(float_bits(out[0]), float_bits(out[2]))


def test_skipped_queries_keep_their_slot_and_short_rays_see_the_sky():
    """7: mode_or_data < 0 leaves the slot alone; a query whose t_max ends before the first surface == the query in the empty scene"""
    s = scenes.cornell32()
    cam = s.camera_params()
    r = renderer(s, 64, 48)
    q = probe_queries(300, seed=11)
    skip = np.arange(0, 300, 7)
    q.view(np.int32)[skip, 3] = -5
    buf = np.full((300, 4), 1234.5, np.float32)
    r.render_radiance_queries(q, cam, spp=2, results=buf)
    assert (buf[skip] == 1234.5).all()
    keep = np.setdiff1d(np.arange(300), skip)
    assert (buf[keep] != 1234.5).any(axis=1).all()
    short = q[keep].copy()
    short[:, 7] = 1e-4
    got = r.render_radiance_queries(short, cam, spp=2)
    r.close()
    e = scenes.cornell32()
    e.instances = []
    e.prepare_lights()
    r = renderer(e, 64, 48)
    sky = r.render_radiance_queries(short, cam, spp=2)
    r.close()
    assert (got[:, 3] == 0).all() and np.array_equal(float_bits(got), float_bits(sky))


@pytest.mark.parametrize("fif", [1, 3])
def test_a_query_run_leaves_the_frame_alone(fif):
    """8: 2 spp, queries, 2 spp more without a reset: image, spp and AOV read-backs are those of the run without the queries"""
    s = scenes.two_level_test()
    W, H = 96, 64
    cam = s.camera_params()
    q = probe_queries(W * H + 50, seed=2)

    def run(with_queries):
        r = renderer(s, W, H, frames_in_flight=fif)
        cfg = backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True)
        r.render(cfg, spp=2)
        if with_queries:  # ... and right after the run: rptr_hip_stats and the image are the frame's
            before, after = abi.Stats(), abi.Stats()
            img0, img1 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
            assert r._L.rptr_hip_stats(r._h, C.byref(before)) == 0 and r.readback_framebuffer(img0) == W * H * 4
            r.render_radiance_queries(q, cam, spp=3)
            assert r._L.rptr_hip_stats(r._h, C.byref(after)) == 0 and r.readback_framebuffer(img1) == W * H * 4
            assert bytes(before) == bytes(after) and before.spp == 2 and before.rays_closest > 0
            assert np.array_equal(float_bits(img0), float_bits(img1))
        cfg.reset_accumulation = False
        st = r.render(cfg, spp=2)
        img = np.zeros((H, W, 4), np.float32)
        assert r.readback_framebuffer(img) == W * H * 4
        u8 = np.zeros((H, W, 4), np.uint8)
        assert r.readback_framebuffer(u8) == W * H * 4
        aovs = []
        for k in range(3):
            a = np.zeros((H, W, 4), np.float16)
            assert r.readback_aov(k, a) == W * H * 4
            aovs.append(a.view(np.uint16).copy())
        r.close()
        return img, u8, aovs, st.spp, int(st.raw.rays_closest), int(st.raw.rays_shadow)

    a, b = run(False), run(True)
    assert np.array_equal(float_bits(a[0]), float_bits(b[0])) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    assert a[3:] == b[3:] and a[3] == 4


def test_device_entry_budget_and_refusals():
    """9: the device entry over the enable_ray_queries buffers == the host entry; over budget, world_size 2 and bad arguments return the
    documented codes"""
    import torch
    s = scenes.cornell32()
    cam = s.camera_params()
    r = renderer(s, 64, 48)
    n = 4000
    q = probe_queries(n, seed=4)
    host = r.render_radiance_queries(q, cam, spp=3)
    dq, dr = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    r.render_radiance_queries_device(n, cam, spp=3)
    r.render_ray_queries(q[:1])  # (a synchronous call on the backend's stream: the run above has finished)
    dev = np.zeros((n, 4), np.float32)
    assert hip.hipMemcpy(dev.ctypes.data_as(C.c_void_p), dr, dev.nbytes, 2) == 0
    assert np.array_equal(float_bits(host), float_bits(dev))
    # a caller's buffers on a caller's stream
    tq = torch.from_numpy(q).cuda()
    tr = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.render_radiance_queries_device(n, cam, spp=3, device_queries=tq.data_ptr(), device_results=tr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(float_bits(host), float_bits(tr.cpu().numpy()))

    def refused(code, what, call):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == code and what in str(e.value), str(e.value)

    refused(abi.RPTR_E_INVALID, "exceed the budget", lambda: r.render_radiance_queries_device(n + 1, cam))
    refused(abi.RPTR_E_INVALID, "samples_per_query", lambda: r.render_radiance_queries(q, cam, spp=0))
    refused(abi.RPTR_E_INVALID, "first_sample", lambda: r.render_radiance_queries(q, cam, first_sample=-1))
    refused(abi.RPTR_E_INVALID, "unknown variant", lambda: r.render_radiance_queries(q, cam, variant=17))
    L = r._L
    buf = np.zeros((n, 4), np.float32)
    assert L.rptr_hip_trace_radiance(r._h, q.ctypes.data_as(C.c_void_p), n, None, 0, 1, 0, buf.ctypes.data_as(C.c_void_p), None) == abi.RPTR_E_INVALID
    assert b"NULL camera" in L.rptr_hip_last_error(r._h)
    r.close()
    r = backend.RenderHip()
    refused(abi.RPTR_E_INVALID, "before set_scene", lambda: r.render_radiance_queries(q, cam))
    r.close()
    r = backend.RenderHip()
    r.set_scene(s)
    refused(abi.RPTR_E_INVALID, "before initialize", lambda: r.render_radiance_queries(q, cam))
    r.close()
    r = backend.RenderHip(rank=0, world_size=2)
    r.initialize(64, 48)
    r.set_scene(s)
    refused(abi.RPTR_E_UNSUPPORTED, "world_size 1", lambda: r.render_radiance_queries(q, cam))
    r.close()
