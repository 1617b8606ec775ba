"""The temporal denoiser on the GPU (csrc/denoise_temporal.h, rptr_hip_denoise_temporal) against its numpy restatement
(tests/denoise_temporal_ref.py, written from the header) fed the frames' own read-backs and its own history: the stored images and the
history must agree bit for bit and byte for byte along a moving camera; a call without history equals rptr_hip_denoise; and what the call
promises to leave alone is compared before and after."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import denoise_temporal_ref as T
from common import config, float_bits, fly_camera, raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu


SCENES = [("cornell-37x21", scenes.cornell32, abi.VARIANT_GLTF, 37, 21),
          ("grid-sky-72x40", lambda: scenes.grid(120, 60), abi.VARIANT_SIMPLE, 72, 40)]
PARAMS = [("defaults", {}),
          ("non-default", dict(iterations=2, alpha_color=0.5, alpha_moments=0.1, normal_threshold=0.5, depth_tolerance=0.02, demodulate_albedo=0))]
PARITY = [(s[0] + "-" + p[0],) + s[1:] + (p[1],) for s in SCENES for p in PARAMS]


@pytest.mark.parametrize("name,make,variant,W,H,fields", PARITY, ids=[c[0] for c in PARITY])
def test_images_and_history_equal_the_restatement_bit_for_bit(name, make, variant, W, H, fields):
    """5 frames of 1 spp along the fly-through path in reprojection_mode 1 (a frame shows its own samples), one call per frame: after
    every call the float image, the RGBA8 image and the history equal the restatement's, which is fed the frame's read-backs and keeps its
    own history. 37 x 21: partial tiles on both axes; 72 x 40: several tiles, sky. On the Cornell box the case is shown not to pass
    trivially: there is motion, pixels with and without history from the second frame on, and the result is not rptr_hip_denoise's."""
    s = make()
    r = renderer(s, W, H)
    r.params.reprojection_mode = 1
    td = T.TemporalDenoiser()
    cam = s.camera_params()
    bad = []
    for k in range(5):
        r.render(config(s, variant, reset=k == 0, camera=fly_camera(cam, k)), spp=1)
        acc, fb, alb, nd, mj = read_frame(r, W, H)
        r.denoise_temporal(**fields)
        got_f, got_u, got_h = r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history()
        want_f, want_u = td.step(acc, alb, nd, mj, fb, **fields)
        want_h = td.history()
        nf = int(np.count_nonzero(float_bits(got_f) != float_bits(want_f)))
        nu = int(np.count_nonzero(got_u != want_u))
        nh = int(np.count_nonzero(float_bits(got_h) != float_bits(want_h)))
        surf = D.surface(nd, alb)
        n = got_h[..., 3]
        moved = int(np.count_nonzero(mj[..., :2]))
        print("%s frame %d: %d float words, %d bytes, %d history words differ; surface %d of %d, n' > 1 on %d, n' == 1 on %d, motion != 0 in %d halfs"
              % (name, k, nf, nu, nh, int(surf.sum()), surf.size, int((n[surf] > 1).sum()), int((n[surf] == 1).sum()), moved))
        if nf or nu or nh:
            bad.append((k, nf, nu, nh))
        assert surf.any() and np.all(n[~surf] == 0)
        if name.startswith("cornell"):
            if k >= 1:
                assert moved > 0, k
                assert (n[surf] > 1).any() and (n[surf] == 1).any(), k
            if k == 4:
                spatial = {f: v for f, v in fields.items() if f in D.DEFAULTS}
                r.denoise(**spatial)
                assert not np.array_equal(float_bits(r.readback_denoised_f32()), float_bits(got_f))
        else:
            assert (~surf).any()
    r.close()
    assert not bad, bad


def test_first_call_reset_and_reinitialize_equal_the_spatial_denoiser():
    """a call without history -- the first one, one with reset_history = 1, the first after initialize at another size, one whose
    demodulate_albedo differs from the history's -- stores rptr_hip_denoise's images of the same frame bit for bit"""
    s = scenes.cornell32()
    W, H = 37, 21
    r = renderer(s, W, H)
    r.params.reprojection_mode = 1

    def both(**fields):
        spatial = {f: v for f, v in fields.items() if f in D.DEFAULTS}
        r.denoise(**spatial)
        want = r.readback_denoised_f32(), r.readback_denoised_u8()
        r.denoise_temporal(**fields)
        got = r.readback_denoised_f32(), r.readback_denoised_u8()
        return same_images(got, want), r.readback_denoise_history()

    r.render(config(s, abi.VARIANT_GLTF), spp=1)
    same, hist = both(iterations=3)
    assert same and set(np.unique(hist[..., 3])) <= {0.0, 1.0}                       # the first call
    r.render(config(s, abi.VARIANT_GLTF, reset=False), spp=1)
    same, hist = both(iterations=3)
    assert not same and hist[..., 3].max() == 2                                      # (a call with history is another image)
    r.render(config(s, abi.VARIANT_GLTF, reset=False), spp=1)
    same, hist = both(iterations=3, reset_history=1)
    assert same and hist[..., 3].max() == 1                                          # reset_history
    r.render(config(s, abi.VARIANT_GLTF, reset=False), spp=1)
    same, hist = both(iterations=3, demodulate_albedo=0)
    assert same and hist[..., 3].max() == 1                                          # the history is in other units
    W, H = 40, 24
    r.initialize(W, H)
    r.set_scene(s)
    with pytest.raises(backend.BackendError):
        r.readback_denoise_history()                                                 # initialize dropped it
    r.render(config(s, abi.VARIANT_GLTF), spp=1)
    same, hist = both(iterations=3, demodulate_albedo=0)
    assert same and hist.shape == (H, W, 4) and hist[..., 3].max() == 1              # the first call after initialize at another size
    r.close()


def test_it_denoises_better_than_one_frame_can():
    """static camera, Cornell at 64 x 64, 1 spp per frame in mode 1, 8 calls: against a 512-spp render the result's RMSE is strictly below
    the spatial denoiser's on the 8th frame, and below the raw frame's"""
    s = scenes.cornell32()
    W, H = 64, 64
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_GLTF), spp=512)
    ref = read_frame(r, W, H)[0]
    r.params.reprojection_mode = 1
    raws = []
    for k in range(8):
        r.render(config(s, abi.VARIANT_GLTF, reset=k == 0), spp=1)
        raws.append(read_frame(r, W, H)[0])
        if k == 1:
            assert not np.array_equal(raws[0], raws[1])                              # fresh samples per frame
        r.denoise_temporal()
    temporal = r.readback_denoised_f32()
    r.denoise()
    spatial = r.readback_denoised_f32()
    r.close()
    rmse = lambda img: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2)))
    print("rmse raw %.5f spatial %.5f temporal (8 calls) %.5f" % (rmse(raws[-1]), rmse(spatial), rmse(temporal)))
    assert rmse(temporal) < rmse(spatial) and rmse(temporal) < rmse(raws[-1]), (rmse(temporal), rmse(spatial), rmse(raws[-1]))


def _run(scene, variant, W, H, mode, taa, calls_after):
    """frames 0..3 of 1 spp (no reset after the first); calls_after: frame indices after which denoise_temporal() is called. -> per frame
    its read-backs, and the handle's stats bytes before / after each call"""
    r = renderer(scene, W, H, options={"taa": 1} if taa else None)
    r.params.reprojection_mode = mode
    out, stats = [], []
    for k in range(4):
        r.render(config(scene, variant, reset=k == 0), spp=1)
        before = read_frame(r, W, H)
        if k in calls_after:
            st0 = bytes(raw_stats(r))
            r.denoise_temporal()
            den = r.readback_denoised_f32()
            assert not np.array_equal(den, before[0])
            stats.append((st0, bytes(raw_stats(r))))
            assert same_images(before, read_frame(r, W, H)), k     # the frame's own images and AOVs are what they were
        out.append(before)
    r.close()
    return out, stats


@pytest.mark.parametrize("mode,taa", [(0, False), (2, True)], ids=["mode0", "mode2-taa"])
def test_frame_state_is_left_alone(mode, taa):
    """readback_f32 / _u8, the three AOVs and stats() are identical before and after a call, and the frames rendered between and after
    the calls -- accumulating in mode 0, reprojected and anti-aliased in mode 2 with "taa" -- are bit-identical to a run without them"""
    s = scenes.cornell32()
    W, H = 40, 24
    plain, _ = _run(s, abi.VARIANT_GLTF, W, H, mode, taa, ())
    with_calls, stats = _run(s, abi.VARIANT_GLTF, W, H, mode, taa, (0, 1, 2))
    assert len(stats) == 3 and all(a == b for a, b in stats)
    for k in range(4):
        assert same_images(plain[k], with_calls[k]), k


def test_a_spatial_call_between_two_temporal_calls_changes_nothing():
    """rptr_hip_denoise rewrites the denoiser's (N, z) image; the history has its own, so the next temporal result is what it is
    without the call"""
    s = scenes.cornell32()
    W, H = 40, 24
    results = []
    for interleave in (False, True):
        r = renderer(s, W, H)
        r.params.reprojection_mode = 1
        cam = s.camera_params()
        for k in range(3):
            r.render(config(s, abi.VARIANT_GLTF, reset=k == 0, camera=fly_camera(cam, k)), spp=1)
            r.denoise_temporal()
            out = r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history()
            if interleave:
                r.denoise(iterations=2, demodulate_albedo=0)
                assert not np.array_equal(r.readback_denoised_f32(), out[0])    # the read-backs return the call that ran last
        results.append(out)
        r.close()
    assert results[0][2][..., 3].max() == 3
    assert same_images(results[0], results[1])


def test_frames_in_flight_denoise_the_waited_frame():
    """two frame contexts: each frame is waited for while the next one is already submitted; the temporal calls then work on the waited
    frame's context images and equal the synchronous run bit for bit"""
    s = scenes.cornell32()
    W, H = 40, 24
    r = renderer(s, W, H)
    want = []
    for k in range(2):
        r.render(config(s, abi.VARIANT_GLTF, reset=k == 0), spp=1)
        r.denoise_temporal(iterations=4)
        want.append((r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history()))
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)
    t0 = r.render_async(config(s, abi.VARIANT_GLTF), spp=1)
    t1 = r.render_async(config(s, abi.VARIANT_GLTF, reset=False), spp=1)
    r.wait(t0)
    r.denoise_temporal(iterations=4)
    got0 = r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history()
    r.wait(t1)
    with pytest.raises(backend.BackendError) as e:   # frame 1 is the read-backs' frame now: the denoised image is stale
        r.readback_denoised_f32()
    assert e.value.code == abi.RPTR_E_INVALID and "stale" in str(e.value)
    r.denoise_temporal(iterations=4)
    got1 = r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history()
    r.close()
    assert same_images(got0, want[0]) and same_images(got1, want[1])
    assert want[1][2][..., 3].max() == 2


def _refused(fn, code, names_call=True):
    with pytest.raises(backend.BackendError) as e:
        fn()
    assert e.value.code == code, e.value
    assert not names_call or "rptr_hip_denoise_temporal" in str(e.value), e.value
    return str(e.value)


def test_refusals():
    s = scenes.cornell32()
    W, H = 32, 24
    cfg = config(s, abi.VARIANT_GLTF)
    INV, UNS = abi.RPTR_E_INVALID, abi.RPTR_E_UNSUPPORTED
    r = renderer(s, W, H)
    assert "before a frame" in _refused(r.denoise_temporal, INV)                 # no frame yet
    assert "rptr_hip_denoise_temporal first" in _refused(r.readback_denoise_history, INV, False)
    r.render(cfg, spp=1)
    _refused(r.readback_denoise_history, INV, False)                             # a frame, but no temporal call
    r.denoise()
    _refused(r.readback_denoise_history, INV, False)                             # ... and the spatial one leaves no history
    L, h = r._L, r._h
    assert L.rptr_hip_denoise_temporal(None, None) == INV
    nan, inf = float("nan"), float("inf")
    for bad in (dict(iterations=0), dict(iterations=6), dict(sigma_luminance=0.0), dict(sigma_luminance=nan), dict(sigma_depth=-1.0),
                dict(sigma_depth=inf), dict(normal_power_log2=-1), dict(normal_power_log2=9), dict(demodulate_albedo=2),
                dict(alpha_color=0.0), dict(alpha_color=1.5), dict(alpha_color=nan), dict(alpha_moments=0.0), dict(alpha_moments=-0.5),
                dict(alpha_moments=nan), dict(normal_threshold=-1.5), dict(normal_threshold=1.25), dict(normal_threshold=nan),
                dict(depth_tolerance=-0.1), dict(depth_tolerance=inf), dict(depth_tolerance=nan), dict(reset_history=2), dict(reset_history=-1)):
        _refused(lambda: r.denoise_temporal(**bad), INV)
    _refused(r.readback_denoise_history, INV, False)                             # a refused call leaves no history either
    p = abi.DenoiseTemporalParams()
    L.rptr_hip_denoise_temporal_defaults(C.byref(p))
    p.reserved[5] = 1
    assert "reserved" in _refused(lambda: r.denoise_temporal(p), INV)
    assert L.rptr_hip_denoise_temporal(h, None) == 0                             # NULL: the defaults
    assert r.readback_denoise_history().shape == (H, W, 4)
    r.denoise_temporal(alpha_color=1.0, alpha_moments=1.0, normal_threshold=-1.0, depth_tolerance=0.0)   # the ends of the ranges
    buf = np.zeros(8, np.float32)
    assert L.rptr_hip_readback_denoise_history_f32(h, buf.ctypes.data_as(C.c_void_p), buf.size) == INV   # too small
    assert L.rptr_hip_readback_denoise_history_f32(h, None, 0) == INV
    r.render(cfg, spp=1)                                                         # a later frame: the denoised image is stale,
    assert "stale" in _refused(r.readback_denoised_f32, INV, False)
    assert r.readback_denoise_history().shape == (H, W, 4)                       # the history is what the last call left
    r.initialize(W, H)                                                           # initialize: no history, and no frame any more
    _refused(r.readback_denoise_history, INV, False)
    _refused(r.denoise_temporal, INV)
    r.set_scene(s)
    r.render(cfg, spp=1)
    r.params.render_upscale_factor = 2
    assert "render_upscale_factor" in _refused(r.denoise_temporal, UNS)
    r.params.render_upscale_factor = 1
    r.denoise_temporal()
    r.close()
    r = renderer(s, W, H, options={"aovs": 0})
    r.render(cfg, spp=1)
    msg = _refused(r.denoise_temporal, UNS)
    assert '"aovs" is 0' in msg and "motion" in msg
    r.close()
    r = renderer(s, W, H, rank=0, world_size=2, stripe_rows=8)
    r.render(cfg, spp=1)
    assert "world_size" in _refused(r.denoise_temporal, UNS)
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                     # the waited frame's context is being rendered to again
    t0 = r.render_async(cfg, spp=1)
    r.wait(t0)
    t1 = r.render_async(cfg, spp=1)
    t2 = r.render_async(cfg, spp=1)
    assert "overwritten" in _refused(r.denoise_temporal, INV)
    r.wait(t1)
    r.wait(t2)
    r.denoise_temporal()
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                     # the waited frame is not the last of its launch sequence
    tickets = r.render_batch_async(cfg, spp=1, n_frames=2, reset_rest=False)
    r.wait(tickets[0])
    assert "launch sequence" in _refused(r.denoise_temporal, INV)
    r.wait(tickets[1])
    r.denoise_temporal()
    r.close()
