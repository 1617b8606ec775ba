"""The denoiser on the GPU (csrc/denoise.h, rptr_hip_denoise) against its numpy restatement (tests/denoise_ref.py, written from the
header) fed the frame's own read-backs: the stored images must agree bit for bit and byte for byte; and what the call promises to leave
alone -- the frame's images, its history, the statistics -- is compared before and after."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
from common import config, raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu


PARITY = [("cornell-37x21", scenes.cornell32, abi.VARIANT_GLTF, 37, 21, False),
          ("grid-sky-72x40", lambda: scenes.grid(120, 60), abi.VARIANT_SIMPLE, 72, 40, True)]


@pytest.mark.parametrize("name,make,variant,W,H,sky", PARITY, ids=[c[0] for c in PARITY])
def test_denoised_images_equal_the_restatement_bit_for_bit(name, make, variant, W, H, sky):
    """a 2-spp frame, iterations 1, 2, 3, 5 x demodulation on / off x normal_power_log2 0 / 7: the float image equals the restatement
    bit for bit and the RGBA8 image byte for byte. 37 x 21: partial tiles on both axes, pass 5's taps at +-32 all fall outside; 72 x 40:
    several tiles, sky pixels (not surface), lattice tiles of spacing 4, 8, 16 with empty lanes."""
    s = make()
    r = renderer(s, W, H)
    r.render(config(s, variant), spp=2)
    acc, fb, alb, nd, _ = read_frame(r, W, H)
    surf = D.surface(nd, alb)
    assert surf.any() and (not sky or (~surf).any()), (int(surf.sum()), surf.size)
    bad = []
    for it in (1, 2, 3, 5):
        for demod in (1, 0):
            for k in (0, 7):
                r.denoise(iterations=it, demodulate_albedo=demod, normal_power_log2=k)
                got_f, got_u = r.readback_denoised_f32(), r.readback_denoised_u8()
                want_f, want_u = D.denoise(acc, alb, nd, fb, iterations=it, demodulate_albedo=demod, normal_power_log2=k)
                nf = int(np.count_nonzero(got_f.view(np.uint32) != want_f.view(np.uint32)))
                nu = int(np.count_nonzero(got_u != want_u))
                print("%s it=%d demod=%d k=%d: %d float words, %d bytes differ" % (name, it, demod, k, nf, nu))
                if nf or nu:
                    bad.append((it, demod, k, nf, nu))
                if it == 5 and demod == 1 and k == 7:
                    assert not np.array_equal(got_f[surf], acc[surf])   # the filter does something
                    assert np.array_equal(got_f.view(np.uint32)[~surf], acc.view(np.uint32)[~surf])
    r.close()
    assert not bad, bad


def test_non_default_sigmas_exposure_and_tone_mapping_equal_the_restatement():
    """the parameters the parity cases leave at their defaults: both sigmas, exposure and the two tone-mapping modes of the RGBA8 image,
    and output_channel != 0 (the RGBA8 image is a copy of the frame's)"""
    s = scenes.cornell32()
    W, H = 37, 21
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_GLTF), spp=2)
    acc, fb, alb, nd, _ = read_frame(r, W, H)
    for mode, exposure in ((-1, 0.0), (1, 1.5), (2, -0.75)):
        r.params.early_tone_mapping_mode = mode
        r.params.exposure = exposure
        r.denoise(iterations=3, sigma_luminance=1.5, sigma_depth=0.25)
        want_f, want_u = D.denoise(acc, alb, nd, fb, iterations=3, sigma_luminance=1.5, sigma_depth=0.25, exposure=exposure, tone_mapping_mode=mode)
        assert np.array_equal(r.readback_denoised_f32().view(np.uint32), want_f.view(np.uint32)), mode
        got_u = r.readback_denoised_u8()
        assert np.array_equal(got_u, want_u), (mode, int(np.count_nonzero(got_u != want_u)))
    r.params.output_channel = 2
    r.denoise(iterations=1)
    assert np.array_equal(r.readback_denoised_u8(), fb)
    r.close()


def test_it_denoises():
    """Cornell at 64 x 64, 1 spp: against a 512-spp render of the same view the denoised image's RMSE is strictly lower than the raw one's"""
    s = scenes.cornell32()
    W, H = 64, 64
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_GLTF), spp=512)
    ref = read_frame(r, W, H)[0]
    r.render(config(s, abi.VARIANT_GLTF), spp=1)
    raw = read_frame(r, W, H)[0]
    r.denoise()
    den = r.readback_denoised_f32()
    r.close()
    rmse = lambda img: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2)))
    print("rmse raw %.5f denoised %.5f" % (rmse(raw), rmse(den)))
    assert rmse(den) < rmse(raw), (rmse(den), rmse(raw))


def _run(scene, variant, W, H, mode, taa, denoise_after):
    """frames 0..3 of 1 spp (no reset after the first); denoise_after: frame indices after which denoise() is called. -> per frame its
    read-backs, and the handle's stats bytes before / after each denoise call"""
    r = renderer(scene, W, H, options={"taa": 1} if taa else None)
    r.params.reprojection_mode = mode
    out, stats = [], []
    for k in range(4):
        r.render(config(scene, variant, reset=k == 0), spp=1)
        before = read_frame(r, W, H)
        if k in denoise_after:
            st0 = bytes(raw_stats(r))
            r.denoise(iterations=5)
            den = r.readback_denoised_f32()
            assert not np.array_equal(den, before[0])
            stats.append((st0, bytes(raw_stats(r))))
            assert same_images(before, read_frame(r, W, H)), k     # the frame's own images and AOVs are what they were
        out.append(before)
    r.close()
    return out, stats


@pytest.mark.parametrize("mode,taa", [(0, False), (2, True)], ids=["mode0", "mode2-taa"])
def test_frame_state_is_left_alone(mode, taa):
    """readback_f32 / _u8, the three AOVs and stats() are identical before and after a denoise call, and the two frames rendered after
    it -- accumulating in mode 0, reprojected and anti-aliased in mode 2 with "taa" -- are bit-identical to a run without the call"""
    s = scenes.cornell32()
    W, H = 40, 24
    plain, _ = _run(s, abi.VARIANT_GLTF, W, H, mode, taa, ())
    with_call, stats = _run(s, abi.VARIANT_GLTF, W, H, mode, taa, (1,))
    assert len(stats) == 1 and stats[0][0] == stats[0][1]
    for k in range(4):
        assert same_images(plain[k], with_call[k]), k


def test_frames_in_flight_denoise_the_waited_frame():
    """two frame contexts: frame 0 is waited for while frame 1 is already submitted; denoising then works on frame 0's context images
    and equals the synchronous run bit for bit"""
    s = scenes.cornell32()
    W, H = 40, 24
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_GLTF), spp=1)
    r.denoise(iterations=4)
    want_f, want_u = r.readback_denoised_f32(), r.readback_denoised_u8()
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)
    t0 = r.render_async(config(s, abi.VARIANT_GLTF), spp=1)
    t1 = r.render_async(config(s, abi.VARIANT_GLTF, reset=False), spp=1)
    r.wait(t0)
    r.denoise(iterations=4)
    got_f, got_u = r.readback_denoised_f32(), r.readback_denoised_u8()
    r.wait(t1)
    with pytest.raises(backend.BackendError) as e:   # frame 1 is the read-backs' frame now: the denoised image is stale
        r.readback_denoised_f32()
    assert e.value.code == abi.RPTR_E_INVALID and "stale" in str(e.value)
    r.close()
    assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)) and np.array_equal(got_u, want_u)


def _refused(fn, code):
    with pytest.raises(backend.BackendError) as e:
        fn()
    assert e.value.code == code, e.value
    assert len(str(e.value).split(": ", 1)[1]) > 0
    return str(e.value)


def test_refusals():
    s = scenes.cornell32()
    W, H = 32, 24
    cfg = config(s, abi.VARIANT_GLTF)
    INV, UNS = abi.RPTR_E_INVALID, abi.RPTR_E_UNSUPPORTED
    r = renderer(s, W, H)
    assert "before a frame" in _refused(r.denoise, INV)                     # no frame yet
    assert "rptr_hip_denoise first" in _refused(r.readback_denoised_f32, INV)
    r.render(cfg, spp=1)
    _refused(r.readback_denoised_f32, INV)                                  # a frame, but no denoise call
    _refused(r.readback_denoised_u8, INV)
    L, h = r._L, r._h
    assert L.rptr_hip_denoise(h, None) == INV and L.rptr_hip_last_error(h)
    assert L.rptr_hip_denoise(None, C.byref(abi.DenoiseParams())) == INV
    for bad in (dict(iterations=0), dict(iterations=6), dict(sigma_luminance=0.0), dict(sigma_luminance=float("nan")), dict(sigma_depth=-1.0),
                dict(sigma_depth=float("inf")), dict(normal_power_log2=-1), dict(normal_power_log2=9), dict(demodulate_albedo=2)):
        _refused(lambda: r.denoise(**bad), INV)
    p = abi.DenoiseParams()
    L.rptr_hip_denoise_defaults(C.byref(p))
    p.reserved[1] = 1
    assert "reserved" in _refused(lambda: r.denoise(p), INV)
    r.denoise()
    assert r.readback_denoised_f32().shape == (H, W, 4)
    buf = np.zeros(8, np.float32)
    assert L.rptr_hip_readback_denoised_f32(h, buf.ctypes.data_as(C.c_void_p), buf.size) == INV     # too small
    assert L.rptr_hip_readback_denoised_f32(h, None, 0) == INV
    r.render(cfg, spp=1)                                                    # a later frame: stale
    assert "stale" in _refused(r.readback_denoised_f32, INV)
    assert "stale" in _refused(r.readback_denoised_u8, INV)
    r.denoise()
    r.readback_denoised_u8()
    r.initialize(W, H)                                                      # initialize: stale, and no frame any more
    _refused(r.readback_denoised_f32, INV)
    _refused(r.denoise, INV)
    r.set_scene(s)
    r.render(cfg, spp=1)
    r.params.render_upscale_factor = 2
    assert "render_upscale_factor" in _refused(r.denoise, UNS)
    r.params.render_upscale_factor = 1
    r.denoise()
    r.close()
    r = renderer(s, W, H, options={"aovs": 0})
    r.render(cfg, spp=1)
    assert '"aovs" is 0' in _refused(r.denoise, UNS)
    r.close()
    r = renderer(s, W, H, rank=0, world_size=2, stripe_rows=8)
    r.render(cfg, spp=1)
    assert "world_size" in _refused(r.denoise, UNS)
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                # the waited frame's context is being rendered to again
    t0 = r.render_async(cfg, spp=1)
    r.wait(t0)
    t1 = r.render_async(cfg, spp=1)
    t2 = r.render_async(cfg, spp=1)
    assert "overwritten" in _refused(r.denoise, INV)
    r.wait(t1)
    r.wait(t2)
    r.denoise()
    r.close()
