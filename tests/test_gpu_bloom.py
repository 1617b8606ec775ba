"""Bloom on the GPU (csrc/bloom.h, rptr_hip_bloom) against its numpy restatement (tests/bloom_ref.py, written from the header) fed the
frame's own read-backs: every level of both pyramids bit for bit, the image byte for byte; what the call promises to leave alone is
compared before and after; every refusal is exercised."""
import ctypes as C

import numpy as np
import pytest

import auto_exposure_ref as A
import bloom_ref as R
from common import config, raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu
F = np.float32

# exposure: chosen per scene so that the default threshold lets a real part of the frame through (checked below on the restatement alone)
PARITY = [("cornell-37x21", scenes.cornell32, abi.VARIANT_GLTF, 37, 21, 1.0),
          ("grid-72x40", lambda: scenes.grid(120, 60), abi.VARIANT_SIMPLE, 72, 40, 1.0)]


def _check(r, src, fb, p, scale, what):
    """one call with parameters p against the restatement at `scale` -> (the restatement's d, u, image)"""
    used = r.bloom(**p)
    full = dict(R.DEFAULTS, **p)
    H, W = src.shape[:2]
    d, u, want_img = R.bloom(src, fb, scale, **p)
    L = r.bloom_levels()
    assert L == len(d) == R.level_count(W, H, full["levels"]), (what, L)
    for l in range(1, L + 1):
        gd, gu = r.bloom_level(0, l), r.bloom_level(1, l)
        assert gd.shape == d[l].shape, (what, l)
        nd, nu = int(np.count_nonzero(gd.view(np.uint32) != d[l].view(np.uint32))), int(np.count_nonzero(gu.view(np.uint32) != u[l].view(np.uint32)))
        assert nd == 0 and nu == 0, (what, "level %d: %d words of d, %d of u differ" % (l, nd, nu))
    got_img = r.readback_bloomed()
    n = int(np.count_nonzero(got_img != want_img))
    print("%s: L %d, d(1) non-zero in %.1f %% of its texels, %d bytes differ" % (what, L, 100.0 * float((d[1][..., :3].max(axis=-1) > 0).mean()), n))
    assert n == 0, (what, "%d bytes differ" % n)
    assert used.levels == full["levels"] and used.exposure_mode == full["exposure_mode"]
    return d, u, want_img


@pytest.mark.parametrize("name,make,variant,W,H,exposure", PARITY, ids=[c[0] for c in PARITY])
def test_pyramids_and_image_equal_the_restatement(name, make, variant, W, H, exposure):
    s = make()
    r = renderer(s, W, H)
    r.render(config(s, variant), spp=2)
    acc, fb = read_frame(r, W, H, aovs=False)
    r.denoise(iterations=2)
    den = r.readback_denoised_f32()
    assert not np.array_equal(den, acc)
    l_max = len(R.sizes(W, H)) - 1
    r.params.exposure = exposure
    scale = A.scale_of(exposure, 0.0)
    # against a vacuous pass, on the restatement alone first: the default threshold passes a real part of the frame, and the glare shows
    d, _, lit = R.bloom(acc, fb, scale)
    exposed = A.expose(acc, fb, scale)
    lit_part, changed = float((d[1][..., :3].max(axis=-1) > 0).mean()), float((lit != exposed).mean())
    print("%s at exposure %g: d(1) non-zero in %.1f %% of its texels, %.1f %% of the bytes change" % (name, exposure, 100 * lit_part, 100 * changed))
    assert lit_part > 0.01 and changed > 0.01
    assert float((R.prefilter(acc, scale)[..., :3].max(axis=-1) > 0).mean()) < 0.9          # ... and the threshold holds something back
    for source, src in ((0, acc), (1, den)):
        base = dict(source=source)
        for tm in (-1, 1, 2):
            _check(r, src, fb, dict(base, tone_mapping_mode=tm), scale, "%s source %d tm %d" % (name, source, tm))
        for levels in (1, l_max, 12, 2):
            _check(r, src, fb, dict(base, levels=levels), scale, "%s source %d levels %d" % (name, source, levels))
        for scatter in (0.0, 1.0):
            _check(r, src, fb, dict(base, scatter=scatter, levels=l_max), scale, "%s source %d scatter %g" % (name, source, scatter))
        _check(r, src, fb, dict(base, threshold=0.0, knee=0.0), scale, "%s source %d T = K = 0" % (name, source))
        _check(r, src, fb, dict(base, threshold=0.0, knee=0.0, clamp=0.5, intensity=1.5), scale, "%s source %d clamp 0.5" % (name, source))
        _check(r, src, fb, dict(base, white_balance=(1.25, 1.0, 0.75), tone_mapping_mode=1), scale, "%s source %d gains" % (name, source))
        _, _, img0 = _check(r, src, fb, dict(base, intensity=0.0, tone_mapping_mode=1, white_balance=(0.9, 1.1, 1.0)), scale, "%s source %d intensity 0" % (name, source))
        r.auto_exposure(mode=0, source=source, tone_mapping_mode=1, white_balance=(0.9, 1.1, 1.0))
        assert np.array_equal(img0, r.readback_exposed())                                    # intensity 0: the image is auto-exposure's
        r.params.exposure = 0.75
        _check(r, src, fb, dict(base, tone_mapping_mode=2), A.scale_of(0.75, 0.0), "%s source %d exposure 0.75" % (name, source))
        r.params.exposure = exposure
    assert np.array_equal(_check(r, acc, fb, dict(), scale, name + " defaults")[2], lit)
    r.close()


@pytest.mark.parametrize("name,make,variant,W,H,exposure", PARITY, ids=[c[0] for c in PARITY])
def test_the_metered_scale_is_read_on_the_device(name, make, variant, W, H, exposure):
    """exposure_mode 1 after a metered call: the scale is the restatement's state's, and the device state is what it was"""
    s = make()
    r = renderer(s, W, H)
    r.render(config(s, variant), spp=2)
    acc, fb = read_frame(r, W, H, aovs=False)
    ae = dict(key=1.5, low_percentile=0.0, high_percentile=1.0)                             # a bright key: highlights well above white
    r.params.exposure = 0.25
    r.auto_exposure(**ae)
    want = A.step(acc, ae, None, 0.25)
    before = r.readback_exposure_state()
    assert not A.same_state(A.state_of(before), want)
    exposed = r.readback_exposed()
    scale = want["scale"]
    assert scale != A.scale_of(0.25, 0.0)
    d, _, img = _check(r, acc, fb, dict(exposure_mode=1), scale, name + " metered")
    assert float((d[1][..., :3].max(axis=-1) > 0).mean()) > 0.01 and float((img != exposed).mean()) > 0.01
    _, _, img0 = _check(r, acc, fb, dict(exposure_mode=1, intensity=0.0), scale, name + " metered, intensity 0")
    assert np.array_equal(img0, exposed)                                                     # ... the matching auto-exposure call's image
    _check(r, acc, fb, dict(exposure_mode=1, levels=12, tone_mapping_mode=2, white_balance=(1.1, 1.0, 0.9)), scale, name + " metered, all levels")
    after = r.readback_exposure_state()
    assert bytes(before) == bytes(after)
    assert np.array_equal(r.readback_exposed(), exposed)                                     # the exposed image too
    r.close()


def _everything(r, W, H):
    return read_frame(r, W, H) + (r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history(), r.readback_upscaled(),
                                  r.readback_exposed(), np.frombuffer(bytes(r.readback_exposure_state()), np.uint8))


def _run(s, W, H, call_after):
    """four 1-spp frames, each denoised (temporal), upscaled and metered; call_after: frames after which bloom runs (both sources, both modes)"""
    r = renderer(s, W, H)
    out = []
    for k in range(4):
        r.render(config(s, abi.VARIANT_GLTF, reset=k == 0), spp=1)
        r.denoise_temporal(iterations=2, reset_history=1 if k == 0 else 0)
        r.taa_upscale(reset_history=1 if k == 0 else 0)
        r.auto_exposure(dt=1 / 60, key=1.0)
        before = _everything(r, W, H)
        if k in call_after:
            st0 = bytes(raw_stats(r))
            for source in (0, 1):
                for mode in (0, 1):
                    r.bloom(source=source, exposure_mode=mode, threshold=0.25, levels=12)
                    assert r.readback_bloomed().any() and r.bloom_level(1, 1).any()
            assert bytes(raw_stats(r)) == st0, k
            assert same_images(before, _everything(r, W, H)), k
        out.append(before)
    r.close()
    return out


def test_the_call_leaves_everything_else_alone():
    """the frame's five read-backs, the denoised images, the denoise history, the upscaler's output, the exposed image, the exposure state
    and the statistics are what they were, and the frames rendered, denoised, upscaled and metered after the calls are bit-identical to a
    run without them"""
    s = scenes.cornell32()
    W, H = 40, 24
    plain = _run(s, W, H, ())
    with_calls = _run(s, W, H, (1, 2))
    for k in range(4):
        assert same_images(plain[k], with_calls[k]), k


def test_an_aov_view_is_copied():
    s = scenes.cornell32()
    W, H = 37, 21
    r = renderer(s, W, H)
    r.params.output_channel = 2
    r.render(config(s, abi.VARIANT_GLTF), spp=1)
    r.bloom(threshold=0.0)
    assert np.array_equal(r.readback_bloomed(), read_frame(r, W, H, aovs=False)[1])
    assert r.bloom_levels() == 0
    with pytest.raises(backend.BackendError):
        r.bloom_level(0, 1)
    r.close()


def _refused(fn, code, fragment):
    with pytest.raises(backend.BackendError) as e:
        fn()
    assert e.value.code == code, e.value
    assert fragment in str(e.value), (fragment, str(e.value))


def test_refusals():
    s = scenes.cornell32()
    W, H = 32, 24
    cfg = config(s, abi.VARIANT_GLTF)
    INV, UNS = abi.RPTR_E_INVALID, abi.RPTR_E_UNSUPPORTED
    r = renderer(s, W, H)
    L, h = r._L, r._h
    _refused(r.bloom, INV, "before a frame")
    _refused(r.readback_bloomed, INV, "rptr_hip_bloom first")
    _refused(r.bloom_levels, INV, "")
    _refused(lambda: r.bloom_level(0, 1), INV, "rptr_hip_bloom first")
    assert L.rptr_hip_bloom(None, C.byref(abi.BloomParams())) == INV
    r.render(cfg, spp=1)
    _refused(r.readback_bloomed, INV, "rptr_hip_bloom first")                        # a frame, but no call
    nan, inf = float("nan"), float("inf")
    for bad, fragment in ((dict(source=2), "source"), (dict(source=-1), "source"), (dict(exposure_mode=2), "exposure_mode"), (dict(exposure_mode=-1), "exposure_mode"),
                          (dict(tone_mapping_mode=3), "tone_mapping_mode"), (dict(tone_mapping_mode=-2), "tone_mapping_mode"),
                          (dict(levels=-1), "levels"), (dict(levels=13), "levels"),
                          (dict(threshold=-0.5), "threshold"), (dict(threshold=nan), "threshold"), (dict(threshold=inf), "threshold"),
                          (dict(knee=-1.0), "knee"), (dict(knee=nan), "knee"), (dict(knee=inf), "knee"),
                          (dict(clamp=0.0), "clamp"), (dict(clamp=-1.0), "clamp"), (dict(clamp=nan), "clamp"), (dict(clamp=inf), "clamp"),
                          (dict(intensity=-0.1), "intensity"), (dict(intensity=nan), "intensity"), (dict(intensity=inf), "intensity"),
                          (dict(scatter=-0.1), "scatter"), (dict(scatter=1.5), "scatter"), (dict(scatter=nan), "scatter"),
                          (dict(white_balance=(1.0, 0.0, 1.0)), "white_balance"), (dict(white_balance=(1.0, 1.0, nan)), "white_balance"),
                          (dict(white_balance=(inf, 1.0, 1.0)), "white_balance")):
        _refused(lambda: r.bloom(**bad), INV, fragment)
    for k in range(4):
        p = abi.BloomParams()
        L.rptr_hip_bloom_defaults(C.byref(p))
        p.reserved[k] = 1
        _refused(lambda: r.bloom(p), INV, "reserved")
    _refused(lambda: r.bloom(source=1), INV, "no denoised image")                   # source 1 before any denoise call
    _refused(lambda: r.bloom(exposure_mode=1), INV, "mode 1 first")                 # no metered call since initialize
    r.auto_exposure(mode=0)
    _refused(lambda: r.bloom(exposure_mode=1), INV, "mode 1 first")                 # a manual call leaves no state
    assert L.rptr_hip_bloom(h, None) == 0                                            # NULL: the defaults
    assert r.readback_bloomed().shape == (H, W, 4) and r.bloom_levels() == R.level_count(W, H) == 4
    buf = np.zeros(8, np.uint8)
    assert L.rptr_hip_readback_bloomed_u8(h, buf.ctypes.data_as(C.c_void_p), buf.size) == INV      # too small
    assert L.rptr_hip_readback_bloomed_u8(h, None, 0) == INV and L.rptr_hip_bloom_levels(h, None) == INV
    small = np.zeros(4 * (16 * 12 - 1), F)
    assert L.rptr_hip_readback_bloom_level_f32(h, 0, 1, small.ctypes.data_as(C.c_void_p), small.size) == INV
    assert L.rptr_hip_readback_bloom_level_f32(h, 0, 1, None, 0) == INV
    _refused(lambda: r.bloom_level(0, 0), INV, "outside 1")
    _refused(lambda: r.bloom_level(1, 5), INV, "outside 1")
    _refused(lambda: r.bloom_level(2, 1), INV, "which")
    assert r.bloom_level(1, 3).shape == (3, 4, 4)
    r.auto_exposure()
    r.bloom(exposure_mode=1)                                                         # a metered call: allowed now
    r.denoise(iterations=1)
    r.bloom(source=1)
    r.render(cfg, spp=1)                                                             # a later frame: the image, the levels, the denoised source are stale
    _refused(r.readback_bloomed, INV, "stale")
    _refused(lambda: r.bloom_level(0, 1), INV, "stale")
    _refused(lambda: r.bloom(source=1), INV, "stale")
    r.bloom(exposure_mode=1)                                                         # (the exposure state stays: the scale of the last metered call)
    r.readback_bloomed()
    r.initialize(W, H)                                                               # initialize: no image, no state, no frame
    _refused(r.readback_bloomed, INV, "rptr_hip_bloom first")
    _refused(r.bloom, INV, "before a frame")
    r.set_scene(s)
    r.render(cfg, spp=1)
    _refused(lambda: r.bloom(exposure_mode=1), INV, "mode 1 first")
    r.bloom()
    r.readback_bloomed()
    r.params.render_upscale_factor = 2
    _refused(r.bloom, UNS, "render_upscale_factor")
    r.params.render_upscale_factor = 1
    r.bloom()
    r.close()
    r = renderer(s, W, H, options={"aovs": 0})
    r.render(cfg, spp=1)
    _refused(lambda: r.bloom(source=1), UNS, '"aovs" is 0')
    r.bloom(source=0)                                                                # source 0 needs no AOV image
    assert r.readback_bloomed().any()
    r.close()
    r = renderer(s, W, H, rank=0, world_size=2, stripe_rows=8)
    r.render(cfg, spp=1)
    _refused(r.bloom, UNS, "world_size")
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                        # the waited frame's context is being rendered to again
    t0 = r.render_async(cfg, spp=1)
    r.wait(t0)
    t1 = r.render_async(cfg, spp=1)
    t2 = r.render_async(cfg, spp=1)
    _refused(r.bloom, INV, "overwritten")
    r.wait(t1)
    r.wait(t2)
    r.bloom()
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                        # a frame of a launch sequence other than its last
    tickets = r.render_batch_async(cfg, spp=1, n_frames=2)
    r.wait(tickets[0])
    _refused(r.bloom, INV, "launch sequence")
    r.wait(tickets[1])
    r.bloom()
    r.close()
