"""Auto-exposure on the GPU (csrc/auto_exposure.h, rptr_hip_auto_exposure) against its numpy restatement (tests/auto_exposure_ref.py,
written from the header) fed the frame's own read-backs: the histogram and the counts must be equal, the four state floats bit for bit,
the image byte for byte; and what the call promises to leave alone is compared before and after."""
import ctypes as C

import numpy as np
import pytest

import auto_exposure_ref as A
from common import config, raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu
F = np.float32

PARITY = [("cornell-37x21", scenes.cornell32, abi.VARIANT_GLTF, 37, 21),
          ("grid-sky-72x40", lambda: scenes.grid(120, 60), abi.VARIANT_SIMPLE, 72, 40)]


def _camera(scene, direction=None):
    cam = scene.camera_params()
    if direction is not None:
        cam.dir[:] = [float(v) for v in direction]
    return cam


SKY = (0.0, 0.8, -0.6)   # pitched up 53 degrees: with the grid's 65-degree field of view the lowest ray is 20 degrees above the horizon


def _check(r, src, fb, p, prev, exposure, what):
    """one call with parameters p against the restatement; prev: the restatement's state before it. -> the state after it"""
    used = r.auto_exposure(**p)
    full = dict(A.DEFAULTS, **p)
    got_img = r.readback_exposed()
    if full["mode"] == 1:
        want = A.step(src, p, prev, exposure)
        got = A.state_of(r.readback_exposure_state())
        bad = A.same_state(got, want)
        print("%s: ev %.6f target %.6f mean %.6f scale %.6f counted %d black %d ignored %d calls %d%s" % (
            what, got["ev"], got["target_ev"], got["mean_log2"], got["scale"], got["counted"], got["black"], got["ignored"], got["calls"],
            "  DIFFERS in " + ", ".join(bad) if bad else ""))
        assert not bad, (what, bad, {k: (got[k], want[k]) for k in bad if k != "histogram"})
        scale, after = want["scale"], want
    else:
        scale, after = A.scale_of(exposure, 0.0), prev
    want_img = A.expose(src, fb, scale, full["tone_mapping_mode"], full["white_balance"])
    n = int(np.count_nonzero(got_img != want_img))
    assert n == 0, (what, "%d bytes differ" % n)
    assert used.mode == full["mode"] and used.source == full["source"]
    return after


@pytest.mark.parametrize("name,make,variant,W,H", PARITY, ids=[c[0] for c in PARITY])
def test_histogram_state_and_image_equal_the_restatement(name, make, variant, W, H):
    """a 2-spp frame; source 0 and 1 (after denoise(iterations=2)) x mode 0 / 1 x tone mapping -1 / 1 / 2, then, metering: percentiles
    (0, 1), a clamping max_ev, non-unit gains, exposure != 0, a rate-limited step. 37 x 21: 777 pixels, three full blocks and a partial
    one; 72 x 40: twelve blocks (the grid cap is not reached), sky rows whose waves hold a few bins."""
    s = make()
    r = renderer(s, W, H)
    r.render(config(s, variant), spp=2)
    acc, fb = read_frame(r, W, H, aovs=False)
    r.denoise(iterations=2)
    den = r.readback_denoised_f32()
    assert not np.array_equal(den, acc)
    prev = None
    for source, src in ((0, acc), (1, den)):
        for mode in (0, 1):
            for tm in (-1, 1, 2):
                prev = _check(r, src, fb, dict(source=source, mode=mode, tone_mapping_mode=tm), prev, 0.0, "%s source %d mode %d tm %d" % (name, source, mode, tm))
        base = dict(source=source, tone_mapping_mode=1)
        prev = _check(r, src, fb, dict(base, low_percentile=0.0, high_percentile=1.0), prev, 0.0, name + " percentiles (0, 1)")
        assert prev["target_ev"] > -1.0
        prev = _check(r, src, fb, dict(base, max_ev=-1.0, min_ev=-3.0), prev, 0.0, name + " max_ev -1")
        assert prev["target_ev"] == F(-1.0)                                           # clamped
        prev = _check(r, src, fb, dict(base, white_balance=(1.25, 1.0, 0.75)), prev, 0.0, name + " gains")
        prev = _check(r, src, fb, dict(base, white_balance=(0.9, 1.1, 1.0), mode=0), prev, 0.0, name + " gains, manual")
        prev = _check(r, src, fb, dict(base, dt=1 / 60, speed_up=0.5, speed_down=4.0, key=0.5), prev, 0.0, name + " adapting")
        assert prev["ev"] != prev["target_ev"] and prev["calls"] > 1
        r.params.exposure = 0.75
        prev = _check(r, src, fb, dict(base, reset_history=1), prev, 0.75, name + " exposure 0.75")
        assert prev["calls"] == 1 and prev["scale"] == F(np.exp2(np.float64(F(0.75) + prev["ev"])))
        prev = _check(r, src, fb, dict(base, mode=0), prev, 0.75, name + " exposure 0.75, manual")
        r.params.exposure = 0.0
    assert prev["counted"] + prev["black"] + prev["ignored"] == W * H
    r.close()


def test_a_view_of_sky_only_counts_every_pixel_in_a_handful_of_bins():
    """few distinct bins among a wave's 64 lanes: many lanes add to the same LDS word (all 64: tests/test_gpu_auto_exposure_probe.py)"""
    s = scenes.grid(120, 60)
    W, H = 72, 40
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_SIMPLE, camera=_camera(s, SKY)), spp=2)
    acc, fb = read_frame(r, W, H, aovs=False)
    st = _check(r, acc, fb, dict(low_percentile=0.0, high_percentile=1.0), None, 0.0, "sky")
    r.close()
    used = np.flatnonzero(st["histogram"])
    print("sky: bins", used.tolist(), "counts", st["histogram"][used].tolist())
    assert st["counted"] == W * H and st["black"] == 0 and st["ignored"] == 0
    # a clear sky away from the sun spans well under five octaves (a factor of 30) over a patch of this size: 40 bins of the 255, and
    # far fewer within one wave's 64 consecutive pixels
    top = np.sort(st["histogram"])[::-1]
    assert int(np.searchsorted(np.cumsum(top), 0.99 * W * H)) + 1 <= 40, used
    b, _ = A.bins(acc)
    waves = b.reshape(-1)[:(W * H // 64) * 64].reshape(-1, 64)
    per_wave = [len(np.unique(w)) for w in waves]
    print("sky: distinct bins per wave, min %d max %d" % (min(per_wave), max(per_wave)))
    assert max(per_wave) <= 16                                                         # 64 neighbouring sky pixels: within two octaves


def _alternating(r, s, W, H, n=6, call=True, **kw):
    """n 1-spp frames whose camera alternates between ground and sky, each followed by a call -> per frame (src, fb, state, image)"""
    out = []
    for k in range(n):
        r.render(config(s, abi.VARIANT_SIMPLE, camera=_camera(s, SKY if k & 1 else None)), spp=1)
        acc, fb = read_frame(r, W, H, aovs=False)
        if call:
            r.auto_exposure(dt=1 / 60, speed_up=0.5, speed_down=4.0, reset_history=1 if k == 4 else 0, **kw)
            out.append((acc, fb, A.state_of(r.readback_exposure_state()), r.readback_exposed()))
        else:
            out.append((acc, fb, None, None))
    return out


def test_adaptation_over_six_frames_equals_the_restatement():
    s = scenes.grid(120, 60)
    W, H = 72, 40
    r = renderer(s, W, H)
    frames = _alternating(r, s, W, H)
    r.close()
    prev, evs = None, []
    for k, (acc, fb, got, img) in enumerate(frames):
        p = dict(dt=1 / 60, speed_up=0.5, speed_down=4.0, reset_history=1 if k == 4 else 0)
        want = A.step(acc, p, prev)
        bad = A.same_state(got, want)
        print("frame %d: ev %.6f target %.6f calls %d %s" % (k, got["ev"], got["target_ev"], got["calls"], bad))
        assert not bad, (k, bad)
        assert np.array_equal(img, A.expose(acc, fb, want["scale"]))
        evs.append((float(got["ev"]), float(got["target_ev"]), got["calls"]))
        prev = want
    assert evs[0][0] == evs[0][1] and evs[0][2] == 1                                   # no state: jumps
    assert evs[4][0] == evs[4][1] and evs[4][2] == 1                                   # reset_history on frame 4: jumps
    for k in (1, 2, 3, 5):
        lo, hi = sorted((evs[k - 1][0], evs[k][1]))
        assert lo < evs[k][0] < hi, (k, evs)                                           # in between: rate-limited
    assert [e[2] for e in evs] == [1, 2, 3, 4, 1, 2]
    assert abs(evs[0][1] - evs[1][1]) > 1.0                                            # ground and sky are more than a stop apart
    # the two directions at their own rates: a falling EV (towards the sky's) covers 1 - exp(-4 / 60), a rising one 1 - exp(-0.5 / 60)
    step = lambda k: (evs[k][0] - evs[k - 1][0]) / (evs[k][1] - evs[k - 1][0])
    down, up = (1, 2) if evs[1][1] < evs[0][0] else (2, 1)
    assert abs(step(down) - (1 - np.exp(-4 / 60))) < 1e-4 and abs(step(up) - (1 - np.exp(-0.5 / 60))) < 1e-4, (step(down), step(up))


@pytest.mark.parametrize("name,make,variant,W,H", PARITY, ids=[c[0] for c in PARITY])
def test_metering_means_what_it_says(name, make, variant, W, H):
    """percentiles (0, 1), the clamp out of the way: mean_log2 is the mean of log2(luminance) over the counted pixels up to the bin width,
    |difference| < log2(1 + 1/16) < 0.0875 (every pixel lies that close to its bin's representative), and ev = float(log2(key) - mean)"""
    s = make()
    r = renderer(s, W, H)
    r.render(config(s, variant), spp=2)
    acc, _ = read_frame(r, W, H, aovs=False)
    r.auto_exposure(low_percentile=0.0, high_percentile=1.0, min_ev=-30.0, max_ev=30.0, key=0.25)
    st = A.state_of(r.readback_exposure_state())
    r.close()
    lum = A.luminance(acc)
    b, ign = A.bins(acc)
    counted = ~ign & (b >= 1)
    assert st["counted"] == int(counted.sum()) > 0 and int(b[counted].max()) < 255
    mean = float(np.mean(np.log2(lum[counted].astype(np.float64))))
    print("%s: mean log2 luminance %.6f, metered %.6f, difference %.6f" % (name, mean, st["mean_log2"], st["mean_log2"] - mean))
    assert abs(mean - float(st["mean_log2"])) < 0.0875
    m, _ = A.percentile_mean(st["histogram"], 0.0, 1.0)
    assert st["ev"] == st["target_ev"] == F(np.log2(np.float64(F(0.25))) - m) and st["mean_log2"] == F(m)


def test_manual_mode_on_the_denoised_image_is_the_denoisers_rgba8():
    """the anchor to shipped code: mode 0, source 1, gains 1, tone_mapping_mode = early_tone_mapping_mode"""
    s = scenes.cornell32()
    W, H = 37, 21
    r = renderer(s, W, H)
    r.render(config(s, abi.VARIANT_GLTF), spp=2)
    for tm, exposure in ((-1, 0.0), (1, 1.5), (2, -0.75)):
        r.params.early_tone_mapping_mode = tm
        r.params.exposure = exposure
        r.denoise(iterations=3)
        want = r.readback_denoised_u8()
        r.auto_exposure(mode=0, source=1, tone_mapping_mode=tm)
        got = r.readback_exposed()
        assert np.array_equal(got, want), (tm, int(np.count_nonzero(got != want)))
    r.denoise_temporal(iterations=2)                                                   # "whichever denoise call ran last"
    want = r.readback_denoised_u8()
    r.auto_exposure(mode=0, source=1, tone_mapping_mode=2)
    assert np.array_equal(r.readback_exposed(), want)
    r.params.output_channel = 2                                                        # an AOV view: the frame's RGBA8, nothing metered
    r.auto_exposure(mode=1)
    assert np.array_equal(r.readback_exposed(), read_frame(r, W, H, aovs=False)[1])
    with pytest.raises(backend.BackendError):
        r.readback_exposure_state()
    r.close()


def _everything(r, W, H):
    return read_frame(r, W, H) + (r.readback_denoised_f32(), r.readback_denoised_u8(), r.readback_denoise_history(), r.readback_upscaled())


def _run(s, W, H, call_after):
    """four 1-spp frames, each denoised (temporal) and upscaled; call_after: frames after which auto_exposure runs (both sources)"""
    r = renderer(s, W, H)
    out = []
    for k in range(4):
        r.render(config(s, abi.VARIANT_GLTF, reset=k == 0), spp=1)
        r.denoise_temporal(iterations=2, reset_history=1 if k == 0 else 0)
        r.taa_upscale(reset_history=1 if k == 0 else 0)
        before = _everything(r, W, H)
        if k in call_after:
            st0 = bytes(raw_stats(r))
            for source in (0, 1):
                r.auto_exposure(source=source, dt=1 / 60, white_balance=(1.1, 1.0, 0.9), tone_mapping_mode=1)
                assert r.readback_exposed().any() and r.readback_exposure_state().calls == (k - call_after[0]) * 2 + source + 1
            assert bytes(raw_stats(r)) == st0, k
            assert same_images(before, _everything(r, W, H)), k
        out.append(before)
    r.close()
    return out


def test_the_call_leaves_everything_else_alone():
    """the frame's five read-backs, the denoised images, the denoise history, the upscaler's output and the statistics are what they
    were, and the frames rendered, denoised and upscaled after the calls are bit-identical to a run without them"""
    s = scenes.cornell32()
    W, H = 40, 24
    plain = _run(s, W, H, ())
    with_calls = _run(s, W, H, (1, 2))
    for k in range(4):
        assert same_images(plain[k], with_calls[k]), k


def test_frames_in_flight_equal_the_synchronous_run():
    s = scenes.grid(120, 60)
    W, H = 72, 40
    r = renderer(s, W, H)
    want = _alternating(r, s, W, H, n=3, tone_mapping_mode=2)
    r.close()
    r = renderer(s, W, H, frames_in_flight=3)
    tickets = [r.render_async(config(s, abi.VARIANT_SIMPLE, camera=_camera(s, SKY if k & 1 else None)), spp=1) for k in range(3)]
    for k, t in enumerate(tickets):
        r.wait(t)
        r.auto_exposure(dt=1 / 60, speed_up=0.5, speed_down=4.0, tone_mapping_mode=2)
        got = A.state_of(r.readback_exposure_state())
        assert not A.same_state(got, want[k][2]), k
        assert np.array_equal(r.readback_exposed(), want[k][3]), k
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
    _refused(r.auto_exposure, INV, "before a frame")
    _refused(r.readback_exposed, INV, "rptr_hip_auto_exposure first")
    _refused(r.readback_exposure_state, INV, "mode 1 first")
    assert L.rptr_hip_auto_exposure(None, C.byref(abi.AutoExposureParams())) == INV
    r.render(cfg, spp=1)
    _refused(r.readback_exposed, INV, "rptr_hip_auto_exposure first")               # a frame, but no call
    nan, inf = float("nan"), float("inf")
    for bad, fragment in ((dict(source=2), "source"), (dict(source=-1), "source"), (dict(mode=2), "mode"), (dict(reset_history=2), "reset_history"),
                          (dict(tone_mapping_mode=3), "tone_mapping_mode"), (dict(tone_mapping_mode=-2), "tone_mapping_mode"),
                          (dict(key=0.0), "key"), (dict(key=nan), "key"), (dict(key=inf), "key"),
                          (dict(low_percentile=-0.1), "percentiles"), (dict(low_percentile=1.0, high_percentile=1.0), "percentiles"),
                          (dict(low_percentile=0.5, high_percentile=0.5), "percentiles"), (dict(high_percentile=1.5), "percentiles"), (dict(high_percentile=nan), "percentiles"),
                          (dict(min_ev=2.0, max_ev=1.0), "min_ev"), (dict(min_ev=-inf), "min_ev"), (dict(max_ev=nan), "min_ev"),
                          (dict(speed_up=-1.0), "speed_up"), (dict(speed_down=inf), "speed_up"), (dict(speed_down=nan), "speed_up"),
                          (dict(dt=-1.0), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
                          (dict(white_balance=(1.0, 0.0, 1.0)), "white_balance"), (dict(white_balance=(1.0, 1.0, nan)), "white_balance"),
                          (dict(white_balance=(inf, 1.0, 1.0)), "white_balance")):
        _refused(lambda: r.auto_exposure(**bad), INV, fragment)
    p = abi.AutoExposureParams()
    L.rptr_hip_auto_exposure_defaults(C.byref(p))
    p.reserved = 1
    _refused(lambda: r.auto_exposure(p), INV, "reserved")
    _refused(lambda: r.auto_exposure(source=1), INV, "no denoised image")            # source 1 before any denoise call
    assert L.rptr_hip_auto_exposure(h, None) == 0                                     # NULL: the defaults
    assert r.readback_exposed().shape == (H, W, 4) and r.readback_exposure_state().calls == 1
    buf = np.zeros(8, np.uint8)
    assert L.rptr_hip_readback_exposed_u8(h, buf.ctypes.data_as(C.c_void_p), buf.size) == INV     # too small
    assert L.rptr_hip_readback_exposed_u8(h, None, 0) == INV and L.rptr_hip_readback_exposure_state(h, None) == INV
    r.denoise(iterations=1)
    r.auto_exposure(source=1)
    r.render(cfg, spp=1)                                                            # a later frame: the image and the denoised source are stale
    _refused(r.readback_exposed, INV, "stale")
    _refused(lambda: r.auto_exposure(source=1), INV, "stale")
    assert r.readback_exposure_state().calls == 2                                   # (the state is the adaptation's memory: it stays)
    r.auto_exposure()
    r.readback_exposed()
    r.initialize(W, H)                                                              # initialize: no image, no state, no frame
    _refused(r.readback_exposed, INV, "rptr_hip_auto_exposure first")
    _refused(r.readback_exposure_state, INV, "mode 1 first")
    _refused(r.auto_exposure, INV, "before a frame")
    r.set_scene(s)
    r.render(cfg, spp=1)
    r.auto_exposure(mode=0)
    r.readback_exposed()
    _refused(r.readback_exposure_state, INV, "mode 1 first")                         # manual calls leave no state
    r.params.render_upscale_factor = 2
    _refused(r.auto_exposure, UNS, "render_upscale_factor")
    r.params.render_upscale_factor = 1
    r.auto_exposure()
    assert r.readback_exposure_state().calls == 1
    r.close()
    r = renderer(s, W, H, options={"aovs": 0})
    r.render(cfg, spp=1)
    _refused(lambda: r.auto_exposure(source=1), UNS, '"aovs" is 0')
    r.auto_exposure(source=0)                                                       # source 0 needs no AOV image
    assert r.readback_exposure_state().counted > 0
    r.close()
    r = renderer(s, W, H, rank=0, world_size=2, stripe_rows=8)
    r.render(cfg, spp=1)
    _refused(r.auto_exposure, UNS, "world_size")
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                        # the waited frame's context is being rendered to again
    t0 = r.render_async(cfg, spp=1)
    r.wait(t0)
    t1 = r.render_async(cfg, spp=1)
    t2 = r.render_async(cfg, spp=1)
    _refused(r.auto_exposure, INV, "overwritten")
    r.wait(t1)
    r.wait(t2)
    r.auto_exposure()
    r.close()
    r = renderer(s, W, H, frames_in_flight=2)                                        # a frame of a launch sequence other than its last
    tickets = r.render_batch_async(cfg, spp=1, n_frames=2)
    r.wait(tickets[0])
    _refused(r.auto_exposure, INV, "launch sequence")
    r.wait(tickets[1])
    r.auto_exposure()
    r.close()
