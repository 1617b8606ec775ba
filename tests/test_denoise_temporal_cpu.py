"""The temporal denoiser without a GPU: its three entry points in the header, abi.py and the library; the parameter struct and its
defaults; and properties of the numpy restatement (tests/denoise_temporal_ref.py, written from the header of csrc/denoise_temporal.h)
that the GPU tests then hold the kernel to bit for bit."""
import copy
import ctypes as C
import os
import re

import numpy as np

import denoise_ref as D
import denoise_temporal_ref as T
from common import float_bits, synthetic_frame
from realtimepathtracingresearchframework_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rptr_hip_denoise_temporal_defaults", "rptr_hip_denoise_temporal", "rptr_hip_readback_denoise_history_f32"]
F = np.float32


def _motion(H, W, mx=0.0, my=0.0):
    mj = np.zeros((H, W, 4), np.float16)
    mj[..., 0] = mx
    mj[..., 1] = my
    return mj


def _noisy(k, amplitude=0.35):
    """synthetic_frame's layout with fresh noise for frame k -> (accum, albedo, nd, clean)"""
    _, alb, nd, clean = synthetic_frame()
    H, W = clean.shape[:2]
    noise = np.random.RandomState(100 + k).rand(H, W, 3).astype(F) - F(0.5)
    accum = np.empty((H, W, 4), F)
    accum[..., :3] = clean + alb[..., :3].astype(F) * (F(amplitude) * noise)
    accum[..., 3] = 1.0
    return accum, alb, nd, clean


def test_the_three_symbols_are_declared_listed_and_bound():
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    declared = set(re.findall(r"\b(rptr_hip_[a-z0-9_]+)\s*\(", text))
    L = backend.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in abi.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name   # a prototype was declared, not only the symbol found
    for method in ("denoise_temporal", "readback_denoise_history"):
        assert callable(getattr(backend.RenderHip, method))


def test_parameter_struct_defaults_and_pins():
    assert C.sizeof(abi.DenoiseTemporalParams) == 64
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    body = re.search(r"typedef struct RptrDenoiseTemporalParams \{(.*?)\} RptrDenoiseTemporalParams;", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:int32_t|float)\s+(\w+)", body, re.M)
    assert fields == [f[0] for f in abi.DenoiseTemporalParams._fields_]
    assert fields[:5] == [f[0] for f in abi.DenoiseParams._fields_][:5]      # the five spatial parameters lead, in the denoiser's order
    L = backend.load_library()
    for fill in (0x00, 0xFF):
        p = abi.DenoiseTemporalParams()
        C.memset(C.byref(p), fill, C.sizeof(p))
        L.rptr_hip_denoise_temporal_defaults(C.byref(p))
        assert (p.iterations, p.sigma_luminance, p.sigma_depth, p.normal_power_log2, p.demodulate_albedo) == (5, 4.0, 1.0, 7, 1)
        assert (p.alpha_color, p.alpha_moments, p.normal_threshold, p.depth_tolerance) == (F(0.2), F(0.2), F(0.9), F(0.1))
        assert p.reset_history == 0 and list(p.reserved) == [0] * 6
        assert {k: F(getattr(p, k)) for k in T.DEFAULTS} == {k: F(v) for k, v in T.DEFAULTS.items()}
    L.rptr_hip_denoise_temporal_defaults(None)                               # NULL: nothing happens
    L.rptr_hip_option_count.restype = C.c_int
    assert L.rptr_hip_option_count() == 22
    assert abi.ABI_VERSION == 5


def test_the_first_call_and_a_reset_equal_the_spatial_denoiser_bit_for_bit():
    accum, alb, nd, _ = _noisy(0)
    accum2 = _noisy(1)[0]
    fb = np.full(accum.shape, 77, np.uint8)
    mj = _motion(*accum.shape[:2])
    for demod in (0, 1):
        for it in (1, 5):
            td = T.TemporalDenoiser()
            assert td.history() is None
            f, u = td.step(accum, alb, nd, mj, fb, iterations=it, demodulate_albedo=demod)
            wf, wu = D.denoise(accum, alb, nd, fb, iterations=it, demodulate_albedo=demod)
            assert np.array_equal(float_bits(f), float_bits(wf)) and np.array_equal(u, wu), (demod, it)
            assert not td.had_history.any() and np.all(td.history()[..., 3] == 1)
            f, _ = td.step(accum2, alb, nd, mj, iterations=it, demodulate_albedo=demod)       # history: another image ...
            wf, wu = D.denoise(accum2, alb, nd, fb, iterations=it, demodulate_albedo=demod)
            assert td.had_history.all() and not np.array_equal(float_bits(f), float_bits(wf))
            f, u = td.step(accum2, alb, nd, mj, fb, iterations=it, demodulate_albedo=demod, reset_history=1)   # ... a reset: the spatial one
            assert np.array_equal(float_bits(f), float_bits(wf)) and np.array_equal(u, wu), (demod, it)
            assert not td.had_history.any()
            f, _ = td.step(accum, alb, nd, mj, iterations=it, demodulate_albedo=1 - demod)    # other units: no history either
            assert np.array_equal(float_bits(f), float_bits(D.denoise(accum, alb, nd, iterations=it, demodulate_albedo=1 - demod)[0]))
            assert not td.had_history.any()


def test_zero_motion_eight_frames_history_length_and_error():
    """fresh noise per frame, no motion, 5 iterations: n' counts the calls on every pixel, and after 8 calls the error against the clean
    image is below 0.75 x that of the spatial denoiser on the 8th frame"""
    td = T.TemporalDenoiser()
    rmse = lambda img, clean: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - clean) ** 2)))
    for k in range(8):
        accum, alb, nd, clean = _noisy(k)
        out, _ = td.step(accum, alb, nd, _motion(*accum.shape[:2]))
        assert np.all(td.history()[..., 3] == min(k + 1, 255)), k
    spatial, _ = D.denoise(accum, alb, nd)
    e_t, e_s, e_raw = rmse(out, clean), rmse(spatial, clean), rmse(accum, clean)
    print("rmse after 8 calls: temporal %.5f, spatial (frame 8) %.5f, raw %.5f, ratio %.3f" % (e_t, e_s, e_raw, e_t / e_s))
    assert e_t < 0.75 * e_s, (e_t, e_s)


def test_the_history_length_saturates_at_255():
    accum, alb, nd, _ = _noisy(0)
    td = T.TemporalDenoiser()
    td.blend(accum, alb, nd, _motion(*accum.shape[:2]))
    td.he[..., 3] = 254.5
    td.blend(accum, alb, nd, _motion(*accum.shape[:2]))
    assert np.all(td.history()[..., 3] == 255)


def test_an_integer_pan_blends_with_the_texel_four_pixels_away():
    """W = 64 and motion.x = 0.125 (exact in half: 0.5 * 0.125 * 64 = 4 pixels): fx = fy = 0 exactly, so the blended colour at p is the
    blend of e with the previous e' at p + (4, 0), bit for bit; the 4 columns whose taps fall outside the image have n' = 1"""
    H, W = 32, 64
    a0, alb0, nd0, _ = synthetic_frame(H, W)
    shift = lambda img: np.roll(img, -4, axis=1)      # the previous frame's p + (4, 0) is this frame's p
    a1 = shift(synthetic_frame(H, W, amplitude=0.2)[0])
    alb1, nd1 = shift(alb0), shift(nd0)
    td = T.TemporalDenoiser()
    td.blend(a0, alb0, nd0, _motion(H, W))
    prev = td.history()
    ev, _, _, surf = td.blend(a1, alb1, nd1, _motion(H, W, 0.125))
    assert surf.all()
    hist = td.history()
    inside = np.zeros((H, W), bool)
    inside[:, :W - 4] = True
    assert np.all(hist[..., 3][inside] == 2) and np.all(hist[..., 3][~inside] == 1)
    assert np.array_equal(td.had_history, inside)
    e = D.prepare(a1, alb1, nd1)[0][..., :3]
    want = (F(1) - F(0.5)) * shift(prev[..., :3]) + F(0.5) * e            # ac = fmax(1 / 2, 0.2)
    assert np.array_equal(float_bits(hist[..., :3])[inside], float_bits(want)[inside])
    assert np.array_equal(float_bits(hist[..., :3])[~inside], float_bits(e)[~inside])
    assert np.array_equal(float_bits(ev[..., :3]), float_bits(hist[..., :3]))


def test_disocclusion_by_normal_and_by_depth_drops_the_history():
    """a history whose normals are perpendicular on the right half, and one whose depth there is off by more than the tolerance: n' = 1
    there, and whatever colours and moments that part of the history holds, the output is bit-identical"""
    a0, alb, nd, _ = _noisy(0)
    a1 = _noisy(1)[0]
    H, W = a0.shape[:2]
    right = np.zeros((H, W), bool)
    right[:, W // 2:] = True
    for how in ("normal", "depth"):
        td = T.TemporalDenoiser()
        td.step(a0, alb, nd, _motion(H, W))
        if how == "normal":
            td.hndz[right, :3] = (1.0, 0.0, 0.0)
        else:
            td.hndz[right, 3] *= F(1.25)                 # tolerance 0.1 z + gz, gz ~ 0.02
        other = copy.deepcopy(td)
        other.he[right, :3] = 1e6
        other.hm[right] = 1e9
        mj = _motion(H, W, 0.0107, -0.0041)              # fractional taps: pixels left of the edge have taps on it
        out_a, _ = td.step(a1, alb, nd, mj)
        out_b, _ = other.step(a1, alb, nd, mj)
        assert np.array_equal(float_bits(out_a), float_bits(out_b)), how
        assert np.array_equal(float_bits(td.history()), float_bits(other.history())), how
        n = td.history()[..., 3]
        assert np.all(n[:, W // 2 + 1:] == 1), how       # (the column at the edge may find the left half's texels)
        assert np.all(n[2:-2, 2:W // 2 - 2] == 2), how


def test_pixels_that_are_not_surface_come_back_bit_identical_and_are_never_tapped():
    rng = np.random.RandomState(5)
    frames = []
    for k in range(2):
        accum, alb, nd, _ = _noisy(k)
        H, W = accum.shape[:2]
        alb, nd = alb.copy(), nd.copy()
        sky = np.zeros((H, W), bool)
        sky[:7, :] = True
        nd[sky, :3] = 0.0
        nd[sky, 3] = np.inf
        lamp = np.zeros((H, W), bool)
        lamp[12:18, 20:30] = True
        alb[lamp, :3] = 0.0
        accum[lamp, :3] = 15.0
        accum[sky] = (rng.randn(int(sky.sum()), 4) * 1e6).astype(F)
        frames.append((accum, alb, nd))
    off = sky | lamp
    mj = _motion(H, W, 0.0107, 0.0213)
    outs = []
    for variant in range(2):
        td = T.TemporalDenoiser()
        for accum, alb, nd in frames:
            accum = accum.copy()
            if variant:
                accum[off, :3] = 0.125
            out, _ = td.step(accum, alb, nd, mj)
            assert np.array_equal(float_bits(out)[off], float_bits(accum)[off])
            assert np.all(td.history()[off] == 0) and np.all(td.hm[off] == 0) and np.all(td.hndz[off] == 0)
        assert (td.history()[..., 3] > 1).any()
        outs.append((out, td.history()))
    assert np.array_equal(float_bits(outs[0][0])[~off], float_bits(outs[1][0])[~off])
    assert np.array_equal(float_bits(outs[0][1]), float_bits(outs[1][1]))


def test_an_interleaved_spatial_call_changes_nothing():
    """(for the restatement's API: denoise_ref.denoise shares no state with a TemporalDenoiser; the library's dn.ndz is rewritten by
    rptr_hip_denoise, which is why the history keeps its own copy -- tests/test_gpu_denoise_temporal.py)"""
    runs = []
    for interleave in (False, True):
        td = T.TemporalDenoiser()
        for k in range(3):
            accum, alb, nd, _ = _noisy(k)
            out, _ = td.step(accum, alb, nd, _motion(*accum.shape[:2]), iterations=2)
            if interleave:
                D.denoise(accum, alb, nd, iterations=3, demodulate_albedo=0)
        runs.append((out, td.history()))
    assert np.array_equal(float_bits(runs[0][0]), float_bits(runs[1][0])) and np.array_equal(float_bits(runs[0][1]), float_bits(runs[1][1]))
