"""The denoiser without a GPU: its four entry points in the header, abi.py and the library; the parameter struct and its defaults; and
properties of the numpy restatement (tests/denoise_ref.py, written from the header of csrc/denoise.h) that the GPU tests then hold the
kernels to bit for bit."""
import ctypes as C
import os
import re

import numpy as np

import denoise_ref as D
from common import float_bits, synthetic_frame
from realtimepathtracingresearchframework_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rptr_hip_denoise_defaults", "rptr_hip_denoise", "rptr_hip_readback_denoised_f32", "rptr_hip_readback_denoised_u8"]
F = np.float32


def test_the_four_symbols_are_declared_listed_and_bound():
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    declared = set(re.findall(r"\b(rptr_hip_[a-z0-9_]+)\s*\(", text))
    L = backend.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in abi.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name   # a prototype was declared, not only the symbol found
    for method in ("denoise", "readback_denoised_f32", "readback_denoised_u8"):
        assert callable(getattr(backend.RenderHip, method))


def test_parameter_struct_defaults_and_option_count():
    assert C.sizeof(abi.DenoiseParams) == 32
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    body = re.search(r"typedef struct RptrDenoiseParams \{(.*?)\} RptrDenoiseParams;", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:int32_t|float)\s+(\w+)", body, re.M)
    assert fields == [f[0] for f in abi.DenoiseParams._fields_]
    L = backend.load_library()
    p = abi.DenoiseParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    L.rptr_hip_denoise_defaults(C.byref(p))
    assert (p.iterations, p.sigma_luminance, p.sigma_depth, p.normal_power_log2, p.demodulate_albedo) == (5, 4.0, 1.0, 7, 1)
    assert list(p.reserved) == [0, 0, 0]
    assert {k: getattr(p, k) for k in D.DEFAULTS} == D.DEFAULTS
    L.rptr_hip_option_count.restype = C.c_int
    assert L.rptr_hip_option_count() == 22
    assert abi.ABI_VERSION == 5


def _flat_frame(H, W, colour, albedo, normal=(0.0, 0.0, 1.0), z=4.0):
    accum = np.empty((H, W, 4), F)
    accum[..., :3] = colour
    accum[..., 3] = 1.0
    alb = np.empty((H, W, 4), np.float16)
    alb[..., :3] = albedo
    alb[..., 3] = 1.0
    nd = np.empty((H, W, 4), np.float16)
    nd[..., :3] = normal
    nd[..., 3] = z
    return accum, alb, nd


def test_a_constant_surface_is_a_fixed_point():
    """a constant image on a flat surface comes back unchanged for 1..5 iterations. (Colour and albedo with short mantissas: every
    product w * e and every partial sum is then exact, so se / sw = e exactly, at the image's edges too where taps are missing.)"""
    accum, alb, nd = _flat_frame(21, 37, (0.5, 0.25, 0.75), (0.5, 0.5, 0.25))
    for it in range(1, 6):
        for demod in (0, 1):
            out, _ = D.denoise(accum, alb, nd, iterations=it, demodulate_albedo=demod)
            assert np.array_equal(float_bits(out), float_bits(accum)), (it, demod)


def test_pixels_that_are_not_surface_come_back_bit_identical():
    """a camera ray that missed stores N = 0 and an infinite depth: those texels (whatever they hold: huge, negative, NaN) are returned
    bit for bit, and never reach a surface pixel's sums"""
    rng = np.random.RandomState(7)
    H, W = 24, 40
    accum, alb, nd = _flat_frame(H, W, (0.5, 0.25, 0.75), (0.5, 0.5, 0.25))
    accum[..., :3] += rng.rand(H, W, 3).astype(F) * F(0.25)
    sky = np.zeros((H, W), bool)
    sky[:9, :] = True
    sky[:, 30:] = True
    nd[sky, :3] = 0.0
    nd[sky, 3] = np.inf
    accum[sky] = (rng.randn(int(sky.sum()), 4) * 1e6).astype(F)
    accum[0, 0] = np.nan
    out, _ = D.denoise(accum, alb, nd, iterations=5)
    assert np.array_equal(float_bits(out)[sky], float_bits(accum)[sky])
    assert not np.array_equal(out[~sky], accum[~sky]) and np.all(np.isfinite(out[~sky]))
    other = accum.copy()
    other[sky] = 1.0
    out2, _ = D.denoise(other, alb, nd, iterations=5)
    assert np.array_equal(float_bits(out)[~sky], float_bits(out2)[~sky])


def test_a_directly_visible_emitter_is_left_alone_and_never_tapped():
    """an emitter stores albedo (0, 0, 0): its texels come back bit for bit, and the surface around it -- same normal, same depth --
    is what it is with any other radiance in the emitter's place (divided by the albedo floor the lamp would otherwise flood it)"""
    rng = np.random.RandomState(3)
    H, W = 24, 40
    accum, alb, nd = _flat_frame(H, W, (0.5, 0.25, 0.75), (0.5, 0.5, 0.25))
    accum[..., :3] += rng.rand(H, W, 3).astype(F) * F(0.25)
    lamp = np.zeros((H, W), bool)
    lamp[8:14, 15:25] = True
    alb[lamp, :3] = 0.0
    accum[lamp, :3] = 15.0
    out, _ = D.denoise(accum, alb, nd, iterations=5)
    assert np.array_equal(float_bits(out)[lamp], float_bits(accum)[lamp])
    other = accum.copy()
    other[lamp, :3] = 0.125
    out2, _ = D.denoise(other, alb, nd, iterations=5)
    assert np.array_equal(float_bits(out)[~lamp], float_bits(out2)[~lamp])
    assert float(out[~lamp][:, :3].max()) < 1.1 and not np.array_equal(out[~lamp], accum[~lamp])


def test_an_edge_between_perpendicular_normals_is_never_crossed():
    """two half-planes with perpendicular normals and normal_power_log2 >= 1: the normal weight across the edge is exactly 0, so
    replacing one side's colours leaves the other side's output bit-identical (the prepare variance only looks at neighbours that face
    the pixel's way, for this reason: csrc/denoise.h)"""
    rng = np.random.RandomState(11)
    H, W = 32, 48
    accum, alb, nd = _flat_frame(H, W, (0.5, 0.5, 0.5), (0.75, 0.5, 0.25))
    accum[..., :3] += rng.rand(H, W, 3).astype(F)
    right = np.zeros((H, W), bool)
    right[:, 23:] = True
    nd[right, :3] = (1.0, 0.0, 0.0)
    other = accum.copy()
    other[right, :3] = rng.rand(int(right.sum()), 3).astype(F) * F(50.0)
    for k in (1, 7):
        for it in (1, 3, 5):
            a, _ = D.denoise(accum, alb, nd, iterations=it, normal_power_log2=k)
            b, _ = D.denoise(other, alb, nd, iterations=it, normal_power_log2=k)
            assert np.array_equal(float_bits(a)[~right], float_bits(b)[~right]), (k, it)
            assert not np.array_equal(a[right], b[right])
            assert not np.array_equal(a[~right], accum[~right])   # ... while the side itself is filtered


def test_every_iteration_lowers_the_error_of_a_noisy_frame():
    """48 x 32, albedo checker x smooth irradiance + hash noise: the RMSE against the noise-free image falls with every iteration 1..3"""
    accum, alb, nd, clean = synthetic_frame()
    rmse = lambda img: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - clean) ** 2)))
    errs = [rmse(accum)] + [rmse(D.denoise(accum, alb, nd, iterations=it)[0]) for it in (1, 2, 3)]
    assert errs[0] > errs[1] > errs[2] > errs[3], errs
    assert errs[3] < 0.5 * errs[0], errs


def test_the_rgba8_image_follows_the_frames_rules():
    """alpha < 0 keeps the frame's texel; output_channel != 0 copies the frame; exposure and both tone-mapping modes change the bytes"""
    accum, alb, nd, _ = synthetic_frame()
    accum[3, 5, 3] = -1.0
    fb = np.full(accum.shape, 77, np.uint8)
    _, u8 = D.denoise(accum, alb, nd, fb, iterations=2)
    assert np.array_equal(u8[3, 5], fb[3, 5]) and not np.any(np.all(u8[4:] == 77, axis=-1))
    assert np.all(u8[4:, :, 3] == 255)
    _, copy = D.denoise(accum, alb, nd, fb, iterations=2, output_channel=2)
    assert np.array_equal(copy, fb)
    seen = {u8.tobytes()}
    for kw in (dict(exposure=1.0), dict(tone_mapping_mode=1), dict(tone_mapping_mode=2)):
        seen.add(D.denoise(accum, alb, nd, fb, iterations=2, **kw)[1].tobytes())
    assert len(seen) == 4
