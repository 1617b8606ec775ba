"""Auto-exposure without a GPU: its entry points in the header, abi.py and the library; the two structs' layouts and the defaults; and
properties of the numpy restatement (tests/auto_exposure_ref.py, written from the header of csrc/auto_exposure.h) that the GPU tests
then hold the kernels to bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import auto_exposure_ref as A
import denoise_ref as D
from realtimepathtracingresearchframework_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rptr_hip_auto_exposure_defaults", "rptr_hip_auto_exposure", "rptr_hip_readback_exposed_u8", "rptr_hip_readback_exposure_state"]
F = np.float32


def _texels(lum):
    """grey texels of the given luminances, alpha 1 (0.2126 + 0.7152 + 0.0722 rounds back: checked where it matters)"""
    lum = np.asarray(lum, F)
    src = np.zeros(lum.shape + (4,), F)
    src[..., 1] = lum / F(0.7152)
    src[..., 3] = 1.0
    return src


def test_the_entry_points_are_declared_listed_and_bound():
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    declared = set(re.findall(r"\b(rptr_hip_[a-z0-9_]+)\s*\(", text))
    L = backend.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in abi.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for method in ("auto_exposure", "readback_exposed", "readback_exposure_state"):
        assert callable(getattr(backend.RenderHip, method))
    L.rptr_hip_option_count.restype = C.c_int
    assert L.rptr_hip_option_count() == 22
    assert abi.ABI_VERSION == 5 and L.rptr_hip_abi_version() == 5


def test_the_structs_have_one_layout_in_c_and_in_ctypes(tmp_path):
    P, S = abi.AutoExposureParams, abi.ExposureState
    pf, sf = [n for n, _ in P._fields_], [n for n, _ in S._fields_]
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    for name, fields in (("RptrAutoExposureParams", pf), ("RptrExposureState", sf)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decl = [w.strip().split("[")[0] for line in re.findall(r"(?:int32_t|uint32_t|float)\s+([^;]+);", body) for w in line.split(",")]
        assert decl == fields, name
    offs = ["offsetof(RptrAutoExposureParams, %s)" % f for f in pf] + ["offsetof(RptrExposureState, %s)" % f for f in sf]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rptr_hip.h"\nint main(void) {\n    size_t v[] = {sizeof(RptrAutoExposureParams), '
                   'sizeof(RptrExposureState), %s};\n    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);\n    return 0;\n}\n' % ", ".join(offs))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[:2] == [64, 32 + 1024] == [C.sizeof(P), C.sizeof(S)]
    assert got[2:] == [getattr(P, f).offset for f in pf] + [getattr(S, f).offset for f in sf]
    assert P.white_balance.size == 12 and S.histogram.size == 1024 and P.reserved.offset == 60


def test_defaults():
    L = backend.load_library()
    for fill in (0x00, 0xFF):
        p = abi.AutoExposureParams()
        C.memset(C.byref(p), fill, C.sizeof(p))
        L.rptr_hip_auto_exposure_defaults(C.byref(p))
        assert (p.source, p.mode, p.reset_history, p.tone_mapping_mode, p.reserved) == (0, 1, 0, -1, 0)
        assert (p.key, p.low_percentile, p.high_percentile, p.min_ev, p.max_ev) == (F(0.18), F(0.5), F(0.95), -8.0, 8.0)
        assert (p.speed_up, p.speed_down, p.dt, list(p.white_balance)) == (1.0, 3.0, 0.0, [1.0, 1.0, 1.0])
        for k, v in A.DEFAULTS.items():
            got = list(getattr(p, k)) if k == "white_balance" else getattr(p, k)
            assert np.array_equal(F(got), F(v)), k
    assert p.speed_down > p.speed_up     # a falling EV is a brightening scene: the faster direction
    L.rptr_hip_auto_exposure_defaults(None)
    assert L.rptr_hip_auto_exposure(None, None) == abi.RPTR_E_INVALID


def test_the_binning_rule_at_its_edges():
    tiny = np.finfo(F).tiny
    edge = F(2.0 ** -16)
    cases = [(0.0, 0), (-0.0, 0), (float(np.nextafter(F(0), F(1))), 0), (float(tiny) / 2, 0), (float(np.nextafter(edge, F(0))), 0), (float(edge), 1),
             (0.18, 108), (1.0, 129), (float(np.nextafter(F(1), F(0))), 128), (3e38, 255), (57344.0, 255), (float(np.nextafter(F(57344.0), F(0))), 254)]   # (bin 255 starts at 2^15 x 1.75)
    lum = np.array([c[0] for c in cases], F)
    src = np.zeros((len(cases), 4), F)
    src[:, 0] = src[:, 1] = src[:, 2] = lum        # (0.2126 l + 0.7152 l) + 0.0722 l
    src[:, 3] = 1
    b, ign = A.bins(src)
    got_lum = A.luminance(src)
    for k, (_, want) in enumerate(cases):
        if got_lum[k] == lum[k]:                   # (the weights add up to 1 only approximately: test the rule on the luminance it saw)
            assert b[k] == want and not ign[k], (cases[k], int(b[k]))
    assert (got_lum == lum).sum() >= 8
    # ... and directly on luminances (green alone, lum = 0.7152 g, is hard to aim): the rule is a function of the float's bits
    direct = lambda v: int(np.clip(int(np.abs(F(v)).view(np.uint32) >> 20) - 887, 0, 255))
    for v, want in cases:
        assert direct(v) == want, (v, want)
    bad = np.array([[np.nan, 0, 0, 1], [-1, -1, -1, 1], [np.inf, 0, 0, 1], [0.5, 0.5, 0.5, -1.0], [3e38, 3e38, 3e38, 1], [0.5, 0.5, 0.5, np.nan]], F)
    _, ign = A.bins(bad)
    assert list(ign) == [True, True, True, True, False, False]     # (the weights add up to 1: 3e38 stays finite, bin 255; a NaN alpha is not < 0)
    hist, counted, black, ignored = A.meter(np.concatenate([src, bad]))
    assert counted + black + ignored == len(src) + len(bad) and ignored == 4 and int(hist.sum()) == counted + black


def test_every_counted_luminance_lies_within_the_bound_of_its_representative():
    rng = np.random.default_rng(7)
    lum = np.exp2(rng.uniform(-16, 15.75, 200000)).astype(F)
    b = np.clip((lum.view(np.uint32) >> 20).astype(np.int64) - 887, 0, 255)
    keep = (b >= 1) & (b <= 254)
    v = np.array([A.representative(int(k)) for k in range(1, 255)])
    err = np.abs(np.log2(lum[keep].astype(np.float64)) - v[b[keep] - 1])
    print("largest |log2 lum - v_b| = %.6f over %d samples, bins %d..%d" % (err.max(), keep.sum(), b[keep].min(), b[keep].max()))
    assert b[keep].min() == 1 and b[keep].max() == 254
    assert err.max() < 0.0875
    assert abs(float(np.mean(np.log2(lum[keep].astype(np.float64)) - v[b[keep] - 1]))) < 0.005   # the log midpoint: no bias on log-uniform data


def _sorted_mean(hist, low, high):
    """the percentile walk restated with a sort: the representatives of all counted samples ascending, the slice [lo, hi)"""
    v = np.concatenate([np.full(int(hist[b]), A.representative(b)) for b in range(1, 256)]) if hist[1:].sum() else np.zeros(0)
    n = len(v)
    lo, hi = int(float(F(low)) * float(n)), int(float(F(high)) * float(n))
    return (float(np.mean(v[lo:hi])) if hi > lo else None), max(hi - lo, 0)


def test_the_percentile_walk_equals_a_sort():
    rng = np.random.default_rng(11)
    for trial in range(40):
        hist = np.zeros(256, np.uint32)
        k = int(rng.integers(1, 40))
        hist[rng.integers(0, 256, k)] = rng.integers(1, 500, k)
        for low, high in ((0.5, 0.95), (0.0, 1.0), (0.25, 0.26), (0.9, 1.0), (0.0, 1e-6)):
            m, N = A.percentile_mean(hist, low, high)
            ms, Ns = _sorted_mean(hist, low, high)
            assert N == Ns, (trial, low, high)
            assert (m is None) == (ms is None) and (m is None or abs(m - ms) < 1e-9), (trial, low, high, m, ms)
    one = np.zeros(256, np.uint32)
    one[100] = 3
    assert A.percentile_mean(one, 0.4, 0.5) == (None, 0)              # lo = hi = 1: nothing between the percentiles
    black = np.zeros(256, np.uint32)
    black[0] = 1000
    assert A.percentile_mean(black, 0.0, 1.0) == (None, 0)
    p = dict(A.DEFAULTS)
    assert A.target_ev(black, p, None) == (F(0), F(0)) and A.target_ev(black, p, F(1.5)) == (F(1.5), F(0))   # a black frame keeps the ev
    st = A.step(np.zeros((4, 5, 4), F), {}, None)
    assert (st["counted"], st["black"], st["ignored"], st["calls"]) == (0, 20, 0, 1) and st["ev"] == 0 and st["scale"] == 1


def test_the_adapt_rule():
    p = dict(A.DEFAULTS, dt=1 / 60, speed_up=0.5, speed_down=4.0)
    up, down = A.adapt(F(0), F(2), p), A.adapt(F(0), F(-2), p)
    assert float(up) == float(F(2 * (1 - math.exp(-float(F(1 / 60)) * 0.5))))         # target above: speed_up
    assert float(down) == float(F(-2 * (1 - math.exp(-float(F(1 / 60)) * 4.0))))      # target below: speed_down
    assert 0 < up < -down < 2
    assert A.adapt(F(1.25), F(1.25), p) == F(1.25)                                     # the fixed point
    assert A.adapt(F(0), F(2), dict(p, dt=0.0)) == F(2)                                # dt = 0 jumps
    assert A.adapt(F(0), F(2), dict(p, reset_history=1)) == F(2)
    assert A.adapt(None, F(2), p) == F(2)                                              # no state: nothing to adapt from
    assert A.adapt(F(0), F(2), dict(p, speed_up=0.0)) == F(0)                          # rate 0 holds
    ev = F(0)
    for _ in range(2000):
        ev = A.adapt(ev, F(2), p)
    assert abs(float(ev) - 2) < 1e-4                                                   # ... and converges
    # a metered sequence: bright, then dark, then reset
    bright, dark = _texels(np.full((8, 8), 4.0)), _texels(np.full((8, 8), 0.01))
    s0 = A.step(bright, p, None)
    s1 = A.step(dark, p, s0)
    s2 = A.step(dark, dict(p, reset_history=1), s1)
    assert s0["ev"] == s0["target_ev"] and s0["calls"] == 1
    assert s0["ev"] < s1["ev"] < s1["target_ev"] and s1["calls"] == 2                  # darker scene: the ev rises, at speed_up
    assert s2["ev"] == s2["target_ev"] == s1["target_ev"] and s2["calls"] == 1
    assert abs(float(s0["mean_log2"]) - 2) < 0.0875 and s0["scale"] == F(np.exp2(np.float64(s0["ev"])))


def test_the_display_image():
    rng = np.random.default_rng(3)
    src = np.exp2(rng.uniform(-6, 3, (12, 16, 4))).astype(F)
    src[..., 3] = 1
    src[0, 0, 3] = -1.0                     # keeps the frame's texel
    src[0, 1, 3] = 0.25
    src[0, 2, :3] = (-0.5, np.nan, np.inf)
    fb = rng.integers(0, 256, (12, 16, 4)).astype(np.uint8)
    for mode in (-1, 0, 1, 2):
        for exposure in (0.0, 1.5, -0.75):
            scale = A.scale_of(exposure, 0.0)
            got = A.expose(src, fb, scale, mode)
            # manual mode equals the denoiser's RGBA8 rule for the same colour
            _, want = D.denoise(src, np.zeros((12, 16, 4), np.float16), np.zeros((12, 16, 4), np.float16), fb, iterations=1, exposure=exposure, tone_mapping_mode=mode)
            assert np.array_equal(got, want), (mode, exposure)
            # gains of exactly 1 leave the bytes alone; M2 M1 in fp32 would not
            assert np.array_equal(A.expose(src, fb, scale, mode, (1.0, 1.0, 1.0)), got)
    assert np.array_equal(got[0, 0], fb[0, 0]) and got[0, 1, 3] == 64
    warm = A.expose(src, fb, F(1), -1, (1.2, 1.0, 0.8))
    assert not np.array_equal(warm, A.expose(src, fb, F(1), -1))
    x = src[3:, :, :3]
    l = np.stack([A._row(A.M1[k], x) for k in range(3)], -1)
    back = np.stack([A._row(A.M2[k], l) for k in range(3)], -1)
    # the published pair carries six digits: M2 M1 = I up to 2 x 5e-6 x (largest row sum of |M2|, 4.5) x (of |M1|, 1.1) < 1e-4 of the
    # pixel's largest component -- close, and not the identity to the bit
    assert not np.array_equal(back, x) and (np.abs(back - x) <= 1e-4 * np.abs(x).max(axis=-1, keepdims=True)).all()
    lum = lambda im: im[3:, :, :3].astype(np.float64).mean(axis=(0, 1))
    assert lum(warm)[0] > lum(A.expose(src, fb, F(1), -1))[0] and lum(warm)[2] < lum(A.expose(src, fb, F(1), -1))[2]


def test_the_python_mirror_refuses_unknown_fields():
    class Stub(backend.RenderHip):
        def __init__(self):
            self._L = backend.load_library()
    r = Stub()
    for bad in (dict(reserved=1), dict(exposure=1.0), dict(speed=2.0)):
        with pytest.raises(TypeError):
            r.auto_exposure(**bad)
