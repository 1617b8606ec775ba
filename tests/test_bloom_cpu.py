"""Bloom without a GPU: its entry points in the header, abi.py and the library; the struct's layout and the defaults; the kernels' scratch
use from the code object; and properties of the numpy restatement (tests/bloom_ref.py, written from the header of csrc/bloom.h), checked
against a float64 restatement, that the GPU tests then hold the kernels to bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import auto_exposure_ref as A
import bloom_ref as R
import code_object
from realtimepathtracingresearchframework_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rptr_hip_bloom_defaults", "rptr_hip_bloom", "rptr_hip_readback_bloomed_u8", "rptr_hip_bloom_levels", "rptr_hip_readback_bloom_level_f32"]
F = np.float32
EPS = float(np.finfo(F).eps) / 2      # the unit roundoff of binary32, 2^-24: a rounded result is within (1 + EPS) of the exact one


def test_the_entry_points_are_declared_listed_and_bound():
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    declared = set(re.findall(r"\b(rptr_hip_[a-z0-9_]+)\s*\(", text))
    L = backend.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in abi.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for method in ("bloom", "readback_bloomed", "bloom_level", "bloom_levels"):
        assert callable(getattr(backend.RenderHip, method))
    L.rptr_hip_option_count.restype = C.c_int
    assert L.rptr_hip_option_count() == 22
    assert abi.ABI_VERSION == 5 and L.rptr_hip_abi_version() == 5
    assert "#define RPTR_BLOOM_MAX_LEVELS 12" in text and abi.BLOOM_MAX_LEVELS == R.MAX_LEVELS == 12


def test_the_struct_has_one_layout_in_c_and_in_ctypes(tmp_path):
    P = abi.BloomParams
    assert C.sizeof(P) == 64
    pf = [n for n, _ in P._fields_]
    text = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    body = re.search(r"typedef struct RptrBloomParams \{(.*?)\} RptrBloomParams;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [w.strip().split("[")[0] for line in re.findall(r"(?:int32_t|uint32_t|float)\s+([^;]+);", body) for w in line.split(",")]
    assert decl == pf
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rptr_hip.h"\nint main(void) {\n    size_t v[] = {sizeof(RptrBloomParams), %s};\n'
                   '    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);\n    return 0;\n}\n'
                   % ", ".join("offsetof(RptrBloomParams, %s)" % f for f in pf))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == 64 and got[1:] == [getattr(P, f).offset for f in pf]
    assert P.white_balance.size == 12 and P.reserved.size == 16 and P.reserved.offset == 48


def test_defaults():
    L = backend.load_library()
    for fill in (0x00, 0xFF):
        p = abi.BloomParams()
        C.memset(C.byref(p), fill, C.sizeof(p))
        L.rptr_hip_bloom_defaults(C.byref(p))
        assert (p.source, p.exposure_mode, p.tone_mapping_mode, p.levels, list(p.reserved)) == (0, 0, -1, 0, [0, 0, 0, 0])
        assert (p.threshold, p.knee, p.clamp, p.intensity, p.scatter) == (1.0, 0.5, 16.0, F(0.2), F(0.7))
        for k, v in R.DEFAULTS.items():
            got = list(getattr(p, k)) if k == "white_balance" else getattr(p, k)
            assert np.array_equal(F(got), F(v)), k
    L.rptr_hip_bloom_defaults(None)
    assert L.rptr_hip_bloom(None, None) == abi.RPTR_E_INVALID
    n = C.c_uint32(7)
    assert L.rptr_hip_bloom_levels(None, C.byref(n)) == abi.RPTR_E_INVALID


def test_the_bloom_kernels_use_no_scratch():
    regs = code_object.kernel_regs()
    mine = {k: v for k, v in regs.items() if "rp_k_bloom" in k}
    for k, (vgpr, sgpr, scratch, lds) in sorted(mine.items()):
        print("%-60s vgpr %3d sgpr %3d scratch %d lds %d" % (k, vgpr, sgpr, scratch, lds))
        assert scratch == 0, k
    for name in ("rp_k_bloom_down", "rp_k_bloom_up", "rp_k_bloom_composite"):       # what every form of the call launches
        assert any(name in k for k in mine), name
    assert any("rp_k_bloom_down1_tile" in k for k in mine) or any("rp_k_bloom_downILb1" in k for k in mine)   # one form of level 1
    tile = [v for k, v in mine.items() if "rp_k_bloom_down1_tile" in k]
    if tile:
        assert tile[0][3] == 3 * 34 * 35 * 4                                         # three planes of 34 x (34 + 1) floats
    assert [v for k, v in regs.items() if "rp_k_expose" in k][0][2] == 0


def test_the_python_mirror_refuses_unknown_fields():
    class Stub(backend.RenderHip):
        def __init__(self):
            self._L = backend.load_library()
    r = Stub()
    for bad in (dict(reserved=1), dict(exposure=1.0), dict(mode=1), dict(radius=2.0)):
        with pytest.raises(TypeError):
            r.bloom(**bad)


def test_level_sizes_and_counts():
    assert R.sizes(37, 21) == [(37, 21), (19, 11), (10, 6), (5, 3), (3, 2), (2, 1), (1, 1)]
    assert R.level_count(37, 21, 0) == 4 and R.level_count(37, 21, 12) == 6 and R.level_count(37, 21, 1) == 1 and R.level_count(37, 21, 6) == 6
    assert R.level_count(1920, 1080, 0) == 8 and R.sizes(1920, 1080)[8] == (8, 5) and R.level_count(1920, 1080, 12) == 11
    assert R.level_count(1, 1, 0) == 1 and R.level_count(1, 7, 0) == 1 and R.level_count(7, 1, 5) == 3 and R.level_count(2, 2, 0) == 1
    assert R.level_count(16384, 16384, 0) == 8 and R.level_count(16384, 16384, 12) == 12     # L_max = 14: the asked-for 12 stands


# ---- float64 restatements: the same taps and weights (all of them exact in binary), no rounding in between
def _down64(img):
    img = np.asarray(img, np.float64)[..., :3]
    h, w = img.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    wt = (0.125, 0.375, 0.375, 0.125)
    out = np.zeros((dh, dw, 3))
    for j in range(4):
        ys = np.clip(2 * np.arange(dh) - 1 + j, 0, h - 1)
        for i in range(4):
            xs = np.clip(2 * np.arange(dw) - 1 + i, 0, w - 1)
            out += wt[j] * wt[i] * img[ys][:, xs]
    return out


def _up64(u, w, h):
    u = np.asarray(u, np.float64)[..., :3]
    ch, cw = u.shape[:2]
    x, y = np.arange(w), np.arange(h)
    i0, i1 = np.clip((x - 1) >> 1, 0, cw - 1), np.clip(((x - 1) >> 1) + 1, 0, cw - 1)
    j0, j1 = np.clip((y - 1) >> 1, 0, ch - 1), np.clip(((y - 1) >> 1) + 1, 0, ch - 1)
    a0 = np.where(x & 1, 0.75, 0.25)[None, :, None]
    b0 = np.where(y & 1, 0.75, 0.25)[:, None, None]
    return b0 * (a0 * u[j0][:, i0] + (1 - a0) * u[j0][:, i1]) + (1 - b0) * (a0 * u[j1][:, i0] + (1 - a0) * u[j1][:, i1])


def test_a_constant_image_stays_constant_to_a_few_ulps_per_level():
    """The bound: a row r_j is four products (each rounded, relative EPS; the two by 0.125 are exact) and three sums (each rounded):
    every term passes through one product rounding and two sum roundings, so |r_j - v| <= ((1 + EPS)^3 - 1) v. The column step does the
    same to the r_j: three more. Six roundings on every path from a tap to d: |d - v| <= ((1 + EPS)^6 - 1) v per level, (1 + EPS)^(6 l)
    after l levels (the weights are non-negative and sum to 1, so the errors do not cancel into more than that).
    An up level: B is two products and a sum per axis, four roundings (for a constant u); the product by scatter one, the sum with d
    one: u(l) is within (1 + EPS)^6 of d(l) + scatter u(l+1) evaluated on exact inputs, and its inputs carry their own bounds."""
    v = np.array([3.3, 1.7, 9.1], F)
    src = np.zeros((45, 83, 4), F)
    src[..., :3] = v
    src[..., 3] = 1
    scatter, L = F(0.7), 7
    d, u = R.pyramids(src, 1.0, levels=L, threshold=0.0, knee=0.0, clamp=100.0, scatter=scatter)
    assert len(d) == L == R.level_count(83, 45, L)
    p = R.prefilter(src, 1.0, 0.0, 0.0, 100.0)[0, 0, :3].astype(np.float64)
    assert np.array_equal(p, v.astype(np.float64))                        # T = K = 0: unchanged (b / b = 1)
    want_u = {}
    for l in range(L, 0, -1):
        rel = (1 + EPS) ** (6 * l) - 1
        err = np.abs(d[l][..., :3].astype(np.float64) - p).max(axis=(0, 1))
        print("d(%d): largest |d - v| / v = %.3g (bound %.3g = %.1f ulp)" % (l, (err / p).max(), rel, rel / (2 * EPS)))
        assert (err <= rel * p).all(), l
        assert not d[l][..., 3].any() and np.signbit(d[l][..., 3]).sum() == 0
        # u: the exact value is v * (1 + s + ... + s^(L - l)); its bound (1 + EPS)^(6 l) for d plus six roundings per up step on top
        want_u[l] = p if l == L else p + float(scatter) * want_u[l + 1]
        rel_u = (1 + EPS) ** (6 * L + 6 * (L - l)) - 1
        err_u = np.abs(u[l][..., :3].astype(np.float64) - want_u[l]).max(axis=(0, 1))
        assert (err_u <= rel_u * want_u[l]).all(), l
    assert R.same_bits(u[L], d[L])


def test_an_interior_impulse_keeps_its_mass_down_the_pyramid():
    """a power-of-two image, an impulse whose 4 x 4 footprints never touch the clamped border while the level is larger than 4: every
    source texel is then a tap of two outputs per axis whose weights sum to 1/2 (1/8 + 3/8), so 4 sum d(l+1) = sum d(l). Checked
    against float64: the float32 levels agree with the float64 pyramid to the constant-image bound per texel, and the float64 pyramid
    keeps the mass to 1e-12."""
    W = H = 64
    src = np.zeros((H, W, 4), F)
    src[..., 3] = 1
    src[29, 34, :3] = (5.0, 2.5, 1.25)
    d, _ = R.pyramids(src, 1.0, levels=4, threshold=0.0, knee=0.0, clamp=100.0)
    cur64 = R.prefilter(src, 1.0, 0.0, 0.0, 100.0)[..., :3].astype(np.float64)
    assert cur64.sum() == 8.75
    for l in range(1, 5):
        prev_sum = cur64.sum(axis=(0, 1))
        cur64 = _down64(cur64)
        assert np.abs(4 * cur64.sum(axis=(0, 1)) - prev_sum).max() <= 1e-12 * prev_sum.max(), l         # the border is never reached
        got = d[l][..., :3].astype(np.float64)
        rel = (1 + EPS) ** (6 * l) - 1
        assert (np.abs(got - cur64) <= rel * cur64 + 1e-45).all(), l                                     # non-negative terms: relative per texel
        s32 = got.sum(axis=(0, 1))
        print("level %d: 4^l sum d = %s" % (l, (4.0 ** l * s32).tolist()))
        assert np.abs(4.0 ** l * s32 - np.array([5.0, 2.5, 1.25])).max() <= 4.0 ** l * rel * cur64.sum() * 4
        assert (got[cur64 == 0] == 0).all()
    # with power-of-two values and this footprint the first level is exact: the weights are k / 64
    assert np.array_equal(d[1][..., :3].astype(np.float64), _down64(R.prefilter(src, 1.0, 0.0, 0.0, 100.0)))


def test_the_prefilter():
    rng = np.random.default_rng(2)
    src = np.exp2(rng.uniform(-8, 6, (9, 11, 4))).astype(F)
    src[..., 3] = 1
    C_ = 16.0
    p = R.prefilter(src, 1.0, 0.0, 0.0, C_)
    b = src[..., :3].max(axis=-1)
    low = b <= C_
    assert low.sum() > 20 and (~low).sum() > 5
    assert np.array_equal(p[low][:, :3], src[low][:, :3])                # T = K = 0 passes a texel unchanged up to C ...
    over = p[~low][:, :3].astype(np.float64)
    assert np.abs(over.max(axis=-1) - C_).max() <= 2 * EPS * C_ * 2       # ... and scales a brighter one so that its largest channel is C
    ratio = over / src[~low][:, :3].astype(np.float64)
    assert np.abs(ratio - ratio[:, :1]).max() <= 4 * EPS                  # its hue stays
    # a firefly: 1e6 contributes at most C (two roundings: the quotient, the product)
    fire = np.array([[[1e6, 3e5, 10.0, 1.0]]], F)
    for T, K in ((1.0, 0.5), (0.0, 0.0), (4.0, 4.0)):
        q = R.prefilter(fire, 1.0, T, K, C_)[0, 0]
        assert 0 < q[0] <= C_ * (1 + 2 * EPS) and q[1] < q[0] and q[3] == 0, (T, K, q)
    assert R.prefilter(fire, 2.0 ** 120, 1.0, 0.5, C_)[0, 0].tolist() == [0, 0, 0, 0]     # 1e6 * 2^120 overflows: infinite, dropped
    # the knee: nothing below T - K, the quadratic inside, b - T above T + K, continuous at both ends (float64 restatement)
    T, K = 1.0, 0.5
    g = np.zeros((1, 400, 4), F)
    g[0, :, :3] = np.linspace(0.0, 3.0, 400, dtype=F)[:, None]
    g[..., 3] = 1
    e = R.prefilter(g, 1.0, T, K, C_)[0, :, 0].astype(np.float64)
    x = g[0, :, 0].astype(np.float64)
    q = np.clip(x - (T - K), 0, 2 * K)
    want = np.minimum(np.maximum(q * q / (4 * K + 1e-5), x - T), C_)
    assert np.abs(e - want).max() <= 1e-6 and (e[x <= T - K] == 0).all() and (np.diff(e) >= -1e-7).all()
    assert np.abs(e[x >= T + K] - (x[x >= T + K] - T)).max() <= 1e-5
    # what does not contribute
    bad = np.array([[[np.nan, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, -np.inf, 1], [5, 5, 5, -1.0], [5, 5, 5, -np.inf], [-3, -2, -1, 1], [-0.0, -0.0, -0.0, 1]]], F)
    out = R.prefilter(bad, 1.0, 0.0, 0.0, C_)
    assert not out.any() and not np.signbit(out).any()
    ok = np.array([[[5, -2, 1, np.nan], [5, 5, 5, 7.0], [5, 5, 5, -0.0], [5, 5, 5, 0.25]]], F)    # alpha NaN (fmin gives 1), > 1, -0, in range
    out = R.prefilter(ok, 1.0, 0.0, 0.0, C_)
    assert out[0, :, :3].tolist() == [[5, 0, 1], [5, 5, 5], [5, 5, 5], [5, 5, 5]]


def test_the_upsample_is_the_exact_bilinear_and_the_up_sweep_sums_the_levels():
    rng = np.random.default_rng(4)
    for (cw, ch), (w, h) in (((5, 3), (10, 6)), ((5, 3), (9, 5)), ((1, 1), (2, 1)), ((3, 2), (5, 3)), ((1, 1), (1, 1))):
        u = rng.uniform(0, 4, (ch, cw, 4)).astype(F)
        got = R.upsample(u, w, h).astype(np.float64)
        want = _up64(u, w, h)
        assert np.abs(got - want).max() <= 4 * EPS * 4, (cw, ch)
        # ... which is the sample of the bilinear interpolant at the texel centre ((x + 0.5) / 2 - 0.5), clamped to the edge
        for y in range(h):
            for x in range(w):
                fx, fy = min(max((x + 0.5) / 2 - 0.5, 0), cw - 1), min(max((y + 0.5) / 2 - 0.5, 0), ch - 1)
                x0, y0 = min(int(fx), max(cw - 2, 0)), min(int(fy), max(ch - 2, 0))
                x1, y1 = min(x0 + 1, cw - 1), min(y0 + 1, ch - 1)
                tx, ty = fx - x0, fy - y0
                u64 = u.astype(np.float64)[..., :3]
                bil = (1 - ty) * ((1 - tx) * u64[y0, x0] + tx * u64[y0, x1]) + ty * ((1 - tx) * u64[y1, x0] + tx * u64[y1, x1])
                assert np.abs(want[y, x] - bil).max() <= 1e-12, (x, y, cw, ch)
    src = np.exp2(rng.uniform(-3, 5, (21, 37, 4))).astype(F)
    src[..., 3] = 1
    for scatter in (0.0, 1.0, 0.7):
        d, u = R.pyramids(src, 1.0, levels=6, scatter=scatter)
        assert sorted(d) == [1, 2, 3, 4, 5, 6] and d[6].shape == (1, 1, 4) and d[1].shape == (11, 19, 4)
        if scatter == 0.0:
            assert all(R.same_bits(u[l], d[l]) for l in d)                # nothing of the coarser levels arrives (d + 0 * B = d: B is finite)
    assert R.gain(0.2, 1.0, 6) == F(float(F(0.2)) / 6) and R.gain(0.2, 0.0, 6) == F(0.2) and R.gain(0.5, 0.7, 1) == F(0.5)


def test_intensity_zero_reproduces_auto_exposure():
    rng = np.random.default_rng(3)
    src = np.exp2(rng.uniform(-6, 5, (12, 16, 4))).astype(F)
    src[..., 3] = 1
    src[0, 0, 3] = -1.0
    src[0, 1, 3] = 0.25
    src[0, 2, :3] = (-0.5, np.nan, np.inf)
    fb = rng.integers(0, 256, (12, 16, 4)).astype(np.uint8)
    differs = 0
    for mode in (-1, 1, 2):
        for gains in ((1.0, 1.0, 1.0), (1.2, 1.0, 0.8)):
            for scale in (F(1), A.scale_of(0.75, 0.0)):
                want = A.expose(src, fb, scale, mode, gains)
                _, _, got = R.bloom(src, fb, scale, intensity=0.0, tone_mapping_mode=mode, white_balance=gains)
                assert np.array_equal(got, want), (mode, gains)
                _, _, lit = R.bloom(src, fb, scale, intensity=0.5, tone_mapping_mode=mode, white_balance=gains)
                assert np.array_equal(lit[0, 0], fb[0, 0])              # a texel the display rule leaves at the frame's RGBA8 stays there
                differs += int(np.count_nonzero(lit != want))
    assert differs > 1000
