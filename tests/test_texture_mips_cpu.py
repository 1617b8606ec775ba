"""Dynamic textures without a device: the sRGB table the library hands out, the tap table and the arithmetic of the mip filter as
tests/texture_mips_ref.py restates them (include/rptr_hip.h "dynamic textures"), scenes.generate_mips against that restatement, and the
ABI's declarations."""
import os
import re

import numpy as np
import pytest

import texture_mips_ref as TM
from host_tools import ROOT
from realtimepathtracingresearchframework_amd import abi, backend, scenes

f32 = np.float32


@pytest.fixture(scope="module")
def table():
    return backend.srgb_decode_table()


def _random_texture(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def test_the_table_is_the_srgb_decode_to_one_ulp_and_increases(table):
    """The float64 restatement is of the table's own expression (csrc/dshade.h rp_srgb_decode_lut): c = float(i) / 255.0f,
    c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f) -- the float32 operands as the library forms them, the power in float64.
    One ulp is powf's allowance; measured: 0.50 ulp. The IEC 61966-2-1 curve evaluated in float64 from exact operands is another number:
    the three roundings of the base (c, the sum, the quotient: 4 half-ulps of 2^-23 with the two constants) are amplified 2.4 times
    (5.7e-7), 2.4f differs from 2.4 by 9.5e-8 (times |ln base| <= 2.4: 2.3e-7), powf adds 1.2e-7: within 1e-6 relative. Measured: 5.6 ulp,
    6.7e-7. The table is what every frame samples through, so it is not the thing to change."""
    assert table.dtype == f32 and table.shape == (256,)
    i = np.arange(256)
    c = i.astype(f32) / f32(255.0)
    base = (c + f32(0.055)) / f32(1.055)
    assert c.dtype == f32 and base.dtype == f32
    restated = np.where(c <= f32(0.04045), (c / f32(12.92)).astype(np.float64), base.astype(np.float64) ** np.float64(f32(2.4)))
    ulp = np.spacing(table).astype(np.float64)
    err = np.abs(table.astype(np.float64) - restated) / ulp
    exact = TM.srgb_decode64(i)
    rel = np.abs(table.astype(np.float64) - exact)[1:] / exact[1:]
    print("table against its float64 restatement: %.3f ulp at most; against the exact curve: %.3e relative" % (err.max(), rel.max()))
    assert table[0] == 0.0 and table[255] == 1.0
    assert (err <= 1.0).all()
    assert (rel <= 1e-6).all()
    assert (np.diff(table) > 0).all()
    T = TM.thresholds(table)
    assert (np.diff(T[1:]) > 0).all() and T[1] > table[0] and T[255] < table[255]
    assert ((T[1:] > table[:-1]) & (T[1:] < table[1:])).all()    # code k decodes to a value between T[k] and T[k + 1]


def test_tap_weights_sum_to_the_total_and_cover_every_source_texel():
    for n in range(1, 41):
        idx, w, total = TM.axis_taps(n)
        m = max(1, n >> 1)
        assert idx.shape == w.shape and idx.shape[0] == m
        assert total == (1 if n == 1 else 2 if n % 2 == 0 else n)
        assert (w.sum(axis=1) == total).all() and (w > 0).all()
        assert idx.min() == 0 and idx.max() == n - 1
        assert (np.diff(idx, axis=1) == 1).all()                 # neighbouring source texels, left to right
        cover = np.zeros(n, np.int64)
        np.add.at(cover, idx.reshape(-1), w.reshape(-1))
        assert (cover == (1 if n == 1 or n % 2 == 0 else n >> 1)).all(), n   # exact area: every source texel weighs the same


def test_even_sizes_are_the_integer_box_filter(table):
    for h, w in ((2, 2), (4, 6), (16, 8), (2, 64)):
        src = _random_texture(h, w, 10 + h + w)
        s = src.astype(np.int64)
        box = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        assert np.array_equal(TM.level(src, False, table), box.astype(np.uint8))
        assert np.array_equal(TM.level(src, True, table)[..., 3], box[..., 3].astype(np.uint8))   # alpha is linear in an sRGB texture too


@pytest.mark.parametrize("srgb", [False, True])
def test_constant_textures_stay_constant_for_all_codes(table, srgb):
    for code in range(256):
        src = np.full((5, 7, 4), code, np.uint8)
        levels = TM.chain(src, srgb, table)
        assert [l.shape for l in levels] == [(2, 3, 4), (1, 1, 4)]
        assert all((l == code).all() for l in levels), code


@pytest.mark.parametrize("srgb", [False, True])
def test_a_constant_is_exact_at_the_largest_odd_size(table, srgb):
    """n = 16383: the weights reach 8191 and the total 16383, and the quotient still decodes to the code it came from"""
    for code in (0, 1, 2, 37, 127, 128, 200, 254, 255):
        row = np.full((1, 16383, 4), code, np.uint8)
        assert (TM.level(row, srgb, table) == code).all(), code
        assert (TM.level(row.reshape(16383, 1, 4), srgb, table) == code).all(), code


def test_the_search_counts_the_thresholds(table):
    """what the kernel's 8-step search and scenes.generate_mips' searchsorted compute is the count of the definition, ties included"""
    T = TM.thresholds(table)
    probes = np.concatenate([T[1:], np.nextafter(T[1:], f32(0)), np.nextafter(T[1:], f32(2)), table, f32([0.0, 1.0, 0.5])]).astype(f32)
    counted = TM.encode_srgb(probes, T)
    assert np.array_equal(counted, np.searchsorted(T[1:], probes, side="right"))
    code = np.zeros(len(probes), np.int64)
    for step in (128, 64, 32, 16, 8, 4, 2, 1):
        code = np.where(probes >= T[code + step], code + step, code)
    assert np.array_equal(counted, code)
    assert np.array_equal(TM.encode_srgb(table, T), np.arange(256))          # every code survives decode + encode


@pytest.mark.parametrize("srgb", [False, True])
def test_scenes_generate_mips_equals_the_reference(table, srgb):
    for h, w in ((1, 1), (2, 2), (1, 8), (8, 1), (16, 8), (3, 3), (3, 5), (7, 7), (10, 6), (17, 33), (64, 64), (20, 300), (5, 7)):
        src = _random_texture(h, w, 100 + 7 * h + w)
        want = TM.chain(src, srgb, table)
        got = scenes.generate_mips(src, srgb, table)
        assert len(got) == len(want) == TM.full_levels(h, w) - 1
        for l, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (h, w, l + 1)
        tex = scenes.Texture(rgba=src, srgb=srgb).with_generated_mips(table)
        assert len(tex.levels()) == TM.full_levels(h, w) and tex.levels()[0] is not None
        assert all(np.array_equal(a, b) for a, b in zip(tex.levels()[1:], want))


def test_the_abi_declares_the_calls():
    L = backend.load_library()
    for name in ("rptr_hip_update_texture", "rptr_hip_update_texture_device", "rptr_hip_readback_texture", "rptr_hip_texture_levels",
                 "rptr_hip_srgb_decode_table"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.rptr_hip_option_count() == 22
    header = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    assert re.search(r"#define RPTR_HIP_ABI_VERSION 5\b", header) and abi.ABI_VERSION == 5
    assert re.search(r"#define RPTR_TEXTURE_GENERATE_MIPS 1u", header) and abi.TEXTURE_GENERATE_MIPS == 1
    # a call without a handle is refused before anything else is looked at
    assert L.rptr_hip_update_texture(None, 0, None, 0, abi.TEXTURE_GENERATE_MIPS) == abi.RPTR_E_INVALID
    assert L.rptr_hip_readback_texture(None, 0, 0, None, 0) == abi.RPTR_E_INVALID
