"""What the tests of the device shading probes share (tests/device_probes/shade_probe.hip through ctypes) -- TEST INFRASTRUCTURE: the loaded
probe libraries, the comparison helpers and the bounds every device test of csrc/dshade.h uses. tests/test_gpu_shade_functions.py lists the
function classes and what each is held to."""
import ctypes as C
import os

import numpy as np

import device_probes as DP

ULP_LIBM = 64          # sample directions / sky / sRGB / anisotropic lookups: device libm vs glibc, amplified through the formulas
SAMPLE_PDF_REL = 1e-3  # sampled pdf / MIS pdf against the oracle's at the same inputs
EXCEPTIONS = 1e-3      # share of samples allowed to take another branch (their oracle value lies at a decision boundary)

_LIBS = {}


def probes(fast):
    if fast not in _LIBS:
        d = os.environ.get("RPTR_SHADE_PROBE_DIR")
        if d:
            path = DP.lib_paths(d)[fast]
        else:
            if DP.needs_build():
                DP.build()
            path = DP.lib_paths()[fast]
        L = C.CDLL(path)
        for name in ("sp_gltf_sample", "sp_gltf_eval", "sp_gltf_t_sample", "sp_gltf_t_eval", "sp_simple", "sp_tri_light", "sp_sample_sun", "sp_sun_pdf",
                     "sp_nee_mis", "sp_sky_radiance", "sp_hit_attributes", "sp_dequantize", "sp_footprint", "sp_texture", "sp_linear_to_srgb", "sp_half4",
                     "sp_tri_lights", "sp_pointset", "sp_randf", "sp_div", "sp_slot_geometry", "sp_slots", "sp_slot_frame"):
            getattr(L, name).restype = C.c_int
        L.sp_sample_sun.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.sp_texture.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.sp_tri_lights.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.sp_pointset.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sp_slot_frame.argtypes = [C.c_int] * 3 + [C.c_uint32] * 3 + [C.c_void_p, C.c_int, C.c_void_p]
        assert L.sp_fast_math() == fast
        _LIBS[fast] = L
    return _LIBS[fast]


def call(fast, name, *args):
    rc = getattr(probes(fast), name)(*args)
    assert rc == 0, "%s returned %d" % (name, rc)


def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulps(a, b):
    """distance in binary32 ulps (monotone integer map; NaN == NaN: 0, NaN vs number: huge)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b)).astype(np.float64)
    na, nb = np.isnan(np.asarray(a, np.float32)), np.isnan(np.asarray(b, np.float32))
    return np.where(na & nb, 0.0, np.where(na | nb, 2.0 ** 40, d))


def dir_ulps(a, b):
    """the distance of two unit vectors in ulps of 1 (2^-24; NaN == NaN: 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b).max(axis=-1) / 2.0 ** -24
    nan_a, nan_b = np.isnan(a).any(axis=-1), np.isnan(b).any(axis=-1)
    return np.where(nan_a & nan_b, 0.0, np.where(nan_a | nan_b, 2.0 ** 40, d))


def line(name, build, ulp_max, rel, nonfinite):
    print("%-40s %-5s max ulp vs oracle %-12s max rel vs float64 %-10s non-finite %d" % (
        name, build, "-" if ulp_max is None else "%d" % ulp_max, "-" if rel is None else "%.2e" % rel, nonfinite))


def nonfinite(*a):
    return int(sum((~np.isfinite(np.asarray(x, np.float32))).sum() for x in a))
