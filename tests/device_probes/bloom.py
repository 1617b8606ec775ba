"""Builds the bloom probe (bloom_probe.hip) -- TEST INFRASTRUCTURE, not linked into librptr_hip.so.

bloom_probe.hip includes csrc/bloom.h and runs its launch sequence on a float image and an RGBA8 image the caller supplies, with either
form of level 1 and of the chain; it is compiled with the product's own flags (build.FLAGS): libbloom_probe.so."""
import ctypes as C
import os
import subprocess

import numpy as np

from realtimepathtracingresearchframework_amd import abi
from realtimepathtracingresearchframework_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "bloom_probe.hip")
LIB = "libbloom_probe.so"
DEPENDS = ("bloom.h", "auto_exposure.h", "denoise.h", "realtime_resolve.h", "kernels.h", "dshade.h", "dmath.h")
ABI_HEADERS = [os.path.join(os.path.dirname(B.HERE), "include", f) for f in ("rptr_hip.h", "rptr_bvh.h")]
STAGE_LEVEL1, STAGE_CHAIN, STAGE_COMPOSITE, STAGE_ALL, STAGE_EXPOSE_ALONE = 1, 2, 4, 7, 8
_LIB = None


def lib_path(out_dir=HERE):
    return os.path.join(out_dir, LIB)


def needs_build(out_dir=HERE, csrc_dir=B.CSRC):
    newest = max(os.path.getmtime(p) for p in [SOURCE] + ABI_HEADERS + [os.path.join(csrc_dir, f) for f in DEPENDS])
    path = lib_path(out_dir)
    return not os.path.exists(path) or os.path.getmtime(path) < newest


def build(out_dir=HERE, csrc_dir=B.CSRC, verbose=False):
    """hipcc the probe library into out_dir; returns its path"""
    os.makedirs(out_dir, exist_ok=True)
    path = lib_path(out_dir)
    cmd = [B._hipcc()] + B.FLAGS + ["-I" + os.path.abspath(csrc_dir), "-I" + B.CSRC, "-shared", SOURCE, "-o", path]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (path, r.stdout))
    return path


def load():
    global _LIB
    if _LIB is None:
        if needs_build():
            build()
        _LIB = C.CDLL(lib_path())
        _LIB.bp_constants.restype = None
        _LIB.bp_constants.argtypes = [C.POINTER(C.c_int * 6)]
        _LIB.bp_run.restype = C.c_int
        _LIB.bp_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.BloomParams), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _LIB.bp_time.restype = C.c_int
        _LIB.bp_time.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.BloomParams), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.POINTER(C.c_float)]
    return _LIB


def constants():
    """dict(tile, tile_src, tail_texels, max_levels, ship_tile, ship_tail) of csrc/bloom.h"""
    v = (C.c_int * 6)()
    load().bp_constants(C.byref(v))
    return dict(zip(("tile", "tile_src", "tail_texels", "max_levels", "ship_tile", "ship_tail"), [int(x) for x in v]))


def params(**fields):
    """the library's defaults (tests/bloom_ref.py DEFAULTS) with single fields replaced"""
    import bloom_ref as R
    p = abi.BloomParams()
    for k, v in dict(R.DEFAULTS, **fields).items():
        if k == "white_balance":
            p.white_balance[:] = [float(g) for g in v]
        else:
            setattr(p, k, v)
    return p


def run(src, fb, p, scale=1.0, from_state=False, tile=True, tail=True, max_blocks=2048):
    """the bloom pass on an (H, W, 4) float32 image and an (H, W, 4) uint8 image -> (d, u, image, tail_start): d and u are dicts
    level -> (h_l, w_l, 4) float32; tail_start is the first level rp_k_bloom_tail ran (L + 1: none)"""
    src = np.ascontiguousarray(src, np.float32)
    fb = np.ascontiguousarray(fb, np.uint8)
    H, W = src.shape[:2]
    assert src.shape == (H, W, 4) and fb.shape == (H, W, 4)
    sizes = []
    w, h = W, H
    for _ in range(abi.BLOOM_MAX_LEVELS):
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append((w, h))
    room = sum(a * b for a, b in sizes)
    d_flat, u_flat = np.zeros((room, 4), np.float32), np.zeros((room, 4), np.float32)
    image = np.zeros((H, W, 4), np.uint8)
    L, t0 = C.c_int(0), C.c_int(0)
    rc = load().bp_run(src.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p), W, H, C.byref(p), float(scale), 1 if from_state else 0, 1 if tile else 0,
                       1 if tail else 0, int(max_blocks), C.byref(L), C.byref(t0), d_flat.ctypes.data_as(C.c_void_p), u_flat.ctypes.data_as(C.c_void_p), room,
                       image.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("bp_run failed (%d)" % rc)
    d, u, at = {}, {}, 0
    for l in range(1, L.value + 1):
        w, h = sizes[l - 1]
        d[l] = d_flat[at:at + w * h].reshape(h, w, 4).copy()
        u[l] = u_flat[at:at + w * h].reshape(h, w, 4).copy()
        at += w * h
    return d, u, image, t0.value


def time(src, fb, p, scale=1.0, tile=True, tail=True, max_blocks=2048, stages=STAGE_ALL, warmup=20, reps=200):
    """median microseconds of the stages (STAGE_* above, or-ed; STAGE_EXPOSE_ALONE: rp_k_expose on the same arrays)"""
    src = np.ascontiguousarray(src, np.float32)
    fb = np.ascontiguousarray(fb, np.uint8)
    H, W = src.shape[:2]
    us = C.c_float(0)
    rc = load().bp_time(src.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p), W, H, C.byref(p), float(scale), 1 if tile else 0, 1 if tail else 0,
                        int(max_blocks), int(stages), int(warmup), int(reps), C.byref(us))
    if rc != 0:
        raise RuntimeError("bp_time failed (%d)" % rc)
    return float(us.value)
