"""Builds the exposure probe (exposure_probe.hip) -- TEST INFRASTRUCTURE, not linked into librptr_hip.so.

exposure_probe.hip includes csrc/auto_exposure.h and launches rp_k_meter and rp_k_meter_reduce on a float4 array the caller supplies; it
is compiled with the product's own flags (build.FLAGS): libexposure_probe.so."""
import ctypes as C
import os
import subprocess

import numpy as np

from realtimepathtracingresearchframework_amd import abi
from realtimepathtracingresearchframework_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "exposure_probe.hip")
LIB = "libexposure_probe.so"
DEPENDS = ("auto_exposure.h", "denoise.h", "realtime_resolve.h", "kernels.h", "dshade.h", "dmath.h")
ABI_HEADERS = [os.path.join(os.path.dirname(B.HERE), "include", f) for f in ("rptr_hip.h", "rptr_bvh.h")]
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
        _LIB.ep_meter.restype = C.c_int
        _LIB.ep_meter.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.AutoExposureParams), C.c_float, C.c_int, C.c_int, C.POINTER(abi.ExposureState),
                                  C.POINTER(abi.ExposureState), C.c_void_p]
        _LIB.ep_time_meter.restype = C.c_int
        _LIB.ep_time_meter.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    return _LIB


def params(**fields):
    """the library's defaults (tests/auto_exposure_ref.py DEFAULTS) with single fields replaced"""
    import auto_exposure_ref as A
    p = abi.AutoExposureParams()
    for k, v in dict(A.DEFAULTS, **fields).items():
        if k == "white_balance":
            p.white_balance[:] = [float(g) for g in v]
        else:
            setattr(p, k, v)
    return p


def meter(texels, p, exposure=0.0, blocks=4, combine=False, state_in=None):
    """rp_k_meter<combine> (False: the instantiation the library launches) + rp_k_meter_reduce on an (N, 4) float32 array ->
    (abi.ExposureState, the working histogram afterwards)"""
    texels = np.ascontiguousarray(texels, np.float32).reshape(-1, 4)
    out = abi.ExposureState()
    after = np.full(257, 0xFFFFFFFF, np.uint32)
    rc = load().ep_meter(texels.ctypes.data_as(C.c_void_p), len(texels), C.byref(p), float(exposure), int(blocks), 1 if combine else 0,
                         C.byref(state_in) if state_in is not None else None, C.byref(out), after.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("ep_meter failed (%d)" % rc)
    return out, after


def time_meter(texels, blocks, combine, warmup=20, reps=200):
    """median microseconds of one rp_k_meter launch"""
    texels = np.ascontiguousarray(texels, np.float32).reshape(-1, 4)
    us = C.c_float(0)
    rc = load().ep_time_meter(texels.ctypes.data_as(C.c_void_p), len(texels), int(blocks), 1 if combine else 0, int(warmup), int(reps), C.byref(us))
    if rc != 0:
        raise RuntimeError("ep_time_meter failed (%d)" % rc)
    return float(us.value)
