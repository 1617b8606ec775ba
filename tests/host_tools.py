"""The C++ host programs of host/ built for the tests, once per process, and readers of the image files they write."""
import atexit
import ctypes as C
import glob
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np

from realtimepathtracingresearchframework_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "realtimepathtracingresearchframework_amd", "host")
_cache = {}
_dir = None


def build_host_tool(name, werror=True, link_library=True, extra=()):
    """the path of an executable built from host/<name>.cpp with g++ -std=c++17 -O1 -Wall [-Werror] [extra], linked against the
    library (built first if it is missing) unless link_library is False. One compile per process for each source, flag set and newest
    modification time among the host sources, the ABI headers and the library; the executables live in one temporary directory that
    is removed when the process ends, so callers keep their outputs somewhere else."""
    global _dir
    src = os.path.join(HOST, name + ".cpp")
    compile_flags = ["-std=c++17", "-O1", "-Wall"] + (["-Werror"] if werror else [])
    link_flags = list(extra)  # after the source: the order a linker resolves in
    inputs = glob.glob(os.path.join(HOST, "*.hpp")) + glob.glob(os.path.join(HOST, "*.cpp")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if link_library:
        if not os.path.exists(build.LIB_PATH):
            build.build_library()
        libdir = os.path.dirname(build.LIB_PATH)
        link_flags += ["-L" + libdir, "-lrptr_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
        inputs.append(build.LIB_PATH)
    key = (src, tuple(compile_flags + link_flags), max(os.path.getmtime(f) for f in inputs))
    if key not in _cache:
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="rptr_host_tools_")
            atexit.register(shutil.rmtree, _dir, ignore_errors=True)
        out = os.path.join(_dir, str(len(_cache)))
        os.mkdir(out)
        exe = os.path.join(out, name)
        subprocess.check_call(["g++"] + compile_flags + [src, "-o", exe] + link_flags)
        _cache[key] = exe
    return _cache[key]


def read_pfm(path):
    """the reference's layout: 'PF', 'w h', '-1.0' (little endian), rows bottom-up, RGB float32"""
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(v) for v in f.readline().split())
        assert f.readline() == b"-1.0\n"
        data = np.frombuffer(f.read(), dtype="<f4")
    assert data.size == w * h * 3
    return data.reshape(h, w, 3)[::-1]


def read_exr(path):
    """minimal reader of what write_image.hpp writes: single-part scan-line OpenEXR, no compression, channels A B G R of one
    type -> (h, w, 4) RGBA array (float32, or uint16 holding halfs)"""
    raw = open(path, "rb").read()
    assert struct.unpack_from("<II", raw, 0) == (20000630, 2)
    at, attrs = 8, {}
    while raw[at] != 0:
        name_end = raw.index(b"\0", at)
        type_end = raw.index(b"\0", name_end + 1)
        size = struct.unpack_from("<I", raw, type_end + 1)[0]
        attrs[raw[at:name_end].decode()] = (raw[name_end + 1:type_end].decode(), raw[type_end + 5:type_end + 5 + size])
        at = type_end + 5 + size
    at += 1
    assert attrs["compression"][1] == b"\0" and attrs["lineOrder"][1] == b"\0"
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    ch, names, types = attrs["channels"][1], [], []
    k = 0
    while ch[k] != 0:
        e = ch.index(b"\0", k)
        names.append(ch[k:e].decode())
        types.append(struct.unpack_from("<I", ch, e + 1)[0])
        k = e + 1 + 16
    assert names == ["A", "B", "G", "R"] and len(set(types)) == 1
    dt = np.float32 if types[0] == 2 else np.uint16
    offsets = struct.unpack_from("<%dQ" % h, raw, at)
    img = np.zeros((h, w, 4), dt)
    for y in range(h):
        yy, size = struct.unpack_from("<iI", raw, offsets[y])
        assert yy == y and size == w * 4 * np.dtype(dt).itemsize
        rows = np.frombuffer(raw, dtype=dt, count=4 * w, offset=offsets[y] + 8).reshape(4, w)
        img[y, :, 3], img[y, :, 2], img[y, :, 1], img[y, :, 0] = rows[0], rows[1], rows[2], rows[3]
    return img


def read_png(path):
    """8-bit RGBA PNG with filter type 0 rows (what write_image.hpp writes) -> (h, w, 4) uint8; checks every chunk's CRC"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, w, h = 8, b"", 0, 0
    while at < len(raw):
        n, kind = struct.unpack_from(">I4s", raw, at)
        data = raw[at + 8:at + 8 + n]
        assert zlib.crc32(kind + data) == struct.unpack_from(">I", raw, at + 8 + n)[0]
        if kind == b"IHDR":
            w, h, depth, colour = struct.unpack_from(">IIBB", data, 0)
            assert (depth, colour) == (8, 6)
        elif kind == b"IDAT":
            idat += data
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4).copy()


# a --config file for rptr_cli: reprojection_mode 2 (REPROJECTION_MODE_ACCUMULATE): the moving camera of --fly-through then keeps its history instead of restarting
ACCUMULATE_INI = """[Application][]
[.][Filtering]
[.][*reprojection]
ACCUMULATE= 1
..
..
..
"""


# host/sky_fit.hpp behind a C interface: the sky fit and the sun direction, for ctypes
SKY_SHIM = r'''
#include "sky_fit.hpp"
extern "C" int shim_fit(const char *where, const float *sun_dir, float turbidity, const float *albedo, int light_count, RptrSceneParams *out, char *err, int cap) {
    static rptr::SkyTables t;
    static std::string loaded;
    std::string e;
    if (loaded != where) {
        t = rptr::SkyTables();
        if (!rptr::load_sky_tables(where, t, e)) { snprintf(err, cap, "%s", e.c_str()); return 1; }
        loaded = where;
    }
    snprintf(err, cap, "%s", e.c_str());
    return rptr::fit_sky(t, sun_dir, turbidity, albedo, light_count, *out) ? 0 : 2;
}
extern "C" void shim_sun(float h, float a, float *out) { rptr::sun_dir_from_height_angle(h, a, out); }
'''


def build_sky_shim(tmp_path):
    src = tmp_path / "sky_shim.cpp"
    src.write_text(SKY_SHIM)
    so = str(tmp_path / "libsky_shim.so")
    # (the reference side is built with plain -O2: no contraction on x86-64 without -mfma, same here)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", "-I" + HOST, str(src), "-o", so])
    L = C.CDLL(so)
    L.shim_fit.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.c_int, C.POINTER(abi.SceneParams), C.c_char_p, C.c_int]
    return L


def sky_words(sp):
    """the words of an abi.SceneParams that the fit writes"""
    return np.frombuffer(bytes(sp), np.uint32)[:(160 + 12 + 4 + 16) // 4]   # sky params, sun_dir, sun_cos_angle, sun_radiance
