"""bin/rptr_hip --taa-upscale (host/rptr_cli.cpp): the RGBA8 images of a profiling run are the upscaled ones, at twice --img, the images
the Python mirror's taa_upscale() returns for the same frames; combined with --denoise the flag is refused."""
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from realtimepathtracingresearchframework_amd import abi, backend, build, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "realtimepathtracingresearchframework_amd", "host")

# reprojection_mode 2 (REPROJECTION_MODE_ACCUMULATE): the moving camera of --fly-through then keeps its history instead of restarting
INI = """[Application][]
[.][Filtering]
[.][*reprojection]
ACCUMULATE= 1
..
..
..
"""


def _build_cli(tmp_path):
    if not os.path.exists(build.LIB_PATH):
        build.build_library()
    exe = str(tmp_path / "rptr_hip")
    libdir = os.path.dirname(build.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HOST, "rptr_cli.cpp"), "-o", exe, "-L" + libdir,
                           "-lrptr_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _read_png(path):
    """the RGBA8 PNG files host/write_image.hpp writes: one IDAT chunk, filter type 0 on every scan line"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 6)
            size = (w, h)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 4)


def _fly_camera(cam, k):
    """frame k of --fly-through (rptr_cli.cpp fly_camera, bench.py's path): yawed by 0.002 rad x s about the up axis from 2 cm x s further
    to the right, s = k mod 64 - 32; evaluated in double, rounded to float once"""
    s = k % 64 - 32
    a = 0.002 * s
    d = [float(v) for v in cam.dir[:]]
    u = [float(v) for v in cam.up[:]]
    r = [d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]]
    rl = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    r = [x / rl for x in r]
    nd = [math.cos(a) * d[i] + math.sin(a) * r[i] for i in range(3)]
    nl = math.sqrt(nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2])
    c = abi.Camera()
    c.pos[:] = [float(np.float32(float(cam.pos[i]) + 0.02 * s * r[i])) for i in range(3)]
    c.dir[:] = [float(np.float32(nd[i] / nl)) for i in range(3)]
    c.up[:] = cam.up[:]
    c.fovy = cam.fovy
    return c


def test_taa_upscale_flag_writes_the_mirrors_upscaled_images(tmp_path):
    exe = _build_cli(tmp_path)
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    ini = tmp_path / "realtime.ini"
    ini.write_text(INI)
    W, H, n = 64, 48, 3
    common = [exe, path, "--config", str(ini), "--img", str(W), str(H), "--batch-spp", "1", "--synchronous", "--fly-through", "--png",
              "--profiling-fps", "1", "--profiling-count", str(n)]   # (one frame per second of animation time: an image per frame)
    run = subprocess.run(common + ["--profiling", str(tmp_path / "up"), "--profiling-img", str(tmp_path / "up"), "--taa-upscale"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    plain = subprocess.run(common + ["--profiling", str(tmp_path / "plain"), "--profiling-img", str(tmp_path / "plain")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    # the mirror: the run's four warm-up frames (the first view, each restarting the accumulation), then the three frames
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    r.params.reprojection_mode = 2
    cam = s.camera_params()
    for _ in range(4):
        r.render(backend.RenderConfiguration(_fly_camera(cam, 0), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)
    want, frames = [], []
    for k in range(n):
        r.render(backend.RenderConfiguration(_fly_camera(cam, k), active_variant=abi.VARIANT_GLTF, reset_accumulation=k == 0), spp=1)
        fb = np.zeros((H, W, 4), np.uint8)
        r.readback_framebuffer(fb)
        frames.append(fb)
        r.taa_upscale(reset_history=int(k == 0))
        want.append(r.readback_upscaled())
    r.close()
    for k in range(n):
        got = _read_png("%s_%04d.png" % (tmp_path / "up", k + 1))
        assert got.shape == (2 * H, 2 * W, 4)
        assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))
        assert np.array_equal(_read_png("%s_%04d.png" % (tmp_path / "plain", k + 1)), frames[k]), k   # without the flag: the frame
    rep = np.repeat(np.repeat(frames[-1], 2, axis=0), 2, axis=1)
    assert not np.array_equal(want[-1], rep)   # the last image carries history


def test_taa_upscale_with_denoise_is_refused(tmp_path):
    exe = _build_cli(tmp_path)
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    run = subprocess.run([exe, path, "--validation", str(tmp_path / "x"), "--img", "32", "32", "--taa-upscale", "--denoise", "3"], capture_output=True, text=True)
    assert run.returncode != 0
    assert "--taa-upscale and --denoise cannot be combined" in run.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x_")]
