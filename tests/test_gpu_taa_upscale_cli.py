"""bin/rptr_hip --taa-upscale (host/rptr_cli.cpp): the RGBA8 images of a profiling run are the upscaled ones, at twice --img, the images
the Python mirror's taa_upscale() returns for the same frames; combined with --denoise the flag is refused."""
import os
import subprocess

import numpy as np
import pytest

from common import fly_camera
from host_tools import ACCUMULATE_INI, build_host_tool, read_png
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu


def test_taa_upscale_flag_writes_the_mirrors_upscaled_images(tmp_path):
    exe = build_host_tool("rptr_cli")
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    ini = tmp_path / "realtime.ini"
    ini.write_text(ACCUMULATE_INI)
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
        r.render(backend.RenderConfiguration(fly_camera(cam, 0), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)
    want, frames = [], []
    for k in range(n):
        r.render(backend.RenderConfiguration(fly_camera(cam, k), active_variant=abi.VARIANT_GLTF, reset_accumulation=k == 0), spp=1)
        fb = np.zeros((H, W, 4), np.uint8)
        r.readback_framebuffer(fb)
        frames.append(fb)
        r.taa_upscale(reset_history=int(k == 0))
        want.append(r.readback_upscaled())
    r.close()
    for k in range(n):
        got = read_png("%s_%04d.png" % (tmp_path / "up", k + 1))
        assert got.shape == (2 * H, 2 * W, 4)
        assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))
        assert np.array_equal(read_png("%s_%04d.png" % (tmp_path / "plain", k + 1)), frames[k]), k   # without the flag: the frame
    rep = np.repeat(np.repeat(frames[-1], 2, axis=0), 2, axis=1)
    assert not np.array_equal(want[-1], rep)   # the last image carries history


def test_taa_upscale_with_denoise_is_refused(tmp_path):
    exe = build_host_tool("rptr_cli")
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    run = subprocess.run([exe, path, "--validation", str(tmp_path / "x"), "--img", "32", "32", "--taa-upscale", "--denoise", "3"], capture_output=True, text=True)
    assert run.returncode != 0
    assert "--taa-upscale and --denoise cannot be combined" in run.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x_")]
