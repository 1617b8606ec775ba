"""bin/rptr_hip --denoise-temporal (host/rptr_cli.cpp): every frame of a run goes through rptr_hip_denoise_temporal as it is collected and
the images written are the denoised ones, the images the Python mirror's denoise_temporal() leaves for the same frames; combined with
--denoise, --taa-upscale or several devices the flag is refused."""
import os
import subprocess

import numpy as np
import pytest

from common import fly_camera
from host_tools import ACCUMULATE_INI, build_host_tool, read_png
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu


def test_denoise_temporal_flag_writes_the_mirrors_denoised_images(tmp_path):
    exe = build_host_tool("rptr_cli")
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    ini = tmp_path / "realtime.ini"
    ini.write_text(ACCUMULATE_INI)   # (reprojection_mode 2: the moving camera keeps its accumulation, so only the first frame resets the history)
    W, H, n = 64, 48, 3
    run = subprocess.run([exe, path, "--config", str(ini), "--img", str(W), str(H), "--batch-spp", "1", "--synchronous", "--fly-through", "--png",
                          "--profiling-fps", "1", "--profiling-count", str(n), "--profiling", str(tmp_path / "dt"), "--profiling-img", str(tmp_path / "dt"),
                          "--denoise-temporal", "3"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    # the mirror: the run's four warm-up frames (the first view, each restarting the accumulation), then the three frames
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    r.params.reprojection_mode = 2
    cam = s.camera_params()
    for _ in range(4):
        r.render(backend.RenderConfiguration(fly_camera(cam, 0), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)
    want = []
    for k in range(n):
        r.render(backend.RenderConfiguration(fly_camera(cam, k), active_variant=abi.VARIANT_GLTF, reset_accumulation=k == 0), spp=1)
        r.denoise_temporal(iterations=3, reset_history=int(k == 0))
        want.append(r.readback_denoised_u8())
    assert r.readback_denoise_history()[..., 3].max() == n                    # the last image carries the history of all three
    r.denoise(iterations=3)
    assert not np.array_equal(r.readback_denoised_u8(), want[-1])             # ... and is not the spatial denoiser's
    r.close()
    for k in range(n):
        got = read_png("%s_%04d.png" % (tmp_path / "dt", k + 1))
        assert got.shape == (H, W, 4)
        assert np.array_equal(got, want[k]), (k, int(np.count_nonzero(got != want[k])))


REFUSED = [(["--denoise", "3"], "--denoise-temporal and --denoise cannot be combined"),
           (["--taa-upscale"], "--denoise-temporal and --taa-upscale cannot be combined"),
           (["--devices", "0,0"], "--denoise-temporal needs one device")]


def test_denoise_temporal_refused_combinations(tmp_path):
    exe = build_host_tool("rptr_cli")
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    for extra, message in REFUSED:
        run = subprocess.run([exe, path, "--validation", str(tmp_path / "x"), "--img", "32", "32", "--denoise-temporal", "3"] + extra, capture_output=True, text=True)
        assert run.returncode != 0, extra
        assert message in run.stderr, (extra, run.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("x_")], extra
    run = subprocess.run([exe, path, "--validation", str(tmp_path / "x"), "--img", "32", "32", "--denoise-temporal", "6"], capture_output=True, text=True)
    assert run.returncode != 0 and "--denoise-temporal takes 1..5 iterations" in run.stderr
