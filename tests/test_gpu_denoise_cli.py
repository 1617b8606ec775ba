"""bin/rptr_hip --denoise <iterations> (host/rptr_cli.cpp): the image files of a run hold the denoised frame, the one the Python mirror's
denoise(iterations=n) returns for that frame; without the flag the files are what they always were."""
import subprocess

import numpy as np
import pytest

from host_tools import build_host_tool, read_pfm
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu


def test_denoise_flag_writes_the_mirrors_denoised_image(tmp_path):
    exe = build_host_tool("rptr_cli")
    s = scenes.cornell32()
    path = str(tmp_path / "cornell.rpsc")
    s.dump(path)
    W, H, spp = 48, 32, 2
    common = [exe, path, "--validation-spp", str(spp), "--batch-spp", str(spp), "--img", str(W), str(H), "--pfm"]
    plain = subprocess.run(common + ["--validation", str(tmp_path / "plain")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    den = subprocess.run(common + ["--validation", str(tmp_path / "den"), "--denoise", "3"], capture_output=True, text=True)
    assert den.returncode == 0, den.stderr
    r = backend.RenderHip()
    r.initialize(W, H)
    r.set_scene(s)
    r.render(backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=spp)
    raw = np.zeros((H, W, 4), np.float32)
    r.readback_framebuffer(raw)
    r.denoise(iterations=3)
    want = r.readback_denoised_f32()
    r.close()
    got_plain = read_pfm("%s_%04d.pfm" % (tmp_path / "plain", spp))
    got_den = read_pfm("%s_%04d.pfm" % (tmp_path / "den", spp))
    assert np.array_equal(got_plain.view(np.uint32), np.ascontiguousarray(raw[..., :3]).view(np.uint32))     # without the flag: the frame
    assert np.array_equal(got_den.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))
    assert not np.array_equal(got_den, got_plain)
    assert subprocess.run(common + ["--validation", str(tmp_path / "x"), "--denoise", "6"], capture_output=True).returncode == 2
