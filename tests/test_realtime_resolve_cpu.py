"""The real-time resolve without a GPU: known answers of its numpy restatement (tests/realtime_resolve_ref.py, the statement the GPU tests
hold csrc/realtime_resolve.h to), the .ini reader's REPROJECTION_MODE_ACCUMULATE and the "taa" option in the C ABI's table."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import realtime_resolve_ref as R
from code_object import kernel_regs
from host_tools import build_host_tool
from realtimepathtracingresearchframework_amd import abi, backend, build, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12


def _frame(color, alpha=1.0, depth=2.0, motion=(0.0, 0.0)):
    mean = np.zeros((H, W, 4), np.float32)
    mean[..., :3] = color
    mean[..., 3] = alpha
    nd = np.zeros((H, W, 4), np.float16)
    nd[..., 2] = 1.0
    nd[..., 3] = depth
    mj = np.zeros((H, W, 4), np.float16)
    mj[..., 0], mj[..., 1] = motion
    return mean, nd, mj


def _run(colors, spp, window):
    """frames of uniform colours through the restatement; returns the per-frame new-sample weights and stored images"""
    weights, stored = [], []
    hist = hist_nd = None
    for k, col in enumerate(colors):
        mean, nd, mj = _frame(col)
        st, shown, w = R.reproject(mean, nd, mj, hist, hist_nd, spp, window, use_history=k > 0, return_weight=True)
        assert np.array_equal(shown[..., :3], st[..., :3]) and np.all(shown[..., 3] == 1.0)
        weights.append(w)
        stored.append(st)
        hist, hist_nd = st, nd
    return weights, stored


def test_weight_sequence_of_alternating_uniform_colours():
    """zero motion, constant normal and depth, a colour uniform over the image that alternates a, b: frame 0 stores its mean, frame 1
    folds with weight 1 (the history alpha is the coverage, 1), frame k >= 2 follows old / (1 + old * spp) floored at 1 / window -- the
    projection gives t = 1 and adds nothing. (Interior pixels: the border's 3x3 rings read zeros outside the image.)"""
    a, b = np.array([0.2, 0.5, 0.9], np.float32), np.array([0.7, 0.1, 0.3], np.float32)
    for spp, window in ((1, 8), (2, 8), (4, 3)):
        weights, stored = _run([a if k % 2 == 0 else b for k in range(10)], spp, window)
        want, old = [1.0, 1.0], 1.0
        for k in range(2, 10):
            w = max(old / (1.0 + old * spp), 1.0 / window)
            want.append(w)
            old = w
        inner = (slice(1, H - 1), slice(1, W - 1))
        for k in range(10):
            got = weights[k][inner]
            assert np.allclose(got, want[k], rtol=1e-5, atol=1e-6), (spp, window, k, float(got.min()), float(got.max()), want[k])
        assert np.allclose(stored[0][..., :3], a) and np.all(stored[0][..., 3] == 1.0)
        assert np.allclose(stored[1][inner][..., :3], b) and np.all(stored[1][inner][..., 3] == 0.0)
        # the stored colour is the running blend: history + (mean - history) * w
        h = b.astype(np.float64)
        for k in range(2, 10):
            h = h + ((a if k % 2 == 0 else b) - h) * want[k]
            assert np.allclose(stored[k][inner][..., :3], h, rtol=1e-5, atol=1e-6)
            assert np.allclose(stored[k][inner][..., 3], 1.0 - want[k], atol=1e-6)


def test_history_equal_to_the_current_colour_gives_weight_one():
    """BILATERAL_PROJECTION: t = dot / dot(line, line) is 0 / 0 when the history equals this frame's colour; max(NaN, 0) = 0 (fmaxf) and
    the new-sample weight becomes 1 -- restated as the reference has it, not guarded away"""
    c = np.array([0.4, 0.4, 0.4], np.float32)
    weights, stored = _run([c] * 5, 2, 8)
    for k in range(5):
        assert np.all(weights[k] == 1.0)
        assert np.allclose(stored[k][..., :3], c)


def test_reconstruction_outside_the_image_and_a_depth_jump_reset_the_pixel():
    """a reconstruction point outside [0, 1) has no history: weight 1; a depth jump between the history's normal + depth and this frame's
    gives a bilateral weight of 0 everywhere, hence weight 1"""
    a, b = np.array([0.2, 0.5, 0.9], np.float32), np.array([0.7, 0.1, 0.3], np.float32)
    _, stored = _run([a, b, a], 2, 8)
    hist = stored[-1]
    # motion pointing half a frame to the left: pixels in the left half reconstruct outside the image
    mean, nd, mj = _frame(b, motion=(-1.0, 0.0))
    _, _, w = R.reproject(mean, nd, mj, hist, nd, 2, 8, return_weight=True)
    left = np.arange(W) + 0.5 < W / 2
    assert np.all(w[:, left] == 1.0)
    assert np.all(w[1:-1, ~left][:, 1:-1] < 1.0)
    # a depth jump: the history's surface is ten times as far
    mean, nd, mj = _frame(b)
    far = nd.copy()
    far[..., 3] = 20.0
    _, _, w = R.reproject(mean, nd, mj, hist, far, 2, 8, return_weight=True)
    assert np.all(w == 1.0)
    _, _, w = R.reproject(mean, nd, mj, hist, nd, 2, 8, return_weight=True)
    assert np.all(w[1:-1, 1:-1] < 1.0)


def test_taa_of_uniform_images_and_outside_reconstruction():
    """the TAA pass: a uniform frame over a uniform history clamps to the neighbourhood box, which has no width, so the frame is kept
    (interior pixels); a
    reconstruction point outside the image keeps the frame as well; with a textured frame the result stays inside [box low, box high]"""
    pre = np.full((H, W, 4), 200, np.uint8)
    hist = np.full((H, W, 4), 40, np.uint8)
    mj = np.zeros((H, W, 4), np.float16)
    assert np.array_equal(R.taa(pre, hist, mj)[1:-1, 1:-1], pre[1:-1, 1:-1])   # (the border's boxes hold zeros from outside the image)
    mj[..., 0] = 4.0
    assert np.array_equal(R.taa(pre, hist, mj), pre)
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    mj[...] = 0
    out = R.taa(pre, hist, mj)
    # history darker than the frame: the blend pulls towards it, never above the frame where the box allows it
    assert out.dtype == np.uint8 and out.shape == pre.shape
    assert np.mean(out[1:-1, 1:-1].astype(np.int32)) < np.mean(pre[1:-1, 1:-1].astype(np.int32))


def test_reset_frame_stores_the_mean_with_its_coverage():
    mean, nd, mj = _frame(np.array([0.3, 0.2, 0.1], np.float32), alpha=0.75)
    st, shown = R.reproject(mean, nd, mj, None, None, 2, 8, use_history=False)
    assert np.array_equal(st, mean) and np.array_equal(shown, mean)


INI = """[Application][scene.vks]
[.][Filtering]
[.][*reprojection]
ACCUMULATE= 1
..
..
"""


def test_ini_reprojection_accumulate_is_mode_two(tmp_path):
    """.ini `reprojection ACCUMULATE` (REPROJECTION_MODE_NAMES) is the real-time resolve, mode 2, without a note that NONE is used"""
    exe = build_host_tool("rptr_cli")
    path = str(tmp_path / "c.rpsc")
    scenes.cornell32().dump(path)
    (tmp_path / "acc.ini").write_text(INI)
    out = subprocess.run([exe, path, "--describe", "--config", str(tmp_path / "acc.ini")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    cfg = out.stdout.strip().splitlines()[1].split()
    kv = dict(zip(cfg[1::2], cfg[2::2]))
    assert int(kv["reprojection_mode"]) == abi.REPROJECTION_MODE_ACCUMULATE == 2
    assert "NONE is used" not in out.stdout + out.stderr


def test_taa_option_is_in_the_table_and_the_header():
    """option "taa" (RenderBackendOptions::enable_taa): enumerated, default 0, range 0..1, documented with RPTR_TAA in include/rptr_hip.h,
    whose options table now has 22 keys; mode 2 is documented there too"""
    L = backend.load_library()
    hdr = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    n = L.rptr_hip_option_count()
    keys = [L.rptr_hip_option_name(i).decode() for i in range(n)]
    assert "taa" in keys and n == 22
    assert re.search(r"^ \*   taa\s+0\s+next frame.*RPTR_TAA", hdr, re.M)
    assert "REPROJECTION_MODE_ACCUMULATE" in hdr
    v = C.c_int64(-1)
    assert L.rptr_hip_get_option(None, b"taa", C.byref(v)) == 0 and v.value == int(os.environ.get("RPTR_TAA", "0"))
    assert L.rptr_hip_set_option(None, b"taa", 2) == abi.RPTR_E_INVALID


def test_the_taa_kernel_uses_no_scratch():
    """rp_k_taa in the gfx950 code object: no private segment; its LDS is the 24 x 24 history window, the 10 x 10 float4 neighbourhood and
    the byte / 255 table (the window's base lives in registers). Registers: at most 128, the step at which four waves per SIMD fit
    (512 / 128)"""
    regs = kernel_regs()
    taa = [v for k, v in regs.items() if "rp_k_taa" in k and "rp_k_taa_upscale" not in k]
    assert len(taa) == 1, sorted(regs)
    vgpr, _, scratch, lds = taa[0]
    assert scratch == 0
    assert lds == 24 * 24 * 4 + 100 * 16 + 256 * 4, lds
    assert vgpr <= 128, vgpr
