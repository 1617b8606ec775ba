"""Persistent traversal grids sized for the frames that really share the GPU (csrc/host_state.h traversal_grid).

A frame alone on the GPU gets every block that fits; a frame submitted while others of its handle are in flight gets about 12 / n blocks
per CU, n at most the hardware queues. The kernels pull their work from a cursor, so the grid changes no image and no ray count: five frame
contexts with launch sequences of four frames give the images of a one-context handle, bit for bit, at two and at four hardware queues.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from realtimepathtracingresearchframework_amd import abi, backend, scenes  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, N_CTX, N_SEQ, PER_SEQ = 160, 96, 2, 5, 5, 4


def test_grids_stay_within_the_resident_maximum_for_every_context_count():
    queues = max(1, int(os.environ.get("GPU_MAX_HW_QUEUES", "4")))
    for n in range(1, 12):
        r = backend.RenderHip(frames_in_flight=n)
        r.initialize(64, 64)
        g = {k: r.get_option(k) for k in ("traversal_resident_blocks", "traversal_grid_alone", "traversal_grid_shared",
                                          "traversal_stack_blocks", "traversal_concurrency")}
        r.close()
        assert g["traversal_concurrency"] == min(n, queues), (n, g)
        assert 0 < g["traversal_grid_shared"] <= g["traversal_grid_alone"] <= g["traversal_resident_blocks"], (n, g)
        assert g["traversal_grid_alone"] == g["traversal_resident_blocks"], (n, g)   # a frame alone fills the device
        assert g["traversal_stack_blocks"] >= g["traversal_grid_alone"], (n, g)      # the stack scratch holds the largest grid
        if g["traversal_concurrency"] == 1:
            assert g["traversal_grid_shared"] == g["traversal_grid_alone"], (n, g)


def test_a_frame_alone_gets_the_full_grid_on_a_handle_with_five_contexts():
    s = scenes.cornell32()
    r = backend.RenderHip(frames_in_flight=N_CTX)
    r.initialize(64, 64)
    r.set_scene(s)
    alone = r.get_option("traversal_grid_alone")
    for _ in range(2):   # (the first frame of a handle runs without the tail kernel)
        r.wait(r.render_async(backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1))
        assert r.get_option("last_traversal_grid") == alone
    tickets = [r.render_async(backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)
               for _ in range(3)]
    assert r.get_option("traversal_grid_shared") <= r.get_option("last_traversal_grid") <= alone
    for t in tickets:
        r.wait(t)
    r.close()


def _render(n_ctx, out_path):
    """N_SEQ x PER_SEQ frames: with n_ctx > 1 in launch sequences of PER_SEQ frames, all of them in flight before the first is
    collected; with one context frame by frame. Writes every frame's RGBA32F image and the rays of each launch sequence."""
    s = scenes.grid(120, 60, with_emitters=True)
    cam = s.camera_params()
    r = backend.RenderHip(frames_in_flight=n_ctx)
    r.initialize(W, H)
    r.set_scene(s)
    images, rays = [], []

    def collect(t):
        st = r.wait(t)
        img = np.zeros((H, W, 4), np.float32)
        assert r.readback_framebuffer(img) == W * H * 4
        images.append(img)
        rays.append((int(st.raw.rays_closest), int(st.raw.rays_shadow)))

    cfg = backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True)
    if n_ctx > 1:
        queued = [r.render_batch_async(cfg, spp=SPP, n_frames=PER_SEQ, reset_rest=True) for _ in range(N_SEQ)]
        for tickets in queued:
            for t in tickets:
                collect(t)
    else:
        for _ in range(N_SEQ * PER_SEQ):
            collect(r.render_async(cfg, spp=SPP))
    r.close()
    np.savez(out_path, images=np.stack(images), rays=np.asarray(rays, np.int64))


@pytest.mark.parametrize("queues", [2, 4])
def test_five_contexts_give_the_images_of_one_context(tmp_path, queues):
    """each run in a child process: the HIP runtime reads GPU_MAX_HW_QUEUES once, at the process's first HIP call"""
    out = {}
    for n_ctx in (1, N_CTX):
        path = str(tmp_path / ("ctx%d.npz" % n_ctx))
        env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(n_ctx), path], capture_output=True, text=True, timeout=300,
                           env=env, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        out[n_ctx] = np.load(path)
    ref, got = out[1], out[N_CTX]
    assert ref["images"].shape == got["images"].shape == (N_SEQ * PER_SEQ, H, W, 4)
    assert np.array_equal(ref["images"].view(np.uint32), got["images"].view(np.uint32))
    # a frame of a launch sequence reports an equal share of the sequence's counts (rounded down): the totals of the same frames one by one
    share = ref["rays"].reshape(N_SEQ, PER_SEQ, 2).sum(axis=1) // PER_SEQ
    assert np.array_equal(got["rays"].reshape(N_SEQ, PER_SEQ, 2), np.repeat(share[:, None, :], PER_SEQ, axis=1)), (ref["rays"], got["rays"])
    assert len({img.tobytes() for img in ref["images"]}) == N_SEQ * PER_SEQ   # every frame has seeds of its own


if __name__ == "__main__":
    _render(int(sys.argv[1]), sys.argv[2])
