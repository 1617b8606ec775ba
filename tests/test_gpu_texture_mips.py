"""Dynamic textures on the device (include/rptr_hip.h "dynamic textures", csrc/texture_mips.h): rptr_hip_update_texture[_device],
readback_texture and texture_levels against tests/texture_mips_ref.py. Every comparison is exact: levels byte for byte, frames bit for
bit against a fresh set_scene whose Texture.mips are the reference's chains."""
import copy
import ctypes as C

import numpy as np
import pytest

import texture_mips_ref as TM
from common import config, one_grid_elements, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
W = H = 48
SPP = 2
# (width, height) of the chain cases: one level; 2 x 2; one axis stops at 1; non-square even; three taps; even -> odd -> even along the
# chain; odd both ways; more than one block; several blocks along x with an odd tail -- and the transposes of the non-square ones
SIZES = [(1, 1), (2, 2), (1, 8), (8, 1), (16, 8), (8, 16), (3, 3), (5, 3), (3, 5), (7, 7), (6, 10), (10, 6), (33, 17), (17, 33), (64, 64),
         (300, 20), (20, 300)]


@pytest.fixture(scope="module")
def table():
    return backend.srgb_decode_table()


def _random_texture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def _with_textures(scene, replaced):
    """a copy of the scene with textures[k] = replaced[k]"""
    s = copy.copy(scene)
    s.textures = [replaced.get(k, t) for k, t in enumerate(scene.textures)]
    return s


def _chained(scene, table, which=(0, 1, 2)):
    """a copy whose textures `which` carry the reference's full chains"""
    return _with_textures(scene, {k: scenes.Texture(rgba=scene.textures[k].rgba, srgb=scene.textures[k].srgb,
                                                    mips=TM.chain(scene.textures[k].rgba, scene.textures[k].srgb, table) or None) for k in which})


def _frame(r, scene, stats=False):
    st = r.render(config(scene, abi.VARIANT_GLTF, reset=True, freeze_frame=True), spp=SPP)
    return (read_frame(r, W, H), int(st.raw.device_bytes_allocated)) if stats else read_frame(r, W, H)


def _assert_chain(r, index, level0, srgb, table, what=""):
    want = [np.ascontiguousarray(level0)] + TM.chain(level0, srgb, table)
    assert r.texture_levels(index) == len(want) == TM.full_levels(*level0.shape[:2]), what
    for l, lv in enumerate(want):
        got = r.readback_texture(index, l)
        assert got.shape == lv.shape, (what, l)
        assert np.array_equal(got, lv), "%s level %d (%d x %d): %d of %d bytes differ" % (what, l, lv.shape[1], lv.shape[0], int((got != lv).sum()), lv.size)


def _code(exc):
    return exc.value.code


# ------------------------------------------------------------------ 1. the chain against the reference
def test_every_level_equals_the_reference(table):
    """One scene holds every case twice (sRGB and linear, random colours and alpha); update_texture(t, None) makes each chain."""
    base = scenes.textured_test()
    first = len(base.textures)
    cases = [(w, h, srgb) for w, h in SIZES for srgb in (True, False)]
    scene = copy.copy(base)
    scene.textures = list(base.textures) + [scenes.Texture(rgba=_random_texture(w, h, 1000 + 31 * w + h + int(srgb)), srgb=srgb) for w, h, srgb in cases]
    r = renderer(scene, W, H)
    for k, (w, h, srgb) in enumerate(cases):
        t = first + k
        assert r.texture_levels(t) == 1
        r.update_texture(t, None)
        _assert_chain(r, t, scene.textures[t].rgba, srgb, table, "%d x %d %s" % (w, h, "sRGB" if srgb else "linear"))
    for k in range(len(cases)):   # (a later texture's update left the earlier ones alone)
        assert np.array_equal(r.readback_texture(first + k, 0), scene.textures[first + k].rgba)
    r.close()


def test_a_level_past_one_grid(table):
    """rp_k_mip_level is grid-stride under grid_for's cap (common.one_grid_elements: 524 288 texels on 256 CUs). Level 0 is
    (2k + 1) x (2k + 1) sRGB texels with k the smallest number whose k x k level 1 has more than cap + 256 texels and no multiple of 256
    of them -- 1451 x 1451 and 725 x 725 on 256 CUs -- so level 1's launch takes the second trip with full blocks and a partial one, on
    the three-tap path."""
    cap = one_grid_elements()
    k = int(np.sqrt(cap))
    while not (k * k > cap + 256 and (k * k) % 256 != 0):
        k += 1
    size = 2 * k + 1
    base = scenes.textured_test()
    level0 = _random_texture(size, size, 77)
    scene = _with_textures(base, {0: scenes.Texture(rgba=level0, srgb=True)})
    r = renderer(scene, W, H)
    r.update_texture(0, None)
    print("cap %d texels: level 0 %d x %d, level 1 %d texels" % (cap, size, size, k * k))
    _assert_chain(r, 0, level0, True, table, "past one grid")
    r.close()


# ------------------------------------------------------------------ 2. the levels are sampled
@pytest.mark.parametrize("fast_math", [0, 1])
def test_generated_chains_render_as_uploaded_chains(table, fast_math):
    """(a) level 0 only + update_texture(t, None) on textures 0, 1, 2 == a fresh set_scene whose mips are the reference's chains;
    (b) that frame differs from the level-0-only frame."""
    scene = scenes.textured_test()
    fresh = _chained(scene, table)
    opts = {"fast_math": fast_math}
    a, b, c = renderer(scene, W, H, options=opts), renderer(fresh, W, H, options=opts), renderer(scene, W, H, options=opts)
    for t in (0, 1, 2):
        a.update_texture(t, None)
        _assert_chain(a, t, scene.textures[t].rgba, scene.textures[t].srgb, table, "texture %d" % t)
    fa, fb, fc = _frame(a, scene), _frame(b, fresh), _frame(c, scene)
    assert same_images(fa, fb)
    differing = int((fb[0].view(np.uint32) != fc[0].view(np.uint32)).any(axis=2).sum())
    print("fast_math %d: %d of %d pixels differ from the level-0-only frame" % (fast_math, differing, W * H))
    assert differing > 0
    for r in (a, b, c):
        r.close()


# ------------------------------------------------------------------ 3. new texels
def test_new_texels_with_and_without_the_chain_reuse_the_storage(table):
    scene = scenes.textured_test()
    r = renderer(scene, W, H)
    h0, w0 = scene.textures[0].rgba.shape[:2]
    news = [_random_texture(w0, h0, 200 + k) for k in range(3)]
    for n in news:
        n[..., 3] = 255
    bytes_seen = []
    for step, (texels, mips) in enumerate(zip(news, (True, False, True))):
        r.update_texture(0, texels, generate_mips=mips)
        new_tex = scenes.Texture(rgba=texels, srgb=True, mips=(TM.chain(texels, True, table) if mips else None))
        fresh = _with_textures(scene, {0: new_tex})
        if mips:
            _assert_chain(r, 0, texels, True, table, "update %d" % step)
        else:   # a texture that had a chain becomes level 0 only: the stale levels are out of reach
            assert r.texture_levels(0) == 1
            assert np.array_equal(r.readback_texture(0, 0), texels)
            with pytest.raises(backend.BackendError) as e:
                r.readback_texture(0, 1)
            assert _code(e) == abi.RPTR_E_INVALID
        b = renderer(fresh, W, H)
        fa, nbytes = _frame(r, scene, stats=True)
        assert same_images(fa, _frame(b, fresh)), "update %d" % step
        b.close()
        bytes_seen.append(nbytes)
    print("device bytes after the three updates:", bytes_seen)
    assert bytes_seen[0] == bytes_seen[1] == bytes_seen[2]      # the first update made the one allocation; nothing grows afterwards
    for t in (1, 2, 3):
        assert r.texture_levels(t) == 1 and np.array_equal(r.readback_texture(t, 0), scene.textures[t].rgba)
    r.close()


# ------------------------------------------------------------------ 4. device source
def test_a_device_source_equals_the_host_source(table):
    import torch
    scene = scenes.textured_test()
    texels = _random_texture(32, 32, 300)      # texture 2, the normal map: linear
    a, b = renderer(scene, W, H), renderer(scene, W, H)
    dev = torch.from_numpy(texels).cuda()
    torch.cuda.synchronize()                   # the tensor was written on torch's stream: finished before the backend's stream reads it
    a.update_texture(2, dev)
    b.update_texture(2, texels)
    _assert_chain(a, 2, texels, False, table, "device source")
    _assert_chain(b, 2, texels, False, table, "host source")
    assert same_images(_frame(a, scene), _frame(b, scene))
    a.update_texture(2, dev, generate_mips=False)
    assert a.texture_levels(2) == 1 and np.array_equal(a.readback_texture(2, 0), texels)
    a.close()
    b.close()
    del dev


# ------------------------------------------------------------------ 5. frames in flight
def test_three_frames_in_flight_see_the_update_in_submission_order(table):
    """Frames submitted before the update show the old texels (the call waits for them), frames submitted after it -- on every frame
    context, behind a device-source update that never synchronises the host -- show the new ones; both equal the one-at-a-time run."""
    import torch
    scene = scenes.textured_test()
    h0, w0 = scene.textures[0].rgba.shape[:2]
    texels = _random_texture(w0, h0, 400)
    texels[..., 3] = 255
    one = renderer(scene, W, H)
    old = _frame(one, scene)
    one.update_texture(0, texels)
    new = _frame(one, scene)
    one.close()
    assert not same_images(old, new)
    r = renderer(scene, W, H, frames_in_flight=3)
    cfg = config(scene, abi.VARIANT_GLTF, reset=True, freeze_frame=True)
    for _ in range(2):
        r.render_async(cfg, spp=SPP)
    dev = torch.from_numpy(texels).cuda()
    torch.cuda.synchronize()
    r.update_texture(0, dev)                   # waits for the two frames: the read-backs return the one finished last
    assert same_images(read_frame(r, W, H), old)
    tickets = [r.render_async(cfg, spp=SPP) for _ in range(3)]
    for t in tickets:
        r.wait(t)
        assert same_images(read_frame(r, W, H), new)
    _assert_chain(r, 0, texels, True, table, "frames in flight")
    r.close()
    del dev


# ------------------------------------------------------------------ 6. surface queries
def test_a_surface_query_returns_the_new_base_colour(table):
    scene = scenes.textured_test()
    r = renderer(scene, W, H)
    q = np.zeros((1, 8), f32)
    q[0, 0:3], q[0, 4:7], q[0, 7] = (0.3, 1.7, 2.0), (0.0, 0.0, -1.0), 1e20   # under the emissive quad, over the patch, into the flat quad
    cam = scene.camera_params()
    before = r.render_surface_queries(q, cam)[0]
    assert before["t"] > 0 and before["material_id"] == 1
    h0, w0 = scene.textures[0].rgba.shape[:2]
    texels = np.empty((h0, w0, 4), np.uint8)
    texels[...] = (200, 100, 50, 255)
    r.update_texture(0, texels)
    after = r.render_surface_queries(q, cam)[0]
    want = table[[200, 100, 50]]
    print("base colour before %s, after %s, the constant decodes to %s" % (before["base_color"], after["base_color"], want))
    # (sanity beside the exact comparison below: the sampler's weights of a constant are sums of products that round, a few dozen
    # operations of relative error 2^-24 each on values below 1)
    assert np.abs(after["base_color"] - want).max() <= 64 * 2.0 ** -24
    assert np.abs(before["base_color"] - want).max() > 1e-2
    fresh = renderer(_with_textures(scene, {0: scenes.Texture(rgba=texels, srgb=True, mips=TM.chain(texels, True, table))}), W, H)
    assert fresh.render_surface_queries(q, cam)[0].tobytes() == after.tobytes()
    fresh.close()
    r.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_change_nothing(table):
    L = backend.load_library()
    buf = np.zeros(4, np.uint8)
    n = C.c_uint32(7)
    assert L.rptr_hip_update_texture(None, 0, buf.ctypes.data_as(C.c_void_p), 4, 0) == abi.RPTR_E_INVALID
    assert L.rptr_hip_update_texture_device(None, 0, None, 0, abi.TEXTURE_GENERATE_MIPS) == abi.RPTR_E_INVALID
    assert L.rptr_hip_readback_texture(None, 0, 0, buf.ctypes.data_as(C.c_void_p), 4) == abi.RPTR_E_INVALID
    assert L.rptr_hip_texture_levels(None, 0, C.byref(n)) == abi.RPTR_E_INVALID and n.value == 7
    scene = scenes.textured_test()
    r = backend.RenderHip()
    r.initialize(W, H)
    for call in (lambda: r.update_texture(0, None), lambda: r.texture_levels(0)):      # before set_scene
        with pytest.raises(backend.BackendError) as e:
            call()
        assert _code(e) == abi.RPTR_E_INVALID and "set_scene" in str(e.value)
    assert L.rptr_hip_readback_texture(r._h, 0, 0, buf.ctypes.data_as(C.c_void_p), 4) == abi.RPTR_E_INVALID
    r.set_scene(scene)
    r.update_texture(1, None)                  # texture 1 has a chain, the others level 0 only
    levels0 = [r.texture_levels(t) for t in range(4)]
    assert levels0 == [1, 4, 1, 1]
    h0, w0 = scene.textures[0].rgba.shape[:2]
    good = _random_texture(w0, h0, 500)

    def unchanged():
        assert [r.texture_levels(t) for t in range(4)] == levels0
        for t in range(4):
            assert np.array_equal(r.readback_texture(t, 0), scene.textures[t].rgba)
        _assert_chain(r, 1, scene.textures[1].rgba, False, table, "texture 1")

    def raw(flags, texture=0, texels=good):
        return L.rptr_hip_update_texture(r._h, texture, texels.ctypes.data_as(C.c_void_p), texels.size, flags)
    invalid = {
        "texture >= num_textures": lambda: r.update_texture(4, good),
        "texture far out": lambda: r.update_texture(0xFFFFFFFF, None),
        "too few bytes": lambda: r.update_texture(0, good[:-1]),
        "too many bytes": lambda: r.update_texture(0, np.concatenate([good, good])),
        "another texture's size": lambda: r.update_texture(1, good),
        "NULL without the flag": lambda: r.update_texture(0, None, generate_mips=False),
        "unknown flag bits": lambda: r._check(raw(2)),
        "unknown flag bits beside the flag": lambda: r._check(raw(abi.TEXTURE_GENERATE_MIPS | 0x80000000)),
        "NULL with a byte count": lambda: r._check(L.rptr_hip_update_texture(r._h, 0, None, good.size, abi.TEXTURE_GENERATE_MIPS)),
        "a level beyond the levels": lambda: r.readback_texture(0, 1),
        "a level beyond the full chain": lambda: r.readback_texture(1, 4),
        "a read-back of another size": lambda: r._check(L.rptr_hip_readback_texture(r._h, 0, 0, buf.ctypes.data_as(C.c_void_p), 4)),
        "levels of a texture that is none": lambda: r.texture_levels(4),
    }
    for what, call in invalid.items():
        with pytest.raises(backend.BackendError) as e:
            call()
        assert _code(e) == abi.RPTR_E_INVALID, what
        assert "texture" in str(e.value), (what, str(e.value))
        unchanged()
    emissive = _random_texture(2, 2, 501)      # texture 3 colours the emissive quad: RptrSceneDesc.lights were made from it
    for call in (lambda: r.update_texture(3, emissive), lambda: r.update_texture(3, None), lambda: r.update_texture(3, emissive, generate_mips=False)):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert _code(e) == abi.RPTR_E_UNSUPPORTED and "texture 3" in str(e.value) and "emission" in str(e.value)
        unchanged()
    r.update_texture(0, good)                  # and the handle still works
    _assert_chain(r, 0, good, True, table, "after the refusals")
    r.close()
