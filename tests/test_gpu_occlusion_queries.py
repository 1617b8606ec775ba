"""Occlusion queries (rptr_hip_trace_occlusion*, RenderHip.render_occlusion_queries): one bit per query, exact. Opaque mode against the
counted any-hit diagnostic, the oracle's brute force and the closest-hit query; the bits a run must leave alone; more pools than waves;
the cutout rule against scenes that omit what it ignores; moved instances; frames in flight."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from common import raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 33, 65, 4099)
SKIP = np.int32(-1).view(np.float32)  # mode_or_data < 0


def _rays(n, seed, lo, hi):
    """generic rays: origins uniform in the box [lo, hi], directions uniform on the sphere; a random half ends inside the scene
    (t_max between 2 % and 60 % of the box diagonal), the others never"""
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(lo), np.float32(hi)
    q = np.zeros((n, 8), np.float32)
    q[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    q[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    diag = float(np.linalg.norm(hi - lo))
    q[:, 7] = np.where(rng.random(n) < 0.5, rng.uniform(0.02 * diag, 0.6 * diag, n), 1e20)
    return q


def _bits_of(r, q, **kw):
    return r.render_occlusion_queries(q, **kw)


def _closest_hit(r, q):
    return r.render_ray_queries(q).view(np.int32)[:, 3] >= 0


CASES = {  # scene, renderer options, the box the origins come from
    "cornell32": (lambda: scenes.cornell32(), None, (-1, -1, -1), (1, 1, 1)),                       # one instance record: SINGLE
    "two_level_walk": (lambda: scenes.two_level_test(), {"flatten": 0}, (-5, -5, -5), (5, 5, 5)),   # instance walk
    "two_level_flat": (lambda: scenes.two_level_test(), None, (-5, -5, -5), (5, 5, 5)),             # flattened
    "soup": (lambda: scenes.soup(17), None, (-5, -5, -5), (5, 5, 5)),
}


# ---------------------------------------------------------------- 1. opaque mode
@pytest.mark.parametrize("case", sorted(CASES))
def test_opaque_bits_are_the_counted_diagnostics_the_brute_forces_and_the_closest_hit_querys(case):
    make, options, lo, hi = CASES[case]
    s = make()
    r = renderer(s, 64, 48, options=options)
    osc = O.OracleScene(s)
    full = _rays(max(SIZES), 1000 + len(case), lo, hi)
    for n in SIZES:
        q = full[-n:]  # (the tail: every size starts at another ray)
        got = _bits_of(r, q)
        assert got.dtype == np.bool_ and got.shape == (n,)
        counted = r.trace_counted(q, tmin=None, any_hit=True)[0][:, 0] != 0
        o = q[:, 0:3]
        tmin = np.float32(5e-6) * np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2], dtype=np.float32)
        assert tmin.dtype == np.float32
        _, ids = osc.trace_ex(o, q[:, 4:7], tmin, q[:, 7], any_hit=True, bvh_mode=O.BVH_BRUTE)
        brute = ids[:, 0] != 0
        closest = _closest_hit(r, q)
        print("%s n=%d: %d occluded; differs from counted %d, brute force %d, closest hit %d" % (
            case, n, int(got.sum()), int((got != counted).sum()), int((got != brute).sum()), int((got != closest).sum())))
        assert np.array_equal(got, counted), n
        assert np.array_equal(got, brute), n
        assert np.array_equal(got, closest), n
        if n == max(SIZES):  # the rays cover every case: hits and misses, among the bounded and the unbounded ones
            bounded = q[:, 7] < 1e19
            for sel in (bounded, ~bounded):
                assert got[sel].sum() >= 20 and (~got[sel]).sum() >= 20, (case, int(got[sel].sum()), int(sel.sum()))
    r.close()
    osc.close()


# ---------------------------------------------------------------- 2. the bits a run leaves alone
@pytest.mark.parametrize("n", [33, 4099])
def test_skipped_queries_and_the_bits_behind_n_keep_the_callers_pattern(n):
    import torch
    s = scenes.two_level_test()
    r = renderer(s, 64, 48)
    q = _rays(n, 50 + n, (-5, -5, -5), (5, 5, 5))
    answer = _bits_of(r, q)
    assert n < 100 or (answer.sum() > 20 and (~answer).sum() > 20)
    skipped = np.zeros(n, bool)
    skipped[::3] = True
    skipped[(n // 64) * 32:(n // 64) * 32 + 32] = True  # one whole 32-query word
    q[skipped, 3] = SKIP
    nw = (n + 31) // 32
    pattern = np.random.default_rng(n).integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)
    pat_bools = backend.RenderHip.unpack_occlusion_bits(pattern, nw * 32)
    want = np.where(skipped, pat_bools[:n], answer)
    want_words = backend.RenderHip.pack_occlusion_bits(np.concatenate([want, pat_bools[n:]]))

    def check(words, what):
        words = np.asarray(words, np.uint32)
        got = backend.RenderHip.unpack_occlusion_bits(words, nw * 32)
        assert np.array_equal(got[n:], pat_bools[n:]), what + ": bits >= n"
        assert np.array_equal(got[:n][skipped], pat_bools[:n][skipped]), what + ": skipped queries"
        assert np.array_equal(got[:n][~skipped], answer[~skipped]), what + ": answers"
        assert np.array_equal(words, want_words), what

    # the C entry on host arrays
    words = pattern.copy()
    assert r._L.rptr_hip_trace_occlusion(r._h, q.ctypes.data_as(C.c_void_p), n, None, words.ctypes.data_as(C.c_void_p)) == abi.RPTR_OK
    check(words, "host arrays")
    # the Python method: the bools of skipped queries come from `results`
    res = pat_bools[:n].copy()
    assert _bits_of(r, q, results=res) is res and np.array_equal(res, want)
    # n == 0 touches nothing
    guard = pattern.copy()
    assert r._L.rptr_hip_trace_occlusion(r._h, q.ctypes.data_as(C.c_void_p), 0, None, guard.ctypes.data_as(C.c_void_p)) == abi.RPTR_OK
    assert np.array_equal(guard, pattern)
    # device buffers on a caller's stream
    tq = torch.from_numpy(q).cuda()
    tb = torch.from_numpy(pattern.view(np.int32).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.render_occlusion_queries_device(n, device_queries=tq.data_ptr(), device_bits=tb.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    check(tb.cpu().numpy().view(np.uint32), "device buffers, caller's stream")
    # device_queries = NULL: the query buffer of enable_ray_queries, on the backend's stream
    dq, _ = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    tb2 = torch.from_numpy(pattern.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    r.render_occlusion_queries_device(n, device_bits=tb2.data_ptr())
    r.render_ray_queries(q[:1])  # (a synchronous call on the backend's stream: the run above has finished)
    check(tb2.cpu().numpy().view(np.uint32), "the backend's query buffer")
    with pytest.raises(backend.BackendError) as e:  # one query more than the budget
        r.render_occlusion_queries_device(n + 1, device_bits=tb2.data_ptr())
    assert e.value.code == abi.RPTR_E_INVALID and "exceed the budget" in str(e.value)
    r.close()


def test_calls_before_set_scene_and_before_initialize_are_refused():
    s = scenes.cornell32()
    q = _rays(40, 1, (-1, -1, -1), (1, 1, 1))
    for prepare, what in ((lambda r: None, "before set_scene"), (lambda r: r.set_scene(s), "before initialize")):
        r = backend.RenderHip()
        prepare(r)
        with pytest.raises(backend.BackendError) as e:
            _bits_of(r, q)
        assert e.value.code == abi.RPTR_E_INVALID and what in str(e.value), str(e.value)
        r.close()


def test_world_size_two_answers_like_one_rank():
    """every rank holds the whole scene: as for rptr_hip_trace, the ranks are not asked"""
    s = scenes.cornell32()
    q = _rays(500, 3, (-1, -1, -1), (1, 1, 1))
    r = renderer(s, 64, 48)
    one = _bits_of(r, q)
    r.close()
    r = backend.RenderHip(rank=0, world_size=2)
    r.initialize(64, 48)
    r.set_scene(s)
    two = _bits_of(r, q)
    r.close()
    assert np.array_equal(one, two) and one.any() and not one.all()


# ---------------------------------------------------------------- 3. more pools than waves
def test_waves_that_take_several_pools_agree_with_the_closest_hit_query_and_with_themselves():
    import torch
    s = scenes.cornell32()
    r = renderer(s, 64, 48)
    n = 2 ** 20 + 37
    resident_waves = r.get_option("traversal_resident_blocks") * 4  # 256 threads per block
    while n <= resident_waves * 64:
        n += 2 ** 20
    print("%d queries, %d resident waves x 64 = %d" % (n, resident_waves, resident_waves * 64))
    assert 0 < resident_waves * 64 < n
    q = _rays(n, 77, (-1, -1, -1), (1, 1, 1))
    tq = torch.from_numpy(q).cuda()
    tr = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    nw = (n + 31) // 32
    runs = [torch.full((nw,), fill, dtype=torch.int32, device="cuda") for fill in (0, -1)]  # (one run clears bits, the other sets them)
    torch.cuda.synchronize()
    r.trace_device(tq.data_ptr(), n, tr.data_ptr())
    for tb in runs:
        r.render_occlusion_queries_device(n, device_queries=tq.data_ptr(), device_bits=tb.data_ptr())
    r.render_ray_queries(q[:1])  # (synchronous on the backend's stream)
    closest = tr.cpu().numpy().view(np.int32)[:, 3] >= 0
    words = [tb.cpu().numpy().view(np.uint32) for tb in runs]
    r.close()
    tail = backend.RenderHip.unpack_occlusion_bits(words[0], nw * 32)[n:], backend.RenderHip.unpack_occlusion_bits(words[1], nw * 32)[n:]
    assert not tail[0].any() and tail[1].all()  # the bits behind n are each run's own fill
    a, b = (backend.RenderHip.unpack_occlusion_bits(w, n) for w in words)
    print("%d occluded; differs from the closest-hit query in %d, between the runs in %d" % (int(a.sum()), int((a != closest).sum()), int((a != b).sum())))
    assert np.array_equal(a, b)
    assert np.array_equal(a, closest)
    assert closest.sum() > 1000 and (~closest).sum() > 1000


# ---------------------------------------------------------------- 4. the cutout rule, exact
A64, A191, NOALPHA0, LITERAL = "alpha 64/255", "alpha 191/255", "alpha 0, NOALPHA", "literal colour"


def _screens_scene(screens, wall=True):
    """parallel screens z = 2.0, 1.5, 1.0, 0.5 in front of a wall at z = 0, staggered in x so that rays cross every combination; each screen
    is a mesh, a material and an instance of its own, so leaving one out changes nothing about the others"""
    s = scenes.Scene(name="cutout_screens")

    def const_tex(alpha):
        s.textures.append(scenes.Texture(rgba=np.tile(np.uint8([200, 120, 60, alpha]), (4, 4, 1)), srgb=True))
        return len(s.textures) - 1

    def textured(tex, flags):
        m = abi.make_material((0.8, 0.8, 0.8), flags=flags)
        abi.set_float_bits(m.base_color, 0, 0x80000000 | tex)
        return m

    kinds = {A64: lambda: textured(const_tex(64), 0), A191: lambda: textured(const_tex(191), 0),
             NOALPHA0: lambda: textured(const_tex(0), abi.BASE_MATERIAL_NOALPHA), LITERAL: lambda: abi.make_material((0.9, 0.5, 0.1), flags=0)}
    place = {A64: (2.0, -1.6, 0.4), A191: (1.5, -0.9, 1.1), NOALPHA0: (1.0, -0.2, 1.8), LITERAL: (0.5, -1.2, 0.1)}  # z, x0, x1

    def add(tris, uvs, material):
        nrm = np.tile(np.float32([0, 0, 1]), (len(tris), 3, 1))
        mesh = scenes._add_mesh(s, np.float32(tris), nrm, np.float32(uvs))
        s.materials.append(material)
        s.pmeshes.append(scenes.ParameterizedMesh(mesh=mesh, material_offsets=np.array([len(s.materials) - 1], np.int32)))
        s.instances.append(scenes.Instance(transform=scenes.IDENTITY.copy(), pmesh=len(s.pmeshes) - 1))

    uv = [[[0, 0], [3, 0], [3, 2]], [[0, 0], [3, 2], [0, 2]]]
    for kind in (A64, A191, NOALPHA0, LITERAL):
        if kind in screens:
            z, x0, x1 = place[kind]
            add(scenes._quad((x0, -0.7, z), (x1, -0.7, z), (x1, 1.3, z), (x0, 1.3, z)), uv, kinds[kind]())
    if wall:
        add(scenes._quad((-2.5, -1.5, 0), (2.5, -1.5, 0), (2.5, 2.0, 0), (-2.5, 2.0, 0)), uv, abi.make_material((0.7, 0.7, 0.7)))
    s.camera = dict(eye=(0, 0.5, 5), center=(0, 0.3, 0), up=(0, 1, 0), fov=45.0)
    s.config = scenes.SceneConfig(**scenes.SKY_CONFIGS["low_sun"])
    s.sky_key = "low_sun"
    s.prepare_lights()
    return s


def test_cutout_bits_are_the_opaque_bits_of_the_scene_without_what_the_cutoff_ignores():
    everything = (A64, A191, NOALPHA0, LITERAL)
    q = _rays(6000, 404, (-2.0, -1.0, 0.1), (2.0, 1.6, 3.0))
    q[:, 6] = -np.abs(q[:, 6])  # towards the screens and the wall
    handles = {name: renderer(_screens_scene(keep, wall), 64, 48) for name, keep, wall in (
        ("all", everything, True), ("without 64", (A191, NOALPHA0, LITERAL), True), ("without both", (NOALPHA0, LITERAL), True),
        ("only the two solid", (NOALPHA0, LITERAL), False))}
    opaque = {name: _bits_of(h, q) for name, h in handles.items()}
    full = handles["all"]
    cut = {c: _bits_of(full, q, alpha_cutoff=c) for c in (0.2, 0.5, 0.9, 1.0)}
    for h in handles.values():
        h.close()
    # (the scenes differ where the rule can show: each textured alpha screen decides some rays alone)
    assert (opaque["all"] & ~opaque["without 64"]).sum() > 50 and (opaque["without 64"] & ~opaque["without both"]).sum() > 50
    assert (~opaque["all"]).sum() > 50
    for c, want in ((0.2, "all"), (0.5, "without 64"), (0.9, "without both"), (1.0, "without both")):
        print("cutoff %.1f: %d occluded, differs from the opaque bits of the scene '%s' in %d" % (c, int(cut[c].sum()), want, int((cut[c] != opaque[want]).sum())))
        assert np.array_equal(cut[c], opaque[want]), c
    # the NOALPHA screen (whatever its texel says) and the literal colour (alpha 1) occlude at every cutoff
    assert opaque["only the two solid"].sum() > 200
    for c in cut:
        assert not (opaque["only the two solid"] & ~cut[c]).any(), c


# ---------------------------------------------------------------- 5. the cutout rule on fractional texels: properties
def test_cutout_on_fractional_texels_is_monotonic_and_a_subset_of_opaque():
    s = scenes.alpha_test()
    r = renderer(s, 64, 48)
    q = _rays(8000, 55, (-2.0, 0.05, -1.0), (2.0, 2.5, 3.0))
    opaque = _bits_of(r, q)
    counted = r.trace_counted(q, tmin=None, any_hit=True)[0][:, 0] != 0
    assert np.array_equal(opaque, counted)  # the flag clear
    cut = [_bits_of(r, q, alpha_cutoff=c) for c in (0.25, 0.5, 0.75)]
    again = _bits_of(r, q, alpha_cutoff=0.5)
    r.close()
    print("occluded: opaque %d, cutoff 0.25 / 0.5 / 0.75: %d / %d / %d" % ((int(opaque.sum()),) + tuple(int(c.sum()) for c in cut)))
    for c in cut:
        assert not (c & ~opaque).any()  # cutout is a subset of opaque
    assert not (cut[1] & ~cut[0]).any() and not (cut[2] & ~cut[1]).any()  # a higher cutoff never occludes a clear ray
    assert np.array_equal(again, cut[1])  # deterministic
    assert cut[2].sum() < cut[1].sum() < cut[0].sum() < opaque.sum()  # (the rays do cross cut-outs and fractional texels)


# ---------------------------------------------------------------- 6. moved instances
def test_bits_follow_moved_instances_like_a_fresh_scene():
    def scene(moved):
        s = scenes.two_level_test()
        for m in s.meshes:
            m.dynamic = abi.MESH_INSTANCES_MOVE
        for k, M in moved.items():
            s.instances[k].transform = M.copy()
        return s

    s = scene({})
    movable = [k for k, inst in enumerate(s.instances) if inst.pmesh != 2][:4]  # (parameterized mesh 2 emits: its instances stay)
    rng = np.random.default_rng(9)
    moved = {}
    for k in movable:
        M = s.instances[k].transform.copy()
        M[:, 3] = rng.uniform(-4, 4, 3).astype(np.float32)
        M[:, :3] = M[:, :3] @ np.float32([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])  # a quarter turn as well
        moved[k] = M
    q = _rays(6000, 66, (-5, -5, -5), (5, 5, 5))
    r = renderer(s, 64, 48)
    before = _bits_of(r, q)
    for k, M in moved.items():
        r.update_instances(k, M[None])
    r.refit()
    after = _bits_of(r, q)
    assert np.array_equal(after, _closest_hit(r, q))
    r.close()
    fresh = renderer(scene(moved), 64, 48)
    want = _bits_of(fresh, q)
    fresh.close()
    print("occluded before / after the move: %d / %d, %d bits changed" % (int(before.sum()), int(after.sum()), int((before != after).sum())))
    assert (before != after).sum() > 20
    assert np.array_equal(after, want)


# ---------------------------------------------------------------- 7. frames in flight and isolation
def test_a_run_beside_a_frame_in_flight_is_right_and_leaves_the_frame_alone():
    s = scenes.two_level_test()
    W, H = 96, 64
    cam = s.camera_params()
    q = _rays(3000, 12, (-5, -5, -5), (5, 5, 5))
    r = renderer(s, W, H)
    want = _bits_of(r, q)
    r.close()

    def run(with_queries):
        r = renderer(s, W, H, frames_in_flight=2)
        t0 = r.render_async(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=2)
        if with_queries:  # submitted and not waited for: the run waits for it
            assert np.array_equal(_bits_of(r, q), want)
        else:
            r.wait(t0)
        st = raw_stats(r)
        out = read_frame(r, W, H), (st.spp, int(st.rays_closest), int(st.rays_shadow), int(st.hits_shaded))
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_images(a[0], b[0])
    assert a[1] == b[1] and a[1][0] == 2


def test_a_run_on_an_idle_handle_leaves_images_and_stats_alone():
    s = scenes.two_level_test()
    W, H = 96, 64
    cam = s.camera_params()
    q = _rays(W * H + 50, 2, (-5, -5, -5), (5, 5, 5))
    r = renderer(s, W, H)
    r.render(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=2)
    before, first = raw_stats(r), read_frame(r, W, H)
    assert _bits_of(r, q).any()
    assert bytes(before) == bytes(raw_stats(r)) and before.spp == 2 and before.rays_closest > 0
    assert same_images(first, read_frame(r, W, H))
    r.close()


def test_an_occlusion_run_between_a_surface_and_a_closest_run_starts_from_a_fresh_cursor():
    """more queries than the static pools hold (tests/test_gpu_query_entries.py): each of the three runs must reset the borrowed cursor"""
    s = scenes.two_level_test()
    r = backend.RenderHip(frames_in_flight=4, options={"traverse_fetch": 64})
    r.initialize(64, 64)
    r.set_scene(s)
    grid = max(r.get_option("traversal_grid_shared"), r.get_option("traversal_grid_alone"))
    n = grid * 4 * 64 + 10000
    assert 0 < grid and n <= 2_500_000
    q = _rays(n, 11, (-6, -6, -6), (6, 6, 6))
    cam = s.camera_params()
    surf = r.render_surface_queries(q, cam)
    occ = _bits_of(r, q)
    closest = r.render_ray_queries(q, np.full((n, 4), np.float32(7.0), np.float32))
    r.close()
    assert not (closest == np.float32(7.0)).all(axis=1).any()  # every slot written
    hit = closest.view(np.int32)[:, 3] >= 0
    assert np.array_equal(occ, hit)
    # (the surface run's interval starts at 0, the other two at eps |origin|: a hit closer than that is the one difference allowed)
    differ = (surf["t"] >= 0) != hit
    assert differ.sum() <= 2 and (surf["t"][differ] < 1e-4).all()
    assert hit.sum() > 1000 and (~hit).sum() > 1000
