"""Surface queries (rptr_hip_trace_surface*, RenderHip.render_surface_queries): position, normals and material at a query ray's closest
hit. Against the oracle the queries ARE the camera rays of a frame and the records are compared with its AOV images (the oracle has no
query entry); indices are compared with rptr_hip_trace_counted, untextured materials with the scene's material table, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from common import aov_close, float_bits, probe_queries, raw_stats, read_frame, renderer, same_images
from realtimepathtracingresearchframework_amd import abi, backend, scenes
from surface_query_cases import CASES, primary_rays, scene

pytestmark = pytest.mark.gpu

DT = abi.SURFACE_HIT_DTYPE


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _miss_record():
    m = np.zeros(1, DT)
    m["t"], m["instance_geometry"], m["primitive"], m["material_id"], m["roughness"], m["ior"] = -1.0, -1, -1, -1, 1.0, 1.0
    return m


# ---------------------------------------------------------------- 1. camera rays against the oracle's AOV images
@pytest.mark.parametrize("name,variant,W,H", CASES)
def test_camera_ray_records_match_the_oracles_aov_images(name, variant, W, H):
    """the records of the oracle's own primary rays of sample 0, laid out as the normal + depth and the albedo + roughness image, against
    the images of OracleScene.render(aovs=True); the sky pixels are the miss texels (normal 0 at an infinite depth; albedo 0, roughness 1)"""
    s = scene(name)
    osc = O.OracleScene(s)
    q, _ = primary_rays(osc, s, W, H, variant)
    _, _, aovs = osc.render(W, H, 1, variant=variant, aovs=True)
    r = renderer(s, W, H)
    cam = s.camera_params()
    res = r.render_surface_queries(q, cam, variant=variant)
    r.close()
    hit = res["t"] >= 0
    assert np.array_equal(_bytes(res[~hit]), np.repeat(_bytes(_miss_record()), int((~hit).sum()), axis=0))
    assert hit.any() and (res["t"][hit] > 0).all()
    nd = np.zeros((W * H, 4), np.float32)
    nd[:, 0:3] = res["normal"]
    with np.errstate(over="ignore"):
        depth = np.linalg.norm(res["position"] - np.asarray(list(cam.pos), np.float32), axis=1).astype(np.float32)
        nd[:, 3] = np.where(hit, depth, np.float32(np.inf))
        nd16 = nd.astype(np.float16).reshape(H, W, 4)
    ar = np.zeros((W * H, 4), np.float32)
    ar[:, 0:3] = res["base_color"]
    ar[:, 3] = np.where(res["ior"] != 1.0, res["roughness"], np.float32(1.0))
    aov_close(nd16, aovs[1], "%s normal + depth" % name)
    aov_close(ar.astype(np.float16).reshape(H, W, 4), aovs[0], "%s albedo + roughness" % name)
    # the miss pattern itself: where the oracle's depth is not finite the query missed, and nowhere else
    sky = ~np.isfinite(aovs[1][..., 3].astype(np.float32)).reshape(-1)
    assert (sky == ~hit).mean() > 0.9995
    assert (aovs[0].reshape(-1, 4)[sky & ~hit] == np.float16([0, 0, 0, 1])).all() and (aovs[1].reshape(-1, 4)[sky & ~hit, 0:3] == 0).all()


# ---------------------------------------------------------------- 2. indices and interval
@pytest.mark.parametrize("name", ["cornell32", "two_level_test"])
def test_indices_hits_and_positions_are_those_of_the_closest_hit_query(name):
    """instance_geometry, primitive and hit / miss == rptr_hip_trace_counted over (0, t_max), bit for bit; position == origin + t dir per
    coordinate within 2^-22 (|o| + |t d|) (one product and one sum, fused or not, plus a margin); 0 < t < t_max"""
    s = scene(name)
    r = renderer(s, 64, 48)
    q = probe_queries(6000, seed=7, short=True) if name == "cornell32" else probe_queries(6000, seed=8, spread=4.0, centre=(0, 0, 0), short=True)
    res = r.render_surface_queries(q, s.camera_params())
    ref, _ = r.trace_counted(q, tmin=np.zeros(len(q), np.float32))
    r.close()
    ids = ref.view(np.int32)
    hit = ids[:, 3] >= 0
    print("%s: %d hits, %d misses, %d of the short rays hit" % (name, hit.sum(), (~hit).sum(), hit[1::2].sum()))
    assert hit.sum() > 300 and (~hit).sum() > 100 and hit[1::2].sum() > 50 and (~hit[1::2]).any()  # (the probes cover every case)
    assert np.array_equal(res["t"] >= 0, hit)
    assert np.array_equal(res["instance_geometry"], ids[:, 2]) and np.array_equal(res["primitive"], ids[:, 3])
    assert np.array_equal(_bytes(res[~hit]), np.repeat(_bytes(_miss_record()), int((~hit).sum()), axis=0))
    t = res["t"][hit]
    assert (t > 0).all() and (t < q[hit, 7]).all()
    o, d = q[hit, 0:3].astype(np.float64), q[hit, 4:7].astype(np.float64)
    td = t.astype(np.float64)[:, None] * d
    err = np.abs(res["position"][hit].astype(np.float64) - (o + td))
    bound = 2.0 ** -22 * (np.abs(o) + np.abs(td))
    print("position: worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    # both normals have unit length and the geometric one faces the ray (no material of these scenes is one-sided)
    gn, nn = res["geo_normal"][hit].astype(np.float64), res["normal"][hit].astype(np.float64)
    assert np.allclose(np.linalg.norm(gn, axis=1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(nn, axis=1), 1.0, atol=1e-5)
    assert ((gn * -d).sum(axis=1) >= 0).all() and ((nn * -d).sum(axis=1) >= 0).all()


# ---------------------------------------------------------------- 3. untextured materials are exact
def _material_table(s):
    m = s.materials
    return (np.array([list(x.base_color) for x in m], np.float32), np.array([x.roughness for x in m], np.float32), np.array([x.ior for x in m], np.float32),
            np.array([x.metallic for x in m], np.float32), np.array([x.emission_intensity for x in m], np.float32))


def test_untextured_materials_are_the_scenes_bit_for_bit():
    """cornell32, glTF program: roughness, ior, metallic and base_color of every hit are the float32 fields of materials[material_id]
    (base_color 0 where the material emits: the record's own rule, as in the albedo AOV)"""
    s = scenes.cornell32()
    r = renderer(s, 64, 48)
    q = probe_queries(6000, seed=21)
    res = r.render_surface_queries(q, s.camera_params(), variant=abi.VARIANT_GLTF)
    r.close()
    base, rough, ior, metal, emi = _material_table(s)
    h = res[res["t"] >= 0]
    mid = h["material_id"]
    assert len(h) > 3000 and mid.min() >= 0 and mid.max() < len(s.materials) and len(np.unique(mid)) == len(s.materials)
    emits = emi[mid] != 0
    assert emits.any() and (~emits).any()
    assert np.array_equal(float_bits(h["base_color"]), float_bits(np.where(emits[:, None], np.float32(0), base[mid])))
    assert np.array_equal(float_bits(h["roughness"]), float_bits(rough[mid])) and np.array_equal(float_bits(h["ior"]), float_bits(ior[mid]))
    assert np.array_equal(float_bits(h["metallic"]), float_bits(metal[mid]))
    assert np.array_equal(float_bits(h["emission"]), float_bits(base[mid] * emi[mid][:, None]))
    assert (h["uv"] == 0).all()  # (the scene has no texture coordinates)


def test_emission_is_the_emitters_radiance_and_its_base_color_is_zero():
    """the emitter grid: emission == float32(base_color) * float32(emission_intensity), non-zero on exactly the hits whose material emits,
    where base_color is 0; the diffuse program reports roughness 1, ior 1, metallic 0"""
    s = scenes.grid(120, 60, with_emitters=True)
    r = renderer(s, 64, 48)
    rng = np.random.default_rng(5)
    n = 8000
    q = np.zeros((n, 8), np.float32)
    q[:, 0] = rng.uniform(-44, 44, n)
    q[:, 1] = 4.0
    q[:, 2] = rng.uniform(-21, 21, n)
    # upwards at the emissive quads 2 units above (every 16th of the plane is one), or down at the height field
    d = np.stack([rng.uniform(-0.1, 0.1, n), np.where(np.arange(n) % 4 == 3, -1.0, 1.0), rng.uniform(-0.1, 0.1, n)], axis=1)
    q[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    q[:, 7] = 1e20
    base, _, _, _, emi = _material_table(s)
    for variant in (abi.VARIANT_SIMPLE, abi.VARIANT_GLTF):
        res = r.render_surface_queries(q, s.camera_params(), variant=variant)
        h = res[res["t"] >= 0]
        mid = h["material_id"]
        emits = emi[mid] != 0
        print("variant %d: %d hits, %d of them on emitters" % (variant, len(h), emits.sum()))
        assert emits.sum() > 20 and (~emits).sum() > 1000
        assert np.array_equal(float_bits(h["emission"]), float_bits(base[mid] * emi[mid][:, None]))
        assert np.array_equal((h["emission"] != 0).any(axis=1), emits)
        assert (h["base_color"][emits] == 0).all() and np.array_equal(float_bits(h["base_color"][~emits]), float_bits(base[mid[~emits]]))
        if variant == abi.VARIANT_SIMPLE:
            assert (h["roughness"] == 1).all() and (h["ior"] == 1).all() and (h["metallic"] == 0).all()
    r.close()


# ---------------------------------------------------------------- 4. shapes
def test_counts_skipped_slots_and_prefixes():
    """n = 1, 63, 65, 257, 6913: every third record skipped (mode_or_data = -1) keeps a sentinel pattern bit for bit, and every prefix gives
    the records of the full run; n = 0 writes nothing"""
    s = scenes.two_level_test()
    r = renderer(s, 64, 48)
    cam = s.camera_params()
    N = 6913
    q = probe_queries(N, seed=31, spread=5.0, centre=(0, 0, 0))
    q.view(np.int32)[0::3, 3] = -1
    sentinel = np.frombuffer(bytes(range(7, 7 + 96)), dtype=DT)[0]
    full = np.full(N, sentinel, DT)
    r.render_surface_queries(q, cam, results=full)
    skipped = np.zeros(N, bool)
    skipped[0::3] = True
    assert np.array_equal(_bytes(full[skipped]), np.repeat(_bytes(np.array([sentinel])), int(skipped.sum()), axis=0))
    assert (_bytes(full[~skipped]) != _bytes(np.array([sentinel]))).any(axis=1).all()
    assert (full["t"][~skipped] > 0).sum() > 500
    for n in (1, 63, 65, 257):
        part = np.full(n, sentinel, DT)
        r.render_surface_queries(q[:n], cam, results=part)
        assert np.array_equal(_bytes(part), _bytes(full[:n])), n
    # a prefix that skips nothing, too (the slot of query 0 is written)
    q2 = q.copy()
    q2.view(np.int32)[:, 3] = 0
    whole = r.render_surface_queries(q2, cam)
    assert np.array_equal(_bytes(whole[~skipped]), _bytes(full[~skipped]))
    assert np.array_equal(_bytes(r.render_surface_queries(q2[:1], cam)), _bytes(whole[:1]))
    # n = 0
    guard = np.full(4, sentinel, DT)
    assert r._L.rptr_hip_trace_surface(r._h, q.ctypes.data_as(C.c_void_p), 0, C.byref(cam), abi.VARIANT_GLTF, guard.ctypes.data_as(C.c_void_p)) == abi.RPTR_OK
    assert np.array_equal(_bytes(guard), np.repeat(_bytes(np.array([sentinel])), 4, axis=0))
    r.close()


# ---------------------------------------------------------------- 5. device entry
def test_device_entry_budget_and_refusals():
    """device buffers on a caller's stream, and the enable_ray_queries buffer (device_queries = NULL): the records of the host-array call;
    over budget, world_size 2, before set_scene / initialize: the documented codes"""
    import torch
    s = scenes.textured_test()
    cam = s.camera_params()
    r = renderer(s, 64, 48)
    n = 4001
    q = probe_queries(n, seed=4, spread=1.5, centre=(0.0, 1.5, 0.0))
    d = q[:, 4:7].copy()
    d[:, 1] = -np.abs(d[:, 1])  # towards the textured ground
    q[:, 4:7] = d
    host = r.render_surface_queries(q, cam)
    assert (host["t"] > 0).sum() > 1000
    tq = torch.from_numpy(q).cuda()
    tr = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.render_surface_queries_device(n, cam, device_queries=tq.data_ptr(), device_results=tr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(_bytes(host), tr.cpu().numpy().view(np.uint8).reshape(n, -1))
    # the backend's query buffer, on the backend's stream
    dq, _ = r.enable_ray_queries_device(n)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dq, q.ctypes.data_as(C.c_void_p), q.nbytes, 1) == 0
    tr2 = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_surface_queries_device(n, cam, device_results=tr2.data_ptr())
    r.render_ray_queries(q[:1])  # (a synchronous call on the backend's stream: the run above has finished)
    assert np.array_equal(_bytes(host), tr2.cpu().numpy().view(np.uint8).reshape(n, -1))

    def refused(code, what, call):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == code and what in str(e.value), str(e.value)

    refused(abi.RPTR_E_INVALID, "exceed the budget", lambda: r.render_surface_queries_device(n + 1, cam, device_results=tr2.data_ptr()))
    refused(abi.RPTR_E_INVALID, "unknown variant", lambda: r.render_surface_queries(q, cam, variant=17))
    refused(abi.RPTR_E_INVALID, "NULL query or output buffer", lambda: r.render_surface_queries_device(n, cam, device_queries=tq.data_ptr()))
    r.close()
    r = backend.RenderHip()
    refused(abi.RPTR_E_INVALID, "before set_scene", lambda: r.render_surface_queries(q, cam))
    r.close()
    r = backend.RenderHip()
    r.set_scene(s)
    refused(abi.RPTR_E_INVALID, "before initialize", lambda: r.render_surface_queries(q, cam))
    r.close()
    r = backend.RenderHip(rank=0, world_size=2)
    r.initialize(64, 48)
    r.set_scene(s)
    refused(abi.RPTR_E_UNSUPPORTED, "world_size 1", lambda: r.render_surface_queries(q, cam))
    r.close()


# ---------------------------------------------------------------- 6. a run leaves the frame alone
def test_a_query_run_leaves_the_frame_alone():
    """frame, queries, frame == frame, frame: accumulation, RGBA8 frame, the three AOV images; rptr_hip_stats is the same before and after
    the run"""
    s = scenes.two_level_test()
    W, H = 96, 64
    cam = s.camera_params()
    q = probe_queries(W * H + 50, seed=2, spread=5.0, centre=(0, 0, 0))

    def run(with_queries):
        r = renderer(s, W, H)
        cfg = backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True)
        r.render(cfg, spp=2)
        if with_queries:
            before, first = raw_stats(r), read_frame(r, W, H)
            res = r.render_surface_queries(q, cam)
            assert (res["t"] > 0).any()
            assert bytes(before) == bytes(raw_stats(r)) and before.spp == 2 and before.rays_closest > 0
            assert same_images(first, read_frame(r, W, H))
        cfg.reset_accumulation = False
        st = r.render(cfg, spp=2)
        out = read_frame(r, W, H), (st.spp, int(st.raw.rays_closest), int(st.raw.rays_shadow), int(st.raw.hits_shaded))
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_images(a[0], b[0])
    assert a[1] == b[1] and a[1][0] == 4


def test_a_query_run_between_submission_and_wait_leaves_two_frames_in_flight_alone():
    """two frames in flight, the query run between their submission and the wait: the run waits for both (it borrows a frame context's
    cursor and stack scratch), the images and statistics are those of the run without queries"""
    s = scenes.two_level_test()
    W, H = 96, 64
    cam = s.camera_params()
    q = probe_queries(3000, seed=12, spread=5.0, centre=(0, 0, 0))

    def run(with_queries):
        r = renderer(s, W, H, frames_in_flight=2)
        t0 = r.render_async(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=2)
        t1 = r.render_async(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_GLTF, reset_accumulation=False), spp=2)
        if with_queries:
            res = r.render_surface_queries(q, cam)
            assert (res["t"] > 0).any()
        else:
            r.wait(t0)
            r.wait(t1)
        st = raw_stats(r)
        out = read_frame(r, W, H), (st.spp, int(st.rays_closest), int(st.rays_shadow), int(st.hits_shaded))
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_images(a[0], b[0])
    assert a[1] == b[1] and a[1][0] == 4


# ---------------------------------------------------------------- 7. moved geometry
def test_queries_see_a_moved_instance():
    """two_level_test with movable instances: an instance translated with update_instances + refit is found at its new place (its index
    word, its material), the hit positions moved by the translation; the same rays before the move miss it"""
    s = scenes.two_level_test()
    for m in s.meshes:
        m.dynamic = abi.MESH_INSTANCES_MOVE
    r = renderer(s, 64, 48)
    cam = s.camera_params()
    k = 4  # an instance of parameterized mesh 1: index word 1 (one geometry per mesh), material 2
    assert s.instances[k].pmesh == 1 and int(s.pmeshes[1].material_offsets[0]) == 2
    a, move = np.float32([0, 0, 32]), np.float32([0, 16, 0])  # far from the other instances; exact in float32, like every sum below

    def at(centre):
        M = np.zeros((1, 3, 4), np.float32)
        M[0, :, :3] = np.eye(3, dtype=np.float32)
        M[0, :, 3] = centre
        return M

    def rays(centre):  # a 7 x 7 bundle straight down through the blob (triangle soup of +-1 or so around the centre)
        g = (np.arange(7, dtype=np.float32) - 3) * np.float32(0.125)
        q = np.zeros((49, 8), np.float32)
        q[:, 0], q[:, 2] = centre[0] + np.repeat(g, 7), centre[2] + np.tile(g, 7)
        q[:, 1], q[:, 5], q[:, 7] = centre[1] + np.float32(4), -1.0, 8.0
        return q

    assert (r.render_surface_queries(rays(a), cam)["t"] == -1).all() and (r.render_surface_queries(rays(a + move), cam)["t"] == -1).all()
    r.update_instances(k, at(a))
    r.refit()
    first = r.render_surface_queries(rays(a), cam)
    hit = first["t"] > 0
    assert hit.sum() >= 10
    assert (first["instance_geometry"][hit] == 1).all() and (first["material_id"][hit] == 2).all()
    assert (r.render_surface_queries(rays(a + move), cam)["t"] == -1).all()  # the rays at the new place, before the move
    r.update_instances(k, at(a + move))
    r.refit()
    moved = r.render_surface_queries(rays(a + move), cam)
    assert (r.render_surface_queries(rays(a), cam)["t"] == -1).all()
    r.close()
    assert np.array_equal(moved["t"] > 0, hit)
    for f in ("instance_geometry", "primitive", "material_id"):
        assert np.array_equal(moved[f], first[f]), f
    q1 = rays(a + move)[hit]
    want = first["position"][hit].astype(np.float64) + move
    err = np.abs(moved["position"][hit].astype(np.float64) - want)
    bound = 2.0 ** -22 * (np.abs(q1[:, 0:3].astype(np.float64)) + np.abs(moved["t"][hit].astype(np.float64)[:, None] * q1[:, 4:7]))
    print("moved positions: worst error %.3e, smallest bound %.3e" % (float(err.max()), float(bound[bound > 0].min())))
    assert (err <= bound).all()
    assert np.array_equal(float_bits(moved["geo_normal"]), float_bits(first["geo_normal"])) and np.array_equal(float_bits(moved["base_color"]), float_bits(first["base_color"]))
