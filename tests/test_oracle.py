"""CPU tests that pin the oracle: the reference-derived known answers that exist
(SURVEY 8c), golden vectors produced by the reference's own code (oracle/_ref),
the reference's only value-bearing test (rendering/tests/gltf_bsdf.cpp, ported as
a property test) and domain properties for the parts that are "parity unpinned"."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import _p
from realtimepathtracingresearchframework_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- RNG (pinned)
def test_rng_known_answer_from_survey():
    # get_lcg_rng(3, 7, (10,20,256,256)) then one lcg_randomf:
    # state = 1349923967, f = 0.314303666 (state printed after the first draw)
    st, fl = O.rng_probe(3, 7, 10, 20, 256, 2)
    after_first = (st * 1664525 + 1013904223) & 0xFFFFFFFF
    assert after_first == 1349923967
    assert abs(float(fl[0]) - 0.314303666) < 5e-9
    assert fl[0] == np.float32(np.ldexp(np.float32(1349923967), -32))


def test_rng_float_can_reach_one_and_is_ldexp():
    # lcg_randomf = ldexp(float(u32), -32): u32 >= 0xFFFFFF80 rounds to 2^32 -> exactly 1.0f (lcg_rng.glsl:23-26)
    assert np.float32(np.ldexp(np.float32(0xFFFFFFFF), -32)) == np.float32(1.0)


# ---------------------------------------------------------------- quantisation
def test_quantize_numpy_equals_oracle_and_round_trips(oracle):
    rng = np.random.default_rng(0)
    p = rng.uniform(-30, 50, (5000, 3)).astype(np.float32)
    lo, hi = p.min(0), p.max(0)
    ext = (hi - lo).astype(np.float32)
    q_np = scenes.quantize_positions(p, ext, lo)
    q_c = np.zeros(len(p), np.uint64)
    oracle.lib().orc_quantize_positions(_p(p), len(p), _p(ext), _p(lo), _p(q_c))
    assert np.array_equal(q_np, q_c)
    sc, of = scenes.dequantization_scaling(ext), scenes.dequantization_offset(lo, ext)
    d_np = scenes.dequantize_positions(q_np, sc, of)
    d_c = np.zeros_like(p)
    oracle.lib().orc_dequantize_positions(_p(q_c), len(p), _p(sc), _p(of), _p(d_c))
    assert np.array_equal(d_np, d_c)
    # bin-centre reconstruction: error <= half a bin (+ rounding)
    assert np.all(np.abs(d_np - p) <= ext / 2 ** 21 * 0.5 + 1e-5)
    # maximum / minimum coordinates stay in range
    assert (q_np & np.uint64(0x1FFFFF)).max() <= 0x1FFFFF


def test_quantize_normals_uvs_numpy_equals_oracle(oracle):
    rng = np.random.default_rng(1)
    n = rng.normal(size=(4000, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)  # exactly representable axes
    uv = np.stack([rng.uniform(0, 7.9, 4000), rng.uniform(-6.9, 1.0, 4000)], axis=1).astype(np.float32)  # representable range
    packed = np.zeros(len(n), np.uint64)
    oracle.lib().orc_quantize_normal_uv(_p(n), _p(uv), len(n), _p(packed))
    mine = scenes.quantize_normals(n).astype(np.uint64) | (scenes.quantize_uvs(uv).astype(np.uint64) << np.uint64(32))
    assert np.array_equal(mine, packed)
    dn = np.zeros_like(n)
    duv = np.zeros_like(uv)
    oracle.lib().orc_dequantize_normal_uv(_p(packed), len(n), _p(dn), _p(duv))
    assert np.all(np.sum(dn * n, axis=1) > 0.9999)
    assert np.allclose(dn[:6], n[:6], atol=1e-6)  # "represent 0, -1 and 1 precisely" (quantize.h:20)
    assert np.all(np.abs(duv - uv) <= 8.0 / 65535 * 0.5 + 1e-6)


# ---------------------------------------------------------------- sky (pinned by oracle/_ref golden vectors)
def test_sky_eval_matches_reference_c_evaluation_for_zenith_sun(oracle):
    d = json.load(open(scenes.sky_fixture_path()))["entries"]["default"]
    sky = abi.SkyModelParams()
    for i in range(9):
        sky.configs[i][:] = d["configs"][i]
    sky.radiances[:] = d["radiances"]
    cos_t = np.array(d["eval_cos_theta"])
    dirs = np.stack([np.sqrt(1 - cos_t ** 2), cos_t, np.zeros_like(cos_t)], axis=1).astype(np.float32)
    out = np.zeros_like(dirs)
    sun = (C.c_float * 3)(*d["sun_dir"])
    oracle.lib().orc_sky_radiance(C.byref(sky), sun, _p(dirs), len(dirs), _p(out))
    ref = np.array(d["eval_rgb_times_100"]) * 0.01  # sky_model.glsl:58 scales by 0.01
    assert np.allclose(out, ref, rtol=2e-4, atol=1e-6)


@pytest.mark.parametrize("key", ["grid", "low_sun", "forest", "night"])
def test_sky_eval_matches_reference_c_evaluation_on_equal_angle_directions(oracle, key):
    """every sky configuration of the package data, not only the zenith sun: on the directions whose angle to the zenith equals their
    angle to the sun the shader's formula (which uses the zenith angle in the exp(C4 * gamma) term, sky_model.glsl:46-48) and the
    reference's C evaluation arhosek_tristim_skymodel_radiance(theta, gamma = theta) must agree"""
    d = json.load(open(scenes.sky_fixture_path()))["entries"][key]
    sky = abi.SkyModelParams()
    for i in range(9):
        sky.configs[i][:] = d["configs"][i]
    sky.radiances[:] = d["radiances"]
    dirs = np.array(d["eval_equal_angle_dirs"], np.float32)
    assert len(dirs) >= 10
    out = np.zeros_like(dirs)
    sun = (C.c_float * 3)(*d["sun_dir"])
    oracle.lib().orc_sky_radiance(C.byref(sky), sun, _p(dirs), len(dirs), _p(out))
    ref = np.array(d["eval_equal_angle_rgb_times_100"]) * 0.01
    if key == "night":  # sun below the horizon: the reference's fit itself yields NaN coefficients -- reproduced, not fixed
        assert np.array_equal(np.isnan(out), np.isnan(ref))
    else:
        assert np.isfinite(ref).all() and (ref > 0).all()
    assert np.allclose(out, ref, rtol=5e-4, atol=2e-6, equal_nan=True), np.nanmax(np.abs(out - ref))


def test_sky_fixture_is_physical():
    e = json.load(open(scenes.sky_fixture_path()))["entries"]
    for key, d in e.items():
        assert abs(np.linalg.norm(d["sun_dir"]) - 1) < 1e-6
        assert abs(d["sun_cos_angle"] - np.cos(np.radians(0.53) / 2)) < 1e-7
        if d["sun_dir"][1] > 0:
            assert all(v > 0 for v in d["sun_radiance_nolights"][:3]) and d["sun_radiance_lights"][3] == 0.5
        else:
            assert d["sun_radiance_nolights"] == [0.0, 0.0, 0.0, 1.0]  # render_sky.cpp:64-70
            assert d["sun_radiance_lights"][3] == 0.0


# ---------------------------------------------------------------- glTF BSDF (reference's own test, ported)
@pytest.mark.parametrize("metal", [False, True])
def test_gltf_bsdf_reference_stress_property(oracle, metal):
    """rendering/tests/gltf_bsdf.cpp:23-75: material (0.5 grey, specular 0.2, roughness 0.1, ior 1.5),
    random n / w_o / samples: no NaN in value, pdf, mis_pdf; weights are < 2 for almost all samples."""
    rng = np.random.default_rng(42)
    N = 200000
    m = abi.make_material((0.5, 0.5, 0.5), roughness=0.1, specular=0.2, metallic=1.0 if metal else 0.0, ior=1.5)
    n = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    wo = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    flip = np.sum(n * wo, axis=1) < 0
    wo[flip] *= -1
    u = rng.uniform(0, 1, (N, 4)).astype(np.float32)
    wi, w, f = (np.zeros((N, 3), np.float32) for _ in range(3))
    pdf, mis, wpdf = (np.zeros(N, np.float32) for _ in range(3))
    oracle.lib().orc_gltf_sample(C.byref(m), _p(n), _p(wo), _p(u), N, _p(wi), _p(w), _p(pdf), _p(mis), _p(f), _p(wpdf))
    ok = pdf > 0
    assert ok.mean() > 0.9
    assert np.isfinite(w[ok]).all() and np.isfinite(pdf[ok]).all() and np.isfinite(mis[ok]).all()
    assert (w[ok] < 2.0).all(axis=1).mean() > 0.99
    # internal consistency: weight * pdf == f * |cos|, sampled direction is unit length and above the surface
    cos_i = np.abs(np.sum(n * wi, axis=1))
    assert np.allclose(w[ok] * pdf[ok, None], f[ok] * cos_i[ok, None], rtol=2e-4, atol=1e-6)
    assert np.allclose(np.linalg.norm(wi[ok], axis=1), 1.0, atol=1e-4)
    assert (np.sum(n * wi, axis=1)[ok] > 0).all()


def test_gltf_wpdf_integrates_to_one_and_bsdf_conserves_energy(oracle):
    rng = np.random.default_rng(7)
    N = 400000
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (N, 1))
    for rough, metallic in ((0.5, 0.0), (0.3, 1.0), (0.9, 0.0)):
        m = abi.make_material((0.8, 0.8, 0.8), roughness=rough, metallic=metallic, ior=1.5)
        wo = np.tile(np.array([[0.5, 0.0, np.sqrt(0.75)]], np.float32), (N, 1))
        f = np.zeros((N, 3), np.float32)
        wpdf = np.zeros(N, np.float32)
        oracle.lib().orc_gltf_eval(C.byref(m), _p(nrm), _p(wo), _p(d), N, _p(f), _p(wpdf))
        upper = d[:, 2] > 0
        # the MIS pdf is a density over the upper hemisphere
        integral = float(np.mean(np.where(upper, wpdf, 0.0)) * 4 * np.pi)
        assert abs(integral - 1.0) < 0.03, (rough, metallic, integral)
        # albedo <= 1: integral f cos over the hemisphere
        albedo = np.mean(np.where(upper[:, None], f * d[:, 2:3], 0.0), axis=0) * 4 * np.pi
        assert (albedo < 1.02).all() and (albedo > 0.05).all(), albedo
        # no transmission lobe in the shipped megakernel build
        assert (f[~upper] == 0).all() and (wpdf[~upper] == 0).all()


# ---------------------------------------------------------------- glTF BSDF with the transmission lobe (RPTR_VARIANT_GLTF_TRANSMISSION)
def _gltf_t_sample(oracle, m, n, wo, u):
    N = len(n)
    wi, w, f = (np.zeros((N, 3), np.float32) for _ in range(3))
    pdf, mis, wpdf = (np.zeros(N, np.float32) for _ in range(3))
    oracle.lib().orc_gltf_t_sample(C.byref(m), _p(n), _p(wo), _p(u), N, _p(wi), _p(w), _p(pdf), _p(mis), _p(f), _p(wpdf))
    return wi, w, pdf, mis, f, wpdf


def _random_frames(rng, N, both_sides):
    n = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    wo = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    if not both_sides:
        flip = np.sum(n * wo, axis=1) < 0
        wo[flip] *= -1
    return n, wo, rng.uniform(0, 1, (N, 4)).astype(np.float32)


def test_transmission_build_without_transmission_equals_the_shipped_bsdf(oracle):
    """specular_transmission == 0: the build with GLTF_SUPPORT_TRANSMISSION gives the same samples, values and pdfs as the shipped
    two-lobe build, bit for bit (w_o above the surface: the shipped build returns nothing from below, gltf_bsdf.glsl:507-512)"""
    rng = np.random.default_rng(5)
    N = 50000
    n, wo, u = _random_frames(rng, N, both_sides=False)
    for metallic, rough in ((0.0, 0.3), (1.0, 0.1), (0.4, 0.8)):
        m = abi.make_material((0.6, 0.5, 0.4), roughness=rough, metallic=metallic, ior=1.5)
        wi, w, pdf, mis, f, wpdf = _gltf_t_sample(oracle, m, n, wo, u)
        wi0, w0, f0 = (np.zeros((N, 3), np.float32) for _ in range(3))
        pdf0, mis0, wpdf0 = (np.zeros(N, np.float32) for _ in range(3))
        oracle.lib().orc_gltf_sample(C.byref(m), _p(n), _p(wo), _p(u), N, _p(wi0), _p(w0), _p(pdf0), _p(mis0), _p(f0), _p(wpdf0))
        for a, b in ((wi, wi0), (w, w0), (pdf, pdf0), (mis, mis0), (f, f0), (wpdf, wpdf0)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("onesided", [False, True])
def test_transmission_lobe_properties(oracle, onesided):
    """glass (ior 1.5, specular_transmission 0.9): no NaN; weight * pdf == f * |cos| (the sampler and the evaluation agree); the
    transmission component crosses the surface, the other two do not; refraction through a ONESIDED surface obeys Snell's law
    about the sampled half vector; seen from inside (w_o below n) it works with 1/ior; weights stay bounded"""
    rng = np.random.default_rng(9)
    N = 200000
    flags = abi.BASE_MATERIAL_NOALPHA | (abi.BASE_MATERIAL_ONESIDED if onesided else 0)
    m = abi.make_material((0.9, 0.95, 1.0), roughness=0.25, metallic=0.0, ior=1.5, flags=flags)
    m.specular_transmission = 0.9
    m.clearcoat_gloss = 0.04            # reflection roughness = sqrt(clearcoat_gloss) = 0.2 (gltf_bsdf.glsl:54-55)
    n, wo, u = _random_frames(rng, N, both_sides=onesided)
    wi, w, pdf, mis, f, wpdf = _gltf_t_sample(oracle, m, n, wo, u)
    ok = pdf > 0
    assert ok.mean() > (0.6 if onesided else 0.85)       # (from inside, total internal reflection leaves no transmitted direction)
    assert np.isfinite(w[ok]).all() and np.isfinite(pdf[ok]).all() and np.isfinite(mis[ok]).all() and np.isfinite(wi[ok]).all()
    cos_i = np.sum(n * wi, axis=1)
    cos_o = np.sum(n * wo, axis=1)
    assert np.allclose(w[ok] * pdf[ok, None], f[ok] * np.abs(cos_i[ok, None]), rtol=5e-4, atol=1e-6)
    assert np.allclose(np.linalg.norm(wi[ok], axis=1), 1.0, atol=2e-4)
    through = ok & (cos_i * cos_o < 0)
    assert 0.2 < through.sum() / ok.sum() < 0.95         # most of the energy of clear glass goes through
    assert (w[ok] < 4.0).all(axis=1).mean() > 0.98
    assert (mis[ok] > 0).mean() > 0.99
    if onesided:
        # Snell: the tangential parts of w_o and w_i about the half vector h ~ -(eta_i w_i + eta_o w_o) have the ratio of the indices
        outside = cos_o > 0
        ior = np.where(outside, 1.5, 1.0 / 1.5)[:, None]
        h = -(ior * wi + wo)
        h /= np.linalg.norm(h, axis=1, keepdims=True)
        sin_o = np.linalg.norm(wo - h * np.sum(wo * h, axis=1, keepdims=True), axis=1)
        sin_i = np.linalg.norm(wi - h * np.sum(wi * h, axis=1, keepdims=True), axis=1)
        sel = through & (sin_o > 0.05)
        assert np.allclose(sin_o[sel], ior[sel, 0] * sin_i[sel], rtol=2e-3, atol=2e-4)
    else:
        # thin surface: the transmitted direction is the mirror image (about the surface) of a reflection
        refl = wi - 2 * cos_i[:, None] * n
        assert (np.sum(refl * n, axis=1)[through] * cos_o[through] > 0).all()


# ---------------------------------------------------------------- sun + triangle lights
def test_sun_samples_lie_in_the_cone(oracle):
    rng = np.random.default_rng(3)
    u = rng.uniform(0, 1, (10000, 2)).astype(np.float32)
    sd = np.array([0.3, 0.8, 0.5], np.float32)
    sd /= np.linalg.norm(sd)
    cosr = np.float32(np.cos(np.radians(0.53) / 2))
    dirs = np.zeros((len(u), 3), np.float32)
    pdf = C.c_float()
    oracle.lib().orc_sample_sun((C.c_float * 3)(*sd), C.c_float(cosr), _p(u), len(u), _p(dirs), C.byref(pdf))
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1, atol=1e-5)
    assert (dirs @ sd >= cosr - 1e-6).all()
    assert abs(pdf.value * 2 * np.pi * (1 - float(cosr)) - 1) < 1e-4


def test_tri_light_sampling_hits_the_chosen_light(oracle):
    """one light per bin (bin_size 1): samples land inside that triangle, pdf = 1/(bins * solid angle)."""
    s = scenes.cornell32()
    osc = O.OracleScene(s)
    cfg = abi.LightSamplingConfig(0.0, 1, 15.0, 0.0)
    rng = np.random.default_rng(5)
    N = 4000
    p = np.tile(np.array([[0.1, -0.2, 0.3]], np.float32), (N, 1))
    n = np.tile(np.array([[0, 1, 0]], np.float32), (N, 1))
    u = rng.uniform(0, 1, (N, 4)).astype(np.float32)
    L, d = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    dist, pdf, mis = (np.zeros(N, np.float32) for _ in range(3))
    oracle.lib().orc_sample_tri_lights.argtypes = None
    oracle.lib().orc_sample_tri_lights(C.c_void_p(osc.h), C.byref(cfg), _p(p), _p(n), _p(u), N, _p(L), _p(d), _p(dist), _p(pdf), _p(mis))
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-4)
    hitp = p + d * dist[:, None]
    assert np.allclose(hitp[:, 1], 0.995, atol=1e-3)                 # on the light plane
    assert (np.abs(hitp[:, 0]) <= 0.2501).all() and (np.abs(hitp[:, 2]) <= 0.2501).all()  # inside the quad
    lights = s.lights
    for k in range(2):
        sel = (u[:, 2] * 2).astype(int).clip(0, 1) == k
        v = lights[k, :3] - p[0]
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        # exact solid angle (Van Oosterom & Strackee)
        num = abs(np.dot(v[0], np.cross(v[1], v[2])))
        den = 1 + v[0] @ v[1] + v[1] @ v[2] + v[0] @ v[2]
        omega = 2 * np.arctan2(num, den)
        assert np.allclose(pdf[sel], 1.0 / (2 * omega), rtol=2e-3)   # fast atan: 1.16e-5 abs error
        assert np.allclose(L[sel] * pdf[sel, None], lights[k, 3], rtol=1e-5)


# ---------------------------------------------------------------- ray queries: BVH == brute force
@pytest.mark.parametrize("scene_fn", [scenes.cornell32, scenes.two_level_test])
def test_bvh_traversal_equals_brute_force_bitwise(scene_fn):
    s = scene_fn()
    osc = O.OracleScene(s)
    rng = np.random.default_rng(11)
    n = 6000
    o = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:50, 0] = 0  # axis-parallel rays (safe reciprocal path)
    d[50:100, 1] = 0
    tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
    tuv_t, ids_t = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_OWN)
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32))
    assert np.array_equal(ids_b, ids_t)
    assert (ids_b[:, 0] >= 0).sum() > 100
    # any-hit agrees with "a closest hit exists", also for clipped intervals
    tmax = np.where(tuv_b[:, 0] > 0, tuv_b[:, 0] * rng.choice([0.5, 1.5], n), 5.0).astype(np.float32)
    any_b = osc.trace_ex(o, d, 1e-4, tmax, any_hit=True, bvh_mode=O.BVH_BRUTE)[1][:, 0]
    any_t = osc.trace_ex(o, d, 1e-4, tmax, any_hit=True, bvh_mode=O.BVH_OWN)[1][:, 0]
    clo = osc.trace_ex(o, d, 1e-4, tmax, bvh_mode=O.BVH_BRUTE)[1][:, 0] >= 0
    assert np.array_equal(any_b, any_t) and np.array_equal(any_b.astype(bool), clo)


def test_rt_intersect_semantics(oracle):
    """vulkan/rt_intersect.comp:31-68: miss record, mode<0 leaves the slot untouched, custom index + geometry index."""
    s = scenes.two_level_test()
    osc = O.OracleScene(s)
    q = np.zeros((3, 8), np.float32)
    q[0, :3], q[0, 4:7], q[0, 7] = (0, 50, 0), (0, 1, 0), 1e20      # points away: miss
    q[1, :3], q[1, 4:7], q[1, 7] = (0, 0, 20), (0, 0, -1), 1e20
    q[1, 3] = np.array([-1], np.int32).view(np.float32)[0]           # skipped
    q[2, :3], q[2, 4:7], q[2, 7] = (0, 0, 20), (0, 0, -1), 1e20
    out = np.full((3, 4), 7.0, np.float32)
    oracle.lib().orc_trace(C.c_void_p(osc.h), O.BVH_OWN, _p(q), 3, _p(out), None)
    assert out[0, 0] == -1 and out[0, 1] == -1 and out[0, 2:].view(np.int32).tolist() == [-1, -1]
    assert (out[1] == 7.0).all()


# ---------------------------------------------------------------- images
def test_render_bvh_equals_brute_force_image():
    s = scenes.cornell32()
    osc = O.OracleScene(s)
    a, sa = osc.render(48, 48, 2, bvh_mode=O.BVH_BRUTE)
    b, sb = osc.render(48, 48, 2, bvh_mode=O.BVH_OWN)
    assert np.array_equal(a, b) and sa.rays_closest == sb.rays_closest and sa.rays_shadow == sb.rays_shadow


def test_running_mean_accumulation_is_order_exact():
    """process_samples.comp:116-132: N spp at once == N single-sample frames folded one by one; tiles compose."""
    s = scenes.cornell32()
    osc = O.OracleScene(s)
    full, _ = osc.render(40, 32, 3)
    acc = np.zeros_like(full)
    for k in range(3):
        acc, _ = osc.render(40, 32, 1, sample_begin=k, accum=acc)
    assert np.array_equal(full, acc)
    top, _ = osc.render(40, 32, 3, rows=(0, 16))
    both, _ = osc.render(40, 32, 3, rows=(16, 32), accum=top)
    assert np.array_equal(full, both)


def test_white_furnace_diffuse_energy_bound():
    """closed diffuse box, albedo 0.5, no lights, sun below horizon: radiance is 0 (no energy from nowhere)."""
    s = scenes.cornell32()
    for m in s.materials:
        m.emission_intensity = 0.0
    s.sky_key = "night"
    s.prepare_lights()
    osc = O.OracleScene(s)
    img, _ = osc.render(32, 32, 2, variant=abi.VARIANT_SIMPLE)
    # night sky is dark but not black (Hosek below horizon mirrors upward): bounded and finite
    assert np.isfinite(img).all() and img[..., :3].max() < 50.0


def test_alpha_channel_marks_geometry():
    s = scenes.grid(40, 20)
    osc = O.OracleScene(s)
    img, st = osc.render(64, 36, 1, variant=abi.VARIANT_SIMPLE)
    assert set(np.unique(img[..., 3])) <= {0.0, 1.0}  # pt_megakernel.glsl:736
    assert 0.2 < img[..., 3].mean() < 0.9


# ---------------------------------------------------------------- host light preparation (a20)
def test_halton2_and_bin_equalisation_invariants():
    from realtimepathtracingresearchframework_amd import lights as L
    assert [float(L.halton2(i)) for i in range(5)] == [0.0, 0.5, 0.25, 0.75, 0.125]
    rng = np.random.default_rng(9)
    n = 37
    em = np.zeros((n, 4, 3), np.float32)
    for i in range(n):
        c = rng.uniform(-5, 5, 3)
        em[i, 0], em[i, 1], em[i, 2] = c, c + rng.normal(size=3) * 0.3, c + rng.normal(size=3) * 0.3
        em[i, 3] = rng.uniform(0.1, 1) * (100.0 if i == 3 else 1.0)   # one dominant emitter gets cloned
    out, rad = L.update_light_sampling(em, bin_size=16)
    assert len(out) >= n and len(out) == len(rad)
    # total radiance of every source emitter is preserved by cloning (radiance / split_count per clone)
    src_total = em[:, 3].sum(axis=0)
    assert np.allclose(out[:, 3].sum(axis=0), src_total, rtol=1e-4)
    # every output triangle is one of the inputs
    keys = {tuple(np.round(e[:3].reshape(-1), 5)) for e in em}
    assert all(tuple(np.round(e[:3].reshape(-1), 5)) in keys for e in out)


def test_cornell_lights_are_the_two_ceiling_triangles():
    s = scenes.cornell32()
    assert s.num_tris() == 32 and len(s.lights) == 2
    assert np.allclose(s.lights[:, 3], 15.0)
    assert np.allclose(s.lights[:, :3, 1], 0.995, atol=1e-5)


def test_dynamic_vertices_rebuild_equals_brute_force():
    """orc_scene_set_dynamic_vertices: float positions override the quantised stream in the builder, the brute-force
    loop and the hit attributes (pt_megakernel.glsl:526-529)."""
    s = scenes.grid(24, 12, deform_t=0.0)
    osc = O.OracleScene(s)
    rng = np.random.default_rng(2)
    n = 4000
    o = rng.uniform(-55, 55, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(3, 8, n)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 1] = -np.abs(d[:, 1])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    before = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_OWN)[0]
    P = scenes.grid_positions(24, 12, 0.3)
    osc.set_dynamic_vertices(0, P)
    tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
    tuv_t, ids_t = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_OWN)
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t)
    assert not np.array_equal(before, tuv_t) and (ids_t[:, 0] >= 0).sum() > 1000
    # hit points lie on the deformed surface: y(hit) within the new vertex range of the hit triangle
    hit = ids_t[:, 0] >= 0
    y = o[hit, 1] + tuv_t[hit, 0] * d[hit, 1]
    tri = P.reshape(-1, 3, 3)[ids_t[hit, 2]]
    assert (y >= tri[:, :, 1].min(axis=1) - 1e-3).all() and (y <= tri[:, :, 1].max(axis=1) + 1e-3).all()


# ---------------------------------------------------------------- textures (a8 / a9)
def test_texture_sampling_semantics():
    """textureLod(.., 0) with linear filter + REPEAT: texel centres reproduce the texels, the midpoint of two texels is
    their mean, coordinates wrap, sRGB textures are decoded before filtering (alpha stays linear)."""
    s = scenes.textured_test()
    osc = O.OracleScene(s)
    t0, t1 = s.textures[0].rgba, s.textures[1].rgba           # 16x8 sRGB, 8x8 linear
    h, w = t1.shape[:2]
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    centres = np.stack([(ix + 0.5) / w, (iy + 0.5) / h], axis=2).reshape(-1, 2)
    got = osc.texture_probe(1, centres).reshape(h, w, 4)
    assert np.array_equal(got, t1.astype(np.float32) / np.float32(255.0))
    # wrap: +3 / -2 periods (up to the rounding of the coordinate itself)
    assert np.allclose(osc.texture_probe(1, centres + np.array([3.0, -2.0])).reshape(h, w, 4), got, atol=2e-6)
    # midpoint between texel (0,0) and (1,0)
    mid = osc.texture_probe(1, [[1.0 / w, 0.5 / h]])[0]
    assert np.allclose(mid, (t1[0, 0].astype(np.float32) + t1[0, 1].astype(np.float32)) / 510.0, atol=1e-6)
    # across the border: texel (w-1, 0) and (0, 0)
    edge = osc.texture_probe(1, [[0.0, 0.5 / h]])[0]
    assert np.allclose(edge, (t1[0, -1].astype(np.float32) + t1[0, 0].astype(np.float32)) / 510.0, atol=1e-6)
    # sRGB decode at texel centres
    h0, w0 = t0.shape[:2]
    c = osc.texture_probe(0, [[(3 + 0.5) / w0, (2 + 0.5) / h0]])[0]
    e = t0[2, 3].astype(np.float64) / 255.0
    lin = np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)
    assert np.allclose(c[:3], lin[:3], rtol=1e-5) and c[3] == 1.0
    assert np.array_equal(osc.texture_probe(0, [[0.5 / w0, 0.5 / h0]])[0, 3:], [1.0])


def test_textured_parameters_change_the_render_and_bad_handles_are_rejected():
    s = scenes.textured_test()
    osc = O.OracleScene(s)
    img, _ = osc.render(96, 72, 2, variant=abi.VARIANT_GLTF)
    assert np.isfinite(img).all()
    flat = scenes.textured_test()
    for m in flat.materials:                    # same scene without the normal map
        m.normal_map = -1
    img2, _ = O.OracleScene(flat).render(96, 72, 2, variant=abi.VARIANT_GLTF)
    assert not np.array_equal(img, img2)
    bad = scenes.textured_test()
    bad.materials[0].normal_map = 17            # not a texture of the scene
    with pytest.raises(AssertionError):
        O.OracleScene(bad).render(32, 32, 1)


# ---------------------------------------------------------------- alpha-tested geometry (a5)
def test_alpha_test_semantics():
    """pt_megakernel.glsl:153-212: alpha 1 everywhere = opaque (no candidate rejected, no number drawn); alpha 0 everywhere =
    the geometry is not there; fractional alphas lie in between; NOALPHA materials are never tested."""
    W, H, spp = 96, 72, 4
    base = scenes.alpha_test()
    img, st = O.OracleScene(base).render(W, H, spp)
    assert np.isfinite(img).all()

    def variant(alpha=None, noalpha=False, drop_cutouts=False):
        s = scenes.alpha_test()
        if alpha is not None:
            for t in s.textures:
                t.rgba[..., 3] = alpha
        if noalpha:
            for m in s.materials:
                m.flags |= abi.BASE_MATERIAL_NOALPHA
        if drop_cutouts:       # instances 0..2 use the textured cut-out materials only (screens); 3 = per-triangle mix, stays
            s.instances = s.instances[3:]
        return s
    opaque_tex, _ = O.OracleScene(variant(alpha=255)).render(W, H, spp)
    opaque_flag, _ = O.OracleScene(variant(alpha=255, noalpha=True)).render(W, H, spp)
    assert np.array_equal(opaque_tex, opaque_flag)
    # NOALPHA wins over the texture's alpha channel
    flagged, _ = O.OracleScene(variant(noalpha=True)).render(W, H, spp)
    assert np.array_equal(flagged[..., :3] > -1, opaque_flag[..., :3] > -1) and not np.array_equal(flagged, img)
    # the image with cut-outs differs from both extremes
    assert not np.array_equal(img, opaque_tex)


def test_fully_transparent_screens_equal_the_scene_without_them():
    """alpha 0: every candidate of the screens is ignored and no random number is consumed, so the paths are those of the
    scene without the screens (closest hits do not depend on the tree; the per-triangle-material screen is kept in both)"""
    W, H, spp = 96, 72, 2
    a = scenes.alpha_test()
    for t in a.textures:
        t.rgba[..., 3] = 0
    a.instances = [a.instances[i] for i in (0, 1, 2, 4, 5, 6)]      # without the mixed screen (it has an opaque material)
    a.prepare_lights()
    b = scenes.alpha_test()
    b.instances = [b.instances[i] for i in (4, 5, 6)]                # literal-colour quad, room, light
    b.prepare_lights()
    ia, _ = O.OracleScene(a).render(W, H, spp)
    ib, _ = O.OracleScene(b).render(W, H, spp)
    # instance ids differ between the two scenes, which only enters the seeds of rejected-or-not shadow candidates: none here
    assert np.array_equal(ia, ib)


# ---------------------------------------------------------------- AOV images (vulkan/accumulate.glsl:76-103)
def test_aov_semantics():
    s = scenes.textured_test()
    W, H = 96, 72
    osc = O.OracleScene(s)
    img, _, (albedo, normal, motion) = osc.render(W, H, 2, aovs=True)
    plain, _ = osc.render(W, H, 2)
    assert np.array_equal(img, plain)                                  # writing AOVs does not disturb the image
    n = normal.astype(np.float32)
    hit = np.isfinite(n[..., 3])
    assert 0.5 < hit.mean() < 1.0                                      # sky pixels: depth = |2e32 - cam| overflows to inf, normal 0
    assert np.all(n[~hit][:, :3] == 0) and np.all(albedo.astype(np.float32)[~hit] == [0, 0, 0, 1])
    assert np.allclose(np.linalg.norm(n[hit][:, :3], axis=1), 1.0, atol=2e-3)
    a = albedo.astype(np.float32)[hit]
    assert a[:, :3].min() >= 0 and a[:, :3].max() <= 1.0 and 0 < a[:, 3].min() and a[:, 3].max() <= 1.0
    # depth is the distance of the first hit from the camera: compare with a ray query through the pixel centre is off by the
    # jitter, so only bound it by the scene size
    assert n[hit][:, 3].min() > 0.5 and n[hit][:, 3].max() < 20
    # static view: no motion
    m = motion.astype(np.float32)
    assert np.all(m[hit] == 0)
    # the SIMPLE variant reports roughness 1 (ior == 1)
    _, _, (albedo_s, _, _) = osc.render(W, H, 1, variant=abi.VARIANT_SIMPLE, aovs=True)
    assert np.all(albedo_s.astype(np.float32)[hit][:, 3] == 1.0)
    # only the first sample of a frame writes: a frame that starts at sample 2 writes its own AOVs (another jitter)
    _, _, (_, normal2, _) = osc.render(W, H, 1, sample_begin=2, aovs=True, accum=img.copy())
    assert not np.array_equal(normal2, normal)


def test_aov_motion_vectors_follow_the_previous_view():
    """motion.xy = projection of the hit point with the previous frame's VP minus its projection with this frame's
    (accumulate.glsl:76-87), in the clip units of render_vulkan.cpp:2926-2931 (x to the right, y down after GLToVulkan)"""
    s = scenes.textured_test()
    W, H = 64, 48
    cam = s.camera_params()
    prev = s.camera_params()
    prev.pos[0] -= 0.25                                                # the camera moved 0.25 to the right since the last frame
    _, _, (_, normal, motion) = O.OracleScene(s).render(W, H, 1, aovs=True, prev_camera=prev)
    m, n = motion.astype(np.float32), normal.astype(np.float32)
    hit = np.isfinite(n[..., 3])
    # points in front of a camera that moved right appear further right in the previous view... (they moved left on screen)
    assert (m[hit][:, 0] > 0).mean() > 0.99 and np.abs(m[hit][:, 1]).max() < 0.05
    # nearer points move more: motion.x ~ P00 * 0.25 / view depth
    depth_order = np.argsort(n[hit][:, 3])
    near, far = m[hit][depth_order[:200], 0].mean(), m[hit][depth_order[-200:], 0].mean()
    assert near > far > 0
    assert np.all(m[..., 2:] == 0)


def test_halton_table_of_the_screen_jitter():
    """the (2, 3) Halton table behind view_params.screen_jitter (render_vulkan.cpp:2917-2926): regenerated at six decimals; equals
    librender/halton.h entry by entry where the reference tree is at hand"""
    import os, re
    assert O.halton23(0).tolist() == [0.5, np.float32(0.333333)] and O.halton23(7).tolist() == [0.0625, np.float32(0.888889)]
    ref = "/root/reference/librender/halton.h"
    if os.path.exists(ref):
        rows = re.findall(r"\{\s*([0-9.]+)f,\s*([0-9.]+)f\s*\}", open(ref).read())
        assert len(rows) == 64
        for i, (a, b) in enumerate(rows):
            assert O.halton23(i).tolist() == [np.float32(a), np.float32(b)], i


def _mip_chain(level0):
    """box-filtered levels 1.. down to 1 x 1 (test data: the product generates none)"""
    out, cur = [], level0.astype(np.float64)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = max(1, cur.shape[0] // 2), max(1, cur.shape[1] // 2)
        cur = cur[:2 * h if cur.shape[0] > 1 else 1, :2 * w if cur.shape[1] > 1 else 1]
        cur = cur.reshape(h, cur.shape[0] // h, w, cur.shape[1] // w, 4).mean(axis=(1, 3))
        out.append(np.clip(np.round(cur), 0, 255).astype(np.uint8))
    return out


def test_texture_sampler_lod_and_anisotropy():
    """the material sampler as restated after the Vulkan specification (oshade.h texture_grad / texture_lod): zero derivatives = bilinear
    level 0; an isotropic footprint of 4 texels = level 2; fractional levels blend; an 8 : 1 footprint = 8 taps of level 0 along the major
    axis at uv + ddx (i / 9 - 1/2); levels beyond the chain and single-level textures clamp"""
    rng = np.random.default_rng(5)
    s = scenes.textured_test()
    base = rng.integers(0, 256, (16, 16, 4)).astype(np.uint8)
    s.textures.append(scenes.Texture(rgba=base, srgb=False, mips=_mip_chain(base)))
    s.textures.append(scenes.Texture(rgba=base, srgb=False))
    full, single = len(s.textures) - 2, len(s.textures) - 1
    osc = O.OracleScene(s)
    uv = rng.random((64, 2)).astype(np.float32) * 3 - 1
    zero = np.zeros_like(uv)
    assert np.array_equal(osc.texture_grad(full, uv, zero, zero), osc.texture_probe(full, uv))
    assert np.array_equal(osc.texture_lod(full, uv, 0.0), osc.texture_probe(full, uv))
    # level 2 of the chain is a 4 x 4 texture: sample it through a scene texture of its own
    lv = s.textures[full].levels()
    s2 = scenes.textured_test()
    s2.textures.append(scenes.Texture(rgba=lv[2], srgb=False))
    s2.textures.append(scenes.Texture(rgba=lv[1], srgb=False))
    o2 = O.OracleScene(s2)
    l2, l1 = o2.texture_probe(len(s2.textures) - 2, uv), o2.texture_probe(len(s2.textures) - 1, uv)
    iso = np.tile(np.array([[4 / 16, 0.0]], np.float32), (len(uv), 1))
    assert np.array_equal(osc.texture_grad(full, uv, iso, iso[:, ::-1].copy()), l2)
    assert np.array_equal(osc.texture_lod(full, uv, 2.0), l2)
    assert np.allclose(osc.texture_lod(full, uv, 1.25), 0.75 * l1 + 0.25 * l2, atol=2e-7)
    assert np.array_equal(osc.texture_lod(full, uv, 40.0), osc.texture_lod(full, uv, 4.0))         # the 1 x 1 level
    assert np.allclose(osc.texture_lod(full, uv, 4.0), lv[4].reshape(1, 4) / 255.0, atol=1e-7)
    # anisotropy 8: rho = (8, 1) texels -> eta = 8, N = 8, lod = log2(8 / 8) = 0
    ddx = np.tile(np.array([[8 / 16, 0.0]], np.float32), (len(uv), 1))
    ddy = np.tile(np.array([[0.0, 1 / 16]], np.float32), (len(uv), 1))
    taps = [osc.texture_probe(full, uv + ddx * np.float32(np.float32(i) / np.float32(9) - np.float32(0.5))) for i in range(1, 9)]
    assert np.allclose(osc.texture_grad(full, uv, ddx, ddy), np.mean(taps, axis=0), atol=3e-7)
    # beyond anisotropy 12 the level rises: rho = (48, 1) -> eta = 12, lod = log2(4) = 2, 12 taps of level 2
    ddx48 = ddx * np.float32(6)
    taps = [o2.texture_probe(len(s2.textures) - 2, uv + ddx48 * np.float32(np.float32(i) / np.float32(13) - np.float32(0.5))) for i in range(1, 13)]
    assert np.allclose(osc.texture_grad(full, uv, ddx48, ddy), np.mean(taps, axis=0), atol=3e-7)
    # one level: every lod is level 0, the taps stay
    assert np.array_equal(osc.texture_lod(single, uv, 3.0), osc.texture_probe(single, uv))
    assert np.array_equal(osc.texture_grad(single, uv, iso, iso[:, ::-1].copy()), osc.texture_probe(single, uv))


def test_footprint_functions():
    """rendering/rt/footprint.glsl: F = J J^T of the pixel's differentials in the ray's tangent frame; footprint_to_dpdxy returns its
    principal axes (minor first); a mirror reflection keeps the eigenvalues"""
    rng = np.random.default_rng(9)
    for _ in range(50):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        a = np.cross(d, rng.normal(size=3))
        a /= np.linalg.norm(a)
        b = np.cross(d, a)
        la, lb = rng.uniform(0.01, 0.2), rng.uniform(0.3, 0.9)
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        dst = d - 2 * np.dot(d, n) * n
        F, px, py, R = O.footprint_probe(d, a * la, b * lb, dst)
        ev = np.sort(np.linalg.eigvalsh(F.astype(np.float64)))
        assert np.allclose(ev, [la * la, lb * lb], rtol=2e-4) and abs(F[0, 1] - F[1, 0]) < 1e-7
        assert np.isclose(np.linalg.norm(px), la, rtol=2e-3) and np.isclose(np.linalg.norm(py), lb, rtol=2e-3)
        assert abs(np.dot(px, d)) < 1e-5 and abs(np.dot(py, d)) < 1e-5 and abs(np.dot(px, py)) < 1e-4
        assert np.isclose(abs(np.dot(px / np.linalg.norm(px), a)), 1.0, atol=2e-3)
        assert np.allclose(np.sort(np.linalg.eigvalsh(R.astype(np.float64))), ev, rtol=2e-3)


def test_cpu_baseline_build_of_the_oracle_renders_the_same_bits():
    """bench.py's cpu_baseline is the oracle's own sources built -O3 without their diagnostics (oracle/Makefile libcpu_baseline.so:
    -DORC_BASELINE, 32 x 32 tiles instead of row segments): same image bit for bit, same ray counts -- a glTF scene with emitters and a
    two-level scene -- and faster than the instrumented build."""
    import oracle_lib as O
    from realtimepathtracingresearchframework_amd import abi, scenes
    out = {}
    try:
        for name, path in (("oracle", None), ("baseline", O.build_baseline())):
            O.use_library(path)
            for key, s in (("grid", scenes.grid(60, 30, with_emitters=True)), ("two_level", scenes.two_level_test())):
                osc = O.OracleScene(s)
                osc.build_bvh()
                img, st = osc.render(96, 64, 2, variant=abi.VARIANT_GLTF, threads=4)
                out[(name, key)] = (img, int(st.rays_closest), int(st.rays_shadow), st.seconds)
    finally:
        O.use_library(None)
    for key in ("grid", "two_level"):
        a, b = out[("oracle", key)], out[("baseline", key)]
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:3] == b[1:3]
