"""Golden vectors from the reference's OWN shader library (rendering/*.glsl compiled as C++ against GLM by oracle/ref_shader_driver.cpp:
`make -C oracle ref_shaders GLM_ROOT=<dir>` writes tests/golden/ref_shaders.json) against the oracle's restatement of the same functions.

Ten of SURVEY 8(c)'s twelve vector groups come out of that one command (generator table, dequantisation, hit attributes, footprints, glTF and
Lambert BSDF, binned-RIS lights, sun cone, sky radiance, display transfer function; vkr transforms and the emitter bins' Halton table are
pinned by tests/test_vks.py / tests/test_oracle.py against the reference's own compiled code), plus next-event estimation end to end; the same
command writes tests/golden/ref_shade.json from oracle/ref_shade_driver.cpp: one whole shading step of the megakernel, shade_base_material, and
tests/golden/ref_lights.json from oracle/ref_lights_driver.cpp: librender/lights.cpp compiled unmodified, the emitter table (held against the product's
own lights.py).
This is the pin the oracle lacks for the functions that decide a pixel ("parity unpinned" for BSDFs and light
sampling). The build image has no GLM and the rules forbid stand-in headers, so the fixture cannot be produced here: until somebody runs
the one command on a machine that has GLM, every test in this file SKIPS with that reason. With the fixture present they need no GLM, no
reference checkout and no GPU (the GPU side is pinned through the oracle by the whole-frame parity tests).

Tolerance: the oracle fixes one evaluation order per GLSL built-in (oracle/ovec.h: dot = (xx' + yy') + zz', normalize = v * (1 / sqrt(dot)))
where GLM is free to choose another, so values are compared to 2e-5 relative (+ 1e-6 absolute), discrete decisions (which lobe, which
light) must agree except where an input lies within that tolerance of the decision boundary (at most 1 % of the vectors)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import _p
from realtimepathtracingresearchframework_amd import abi, scenes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_shaders.json")
pytestmark = pytest.mark.skipif(not os.path.exists(FIXTURE), reason="tests/golden/ref_shaders.json absent: it is written by `make -C oracle ref_shaders "
                                "GLM_ROOT=<dir with glm/glm.hpp>` from the reference's own rendering/*.glsl; this image has no GLM")
RTOL, ATOL = 2e-5, 1e-6


@pytest.fixture(scope="module")
def ref():
    return json.load(open(FIXTURE))


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return np.isclose(a, b, rtol=RTOL, atol=ATOL) | both_nan


def test_rng_against_the_references_generator(ref):
    state, first = O.rng_probe(3, 7, 10, 20, 256, n=1)   # (SURVEY 8a2's tuple: oracle/ref_shader_driver.cpp)
    assert int(state) == int(ref["rng"]["state"]) and np.float32(first[0]) == np.float32(ref["rng"]["first"])


def test_gltf_bsdf_sample_eval_pdf_against_the_references_functions(ref):
    L = O.lib()
    rows = ref["gltf"]
    bad = 0
    for r in rows:
        m = abi.BaseMaterial()
        m.base_color[:] = r["base_color"]
        m.normal_map = -1
        m.flags = abi.BASE_MATERIAL_NOALPHA
        m.metallic, m.specular, m.roughness, m.ior = r["metallic"], r["specular"], r["roughness"], r["ior"]
        n, wo = (np.array([r[k]], np.float32) for k in ("n", "wo"))
        u = np.array([r["u"]], np.float32)
        wi, w, f = (np.zeros((1, 3), np.float32) for _ in range(3))
        pdf, mis, wpdf = (np.zeros(1, np.float32) for _ in range(3))
        L.orc_gltf_sample(C.byref(m), _p(n), _p(wo), _p(u), 1, _p(wi), _p(w), _p(pdf), _p(mis), _p(f), _p(wpdf))
        ok = _close(wi[0], r["wi"]).all() and _close(w[0], r["weight"]).all() and _close(pdf[0], r["pdf"]) and _close(mis[0], r["mis_pdf"])
        wie = np.array([r["wi_eval"]], np.float32)
        fe, pe = np.zeros((1, 3), np.float32), np.zeros(1, np.float32)
        L.orc_gltf_eval(C.byref(m), _p(n), _p(wo), _p(wie), 1, _p(fe), _p(pe))
        assert _close(fe[0], r["f"]).all() and _close(pe[0], r["wpdf"]), r      # evaluation: no discrete decision, no excuse
        bad += 0 if ok else 1
    assert bad <= len(rows) // 100, "%d of %d sampled directions differ (lobe decisions at a boundary are the only excuse)" % (bad, len(rows))


def test_binned_ris_light_sampling_against_the_references_function(ref):
    L = O.lib()
    L.orc_sample_tri_lights.argtypes = None
    lights = np.array(ref["lights"], np.float32).reshape(-1, 4, 3)
    s = scenes.cornell32()
    s.lights = lights
    osc = O.OracleScene(s)
    bad = 0
    rows = ref["tri_lights"]
    for r in rows:
        cfg = abi.LightSamplingConfig(0.0, int(r["bin_size"]), 15.0, 0.0)
        p, n = (np.array([r[k]], np.float32) for k in ("p", "n"))
        u = np.array([r["u"]], np.float32)
        Lr, d = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)
        dist, pdf, mis = (np.zeros(1, np.float32) for _ in range(3))
        L.orc_sample_tri_lights(C.c_void_p(osc.h), C.byref(cfg), _p(p), _p(n), _p(u), 1, _p(Lr), _p(d), _p(dist), _p(pdf), _p(mis))
        ok = (_close(Lr[0], r["radiance_over_pdf"]).all() and _close(d[0], r["dir"]).all() and _close(dist[0], r["dist"]) and _close(pdf[0], r["pdf"])
              and _close(mis[0], r["mis_wpdf"]))
        bad += 0 if ok else 1
    assert bad <= len(rows) // 100, "%d of %d light samples differ" % (bad, len(rows))


# ---------------------------------------------------------------- the other vector groups of SURVEY 8(c) (round 6: the two drivers make eleven of twelve)
def test_rng_table_state_and_draw_order(ref):
    for r in ref["rng_table"]:
        state, draws = O.rng_probe(r["index"], r["frame_offset"], r["pixel"][0], r["pixel"][1], r["dims"][0], n=8)
        assert int(state) == int(r["state"]), r
        assert np.array_equal(np.asarray(draws, np.float32), np.asarray(r["draws"], np.float32)), r     # integer arithmetic + ldexp: exact, in order


def test_dequantisation_of_positions_normals_uvs(ref):
    L = O.lib()
    d = ref["dequant"]
    words = np.array([(w["hi"] << 32) | w["lo"] for w in d["words"]], np.uint64)
    sc, of = np.array(d["scaling"], np.float32), np.array(d["offset"], np.float32)
    pos, nrm, uv = np.zeros((len(words), 3), np.float32), np.zeros((len(words), 3), np.float32), np.zeros((len(words), 2), np.float32)
    L.orc_dequantize_positions(_p(words), len(words), _p(sc), _p(of), _p(pos))
    L.orc_dequantize_normal_uv(_p(words), len(words), _p(nrm), _p(uv))
    assert _close(pos, [w["position"] for w in d["words"]]).all()
    assert _close(nrm, [w["normal"] for w in d["words"]]).all() and _close(uv, [w["uv"] for w in d["words"]]).all()


def test_hit_attributes(ref):
    L = O.lib()
    L.orc_hit_attributes_probe.restype = C.c_int
    ids = np.array([0, 1, 2, 3], np.uint8)      # (the driver's id_4pack 0x03020100)
    for r in ref["hit_attributes"]:
        verts = np.array([r["va"], r["vb"], r["vc"]], np.float32)
        nuv = np.array([(hi << 32) | lo for lo, hi in r["nuv"]], np.uint64)
        n2w = np.array(r["normals_to_world"], np.float32)
        out = np.zeros(13, np.float32)
        mid = L.orc_hit_attributes_probe(_p(verts), _p(nuv), int(r["has_normals"]), int(r["has_uvs"]), _p(n2w), C.c_float(r["t"]), C.c_float(r["bary"][0]),
                                         C.c_float(r["bary"][1]), int(r["material_in"]), _p(ids), _p(out))
        assert mid == r["material_id"], r
        # degenerate triangles (every 9th / 11th is a sliver) amplify rounding in the tangent frame: those get the looser bound
        tol = dict(rtol=2e-3, atol=1e-5) if min(np.linalg.norm(np.subtract(r["vb"], r["va"])), np.linalg.norm(np.subtract(r["vc"], r["va"]))) < 1e-2 else dict(rtol=RTOL, atol=ATOL)
        for key, got in (("normal", out[0:3]), ("geo_normal", out[3:6]), ("tangent", out[6:9]), ("dist", out[9]), ("bitangent_l", out[10]), ("uv", out[11:13])):
            assert np.isclose(np.asarray(got, np.float64), np.asarray(r[key], np.float64), **tol).all(), (key, r)


def test_texture_footprints(ref):
    for r in ref["footprint"]:
        F, bx, by, R = O.footprint_probe(r["dir"], r["dpdx"], r["dpdy"], r["dst_dir"])     # (2 x 2 as rows; the driver prints column by column)
        assert _close(F.T.reshape(-1), r["footprint"]).all() and _close(bx, r["back_dpdx"]).all() and _close(by, r["back_dpdy"]).all()
        assert _close(R.T.reshape(-1), r["reflected"]).all(), r


def test_simple_bsdf(ref):
    L = O.lib()
    for r in ref["simple"]:
        a = {k: np.array(r[k], np.float32) for k in ("base_color", "n", "wo", "u", "wi_eval")}
        wi, w, f = (np.zeros(3, np.float32) for _ in range(3))
        pdf, mis, wpdf = (np.zeros(1, np.float32) for _ in range(3))
        L.orc_simple_probe(_p(a["base_color"]), _p(a["n"]), _p(a["wo"]), _p(a["u"]), _p(a["wi_eval"]), _p(wi), _p(w), _p(pdf), _p(mis), _p(f), _p(wpdf))
        assert _close(wi, r["wi"]).all() and _close(w, r["weight"]).all() and _close(pdf[0], r["pdf"]) and _close(mis[0], r["mis_pdf"]), r
        assert _close(f, r["f"]).all() and _close(wpdf[0], r["wpdf"]), r


def test_sun_cone_sampling(ref):
    L = O.lib()
    for r in ref["sun"]:
        sd, u = np.array(r["sun_dir"], np.float32), np.array([r["u"]], np.float32)
        d, pdf = np.zeros((1, 3), np.float32), np.zeros(1, np.float32)
        L.orc_sample_sun(_p(sd), C.c_float(r["cos_radius"]), _p(u), 1, _p(d), _p(pdf))
        # (1 - cos_radius cancels: the pdf of a 0.27-degree cone carries the rounding of cos_radius itself)
        assert _close(d[0], r["dir"]).all() and np.isclose(pdf[0], r["pdf"], rtol=1e-4), r


def test_sky_radiance_on_the_direction_grid(ref):
    L = O.lib()
    s = ref["sky"]
    sky = abi.SkyModelParams()
    flat = np.array(s["configs"], np.float32).reshape(-1)
    C.memmove(C.byref(sky), flat.ctypes.data, flat.nbytes)
    rad = np.array(s["radiances"], np.float32)
    C.memmove(C.byref(sky, flat.nbytes), rad.ctypes.data, rad.nbytes)
    dirs = np.array([g["dir"] for g in s["grid"]], np.float32)
    out = np.zeros_like(dirs)
    sd = np.array(s["sun_dir"], np.float32)
    L.orc_sky_radiance(C.byref(sky), _p(sd), _p(dirs), len(dirs), _p(out))
    assert np.isclose(out, np.array([g["radiance"] for g in s["grid"]]), rtol=1e-4, atol=1e-6).all()    # (exp / pow / acos of two maths libraries)


def test_display_transfer_function(ref):
    L = O.lib()
    x = np.array([v[0] for v in ref["srgb"]], np.float32)
    out = np.zeros_like(x)
    L.orc_linear_to_srgb(_p(x), len(x), _p(out))
    assert np.isclose(out, [v[1] for v in ref["srgb"]], rtol=1e-5, atol=1e-7).all()


def test_approx_tri_lights_pdf(ref):
    # lights_linear.glsl:129-137 with the driver's table: 40 lights in bins of 16 -> 3 bins
    for sa, pdf in ref["approx_tri_lights_pdf"]:
        assert np.isclose(np.float32(1.0) / (np.float32(3.0) * np.float32(sa)), pdf, rtol=1e-6)


def test_next_event_estimation_end_to_end(ref):
    """sample_direct_light (mc/nee.glsl:32-90): sun or triangle lights by the selection sample, the light's sample, MIS against the glTF BSDF's pdf,
    strict normals; every visibility query "visible" (the driver's stub = compile.cpp:39; here: the scene's geometry moved out of the way)"""
    L = O.lib()
    L.orc_sample_direct_light.argtypes = None
    nee = ref["nee"]
    s = scenes.cornell32()
    for inst in s.instances:
        inst.transform = inst.transform.copy()
        inst.transform[:, 3] += np.float32(1.0e4)
    s.lights = np.array(ref["lights"], np.float32).reshape(-1, 4, 3)
    osc = O.OracleScene(s)
    sp = abi.SceneParams()
    sp.sun_dir[:] = nee["sun_dir"]
    sp.sun_cos_angle = nee["sun_cos_angle"]
    sp.sun_radiance[:] = nee["sun_radiance"]
    cfg = abi.LightSamplingConfig(0.0, 16, 15.0, 0.0)
    bad = 0
    for r in nee["samples"]:
        m = abi.BaseMaterial()
        m.base_color[:] = r["base_color"]
        m.normal_map = -1
        m.flags = abi.BASE_MATERIAL_NOALPHA
        m.metallic, m.specular, m.roughness, m.ior = r["metallic"], r["specular"], r["roughness"], r["ior"]
        a = {k: np.array([r[k]], np.float32) for k in ("p", "gn", "n", "wo", "u")}
        out = np.zeros((1, 3), np.float32)
        L.orc_sample_direct_light(C.c_void_p(osc.h), C.byref(sp), C.byref(cfg), C.byref(m), _p(a["p"]), _p(a["gn"]), _p(a["n"]), _p(a["wo"]), _p(a["u"]), 1, _p(out))
        bad += 0 if _close(out[0], r["illum"]).all() else 1
    assert bad <= len(nee["samples"]) // 100, "%d of %d NEE samples differ (a selection at a bin / sun boundary is the only excuse)" % (bad, len(nee["samples"]))


SHADE_FIXTURE = os.path.join(os.path.dirname(FIXTURE), "ref_shade.json")


@pytest.mark.skipif(not os.path.exists(SHADE_FIXTURE), reason="tests/golden/ref_shade.json absent: written by the same `make -C oracle ref_shaders GLM_ROOT=...` "
                    "(oracle/ref_shade_driver.cpp: the megakernel's shading step compiled from the reference's files)")
def test_one_shading_step_end_to_end():
    """SURVEY 8(c) group (9): shade_megakernel -> shade_base_material (mc/shade_base_material.glsl:14-96) in the megakernel's configuration: unpack_material
    over the unrolled standard textures (1 x 1 texels = the literals handed to the oracle), direct emitter hit + MIS weight, path-depth cut, AOV channels,
    next-event estimation, glossy-only cut, BSDF sample, termination tests, throughput / prev_bounce_pdf, and the generator's state after the step --
    i.e. the NUMBER and ORDER of the draws (section 7.2-2)."""
    ref = json.load(open(SHADE_FIXTURE))
    L = O.lib()
    L.orc_shade_base_material.argtypes = None
    s = scenes.cornell32()
    for inst in s.instances:
        inst.transform = inst.transform.copy()
        inst.transform[:, 3] += np.float32(1.0e4)
    s.lights = np.array(ref["lights"], np.float32).reshape(-1, 4, 3)
    osc = O.OracleScene(s)
    sp = abi.SceneParams()
    sp.sun_dir[:] = ref["sun_dir"]
    sp.sun_cos_angle = ref["sun_cos_angle"]
    sp.sun_radiance[:] = ref["sun_radiance"]
    cfg = abi.LightSamplingConfig(ref["light_mis_angle"], int(ref["bin_size"]), ref["min_perceived_receiver_dist"], ref["min_radiance"])
    rp = abi.RenderParams.default()
    mats = (abi.BaseMaterial * len(ref["materials"]))()
    for m, r in zip(mats, ref["materials"]):
        m.base_color[:] = r["base_color"]
        m.normal_map = -1
        m.flags = abi.BASE_MATERIAL_NOALPHA
        m.metallic, m.specular, m.roughness, m.ior, m.emission_intensity = r["metallic"], r["specular"], r["roughness"], r["ior"], r["emission_intensity"]
    rows = ref["samples"]
    n = len(rows)
    fin = np.zeros((n, 26), np.float32)
    iin = np.zeros((n, 5), np.int32)
    for i, r in enumerate(rows):
        fin[i, :18] = np.concatenate([r[k] for k in ("p", "gn", "n", "v_x", "v_y", "w_o")])
        fin[i, 18], fin[i, 19] = r["prev_bounce_pdf"], r["approx_solid_angle"]
        fin[i, 20:23], fin[i, 23:26] = r["illum_in"], r["throughput_in"]
        iin[i] = (r["material"], r["bounce"], r["output_channel"], r["glossy_only_mode"], np.uint32(r["rng"]).astype(np.int32))
    iout = np.zeros((n, 3), np.int32)
    fout = np.zeros((n, 10), np.float32)
    L.orc_shade_base_material(C.c_void_p(osc.h), C.byref(rp), C.byref(sp), C.byref(cfg), mats, _p(fin), _p(iin), n, _p(iout), _p(fout))
    bad, seen = 0, set()
    for i, r in enumerate(rows):
        ok = int(iout[i, 0]) == r["result"] and int(iout[i, 1]) == r["bounce_out"] and int(np.int32(iout[i, 2]).astype(np.uint32)) == r["rng_out"]
        ok = ok and _close(fout[i, 0:3], r["illum"]).all()
        if ok and r["result"] == 1:
            ok = _close(fout[i, 3:6], r["w_i"]).all() and _close(fout[i, 6:9], r["throughput"]).all() and _close(fout[i, 9], r["prev_bounce_pdf_out"])
        bad += 0 if ok else 1
        # the generator never depends on a floating-point decision before the BSDF sample: its state must agree on every vector that is not cut earlier
        seen.add((r["result"], r["output_channel"] != 0, r["glossy_only_mode"], mats[r["material"]].emission_intensity > 0, r["bounce"] + 1 >= rp.max_path_depth))
    assert bad <= n // 100, "%d of %d shading steps differ (a lobe / light selection at a boundary or GGX at grazing incidence are the only excuses)" % (bad, n)
    assert len(seen) >= 8, "the vectors no longer cover the step's branches: %r" % (seen,)


LIGHTS_FIXTURE = os.path.join(os.path.dirname(FIXTURE), "ref_lights.json")


@pytest.mark.skipif(not os.path.exists(LIGHTS_FIXTURE), reason="tests/golden/ref_lights.json absent: written by the same `make -C oracle ref_shaders GLM_ROOT=...` "
                    "(oracle/ref_lights_driver.cpp: librender/lights.cpp compiled unmodified)")
def test_emitter_table_preparation_against_the_references_own_lights_cpp():
    """SURVEY 8(c) group (11): update_light_sampling = estimate_normalized_radiance -> trim_dim_emitters -> equalize_emitter_bins (librender/lights.cpp:75-90,
    166-349) on seven seeded emitter sets (equal quads as in C3, radiances over three decades, one bin, bins of 4 / 8, trimming + degenerate triangles,
    a receiver distance inside the emitters, bin_size 1): the PRODUCT's preparation (lights.py; host/lights.hpp is byte-identical to it,
    tests/test_validation_cli.py) makes the same table -- the same emitters in the same order with the same split radiances, bit for bit (that table is
    what the device samples) -- and the same normalised radiances up to the host's atanf."""
    from realtimepathtracingresearchframework_amd import lights
    ref = json.load(open(LIGHTS_FIXTURE))
    assert len(ref["cases"]) >= 7
    for c in ref["cases"]:
        em = np.array(c["emitters"], np.float32).reshape(-1, 4, 3)
        got_e, got_r = lights.update_light_sampling(em, c["min_perceived_receiver_dist"], c["min_radiance"], c["bin_size"])
        want_e = np.array(c["binned_emitters"], np.float32).reshape(-1, 4, 3)
        want_r = np.array(c["binned_radiances"], np.float32)
        assert got_e.shape == want_e.shape, c["name"]
        assert np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32)), c["name"]
        assert np.allclose(got_r, want_r, rtol=1e-6, atol=0), c["name"]
