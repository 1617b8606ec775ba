"""A traversal wave hands in the results of its finished rays when it refills (csrc/dtraverse.h rp_wave_trace): every ray is retired exactly
once, whatever the queue length and the refill threshold.

What can go wrong is a matter of how many entries a wave's pool holds against the threshold, not of image size: a lane that never sees
a refill again (short queues, a pool with fewer entries than the threshold, the last rays of a wave), a lane that is refilled before it
handed in its result, a lane that hands it in twice. So: closest-hit, occlusion and radiance queries at ray counts around the wave size
and the default threshold, each with the threshold forced to 1, 48 and 64 (RPTR_TRAVERSE_PRESET, read once per handle: every threshold
runs in a child process of its own, which writes what the GPU gave; the comparisons against the oracle happen here).

  - hit records and occlusion bits: bit for bit the oracle's brute force;
  - radiance: the queries are the first n camera rays of an oracle frame (tests/test_gpu_radiance_queries.py), same tolerance;
  - a floor under the sun, where every shadow ray is visible: a ray retired twice doubles its sun term, one never retired loses it;
  - a batch with skipped records and rays that miss everything;
  - queues long enough that a wave refills SOME of its lanes from a pool that still holds entries (the path of a real frame), and whose
    last pool holds 20 entries: closest-hit and occlusion queries, and a whole frame through the extend / connect / tail kernels.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle_lib as O  # noqa: E402
from common import RMSE_TOL, image_error  # noqa: E402
from realtimepathtracingresearchframework_amd import abi, backend, scenes  # noqa: E402

pytestmark = pytest.mark.gpu

# around the wave size (64) and the default threshold (48), around one block's four waves (256); 340 = 5 x 64 + 20: short queues are
# dealt out 64 entries per wave, so the sixth wave's only pool holds 20 entries -- fewer than the threshold 48
COUNTS = (1, 47, 48, 49, 63, 64, 65, 255, 256, 257, 340)
THRESHOLDS = (1, 48, 64)
NODE_MIN = 10  # dtraverse.h RP_NODE_MIN, stated so that the preset changes the refill threshold alone
SCENES = ("cornell32", "grid32")
RW, RH = 32, 11  # radiance: the queries are the first n camera rays of a 32 x 11 frame (352 >= max(COUNTS))
FW, FH = 24, 16  # the floor under the sun: all 384 camera rays
MIXED_N = 300
LONG_FETCH = 128  # entries per pool of the long queues (option traverse_fetch): two fills of a wave's 64 lanes
LONG_W, LONG_H = 512, 256  # the whole frame: more pixels than one block per CU holds lanes, twice over
SKIP = np.int32(-5).view(np.float32)  # mode_or_data < 0
F32 = np.float32


def _scene(name):
    if name == "cornell32":
        return scenes.cornell32()
    if name == "grid32":
        return scenes.grid(32, 32)
    assert name == "floor"
    s = scenes.Scene(name="floor_under_the_sun")  # one quad, facing up, nothing above it: every shadow ray reaches the sun (at the zenith)
    mesh = scenes._add_mesh(s, np.array(scenes._quad((-10, 0, -10), (-10, 0, 10), (10, 0, 10), (10, 0, -10)), F32))
    s.materials = [abi.make_material((0.7, 0.7, 0.7))]
    s.pmeshes.append(scenes.ParameterizedMesh(mesh=mesh, material_offsets=np.array([0], np.int32)))
    s.instances.append(scenes.Instance(transform=scenes.IDENTITY.copy(), pmesh=0))
    s.camera = dict(eye=(0, 3, 0), center=(0, 0, 0), up=(0, 0, -1), fov=40.0)
    s.config = scenes.SceneConfig(**scenes.SKY_CONFIGS["default"])
    s.sky_key = "default"
    s.prepare_lights()
    return s


def _rays(name, n, seed):
    """origins inside the scene's box, directions uniform on the sphere, every second ray ends inside the scene: hits and misses of both
    query kinds (the Cornell box is open at the front, half of the rays over the height field point at the sky)"""
    rng = np.random.default_rng(seed)
    lo, hi = ((-0.9, -0.9, -0.9), (0.9, 0.9, 0.9)) if name == "cornell32" else ((-50, 3, -25), (50, 8, 25))
    q = np.zeros((n, 8), F32)
    q[:, 0:3] = rng.uniform(F32(lo), F32(hi), (n, 3))
    d = rng.normal(size=(n, 3))
    q[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    reach = 1.5 if name == "cornell32" else 20.0
    q[:, 7] = np.where(np.arange(n) % 2 == 1, rng.uniform(0.1 * reach, reach, n), 1e20)
    return q


def _primary_rays(osc, s, W, H):
    """the camera rays of sample 0 as the oracle makes them, in pixel order, and the oracle's frame (tests/test_gpu_radiance_queries.py)"""
    ref, ost, rays = osc.render_logged(W, H, 1, 1 << 20, sample_begin=0, accum=np.zeros((H, W, 4), F32), variant=abi.VARIANT_GLTF)
    cam = np.asarray(list(s.camera_params().pos), F32)
    prim = rays[(rays[:, 8] == 0.0) & (rays[:, 3] == 0.0) & (rays[:, 0:3] == cam).all(axis=1)]
    assert len(prim) == W * H, "the ray log holds %d primaries for %d pixels" % (len(prim), W * H)
    q = np.zeros((W * H, 8), F32)
    q[:, 0:3], q[:, 4:7], q[:, 7] = prim[:, 0:3], prim[:, 4:7], F32(2e32)
    return q, ref, ost


def _mixed_queries():
    q = _rays("cornell32", MIXED_N, 21)
    away = np.arange(MIXED_N) % 5 == 1  # from in front of the open side, pointing away from the box: nothing on the ray
    q[away, 0:3] = (0.1, 0.2, 5.0)
    q[away, 4:7] = (0.0, 0.0, 1.0)
    q[away, 7] = 1e20
    skipped = np.arange(MIXED_N) % 7 == 0
    q[skipped, 3] = SKIP
    return q, skipped, away & ~skipped


# ---------------------------------------------------------------- the child: what the GPU gives under one threshold
def _handle(s, W, H, options=None):
    r = backend.RenderHip(options=options)
    r.initialize(W, H)
    r.set_scene(s)
    return r


def _worker(in_path, out_path):
    d = np.load(in_path)
    out = {}
    for name in SCENES:
        s = _scene(name)
        cam = s.camera_params()
        r = _handle(s, RW, RH)
        out[name + "/preset"] = np.int32(r.traversal_preset()[1:])
        for n in COUNTS:
            q = np.ascontiguousarray(d[name + "/q"][:n])
            out["%s/closest/%d" % (name, n)] = r.render_ray_queries(q, np.full((n, 4), 7.0, F32))
            out["%s/occlusion/%d" % (name, n)] = r.render_occlusion_queries(q)
            out["%s/radiance/%d" % (name, n)] = r.render_radiance_queries(np.ascontiguousarray(d[name + "/q_rad"][:n]), cam, spp=1, results=np.zeros((n, 4), F32))
        if name == "cornell32":  # the mixed batch, results pre-filled with what skipped slots must keep
            q = np.ascontiguousarray(d["mixed/q"])
            out["mixed/closest"] = r.render_ray_queries(q, np.full((MIXED_N, 4), 7.0, F32))
            out["mixed/occlusion"] = r.render_occlusion_queries(q, results=np.arange(MIXED_N) % 2 == 0)
            out["mixed/radiance"] = r.render_radiance_queries(q, cam, spp=1, results=np.full((MIXED_N, 4), 1234.5, F32))
        r.close()
    s = _scene("floor")
    r = _handle(s, FW, FH)
    out["floor/radiance"] = r.render_radiance_queries(np.ascontiguousarray(d["floor/q_rad"]), s.camera_params(), spp=1, results=np.zeros((FW * FH, 4), F32))
    st = r.radiance_query_stats().raw
    out["floor/rays"] = np.int64([st.rays_closest, st.rays_shadow])
    r.close()
    # long queues: one block per CU and pools of LONG_FETCH entries, so that every wave's pool outlasts its first fill
    s = _scene("cornell32")
    r = _handle(s, LONG_W, LONG_H, options={"blocks_per_cu": 1, "traverse_fetch": LONG_FETCH})
    grid = max(r.get_option("traversal_grid_shared"), r.get_option("traversal_grid_alone"))
    n = grid * 4 * LONG_FETCH + LONG_FETCH + 20  # behind the static pools the cursor hands out one full pool and one of 20 entries
    q = _rays("cornell32", n, 99)
    out["long/grid_n"] = np.int64([grid, n])
    out["long/closest"] = r.render_ray_queries(q, np.full((n, 4), 7.0, F32))
    out["long/occlusion"] = r.render_occlusion_queries(q)
    st = r.render(backend.RenderConfiguration(s.camera_params(), active_variant=abi.VARIANT_GLTF, reset_accumulation=True), spp=1)
    img = np.zeros((LONG_H, LONG_W, 4), F32)
    assert r.readback_framebuffer(img) == LONG_W * LONG_H * 4
    out["long/frame"] = img
    out["long/frame_rays"] = np.int64([st.raw.rays_closest, st.raw.rays_shadow, r.get_option("last_traversal_grid")])
    r.close()
    np.savez(out_path, **out)


# ---------------------------------------------------------------- here: inputs and references, once
@functools.lru_cache(maxsize=None)
def _reference():
    ref = {"scene": {}, "osc": {}}
    inputs = {}
    for name in SCENES + ("floor",):
        s = _scene(name)
        osc = O.OracleScene(s)
        W, H = (FW, FH) if name == "floor" else (RW, RH)
        q_rad, frame, ost = _primary_rays(osc, s, W, H)
        inputs[name + "/q_rad"] = q_rad
        ref[name + "/frame"] = frame.reshape(-1, 4)
        ref[name + "/rays"] = (int(ost.rays_closest), int(ost.rays_shadow))
        if name != "floor":
            inputs[name + "/q"] = _rays(name, max(COUNTS), 7 + len(name))
        ref["osc"][name] = osc
    inputs["mixed/q"] = _mixed_queries()[0]
    ref["inputs"] = inputs
    return ref


def _brute(osc, q, prefill=7.0):
    """(closest-hit records as rptr_hip_trace lays them out, occlusion bits over (eps |origin|, t_max)) by the oracle's brute force"""
    closest = np.full((len(q), 4), prefill, F32)
    osc.trace(q, bvh_mode=O.BVH_BRUTE, out=closest)
    o = q[:, 0:3]
    tmin = F32(5e-6) * np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2], dtype=F32)  # RPTR_RAY_EPSILON |origin|
    _, ids = osc.trace_ex(o, q[:, 4:7], tmin, q[:, 7], any_hit=True, bvh_mode=O.BVH_BRUTE)
    return closest, ids[:, 0] != 0


@pytest.fixture(scope="module")
def gpu_run(tmp_path_factory):
    """gpu_run(threshold): what a fresh process with RPTR_TRAVERSE_PRESET=NODE_MIN,threshold gave -- one child per threshold"""
    tmp = tmp_path_factory.mktemp("retire_at_refill")
    done = {}

    def run(threshold):
        if threshold not in done:
            in_path, out_path = str(tmp / "inputs.npz"), str(tmp / ("out%d.npz" % threshold))
            if not os.path.exists(in_path):
                np.savez(in_path, **_reference()["inputs"])
            # (the child does not use torch: it skips the import that only orders the HIP runtimes of a process that does)
            env = dict(os.environ, RPTR_TRAVERSE_PRESET="%d,%d" % (NODE_MIN, threshold), RPTR_SKIP_TORCH_PRELOAD="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), in_path, out_path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
            done[threshold] = dict(np.load(out_path))
        return done[threshold]

    return run


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_preset_reaches_the_handle(gpu_run, threshold):
    for name in SCENES:
        assert tuple(gpu_run(threshold)[name + "/preset"]) == (NODE_MIN, threshold)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", SCENES)
def test_hit_records_and_occlusion_bits_are_the_brute_forces(gpu_run, name, threshold, n):
    ref, got = _reference(), gpu_run(threshold)
    q = ref["inputs"][name + "/q"][:n]
    closest, occluded = _brute(ref["osc"][name], q)
    res, bits = got["%s/closest/%d" % (name, n)], got["%s/occlusion/%d" % (name, n)]
    print("%s n=%d threshold %d: %d hits, %d occluded; differs in %d records, %d bits" % (
        name, n, threshold, int((closest.view(np.int32)[:, 3] >= 0).sum()), int(occluded.sum()),
        int((_bits(res) != _bits(closest)).any(axis=1).sum()), int((bits != occluded).sum())))
    assert res.shape == (n, 4) and bits.shape == (n,) and bits.dtype == np.bool_
    assert not (res == 7.0).all(axis=1).any()  # every ray handed in
    assert np.array_equal(_bits(res), _bits(closest))
    assert np.array_equal(bits, occluded)
    if n >= 255:  # the rays cover hits and misses of both kinds
        hit = closest.view(np.int32)[:, 3] >= 0
        assert hit.sum() >= 20 and (~hit).sum() >= 20 and occluded.sum() >= 20 and (~occluded).sum() >= 20


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", SCENES)
def test_radiance_of_the_first_n_camera_rays_is_the_oracle_frames(gpu_run, name, threshold, n):
    want = _reference()[name + "/frame"][:n]
    got = gpu_run(threshold)["%s/radiance/%d" % (name, n)]
    rmse, same, worst = image_error(got[None], want[None])
    print("%s n=%d threshold %d: rmse %.3e worst %.3e" % (name, n, threshold, rmse, worst))
    assert got.shape == (n, 4)
    assert same and rmse < RMSE_TOL
    assert np.array_equal(got[:, 3], want[:, 3])


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_every_visible_shadow_ray_adds_its_sun_term_once(gpu_run, threshold):
    ref, got = _reference(), gpu_run(threshold)
    want, rays = ref["floor/frame"], ref["floor/rays"]
    res = got["floor/radiance"]
    rmse, same, worst = image_error(res[None], want[None])
    print("threshold %d: rmse %.3e worst %.3e, mean radiance %.3f, rays %s / %s" % (threshold, rmse, worst, float(want[:, :3].mean()), tuple(got["floor/rays"]), rays))
    # (what the test rests on: every path has a shadow ray, and the sun term is what the pixels are made of)
    assert rays[1] >= FW * FH and (want[:, 3] == 1.0).all() and want[:, :3].min() > 0.05
    for mine, oracles in zip(got["floor/rays"], rays):  # (up to branch flips by the last bits of device vs libm sin / cos, as in the frame tests)
        assert abs(int(mine) - oracles) <= max(4, 1e-3 * oracles)
    assert same and rmse < RMSE_TOL
    assert np.array_equal(res[:, 3], want[:, 3])


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_skipped_records_keep_their_slot_and_misses_report_a_miss(gpu_run, threshold):
    ref, got = _reference(), gpu_run(threshold)
    q, skipped, away = _mixed_queries()
    assert skipped.sum() >= 30 and away.sum() >= 30
    closest, occluded = _brute(ref["osc"]["cornell32"], q)
    res, bits, rad = got["mixed/closest"], got["mixed/occlusion"], got["mixed/radiance"]
    assert (res[skipped] == 7.0).all() and (closest[skipped] == 7.0).all()
    assert np.array_equal(_bits(res), _bits(closest))
    assert (res[away].view(np.int32)[:, 2:] == -1).all() and (res[away, :2] == -1.0).all()  # rt_intersect's miss record
    pattern = np.arange(MIXED_N) % 2 == 0
    assert np.array_equal(bits[skipped], pattern[skipped])
    assert np.array_equal(bits[~skipped], occluded[~skipped]) and not bits[away].any()
    assert (rad[skipped] == 1234.5).all()
    assert (rad[~skipped] != 1234.5).any(axis=1).all() and np.isfinite(rad[~skipped]).all()
    assert (rad[away, 3] == 0.0).all()  # alpha 0: the first ray left the scene
    hit = closest.view(np.int32)[:, 3] >= 0
    # (the radiance run's interval starts at 0, the closest-hit query's at eps |origin|: no ray of this batch ends between the two)
    assert np.array_equal(rad[~skipped, 3] == 1.0, hit[~skipped])


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_long_queues_refill_some_lanes_at_a_time_and_end_in_a_short_pool(gpu_run, threshold):
    ref, got = _reference(), gpu_run(threshold)
    grid, n = (int(v) for v in got["long/grid_n"])
    assert grid > 0 and n == grid * 4 * LONG_FETCH + LONG_FETCH + 20 and n <= 2_500_000
    q = _rays("cornell32", n, 99)
    closest, occluded = _brute(ref["osc"]["cornell32"], q)
    res, bits = got["long/closest"], got["long/occlusion"]
    print("threshold %d: grid %d, %d queries; differs in %d records, %d bits" % (threshold, grid, n, int((_bits(res) != _bits(closest)).any(axis=1).sum()), int((bits != occluded).sum())))
    assert not (res == 7.0).all(axis=1).any()
    assert np.array_equal(_bits(res), _bits(closest))
    assert np.array_equal(bits, occluded)


@functools.lru_cache(maxsize=None)
def _long_frame():
    return _reference()["osc"]["cornell32"].render(LONG_W, LONG_H, 1, variant=abi.VARIANT_GLTF)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_a_frame_with_pools_of_two_fills_is_the_oracles(gpu_run, threshold):
    got = gpu_run(threshold)
    want, ost = _long_frame()
    img = got["long/frame"]
    closest, shadow, grid = (int(v) for v in got["long/frame_rays"])
    assert 0 < grid * 256 * 2 <= LONG_W * LONG_H  # at least 128 first-queue entries per wave: no lane's first ray is its wave's last
    rmse, same, worst = image_error(img, want)
    print("threshold %d: rmse %.3e worst %.3e rays %d/%d shadow %d/%d" % (threshold, rmse, worst, closest, ost.rays_closest, shadow, ost.rays_shadow))
    assert same and rmse < RMSE_TOL
    assert np.array_equal(img[..., 3], want[..., 3])
    # (ray counts agree up to branch flips caused by the last bits of device vs libm sin / cos: 1e-3 relative, as in the other frame tests)
    assert abs(closest - int(ost.rays_closest)) <= max(4, 1e-3 * ost.rays_closest)
    assert abs(shadow - int(ost.rays_shadow)) <= max(4, 1e-3 * ost.rays_shadow)


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
