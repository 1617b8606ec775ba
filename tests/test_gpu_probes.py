"""Irradiance probes on the device (rptr_hip_trace_probes*, the two stage entry points, RenderHip.trace_probes): every number against
tests/probes_ref.py or the public radiance queries, bit for bit. The stages alone (records, coefficients, skipped probes, blends, loops
past one grid), the whole call (the ray values are those of radiance queries over the generated records, the coefficients their
projection), fresh samples, runs, isolation from the frame in progress, moved instances."""
import numpy as np
import pytest

import probes_ref as P
from common import config, float_bits, movable_two_level, one_grid_elements, random_transforms, raw_stats, read_frame, renderer, same_images, scene_transforms, \
    with_transforms
from realtimepathtracingresearchframework_amd import abi, backend, probes, scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48
KS = (1, 63, 64, 65, 200)  # below, at and above one wave's lanes; a fourth trip of the lane loop
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def cornell():
    s = scenes.cornell32()
    r = renderer(s, W, H)
    yield r, s
    r.close()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()  # (the kernels run on other streams than torch's)
    return t


def _stream():
    import torch
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    return st


def _same_bits(a, b):
    return np.array_equal(float_bits(a), float_bits(b))


def _positions(n, seed, lo, hi, skipped=()):
    pos = np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)
    for k, p in enumerate(skipped):
        pos[p, k % 3] = (NAN, np.float32(np.inf), np.float32(-np.inf))[k % 3]
    return pos


def _values(n, K, seed, bad=True):
    """ray values in [0, 4) (alpha 0 or 1), with rays that have a NaN or an infinity in one component"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 4.0, (n, K, 4)).astype(np.float32)
    v[..., 3] = rng.integers(0, 2, (n, K)).astype(np.float32)
    if bad:
        flat = v.reshape(-1, 4)
        idx = rng.choice(len(flat), max(1, len(flat) // 9), replace=False)
        flat[idx, rng.integers(0, 4, len(idx))] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), len(idx))
    return v


# ---------------------------------------------------------------- 1. the ray stage
@pytest.mark.parametrize("K", KS)
def test_ray_records_equal_the_reference_and_a_skipped_probe_carries_minus_one(cornell, K):
    r, _ = cornell
    pos = _positions(3, K, -1, 1, skipped=(1,))
    R = probes.rotation(100 + K)
    table = probes.directions(K)
    tq = _dev(np.full((3 * K, 8), 7.0, np.float32))
    tp = _dev(pos)
    st = _stream()
    r.probe_rays_device(tp.data_ptr(), 3, tq.data_ptr(), stream=st.cuda_stream, rays_per_probe=K, rotation=R, t_max=7.5)
    st.synchronize()
    got = tq.cpu().numpy()
    want = P.rays(pos, table, R, 7.5)
    assert _same_bits(got, want)
    mode = got.view(np.int32)[:, 3].reshape(3, K)
    assert (mode[1] == -1).all() and (mode[0] == 0).all() and (mode[2] == 0).all()
    assert (got[:, 7] == np.float32(7.5)).all()
    assert K == 1 or not _same_bits(got[:K, 4:7], table)  # (the rotation shows)


# ---------------------------------------------------------------- 2. the projection stage
@pytest.mark.parametrize("clamp", [0.0, 1.5])
@pytest.mark.parametrize("K", KS)
def test_projection_alone_equals_the_reference(cornell, K, clamp):
    r, _ = cornell
    n = 4
    pos = _positions(n, 7 + K, -1, 1, skipped=(2,))
    R = probes.rotation(K)
    table = probes.directions(K)
    values = _values(n, K, 31 * K + int(clamp * 2))
    assert not np.isfinite(values).all()
    tv, tp = _dev(values), _dev(pos)
    st = _stream()
    # blend 1 over a NaN-filled buffer: a plain store; the skipped probe keeps its NaN pattern
    junk = np.full((n, 9, 4), np.nan, np.float32)
    junk.view(np.uint32)[...] |= np.arange(n * 36, dtype=np.uint32).reshape(n, 9, 4)  # (distinct payloads)
    tc = _dev(junk)
    r.probe_project_device(tv.data_ptr(), n, tc.data_ptr(), device_positions=tp.data_ptr(), stream=st.cuda_stream, rays_per_probe=K, rotation=R, clamp=clamp)
    st.synchronize()
    got = tc.cpu().numpy()
    want = P.project(values, table, R, clamp=clamp, old=junk, positions=pos)
    assert np.isfinite(got[[0, 1, 3]]).all() and _same_bits(got[2], junk[2])
    assert _same_bits(got, want)
    # no positions: no probe is skipped
    tc = _dev(junk)
    r.probe_project_device(tv.data_ptr(), n, tc.data_ptr(), stream=st.cuda_stream, rays_per_probe=K, rotation=R, clamp=clamp)
    st.synchronize()
    assert _same_bits(tc.cpu().numpy(), P.project(values, table, R, clamp=clamp))
    # blend 0.25 over known coefficients
    known = np.random.default_rng(K).uniform(-2, 2, (n, 9, 4)).astype(np.float32)
    tc = _dev(known)
    r.probe_project_device(tv.data_ptr(), n, tc.data_ptr(), device_positions=tp.data_ptr(), stream=st.cuda_stream, rays_per_probe=K, rotation=R, clamp=clamp, blend=0.25)
    st.synchronize()
    got = tc.cpu().numpy()
    want = P.project(values, table, R, clamp=clamp, blend=0.25, old=known, positions=pos)
    assert _same_bits(got, want) and _same_bits(got[2], known[2]) and not _same_bits(got[0], known[0])
    if clamp > 0:  # (the clamp bites, and never on alpha)
        assert not _same_bits(P.project(values, table, R, clamp=clamp), P.project(values, table, R))
        assert _same_bits(P.project(values, table, R, clamp=clamp)[..., 3], P.project(values, table, R)[..., 3])


# ---------------------------------------------------------------- 3. the whole call
def _whole_call_case(name):
    if name == "cornell32":
        return scenes.cornell32(), (-0.7, 0.7)
    return movable_two_level(), (-4.0, 4.0)


@pytest.mark.parametrize("scene_name,variant", [("cornell32", abi.VARIANT_GLTF), ("cornell32", abi.VARIANT_SIMPLE), ("two_level", abi.VARIANT_GLTF),
                                                ("two_level", abi.VARIANT_SIMPLE)])
def test_whole_call_is_radiance_queries_over_the_generated_records_then_the_projection(scene_name, variant):
    s, (lo, hi) = _whole_call_case(scene_name)
    r = renderer(s, W, H)
    cam = s.camera_params()
    n, K, m = 5, 96, 2
    pos = _positions(n, 11, lo, hi, skipped=(3,))
    R = probes.rotation(4)
    table = probes.directions(K)
    junk = np.full((n, 9, 4), 123.0, np.float32)
    coeffs = r.trace_probes(pos, cam, variant=variant, coeffs=junk.copy(), rays_per_probe=K, samples_per_ray=m, rotation=R)
    st = r.radiance_query_stats()
    values = r.readback_probe_rays(n * K)
    records = P.rays(pos, table, R, 1e20)
    public = r.render_radiance_queries(records, cam, variant=variant, spp=m, first_sample=0)
    assert _same_bits(values, public)
    assert values[:, :3].max() > 0 and set(np.unique(values[:, 3])) <= {0.0, 0.5, 1.0}
    assert not values[3 * K:4 * K].any()  # the skipped probe's rays read 0
    want = P.project(values.reshape(n, K, 4), table, R, old=junk, positions=pos)
    assert _same_bits(coeffs, want) and (coeffs[3] == 123.0).all()
    pst = r.radiance_query_stats()
    assert st.raw.spp == m and int(st.raw.rays_closest) == int(pst.raw.rays_closest) > 0 and int(st.raw.rays_shadow) == int(pst.raw.rays_shadow)
    # the device form, on a caller's stream
    tp, tc = _dev(pos), _dev(junk)
    stream = _stream()
    r.trace_probes_device(tp.data_ptr(), n, cam, tc.data_ptr(), variant=variant, stream=stream.cuda_stream, rays_per_probe=K, samples_per_ray=m, rotation=R)
    stream.synchronize()
    assert _same_bits(tc.cpu().numpy(), coeffs)
    # n_probes == 0 succeeds and touches nothing; more rays than the last run had are refused
    assert r.trace_probes(pos[:0], cam).shape == (0, 9, 4)
    with pytest.raises(backend.BackendError) as e:
        r.readback_probe_rays(n * K + 1)
    assert e.value.code == abi.RPTR_E_INVALID and "last run" in str(e.value)
    r.close()


def test_calls_before_set_scene_and_before_initialize_and_striped_handles_are_refused():
    s = scenes.cornell32()
    pos = _positions(2, 1, -0.5, 0.5)
    for prepare, what in ((lambda r: None, "before set_scene"), (lambda r: r.set_scene(s), "before initialize")):
        r = backend.RenderHip()
        prepare(r)
        with pytest.raises(backend.BackendError) as e:
            r.trace_probes(pos, s.camera_params())
        assert e.value.code == abi.RPTR_E_INVALID and what in str(e.value), str(e.value)
        with pytest.raises(backend.BackendError) as e:
            r.readback_probe_rays(1)
        assert e.value.code == abi.RPTR_E_INVALID
        r.close()
    r = backend.RenderHip(rank=0, world_size=2)
    r.initialize(W, H)
    r.set_scene(s)
    with pytest.raises(backend.BackendError) as e:
        r.trace_probes(pos, s.camera_params())
    assert e.value.code == abi.RPTR_E_UNSUPPORTED
    r.close()


# ---------------------------------------------------------------- 4. fresh samples
def test_a_run_behind_sample_zero_is_a_fresh_sample_with_that_random_number_index(cornell):
    r, s = cornell
    cam = s.camera_params()
    n, K, sidx = 3, 65, 3
    pos = _positions(n, 21, -0.7, 0.7)
    R = probes.rotation(9)
    records = P.rays(pos, probes.directions(K), R, 1e20)

    def fresh(sample_index, m):
        r.trace_probes(pos, cam, rays_per_probe=K, rotation=R, sample_index=sample_index, samples_per_ray=m)
        return r.readback_probe_rays(n * K)

    c_s = fresh(sidx, 1)
    before = r.render_radiance_queries(records, cam, spp=sidx, first_sample=0)        # R_{s-1}: the mean of samples 0 .. s-1
    after = r.render_radiance_queries(records, cam, spp=sidx + 1, first_sample=0)     # R_s
    fold = before + (c_s - before) / np.float32(sidx + 1)
    assert fold.dtype == np.float32
    assert _same_bits(fold, after)
    assert not _same_bits(c_s, fresh(0, 1))  # (another index, another sample)
    # the public fold from first_sample = s, by contrast, reads the old mean: over zeros it is c_s / (s + 1), not c_s
    assert not _same_bits(r.render_radiance_queries(records, cam, spp=1, first_sample=sidx), c_s)
    # m = 2: the float32 running mean of the two m = 1 runs
    a, b = c_s, fresh(sidx + 1, 1)
    two = fresh(sidx, 2)
    assert _same_bits(two, a + (b - a) / np.float32(2.0))
    assert not _same_bits(a, b)


# ---------------------------------------------------------------- 5. runs
def test_probes_beyond_max_run_rays_go_in_runs_of_whole_probes(cornell):
    r, s = cornell
    cam = s.camera_params()
    n, K = 5, 64
    pos = _positions(n, 33, -0.7, 0.7)
    R = probes.rotation(2)
    kw = dict(rays_per_probe=K, rotation=R, sample_index=1)
    whole = r.trace_probes(pos, cam, max_run_rays=2 * K + K // 2, **kw)  # floor(160 / 64) = 2 probes per run: runs of 2, 2, 1
    last = r.readback_probe_rays(K)
    with pytest.raises(backend.BackendError):
        r.readback_probe_rays(K + 1)  # (the last run had one probe)
    for p0 in (0, 2, 4):
        part = r.trace_probes(pos[p0:p0 + 2], cam, **kw)
        assert _same_bits(whole[p0:p0 + 2], part), p0
    assert _same_bits(last, r.readback_probe_rays(K))
    one_run = r.trace_probes(pos, cam, **kw)
    assert _same_bits(one_run[:2], whole[:2]) and not _same_bits(one_run[2:], whole[2:])  # (a probe's random numbers depend on its index in its run)
    tiny = r.trace_probes(pos[:2], cam, max_run_rays=1, **kw)  # fewer rays than a probe has: one probe per run
    assert _same_bits(tiny[1], r.trace_probes(pos[1:2], cam, **kw)[0])


# ---------------------------------------------------------------- 6. past one grid
def test_both_kernels_take_a_second_trip_of_their_grid_stride_loops(cornell):
    r, _ = cornell
    E = one_grid_elements()
    st = _stream()
    # rays: one thread per ray, more rays than one launch has threads
    K = 200
    n = E // K + 3
    assert n * K > E
    pos = _positions(n, 5, -3, 3, skipped=(n - 2,))
    R = probes.rotation(77)
    table = probes.directions(K)
    tp = _dev(pos)
    tq = _dev(np.zeros((n * K, 8), np.float32))
    r.probe_rays_device(tp.data_ptr(), n, tq.data_ptr(), stream=st.cuda_stream, rays_per_probe=K, rotation=R)
    st.synchronize()
    assert _same_bits(tq.cpu().numpy(), P.rays(pos, table, R, 1e20))
    del tq
    # projection: one wave per probe, more probes than one launch has waves
    K2 = 5
    n2 = E // 64 + 37
    assert n2 * 64 > E
    print("one grid covers %d elements: %d probes x %d rays for the ray kernel, %d probes x %d rays for the projection" % (E, n, K, n2, K2))
    pos2 = _positions(n2, 6, -3, 3, skipped=(n2 - 1, 17))
    values = _values(n2, K2, 99)
    table2 = probes.directions(K2)
    old = np.random.default_rng(1).uniform(-1, 1, (n2, 9, 4)).astype(np.float32)
    tv, tp2, tc = _dev(values), _dev(pos2), _dev(old)
    r.probe_project_device(tv.data_ptr(), n2, tc.data_ptr(), device_positions=tp2.data_ptr(), stream=st.cuda_stream, rays_per_probe=K2, rotation=R, clamp=2.0)
    st.synchronize()
    assert _same_bits(tc.cpu().numpy(), P.project(values, table2, R, clamp=2.0, old=old, positions=pos2))


# ---------------------------------------------------------------- 7. isolation
def test_a_probe_call_between_two_frames_leaves_images_and_stats_alone():
    s = movable_two_level()
    cam = s.camera_params()
    pos = _positions(40, 3, -4, 4)

    def run(with_probes):
        r = renderer(s, W, H)
        r.render(config(s, reset=True), spp=2)
        if with_probes:
            c = r.trace_probes(pos, cam, rays_per_probe=64, sample_index=5, samples_per_ray=2)
            assert np.isfinite(c).all() and c[:, 0, :3].max() > 0
        r.render(config(s, reset=False), spp=2)
        st = raw_stats(r)
        out = read_frame(r, W, H), (st.spp, int(st.rays_closest), int(st.rays_shadow), int(st.hits_shaded))
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_images(a[0], b[0])
    assert a[1] == b[1] and a[1][0] == 4


# ---------------------------------------------------------------- 8. moved scene
def test_coefficients_follow_moved_instances_like_a_fresh_scene():
    s = movable_two_level()
    cam = s.camera_params()
    xf = scene_transforms(s)
    moved_xf = random_transforms(4, 8)
    pos = _positions(24, 13, -4, 4)
    kw = dict(rays_per_probe=128, sample_index=2)
    r = renderer(s, W, H)
    before = r.trace_probes(pos, cam, **kw)
    r.update_instances(0, moved_xf)
    r.refit()
    after = r.trace_probes(pos, cam, **kw)
    r.close()
    fresh = renderer(with_transforms(s, moved_xf), W, H)
    want = fresh.trace_probes(pos, cam, **kw)
    fresh.close()
    assert len(xf) >= 4 and not _same_bits(before, after)
    assert _same_bits(after, want)
