"""Irradiance probes without a device: the direction set of rptr_hip_probe_directions, the quadrature it makes with the L2 basis, the
cosine-lobe convolution, the float32 reference (tests/probes_ref.py) against float64, and the argument refusals that come before the
device is touched."""
import ctypes as C

import numpy as np
import pytest

import probes_ref as P
from realtimepathtracingresearchframework_amd import abi, backend, probes

# quadrature error of the direction set with the basis, a fixed property of both (measured with numpy's libm: 1.26e-3 for K = 256,
# 1.09e-2 for K = 64; the bounds leave 1.6 x and 1.4 x)
GRAM_BOUND = {256: 2e-3, 64: 1.5e-2}


def _err(L):
    return (L.rptr_hip_last_error(None) or b"").decode()


@pytest.mark.parametrize("K", [1, 64, 200, 4096])
def test_directions_are_the_spherical_fibonacci_set_to_one_ulp(K):
    got = probes.directions(K)
    assert got.shape == (K, 3) and got.dtype == np.float32
    want = P.directions_f64(K)
    w32 = want.astype(np.float32)
    ulp = np.maximum(np.spacing(np.abs(w32)), np.float32(2.0 ** -149)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print("K = %d: worst difference %.3g ulp" % (K, float((err / ulp).max())))
    assert (err <= ulp).all()
    assert np.array_equal(got[:, 2], w32[:, 2])  # z takes no libm call: exact
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 2e-7


def test_directions_refuse_bad_arguments():
    L = backend.load_library()
    out = np.zeros((4, 3), np.float32)
    for K in (0, abi.PROBE_MAX_RAYS + 1):
        assert L.rptr_hip_probe_directions(K, out.ctypes.data_as(C.c_void_p)) == abi.RPTR_E_INVALID and "K = %d" % K in _err(L)
    assert L.rptr_hip_probe_directions(4, None) == abi.RPTR_E_INVALID and "NULL" in _err(L)
    with pytest.raises(backend.BackendError):
        probes.directions(0)


@pytest.mark.parametrize("K", sorted(GRAM_BOUND))
def test_gram_matrix_of_the_set_is_the_identity_within_its_quadrature_error(K):
    d = probes.directions(K).astype(np.float64)
    Y = probes.sh_basis(d)
    G = (4.0 * np.pi / K) * Y.T @ Y
    dev = float(np.abs(G - np.eye(9)).max())
    print("K = %d: Gram matrix deviates from the identity by %.3e (bound %.1e)" % (K, dev, GRAM_BOUND[K]))
    assert dev <= GRAM_BOUND[K]


@pytest.mark.parametrize("K", sorted(GRAM_BOUND))
def test_constant_radiance_gives_irradiance_pi_L(K):
    table = probes.directions(K)
    Lrgb = np.float32([0.7, 1.9, 3.3, 1.0])
    values = np.tile(Lrgb, (1, K, 1))
    coeffs = P.project(values, table, np.eye(3))
    rng = np.random.default_rng(5)
    n = rng.normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    E = probes.sh_irradiance(coeffs[0], n)
    rel = float(np.abs(E / (np.pi * Lrgb.astype(np.float64)) - 1.0).max())
    print("K = %d: irradiance of constant radiance is pi L to within %.3e relative (bound %.1e)" % (K, rel, GRAM_BOUND[K]))
    assert E.shape == (50, 4) and rel <= GRAM_BOUND[K]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200, 4096])
def test_float32_reference_agrees_with_float64_within_the_rounding_bound(K):
    """per coefficient, against the same sums in double: one rounding of each product, at most ceil(K / 64) - 1 of the lane's sums, 6 of
    the butterfly, one of the weight and one of the product with it, each relative 2^-24 of a partial sum no larger than sum |terms|:
    (K / 64 + 7) 2^-24 w sum |terms| to first order"""
    rng = np.random.default_rng(K)
    table = probes.directions(K)
    R = probes.rotation(K)
    values = rng.uniform(0.0, 4.0, (3, K, 4)).astype(np.float32)
    got = P.project(values, table, R).astype(np.float64)
    want, mag = P.project_f64(values, table, R)
    bound = (K / 64.0 + 7.0) * 2.0 ** -24 * mag
    worst = float(np.abs(got - want).max())
    print("K = %d: float32 vs float64 worst %.3e absolute, bound at that entry %.3e" % (K, worst, float(bound.flat[np.abs(got - want).argmax()])))
    assert (np.abs(got - want) <= bound).all()


def test_rotation_is_orthonormal_spread_and_deterministic():
    Rs = [probes.rotation(i) for i in range(64)]
    for R in Rs:
        assert R.dtype == np.float32 and R.shape == (3, 3)
        assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() < 1e-6 and np.linalg.det(R.astype(np.float64)) > 0.999
    assert np.array_equal(probes.rotation(7), Rs[7])
    # no two of the first 64 are near each other: the rotation between them turns by more than 5 degrees
    for i in range(64):
        for j in range(i):
            cos = (np.trace(Rs[i].astype(np.float64) @ Rs[j].astype(np.float64).T) - 1.0) / 2.0
            assert cos < np.cos(np.radians(5.0)), (i, j)
    # the images of one axis cover the sphere: every octant is visited
    ax = np.stack([R[:, 2] for R in Rs])
    assert len({tuple(s) for s in np.sign(ax).astype(int)}) == 8


def test_grid_is_cell_centred_and_x_fastest():
    g = probes.grid((0, 0, 0), (4, 2, 1), (4, 2, 1))
    assert g.dtype == np.float32 and g.shape == (8, 3)
    assert np.array_equal(g[:5], np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 1.5, 0.5]]))


def test_struct_mirror_and_defaults():
    L = backend.load_library()
    assert C.sizeof(abi.ProbeParams) == 80 and abi.ProbeParams.rotation.offset == 16 and abi.ProbeParams.blend.offset == 52
    assert abi.ProbeParams.max_run_rays.offset == 64 and abi.ProbeParams.reserved.offset == 68
    p = abi.ProbeParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    L.rptr_hip_probe_defaults(C.byref(p))
    assert (p.rays_per_probe, p.samples_per_ray, p.sample_index, p.flags, p.max_run_rays) == (128, 1, 0, 0, 0)
    assert list(p.rotation) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and p.blend == 1.0 and p.clamp == 0.0 and p.t_max == np.float32(1e20)
    assert list(p.reserved) == [0, 0, 0]
    L.rptr_hip_probe_defaults(None)  # tolerated


BAD_PARAMS = [
    (dict(rays_per_probe=0), "rays_per_probe"), (dict(rays_per_probe=4097), "rays_per_probe"),
    (dict(samples_per_ray=0), "samples_per_ray"),
    (dict(sample_index=-1), "sample_index"), (dict(sample_index=2 ** 31 - 1, samples_per_ray=1), "overflows"),
    (dict(flags=1), "flag"), (dict(reserved=(0, 0, 1)), "reserved"),
    (dict(blend=0.0), "blend"), (dict(blend=1.5), "blend"), (dict(blend=float("nan")), "blend"),
    (dict(clamp=-1.0), "clamp"), (dict(clamp=float("inf")), "clamp"),
    (dict(t_max=0.0), "t_max"), (dict(t_max=float("nan")), "t_max"),
    (dict(rotation=[1, 0, 0, 0, 1, 0, 0, 0, float("nan")]), "rotation"),
    (dict(rotation=[1, 0.002, 0, 0, 1, 0, 0, 0, 1]), "rotation"),
    (dict(rotation=[1.001, 0, 0, 0, 1, 0, 0, 0, 1]), "rotation"),
]


@pytest.mark.parametrize("fields,word", BAD_PARAMS, ids=[w + "-" + "-".join("%s" % k for k in f) + str(i) for i, (f, w) in enumerate(BAD_PARAMS)])
def test_bad_params_are_refused_before_the_handle_is_looked_at(fields, word):
    """the params are checked first and need neither a handle nor a device: with a NULL handle the message names the offending field"""
    L = backend.load_library()
    p = backend.RenderHip.probe_params(**fields)
    cam = abi.Camera()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    calls = (lambda: L.rptr_hip_trace_probes(None, ptr, 1, C.byref(cam), abi.VARIANT_GLTF, C.byref(p), ptr, None),
             lambda: L.rptr_hip_trace_probes_device(None, ptr, 1, C.byref(cam), abi.VARIANT_GLTF, C.byref(p), ptr, None),
             lambda: L.rptr_hip_probe_rays_device(None, ptr, 1, C.byref(p), ptr, None),
             lambda: L.rptr_hip_probe_project_device(None, ptr, 1, None, C.byref(p), ptr, None))
    for call in calls:
        assert call() == abi.RPTR_E_INVALID
        assert word in _err(L), _err(L)


def test_good_params_with_a_null_handle_name_the_handle_and_slightly_bent_rotations_pass():
    L = backend.load_library()
    cam = abi.Camera()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for rot in (np.eye(3), probes.rotation(3), [1.0004, 0, 0, 0, 1, 0, 0, 0, 1]):  # (R R^T within 1e-3 of the identity)
        p = backend.RenderHip.probe_params(rotation=rot)
        assert L.rptr_hip_trace_probes(None, ptr, 1, C.byref(cam), abi.VARIANT_GLTF, C.byref(p), ptr, None) == abi.RPTR_E_INVALID
        assert "NULL handle" in _err(L)
        assert L.rptr_hip_probe_rays_device(None, ptr, 1, C.byref(p), ptr, None) == abi.RPTR_E_INVALID and "NULL handle" in _err(L)
    # params NULL = the defaults; the buffers come before the handle
    assert L.rptr_hip_trace_probes(None, None, 1, C.byref(cam), abi.VARIANT_GLTF, None, ptr, None) == abi.RPTR_E_INVALID and "NULL position" in _err(L)
    assert L.rptr_hip_probe_project_device(None, None, 1, None, None, ptr, None) == abi.RPTR_E_INVALID and "NULL value" in _err(L)
    assert L.rptr_hip_trace_probes(None, ptr, 1, None, abi.VARIANT_GLTF, None, ptr, None) == abi.RPTR_E_INVALID and "camera" in _err(L)
    assert L.rptr_hip_trace_probes(None, ptr, 1, C.byref(cam), 99, None, ptr, None) == abi.RPTR_E_INVALID and "variant" in _err(L)
    assert L.rptr_hip_probe_rays_device(None, ptr, 2 ** 24, None, ptr, None) == abi.RPTR_E_INVALID and "exceed" in _err(L)  # 2^24 x 128 = 2^31 rays
    assert L.rptr_hip_readback_probe_rays(None, ptr, 1) == abi.RPTR_E_INVALID and "NULL handle" in _err(L)
