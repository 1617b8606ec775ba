"""The thin-lens model of tests/dof_ref.py (the yardstick of tests/test_gpu_dof.py) keeps the properties of a thin lens, its generator is the
oracle's, and the host side reads the reference's .ini keys for it. No GPU."""
import os
import subprocess

import numpy as np
import pytest

import dof_ref as D
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "realtimepathtracingresearchframework_amd", "host")

N = 4096
W, H = 96, 64
CAM = dict(pos=(0.3, 1.2, 3.4), dir=(-0.2672612419, -0.5345224838, -0.8017837257), up=(0.0, 1.0, 0.0), fovy=35.0)
R, FOCUS = 0.07, 2.75


@pytest.fixture(scope="module")
def draws():
    rng = np.random.default_rng(5)
    px, py = rng.integers(0, W, N), rng.integers(0, H, N)
    return px, py, rng.random((N, 2), dtype=np.float32), rng.random((N, 2), dtype=np.float32)


@pytest.fixture(scope="module")
def rays(draws):
    px, py, pd, ad = draws
    return D.lens_ray(CAM, W, H, px, py, pd, ad, R, FOCUS), D.lens_ray64(CAM, W, H, px, py, pd, ad, R, FOCUS)


def test_every_ray_passes_through_the_focus_point_of_its_pinhole_ray(draws, rays):
    px, py, pd, ad = draws
    (o, d), _ = rays
    pos, pin = D.lens_ray(CAM, W, H, px, py, pd, ad, 0.0, FOCUS)
    assert np.array_equal(pos, np.broadcast_to(np.asarray(CAM["pos"], np.float32), pos.shape))  # aperture 0: the pinhole ray
    focus = pos.astype(np.float64) + FOCUS * pin.astype(np.float64)
    rel = focus - o.astype(np.float64)
    d64 = d.astype(np.float64)
    dist = np.linalg.norm(rel - (rel * d64).sum(axis=1, keepdims=True) * d64 / (d64 * d64).sum(axis=1, keepdims=True), axis=1)
    assert o.dtype == np.float32 and d.dtype == np.float32
    assert dist.max() <= 1e-5 * FOCUS, dist.max()


def test_origins_lie_on_the_lens_disc(rays):
    (o, _), _ = rays
    pos, du, dv, _ = D.camera_basis(CAM, W, H, np.float64)
    off = o.astype(np.float64) - pos
    n = np.cross(du, dv)
    n /= np.linalg.norm(n)
    assert np.abs(off @ n).max() <= 2e-6  # in the plane through cam_pos spanned by du, dv: a few float32 ulps (2.4e-7) of positions of magnitude 3.4
    assert np.linalg.norm(off, axis=1).max() <= R * (1 + 1e-5)


def test_the_lens_samples_are_uniform_on_the_disc(rays):
    _, (o, _) = rays
    pos = D.camera_basis(CAM, W, H, np.float64)[0]
    r2 = ((o - pos) ** 2).sum(axis=1)
    # uniform on a disc: r^2 is uniform on [0, R^2] -- mean R^2 / 2, standard deviation R^2 / sqrt(12)
    se = R * R / np.sqrt(12.0) / np.sqrt(N)
    assert abs(r2.mean() - R * R / 2) <= 3 * se, (r2.mean(), R * R / 2, se)


def test_float32_and_float64_twins_agree(rays):
    (o, d), (o64, d64) = rays
    assert np.abs(o - o64).max() <= 1e-5 * np.abs(o64).max()
    assert np.abs(d - d64).max() <= 1e-5


def test_the_generator_of_the_model_is_the_oracles():
    for index, frame, px, py in ((0, 0, 0, 0), (3, 17, 95, 63), (1000, 2 ** 31 + 5, 7, 11)):
        s0, fl = O.rng_probe(index, frame, px, py, W, n=6)
        s = D.lcg_seed(index, frame, px, py, W)
        assert int(s) == s0
        got = []
        for _ in range(6):
            s, x = D.lcg_randomf(s)
            got.append(x)
        assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), fl.view(np.uint32))


def test_edge_profile_of_a_plane_in_focus_is_a_pixel_wide_and_widens_with_defocus():
    rows = [31, 32]
    f = 4.0
    pix = 2.0 * np.tan(np.radians(10.0)) / H  # pixel size at distance 1
    Rr = 8.0 * pix * (0.5 * f)  # circle of confusion at 0.5 f: diameter 2 R |d - f| / f = R = 8 pixels there
    sharp = D.edge_width_10_90(D.edge_profile(W, H, 20.0, Rr, f, f, rows, samples=2048))
    near = D.edge_width_10_90(D.edge_profile(W, H, 20.0, Rr, f, 0.5 * f, rows, samples=2048))
    far = D.edge_width_10_90(D.edge_profile(W, H, 20.0, Rr, f, 2.0 * f, rows, samples=2048))
    assert sharp <= 1.0
    # a disc of diameter D across an edge: the 10-90 % width of its cumulative area is 0.687 D (plus the pixel's own box)
    assert 0.687 * 8 - 0.5 <= near <= 0.687 * 8 + 1.0, near
    assert 0.687 * 4 - 0.5 <= far <= 0.687 * 4 + 1.0, far


INI = """[Application][]
batch spp= 2
..

[Application][scene.vks]
[.][Sensor]
aperture radius= 5.000000e-02
focal distance= 3.250000e+00
focal length= 5.000000e+01
..
"""

PROBE = r"""
#include "ini_config.hpp"
#include "render_hip.hpp"
#include <cstdio>
int main(int argc, char **argv) {
    rptr::HostConfig c{};
    c.params.aperture_radius = 0.f;
    c.params.focus_distance = 2.5f;
    c.params.focal_length = 35.f;
    rptr::load_config(argv[1], c);
    rptr::RenderBackendOptions o;
    std::printf("%g %g %g %d\n", c.params.aperture_radius, c.params.focus_distance, c.params.focal_length, o.enable_raytraced_dof ? 1 : 0);
    return 0;
}
"""


def test_ini_keys_reach_the_render_params_and_the_dof_mirror_defaults_to_on(tmp_path):
    (tmp_path / "dof.ini").write_text(INI)
    (tmp_path / "probe.cpp").write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + HOST, str(tmp_path / "probe.cpp"), "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "dof.ini")], capture_output=True, text=True, check=True).stdout.split()
    assert [float(x) for x in out[:3]] == [0.05, 3.25, 50.0]
    assert out[3] == "1"  # RenderBackendOptions::enable_raytraced_dof (render_params.glsl.h:97): default true
