"""The thin-lens camera ray in numpy: the yardstick of tests/test_dof_cpu.py and tests/test_gpu_dof.py (the oracle stays pinhole).

The rule is the one include/rptr_hip.h states at RptrRenderParams (vulkan/raygen.rgen:151-160 of the reference), in the order the device
code (csrc/kernels.h rp_primary_ray_ex) takes its operations:

    point  = (px + 0.5, py + 0.5) [+ (pixel_draw - 0.5)]   ;  point /= (W, H)   [+ 0.5 * screen_jitter]
    dir    = normalize(point.x * du + point.y * dv + dir_top_left)
    focus  = origin + focus_distance * dir
    lens   = (cos(2 pi r.x), sin(2 pi r.x)) * sqrt(r.y) * aperture_radius      cos / sin(2 pi x) ARE sincospi(2 x): 2 x is exact, and
                                                                               the device calls sincospif(2 * r.x)
    origin = origin + lens.x * normalize(du);  origin = origin + lens.y * normalize(dv)
    dir    = normalize(focus - origin)

normalize(v) = v * (1 / sqrt((v.x v.x + v.y v.y) + v.z v.z)) as csrc/dmath.h norm3_ieee spells it. lens_ray rounds every operation to
float32 (no fused multiply-adds: the library is built with -ffp-contract=off); sin / cos of pi * (2 x) are taken in float64 and rounded,
i.e. the correctly rounded values a float32 sincospi is within an ulp or two of. lens_ray64 is the same in float64.

Also here: the uniform generator (rendering/pointsets/lcg_rng.glsl, restated as csrc/dshade.h rp_rng_seed / rp_randf do; checked against
the oracle's in test_dof_cpu.py), the camera basis as csrc/host_frame.inl compute_view makes it, and edge_profile: a float64 Monte-Carlo
of what the lens makes of a straight black/white edge."""
import numpy as np

f32 = np.float32
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ the uniform generator
def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(M32)


def murmur_mix(h, k):
    h, k = np.asarray(h, np.uint64), np.asarray(k, np.uint64)
    k = (k * np.uint64(0xcc9e2d51)) & np.uint64(M32)
    k = _rotl(k, 15)
    k = (k * np.uint64(0x1b873593)) & np.uint64(M32)
    h = h ^ k
    return (_rotl(h, 13) * np.uint64(5) + np.uint64(0xe6546b64)) & np.uint64(M32)


def murmur_finalize(h):
    h = np.asarray(h, np.uint64)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def lcg_seed(sample_index, frame_offset, px, py, width):
    """get_lcg_rng(sample_index, frame_offset, (pixel, dims)): the generator state of a pixel sample, uint64 arrays holding 32-bit values"""
    s = murmur_mix(np.uint64(frame_offset), np.asarray(px, np.uint64) + np.asarray(py, np.uint64) * np.uint64(width))
    return murmur_finalize(murmur_mix(s, np.asarray(sample_index, np.uint64)))


def lcg_next(state):
    return (np.asarray(state, np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(M32)


def lcg_randomf(state):
    """-> (new state, float32 in [0, 1]: float(u32) * 2^-32, which may round to 1.0)"""
    s = lcg_next(state)
    return s, (s.astype(np.uint32).astype(f32) * f32(2.0 ** -32)).astype(f32)


def lcg_draw2(state):
    """two numbers, x first -> (new state, (n, 2) float32)"""
    s, x = lcg_randomf(state)
    s, y = lcg_randomf(s)
    return s, np.stack([x, y], axis=-1)


# ------------------------------------------------------------------ the camera
def _cam_fields(cam):
    if isinstance(cam, dict):
        return cam["pos"], cam["dir"], cam["up"], cam["fovy"]
    return list(cam.pos[:]), list(cam.dir[:]), list(cam.up[:]), cam.fovy


def camera_basis(cam, W, H, dtype=f32):
    """(pos, du, dv, dir_top_left) as csrc/host_frame.inl compute_view (render_vulkan.cpp:2880-2896) computes them, in `dtype`"""
    t = dtype
    pos, d, up, fovy = _cam_fields(cam)
    pos, d, up = np.asarray(pos, t), np.asarray(d, t), np.asarray(up, t)

    def cross(a, b):
        return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], t)

    def normalize(v):
        return (v * (t(1.0) / np.sqrt(t(t(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))).astype(t)

    plane_y = t(2.0) * np.tan(t(t(0.5) * t(fovy)) * t(0.01745329251994329576923690768489))
    plane_x = t(plane_y * t(t(W) / t(H)))
    du = (normalize(cross(d, up)) * plane_x).astype(t)
    dv = (-normalize(cross(du, d)) * t(plane_y)).astype(t)
    tl = ((d - t(0.5) * du) - t(0.5) * dv).astype(t)
    return pos, du, dv, tl


def _norm3(v, t):
    d = ((v[..., 0] * v[..., 0]).astype(t) + (v[..., 1] * v[..., 1]).astype(t)).astype(t)
    d = (d + (v[..., 2] * v[..., 2]).astype(t)).astype(t)
    return (v * (t(1.0) / np.sqrt(d).astype(t)).astype(t)[..., None]).astype(t)


def _lens_ray(basis, W, H, px, py, pixel_draw, aperture_draw, aperture_radius, focus_distance, jitter, t):
    pos, du, dv, tl = [np.asarray(b, t) for b in basis]
    px, py = np.asarray(px), np.asarray(py)
    x = (px.astype(t) + t(0.5)).astype(t)
    y = (py.astype(t) + t(0.5)).astype(t)
    if pixel_draw is not None:
        pd = np.asarray(pixel_draw, t)
        x = (x + (pd[..., 0] - t(0.5)).astype(t)).astype(t)
        y = (y + (pd[..., 1] - t(0.5)).astype(t)).astype(t)
    x = (x / t(W)).astype(t)
    y = (y / t(H)).astype(t)
    if jitter is not None:
        x = (x + (t(jitter[0]) * t(0.5))).astype(t)
        y = (y + (t(jitter[1]) * t(0.5))).astype(t)
    v = ((x[..., None] * du).astype(t) + (y[..., None] * dv).astype(t)).astype(t)
    v = (v + tl).astype(t)
    direction = _norm3(v, t)
    origin = np.broadcast_to(pos, direction.shape).astype(t)
    R = t(aperture_radius)
    if aperture_radius > 0:
        focus = (origin + (t(focus_distance) * direction).astype(t)).astype(t)
        r = np.asarray(aperture_draw, t)
        ang = np.pi * (2.0 * r[..., 0].astype(np.float64))  # sincospi(2 x)
        cs, sn = np.cos(ang).astype(t), np.sin(ang).astype(t)
        rad = np.sqrt(r[..., 1]).astype(t)
        lx = ((cs * rad).astype(t) * R).astype(t)
        ly = ((sn * rad).astype(t) * R).astype(t)
        origin = (origin + (lx[..., None] * _norm3(du, t)).astype(t)).astype(t)
        origin = (origin + (ly[..., None] * _norm3(dv, t)).astype(t)).astype(t)
        direction = _norm3((focus - origin).astype(t), t)
    return origin, direction


def lens_ray(cam, W, H, px, py, pixel_draw, aperture_draw, aperture_radius, focus_distance, jitter=None, basis=None):
    """float32. px, py: pixel coordinates (arrays); pixel_draw: (n, 2) pixel-filter numbers, or None when none is drawn (raster TAA;
    jitter: view_params.screen_jitter then); aperture_draw: (n, 2). basis: (pos, du, dv, dir_top_left) instead of camera_basis(cam).
    -> (origin (n, 3), direction (n, 3))"""
    return _lens_ray(basis or camera_basis(cam, W, H, f32), W, H, px, py, pixel_draw, aperture_draw, aperture_radius, focus_distance, jitter, f32)


def lens_ray64(cam, W, H, px, py, pixel_draw, aperture_draw, aperture_radius, focus_distance, jitter=None, basis=None):
    """the float64 twin of lens_ray"""
    return _lens_ray(basis or camera_basis(cam, W, H, np.float64), W, H, px, py, pixel_draw, aperture_draw, aperture_radius, focus_distance, jitter,
                     np.float64)


# ------------------------------------------------------------------ what the lens makes of an edge
def edge_profile(W, H, fovy, aperture_radius, focus_distance, d, rows, samples=4096, seed=1):
    """A camera at the origin looks down -z at the plane z = -d, whose albedo is 1 for x > 0 and 0 for x < 0 (the edge runs through the
    image centre, top to bottom). -> the mean albedo the camera rays of every pixel column see, averaged over pixel rows `rows`: (W,)
    float64, `samples` rays per pixel (box pixel filter, uniform lens disc; plain numpy.random)."""
    rng = np.random.default_rng(seed)
    cam = dict(pos=(0.0, 0.0, 0.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fovy=fovy)
    out = np.zeros(W)
    px = np.repeat(np.arange(W), samples)
    for row in rows:
        n = W * samples
        o, v = lens_ray64(cam, W, H, px, np.full(n, row), rng.random((n, 2)), rng.random((n, 2)), aperture_radius, focus_distance)
        t_hit = (-d - o[:, 2]) / v[:, 2]
        x = o[:, 0] + t_hit * v[:, 0]
        out += (x > 0).reshape(W, samples).mean(axis=1)
    return out / len(rows)


def edge_width_10_90(profile, plateau=8):
    """the 10-90 % width, in pixels, of a monotone edge profile: the levels are the means of the first and last `plateau` columns, the
    crossings are interpolated linearly between pixel centres"""
    p = np.asarray(profile, np.float64)
    lo, hi = p[:plateau].mean(), p[-plateau:].mean()
    q = (p - lo) / (hi - lo)

    def crossing(level):
        i = int(np.argmax(q >= level))  # first column at or above the level
        if i == 0:
            return 0.0
        return (i - 1) + (level - q[i - 1]) / (q[i] - q[i - 1])
    return crossing(0.9) - crossing(0.1)
