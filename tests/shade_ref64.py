"""A float64 restatement of the shading functions the device and the oracle evaluate in binary32 -- TEST INFRASTRUCTURE.

Written from the reference's GLSL (file:line below, paths relative to the reference checkout) and, for the texture sampler, from the
Vulkan texel-filtering equations oracle/oshade.h states, in vectorised numpy float64: an independent, higher-precision statement of
what csrc/dshade.h and oracle/oshade.h compute. tests/test_shade_ref64.py holds the oracle to it on the CPU, tests/test_gpu_shade_functions.py
the device's IEEE and fast_math builds.

The comparison rule for an ill-conditioned function (band()): the float64 value at the binary32 inputs AND at neighbours of them one ulp
away, per component, bound the value a binary32 evaluation may give; a result must lie in that band widened by a stated margin (ulps of
the result, or a relative excess where rounding inside the formula cancels: tests/test_shade_ref64.py lists them with their measured
values). Near the mirror direction, for instance, an ulp of the half vector moves the GGX lobe by 1e-3 of its value (csrc/dmath.h): the
band holds that movement, the margin the rounding of the operations.
"""
import numpy as np

F32 = np.float32
INV_PI = 1.0 / np.pi


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _norm(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _lum(c):  # rendering/util.glsl luminance
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


# ---------------------------------------------------------------- glTF BSDF, rendering/bsdfs/gltf_bsdf.glsl (shipped build: two lobes)
def material(m):
    """the fields of an abi.BaseMaterial the untextured glTF lobe reads, as float64"""
    return dict(base=np.array(m.base_color[:], np.float64), metallic=float(m.metallic), roughness=float(m.roughness), ior=float(m.ior))


def schlick_weight(c):  # :172-174
    return np.clip(1.0 - c, 0.0, 1.0) ** 5


def gtr_2(cos_theta_h, alpha):  # :193-197
    a2 = alpha * alpha
    return INV_PI * a2 / (1.0 + (a2 - 1.0) * cos_theta_h * cos_theta_h) ** 2


def smith_den1(n_dot_o, alpha_sq):  # :199-201
    return np.abs(n_dot_o) + np.sqrt(alpha_sq + (1.0 - alpha_sq) * n_dot_o * n_dot_o)


def smith_ggx(n_dot_o, n_dot_i, alpha_g):  # :206-211
    a = alpha_g * alpha_g
    return 1.0 / (smith_den1(n_dot_i, a) * smith_den1(n_dot_o, a))


def gtr_2_vndf_pdf(n_dot_o, cos_theta_h, alpha):  # :253-257
    return gtr_2(cos_theta_h, alpha) * (0.5 / smith_den1(n_dot_o, alpha * alpha))


def specular_alpha(m):  # :275-277
    return max(m["roughness"] ** 2, float(F32(0.002)))


def specular_basecolor(m):  # :263-273 (no tint)
    d = ((m["ior"] - 1.0) / (m["ior"] + 1.0)) ** 2
    return d * (1.0 - m["metallic"]) + m["base"] * m["metallic"]


def gltf_schlick_weight(o_dot_h, ior):  # :284-292
    f = schlick_weight(o_dot_h)
    ior = np.broadcast_to(ior, np.shape(o_dot_h))
    below = ior < 1.0
    if np.any(below):
        cc = np.sqrt(np.maximum(1.0 - ior * ior, 0.0))
        t = np.minimum((1.0 - o_dot_h) / np.where(below, 1.0 - cc, 1.0), 1.0)
        f = np.where(below, f * (1.0 - t) + t, f)
    return f


def gltf_eval(m, n, wo, wi):
    """gltf_bsdf (:294-359) and gltf_wpdf (:414-494) of the shipped two-lobe build: (f (N, 3), wpdf (N,))"""
    n, wo, wi = (np.asarray(a, np.float64) for a in (n, wo, wi))
    i_dot_n, o_dot_n = _dot(n, wi), _dot(n, wo)
    ior = np.where(o_dot_n < 0.0, 1.0 / m["ior"], m["ior"])
    opposite = i_dot_n * o_dot_n < 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        w_h = _norm(wi + wo)
        o_dot_h, cos_h = _dot(wo, w_h), _dot(n, w_h)
        diffuse = np.broadcast_to((1.0 - m["metallic"]) * m["base"] * INV_PI, n.shape).copy()
        pdf = INV_PI * np.abs(i_dot_n)
        if m["ior"] > 1.0:
            a = specular_alpha(m)
            f0 = specular_basecolor(m)
            spec = gtr_2(cos_h, a) * smith_ggx(o_dot_n, i_dot_n, a)
            fw = gltf_schlick_weight(np.abs(o_dot_h), ior)
            F = f0[None, :] * (1.0 - fw[:, None]) + fw[:, None]
            f = diffuse * (1.0 - F) + spec[:, None] * F
            # component sampler (:366-394) at o_dot_h for both lobes, visibility (1, vis_y)
            vis_y = 2.0 * np.abs(i_dot_n) / smith_den1(i_dot_n, a * a)
            lum_s = _lum(specular_basecolor(m))
            Fs = lum_s * (1.0 - schlick_weight(np.abs(o_dot_h))) + schlick_weight(np.abs(o_dot_h))
            w0 = (1.0 - Fs) * (1.0 - m["metallic"]) * _lum((1.0 - m["metallic"]) * m["base"])
            w1 = Fs * vis_y
            s = w0 + w1
            w0, w1 = np.where(s > 0, w0 / np.where(s > 0, s, 1.0), 1.0), np.where(s > 0, w1 / np.where(s > 0, s, 1.0), w1)
            pdf = pdf * w0 + gtr_2_vndf_pdf(o_dot_n, cos_h, a) * w1
        else:
            f = diffuse
    f = np.where(opposite[:, None], 0.0, f)
    pdf = np.where(opposite & (m["ior"] > 1.0), 0.0, pdf)
    return f, pdf


# ---------------------------------------------------------------- Lambert, rendering/bsdfs/simple_bsdf.glsl
def simple_eval(base, n, wo, wi):
    """simple_bsdf (:44-59) and simple_pdf (:68-83): (f, pdf)"""
    n, wo, wi = (np.asarray(a, np.float64) for a in (n, wo, wi))
    i_dot_n, o_dot_n = _dot(n, wi), _dot(n, wo)
    opposite = i_dot_n * o_dot_n < 0.0
    f = np.where(opposite[:, None], 0.0, np.asarray(base, np.float64) * INV_PI)
    return f, np.where(opposite, 0.0, INV_PI * np.abs(i_dot_n))


# ---------------------------------------------------------------- emitters
FAST_ATAN_MAX_ABS_ERROR = 1.16e-5  # rendering/lights/tri.glsl:54-57


def tri_solid_angle(v9):
    """the exact solid angle of triangles seen from the origin (v9: (N, 9) vertices), Van Oosterom & Strackee (1983):
    tan(omega / 2) = |v0 . (v1 x v2)| / (1 + v0.v1 + v1.v2 + v0.v2) for unit vectors -- what tri.glsl:83-124 approximates with a
    Householder-reflected determinant and fast_positive_atan"""
    v = np.asarray(v9, np.float64).reshape(-1, 3, 3)
    v = v / np.linalg.norm(v, axis=2, keepdims=True)
    num = np.abs(_dot(v[:, 0], np.cross(v[:, 1], v[:, 2])))
    den = 1.0 + _dot(v[:, 0], v[:, 1]) + _dot(v[:, 1], v[:, 2]) + _dot(v[:, 0], v[:, 2])
    return 2.0 * np.arctan2(num, den)


# ---------------------------------------------------------------- binned light selection, rendering/mc/lights_linear.glsl:19-127
MIN_IRRADIANCE = 6.2e-4 * 0.001
BIN_MAX = 16  # BINNED_LIGHTS_BIN_MAX_SIZE


def pad_lights(lights):
    """(L, 4, 3) float64 records (v0, v1, v2, radiance) followed by BIN_MAX + 1 zeroed ones, as the light buffer is padded"""
    lights = np.asarray(lights, np.float64).reshape(-1, 4, 3)
    return np.concatenate([lights, np.zeros((BIN_MAX + 1, 4, 3))])


def light_bin(num_lights, bin_size, sel_x):
    """:21-36 (bin_begin, bin_end, number of bins). The bin is an integer outcome of ONE binary32 product, sel_x * float(bins), so that
    product is formed in binary32 here as well; everything after it is integer arithmetic"""
    bins = (num_lights + bin_size - 1) // bin_size
    x = np.asarray(sel_x, F32) * F32(bins)
    b = np.minimum(np.floor(x.astype(np.float64)).astype(np.int64), bins - 1)
    return b * bin_size, np.minimum(bin_size * (b + 1), num_lights), bins


def light_contributions(lights, begin, end, p, n):
    """:41-66 -> (contributions (N, BIN_MAX), 0 behind the bin's end; decided (N, BIN_MAX): the facing tests of that light have a margin
    of 1e-5 of the vectors' lengths, so that a binary32 evaluation takes the same branch). The solid angle is the exact one
    (tri_solid_angle), which the shader approximates within 2 * FAST_ATAN_MAX_ABS_ERROR"""
    L = pad_lights(lights)
    p, n = np.asarray(p, np.float64), np.asarray(n, np.float64)
    idx = np.asarray(begin)[:, None] + np.arange(BIN_MAX)[None, :]
    inside = idx < np.asarray(end)[:, None]
    rec = L[np.minimum(idx, len(L) - 1)]                       # (N, BIN_MAX, 4, 3)
    v = rec[:, :, :3, :] - p[:, None, None, :]
    a, b, c = v[:, :, 0], v[:, :, 1], v[:, :, 2]
    triple = _dot(np.cross(a, b), c)
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    dn = np.stack([_dot(x, n[:, None, :]) for x in (a, b, c)], axis=-1)
    front = triple < 0.0
    above = (dn > 0.0).any(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        omega = tri_solid_angle(v.reshape(-1, 9)).reshape(idx.shape)
    contrib = np.where(front & above, _lum(rec[:, :, 3]) * omega, 0.0) + MIN_IRRADIANCE
    eps = 1e-5
    decided = (np.abs(triple) > eps * la * lb * lc) & (np.abs(dn) > eps * np.stack([la, lb, lc], axis=-1) * np.linalg.norm(n, axis=-1)[:, None, None]).all(axis=-1)
    return np.where(inside, contrib, 0.0), decided & inside


def light_select(contributions, count, sel_y, dtype=np.float64):
    """:68-100 the selection among the first `count` contributions -> (offset of the light the loop ends on -- count when sel_y stays
    at or above the last running sum of a bin shorter than BIN_MAX: the light BEHIND the bin --, its share p of the total, the running
    sums (N, BIN_MAX), NaN behind the end of the walk). dtype = numpy.float32 performs the shader's own binary32 operations in its order (+ and
    / only: exactly rounded in numpy as on the device), numpy.float64 states the rule."""
    c = np.asarray(contributions).astype(dtype)
    count = np.asarray(count)
    y = np.asarray(sel_y).astype(dtype)
    N = len(c)
    total = np.zeros(N, dtype)
    for i in range(BIN_MAX):
        total = np.where(i < count, total + c[:, i], total).astype(dtype)
    p, t = np.zeros(N, dtype), np.zeros(N, dtype)
    chosen, done = np.zeros(N, np.int64), np.zeros(N, bool)
    sums = np.full((N, BIN_MAX), np.nan)
    for i in range(BIN_MAX):
        live = ~done
        chosen = np.where(live, i, chosen)
        act = live & (i < count)
        done |= live & ~act
        with np.errstate(invalid="ignore", divide="ignore"):
            pi = (c[:, i] / total).astype(dtype)
        p = np.where(act, pi, p).astype(dtype)
        t = np.where(act, t + pi, t).astype(dtype)
        sums[:, i] = np.where(act, t, np.nan)
        done |= act & (y < t)
    return chosen, p, sums


def name_light(table, radiance_over_pdf, pdf):
    """the record whose radiance is nearest to radiance_over_pdf * pdf among the table and the zeroed record behind it (every light of a
    test table has its own radiance; the light without radiance and the zeroed record share theirs: compare radiances, not indices)"""
    rad = pad_lights(table)[:len(table) + 1, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        got = np.asarray(radiance_over_pdf, np.float64) * np.asarray(pdf, np.float64)[:, None]
        d = np.abs(np.nan_to_num(got, nan=1e300, posinf=1e300, neginf=-1e300)[:, None, :] - rad[None, :, :]).max(axis=2)
    return np.argmin(d, axis=1)


# the oracle's light_dist / mis_wpdf over the float64 band at its own direction, in the rounding units of light_dist_wpdf_excess (a
# worst-case envelope of the formula's own roundings: tens of ulps of the result on a typical query, see there), every query of
# tests/shade_cases.py light_case: measured on the CPU by tests/test_light_selection_cpu.py, which holds the oracle to them. In plain
# ulps of the result the same excess reaches 158 / 228 on the oracle, on single queries whose direction grazes the light's plane: there
# the rounding of the dot products' terms decides, which the envelope accounts for and a band over input ulps does not.
ORACLE_DIST_EXCESS = 0.18   # measured 0.179
ORACLE_WPDF_EXCESS = 0.16   # measured 0.157


def light_dist_wpdf(l0, l1, l2, p, light_dir, num_bins):
    """:112-124 the distance to the light's plane along light_dir and the area pdf turned solid-angle pdf, over the bins"""
    l0, l1, l2, p, d = (np.asarray(x, np.float64) for x in (l0, l1, l2, p, light_dir))
    e_n = np.cross(l1 - l0, l2 - l0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = _dot(d, e_n)
        dist = _dot(l0 - p, e_n) / den
        return dist, 2.0 * dist * dist / np.abs(den) / num_bins


def sun_dir_pdf(cos_radius):  # rendering/lights/sun.glsl:17-20
    with np.errstate(divide="ignore"):
        return 1.0 / (2.0 * np.pi * (1.0 - np.asarray(cos_radius, np.float64)))


def nee_mis(pdf_f, pdf_g):  # rendering/mc/nee_interface.glsl:11-15, n_f = n_g = 1
    f, g = np.asarray(pdf_f, np.float64), np.asarray(pdf_g, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return f / (f + g)


# ---------------------------------------------------------------- output
def linear_to_srgb(x):  # rendering/util.glsl:19-28 (positive_pow clamps its base to FLT_EPSILON)
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x <= float(F32(0.0031308)), 12.92 * x, 1.055 * np.maximum(np.abs(x), 2.0 ** -23) ** (1.0 / 2.4) - 0.055)


# ---------------------------------------------------------------- dequantisation, librender/dequantize.glsl
def dequantize_position(q, scaling, offset):  # :8-21
    q = np.asarray(q, np.uint64)
    c = np.stack([(q >> np.uint64(s)) & np.uint64(0x1FFFFF) for s in (0, 21, 42)], axis=1).astype(np.float64)
    return c * np.asarray(scaling, np.float64) + np.asarray(offset, np.float64)


def dequantize_normal(word):  # :23-41 (octahedral)
    w = np.asarray(word, np.uint64) & np.uint64(0xFFFFFFFF)
    x = ((w & np.uint64(0xFFFF)).astype(np.float64) - 32768.0) / 32767.0
    y = ((w >> np.uint64(16)).astype(np.float64) - 32768.0) / 32767.0
    l1 = np.abs(x) + np.abs(y)
    fold = l1 >= 1.0
    fx = np.where(fold, (1.0 - np.abs(y)) * np.where(x >= 0, 1.0, -1.0), x)
    fy = np.where(fold, (1.0 - np.abs(x)) * np.where(y >= 0, 1.0, -1.0), y)
    return _norm(np.stack([fx, fy, 1.0 - l1], axis=1))


def dequantize_uv(word):  # :43-48
    w = np.asarray(word, np.uint64) & np.uint64(0xFFFFFFFF)
    return np.stack([(w & np.uint64(0xFFFF)).astype(np.float64) * (8.0 / 65535.0),
                     1.0 - (w >> np.uint64(16)).astype(np.float64) * (8.0 / 65535.0)], axis=1)


# ---------------------------------------------------------------- textures (oracle/oshade.h "textures": the Vulkan texel filtering)
SRGB_DECODE = np.array([c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4 for c in np.arange(256) / 255.0])


def _texels(level, srgb):
    t = level.astype(np.float64) / 255.0
    if srgb:
        t[..., :3] = SRGB_DECODE[level[..., :3]]
    return t


def bilinear(level, srgb, uv):
    """one level (h, w, 4) uint8 at uv (N, 2): texel centres at (i + 0.5) / size, REPEAT addressing"""
    h, w = level.shape[:2]
    t = _texels(level, srgb)
    uv = np.asarray(uv, np.float64)
    x, y = uv[:, 0] * w - 0.5, uv[:, 1] * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix0, iy0 = np.mod(x0, w).astype(np.int64), np.mod(y0, h).astype(np.int64)
    ix1, iy1 = (ix0 + 1) % w, (iy0 + 1) % h
    top = t[iy0, ix0] * (1 - fx) + t[iy0, ix1] * fx
    bot = t[iy1, ix0] * (1 - fx) + t[iy1, ix1] * fx
    return top * (1 - fy) + bot * fy


def texture_lod(levels, srgb, uv, lod):
    """lod clamped to [0, min(levels - 1, 16)] (NaN: 0), the two nearest levels blended by the fraction"""
    lod = np.broadcast_to(np.asarray(lod, np.float64), (len(uv),))
    lod = np.clip(np.nan_to_num(lod, nan=0.0), 0.0, min(len(levels) - 1, 16))
    hi = np.floor(lod).astype(np.int64)
    d = (lod - hi)[:, None]
    out = np.zeros((len(uv), 4))
    for l in np.unique(hi):
        s = hi == l
        a = bilinear(levels[l], srgb, uv[s])
        b = bilinear(levels[min(l + 1, len(levels) - 1)], srgb, uv[s])
        out[s] = a * (1 - d[s]) + b * d[s]
    return out


def texture_grad(levels, srgb, uv, ddx, ddy, max_aniso=12.0):
    """rho = |d * size|, eta = min(rho_max / rho_min, 12), N = ceil(eta) taps along the major axis at log2(rho_max / eta); a footprint
    inside one texel and 1 x 1 textures: one bilinear tap of level 0"""
    h, w = levels[0].shape[:2]
    uv, ddx, ddy = (np.asarray(a, np.float64) for a in (uv, ddx, ddy))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rx = np.hypot(ddx[:, 0] * w, ddx[:, 1] * h)
        ry = np.hypot(ddy[:, 0] * w, ddy[:, 1] * h)
        rmax, rmin = np.maximum(rx, ry), np.minimum(rx, ry)
        out = bilinear(levels[0], srgb, uv)
        go = (rmax > 1.0) & (not (w == 1 and h == 1))
        eta = np.where(rmin > 0, np.minimum(rmax / np.where(rmin > 0, rmin, 1.0), max_aniso), max_aniso)
        eta = np.where(np.isnan(eta), max_aniso, eta)
        ntap = np.ceil(eta).astype(np.int64)
        lod = np.log2(rmax / eta)
        major = np.where((rx > ry)[:, None], ddx, ddy)
    for k in np.unique(ntap[go]):
        s = go & (ntap == k)
        acc = np.zeros((s.sum(), 4))
        for i in range(1, k + 1):
            acc += texture_lod(levels, srgb, uv[s] + major[s] * (i / (k + 1) - 0.5), lod[s])
        out[s] = acc / k
    return out


# ---------------------------------------------------------------- comparison rule
def ulp32(x):
    """the spacing of binary32 numbers at |x| (the smallest denormal at 0)"""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    a = np.where(np.isfinite(a), a, np.float32(3.4e38))
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def neighbours(arrays, count, seed=0):
    """`count` copies of the binary32 input arrays with every component moved one ulp up or down at random (NaN / inf stay)"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        out = []
        for a in arrays:
            a = np.asarray(a, np.float32)
            up = rng.random(a.shape) < 0.5
            out.append(np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32))
        yield out


def band(fn, arrays, count=8, seed=0):
    """(lo, hi): elementwise min / max of fn over the inputs and `count` one-ulp neighbourhoods of them (fn returns one array)"""
    v = np.asarray(fn(*arrays), np.float64)
    lo, hi = v.copy(), v.copy()
    for nb in neighbours(arrays, count, seed):
        w = np.asarray(fn(*nb), np.float64)
        with np.errstate(invalid="ignore"):
            lo, hi = np.fmin(lo, w), np.fmax(hi, w)
    return lo, hi


def light_dist_wpdf_rounding(l0, l1, l2, p, light_dir, num_bins):
    """what the binary32 roundings INSIDE light_dist_wpdf amount to, absolutely, for (light_dist, mis_wpdf): every product of the two dot
    products with e_n and of e_n's own components is rounded to half an ulp of ITSELF, so where a sum of them cancels (a direction that
    grazes the light's plane, a receiver close to it) the result carries 2^-24 of the sum of their magnitudes however small it is. First
    order: err(e_n) per component, err(num) and err(den) from the magnitudes, err(dist) = err(num) / |den| + |num| err(den) / den^2,
    err(wpdf) = wpdf (2 err(dist) / |dist| + err(den) / |den|). The band over input ulps does not see this; band_excess takes it as the
    floor of its unit."""
    l0, l1, l2, p, d = (np.asarray(x, np.float64) for x in (l0, l1, l2, p, light_dir))
    eps = 2.0 ** -24
    u, v, a = l1 - l0, l2 - l0, l0 - p
    e_n = np.cross(u, v)
    au, av = np.abs(u), np.abs(v)
    # (the differences u, v, a are rounded too: an eps of the operands each)
    du, dv = eps * (np.abs(l1) + np.abs(l0)), eps * (np.abs(l2) + np.abs(l0))
    da = eps * (np.abs(l0) + np.abs(p))
    mag = np.stack([au[:, 1] * av[:, 2] + au[:, 2] * av[:, 1], au[:, 2] * av[:, 0] + au[:, 0] * av[:, 2], au[:, 0] * av[:, 1] + au[:, 1] * av[:, 0]], axis=1)
    cross_abs = lambda x, y: np.stack([x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] + x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]], axis=1)  # noqa: E731
    err_en = 2 * eps * mag + cross_abs(du, av) + cross_abs(au, dv)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        num, den = _dot(a, e_n), _dot(d, e_n)
        err_num = 2 * eps * _dot(np.abs(a), np.abs(e_n)) + _dot(np.abs(a), err_en) + _dot(da, np.abs(e_n))
        err_den = 2 * eps * _dot(np.abs(d), np.abs(e_n)) + _dot(np.abs(d), err_en)
        dist = num / den
        err_dist = err_num / np.abs(den) + np.abs(num) * err_den / (den * den)
        w = 2.0 * dist * dist / np.abs(den) / num_bins
        err_w = w * (2.0 * err_dist / np.abs(dist) + err_den / np.abs(den))
    return np.nan_to_num(err_dist, nan=0.0, posinf=0.0), np.nan_to_num(err_w, nan=0.0, posinf=0.0)


def light_dist_wpdf_excess(table, num_bins, p, light_id, light_dir, dist, mis_wpdf, extra_ulps=(0.0, 0.0)):
    """the band excess of a binary32 light_dist and mis_wpdf over light_dist_wpdf at the light `light_id` of each query and at the
    binary32 light_dir handed in (the evaluation's OWN direction: what is held is the arithmetic behind the direction sample)
    -> (light_dist, mis_wpdf in ROUNDING UNITS, light_dist, mis_wpdf in plain ulps of the result).
    A rounding unit is light_dist_wpdf_rounding's worst-case envelope of the formula's own roundings, or an ulp of the result where that
    is larger -- which it practically never is: the envelope charges a full 2^-24 per operation on sums of magnitudes and is 33 .. 46 ulps
    of the result at the median for light_dist (83 .. 117 for mis_wpdf), hundreds to thousands on 1 % of the queries, up to 37 000 / 85 000
    on grazing ones; on no query of the cases is it below one ulp. 0.18 units thus reads: 18 % of a pessimistic envelope, 6 .. 8 ulps of
    light_dist on a typical query.
    extra_ulps: REAL ulps of the result by which the band is widened before the excess is taken (a build that divides through a 1-ulp
    reciprocal: one per division; not multiplied by the envelope). The plain-ulp figures are reported without it.
    Queries whose band is not finite (a direction of NaN, the zeroed light behind the table) measure 0."""
    rec = pad_lights(table)[np.asarray(light_id)].astype(np.float32)
    args = [np.ascontiguousarray(rec[:, k]) for k in range(3)] + [np.asarray(p, np.float32), np.asarray(light_dir, np.float32)]
    floors = light_dist_wpdf_rounding(*args, num_bins)
    units, plain = [], []
    for k, got in ((0, dist), (1, mis_wpdf)):
        lo, hi = band(lambda a, b, c, q, d: light_dist_wpdf(a, b, c, q, d, num_bins)[k], args)
        plain.append(band_excess(got, lo, hi))
        with np.errstate(invalid="ignore"):
            w = extra_ulps[k] * ulp32(np.maximum(np.abs(lo), np.abs(hi)))
        units.append(band_excess(got, lo - w, hi + w, floor=floors[k]))
    return units[0], units[1], plain[0], plain[1]


def band_excess(got, lo, hi, floor=0.0):
    """how far a binary32 result lies outside [lo, hi], in ulps of the band's larger end (at least `floor`); 0 inside; NaN results
    where the band is finite count as inf; where the band itself is not finite nothing is measured"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        scale = np.maximum(ulp32(np.maximum(np.abs(lo), np.abs(hi))), floor)
        d = np.maximum(lo - got, got - hi)
        e = np.where(d > 0, d / scale, 0.0)
    finite = np.isfinite(lo) & np.isfinite(hi)
    e = np.where(finite & ~np.isfinite(got), np.inf, e)
    return np.where(finite, e, 0.0)
