"""numpy restatement of the denoiser, written from the header of csrc/denoise.h (not from its kernels): prepare, the a-trous passes,
finish and the RGBA8 image. float32 throughout in the header's operation order; exp / pow / exp2 / log2 in float64, rounded once;
sums left to right in scan order (dy outer, dx inner); min / max as fmin / fmax. Images are (H, W, 4) arrays, row 0 at the top.
"""
import numpy as np

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_depth=1.0, normal_power_log2=7, demodulate_albedo=1)


def _f(x):
    return np.ascontiguousarray(x, dtype=F)


def _lum(e):
    return (F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1]) + F(0.0722) * e[..., 2]


def _shift(img, ox, oy, fill=0):
    """img at p + (ox, oy) for every pixel p; `fill` outside the image"""
    H, W = img.shape[:2]
    out = np.full_like(img, fill)
    ys0, ys1 = max(0, -oy), min(H, H - oy)
    xs0, xs1 = max(0, -ox), min(W, W - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = img[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def surface(nd, albedo):
    nd, A = _f(nd), _f(albedo)
    n, z = nd[..., :3], nd[..., 3]
    with np.errstate(all="ignore"):
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        return np.isfinite(z) & (z > 0) & (nn > 0) & ~((A[..., 0] == 0) & (A[..., 1] == 0) & (A[..., 2] == 0))


def divisor(albedo):
    return np.fmax(_f(albedo)[..., :3], F(0.01))


def prepare(accum, albedo, nd, demodulate=1):
    """-> (ev, ndz, gz, surf): the (e, v) image, (N, z) with zeros where the pixel is not surface, the depth gradient, the mask"""
    accum, nd = _f(accum), _f(nd)
    H, W = accum.shape[:2]
    surf = surface(nd, albedo)
    c = accum[..., :3]
    with np.errstate(all="ignore"):
        e = np.where(surf[..., None], c / divisor(albedo), c) if demodulate else c.copy()
    e = _f(e)
    lum = np.where(surf, _lum(e), F(0)).astype(F)
    ndz = np.where(surf[..., None], nd, F(0)).astype(F)
    z = ndz[..., 3]
    s1 = np.zeros((H, W), F)
    s2 = np.zeros((H, W), F)
    n = np.zeros((H, W), np.int32)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nq = _shift(ndz, dx, dy)
                lq = _shift(lum, dx, dy)
                take = (nq[..., 3] > 0) & (((ndz[..., 0] * nq[..., 0] + ndz[..., 1] * nq[..., 1]) + ndz[..., 2] * nq[..., 2]) > 0)
                s1 = np.where(take, s1 + lq, s1)
                s2 = np.where(take, s2 + lq * lq, s2)
                n += take
        nf = np.maximum(n, 1).astype(F)
        m1, m2 = s1 / nf, s2 / nf
        v = np.where(surf, np.fmax(m2 - m1 * m1, F(0)), F(0)).astype(F)
        gz = np.zeros((H, W), F)
        for dx, dy in ((1, 0), (0, 1)):
            zq = _shift(z, dx, dy)
            gz = np.where(zq > 0, np.fmax(gz, np.abs(zq - z)), gz)
        gz = np.where(surf, gz, F(0)).astype(F)
    ev = np.concatenate([e, v[..., None]], axis=-1).astype(F)
    return ev, ndz, gz, surf


def atrous_pass(ev, ndz, gz, i, sigma_luminance, sigma_depth, normal_power_log2):
    """pass i (spacing 1 << i) over the (e, v) image"""
    s = 1 << i
    H, W = ev.shape[:2]
    surf = ndz[..., 3] > 0
    lum_p = _lum(ev)
    zp = ndz[..., 3]
    sw = np.zeros((H, W), F)
    sv = np.zeros((H, W), F)
    se = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        den_l = F(sigma_luminance) * np.sqrt(ev[..., 3]) + F(1e-4)
        den_z0 = (F(sigma_depth) * gz) * F(s)
        den_z1 = F(1e-3) * zp
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ndq = _shift(ndz, s * dx, s * dy)
                evq = _shift(ev, s * dx, s * dy)
                take = surf & (ndq[..., 3] > 0)
                h = K[abs(dx)] * K[abs(dy)]
                t = (ndz[..., 0] * ndq[..., 0] + ndz[..., 1] * ndq[..., 1]) + ndz[..., 2] * ndq[..., 2]
                t = np.fmin(np.fmax(t, F(0)), F(1))
                for _ in range(int(normal_power_log2)):
                    t = t * t
                az = np.abs(ndq[..., 3] - zp) / (den_z0 * F(max(abs(dx), abs(dy))) + den_z1)
                al = np.abs(_lum(evq) - lum_p) / den_l
                w = ((h * t) * np.exp((-(az + al)).astype(np.float64)).astype(F)).astype(F)
                sw = np.where(take, sw + w, sw)
                se = np.where(take[..., None], se + w[..., None] * evq[..., :3], se)
                sv = np.where(take, sv + (w * w) * evq[..., 3], sv)
        out = np.concatenate([se / sw[..., None], (sv / (sw * sw))[..., None]], axis=-1).astype(F)
    return np.where(surf[..., None], out, ev).astype(F)


def srgb(x):
    x = _f(x)
    p = np.power(np.fmax(np.abs(x), F(1.192092896e-07)).astype(np.float64), np.float64(F(1.0) / F(2.4))).astype(F)
    return np.where(x <= F(0.0031308), F(12.92) * x, F(1.055) * p - F(0.055)).astype(F)


def display(o, exposure=0.0, tone_mapping_mode=-1):
    """the header's display colour of (rgb, alpha)"""
    o = _f(o)
    x = o[..., :3] * np.exp2(np.float64(F(exposure))).astype(F)
    with np.errstate(all="ignore"):
        if tone_mapping_mode == 2:
            x = x / (F(1) + x)
        elif tone_mapping_mode == 1:
            L = np.fmax(np.fmax(x[..., 0], x[..., 1]), np.fmax(x[..., 2], F(1)))
            g = np.log2(L.astype(np.float64)).astype(F)
            k = ((F(0.1) * g) * (F(1) - F(0.8)) + F(1) * F(0.8)) / L
            x = x * k[..., None]
    return np.concatenate([srgb(x), o[..., 3:]], axis=-1).astype(F)


def to_rgba8(c):
    return (np.fmin(np.fmax(_f(c), F(0)), F(1)) * F(255) + F(0.5)).astype(np.uint8)


def denoise(accum, albedo, nd, fb=None, iterations=5, sigma_luminance=4.0, sigma_depth=1.0, normal_power_log2=7, demodulate_albedo=1,
            output_channel=0, exposure=0.0, tone_mapping_mode=-1):
    """-> (RGBA32F image, RGBA8 image or None without fb). accum: the frame's accumulation image; albedo / nd: its albedo + roughness
    and normal + depth AOVs (float16 or float32); fb: its RGBA8 frame"""
    accum = _f(accum)
    ev, ndz, gz, surf = prepare(accum, albedo, nd, demodulate_albedo)
    for i in range(iterations):
        ev = atrous_pass(ev, ndz, gz, i, sigma_luminance, sigma_depth, normal_power_log2)
    rgb = ev[..., :3] * divisor(albedo) if demodulate_albedo else ev[..., :3]
    out = accum.copy()
    out[..., :3] = np.where(surf[..., None], rgb, accum[..., :3])
    if fb is None:
        return out, None
    u8 = np.array(fb, np.uint8, copy=True)
    if output_channel == 0:
        o = out.copy()
        o[..., 3] = np.fmin(out[..., 3], F(1))
        shown = to_rgba8(display(o, exposure, tone_mapping_mode))
        u8 = np.where((o[..., 3] >= 0)[..., None], shown, u8)
    return out, u8
