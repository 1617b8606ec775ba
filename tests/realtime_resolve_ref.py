"""numpy restatement of the real-time resolve (csrc/realtime_resolve.h): reprojection_mode 2 (rendering/postprocess/reprojection.glsl:43-367
with BOUNDARY_SEARCH, BILATERAL, BILATERAL_PROJECTION, FIT_GEOMETRY_DISTRIBUTION) and the TAA pass (vulkan/processing/process_taa.comp).

Vectorised over the image, float32 throughout, in the operation order of the kernels and with their sampling rules (the header of
realtime_resolve.h): bilinear history over texel centres clamped to the edge, zero outside the image for texelFetch / imageLoad,
min / max as fmin / fmax (a NaN operand yields the other one). Images are (H, W, 4) arrays, row 0 at the top as the library stores them.
"""
import numpy as np

F = np.float32


def _f(x):
    return np.asarray(x, dtype=F)


def _fetch(img, x, y):
    """texelFetch / imageLoad at integer coordinates (arrays), zero outside"""
    H, W = img.shape[:2]
    inside = (x >= 0) & (y >= 0) & (x < W) & (y < H)
    v = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
    return np.where(inside[..., None], v, F(0))


def _shift(img, ox, oy):
    """imageLoad(img, p + (ox, oy)) for every pixel p, zero outside"""
    H, W = img.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    return _fetch(img, xs + ox, ys + oy)


def _trunc_i(v):
    return np.trunc(np.fmin(np.fmax(_f(v), F(-1073741824.0)), F(1073741824.0))).astype(np.int64)


def _bilinear(img, u, v):
    H, W = img.shape[:2]
    x = u * F(W) - F(0.5)
    y = v * F(H) - F(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = x - x0f, y - y0f
    x0, y0 = _trunc_i(x0f), _trunc_i(y0f)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    c00, c10, c01, c11 = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]
    w00 = ((F(1) - fx) * (F(1) - fy))[..., None]
    w10 = (fx * (F(1) - fy))[..., None]
    w01 = ((F(1) - fx) * fy)[..., None]
    w11 = (fx * fy)[..., None]
    return ((w00 * c00 + w10 * c10) + w01 * c01) + w11 * c11


def _smoothstep(e0, e1, x):
    t = np.fmin(np.fmax((x - F(e0)) / (F(e1) - F(e0)), F(0)), F(1))
    return t * t * (F(3) - F(2) * t)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def reproject(mean, nd, mj, hist, hist_nd, spp, window, use_history=True, return_weight=False):
    """One frame of reprojection_mode 2.
    mean: this frame's mean (RGBA32F, alpha = coverage); nd / mj: its normal + depth and motion + jitter AOVs (float16 or float32);
    hist / hist_nd: what the previous frame left (its stored accumulation image and its normal + depth); use_history False: the frame
    resets (sample_base_index == 0). Returns (stored, shown): the accumulation image (history.rgb, 1 - new_sample_weight) and the colour
    the frame shows before rp_display_color (history.rgb with the frame's coverage alpha clamped to 1); with return_weight also the
    new-sample weight per pixel."""
    mean = _f(mean)
    H, W = mean.shape[:2]
    if not use_history:
        shown = mean.copy()
        shown[..., 3] = np.fmin(mean[..., 3], F(1))
        w = np.ones((H, W), F)
        return (mean.copy(), shown, w) if return_weight else (mean.copy(), shown)
    nd, mj, hist, hist_nd = _f(nd), _f(mj), _f(hist), _f(hist_nd)
    fw, fh = F(W), F(H)
    ys, xs = np.mgrid[0:H, 0:W]
    mot = mj[..., :2]
    m0 = mot
    # BOUNDARY_SEARCH, centre: the longest motion of the 3x3 ring, scan order, strictly longer wins
    em = m0.copy()
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            m = _shift(mot, ox, oy)
            longer = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) > (em[..., 0] * em[..., 0] + em[..., 1] * em[..., 1])
            em = np.where(longer[..., None], m, em)
    spx = (xs.astype(F) + F(0.5)) / fw
    spy = (ys.astype(F) + F(0.5)) / fh
    rpx = spx + F(0.5) * m0[..., 0]
    rpy = spy + F(0.5) * m0[..., 1]
    apx = _trunc_i(spx + F(0.5) * em[..., 0]).astype(F)
    apy = _trunc_i(spy + F(0.5) * em[..., 1]).astype(F)
    rpx = np.fmin(np.fmax(rpx, np.floor(apx) - F(0.5)), np.floor(apx) + F(1.5))
    rpy = np.fmin(np.fmax(rpy, np.floor(apy) - F(0.5)), np.floor(apy) + F(1.5))
    mx = F(2) * (rpx - spx)
    my = F(2) * (rpy - spy)
    rpx = spx + F(0.5) * mx
    rpy = spy + F(0.5) * my
    inside = (rpx >= 0) & (rpy >= 0) & (rpx < 1) & (rpy < 1)
    hc = np.where(inside[..., None], _bilinear(hist, rpx, rpy), F(0))
    old = F(1) - hc[..., 3]
    new_w = np.where(inside & (old > 0), old / (F(1) + old * F(spp)), F(1)).astype(F)
    msw = F(1) / F(window)
    new_w = np.fmax(new_w, msw)
    new_w = np.where(mean[..., 3] > 1, F(0.95), new_w).astype(F)
    cnd = nd
    bil = new_w < 1
    with np.errstate(all="ignore"):
        rx, ry = _trunc_i(rpx * fw), _trunc_i(rpy * fh)
        an = np.zeros((H, W, 3), F)
        avg_depth = np.zeros((H, W), F)
        sq_depth = np.zeros((H, W), F)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                n = _shift(nd, ox, oy)
                an = an + n[..., :3]
                rel = n[..., 3] / cnd[..., 3]
                avg_depth = avg_depth + rel
                sq_depth = sq_depth + rel * rel
        an = an / F(9)
        avg_depth = avg_depth / F(9)
        sq_depth = sq_depth / F(9)
        normal_sigma = np.fmax(F(1) - np.sqrt(_dot3(an, an)), F(0))
        depth_sigma = np.sqrt(np.fmax(sq_depth - avg_depth * avg_depth, F(0)))
        depth_scale = np.fmin(F(10), F(1) / depth_sigma)
        mix_w = np.zeros((H, W), F)
        mix = np.zeros((H, W, 3), F)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                qx, qy = rx + ox, ry + oy
                h = _fetch(hist, qx, qy)
                nold = F(1) - h[..., 3]
                hn = _fetch(hist_nd, qx, qy)
                angle = _dot3(hn, cnd)
                rdd = np.abs(hn[..., 3] / cnd[..., 3] - F(1))
                w = _smoothstep(-0.66, 1.0, angle + normal_sigma) * np.fmin(np.fmax(F(0), F(1) - depth_scale * rdd), F(1))
                dx = (qx.astype(F) + F(0.5)) - rpx * fw
                dy = (qy.astype(F) + F(0.5)) - rpy * fh
                # exp correctly rounded to float32 (evaluated in float64, rounded once), as the kernel does
                w = (w * np.exp((F(-3) * (dx * dx + dy * dy)).astype(np.float64)).astype(F)).astype(F)
                take = nold > 0
                mix_w = np.where(take, mix_w + w, mix_w)
                mix = np.where(take[..., None], mix + w[..., None] * h[..., :3], mix)
        mixn = mix / mix_w[..., None]
        line = hc[..., :3] - mean[..., :3]
        t = _dot3(mixn - mean[..., :3], line) / _dot3(line, line)
        proj = np.fmax(new_w, F(1) - np.fmax(t, F(0)))
    w_bil = np.where(mix_w > 0, proj, F(1))
    w_bil = np.fmax(w_bil, msw)
    new_w = np.where(bil, w_bil, new_w).astype(F)
    stored = np.empty_like(mean)
    stored[..., :3] = hc[..., :3] + (mean[..., :3] - hc[..., :3]) * new_w[..., None]
    stored[..., 3] = F(1) - new_w
    shown = stored.copy()
    shown[..., 3] = np.fmin(mean[..., 3], F(1))
    return (stored, shown, new_w) if return_weight else (stored, shown)


def linear_to_srgb(x):
    x = _f(x)
    return np.where(x <= F(0.0031308), F(12.92) * x, F(1.055) * np.power(np.fmax(np.abs(x), F(1.192092896e-07)), F(1.0 / 2.4)) - F(0.055)).astype(F)


def to_rgba8(c):
    return (np.clip(_f(c), 0, 1) * F(255) + F(0.5)).astype(np.uint8)


def display(shown):
    """rp_display_color for the default parameters (colour output, exposure 0, no tone mapping) and the RGBA8 store; pixels whose
    alpha is negative keep what the frame buffer held (returned as None where that matters: the tests' scenes have none)"""
    o = _f(shown).copy()
    o[..., :3] = linear_to_srgb(o[..., :3])
    return to_rgba8(o)


def _lanczos_weight(x, r):
    pi = F(np.pi)
    with np.errstate(all="ignore"):
        v = F(r) * np.sin(x * pi) * np.sin((x / F(r)) * pi) / (pi * pi * x * x)
    return np.where(x == 0, F(1), v).astype(F)


def taa(pre, hist, mj):
    """The TAA pass of one frame: pre = this frame's RGBA8 image before the pass, hist = the previous frame's RGBA8 image after it,
    mj = this frame's motion + jitter AOV. Neighbours are read from `pre` (the reference reads the frame it writes, a race); the
    motion is the centre pixel's (its 3x3 loop loads the centre nine times). render_upscale_factor 1. Returns the RGBA8 result."""
    pre = _f(pre) / F(255)
    hist = _f(hist) / F(255)
    mj = _f(mj)
    H, W = pre.shape[:2]
    fw, fh = F(W), F(H)
    ys, xs = np.mgrid[0:H, 0:W]
    motion = mj[..., :2]
    spx = (xs.astype(F) + F(0.5)) / fw
    spy = (ys.astype(F) + F(0.5)) / fh
    rpx = spx + F(0.5) * motion[..., 0]
    rpy = spy + F(0.5) * motion[..., 1]
    inside = (rpx >= 0) & (rpy >= 0) & (rpx <= 1) & (rpy <= 1)
    ptx = rpx * fw - F(0.5)
    pty = rpy * fh - F(0.5)
    cpx, cpy = np.ceil(ptx), np.ceil(pty)
    acc = np.zeros((H, W, 4), F)
    total = np.zeros((H, W), F)
    for oy in range(-5, 5):
        for ox in range(-5, 5):
            npx = F(ox) + cpx
            npy = F(oy) + cpy
            w = _lanczos_weight(npx - ptx, 5.0) * _lanczos_weight(npy - pty, 5.0)
            v = _fetch(hist, _trunc_i(npx), _trunc_i(npy))
            acc = acc + w[..., None] * v
            total = total + w
    with np.errstate(all="ignore"):
        hc = acc / total[..., None]
    trim = np.zeros((H, W, 4), F)
    max2 = np.zeros((H, W, 4), F)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            v = _shift(pre, ox, oy)
            trim = trim + v
            max2 = max2 + v * v
    trim = trim / F(9)
    max2 = np.sqrt(max2 / F(9))
    sd = F(9.0 / 8.0) * (max2 - trim)
    lo = np.fmax(F(0), trim - sd)
    hi = np.fmax(trim + F(3) * sd, pre + sd)
    v = hc + (pre - hc) * F(0.15)
    blended = np.fmin(np.fmax(v, lo), hi)
    out = np.where(inside[..., None], blended, pre)
    return to_rgba8(out)
