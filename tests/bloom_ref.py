"""numpy restatement of bloom, written from the header of csrc/bloom.h (not from its kernels): the prefilter, the level sizes, the down
and up pyramids and the composite. float32 in the header's operation order, every product and sum rounded on its own; the gain in float64,
rounded once. Images are (H, W, 4) arrays, row 0 at the top; pyramid levels are (h_l, w_l, 4) with w = +0.
"""
import numpy as np

import auto_exposure_ref as A
import denoise_ref as D

F = np.float32
MAX_LEVELS = 12
DEFAULTS = dict(source=0, exposure_mode=0, tone_mapping_mode=-1, levels=0, threshold=1.0, knee=0.5, clamp=16.0, intensity=0.2, scatter=0.7,
                white_balance=(1.0, 1.0, 1.0))


def _f(x):
    return np.ascontiguousarray(x, dtype=F)


def sizes(W, H):
    """[(w_0, h_0), (w_1, h_1), ... (1, 1)]: the last index is L_max"""
    out = [(int(W), int(H))]
    while True:
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
        if out[-1] == (1, 1):
            return out


def level_count(W, H, levels=0):
    """L of a call"""
    s = sizes(W, H)
    l_max = len(s) - 1
    if levels == 0:
        ok = [l for l in range(1, min(8, l_max) + 1) if min(s[l]) >= 2]
        return max(ok) if ok else 1
    return min(int(levels), l_max)


def prefilter(src, scale, threshold=1.0, knee=0.5, clamp=16.0):
    """the prefiltered source: (H, W, 4) with w = +0"""
    src = _f(src)
    T, K, C, s = F(threshold), F(knee), F(clamp), F(scale)
    with np.errstate(all="ignore"):
        x = (src[..., :3] * s).astype(F)
        dead = ~(np.fmin(src[..., 3], F(1)) >= 0) | ~np.isfinite(x).all(axis=-1)
        x = np.where(x > 0, x, F(0)).astype(F)
        b = np.maximum(np.maximum(x[..., 0], x[..., 1]), x[..., 2])
        tk, k2, k4e = F(T - K), F(F(2) * K), F(F(4) * K + F(1e-5))
        q = np.minimum(np.maximum((b - tk).astype(F), F(0)), k2)
        q = ((q * q).astype(F) / k4e).astype(F)
        e = np.minimum(np.maximum(q, (b - T).astype(F)), C)
        f = (e / np.maximum(b, F(1e-5))).astype(F)
        p = (x * f[..., None]).astype(F)
    p = np.where(dead[..., None], F(0), p).astype(F)
    return np.concatenate([p, np.zeros(p.shape[:-1] + (1,), F)], -1)


def _1331(a, b, c, d):
    return ((F(0.125) * a + F(0.375) * b).astype(F) + (F(0.375) * c + F(0.125) * d).astype(F)).astype(F)


def down(img):
    """one level: (h, w, 4) -> ((h + 1) // 2, (w + 1) // 2, 4)"""
    img = _f(img)[..., :3]
    h, w = img.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    xs = [np.clip(2 * np.arange(dw) - 1 + i, 0, w - 1) for i in range(4)]
    ys = [np.clip(2 * np.arange(dh) - 1 + j, 0, h - 1) for j in range(4)]
    with np.errstate(all="ignore"):
        rows = []
        for j in range(4):
            line = img[ys[j]]
            rows.append(_1331(line[:, xs[0]], line[:, xs[1]], line[:, xs[2]], line[:, xs[3]]))
        d = _1331(rows[0], rows[1], rows[2], rows[3])
    return np.concatenate([d, np.zeros((dh, dw, 1), F)], -1)


def upsample(u, w, h):
    """B(u) on a w x h grid: (h, w, 3)"""
    u = _f(u)[..., :3]
    ch, cw = u.shape[:2]
    x, y = np.arange(w), np.arange(h)
    i0, i1 = np.clip((x - 1) >> 1, 0, cw - 1), np.clip(((x - 1) >> 1) + 1, 0, cw - 1)
    j0, j1 = np.clip((y - 1) >> 1, 0, ch - 1), np.clip(((y - 1) >> 1) + 1, 0, ch - 1)
    a0 = np.where(x & 1, F(0.75), F(0.25)).astype(F)[None, :, None]
    a1 = np.where(x & 1, F(0.25), F(0.75)).astype(F)[None, :, None]
    b0 = np.where(y & 1, F(0.75), F(0.25)).astype(F)[:, None, None]
    b1 = np.where(y & 1, F(0.25), F(0.75)).astype(F)[:, None, None]
    with np.errstate(all="ignore"):
        h0 = ((a0 * u[j0][:, i0]).astype(F) + (a1 * u[j0][:, i1]).astype(F)).astype(F)
        h1 = ((a0 * u[j1][:, i0]).astype(F) + (a1 * u[j1][:, i1]).astype(F)).astype(F)
        return ((b0 * h0).astype(F) + (b1 * h1).astype(F)).astype(F)


def pyramids(src, scale, levels=0, threshold=1.0, knee=0.5, clamp=16.0, scatter=0.7, **_):
    """-> (d, u): dicts level -> (h_l, w_l, 4), levels 1 .. L"""
    src = _f(src)
    H, W = src.shape[:2]
    L = level_count(W, H, levels)
    d = {0: prefilter(src, scale, threshold, knee, clamp)}
    for l in range(1, L + 1):
        d[l] = down(d[l - 1])
    u = {L: d[L].copy()}
    for l in range(L - 1, 0, -1):
        hl, wl = d[l].shape[:2]
        with np.errstate(all="ignore"):
            v = (F(scatter) * upsample(u[l + 1], wl, hl)).astype(F)
            u[l] = np.concatenate([(d[l][..., :3] + v).astype(F), np.zeros((hl, wl, 1), F)], -1)
    del d[0]
    return d, u


def gain(intensity, scatter, L):
    total, term = 0.0, 1.0
    for _ in range(L):
        total += term
        term *= float(F(scatter))
    return F(float(F(intensity)) / total)


def composite(src, fb, scale, u1, L, intensity=0.2, scatter=0.7, tone_mapping_mode=-1, white_balance=(1.0, 1.0, 1.0), **_):
    """the display image: auto_exposure_ref.expose with gain * B(u(1)) added to the exposed colour"""
    src = _f(src)
    H, W = src.shape[:2]
    with np.errstate(all="ignore"):
        x = (src[..., :3] * F(scale)).astype(F)
        if F(intensity) != 0:
            x = (x + (gain(intensity, scatter, L) * upsample(u1, W, H)).astype(F)).astype(F)
        g = [F(v) for v in white_balance]
        if not (g[0] == 1 and g[1] == 1 and g[2] == 1):
            l = np.stack([A._row(A.M1[k], x) * g[k] for k in range(3)], -1).astype(F)
            x = np.stack([A._row(A.M2[k], l) for k in range(3)], -1).astype(F)
        w = np.fmin(src[..., 3], F(1))
        o = np.concatenate([x, w[..., None]], -1).astype(F)
        shown = D.to_rgba8(D.display(o, 0.0, tone_mapping_mode))
    return np.where((w >= 0)[..., None], shown, np.asarray(fb, np.uint8))


def bloom(src, fb, scale, **params):
    """one call -> (d, u, image)"""
    p = dict(DEFAULTS, **params)
    d, u = pyramids(src, scale, **p)
    return d, u, composite(src, fb, scale, u[1], len(d), **p)


def same_bits(a, b):
    a, b = _f(a), _f(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
