"""numpy restatement of auto-exposure, written from the header of csrc/auto_exposure.h (not from its kernels): the meter's histogram,
the target, the adaptation and the display image. float32 in the header's operation order; exp / exp2 / log2 in float64, rounded
once; the percentile walk and its sums in ascending bin order. Images are (H, W, 4) arrays (or (N, 4) texel lists), row 0 at the top.
"""
import math

import numpy as np

import denoise_ref as D

F = np.float32
DEFAULTS = dict(source=0, mode=1, reset_history=0, tone_mapping_mode=-1, key=0.18, low_percentile=0.5, high_percentile=0.95, min_ev=-8.0,
                max_ev=8.0, speed_up=1.0, speed_down=3.0, dt=0.0, white_balance=(1.0, 1.0, 1.0))
T = [math.log2(1.0 + (s + 0.5) / 8.0) for s in range(8)]
M1 = ((3.90405e-1, 5.49941e-1, 8.92632e-3), (7.08416e-2, 9.63172e-1, 1.35775e-3), (2.31082e-2, 1.28021e-1, 9.36245e-1))
M2 = ((2.85847e+0, -1.62879e+0, -2.48910e-2), (-2.10182e-1, 1.15820e+0, 3.24281e-4), (-4.18120e-2, -1.18169e-1, 1.06867e+0))


def _f(x):
    return np.ascontiguousarray(x, dtype=F)


def luminance(src):
    src = _f(src)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * src[..., 0] + F(0.7152) * src[..., 1]) + F(0.0722) * src[..., 2]).astype(F)


def bins(src):
    """-> (bin per texel, ignored mask); the bin of an ignored texel means nothing"""
    src = _f(src)
    lum = luminance(src)
    with np.errstate(all="ignore"):
        ignored = (src[..., 3] < 0) | ~(lum >= 0) | np.isinf(lum)
    b = (np.abs(lum).view(np.uint32) >> np.uint32(20)).astype(np.int64) - 887
    return np.clip(b, 0, 255), ignored


def meter(src):
    """-> (histogram of 256 words, counted, black, ignored)"""
    b, ign = bins(src)
    hist = np.bincount(b[~ign].ravel(), minlength=256).astype(np.uint32)
    return hist, int(hist[1:].sum()), int(hist[0]), int(ign.sum())


def representative(b):
    """v_b of bin b >= 1"""
    return float((b - 1) // 8 - 16) + T[(b - 1) % 8]


def percentile_mean(hist, low_percentile, high_percentile):
    """the target rule's walk -> (m, N); m is None when N = 0"""
    n = int(np.asarray(hist[1:], np.uint64).sum())
    lo = int(float(F(low_percentile)) * float(n))
    hi = int(float(F(high_percentile)) * float(n))
    c, N, S = 0, 0, 0.0
    for b in range(1, 256):
        hb = int(hist[b])
        tb = min(c + hb, hi) - max(c, lo)
        if tb > 0:
            S += float(tb) * representative(b)
            N += tb
        c += hb
    return (S / float(N) if N > 0 else None), N


def target_ev(hist, p, ev):
    """-> (target, mean_log2) as float32; ev: the current value or None"""
    m, _ = percentile_mean(hist, p["low_percentile"], p["high_percentile"])
    if m is None:
        return F(0.0 if ev is None else ev), F(0.0)
    t = min(max(math.log2(float(F(p["key"]))) - m, float(F(p["min_ev"]))), float(F(p["max_ev"])))
    return F(t), F(m)


def adapt(ev, target, p):
    """ev: the current value (float32) or None when there is no state"""
    if ev is None or p["reset_history"] or F(p["dt"]) == 0:
        return F(target)
    r = p["speed_up"] if F(target) > F(ev) else p["speed_down"]
    k = 1.0 - math.exp(-float(F(p["dt"])) * float(F(r)))
    return F(float(F(ev)) + (float(F(target)) - float(F(ev))) * k)


def scale_of(exposure, ev):
    """float(exp2(double(E))), E = exposure + ev in float32"""
    return F(np.exp2(np.float64(F(exposure) + F(ev))))


def step(src, p, state, exposure=0.0):
    """one mode-1 call: state is None (no state since initialize) or the dict a previous step returned -> the new state"""
    p = dict(DEFAULTS, **p)
    hist, counted, black, ignored = meter(src)
    ev = None if state is None else state["ev"]
    target, mean = target_ev(hist, p, ev)
    ev1 = adapt(ev, target, p)
    fresh = state is None or p["reset_history"]
    return dict(ev=ev1, target_ev=target, mean_log2=mean, scale=scale_of(exposure, ev1), counted=counted, black=black, ignored=ignored,
                calls=1 if fresh else state["calls"] + 1, histogram=hist)


def _row(m, x):
    return (F(m[0]) * x[..., 0] + F(m[1]) * x[..., 1]) + F(m[2]) * x[..., 2]


def expose(src, fb, scale, tone_mapping_mode=-1, white_balance=(1.0, 1.0, 1.0)):
    """the display image: src (the float image), fb (the frame's RGBA8), scale (float32)"""
    src = _f(src)
    with np.errstate(all="ignore"):
        x = (src[..., :3] * F(scale)).astype(F)
        g = [F(v) for v in white_balance]
        if not (g[0] == 1 and g[1] == 1 and g[2] == 1):
            l = np.stack([_row(M1[k], x) * g[k] for k in range(3)], -1).astype(F)
            x = np.stack([_row(M2[k], l) for k in range(3)], -1).astype(F)
        w = np.fmin(src[..., 3], F(1))
        o = np.concatenate([x, w[..., None]], -1).astype(F)
        shown = D.to_rgba8(D.display(o, 0.0, tone_mapping_mode))   # (exposure 0: x * 1 = x, the scale is applied above)
    return np.where((w >= 0)[..., None], shown, np.asarray(fb, np.uint8))


def state_of(st):
    """an abi.ExposureState as the dict step() returns"""
    return dict(ev=F(st.ev), target_ev=F(st.target_ev), mean_log2=F(st.mean_log2), scale=F(st.scale), counted=int(st.counted), black=int(st.black),
                ignored=int(st.ignored), calls=int(st.calls), histogram=np.array(st.histogram[:], np.uint32))


def same_state(a, b):
    """bit for bit: the four floats, the four counts, the histogram; -> list of the fields that differ"""
    bad = [k for k in ("ev", "target_ev", "mean_log2", "scale") if F(a[k]).view(np.uint32) != F(b[k]).view(np.uint32)]
    bad += [k for k in ("counted", "black", "ignored", "calls") if int(a[k]) != int(b[k])]
    if not np.array_equal(a["histogram"], b["histogram"]):
        bad.append("histogram")
    return bad
