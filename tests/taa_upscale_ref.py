"""numpy restatement of temporal upscaling (csrc/taa_upscale.h): the TAA pass of vulkan/processing/process_taa.comp run per DISPLAY pixel
of an (f H, f W) image over a frame rendered at (H, W), f = render_upscale_factor.

Vectorised over the display image, float32 throughout, in the operation order of the kernel's header and with the sampling rules of
tests/realtime_resolve_ref.py (texelFetch / imageLoad read zero outside the image, min / max as fmin / fmax). With f = 1 it is that
file's taa() bit for bit (tests/test_taa_upscale_cpu.py). Images are (rows, columns, 4) arrays, row 0 at the top.
"""
import numpy as np

import realtime_resolve_ref as R

F = np.float32


def replicate(pre, factor=2):
    """every rendered pixel as a factor x factor block: the output of a call without history"""
    return np.repeat(np.repeat(np.asarray(pre), factor, axis=0), factor, axis=1)


def branches(mj, factor=2):
    """(inside, nan): per display pixel, whether the reconstruction point lies in [0, 1]^2 (the history is used) and whether the
    motion is NaN (sky pixels: the test fails, the pixel keeps the frame's value)"""
    mj = R._f(mj)
    H, W = mj.shape[:2]
    f = int(factor)
    ys, xs = np.mgrid[0:f * H, 0:f * W]
    motion = mj[ys // f, xs // f, :2]
    rpx = (xs.astype(F) + F(0.5)) / F(f * W) + F(0.5) * motion[..., 0]
    rpy = (ys.astype(F) + F(0.5)) / F(f * H) + F(0.5) * motion[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (rpx >= 0) & (rpy >= 0) & (rpx <= 1) & (rpy <= 1)
    return inside, np.isnan(motion).any(axis=-1)


def taa_upscale(pre, hist, mj, factor=2):
    """pre: the frame's RGBA8 image (H, W, 4); hist: the previous output (f H, f W, 4) RGBA8; mj: the frame's motion + jitter AOV
    (H, W, 4). Returns the (f H, f W, 4) RGBA8 result."""
    f = int(factor)
    pre = R._f(pre) / F(255)
    hist = R._f(hist) / F(255)
    mj = R._f(mj)
    H, W = pre.shape[:2]
    DH, DW = f * H, f * W
    assert hist.shape[:2] == (DH, DW)
    fw, fh = F(DW), F(DH)
    ys, xs = np.mgrid[0:DH, 0:DW]
    ry, rx = ys // f, xs // f                      # the render pixel under each display pixel
    col = pre[ry, rx]
    motion = mj[ry, rx, :2]                        # (the reference's 3x3 loop reads the centre nine times)
    spx = (xs.astype(F) + F(0.5)) / fw
    spy = (ys.astype(F) + F(0.5)) / fh
    rpx = spx + F(0.5) * motion[..., 0]
    rpy = spy + F(0.5) * motion[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (rpx >= 0) & (rpy >= 0) & (rpx <= 1) & (rpy <= 1)
    ptx = rpx * fw - F(0.5)
    pty = rpy * fh - F(0.5)
    cpx, cpy = np.ceil(ptx), np.ceil(pty)
    acc = np.zeros((DH, DW, 4), F)
    total = np.zeros((DH, DW), F)
    for oy in range(-5, 5):
        for ox in range(-5, 5):
            npx = F(f * ox) + cpx
            npy = F(f * oy) + cpy
            w = R._lanczos_weight((npx - ptx) / F(f), 5.0) * R._lanczos_weight((npy - pty) / F(f), 5.0)
            v = R._fetch(hist, R._trunc_i(npx), R._trunc_i(npy))
            acc = acc + w[..., None] * v
            total = total + w
    with np.errstate(all="ignore"):
        hc = acc / total[..., None]
    trim = np.zeros((DH, DW, 4), F)
    max2 = np.zeros((DH, DW, 4), F)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            v = R._fetch(pre, rx + ox, ry + oy)    # fb_pixel + f * o of the replicated frame
            trim = trim + v
            max2 = max2 + v * v
    trim = trim / F(9)
    max2 = np.sqrt(max2 / F(9))
    sd = F(9.0 / 8.0) * (max2 - trim)
    lo = np.fmax(F(0), trim - sd)
    hi = np.fmax(trim + F(3) * sd, col + sd)
    with np.errstate(invalid="ignore"):
        v = hc + (col - hc) * F(0.15)
    blended = np.fmin(np.fmax(v, lo), hi)
    out = np.where(inside[..., None], blended, col)
    return R.to_rgba8(out)
