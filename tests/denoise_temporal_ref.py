"""numpy restatement of the temporal denoiser, written from the header of csrc/denoise_temporal.h (not from its kernel): prepare's
quantities from tests/denoise_ref.py, then reprojection, tap validity, the history gate, the blends, the variance and the stored
history; the a-trous passes, finish and the RGBA8 image are denoise_ref's. float32 throughout in the header's operation order.
Images are (H, W, 4) arrays, row 0 at the top.
"""
import numpy as np

import denoise_ref as D

F = np.float32
DEFAULTS = dict(D.DEFAULTS, alpha_color=0.2, alpha_moments=0.2, normal_threshold=0.9, depth_tolerance=0.1, reset_history=0)


def _gather(img, qx, qy, ok):
    """img at integer (qx, qy) where ok, zeros elsewhere"""
    out = img[np.where(ok, qy, 0), np.where(ok, qx, 0)]
    return np.where(ok.reshape(ok.shape + (1,) * (out.ndim - ok.ndim)), out, F(0)).astype(F)


class TemporalDenoiser:
    """holds what one call leaves for the next: He = (e', n'), Hm = (m1', m2'), Hndz = (N, z) of the call's frame, and the
    demodulate_albedo they were written with. A new object, like rptr_hip_initialize, has no history."""

    def __init__(self):
        self.he = self.hm = self.hndz = None
        self.demodulate = None
        self.had_history = None   # (H, W) bool: where the last step found history (step 3 of the header)

    def history(self):
        """(H, W, 4): what rptr_hip_readback_denoise_history_f32 returns, or None before any step"""
        return None if self.he is None else self.he.copy()

    def blend(self, accum, albedo, nd, mj, demodulate_albedo=1, alpha_color=0.2, alpha_moments=0.2, normal_threshold=0.9, depth_tolerance=0.1,
              reset_history=0):
        """steps 1 to 7: -> (ev, ndz, gz, surf), and the new history in self"""
        accum = D._f(accum)
        H, W = accum.shape[:2]
        ev, ndz, gz, surf = D.prepare(accum, albedo, nd, demodulate_albedo)
        e, v_s = ev[..., :3], ev[..., 3]
        lum = D._lum(e)
        have = self.he is not None and not reset_history and self.demodulate == int(demodulate_albedo)
        exists = np.zeros((H, W), bool)
        n1 = np.ones((H, W), F)
        ac = np.ones((H, W), F)
        e1, m1, m2 = e.copy(), lum.copy(), (lum * lum).astype(F)
        if have:
            m = D._f(np.asarray(mj)[..., :2])
            ys, xs = np.mgrid[0:H, 0:W]
            fw, fh = F(W), F(H)
            with np.errstate(all="ignore"):
                u = (xs.astype(F) + F(0.5)) / fw + F(0.5) * m[..., 0]
                v = (ys.astype(F) + F(0.5)) / fh + F(0.5) * m[..., 1]
                x, y = u * fw - F(0.5), v * fh - F(0.5)
                finite = np.isfinite(x) & np.isfinite(y)
                x0, y0 = np.floor(x), np.floor(y)
                fx, fy = x - x0, y - y0
                b = [(F(1) - fx) * (F(1) - fy), fx * (F(1) - fy), (F(1) - fx) * fy, fx * fy]
                z_lim = F(depth_tolerance) * ndz[..., 3] + gz
                sb = np.zeros((H, W), F)
                se = np.zeros((H, W, 3), F)
                sn, sm1, sm2 = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
                for k, (j, i) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                    qxf, qyf = x0 + F(j), y0 + F(i)
                    inside = finite & (qxf >= 0) & (qyf >= 0) & (qxf < fw) & (qyf < fh)
                    qx = np.where(inside, qxf, 0).astype(np.int64)
                    qy = np.where(inside, qyf, 0).astype(np.int64)
                    hq = _gather(self.hndz, qx, qy, inside)
                    dot = (ndz[..., 0] * hq[..., 0] + ndz[..., 1] * hq[..., 1]) + ndz[..., 2] * hq[..., 2]
                    ok = inside & (hq[..., 3] > 0) & (dot >= F(normal_threshold)) & (np.abs(hq[..., 3] - ndz[..., 3]) <= z_lim)
                    heq = _gather(self.he, qx, qy, ok)
                    hmq = _gather(self.hm, qx, qy, ok)
                    bk = b[k].astype(F)
                    sb = np.where(ok, sb + bk, sb)
                    se = np.where(ok[..., None], se + bk[..., None] * heq[..., :3], se)
                    sn = np.where(ok, sn + bk * heq[..., 3], sn)
                    sm1 = np.where(ok, sm1 + bk * hmq[..., 0], sm1)
                    sm2 = np.where(ok, sm2 + bk * hmq[..., 1], sm2)
                exists = surf & (sb > F(1e-3))
                nh = np.fmin(sn / sb + F(1), F(255))
                a_c = np.fmax(F(1) / nh, F(alpha_color))
                a_m = np.fmax(F(1) / nh, F(alpha_moments))
                eh = (F(1) - a_c)[..., None] * (se / sb[..., None]) + a_c[..., None] * e
                m1h = (F(1) - a_m) * (sm1 / sb) + a_m * lum
                m2h = (F(1) - a_m) * (sm2 / sb) + a_m * (lum * lum)
            n1 = np.where(exists, nh, n1).astype(F)
            ac = np.where(exists, a_c, ac).astype(F)
            e1 = np.where(exists[..., None], eh, e1).astype(F)
            m1 = np.where(exists, m1h, m1).astype(F)
            m2 = np.where(exists, m2h, m2).astype(F)
        with np.errstate(all="ignore"):
            v_t = np.fmax(m2 - m1 * m1, F(0))
            var = (np.where(n1 >= F(4), v_t, v_s) * ac).astype(F)
        s3 = surf[..., None]
        out_ev = np.concatenate([np.where(s3, e1, e), np.where(surf, var, F(0))[..., None]], -1).astype(F)
        self.he = np.concatenate([np.where(s3, e1, F(0)), np.where(surf, n1, F(0))[..., None]], -1).astype(F)
        self.hm = np.where(s3, np.stack([m1, m2], -1), F(0)).astype(F)
        self.hndz = ndz.copy()
        self.demodulate = int(demodulate_albedo)
        self.had_history = exists
        return out_ev, ndz, gz, surf

    def step(self, accum, albedo, nd, mj, fb=None, iterations=5, sigma_luminance=4.0, sigma_depth=1.0, normal_power_log2=7, demodulate_albedo=1,
             alpha_color=0.2, alpha_moments=0.2, normal_threshold=0.9, depth_tolerance=0.1, reset_history=0, output_channel=0, exposure=0.0,
             tone_mapping_mode=-1):
        """one rptr_hip_denoise_temporal call -> (RGBA32F image, RGBA8 image or None without fb)"""
        accum = D._f(accum)
        ev, ndz, gz, surf = self.blend(accum, albedo, nd, mj, demodulate_albedo, alpha_color, alpha_moments, normal_threshold, depth_tolerance,
                                       reset_history)
        for i in range(iterations):
            ev = D.atrous_pass(ev, ndz, gz, i, sigma_luminance, sigma_depth, normal_power_log2)
        # finish, as denoise_ref.denoise
        rgb = ev[..., :3] * D.divisor(albedo) if demodulate_albedo else ev[..., :3]
        out = accum.copy()
        out[..., :3] = np.where(surf[..., None], rgb, accum[..., :3])
        if fb is None:
            return out, None
        u8 = np.array(fb, np.uint8, copy=True)
        if output_channel == 0:
            o = out.copy()
            o[..., 3] = np.fmin(out[..., 3], F(1))
            shown = D.to_rgba8(D.display(o, exposure, tone_mapping_mode))
            u8 = np.where((o[..., 3] >= 0)[..., None], shown, u8)
        return out, u8
