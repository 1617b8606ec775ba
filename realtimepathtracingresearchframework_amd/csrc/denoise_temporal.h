// denoise_temporal.h -- the temporal part of SVGF (Schied et al., HPG 2017) in front of denoise.h's a-trous passes
// (rptr_hip_denoise_temporal, include/rptr_hip.h): demodulated colour, the two luminance moments and a history length are carried from
// call to call along the frame's motion + jitter AOV, and the passes get the variance of the blended signal instead of one frame's 3x3
// estimate. One kernel, rp_k_denoise_temporal, stands where rp_k_denoise_prepare stands in the launch sequence; rp_k_denoise_pass and
// rp_k_denoise_finish follow unchanged. Included by rptr_hip.hip only (after denoise.h).
//
// Arithmetic. denoise.h's rules: fp32 under the build's -ffp-contract=off, IEEE division, products and sums in the order written,
// dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, min / max are fminf / fmaxf. Every operation is correctly rounded, so the numpy restatement
// (tests/denoise_temporal_ref.py, written from THIS text; it imports tests/denoise_ref.py for what is shared) reproduces the stored
// images bit for bit.
//
// Per pixel p = (px, py): c, a, A, N, z, surface(p), d, e, lum(e), the 3x3 variance v_s and the depth gradient gz are exactly denoise.h's
// "Prepare". m = the motion + jitter AOV's .xy widened from half (as rp_k_reproject reads it: the step from the PREVIOUS FRAME's view to
// this one, in uv units times two). The history is what the previous call stored: He = (e'.rgb, n'), Hm = (m1', m2'), Hndz = (N, z) of
// that call's frame, all zero where its pixel was not surface.
// 1. Reprojection.  fw = float(W), fh = float(H);  u = (float(px) + 0.5f) / fw + 0.5f * m.x,  v = (float(py) + 0.5f) / fh + 0.5f * m.y;
//    x = u * fw - 0.5f, y = v * fh - 0.5f;  x0 = floorf(x), y0 = floorf(y), fx = x - x0, fy = y - y0. If x or y is not finite no tap is
//    valid. Taps q_k = (x0 + j, y0 + i), (j, i) = (0,0), (1,0), (0,1), (1,1), with the bilinear weights
//    b = (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.
// 2. A tap is valid when it lies inside the image (0 <= q.x < fw, 0 <= q.y < fh, tested in float before any conversion to int),
//    Hndz(q).w > 0, dot(N_p, Hndz(q).xyz) >= normal_threshold and fabsf(Hndz(q).w - z_p) <= depth_tolerance * z_p + gz_p.
// 3. sb = the sum of b_k over the valid taps, in tap order. History exists for p when the call has history, p is surface and
//    sb > 1e-3f.
// 4. With history: he, hn, hm1, hm2 = (sum of b_k * value_k over the valid taps, in tap order) / sb of He.rgb, He.w, Hm.x, Hm.y;
//    n' = fminf(hn + 1.0f, 255.0f);  ac = fmaxf(1.0f / n', alpha_color), am = fmaxf(1.0f / n', alpha_moments);
//    e' = (1.0f - ac) * he + ac * e per channel;  m1' = (1.0f - am) * hm1 + am * lum(e);  m2' = (1.0f - am) * hm2 + am * (lum(e) * lum(e)).
// 5. Without history (surface pixels): e' = e, m1' = lum(e), m2' = lum(e) * lum(e), n' = 1.0f, ac = 1.0f.
// 6. v_t = fmaxf(m2' - m1' * m1', 0.0f);  v = ((n' >= 4.0f) ? v_t : v_s) * ac -- the variance of the blended signal, not of one sample
//    (a blend that keeps the fraction ac of the new frame's noise; the unscaled variance made the passes blur as if nothing had been
//    accumulated).
// 7. Stored: ev[0] = (e', v); ndz and gz as prepare stores them; the new history He = (e', n'), Hm = (m1', m2'), Hndz = ndz. A pixel that
//    is not surface stores ev = (c.rgb, 0) as prepare does and all-zero history, so it is never a valid tap.
// 8. `iterations` launches of rp_k_denoise_pass and rp_k_denoise_finish follow.
// A call without history stores exactly prepare's (e, v_s), v_s * 1.0f being exact: its images equal rptr_hip_denoise's bit for bit.
// The history ping-pongs between two sets of images: a call reads one and writes the other, no thread reads what another stores.
//
// Layout. Prepare's: one block = 256 threads = 16 x 16 adjacent pixels, lum and (N, z) of the tile and a 1-pixel apron staged in LDS
// (18 x 18 x 20 bytes = 6.3 KB) for v_s and gz, by the two functions both kernels call (denoise.h rp_dn_stage, rp_dn_spatial). The four
// history taps are gathered from global memory where the motion points: Hndz (16 bytes) of every tap in the image first, He (16 bytes)
// and Hm (8 bytes) of the valid ones after the tests. Neighbouring lanes' taps are neighbours for a smooth motion, so a wave's 16-byte
// loads cover whole 128-byte lines and the four taps of a pixel share lines with its neighbours' -- staging a window as rp_k_taa does
// would save nothing but L1 hits and would need the tile's motion to be nearly uniform. Per pixel: 40 bytes in (accumulation, three
// AOVs), 40 unique bytes of history for a smooth motion, 76 bytes out: ~160 bytes, estimated; profiles/denoise_temporal_notes.md has
// what was measured, and the kernel's registers and LDS (no scratch).
#pragma once
#include "denoise.h"

struct RpDenoiseTemporalArgs {
    const uint2 *mj;       // the source frame's motion + jitter AOV (RGBA16F)
    const float4 *he_in;   // the history the previous call left: (e', n')
    const float2 *hm_in;   // (m1', m2')
    const float4 *hndz_in; // (N, z) of its frame; all zero where the pixel was not surface
    float4 *he_out;        // the history this call leaves
    float2 *hm_out;
    float4 *hndz_out;
    float alpha_color, alpha_moments, normal_threshold, depth_tolerance;
    int have_history;
};

// steps 1 to 7 of the header
__global__ __launch_bounds__(256) void rp_k_denoise_temporal(RpDenoiseArgs a, RpDenoiseTemporalArgs h, float4 *ev) {
    __shared__ float s_lum[RP_DN_SPAN * RP_DN_SPAN];
    __shared__ float4 s_nd[RP_DN_SPAN * RP_DN_SPAN];
    rp_dn_stage(a, s_lum, s_nd);
    const int W = a.width, H = a.height;
    const int t = int(threadIdx.x);
    const int lx = t & (RP_DN_TILE - 1), ly = t / RP_DN_TILE;
    const int px = int(blockIdx.x) * RP_DN_TILE + lx, py = int(blockIdx.y) * RP_DN_TILE + ly;
    if (px >= W || py >= H) return;
    const size_t i = size_t(py) * size_t(W) + size_t(px);
    const int c = (ly + 1) * RP_DN_SPAN + (lx + 1);
    const float4 ndp = s_nd[c];
    const bool surface = ndp.w > 0.0f;
    float4 e = rp_dn_signal(a, i, surface);
    float gz = 0.0f;
    float4 he = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 hm = make_float2(0.f, 0.f);
    if (surface) {
        float v_s;
        rp_dn_spatial(s_lum, s_nd, c, ndp, v_s, gz);
        const float l = s_lum[c];
        float n1 = 1.0f, ac = 1.0f, m1 = l, m2 = l * l;
        if (h.have_history) {
            const float fw = float(W), fh = float(H);
            const float2 m = rp_half2_lo(h.mj[i].x);
            const float u = (float(px) + 0.5f) / fw + 0.5f * m.x, v = (float(py) + 0.5f) / fh + 0.5f * m.y;
            const float x = u * fw - 0.5f, y = v * fh - 0.5f;
            if (fabsf(x) < INFINITY && fabsf(y) < INFINITY) { // (false for a NaN too)
                const float x0 = floorf(x), y0 = floorf(y);
                const float fx = x - x0, fy = y - y0;
                const float b[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
                const float z_lim = h.depth_tolerance * ndp.w + gz;
                size_t q[4];
                bool ok[4];
                float4 hq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float qx = x0 + float(k & 1), qy = y0 + float(k >> 1);
                    ok[k] = qx >= 0.0f && qy >= 0.0f && qx < fw && qy < fh;
                    q[k] = ok[k] ? size_t(int(qy)) * size_t(W) + size_t(int(qx)) : 0;
                    hq[k] = ok[k] ? h.hndz_in[q[k]] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                float sb = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sn = 0.0f, sm1h = 0.0f, sm2h = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!(ok[k] && hq[k].w > 0.0f && ((ndp.x * hq[k].x + ndp.y * hq[k].y) + ndp.z * hq[k].z) >= h.normal_threshold &&
                          fabsf(hq[k].w - ndp.w) <= z_lim))
                        continue;
                    const float4 eq = h.he_in[q[k]];
                    const float2 mq = h.hm_in[q[k]];
                    sb += b[k];
                    sx += b[k] * eq.x;
                    sy += b[k] * eq.y;
                    sz += b[k] * eq.z;
                    sn += b[k] * eq.w;
                    sm1h += b[k] * mq.x;
                    sm2h += b[k] * mq.y;
                }
                if (sb > 1e-3f) {
                    n1 = fminf(sn / sb + 1.0f, 255.0f);
                    ac = fmaxf(1.0f / n1, h.alpha_color);
                    const float am = fmaxf(1.0f / n1, h.alpha_moments);
                    e.x = (1.0f - ac) * (sx / sb) + ac * e.x;
                    e.y = (1.0f - ac) * (sy / sb) + ac * e.y;
                    e.z = (1.0f - ac) * (sz / sb) + ac * e.z;
                    m1 = (1.0f - am) * (sm1h / sb) + am * l;
                    m2 = (1.0f - am) * (sm2h / sb) + am * (l * l);
                }
            }
        }
        const float v_t = fmaxf(m2 - m1 * m1, 0.0f);
        e.w = ((n1 >= 4.0f) ? v_t : v_s) * ac;
        he = make_float4(e.x, e.y, e.z, n1);
        hm = make_float2(m1, m2);
    }
    ev[i] = e;
    a.gz[i] = gz;
    a.ndz[i] = ndp;
    h.he_out[i] = he;
    h.hm_out[i] = hm;
    h.hndz_out[i] = ndp;
}
