// taa_upscale.h -- temporal 2x upscaling: the reference's TAA pass (vulkan/processing/process_taa.comp) with render_upscale_factor = 2,
// run once per DISPLAY pixel of a 2W x 2H image over a frame rendered at W x H (rptr_hip_taa_upscale, host_access.inl). Included by
// rptr_hip.hip only (after realtime_resolve.h, whose rp_lanczos_weight, rp_half2_lo, rp_trunc_i and rp_rgba8 it uses).
//
// The reference's application renders at half the display resolution, writes every rendered pixel into a 2x2 block of a display-size
// frame buffer (process_samples.comp:192-197) and lets the pass fill in the sub-pixel detail from the history. Here the replicated frame
// is never stored: display pixel (X, Y) reads the frame at render pixel (X / 2, Y / 2).
//   pre   the last finished frame's RGBA8 image, W x H
//   hist  the previous call's output, 2W x 2H (texelFetch of RGBA8 = byte / 255; a texel outside the image reads zero)
//   mj    the frame's motion + jitter AOV, W x H (RGBA16F)
// The two deviations of rp_k_taa hold here too: neighbours are read from the frame before the pass (`pre`), not in place, and the 3x3
// motion loop reads the centre nine times as written, so the motion is the centre's.
//
// Per display pixel, in fp32, every operation rounded once (-ffp-contract=off, IEEE division and square root), in this order:
//   col       = pre[Y / 2][X / 2] / 255                                  (per channel; the same holds for the nine box pixels below)
//   motion    = mj[Y / 2][X / 2].xy                                      (process_taa.comp:61: fb_pixel / render_upscale_factor)
//   sp        = (float(X) + 0.5) / float(2W), (float(Y) + 0.5) / float(2H)
//   rp        = sp + 0.5 * motion
//   history is used when rp.x >= 0 && rp.y >= 0 && rp.x <= 1 && rp.y <= 1 (NaN motion of sky pixels fails it: the pixel keeps col)
//   pt        = rp * float(2W | 2H) - 0.5,   cp = ceil(pt)
//   tap o in [-5, 5) per axis: np = float(2 * o) + cp, texel ivec2(np), factor = lanczosWeight((np - pt) / 2, 5)   (:43-44)
//   lanczosWeight(x, r) = x == 0 ? 1 : r * sinf(x * pi) * sinf((x / r) * pi) / (pi * pi * x * x)   (rp_lanczos_weight, left to right)
//   the 10 + 10 factors are evaluated once; weight(ox, oy) = factor_x[ox] * factor_y[oy], the product the reference's 100 taps form
//   acc += weight * texel, total += weight, oy outer and ox inner, both ascending; hc = acc / total
//   box: render pixels (X / 2 + ox, Y / 2 + oy), ox, oy in {-1, 0, 1}, oy outer (fb_pixel + 2 * o of the replicated image, :91),
//        zero outside the image: trim += v, max2 += v * v; trim / 9, sqrtf(max2 / 9)
//   sd = 9 / 8 * (max2 - trim); lo = fmaxf(0, trim - sd); hi = fmaxf(trim + 3 * sd, col + sd)
//   col = fminf(fmaxf(hc + (col - hc) * 0.15, lo), hi)                   (:98-104)
//   out = rp_rgba8(col)
// tests/taa_upscale_ref.py restates this in numpy; the two differ where sinf does (tests/test_gpu_taa_upscale.py: 1 LSB of RGBA8).
//
// One block = one 8 x 8 display tile = one wave. Staged in LDS: the 6 x 6 render pixels around the tile's 4 x 4 as float4, the
// byte / 255 table, and a 32 x 32 window of history texels -- the tile's ten stride-2 taps per axis span 8 + 18 texels, plus 3 texels of
// motion spread each side -- placed by the motion of the tile's first pixel. The window's rows are 40 words apart: a half-wave's lanes
// (8 columns x 4 rows of the tile) read texels whose addresses differ by lx + 40 * ly, 32 different banks. Taps outside the window
// (motions that differ by more than 3 display pixels inside a tile, NaN motion of the first pixel) read global memory: the same values.
#pragma once
#include "realtime_resolve.h"

#define RP_TU_TILE 8     // display pixels per block and axis
#define RP_TU_PRE 6      // render pixels staged per axis: the tile's 4 and one each side
#define RP_TU_WIN 32     // history texels staged per axis
#define RP_TU_PITCH 40   // words between the window's rows in LDS (see above)
#define RP_TU_LEAD 13    // the window starts this many texels before the first pixel's ceil(pt): its first tap (-10) and 3 of spread

// the output of a call without history: the 2x2 replication of the frame (what the reference's history holds after its first frame,
// process_taa.cpp:95 skips frame_id <= 1)
__global__ __launch_bounds__(256) void rp_k_upscale_replicate(int W, int H, const uchar4 *pre, uchar4 *out) {
    const size_t DW = size_t(W) * 2, n = DW * (size_t(H) * 2);
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += size_t(gridDim.x) * 256) {
        const size_t y = i / DW, x = i - y * DW;
        out[i] = pre[(y >> 1) * size_t(W) + (x >> 1)];
    }
}

__global__ __launch_bounds__(64) void rp_k_taa_upscale(int W, int H, const uchar4 *pre, const uchar4 *hist, const uint2 *mj, uchar4 *out) {
    __shared__ float4 s_pre[RP_TU_PRE * RP_TU_PRE];
    __shared__ uchar4 s_hist[RP_TU_WIN * RP_TU_PITCH];
    __shared__ float s_unorm[256]; // byte / 255 (texelFetch of RGBA8), the same IEEE quotients without a division per tap
    const int DW = 2 * W, DH = 2 * H;
    const int tx0 = int(blockIdx.x) * RP_TU_TILE, ty0 = int(blockIdx.y) * RP_TU_TILE; // (even: the tile covers whole 2x2 blocks)
    const int t = int(threadIdx.x);
    const float fw = float(DW), fh = float(DH);
    for (int k = t; k < 256; k += 64) s_unorm[k] = float(k) / 255.0f;
    if (t < RP_TU_PRE * RP_TU_PRE) {
        const int sy = t / RP_TU_PRE, sx = t - sy * RP_TU_PRE;
        const int gx = tx0 / 2 + sx - 1, gy = ty0 / 2 + sy - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f); // imageLoad outside the image: zero
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            const uchar4 b = pre[size_t(gy) * size_t(W) + size_t(gx)];
            v = make_float4(float(b.x) / 255.0f, float(b.y) / 255.0f, float(b.z) / 255.0f, float(b.w) / 255.0f);
        }
        s_pre[t] = v;
    }
    // the window: where the first pixel's taps begin (every thread computes the same two integers)
    int bx, by;
    {
        const float2 m0 = rp_half2_lo(mj[size_t(ty0 / 2) * size_t(W) + size_t(tx0 / 2)].x);
        const float bpx = (((float(tx0) + 0.5f) / fw + 0.5f * m0.x) * fw) - 0.5f;
        const float bpy = (((float(ty0) + 0.5f) / fh + 0.5f * m0.y) * fh) - 0.5f;
        bx = rp_trunc_i(ceilf(bpx)) - RP_TU_LEAD;
        by = rp_trunc_i(ceilf(bpy)) - RP_TU_LEAD;
        for (int k = t; k < RP_TU_WIN * RP_TU_WIN; k += 64) {
            const int wy = k / RP_TU_WIN, wx = k % RP_TU_WIN;
            const int qy = by + wy, qx = bx + wx;
            s_hist[wy * RP_TU_PITCH + wx] = (qx >= 0 && qy >= 0 && qx < DW && qy < DH) ? hist[size_t(qy) * size_t(DW) + size_t(qx)] : make_uchar4(0, 0, 0, 0);
        }
    }
    __syncthreads();
    const int lx = t & 7, ly = t >> 3;
    const int px = tx0 + lx, py = ty0 + ly;
    if (px >= DW || py >= DH) return;
    const size_t i = size_t(py) * size_t(DW) + size_t(px);
    const size_t ri = size_t(py >> 1) * size_t(W) + size_t(px >> 1); // the render pixel under this display pixel
    const int c = ((ly >> 1) + 1) * RP_TU_PRE + ((lx >> 1) + 1);
    float4 col = s_pre[c];
    float2 motion = rp_half2_lo(mj[ri].x);
    float motion_len = motion.x * motion.x + motion.y * motion.y;
    for (int k = 0; k < 9; ++k) { // process_taa.comp:63-71 as written: the centre, nine times
        const float2 m = rp_half2_lo(mj[ri].x);
        const float ml = m.x * m.x + m.y * m.y;
        if (ml > motion_len) {
            motion = m;
            motion_len = ml;
        }
    }
    const float spx = (float(px) + 0.5f) / fw, spy = (float(py) + 0.5f) / fh;
    const float rpx = spx + 0.5f * motion.x, rpy = spy + 0.5f * motion.y;
    float4 hc = make_float4(0.f, 0.f, 0.f, 0.f);
    float new_w = 1.0f;
    if (rpx >= 0.0f && rpy >= 0.0f && rpx <= 1.0f && rpy <= 1.0f) {
        const float ptx = rpx * fw - 0.5f, pty = rpy * fh - 0.5f;
        const float cpx = ceilf(ptx), cpy = ceilf(pty);
        float wx[10], wy[10];
        for (int o = 0; o < 10; ++o) {
            wx[o] = rp_lanczos_weight(((float(2 * (o - 5)) + cpx) - ptx) / 2.0f, 5.0f);
            wy[o] = rp_lanczos_weight(((float(2 * (o - 5)) + cpy) - pty) / 2.0f, 5.0f);
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float total = 0.0f;
        for (int oy = -5; oy < 5; ++oy)
            for (int ox = -5; ox < 5; ++ox) {
                const float npx = float(2 * ox) + cpx, npy = float(2 * oy) + cpy;
                const float w = wx[ox + 5] * wy[oy + 5];
                const int qx = rp_trunc_i(npx), qy = rp_trunc_i(npy);
                uchar4 b = make_uchar4(0, 0, 0, 0);
                const unsigned wxi = unsigned(qx - bx), wyi = unsigned(qy - by);
                if (wxi < unsigned(RP_TU_WIN) && wyi < unsigned(RP_TU_WIN))
                    b = s_hist[wyi * RP_TU_PITCH + wxi];
                else if (qx >= 0 && qy >= 0 && qx < DW && qy < DH)
                    b = hist[size_t(qy) * size_t(DW) + size_t(qx)];
                acc.x += w * s_unorm[b.x];
                acc.y += w * s_unorm[b.y];
                acc.z += w * s_unorm[b.z];
                acc.w += w * s_unorm[b.w];
                total += w;
            }
        hc = make_float4(acc.x / total, acc.y / total, acc.z / total, acc.w / total);
        new_w = 0.15f;
    }
    if (new_w < 1.0f) { // the neighbourhood's trimmed box over the render pixels (:86-106)
        float4 trim = make_float4(0.f, 0.f, 0.f, 0.f), max2 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const float4 v = s_pre[c + oy * RP_TU_PRE + ox];
                trim.x += v.x;
                trim.y += v.y;
                trim.z += v.z;
                trim.w += v.w;
                max2.x += v.x * v.x;
                max2.y += v.y * v.y;
                max2.z += v.z * v.z;
                max2.w += v.w * v.w;
            }
        const float tr[4] = {trim.x / 9.0f, trim.y / 9.0f, trim.z / 9.0f, trim.w / 9.0f};
        const float m2[4] = {sqrtf(max2.x / 9.0f), sqrtf(max2.y / 9.0f), sqrtf(max2.z / 9.0f), sqrtf(max2.w / 9.0f)};
        float cc[4] = {col.x, col.y, col.z, col.w};
        const float hh[4] = {hc.x, hc.y, hc.z, hc.w};
        for (int k = 0; k < 4; ++k) {
            const float sd = 9.0f / 8.0f * (m2[k] - tr[k]);
            const float lo = fmaxf(0.0f, tr[k] - sd), hi = fmaxf(tr[k] + 3.0f * sd, cc[k] + sd);
            const float v = hh[k] + (cc[k] - hh[k]) * new_w;
            cc[k] = fminf(fmaxf(v, lo), hi);
        }
        col = make_float4(cc[0], cc[1], cc[2], cc[3]);
    }
    out[i] = rp_rgba8(col);
}
