// taa_upscale.h -- temporal 2x upscaling: the reference's TAA pass (vulkan/processing/process_taa.comp) with render_upscale_factor = 2,
// run once per DISPLAY pixel of a 2W x 2H image over a frame rendered at W x H (rptr_hip_taa_upscale, host_access.inl). Included by
// rptr_hip.hip only (after realtime_resolve.h, whose rp_taa_pass<F> is the pass for both factors: rp_k_taa is F = 1, rp_k_taa_upscale
// F = 2). This text is the specification of the pass for a factor F.
//
// The reference's application renders at 1 / F of the display resolution, writes every rendered pixel into an F x F block of a
// display-size frame buffer (process_samples.comp:192-197) and lets the pass fill in the sub-pixel detail from the history. Here the
// replicated frame is never stored: display pixel (X, Y) reads the frame at render pixel (X / F, Y / F).
//   pre   the last finished frame's RGBA8 image, W x H (in a frame, F = 1: the frame before the pass)
//   hist  the previous output of the pass, FW x FH (texelFetch of RGBA8 = byte / 255; a texel outside the image reads zero)
//   mj    the frame's motion + jitter AOV, W x H (RGBA16F)
// The two deviations realtime_resolve.h states hold for every F: neighbours are read from the frame before the pass (`pre`), not in
// place, and the 3x3 motion loop reads the centre nine times as written, so the motion is the centre's.
//
// Per display pixel, in fp32, every operation rounded once (-ffp-contract=off, IEEE division and square root), in this order:
//   col       = pre[Y / F][X / F] / 255                                  (per channel; the same holds for the nine box pixels below)
//   motion    = mj[Y / F][X / F].xy                                      (process_taa.comp:61: fb_pixel / render_upscale_factor)
//   sp        = (float(X) + 0.5) / float(FW), (float(Y) + 0.5) / float(FH)
//   rp        = sp + 0.5 * motion
//   history is used when rp.x >= 0 && rp.y >= 0 && rp.x <= 1 && rp.y <= 1 (NaN motion of sky pixels fails it: the pixel keeps col)
//   pt        = rp * float(FW | FH) - 0.5,   cp = ceil(pt)
//   tap o in [-5, 5) per axis: np = float(F * o) + cp, texel ivec2(np), factor = lanczosWeight((np - pt) / float(F), 5)   (:43-44;
//        at F = 1 the division changes no bit)
//   lanczosWeight(x, r) = x == 0 ? 1 : r * sinf(x * pi) * sinf((x / r) * pi) / (pi * pi * x * x)   (rp_lanczos_weight, left to right)
//   the 10 + 10 factors are evaluated once; weight(ox, oy) = factor_x[ox] * factor_y[oy], the product the reference's 100 taps form
//   acc += weight * texel, total += weight, oy outer and ox inner, both ascending; hc = acc / total
//   box: render pixels (X / F + ox, Y / F + oy), ox, oy in {-1, 0, 1}, oy outer (fb_pixel + F * o of the replicated image, :91),
//        zero outside the image: trim += v, max2 += v * v; trim / 9, sqrtf(max2 / 9)
//   sd = 9 / 8 * (max2 - trim); lo = fmaxf(0, trim - sd); hi = fmaxf(trim + 3 * sd, col + sd)
//   col = fminf(fmaxf(hc + (col - hc) * 0.15, lo), hi)                   (:98-104)
//   out = rp_rgba8(col)
// tests/taa_upscale_ref.py restates this in numpy for any F, tests/realtime_resolve_ref.py independently for F = 1; they and the
// kernels differ where sinf does (tests/test_gpu_taa_upscale.py, tests/test_gpu_realtime_resolve.py: 1 LSB of RGBA8).
#pragma once
#include "realtime_resolve.h"

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
    rp_taa_pass<2>(W, H, pre, hist, mj, out, nullptr);
}
