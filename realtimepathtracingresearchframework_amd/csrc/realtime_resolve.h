// realtime_resolve.h -- the reference's ENABLE_REALTIME_RESOLVE passes: reprojection_mode == REPROJECTION_MODE_ACCUMULATE (2), the
// motion-reprojected accumulation of vulkan/process_samples.comp:106-112 + rendering/postprocess/reprojection.glsl:43-367, and the TAA pass
// on the RGBA8 frame (vulkan/processing/process_taa.comp, process_taa.cpp:90-127). Included by rptr_hip.hip only (after kernels_misc.h).
//
// Frame = one reference frame: one render call of `spp` samples (app.cpp:352-354, batch_spp = spp). rp_k_resolve first leaves the MEAN of
// this call's samples in a scratch image (as in DISCARD_HISTORY); rp_k_reproject then folds it into the history:
//   accum_color        = that mean (coverage mean in .a)
//   sample_base_index  = frame_id before the call (0: no history is folded in, the mean is stored: process_samples.comp:117-131)
//   sample_batch_size  = spp, min_sample_weight = 1 / spp_accumulation_window
// History = what the previous frame left: its RGBA32F accumulation image and its normal + depth AOV (render_vulkan.cpp:1943-1949,
// 2049-2059, 2438-2440: the !active_accum_buffer ping-pong). Both are ping-pong images here too; the kernel reads the history and writes
// the other image, so no thread reads what another one stores.
//
// reprojection.glsl is compiled with the defines the reference ships on: BOUNDARY_SEARCH, BILATERAL, BILATERAL_PROJECTION,
// FIT_GEOMETRY_DISTRIBUTION (CONFLICT_RESOLUTION, ACCUM_GBUFFER, BACKGROUND, BILATERAL_TEST, TEST_BILATERAL_ACCUM_GUESS off). With those,
// several of its values are computed and never read; they are left out here, which changes no stored bit:
//   - the boundary search (:55-82) rewrites all nine motions, but only the centre's is read afterwards (the others feed
//     CONFLICT_RESOLUTION); the centre's edge motion only sees the 3x3 ring (|o - n| <= 1), so the 5x5 loop reads 3x3 motions here;
//   - motion_rate (:85-87) feeds BACKGROUND / BILATERAL_TEST only;
//   - the 3x3 statistics of the current colour (accum_mean / accum_sigma, :206-221), bilateral_history / _sq / sigma_ldr, max_weight and
//     min_depth / max_depth feed BILATERAL_TEST or BACKGROUND only.
// Sampling rules (Vulkan leaves some undefined; these are the ones restated, tests/realtime_resolve_ref.py follows them):
//   - textureLod(history, uv): bilinear in fp32 over texel centres, x = uv.x * W - 0.5, x0 = floor(x), fx = x - x0 (same for y), texel
//     indices clamped to the edge (screen_sampler, render_vulkan.cpp:417-427), sum in the order
//     (1-fx)(1-fy) c00 + fx(1-fy) c10 + (1-fx)fy c01 + fx fy c11, left to right;
//   - texelFetch / imageLoad outside the image read zero (Vulkan robust access);
//   - min / max / clamp are fminf / fmaxf (a NaN operand gives the other one). In BILATERAL_PROJECTION, t = dot / dot(line, line) is
//     0 / 0 when the history colour equals the current one: max(NaN, 0) = 0 and the new-sample weight becomes 1, as stated;
//   - smoothstep(e0, e1, x) = t * t * (3 - 2 t), t = clamp((x - e0) / (e1 - e0), 0, 1); ivec2(v) truncates toward zero (of values
//     clamped to +-2^30 first); dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
//   - The reference's anchor point (:75) is ivec2(uv) -- a truncation of uv coordinates, not pixels: it is restated as written.
//   - exp (the filter weight, :258) is evaluated in double and rounded once to float: the correctly rounded value, which GLSL's exp
//     allows and which the numpy restatement computes the same way. With -ffp-contract=off and IEEE division / square root every other
//     operation is correctly rounded too, so the stored image equals the restatement bit for bit.
//   - A pixel whose alpha is negative (the reference's debug renderer; no shipped material) keeps the frame buffer's previous value;
//     with TAA that value then goes through the pass like any other.
// Stored: the accumulation image gets (history.rgb, 1 - new_sample_weight) (what rptr_hip_readback_f32 returns); the frame shows
// history.rgb with the frame's own coverage alpha (:344-366, test_result.w < 0) through rp_display_color.
#pragma once
#include "kernels_misc.h"

#define RP_RT_TILE 8                   // 8 x 8 pixels per block: one wave64
#define RP_RT_APRON 1                  // the 3x3 rings of motion and normal + depth around a tile
#define RP_RT_SPAN (RP_RT_TILE + 2 * RP_RT_APRON)

struct RpReprojectArgs {
    const float4 *cur;      // this frame's mean (rp_k_resolve's output in mode 2)
    const uint2 *nd;        // this frame's normal + depth AOV (RGBA16F)
    const uint2 *mj;        // this frame's motion + jitter AOV (RGBA16F)
    const float4 *hist;     // the previous frame's accumulation image
    const uint2 *hist_nd;   // the previous frame's normal + depth
    float4 *accum;          // out: this frame's accumulation image
    uint2 *out_nd;          // out: copy of this frame's normal + depth (the next frame's history)
    uchar4 *fb;             // out: the RGBA8 frame (before TAA when TAA runs)
    const uchar4 *fb_keep;  // the frame buffer as the previous frame left it: what a pixel with alpha < 0 keeps (process_samples.comp:139-140)
    float4 *out_accum;      // frames in flight: the context's copies (else NULL; each is checked on its own)
    uchar4 *out_fb;
    float min_sample_weight;
    int sample_batch_size;
    int use_history;        // sample_base_index > 0 and the previous frame left a history
};

RP_DEV uchar4 rp_rgba8(float4 o) {
    return make_uchar4((unsigned char)(clamp1(o.x, 0.f, 1.f) * 255.0f + 0.5f), (unsigned char)(clamp1(o.y, 0.f, 1.f) * 255.0f + 0.5f),
                       (unsigned char)(clamp1(o.z, 0.f, 1.f) * 255.0f + 0.5f), (unsigned char)(clamp1(o.w, 0.f, 1.f) * 255.0f + 0.5f));
}
RP_DEV float rp_smoothstep(float e0, float e1, float x) {
    const float t = fminf(fmaxf((x - e0) / (e1 - e0), 0.0f), 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
RP_DEV int rp_trunc_i(float v) { return int(fminf(fmaxf(v, -1073741824.0f), 1073741824.0f)); } // ivec2(v), range-clamped
RP_DEV float2 rp_half2_lo(uint32_t h) {
    return make_float2((float)__builtin_bit_cast(_Float16, (uint16_t)(h & 0xFFFFu)), (float)__builtin_bit_cast(_Float16, (uint16_t)(h >> 16)));
}
RP_DEV float4 rp_bilinear(const float4 *img, float u, float v, int W, int H) { // textureLod with the screen sampler, clamp to edge
    const float x = u * float(W) - 0.5f, y = v * float(H) - 0.5f;
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = rp_trunc_i(x0f), y0 = rp_trunc_i(y0f);
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    const float4 c00 = img[size_t(ya) * W + xa], c10 = img[size_t(ya) * W + xb], c01 = img[size_t(yb) * W + xa], c11 = img[size_t(yb) * W + xb];
    const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
    return make_float4(((w00 * c00.x + w10 * c10.x) + w01 * c01.x) + w11 * c11.x, ((w00 * c00.y + w10 * c10.y) + w01 * c01.y) + w11 * c11.y,
                       ((w00 * c00.z + w10 * c10.z) + w01 * c01.z) + w11 * c11.z, ((w00 * c00.w + w10 * c10.w) + w01 * c01.w) + w11 * c11.w);
}

// One block = one 8 x 8 tile = one wave. The motion (.xy) and the normal + depth of the tile and a 1-pixel apron are staged in LDS (packed
// fp16 loads, zero outside the image); the history is read where the motion points, from global memory.
// Cost (configs[1] frame, 1920x1080, rocprofv3 kernel trace): 73 us per frame with history, 28 us on a reset frame. The reset frame moves
// ~60 bytes per pixel (mean, both AOVs in; accumulation, normal + depth copy, RGBA8 out): ~124 MB in 28 us, memory bound. With history
// each pixel adds the bilinear history (4 texels) and the 3x3 history colour + normal + depth at the reconstruction point -- mostly cache
// hits for a smooth pan, ~24 more bytes per pixel from memory -- and the arithmetic of nine bilateral weights (nine divisions each for
// the relative depths and smoothstep, nine exp in double). Estimated, not measured with counters: ~40 us of that is the memory floor,
// the rest is VALU (the IEEE divisions and the double exp); a counter pass (rocprofv3 --pmc) is what would settle it.
__global__ __launch_bounds__(64) void rp_k_reproject(RpFrame f, RpReprojectArgs a) {
    __shared__ float2 s_mot[RP_RT_SPAN * RP_RT_SPAN];
    __shared__ float4 s_nd[RP_RT_SPAN * RP_RT_SPAN];
    const int W = f.width, H = f.height;
    const int tx0 = int(blockIdx.x) * RP_RT_TILE, ty0 = int(blockIdx.y) * RP_RT_TILE;
    const int t = int(threadIdx.x);
    if (a.use_history)
        for (int k = t; k < RP_RT_SPAN * RP_RT_SPAN; k += 64) {
            const int sy = k / RP_RT_SPAN, sx = k - sy * RP_RT_SPAN;
            const int gx = tx0 + sx - RP_RT_APRON, gy = ty0 + sy - RP_RT_APRON;
            float2 m = make_float2(0.f, 0.f);
            float4 nd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
                const size_t g = size_t(gy) * size_t(W) + size_t(gx);
                m = rp_half2_lo(a.mj[g].x);
                nd = rp_half4_to_float4(a.nd[g]);
            }
            s_mot[k] = m;
            s_nd[k] = nd;
        }
    __syncthreads();
    const int lx = t & 7, ly = t >> 3;
    const int px = tx0 + lx, py = ty0 + ly;
    if (px >= W || py >= H) return;
    const size_t i = size_t(py) * size_t(W) + size_t(px);
    const float4 accum_color = a.cur[i];
    const uint2 nd_raw = a.nd[i];
    float4 hist = make_float4(0.f, 0.f, 0.f, 0.f);
    float new_w = 1.0f;
    if (a.use_history) {
        const float fw = float(W), fh = float(H);
        const int c = (ly + RP_RT_APRON) * RP_RT_SPAN + (lx + RP_RT_APRON);
        const float2 m0 = s_mot[c];
        // BOUNDARY_SEARCH (:50-82), the centre: the longest motion of the 3x3 ring (scan order, strictly longer wins)
        float2 em = m0;
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const float2 m = s_mot[c + oy * RP_RT_SPAN + ox];
                if (m.x * m.x + m.y * m.y > em.x * em.x + em.y * em.y) em = m;
            }
        const float spx = (float(px) + 0.5f) / fw, spy = (float(py) + 0.5f) / fh;
        float rpx = spx + 0.5f * m0.x, rpy = spy + 0.5f * m0.y;
        const float apx = float(rp_trunc_i(spx + 0.5f * em.x)), apy = float(rp_trunc_i(spy + 0.5f * em.y));
        rpx = fminf(fmaxf(rpx, floorf(apx) - 0.5f), floorf(apx) + 1.5f);
        rpy = fminf(fmaxf(rpy, floorf(apy) - 0.5f), floorf(apy) + 1.5f);
        const float mx = 2.0f * (rpx - spx), my = 2.0f * (rpy - spy);
        // :83-84, 97-154
        rpx = spx + 0.5f * mx;
        rpy = spy + 0.5f * my;
        if (rpx >= 0.0f && rpy >= 0.0f && rpx < 1.0f && rpy < 1.0f) {
            hist = rp_bilinear(a.hist, rpx, rpy, W, H);
            const float old = 1.0f - hist.w;
            if (old > 0.0f) new_w = old / (1.0f + old * float(a.sample_batch_size));
        }
        new_w = fmaxf(new_w, a.min_sample_weight);
        if (accum_color.w > 1.0f) new_w = 0.95f; // non-accumulation object types (:157-158)
        const float4 cnd = s_nd[c];
        if (new_w < 1.0f) { // BILATERAL (:162-339)
            const int rx = rp_trunc_i(rpx * fw), ry = rp_trunc_i(rpy * fh);
            // FIT_GEOMETRY_DISTRIBUTION (:166-191)
            float anx = 0.f, any = 0.f, anz = 0.f, avg_depth = 0.f, sq_depth = 0.f;
            for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                    const float4 n = s_nd[c + oy * RP_RT_SPAN + ox];
                    anx += n.x;
                    any += n.y;
                    anz += n.z;
                    const float rel = n.w / cnd.w;
                    avg_depth += rel;
                    sq_depth += rel * rel;
                }
            anx /= 9.0f;
            any /= 9.0f;
            anz /= 9.0f;
            avg_depth /= 9.0f;
            sq_depth /= 9.0f;
            const float normal_sigma = fmaxf(1.0f - sqrtf((anx * anx + any * any) + anz * anz), 0.0f);
            const float depth_sigma = sqrtf(fmaxf(sq_depth - avg_depth * avg_depth, 0.0f));
            const float depth_scale = fminf(10.0f, 1.0f / depth_sigma);
            float mix_w = 0.f;
            float4 mix = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                    const int qx = rx + ox, qy = ry + oy;
                    const bool in = qx >= 0 && qy >= 0 && qx < W && qy < H;
                    const size_t q = in ? size_t(qy) * size_t(W) + size_t(qx) : 0;
                    const float4 hc = in ? a.hist[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float nold = 1.0f - hc.w;
                    const float4 hn = in ? rp_half4_to_float4(a.hist_nd[q]) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float angle = (hn.x * cnd.x + hn.y * cnd.y) + hn.z * cnd.z;
                    const float rdd = fabsf(hn.w / cnd.w - 1.0f);
                    float w = rp_smoothstep(-0.66f, 1.0f, angle + normal_sigma) * fminf(fmaxf(0.0f, 1.0f - depth_scale * rdd), 1.0f);
                    const float dx = (float(qx) + 0.5f) - rpx * fw, dy = (float(qy) + 0.5f) - rpy * fh;
                    w *= float(exp(double(-3.0f * (dx * dx + dy * dy)))); // exp, correctly rounded to float (see the header)
                    if (nold > 0.0f) {
                        mix_w += w;
                        mix.x += w * hc.x;
                        mix.y += w * hc.y;
                        mix.z += w * hc.z;
                    }
                }
            if (mix_w > 0.0f) { // BILATERAL_PROJECTION (:316-319)
                mix.x /= mix_w;
                mix.y /= mix_w;
                mix.z /= mix_w;
                const float lnx = hist.x - accum_color.x, lny = hist.y - accum_color.y, lnz = hist.z - accum_color.z;
                const float tt = (((mix.x - accum_color.x) * lnx + (mix.y - accum_color.y) * lny) + (mix.z - accum_color.z) * lnz) /
                                 ((lnx * lnx + lny * lny) + lnz * lnz);
                new_w = fmaxf(new_w, 1.0f - fmaxf(tt, 0.0f)); // 0 / 0 -> fmaxf(NaN, 0) = 0 -> weight 1
            } else
                new_w = 1.0f;
            new_w = fmaxf(new_w, a.min_sample_weight);
        }
    } else
        new_w = 0.0f; // (no history: the mean itself, below)
    float4 res;
    if (a.use_history) { // :341-345
        res.x = hist.x + (accum_color.x - hist.x) * new_w;
        res.y = hist.y + (accum_color.y - hist.y) * new_w;
        res.z = hist.z + (accum_color.z - hist.z) * new_w;
        res.w = 1.0f - new_w;
    } else
        res = accum_color; // process_samples.comp:116-131 with sample_base_index == 0
    a.accum[i] = res;
    a.out_nd[i] = nd_raw;
    float4 o = make_float4(res.x, res.y, res.z, fminf(accum_color.w, 1.0f));
    if (!a.use_history) o.w = fminf(res.w, 1.0f);
    uchar4 shown = a.fb_keep[i];
    if (o.w >= 0.0f) shown = rp_rgba8(rp_display_color(f, o, int(i)));
    a.fb[i] = shown;
    if (a.out_accum) a.out_accum[i] = res;
    if (a.out_fb) a.out_fb[i] = shown;
}

// ------------------------------------------------------------------ TAA (vulkan/processing/process_taa.comp)
// Runs after the resolve on the RGBA8 frame, when option "taa" is 1 in mode 2 and frame_id (after the call) > 1 (process_taa.cpp:92).
// History: the previous frame's post-TAA RGBA8 image (render_targets[!active_render_target], the screen sampler; texelFetch of RGBA8 =
// byte / 255). taa_upscale.h states every operation of the pass for a render_upscale_factor F; rp_taa_pass<F> below is that text.
// Deviations from the reference, both stated:
//   - process_taa.comp:91 reads the 3x3 neighbours from the frame buffer it stores to in place -- a race between invocations. Here `pre`
//     (the frame before the pass) is read and `out` written, so every neighbour is the pre-TAA value.
//   - its 3x3 motion loop (:63-71) loads the CENTRE pixel nine times (fb_pixel / render_upscale_factor, no offset): kept as written, so
//     the motion is the centre's.
// render_upscale_factor is 1 in a frame (it renders and shows at one resolution; option "taa" with factor 2 is refused): rp_k_taa. The
// pass at twice the render resolution is a call of its own on a finished frame: rp_k_taa_upscale, taa_upscale.h.
// Cost of rp_k_taa (same frame): 122 us. 100 Lanczos taps per pixel, each an LDS read of the staged history texel plus four LDS reads of
// the byte / 255 table and four multiply-adds: ~500 LDS reads per pixel, estimated ~50 us of LDS issue alone, the rest VALU. Estimated,
// not measured with counters.
//
// Layout, for both factors. One block = one 8 x 8 tile of DISPLAY pixels (F W x F H of them over a W x H frame) = one wave. Staged in
// LDS: the render pixels under the tile and one each side as float4, the byte / 255 table, and a window of history texels placed by the
// motion of the tile's first pixel. The tile's ten stride-F taps per axis span 8 + 9 F texels; with 3 texels of motion spread each side
// that is 23 of 24 at factor 1 and 32 of 32 at factor 2. The window's rows are PITCH words apart: a half-wave's lanes (8 columns x 4 rows
// of the tile) read texels whose addresses differ by lx + PITCH * ly, and both 24 and 40 put the four rows into 32 different banks (32
// would put them into the same eight). Taps outside the window (motions that differ by more than 3 display pixels inside a tile, NaN
// motion of the first pixel) read global memory: the same values.
#define RP_TAA_TILE RP_RT_TILE // display pixels per block and axis (8; a frame launches rp_k_taa on rp_k_reproject's grid of tiles)
template <int F> struct RpTaaLayout {
    static constexpr int SHIFT = F == 1 ? 0 : 1;    // log2(F): display pixel p lies over render pixel p >> SHIFT
    static constexpr int PRE = RP_TAA_TILE / F + 2; // render pixels staged per axis: the tile's 8 / F and one each side
    static constexpr int WIN = F == 1 ? 24 : 32;    // history texels staged per axis
    static constexpr int PITCH = F == 1 ? 24 : 40;  // words between the window's rows in LDS (see above)
    static constexpr int LEAD = 5 * F + 3;          // the window starts this many texels before the first pixel's ceil(pt): its first tap (-5 F) and 3 of spread
};
RP_DEV float rp_lanczos_weight(float x, float r) { // :28-31
    const float pi = 3.14159265358979323846f;
    if (x == 0.0f) return 1.0f;
    return r * sinf(x * pi) * sinf((x / r) * pi) / (pi * pi * x * x);
}
// pre, mj: W x H; hist, out, out_copy (a second image that gets the same texels, or NULL): F W x F H
template <int F> RP_DEV void rp_taa_pass(int W, int H, const uchar4 *pre, const uchar4 *hist, const uint2 *mj, uchar4 *out, uchar4 *out_copy) {
    using L = RpTaaLayout<F>;
    __shared__ float4 s_pre[L::PRE * L::PRE];
    __shared__ uchar4 s_hist[L::WIN * L::PITCH];
    __shared__ float s_unorm[256]; // byte / 255 (texelFetch of RGBA8), the same IEEE quotients without a division per tap
    const int DW = F * W, DH = F * H;
    const int tx0 = int(blockIdx.x) * RP_TAA_TILE, ty0 = int(blockIdx.y) * RP_TAA_TILE; // (multiples of F: the tile covers whole F x F blocks)
    const int t = int(threadIdx.x);
    const float fw = float(DW), fh = float(DH);
    for (int k = t; k < 256; k += 64) s_unorm[k] = float(k) / 255.0f;
    for (int k = t; k < L::PRE * L::PRE; k += 64) {
        const int sy = k / L::PRE, sx = k - sy * L::PRE;
        const int gx = (tx0 >> L::SHIFT) + sx - 1, gy = (ty0 >> L::SHIFT) + sy - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f); // imageLoad outside the image: zero
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            const uchar4 b = pre[size_t(gy) * size_t(W) + size_t(gx)];
            v = make_float4(float(b.x) / 255.0f, float(b.y) / 255.0f, float(b.z) / 255.0f, float(b.w) / 255.0f);
        }
        s_pre[k] = v;
    }
    // the window: where the first pixel's taps begin (every thread computes the same two integers)
    int bx, by;
    {
        const float2 m0 = rp_half2_lo(mj[size_t(ty0 >> L::SHIFT) * size_t(W) + size_t(tx0 >> L::SHIFT)].x);
        const float bpx = (((float(tx0) + 0.5f) / fw + 0.5f * m0.x) * fw) - 0.5f;
        const float bpy = (((float(ty0) + 0.5f) / fh + 0.5f * m0.y) * fh) - 0.5f;
        bx = rp_trunc_i(ceilf(bpx)) - L::LEAD;
        by = rp_trunc_i(ceilf(bpy)) - L::LEAD;
        for (int k = t; k < L::WIN * L::WIN; k += 64) {
            const int wy = k / L::WIN, wx = k % L::WIN;
            const int qy = by + wy, qx = bx + wx;
            s_hist[wy * L::PITCH + wx] = (qx >= 0 && qy >= 0 && qx < DW && qy < DH) ? hist[size_t(qy) * size_t(DW) + size_t(qx)] : make_uchar4(0, 0, 0, 0);
        }
    }
    __syncthreads();
    const int lx = t & 7, ly = t >> 3;
    const int px = tx0 + lx, py = ty0 + ly;
    if (px >= DW || py >= DH) return;
    const size_t i = size_t(py) * size_t(DW) + size_t(px);
    const size_t ri = size_t(py >> L::SHIFT) * size_t(W) + size_t(px >> L::SHIFT); // the render pixel under this display pixel
    const int c = ((ly >> L::SHIFT) + 1) * L::PRE + ((lx >> L::SHIFT) + 1);
    float4 col = s_pre[c];
    float2 motion = rp_half2_lo(mj[ri].x);
    float motion_len = motion.x * motion.x + motion.y * motion.y;
    for (int k = 0; k < 9; ++k) { // :63-71 as written: the centre, nine times
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
    if (rpx >= 0.0f && rpy >= 0.0f && rpx <= 1.0f && rpy <= 1.0f) { // lanczos(reconstruction_point, 5) (:35-51, 82)
        const float ptx = rpx * fw - 0.5f, pty = rpy * fh - 0.5f;
        const float cpx = ceilf(ptx), cpy = ceilf(pty);
        // lanczosWeight(vec2) is a product of one factor per axis: the 10 + 10 factors are evaluated once (the same values the
        // reference's 100 taps compute, in the same products). At F = 1 the division is by 1.0f: exact, and the compiler drops it
        float wx[10], wy[10];
        for (int o = 0; o < 10; ++o) {
            wx[o] = rp_lanczos_weight(((float(F * (o - 5)) + cpx) - ptx) / float(F), 5.0f);
            wy[o] = rp_lanczos_weight(((float(F * (o - 5)) + cpy) - pty) / float(F), 5.0f);
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float total = 0.0f;
        for (int oy = -5; oy < 5; ++oy)
            for (int ox = -5; ox < 5; ++ox) {
                const float npx = float(F * ox) + cpx, npy = float(F * oy) + cpy;
                const float w = wx[ox + 5] * wy[oy + 5];
                const int qx = rp_trunc_i(npx), qy = rp_trunc_i(npy);
                uchar4 b = make_uchar4(0, 0, 0, 0);
                const unsigned wxi = unsigned(qx - bx), wyi = unsigned(qy - by);
                if (wxi < unsigned(L::WIN) && wyi < unsigned(L::WIN))
                    b = s_hist[wyi * L::PITCH + wxi];
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
                const float4 v = s_pre[c + oy * L::PRE + ox];
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
    const uchar4 o = rp_rgba8(col);
    out[i] = o;
    if (out_copy) out_copy[i] = o;
}
__global__ __launch_bounds__(64) void rp_k_taa(RpFrame f, const uchar4 *pre, const uchar4 *hist, const uint2 *mj, uchar4 *out, uchar4 *out_copy) {
    rp_taa_pass<1>(f.width, f.height, pre, hist, mj, out, out_copy);
}

