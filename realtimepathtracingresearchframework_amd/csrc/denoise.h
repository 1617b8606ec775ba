// denoise.h -- a spatial denoiser for the last finished frame (rptr_hip_denoise, include/rptr_hip.h): an edge-avoiding a-trous wavelet
// filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for Fast Global Illumination Filtering", HPG 2010)
// with the edge-stopping weights and the variance guidance of the spatial part of SVGF (Schied et al., HPG 2017), run on
// albedo-demodulated colour and guided by the frame's own normal + depth and albedo AOV images. It stands where the reference's hosts
// link Open Image Denoise (enable_denoising; process_samples.comp's denoise_buffer): that library cannot exist here. Included by
// rptr_hip.hip only (after realtime_resolve.h). The denoiser writes images of its own; it reads the frame's images and stores to none.
//
// Arithmetic. Everything is fp32 under the build's -ffp-contract=off, with IEEE division and square root; exp, pow, exp2 and log2 are
// evaluated in double and rounded once to float (as realtime_resolve.h does with its exp); sums run left to right in scan order, dy
// outer, dx inner; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; min / max are fminf / fmaxf. Every operation is then correctly rounded,
// so the numpy restatement (tests/denoise_ref.py, written from THIS text) reproduces the stored images bit for bit.
//
// Inputs per pixel p: c, a = the accumulation image's rgb and w; A = the albedo AOV's rgb; N, z = the normal + depth AOV (halfs widened
// to float). surface(p): z is finite, z > 0, dot(N, N) > 0 (a camera ray that missed stores N = 0 and an infinite half depth) and A is
// not (0, 0, 0). The last condition is this file's addition to the rule the feature was specified with: a directly visible emitter
// stores albedo 0 (dshade.h rp_unpack_material zeroes an emitter's base colour) and its radiance is no reflected light -- divided by
// the floor 0.01 it becomes 100 x the radiance, and the ceiling around a Cornell box's lamp, same normal and depth, came out at 400
// where it should be 0.5 (profiles/denoise_notes.md). Emitters are therefore left as they are and never tapped, like the background.
//
// Prepare.  d = max(A, 0.01) per channel; e = c / d when demodulating, else e = c.  lum(e) = (0.2126 e.x + 0.7152 e.y) + 0.0722 e.z.
//   v  = the variance of lum over the 3x3 neighbours q (p included) that lie inside the image, are surface and face p's way,
//        dot(N_p, N_q) > 0: s1 += lum, s2 += lum * lum, m1 = s1 / float(n), m2 = s2 / float(n), v = max(m2 - m1 * m1, 0).
//        (The normal test is this file's addition to the rule the feature was specified with: without it the colours beyond a
//        geometric edge reach v of the pixels along it, and through v their luminance weights -- the filter would not be edge-avoiding
//        in the exact sense tests/test_denoise_cpu.py checks: replacing one side of a right-angled edge leaves the other side's bits.)
//   gz = the larger of |z(x+1, y) - z| and |z(x, y+1) - z| over those of the two neighbours that are inside the image and surface; 0 if
//        none is.
//   A pixel that is not surface (background, emitter) gets e = c, v = 0, gz = 0.
// Pass i = 0 .. iterations - 1, spacing s = 1 << i. Reads the (e, v) image pass i - 1 stored (pass 0: prepare's), for surface p only;
//   other pixels carry (e, v) through. Taps q = p + s (dx, dy), dx, dy in -2 .. 2; taps outside the image or on pixels that are not
//   surface are skipped. With lum_p = lum(e_p), lum_q = lum(e_q) of the pass's INPUT image and v_p its input variance:
//     h  = k[|dx|] * k[|dy|], k = {3/8, 1/4, 1/16}
//     t  = min(max(dot(N_p, N_q), 0), 1), then t = t * t, normal_power_log2 times
//     az = |z_q - z_p| / ((((sigma_depth * gz_p) * float(s)) * float(max(|dx|, |dy|))) + 1e-3f * z_p)
//     al = |lum_q - lum_p| / (sigma_luminance * sqrt(v_p) + 1e-4f)
//     w  = (h * t) * float(exp(double(-(az + al))))
//     sw += w;  se += w * e_q (per channel);  sv += (w * w) * v_q
//   stored: e' = se / sw, v' = sv / (sw * sw). The centre tap has w = 9/64, so sw >= 9/64.
//   The passes ping-pong between two images: no thread reads what another stores in the same launch.
// Finish.  A surface pixel gets (e * d, a), or (e, a) without demodulation; any other pixel the accumulation image's texel bit for bit.
//   RGBA8: with output_channel 0, o = (that colour, min(a, 1)); o.w < 0 keeps the frame's own RGBA8 texel (the resolve's rule), else
//   rp_rgba8 of the display colour below. With output_channel != 0 the RGBA8 image is a copy of the frame's (an AOV view: nothing to
//   denoise).
//   Display colour -- rp_display_color's OUTPUT_CHANNEL_COLOR branch with its transcendental functions evaluated in double and rounded
//   once (THE ONE RULE CHANGED AGAINST rp_display_color: powf / exp2f / log2f of the device library are accurate to an ulp or two, not
//   correctly rounded, and no restatement could name their bits; a texel can therefore differ from the frame's own RGBA8 by one step
//   where the denoiser changed nothing):
//     x = o.rgb * float(exp2(double(exposure)));
//     early_tone_mapping_mode 2: x = x / (1 + x); 1: L = max(max(x.r, x.g), max(x.b, 1)), g = float(log2(double(L))),
//       x = x * (((0.1f * g) * (1 - 0.8f) + 1 * 0.8f) / L); other: x
//     srgb(x) = x <= 0.0031308f ? 12.92f * x : 1.055f * float(pow(double(max(|x|, 1.192092896e-07f)), double(1.f / 2.4f))) - 0.055f
//   The render parameters are those in force at the denoise call.
//
// Layout of the pass (the hot kernel: 25 taps of two 16-byte records, (e, v) and (N, z), per pixel). One block = 256 threads = a tile of
// 16 x 16 pixels; the records of the tile and of its two-tap apron are staged in LDS once and every tap is an LDS read.
//   Spacings 1 and 2: the tile is 16 x 16 ADJACENT pixels, its window (16 + 4 s)^2 records: 20 x 20 (12.5 KB) and 24 x 24 (18 KB).
//   Spacings 4, 8, 16: the tile is 16 x 16 pixels of ONE sub-lattice (x mod s, y mod s) = (ox, oy), pixels ox + s i, oy + s j; in lattice
//   units the taps are the neighbours -2 .. 2 again, the window is 20 x 20 records whatever s is, and the same LDS code serves every
//   spacing. The alternative -- adjacent tiles that gather their 25 taps from global memory -- reads 25 x 32 = 800 bytes per pixel
//   through the vector L1 (1.7 GB per 1080p pass; at s >= 4 no two taps of a pixel share a 128-byte line and neighbouring lanes only
//   share along x), where the lattice tile reads (20 / 16)^2 x 32 = 50 bytes per pixel, the same as spacing 1. Its price: a wave's
//   16-byte loads and stores lie s x 16 bytes apart (64 .. 256), so one wave instruction touches 16 .. 64 lines instead of 8; the lines
//   are shared with the s x s blocks of the other sub-lattices of the same area, which run at about the same time, and the two input
//   images of a 1080p frame (66 MB) fit the 256 MB last-level cache. Estimated, see profiles/denoise_notes.md for what was measured.
//   The window cell of a tap outside the image holds zeros, prepare stores z = 0 for a pixel that is not surface: one test, z_q > 0,
//   skips both. Partial tiles: lanes beyond the right / bottom edge (or beyond the lattice's last column / row) stage and then leave.
// Code object (hipcc 6.x, gfx950, -O3): see profiles/denoise_notes.md for registers and LDS of the three kernels; none uses scratch.
#pragma once
#include "realtime_resolve.h"

#define RP_DN_TILE 16 // pixels per tile and axis: 256 threads, four waves
#define RP_DN_TAPS 2  // taps to each side

struct RpDenoiseArgs {
    const float4 *accum;  // the source frame's accumulation image
    const uint2 *albedo;  // its albedo + roughness AOV (RGBA16F)
    const uint2 *nd;      // its normal + depth AOV (RGBA16F)
    const uchar4 *fb;     // its RGBA8 frame
    float4 *ndz;          // (N, z) widened to float; all zero where the pixel is not surface
    float *gz;            // the depth gradient of prepare
    float4 *out_f32;      // the denoised images
    uchar4 *out_u8;
    int width, height;
    float sigma_luminance, sigma_depth;
    int normal_power_log2, demodulate;
    int output_channel, tone_mapping_mode; // RptrRenderParams at the call
    float exposure_scale;                  // float(exp2(double(exposure))), rounded on the host
};

RP_DEV float rp_dn_lum(float4 e) { return (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z; }
RP_DEV bool rp_dn_surface(float4 nd, uint2 albedo) {
    const float4 A = rp_half4_to_float4(albedo);
    return nd.w > 0.0f && nd.w < INFINITY && ((nd.x * nd.x + nd.y * nd.y) + nd.z * nd.z) > 0.0f && !(A.x == 0.0f && A.y == 0.0f && A.z == 0.0f);
}
RP_DEV float4 rp_dn_divisor(uint2 albedo) {
    const float4 A = rp_half4_to_float4(albedo);
    return make_float4(fmaxf(A.x, 0.01f), fmaxf(A.y, 0.01f), fmaxf(A.z, 0.01f), 1.0f);
}
// (e, 0) of one pixel
RP_DEV float4 rp_dn_signal(const RpDenoiseArgs &a, size_t i, bool surface) {
    const float4 c = a.accum[i];
    if (!surface || !a.demodulate) return make_float4(c.x, c.y, c.z, 0.0f);
    const float4 d = rp_dn_divisor(a.albedo[i]);
    return make_float4(c.x / d.x, c.y / d.y, c.z / d.z, 0.0f);
}

// What prepare and rp_k_denoise_temporal (denoise_temporal.h) share. One block = 16 x 16 adjacent pixels; lum and (N, z) (zeros: outside
// the image, or not surface) of the tile and a 1-pixel apron go through LDS, in two arrays of RP_DN_SPAN * RP_DN_SPAN the kernel declares.
#define RP_DN_SPAN (RP_DN_TILE + 2)
RP_DEV void rp_dn_stage(const RpDenoiseArgs &a, float *s_lum, float4 *s_nd) {
    const int W = a.width, H = a.height;
    const int tx0 = int(blockIdx.x) * RP_DN_TILE, ty0 = int(blockIdx.y) * RP_DN_TILE;
    for (int k = int(threadIdx.x); k < RP_DN_SPAN * RP_DN_SPAN; k += 256) {
        const int sy = k / RP_DN_SPAN, sx = k - sy * RP_DN_SPAN;
        const int gx = tx0 + sx - 1, gy = ty0 + sy - 1;
        float lum = 0.0f;
        float4 ndz = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            const size_t g = size_t(gy) * size_t(W) + size_t(gx);
            const float4 nd = rp_half4_to_float4(a.nd[g]);
            if (rp_dn_surface(nd, a.albedo[g])) {
                lum = rp_dn_lum(rp_dn_signal(a, g, true));
                ndz = nd;
            }
        }
        s_lum[k] = lum;
        s_nd[k] = ndz;
    }
    __syncthreads();
}
// v_s and gz (the header's "Prepare") of the surface pixel at cell c of the staged arrays, ndp = s_nd[c]
RP_DEV void rp_dn_spatial(const float *s_lum, const float4 *s_nd, int c, float4 ndp, float &v_s, float &gz) {
    float s1 = 0.0f, s2 = 0.0f;
    int n = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int q = c + dy * RP_DN_SPAN + dx;
            const float4 ndq = s_nd[q];
            if (ndq.w > 0.0f && ((ndp.x * ndq.x + ndp.y * ndq.y) + ndp.z * ndq.z) > 0.0f) {
                const float l = s_lum[q];
                s1 += l;
                s2 += l * l;
                ++n;
            }
        }
    const float m1 = s1 / float(n), m2 = s2 / float(n); // (n >= 1: p itself)
    v_s = fmaxf(m2 - m1 * m1, 0.0f);
    gz = 0.0f;
    const float zr = s_nd[c + 1].w, zd = s_nd[c + RP_DN_SPAN].w;
    if (zr > 0.0f) gz = fmaxf(gz, fabsf(zr - ndp.w));
    if (zd > 0.0f) gz = fmaxf(gz, fabsf(zd - ndp.w));
}

__global__ __launch_bounds__(256) void rp_k_denoise_prepare(RpDenoiseArgs a, float4 *ev) {
    __shared__ float s_lum[RP_DN_SPAN * RP_DN_SPAN];
    __shared__ float4 s_nd[RP_DN_SPAN * RP_DN_SPAN];
    rp_dn_stage(a, s_lum, s_nd);
    const int t = int(threadIdx.x);
    const int lx = t & (RP_DN_TILE - 1), ly = t / RP_DN_TILE;
    const int px = int(blockIdx.x) * RP_DN_TILE + lx, py = int(blockIdx.y) * RP_DN_TILE + ly;
    if (px >= a.width || py >= a.height) return;
    const size_t i = size_t(py) * size_t(a.width) + size_t(px);
    const int c = (ly + 1) * RP_DN_SPAN + (lx + 1);
    const float4 ndp = s_nd[c];
    const bool surface = ndp.w > 0.0f;
    float4 e = rp_dn_signal(a, i, surface);
    float gz = 0.0f;
    if (surface) rp_dn_spatial(s_lum, s_nd, c, ndp, e.w, gz);
    ev[i] = e;
    a.gz[i] = gz;
    a.ndz[i] = ndp;
}

RP_DEV float rp_dn_kernel(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// S = 1, 2: adjacent tiles of that spacing (s == S); S = 0: a tile of one sub-lattice of spacing s (4, 8, 16). Window cell (wx, wy) holds
// pixel (x0 + wx * pitch, y0 + wy * pitch); a tap step is STEP cells.
template <int S>
__global__ __launch_bounds__(256) void rp_k_denoise_pass(RpDenoiseArgs a, const float4 *in, float4 *out, int s) {
    constexpr int STEP = S ? S : 1;
    constexpr int APRON = RP_DN_TAPS * STEP;
    constexpr int WIN = RP_DN_TILE + 2 * APRON;
    __shared__ float4 s_ev[WIN * WIN];
    __shared__ float4 s_nd[WIN * WIN];
    const int W = a.width, H = a.height;
    int pitch, x0, y0;
    if (S) {
        pitch = 1;
        x0 = int(blockIdx.x) * RP_DN_TILE - APRON;
        y0 = int(blockIdx.y) * RP_DN_TILE - APRON;
    } else { // blockIdx = lattice offset + s * lattice tile
        pitch = s;
        const int bx = int(blockIdx.x), by = int(blockIdx.y);
        x0 = bx % s + ((bx / s) * RP_DN_TILE - APRON) * s;
        y0 = by % s + ((by / s) * RP_DN_TILE - APRON) * s;
    }
    const int t = int(threadIdx.x);
    for (int k = t; k < WIN * WIN; k += 256) {
        const int wy = k / WIN, wx = k - wy * WIN;
        const int gx = x0 + wx * pitch, gy = y0 + wy * pitch;
        float4 ev = make_float4(0.f, 0.f, 0.f, 0.f), nd = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            const size_t g = size_t(gy) * size_t(W) + size_t(gx);
            ev = in[g];
            nd = a.ndz[g];
        }
        s_ev[k] = ev;
        s_nd[k] = nd;
    }
    __syncthreads();
    const int lx = t & (RP_DN_TILE - 1), ly = t / RP_DN_TILE;
    const int px = x0 + (lx + APRON) * pitch, py = y0 + (ly + APRON) * pitch;
    if (px >= W || py >= H) return;
    const size_t i = size_t(py) * size_t(W) + size_t(px);
    const int c = (ly + APRON) * WIN + (lx + APRON);
    const float4 ndp = s_nd[c], evp = s_ev[c];
    if (!(ndp.w > 0.0f)) { // not surface: carried through
        out[i] = evp;
        return;
    }
    const float lump = rp_dn_lum(evp);
    const float den_l = a.sigma_luminance * sqrtf(evp.w) + 1e-4f;
    const float den_z0 = (a.sigma_depth * a.gz[i]) * float(s), den_z1 = 1e-3f * ndp.w;
    float sw = 0.0f, sv = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int dy = -RP_DN_TAPS; dy <= RP_DN_TAPS; ++dy)
        for (int dx = -RP_DN_TAPS; dx <= RP_DN_TAPS; ++dx) {
            const int q = c + (dy * WIN + dx) * STEP;
            const float4 ndq = s_nd[q];
            if (!(ndq.w > 0.0f)) continue;
            const float4 evq = s_ev[q];
            const float h = rp_dn_kernel(dx) * rp_dn_kernel(dy);
            float tn = fminf(fmaxf((ndp.x * ndq.x + ndp.y * ndq.y) + ndp.z * ndq.z, 0.0f), 1.0f);
            for (int j = 0; j < a.normal_power_log2; ++j) tn = tn * tn;
            const int m = max(abs(dx), abs(dy));
            const float az = fabsf(ndq.w - ndp.w) / (den_z0 * float(m) + den_z1);
            const float al = fabsf(rp_dn_lum(evq) - lump) / den_l;
            const float w = (h * tn) * float(exp(double(-(az + al)))); // exp, correctly rounded to float (see the header)
            sw += w;
            sx += w * evq.x;
            sy += w * evq.y;
            sz += w * evq.z;
            sv += (w * w) * evq.w;
        }
    out[i] = make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
}

// rp_display_color's colour branch, transcendental functions in double and rounded once (the header's "Display colour")
RP_DEV float rp_dn_srgb(float x) {
    return (x <= 0.0031308f) ? 12.92f * x : 1.055f * float(pow(double(fmaxf(fabsf(x), 1.192092896e-07f)), double(1.f / 2.4f))) - 0.055f;
}
// ... from the exposed colour on: the tone map and sRGB (auto_exposure.h ends with the same two steps)
RP_DEV float4 rp_dn_tone_map_srgb(int tone_mapping_mode, float x, float y, float z, float w) {
    if (tone_mapping_mode == 2) {
        x = x / (1.0f + x);
        y = y / (1.0f + y);
        z = z / (1.0f + z);
    } else if (tone_mapping_mode == 1) {
        const float L = fmaxf(fmaxf(x, y), fmaxf(z, 1.0f));
        const float g = float(log2(double(L)));
        const float k = ((0.1f * g) * (1.0f - 0.8f) + 1.0f * 0.8f) / L;
        x = x * k;
        y = y * k;
        z = z * k;
    }
    return make_float4(rp_dn_srgb(x), rp_dn_srgb(y), rp_dn_srgb(z), w);
}
RP_DEV float4 rp_dn_display(const RpDenoiseArgs &a, float4 o) {
    return rp_dn_tone_map_srgb(a.tone_mapping_mode, o.x * a.exposure_scale, o.y * a.exposure_scale, o.z * a.exposure_scale, o.w);
}

// One thread per pixel: remodulate, store both images
__global__ __launch_bounds__(256) void rp_k_denoise_finish(RpDenoiseArgs a, const float4 *ev) {
    const size_t npix = size_t(a.width) * size_t(a.height);
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < npix; i += size_t(gridDim.x) * blockDim.x) {
        float4 res = a.accum[i];
        if (a.ndz[i].w > 0.0f) {
            const float4 e = ev[i];
            if (a.demodulate) {
                const float4 d = rp_dn_divisor(a.albedo[i]);
                res = make_float4(e.x * d.x, e.y * d.y, e.z * d.z, res.w);
            } else
                res = make_float4(e.x, e.y, e.z, res.w);
        }
        a.out_f32[i] = res;
        uchar4 shown = a.fb[i];
        if (a.output_channel == 0) {
            const float4 o = make_float4(res.x, res.y, res.z, fminf(res.w, 1.0f));
            if (o.w >= 0.0f) shown = rp_rgba8(rp_dn_display(a, o));
        }
        a.out_u8[i] = shown;
    }
}
