// bloom.h -- a glare pass between exposure and the display image (rptr_hip_bloom, include/rptr_hip.h): what exceeds a threshold in the
// exposed linear image is spread over a pyramid of ever coarser images and added back in front of the tone map, so that an 8-bit image can
// show that a light is brighter than white. Included by rptr_hip.hip only (after auto_exposure.h, whose display arithmetic and device
// state it uses). The pass reads the source image, the frame's RGBA8 image and the exposure state and stores to none of them.
//
// Arithmetic. fp32 under the build's -ffp-contract=off with IEEE division; every product and sum is rounded, in the order written.
// Pyramid texels are float4 with w = +0. min / max below never see a NaN. tests/bloom_ref.py is written from THIS text and reproduces
// every level of both pyramids and the image bit for bit.
//
// Scale. exposure_mode 0: s = float(exp2(double(RptrRenderParams.exposure))), evaluated by the host (auto-exposure's manual rule).
//   exposure_mode 1: s = the `scale` of the device's RptrExposureState, as the last mode-1 rptr_hip_auto_exposure call left it; every kernel
//   that needs it reads it from there.
// Prefilter. Per source texel (c, a), with T = threshold, K = knee, C = clamp: x_k = c_k * s. The texel contributes (0, 0, 0) when
//   !(fminf(a, 1) >= 0) (rp_k_expose's rule: such a texel shows the frame's RGBA8) or any x_k is NaN or infinite. Otherwise
//     x_k = x_k > 0 ? x_k : +0          (fmaxf(x_k, 0), with -0 becoming +0)
//     b = max(max(x_0, x_1), x_2)
//     q = min(max(b - (T - K), 0), 2 K);   q = (q * q) / (4 K + 1e-5f)
//     e = min(max(q, b - T), C)
//     f = e / max(b, 1e-5f);   p_k = x_k * f
//   (T - K, 2 K and 4 K + 1e-5f are fp32 expressions of the parameters alone: the host evaluates them.) The soft knee is the usual
//   quadratic between T - K and T + K; e is how much of the brightest channel passes, at most C: one firefly texel of 1e6 contributes what a
//   texel of T + C does. With T = K = 0 a texel passes unchanged up to C (b / b is exactly 1).
// Sizes. w_0 x h_0 = W x H, w_l = (w_(l-1) + 1) / 2, likewise h (integer division). L_max is the first level at which both are 1.
//   levels = 0: L = the largest level <= 8 with min(w_L, h_L) >= 2, at least 1. Otherwise L = min(levels, L_max).
// Down. Level 1 reads the prefiltered source, level l > 1 reads d(l-1). With P[j][i] the source at (clamp(2x - 1 + i), clamp(2y - 1 + j)),
//   i, j = 0..3, clamped to the source's extent, per channel
//     r_j = (0.125f P[j][0] + 0.375f P[j][1]) + (0.375f P[j][2] + 0.125f P[j][3])
//     d   = (0.125f r_0 + 0.375f r_1) + (0.375f r_2 + 0.125f r_3)
//   (the binomial 1 3 3 1 / 8 on both axes: its weights sum to 1 and it is centred on the 2 x 2 block the texel stands for).
// Up. u(L) = d(L); for l = L - 1 .. 1: u(l) = d(l) + scatter * B(u(l+1)), B the exact 2x bilinear at texel (x, y) of the finer level:
//     i0 = (x - 1) >> 1 (arithmetic shift), i1 = i0 + 1, both clamped to the coarser level's extent;
//     a0 = 0.75f for odd x, 0.25f for even x, a1 the other; the same rule in y gives j0, j1, b0, b1;
//     h_j = a0 u[j][i0] + a1 u[j][i1];   B = b0 h_j0 + b1 h_j1.
// Composite, per displayed pixel with source texel (c, a): x_k = c_k * s; when intensity != 0: x_k = x_k + gain * B(u(1))_k, B as above
//   at the pixel; gain = float(double(intensity) / S), S = the sum of double(scatter)^k over k = 0 .. L - 1, accumulated upwards with the
//   powers made by repeated multiplication (host). Then auto_exposure.h's display rule from its balance step on (rp_ae_display): balance,
//   tone map, sRGB, rp_rgba8; a texel with !(fminf(a, 1) >= 0) keeps the frame's RGBA8 texel. With intensity 0 the image is
//   rptr_hip_readback_exposed_u8's for the same mode and parameters, byte for byte.
//
// Kernels. Two launches are hot at 1920 x 1080: level 1 (reads the 33 MB float image, each source texel is a tap of four outputs) and the
// composite (reads the float image, the RGBA8 frame and u(1), writes 8 MB). The rest is a chain of dependent launches on small images:
// launch latency, as texture_mips.h found for its chain.
//   rp_k_bloom_down<FIRST>    one thread per output texel, grid-stride; FIRST: the taps are prefiltered source texels (16 fetches and 16
//                             divisions per output).
//   rp_k_bloom_down1_tile     level 1 with the prefiltered source tile in LDS: a block of 256 makes 16 x 16 outputs from a 34 x 34 tile,
//                             kept as three planes of floats (13.9 KB); each source texel is fetched, and divided, once per block, 1.13
//                             times per texel over the image where the plain form has 4.
//   rp_k_bloom_up             one thread per texel of u(l).
//   rp_k_bloom_tail           ONE workgroup runs every level from the first whose texel count is at most RP_BLOOM_TAIL_TEXELS down to L
//                             and the up sweep back to that level, in LDS (dynamic, 12 bytes per texel of those levels: at most
//                             2 * 2048 + 12 texels, 49 KB, so below the 64 KB that would need the dynamic-LDS attribute); u(l) overwrites
//                             d(l) in place, since a texel of u(l) reads only its own texel of d(l); d and u go to the global pyramids as
//                             they are made. At 1080p levels 5 .. 8 (60 x 34 and below): one launch where the plain chain has seven.
//   rp_k_bloom_composite      one thread per pixel, rp_k_expose's shape.
// Every form calls the same per-texel functions (rp_bloom_prefilter, rp_bloom_down_texel, rp_bloom_upsample): identical bits.
// Which forms the library launches, why, and registers and LDS per kernel: profiles/bloom_notes.md. The other forms stay reachable from
// tests/device_probes/bloom_probe.hip. No kernel uses scratch (tests/test_bloom_cpu.py reads it from the code object).
#pragma once
#include "auto_exposure.h"

#define RP_BLOOM_MAX_LEVELS 12    // RPTR_BLOOM_MAX_LEVELS
#define RP_BLOOM_TILE 16          // rp_k_bloom_down1_tile: outputs per tile edge; the source tile has 2 * 16 + 2 texels per edge
#define RP_BLOOM_TILE_SRC (2 * RP_BLOOM_TILE + 2)
#define RP_BLOOM_TAIL_TEXELS 2048 // rp_k_bloom_tail: the first level with at most this many texels starts the tail
#define RP_BLOOM_TAIL_THREADS 1024
// the forms rptr_hip_bloom launches (profiles/bloom_notes.md has the measurements behind the choice)
#define RP_BLOOM_SHIP_TILE 1      // level 1: rp_k_bloom_down1_tile
#define RP_BLOOM_SHIP_TAIL 1      // the small levels: rp_k_bloom_tail

// the sizes of the levels and where each starts in a pyramid buffer (texels; level l at off[l], levels 1 .. L back to back)
struct RpBloomPyramid {
    int L, L_max;
    uint32_t w[RP_BLOOM_MAX_LEVELS + 1], h[RP_BLOOM_MAX_LEVELS + 1];
    uint32_t off[RP_BLOOM_MAX_LEVELS + 2]; // off[L + 1] = the texels of levels 1 .. L
};
// levels: RptrBloomParams.levels (0: auto). W, H >= 1. (A frame is at most 16384 x 16384: the offsets fit 32 bits.)
static inline RpBloomPyramid rp_bloom_pyramid(uint32_t W, uint32_t H, int levels) {
    RpBloomPyramid p;
    memset(&p, 0, sizeof(p));
    p.w[0] = W;
    p.h[0] = H;
    int l_max = 1, l_auto = 1;
    for (uint32_t w = W, h = H, l = 1;; ++l) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (l <= RP_BLOOM_MAX_LEVELS) {
            p.w[l] = w;
            p.h[l] = h;
        }
        if (l <= 8 && (w < h ? w : h) >= 2) l_auto = int(l);
        if (w == 1 && h == 1) {
            l_max = int(l);
            break;
        }
    }
    p.L_max = l_max;
    p.L = levels == 0 ? l_auto : (levels < l_max ? levels : l_max);
    if (p.L > RP_BLOOM_MAX_LEVELS) p.L = RP_BLOOM_MAX_LEVELS;
    p.off[1] = 0;
    for (int l = 1; l <= p.L; ++l) p.off[l + 1] = p.off[l] + p.w[l] * p.h[l];
    return p;
}

struct RpBloomPrefilter {
    const RptrExposureState *state; // exposure_mode 1: s is read from here; NULL: `scale`
    float scale;
    float T, C;
    float t_minus_k, k2, k4e; // T - K, 2 K, 4 K + 1e-5f
};
static inline RpBloomPrefilter rp_bloom_prefilter_args(const RptrExposureState *state, float scale, float T, float K, float C) {
    RpBloomPrefilter p;
    p.state = state;
    p.scale = scale;
    p.T = T;
    p.C = C;
    p.t_minus_k = T - K;
    p.k2 = 2.0f * K;
    p.k4e = 4.0f * K + 1e-5f;
    return p;
}
// gain of the composite: float(double(intensity) / sum of double(scatter)^k, k < L)
static inline float rp_bloom_gain(float intensity, float scatter, int L) {
    double sum = 0.0, term = 1.0;
    for (int k = 0; k < L; ++k) {
        sum += term;
        term *= double(scatter);
    }
    return float(double(intensity) / sum);
}

struct RpBloomDownArgs {
    const float4 *src; // FIRST / tile: the source image; else d(l-1)
    float4 *dst;       // d(l)
    float4 *dst_u;     // l == L: u(L) as well; else NULL
    int sw, sh, dw, dh;
    RpBloomPrefilter pf;
};
struct RpBloomUpArgs {
    const float4 *d;  // d(l)
    const float4 *uc; // u(l+1), cw x ch
    float4 *u;        // u(l), w x h
    int w, h, cw, ch;
    float scatter;
};
struct RpBloomTailArgs {
    const float4 *src;   // first: the source image; else d(l0 - 1)
    float4 *d, *u;       // the global pyramids
    int first;           // l0 == 1
    int l0, L;
    uint32_t w[RP_BLOOM_MAX_LEVELS + 1], h[RP_BLOOM_MAX_LEVELS + 1], off[RP_BLOOM_MAX_LEVELS + 2];
    float scatter;
    RpBloomPrefilter pf;
};
struct RpBloomCompositeArgs {
    RpExposeArgs x;   // src, fb, out, state / scale, the display fields
    const float4 *u1; // w1 x h1
    int W, H, w1, h1;
    float gain;
    int add;          // intensity != 0
};

struct RpBloom3 {
    float x, y, z;
};
RP_DEV float4 rp_bloom_texel(const RpBloom3 &v) { return make_float4(v.x, v.y, v.z, 0.0f); }
RP_DEV int rp_bloom_clamp(int v, int n) { return min(max(v, 0), n - 1); }

RP_DEV RpBloom3 rp_bloom_prefilter(const float4 c, float s, const RpBloomPrefilter &p) {
    float x = c.x * s, y = c.y * s, z = c.z * s;
    const bool finite = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; // (false for a NaN)
    if (!(fminf(c.w, 1.0f) >= 0.0f) || !finite) return RpBloom3{0.0f, 0.0f, 0.0f};
    x = x > 0.0f ? x : 0.0f;
    y = y > 0.0f ? y : 0.0f;
    z = z > 0.0f ? z : 0.0f;
    const float b = fmaxf(fmaxf(x, y), z);
    float q = fminf(fmaxf(b - p.t_minus_k, 0.0f), p.k2);
    q = (q * q) / p.k4e;
    const float e = fminf(fmaxf(q, b - p.T), p.C);
    const float f = e / fmaxf(b, 1e-5f);
    return RpBloom3{x * f, y * f, z * f};
}

RP_DEV float rp_bloom_1331(float a, float b, float c, float d) { return (0.125f * a + 0.375f * b) + (0.375f * c + 0.125f * d); }

// P(xx, yy): the source texel, coordinates already clamped to sw x sh
template <class Fetch>
RP_DEV RpBloom3 rp_bloom_down_texel(const Fetch &P, int x, int y, int sw, int sh) {
    int xs[4];
    for (int i = 0; i < 4; ++i) xs[i] = rp_bloom_clamp(2 * x - 1 + i, sw);
    RpBloom3 r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = rp_bloom_clamp(2 * y - 1 + j, sh);
        const RpBloom3 t0 = P(xs[0], yy), t1 = P(xs[1], yy), t2 = P(xs[2], yy), t3 = P(xs[3], yy);
        r[j] = RpBloom3{rp_bloom_1331(t0.x, t1.x, t2.x, t3.x), rp_bloom_1331(t0.y, t1.y, t2.y, t3.y), rp_bloom_1331(t0.z, t1.z, t2.z, t3.z)};
    }
    return RpBloom3{rp_bloom_1331(r[0].x, r[1].x, r[2].x, r[3].x), rp_bloom_1331(r[0].y, r[1].y, r[2].y, r[3].y), rp_bloom_1331(r[0].z, r[1].z, r[2].z, r[3].z)};
}

// B(u) at texel (x, y) of the finer level; U(i, j): the coarser level's texel, cw x ch
template <class Fetch>
RP_DEV RpBloom3 rp_bloom_upsample(const Fetch &U, int x, int y, int cw, int ch) {
    const int i0 = rp_bloom_clamp((x - 1) >> 1, cw), i1 = rp_bloom_clamp(((x - 1) >> 1) + 1, cw);
    const int j0 = rp_bloom_clamp((y - 1) >> 1, ch), j1 = rp_bloom_clamp(((y - 1) >> 1) + 1, ch);
    const float a0 = (x & 1) ? 0.75f : 0.25f, a1 = (x & 1) ? 0.25f : 0.75f;
    const float b0 = (y & 1) ? 0.75f : 0.25f, b1 = (y & 1) ? 0.25f : 0.75f;
    const RpBloom3 p00 = U(i0, j0), p01 = U(i1, j0), p10 = U(i0, j1), p11 = U(i1, j1);
    const RpBloom3 h0{a0 * p00.x + a1 * p01.x, a0 * p00.y + a1 * p01.y, a0 * p00.z + a1 * p01.z};
    const RpBloom3 h1{a0 * p10.x + a1 * p11.x, a0 * p10.y + a1 * p11.y, a0 * p10.z + a1 * p11.z};
    return RpBloom3{b0 * h0.x + b1 * h1.x, b0 * h0.y + b1 * h1.y, b0 * h0.z + b1 * h1.z};
}

struct RpBloomFetchGlobal { // a pyramid level (or any float4 image)
    const float4 *img;
    int w;
    RP_DEV RpBloom3 operator()(int x, int y) const {
        const float4 t = img[size_t(y) * size_t(w) + size_t(x)];
        return RpBloom3{t.x, t.y, t.z};
    }
};
struct RpBloomFetchSource { // the source image through the prefilter
    const float4 *img;
    int w;
    float s;
    const RpBloomPrefilter *pf;
    RP_DEV RpBloom3 operator()(int x, int y) const { return rp_bloom_prefilter(img[size_t(y) * size_t(w) + size_t(x)], s, *pf); }
};
struct RpBloomFetchLds { // a level kept as three floats per texel
    const float *lvl;
    int w;
    RP_DEV RpBloom3 operator()(int x, int y) const {
        const float *t = lvl + 3 * (y * w + x);
        return RpBloom3{t[0], t[1], t[2]};
    }
};

// One thread per output texel. (dw * dh <= 2^26.)
template <bool FIRST>
__global__ __launch_bounds__(256) void rp_k_bloom_down(RpBloomDownArgs a) {
    const float s = FIRST ? (a.pf.state ? a.pf.state->scale : a.pf.scale) : 0.0f;
    const uint32_t n = uint32_t(a.dw) * uint32_t(a.dh);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = int(i / uint32_t(a.dw)), x = int(i - uint32_t(y) * uint32_t(a.dw));
        RpBloom3 v;
        if (FIRST)
            v = rp_bloom_down_texel(RpBloomFetchSource{a.src, a.sw, s, &a.pf}, x, y, a.sw, a.sh);
        else
            v = rp_bloom_down_texel(RpBloomFetchGlobal{a.src, a.sw}, x, y, a.sw, a.sh);
        a.dst[i] = rp_bloom_texel(v);
        if (a.dst_u) a.dst_u[i] = rp_bloom_texel(v);
    }
}

// Level 1 from a prefiltered source tile in LDS: tile (tx, ty) makes the outputs [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16) from the source
// texels clamp(32 tx - 1 + i), clamp(32 ty - 1 + j), i, j = 0..33 -- stored already clamped, so that a tap is an LDS read at (2 lx + i, 2 ly + j).
__global__ __launch_bounds__(256) void rp_k_bloom_down1_tile(RpBloomDownArgs a) {
    __shared__ float s_t[3][RP_BLOOM_TILE_SRC][RP_BLOOM_TILE_SRC + 1];
    const float s = a.pf.state ? a.pf.state->scale : a.pf.scale;
    const int t = int(threadIdx.x), lx = t & (RP_BLOOM_TILE - 1), ly = t / RP_BLOOM_TILE;
    const uint32_t tiles_x = (uint32_t(a.dw) + RP_BLOOM_TILE - 1) / RP_BLOOM_TILE, tiles_y = (uint32_t(a.dh) + RP_BLOOM_TILE - 1) / RP_BLOOM_TILE;
    for (uint32_t tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) { // (block-uniform: every thread makes every round)
        const int ty = int(tile / tiles_x), tx = int(tile - uint32_t(ty) * tiles_x);
        const int sx0 = 2 * RP_BLOOM_TILE * tx - 1, sy0 = 2 * RP_BLOOM_TILE * ty - 1;
        for (int k = t; k < RP_BLOOM_TILE_SRC * RP_BLOOM_TILE_SRC; k += 256) {
            const int j = k / RP_BLOOM_TILE_SRC, i = k - j * RP_BLOOM_TILE_SRC;
            const int xx = rp_bloom_clamp(sx0 + i, a.sw), yy = rp_bloom_clamp(sy0 + j, a.sh);
            const RpBloom3 p = rp_bloom_prefilter(a.src[size_t(yy) * size_t(a.sw) + size_t(xx)], s, a.pf);
            s_t[0][j][i] = p.x;
            s_t[1][j][i] = p.y;
            s_t[2][j][i] = p.z;
        }
        __syncthreads();
        const int x = RP_BLOOM_TILE * tx + lx, y = RP_BLOOM_TILE * ty + ly;
        if (x < a.dw && y < a.dh) {
            RpBloom3 r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jj = 2 * ly + j, ii = 2 * lx;
                r[j] = RpBloom3{rp_bloom_1331(s_t[0][jj][ii], s_t[0][jj][ii + 1], s_t[0][jj][ii + 2], s_t[0][jj][ii + 3]),
                                rp_bloom_1331(s_t[1][jj][ii], s_t[1][jj][ii + 1], s_t[1][jj][ii + 2], s_t[1][jj][ii + 3]),
                                rp_bloom_1331(s_t[2][jj][ii], s_t[2][jj][ii + 1], s_t[2][jj][ii + 2], s_t[2][jj][ii + 3])};
            }
            const RpBloom3 v{rp_bloom_1331(r[0].x, r[1].x, r[2].x, r[3].x), rp_bloom_1331(r[0].y, r[1].y, r[2].y, r[3].y), rp_bloom_1331(r[0].z, r[1].z, r[2].z, r[3].z)};
            const size_t o = size_t(y) * size_t(a.dw) + size_t(x);
            a.dst[o] = rp_bloom_texel(v);
            if (a.dst_u) a.dst_u[o] = rp_bloom_texel(v);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rp_k_bloom_up(RpBloomUpArgs a) {
    const uint32_t n = uint32_t(a.w) * uint32_t(a.h);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = int(i / uint32_t(a.w)), x = int(i - uint32_t(y) * uint32_t(a.w));
        const RpBloom3 v = rp_bloom_upsample(RpBloomFetchGlobal{a.uc, a.cw}, x, y, a.cw, a.ch);
        const float4 d = a.d[i];
        a.u[i] = make_float4(d.x + a.scatter * v.x, d.y + a.scatter * v.y, d.z + a.scatter * v.z, 0.0f);
    }
}

// One workgroup: levels l0 .. L down, then up to l0, in LDS (s_pyr: the levels back to back, three floats per texel).
__global__ __launch_bounds__(RP_BLOOM_TAIL_THREADS) void rp_k_bloom_tail(RpBloomTailArgs a) {
    extern __shared__ float s_pyr[];
    const int t = int(threadIdx.x), nt = int(blockDim.x);
    const float s = a.first ? (a.pf.state ? a.pf.state->scale : a.pf.scale) : 0.0f;
    const uint32_t base = a.off[a.l0]; // level l sits at 3 * (off[l] - base) in s_pyr
    for (int l = a.l0; l <= a.L; ++l) {
        const int w = int(a.w[l]), h = int(a.h[l]), sw = int(a.w[l - 1]), sh = int(a.h[l - 1]);
        float *lvl = s_pyr + 3 * (a.off[l] - base);
        for (int i = t; i < w * h; i += nt) {
            const int y = i / w, x = i - y * w;
            RpBloom3 v;
            if (l > a.l0)
                v = rp_bloom_down_texel(RpBloomFetchLds{s_pyr + 3 * (a.off[l - 1] - base), sw}, x, y, sw, sh);
            else if (a.first)
                v = rp_bloom_down_texel(RpBloomFetchSource{a.src, sw, s, &a.pf}, x, y, sw, sh);
            else
                v = rp_bloom_down_texel(RpBloomFetchGlobal{a.src, sw}, x, y, sw, sh);
            lvl[3 * i + 0] = v.x;
            lvl[3 * i + 1] = v.y;
            lvl[3 * i + 2] = v.z;
            a.d[a.off[l] + uint32_t(i)] = rp_bloom_texel(v);
            if (l == a.L) a.u[a.off[l] + uint32_t(i)] = rp_bloom_texel(v);
        }
        __syncthreads();
    }
    for (int l = a.L - 1; l >= a.l0; --l) {
        const int w = int(a.w[l]), h = int(a.h[l]), cw = int(a.w[l + 1]), ch = int(a.h[l + 1]);
        float *lvl = s_pyr + 3 * (a.off[l] - base);
        for (int i = t; i < w * h; i += nt) {
            const int y = i / w, x = i - y * w;
            const RpBloom3 v = rp_bloom_upsample(RpBloomFetchLds{s_pyr + 3 * (a.off[l + 1] - base), cw}, x, y, cw, ch);
            const RpBloom3 r{lvl[3 * i + 0] + a.scatter * v.x, lvl[3 * i + 1] + a.scatter * v.y, lvl[3 * i + 2] + a.scatter * v.z};
            lvl[3 * i + 0] = r.x;
            lvl[3 * i + 1] = r.y;
            lvl[3 * i + 2] = r.z;
            a.u[a.off[l] + uint32_t(i)] = rp_bloom_texel(r);
        }
        __syncthreads();
    }
}

// One thread per pixel, rp_k_expose with one add. (A frame is at most 16384 x 16384: a pixel index fits 32 bits.)
__global__ __launch_bounds__(256) void rp_k_bloom_composite(RpBloomCompositeArgs a) {
    const float scale = a.x.state ? a.x.state->scale : a.x.scale;
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.x.npix; i += size_t(gridDim.x) * blockDim.x) {
        const float4 c = a.x.src[i];
        uchar4 shown = a.x.fb[i];
        const float w = fminf(c.w, 1.0f);
        if (w >= 0.0f) {
            float x = c.x * scale, y = c.y * scale, z = c.z * scale;
            if (a.add) {
                const int py = int(uint32_t(i) / uint32_t(a.W)), px = int(uint32_t(i) - uint32_t(py) * uint32_t(a.W));
                const RpBloom3 g = rp_bloom_upsample(RpBloomFetchGlobal{a.u1, a.w1}, px, py, a.w1, a.h1);
                x = x + a.gain * g.x;
                y = y + a.gain * g.y;
                z = z + a.gain * g.z;
            }
            shown = rp_ae_display(a.x, x, y, z, w);
        }
        a.x.out[i] = shown;
    }
}

// ---- the launch sequence, shared by rptr_hip_bloom (host_access.inl) and tests/device_probes/bloom_probe.hip
struct RpBloomRun {
    RpBloomPyramid pyr;
    RpBloomPrefilter pf;
    RpBloomCompositeArgs comp; // complete but for u1, w1, h1
    float4 *d, *u;             // the pyramids: pyr.off[pyr.L + 1] texels each
    float scatter;
    unsigned max_blocks;       // grid cap of every grid-stride launch
    int stages;                // bit 0: level 1, bit 1: the rest of the pyramid, bit 2: the composite (7: all; subsets: timing)
};
static inline int rp_bloom_tail_start(const RpBloomPyramid &p) { // the first level the tail runs; L + 1: none fits
    for (int l = 1; l <= p.L; ++l)
        if (p.w[l] * p.h[l] <= RP_BLOOM_TAIL_TEXELS) return l;
    return p.L + 1;
}
static inline unsigned rp_bloom_grid(size_t work_items, unsigned max_blocks) {
    const size_t blocks = (work_items + 255) / 256;
    return unsigned(blocks < 1 ? 1 : (blocks > max_blocks ? max_blocks : blocks));
}
// TILE: level 1 by rp_k_bloom_down1_tile (else rp_k_bloom_down<true>); TAIL: the levels that fit by rp_k_bloom_tail (else one launch per
// level). Template arguments, so that a translation unit holds only the forms it asks for: the library's one pair, the probe's four.
template <bool TILE, bool TAIL>
static inline void rp_bloom_enqueue(const RpBloomRun &r, hipStream_t st) {
    const RpBloomPyramid &p = r.pyr;
    const int L = p.L, l0 = TAIL ? rp_bloom_tail_start(p) : L + 1;
    const float4 *src = r.comp.x.src;
    for (int l = 1; l <= L && l < l0; ++l) {
        if ((l == 1 && !(r.stages & 1)) || (l > 1 && !(r.stages & 2))) continue;
        RpBloomDownArgs a;
        a.src = l == 1 ? src : r.d + p.off[l - 1];
        a.dst = r.d + p.off[l];
        a.dst_u = l == L ? r.u + p.off[l] : nullptr;
        a.sw = int(p.w[l - 1]);
        a.sh = int(p.h[l - 1]);
        a.dw = int(p.w[l]);
        a.dh = int(p.h[l]);
        a.pf = r.pf;
        const size_t n = size_t(a.dw) * size_t(a.dh);
        if (l == 1) {
            if constexpr (TILE) {
                const size_t tiles = size_t((a.dw + RP_BLOOM_TILE - 1) / RP_BLOOM_TILE) * size_t((a.dh + RP_BLOOM_TILE - 1) / RP_BLOOM_TILE);
                hipLaunchKernelGGL(rp_k_bloom_down1_tile, dim3(rp_bloom_grid(tiles * 256, r.max_blocks)), dim3(256), 0, st, a);
            } else
                hipLaunchKernelGGL(rp_k_bloom_down<true>, dim3(rp_bloom_grid(n, r.max_blocks)), dim3(256), 0, st, a);
        } else
            hipLaunchKernelGGL(rp_k_bloom_down<false>, dim3(rp_bloom_grid(n, r.max_blocks)), dim3(256), 0, st, a);
    }
    if constexpr (TAIL) if (l0 <= L && (r.stages & (l0 == 1 ? 1 : 2))) {
        RpBloomTailArgs a;
        memset(&a, 0, sizeof(a));
        a.src = l0 == 1 ? src : r.d + p.off[l0 - 1];
        a.d = r.d;
        a.u = r.u;
        a.first = l0 == 1 ? 1 : 0;
        a.l0 = l0;
        a.L = L;
        memcpy(a.w, p.w, sizeof(a.w));
        memcpy(a.h, p.h, sizeof(a.h));
        memcpy(a.off, p.off, sizeof(a.off));
        a.scatter = r.scatter;
        a.pf = r.pf;
        const size_t lds = size_t(p.off[L + 1] - p.off[l0]) * 3 * sizeof(float); // <= (2 * RP_BLOOM_TAIL_TEXELS + 12) * 12 bytes
        hipLaunchKernelGGL(rp_k_bloom_tail, dim3(1), dim3(RP_BLOOM_TAIL_THREADS), lds, st, a);
    }
    if (r.stages & 2)
        for (int l = (L - 1 < l0 - 1 ? L - 1 : l0 - 1); l >= 1; --l) {
            RpBloomUpArgs a;
            a.d = r.d + p.off[l];
            a.uc = r.u + p.off[l + 1];
            a.u = r.u + p.off[l];
            a.w = int(p.w[l]);
            a.h = int(p.h[l]);
            a.cw = int(p.w[l + 1]);
            a.ch = int(p.h[l + 1]);
            a.scatter = r.scatter;
            hipLaunchKernelGGL(rp_k_bloom_up, dim3(rp_bloom_grid(size_t(a.w) * size_t(a.h), r.max_blocks)), dim3(256), 0, st, a);
        }
    if (r.stages & 4) {
        RpBloomCompositeArgs c = r.comp;
        c.u1 = r.u + p.off[1];
        c.w1 = int(p.w[1]);
        c.h1 = int(p.h[1]);
        hipLaunchKernelGGL(rp_k_bloom_composite, dim3(rp_bloom_grid(c.x.npix, r.max_blocks)), dim3(256), 0, st, c);
    }
}
