// auto_exposure.h -- a metered display pass for the last finished frame or the denoiser's result (rptr_hip_auto_exposure,
// include/rptr_hip.h): a log-luminance histogram of the float image, an exposure value that adapts over time on the device, and an
// RGBA8 image of its own. It stands where the reference's application runs its "uber post" step (RenderProcessingStep::UberPost; the
// resolve tone-maps only "if we don't have the uber post pass"), whose source is not shipped: the library defines the step. Included by
// rptr_hip.hip only (after denoise.h). The pass reads the source image and the frame's RGBA8 image and stores to neither.
//
// Arithmetic. fp32 under the build's -ffp-contract=off with IEEE division; exp, exp2 and log2 are evaluated in double and rounded once;
// sums run in the stated order. tests/auto_exposure_ref.py is written from THIS text and reproduces the histogram, the state and the
// image bit for bit.
//
// Meter (mode 1). Per pixel with source texel (c, a): lum = (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z. The pixel is IGNORED when a < 0 or
//   lum is NaN, < 0 or infinite. Otherwise bin = min(max(int(bits(|lum|) >> 20) - 887, 0), 255): eight bins per octave, cut by the float's
//   exponent and its top three mantissa bits (|lum| differs from lum for -0 only, which is black like +0). Bin 0 holds everything below
//   2^-16 (BLACK: zero, denormals), bin 1 starts at 2^-16 exactly, 1.0 is bin 129, bin 255 is open-ended. No transcendental function is
//   involved: the integer histogram is exact whatever the order of the atomics.
//   counted = sum of bins 1..255, black = bin 0, ignored as above; the three add up to W H.
//   The representative of bin b >= 1 is v_b = double((b - 1) / 8 - 16) + T[(b - 1) % 8] (integer division), T[s] = log2(1 + (s + 0.5) / 8):
//   the log of the bin's midpoint. Every counted pixel below bin 255 lies within log2(1 + 1/16) < 0.0875 of its representative.
// Target. n = counted, lo = uint64(double(low_percentile) * double(n)), hi = uint64(double(high_percentile) * double(n)). Walking the bins
//   1..255 upwards with the running count c (before the bin), bin b contributes t_b = max(0, min(c + h_b, hi) - max(c, lo)) samples;
//   S = sum of double(t_b) * v_b, N = sum of t_b, both ascending, over the bins with t_b > 0; m = S / double(N);
//   target = float(min(max(log2(double(key)) - m, double(min_ev)), double(max_ev))), mean_log2 = float(m).
//   N = 0 (a black frame, or lo = hi): target = the current ev, or 0 when there is none; mean_log2 = 0.
// Adapt. No state since initialize, or reset_history, or dt = 0: ev' = target. Otherwise r = target > ev ? speed_up : speed_down and
//   ev' = float(double(ev) + (double(target) - double(ev)) * (1 - exp(-double(dt) * double(r)))).
//   calls = 1 after a call without state or with reset_history, else the previous calls + 1.
//   Of these, T, log2(double(key)) and the two factors 1 - exp(...) do not depend on the image: the host evaluates them (in double) and
//   passes them to the reduce kernel, which does the rest: the running counts as a parallel scan, the two sums and the scalar rules on
//   one lane, in the stated order.
// Display. E = exposure + ev' (one float add; RptrRenderParams.exposure at the call; ev' = 0 in manual mode), scale = float(exp2(double(E)))
//   -- computed once by the reduce kernel and stored in the state; in manual mode by the host. Per pixel x = c * scale. If white_balance is
//   not exactly (1, 1, 1): l = M1 x, l = l * gains, x = M2 l, each row (m0 x0 + m1 x1) + m2 x2, with the published linear-sRGB <-> LMS pair
//     M1 = ( 3.90405e-1  5.49941e-1  8.92632e-3 )      M2 = (  2.85847e+0  -1.62879e+0  -2.48910e-2 )
//          ( 7.08416e-2  9.63172e-1  1.35775e-3 )           ( -2.10182e-1   1.15820e+0   3.24281e-4 )
//          ( 2.31082e-2  1.28021e-1  9.36245e-1 )           ( -4.18120e-2  -1.18169e-1   1.06867e+0 )
//   (gains of exactly 1 skip the step: M2 M1 is not the identity in fp32). Then the tone map and sRGB of denoise.h's display colour
//   (rp_dn_tone_map_srgb) with the call's tone_mapping_mode, then rp_rgba8. Alpha is min(a, 1); a texel whose min(a, 1) is not >= 0
//   keeps the frame's RGBA8 texel. With mode 0, source 1, gains 1 and tone_mapping_mode = early_tone_mapping_mode the image is
//   rptr_hip_readback_denoised_u8's, byte for byte.
//
// Kernels: rp_k_meter (the hot one), rp_k_meter_reduce (one block), rp_k_expose (one thread per pixel). rp_k_meter keeps one 256-word
// histogram per wave in LDS (4 KB per block): a lane's pixel is one LDS atomic add into its wave's copy. At its end each thread sums its
// bin over the four waves and issues at most one no-return global add, each wave one for the ignored count; the grid is capped at four
// blocks per CU, so a call makes at most 1024 x 260 global adds on 256 CUs. The reduce kernel zeroes the working histogram after copying
// it: a call enqueues no fill.
// rp_k_meter<true> combines the lanes of a wave that hold the same bin before the LDS atomic -- a ballot / first-lane loop: the first
// pending lane's bin is broadcast, the lanes that hold it are counted with one ballot, the first lane adds the count -- so that a wave
// whose 64 pixels share a bin issues one atomic where 64 same-address atomics serialise. Measured at 1080p it gains 0.4 - 0.7 us on an all-sky
// frame and on an image of one value and loses 1.3 - 1.5 us on an ordinary frame, whose waves hold many distinct bins and make as many
// rounds of the loop (profiles/auto_exposure_notes.md): the library launches rp_k_meter<false>, the plain one; the other instantiation is
// built by tests/device_probes/exposure_probe.hip alone, for tools/auto_exposure_timing.py to repeat the comparison.
// Code object (gfx950, -O3): see profiles/auto_exposure_notes.md for registers and LDS of the three kernels; none uses scratch.
#pragma once
#include "denoise.h"

#define RP_AE_BINS 256
#define RP_AE_WORDS (RP_AE_BINS + 1) // the working histogram: the bins, then the ignored count

struct RpMeterReduceArgs {
    uint32_t *hist;           // RP_AE_WORDS words; left zero
    RptrExposureState *state; // read (ev, calls) and rewritten
    double T[8];              // log2(1 + (s + 0.5) / 8)
    double log2_key;
    double k_up, k_down;      // 1 - exp(-dt * speed_up), 1 - exp(-dt * speed_down)
    float low_percentile, high_percentile, min_ev, max_ev;
    float exposure;           // RptrRenderParams.exposure at the call
    int have_state;           // a metered call has run since initialize
    int reset_history;
    int jump;                 // dt == 0
};

struct RpExposeArgs {
    const float4 *src;              // the accumulation image or the denoiser's float image
    const uchar4 *fb;               // the frame's RGBA8 image
    uchar4 *out;
    const RptrExposureState *state; // mode 1: scale is read from here; NULL: `scale`
    size_t npix;
    float scale;
    int tone_mapping_mode;
    int balance;                    // white_balance is not (1, 1, 1)
    float gains[3];
};

RP_DEV int rp_ae_bin(float lum) { return min(max(int(__float_as_uint(fabsf(lum)) >> 20) - 887, 0), RP_AE_BINS - 1); }

// COMBINE: the ballot / first-lane loop of the header in front of the LDS atomic (false: what the library launches)
template <bool COMBINE>
__global__ __launch_bounds__(256) void rp_k_meter(const float4 *src, size_t npix, uint32_t *hist) {
    __shared__ uint32_t s_hist[4][RP_AE_BINS];
    const int t = int(threadIdx.x), wave = t >> 6;
    for (int k = 0; k < 4; ++k) s_hist[k][t] = 0u;
    __syncthreads();
    uint32_t ignored = 0; // wave-uniform
    const size_t stride = size_t(gridDim.x) * 256;
    for (size_t base = size_t(blockIdx.x) * 256; base < npix; base += stride) { // (base is block-uniform: every lane makes every round)
        const size_t i = base + size_t(t);
        bool pending = false, ign = false;
        int bin = 0;
        if (i < npix) {
            const float4 c = src[i];
            const float lum = rp_dn_lum(c);
            ign = c.w < 0.0f || !(lum >= 0.0f) || lum == INFINITY;
            pending = !ign;
            bin = rp_ae_bin(lum);
        }
        ignored += uint32_t(__popcll(__ballot(ign)));
        if (COMBINE) {
            for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {
                const int first = __ffsll(todo) - 1;
                const int b = __shfl(bin, first);
                const unsigned long long same = __ballot(pending && bin == b);
                if ((t & 63) == first) atomicAdd(&s_hist[wave][b], uint32_t(__popcll(same)));
                if (bin == b) pending = false;
            }
        } else if (pending)
            atomicAdd(&s_hist[wave][bin], 1u);
    }
    __syncthreads();
    const uint32_t n = (s_hist[0][t] + s_hist[1][t]) + (s_hist[2][t] + s_hist[3][t]);
    if (n) atomicAdd(&hist[t], n);
    if ((t & 63) == 0 && ignored) atomicAdd(&hist[RP_AE_BINS], ignored);
}

// One block; thread b owns bin b. The running counts are a parallel scan (integers: exact), every thread forms its bin's t_b and the
// product double(t_b) * v_b, and lane 0 adds the 255 products in ascending order (a bin with t_b = 0 adds +0.0, which changes no bit of
// the sum) and runs the target and adapt rules: one short dependent chain where a one-lane walk over the bins had two long ones.
__global__ __launch_bounds__(256) void rp_k_meter_reduce(RpMeterReduceArgs a) {
    __shared__ uint32_t s_c[RP_AE_BINS]; // inclusive running count of the bins 1 .. b
    __shared__ uint32_t s_t[RP_AE_BINS]; // t_b
    __shared__ double s_p[RP_AE_BINS];   // double(t_b) * v_b
    const int t = int(threadIdx.x);
    const uint32_t mine = a.hist[t];
    a.state->histogram[t] = mine;
    a.hist[t] = 0u;
    const uint32_t hb = t ? mine : 0u; // (bin 0 is black: not counted)
    s_c[t] = hb;
    __syncthreads();
    for (int d = 1; d < RP_AE_BINS; d <<= 1) {
        const uint32_t below = t >= d ? s_c[t - d] : 0u;
        __syncthreads();
        s_c[t] += below;
        __syncthreads();
    }
    const uint32_t n = s_c[RP_AE_BINS - 1];
    const int64_t lo = int64_t(uint64_t(double(a.low_percentile) * double(n))), hi = int64_t(uint64_t(double(a.high_percentile) * double(n)));
    const int64_t c = int64_t(s_c[t]) - int64_t(hb);
    const int64_t tb = max(min(c + int64_t(hb), hi) - max(c, lo), int64_t(0));
    s_t[t] = uint32_t(tb);
    s_p[t] = (t && tb > 0) ? double(tb) * (double((t - 1) / 8 - 16) + a.T[(t - 1) % 8]) : 0.0;
    __syncthreads();
    if (t != 0) return;
    const uint32_t ignored = a.hist[RP_AE_BINS];
    a.hist[RP_AE_BINS] = 0u;
    uint64_t N = 0;
    double S = 0.0;
    for (int b = 1; b < RP_AE_BINS; ++b) {
        S += s_p[b];
        N += s_t[b];
    }
    const float ev = a.have_state ? a.state->ev : 0.0f;
    float target = ev, mean_log2 = 0.0f;
    if (N > 0) {
        const double m = S / double(N);
        target = float(fmin(fmax(a.log2_key - m, double(a.min_ev)), double(a.max_ev)));
        mean_log2 = float(m);
    }
    const bool fresh = !a.have_state || a.reset_history;
    float ev1 = target;
    if (!fresh && !a.jump) ev1 = float(double(ev) + (double(target) - double(ev)) * (target > ev ? a.k_up : a.k_down));
    const float E = a.exposure + ev1;
    a.state->calls = fresh ? 1u : a.state->calls + 1u;
    a.state->ev = ev1;
    a.state->target_ev = target;
    a.state->mean_log2 = mean_log2;
    a.state->scale = float(exp2(double(E)));
    a.state->counted = n;
    a.state->black = mine;
    a.state->ignored = ignored;
}

RP_DEV float rp_ae_row(float m0, float m1, float m2, float x0, float x1, float x2) { return (m0 * x0 + m1 * x1) + m2 * x2; }

// The display rule from the exposed colour (x, y, z) on: balance, tone map, sRGB, RGBA8 (bloom.h's composite ends with the same steps)
RP_DEV uchar4 rp_ae_display(const RpExposeArgs &a, float x, float y, float z, float w) {
    if (a.balance) {
        const float l = rp_ae_row(3.90405e-1f, 5.49941e-1f, 8.92632e-3f, x, y, z) * a.gains[0];
        const float m = rp_ae_row(7.08416e-2f, 9.63172e-1f, 1.35775e-3f, x, y, z) * a.gains[1];
        const float s = rp_ae_row(2.31082e-2f, 1.28021e-1f, 9.36245e-1f, x, y, z) * a.gains[2];
        x = rp_ae_row(2.85847e+0f, -1.62879e+0f, -2.48910e-2f, l, m, s);
        y = rp_ae_row(-2.10182e-1f, 1.15820e+0f, 3.24281e-4f, l, m, s);
        z = rp_ae_row(-4.18120e-2f, -1.18169e-1f, 1.06867e+0f, l, m, s);
    }
    return rp_rgba8(rp_dn_tone_map_srgb(a.tone_mapping_mode, x, y, z, w));
}

// One thread per pixel, the shape of rp_k_denoise_finish
__global__ __launch_bounds__(256) void rp_k_expose(RpExposeArgs a) {
    const float scale = a.state ? a.state->scale : a.scale;
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.npix; i += size_t(gridDim.x) * blockDim.x) {
        const float4 c = a.src[i];
        uchar4 shown = a.fb[i];
        const float w = fminf(c.w, 1.0f);
        if (w >= 0.0f) shown = rp_ae_display(a, c.x * scale, c.y * scale, c.z * scale, w);
        a.out[i] = shown;
    }
}
