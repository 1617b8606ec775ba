// bloom_probe.hip -- TEST INFRASTRUCTURE: the bloom pass of csrc/bloom.h on caller-supplied arrays.
//
// bp_run runs the prefilter, the pyramid and the composite -- the library's own kernels through the library's own launch sequence
// (rp_bloom_enqueue), nothing of them is restated here -- on a float image and an RGBA8 image the caller chose: what a rendered frame
// cannot supply (NaN, infinities, negatives, alpha outside [0, 1], any size). The caller picks the scale (passed by value, or through a
// device-side RptrExposureState as exposure_mode 1 reads it), either form of level 1 (tile 0: rp_k_bloom_down<true>, 1:
// rp_k_bloom_down1_tile), either form of the chain (tail 0: one launch per level, 1: rp_k_bloom_tail), and a cap on the blocks of every
// grid-stride launch. bp_time times the whole sequence or a part of it (tools/bloom_cost.py; profiles/bloom_notes.md). bp_constants
// exports the tile and tail constants the tests aim their sizes at.
//
// Built by tests/device_probes/bloom.py with the product's compiler flags: libbloom_probe.so. Not part of librptr_hip.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rptr_hip.h"
#include "bloom.h"

#define BP_TRY(expr)                                                                                                                   \
    do {                                                                                                                               \
        const hipError_t e_ = (expr);                                                                                                  \
        if (e_ != hipSuccess) {                                                                                                        \
            fprintf(stderr, "bloom_probe: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);               \
            rc = 1;                                                                                                                    \
            goto done;                                                                                                                 \
        }                                                                                                                              \
    } while (0)

namespace {
struct Buffers {
    float4 *src = nullptr, *d = nullptr, *u = nullptr;
    uchar4 *fb = nullptr, *out = nullptr;
    RptrExposureState *state = nullptr;
};
void release(Buffers &b) {
    (void)hipFree(b.src);
    (void)hipFree(b.d);
    (void)hipFree(b.u);
    (void)hipFree(b.fb);
    (void)hipFree(b.out);
    (void)hipFree(b.state);
}
bool params_ok(const RptrBloomParams *p, int W, int H, int max_blocks) {
    return p && W >= 1 && H >= 1 && W <= 16384 && H <= 16384 && max_blocks >= 1 && max_blocks <= 65536 && p->levels >= 0 && p->levels <= RPTR_BLOOM_MAX_LEVELS &&
           p->threshold >= 0.0f && p->knee >= 0.0f && p->clamp > 0.0f && p->intensity >= 0.0f && p->scatter >= 0.0f && p->scatter <= 1.0f;
}
// the run of one call, filled as csrc/host_access.inl rptr_hip_bloom fills it
RpBloomRun make_run(const Buffers &b, int W, int H, const RptrBloomParams *p, float scale, int from_state, int max_blocks, int stages) {
    RpBloomRun r;
    memset(&r, 0, sizeof(r));
    RpExposeArgs &x = r.comp.x;
    x.src = b.src;
    x.fb = b.fb;
    x.out = b.out;
    x.npix = size_t(W) * size_t(H);
    x.tone_mapping_mode = p->tone_mapping_mode;
    x.balance = (p->white_balance[0] != 1.0f || p->white_balance[1] != 1.0f || p->white_balance[2] != 1.0f) ? 1 : 0;
    for (int k = 0; k < 3; ++k) x.gains[k] = p->white_balance[k];
    x.state = from_state ? b.state : nullptr;
    x.scale = from_state ? 0.0f : scale;
    r.pyr = rp_bloom_pyramid(uint32_t(W), uint32_t(H), p->levels);
    r.pf = rp_bloom_prefilter_args(x.state, x.scale, p->threshold, p->knee, p->clamp);
    r.comp.W = W;
    r.comp.H = H;
    r.comp.gain = rp_bloom_gain(p->intensity, p->scatter, r.pyr.L);
    r.comp.add = p->intensity != 0.0f ? 1 : 0;
    r.d = b.d;
    r.u = b.u;
    r.scatter = p->scatter;
    r.max_blocks = unsigned(max_blocks);
    r.stages = stages;
    return r;
}
void enqueue(const RpBloomRun &r, int tile, int tail) { // every pair of forms: this file alone instantiates the ones the library does not launch
    if (tile && tail)
        rp_bloom_enqueue<true, true>(r, nullptr);
    else if (tile)
        rp_bloom_enqueue<true, false>(r, nullptr);
    else if (tail)
        rp_bloom_enqueue<false, true>(r, nullptr);
    else
        rp_bloom_enqueue<false, false>(r, nullptr);
}
} // namespace

extern "C" {
// out[0..5]: RP_BLOOM_TILE, RP_BLOOM_TILE_SRC, RP_BLOOM_TAIL_TEXELS, RP_BLOOM_MAX_LEVELS, the forms the library launches (tile, tail)
void bp_constants(int out[6]) {
    out[0] = RP_BLOOM_TILE;
    out[1] = RP_BLOOM_TILE_SRC;
    out[2] = RP_BLOOM_TAIL_TEXELS;
    out[3] = RP_BLOOM_MAX_LEVELS;
    out[4] = RP_BLOOM_SHIP_TILE;
    out[5] = RP_BLOOM_SHIP_TAIL;
}

// texels4: W x H float4; fb: W x H RGBA8. Out: the level count, the first level the tail ran (L + 1: none), the two pyramids (levels
// 1 .. L back to back, `pyramid_texels` texels of room each) and the image.
int bp_run(const float *texels4, const unsigned char *fb, int W, int H, const RptrBloomParams *p, float scale, int from_state, int tile, int tail, int max_blocks,
           int *levels_out, int *tail_start_out, float *d_out, float *u_out, size_t pyramid_texels, unsigned char *image_out) {
    if (!texels4 || !fb || !params_ok(p, W, H, max_blocks) || !levels_out || !tail_start_out || !d_out || !u_out || !image_out) return 2;
    int rc = 0;
    Buffers b;
    const size_t npix = size_t(W) * size_t(H);
    const RpBloomPyramid pyr = rp_bloom_pyramid(uint32_t(W), uint32_t(H), p->levels);
    const size_t texels = pyr.off[pyr.L + 1];
    if (pyramid_texels < texels) return 2;
    RptrExposureState st;
    memset(&st, 0, sizeof(st));
    st.scale = scale;
    BP_TRY(hipMalloc(&b.src, npix * sizeof(float4)));
    BP_TRY(hipMalloc(&b.fb, npix * sizeof(uchar4)));
    BP_TRY(hipMalloc(&b.out, npix * sizeof(uchar4)));
    BP_TRY(hipMalloc(&b.d, texels * sizeof(float4)));
    BP_TRY(hipMalloc(&b.u, texels * sizeof(float4)));
    BP_TRY(hipMalloc(&b.state, sizeof(RptrExposureState)));
    BP_TRY(hipMemcpy(b.src, texels4, npix * sizeof(float4), hipMemcpyHostToDevice));
    BP_TRY(hipMemcpy(b.fb, fb, npix * sizeof(uchar4), hipMemcpyHostToDevice));
    BP_TRY(hipMemcpy(b.state, &st, sizeof(st), hipMemcpyHostToDevice));
    BP_TRY(hipMemset(b.out, 0xA5, npix * sizeof(uchar4)));
    BP_TRY(hipMemset(b.d, 0xFF, texels * sizeof(float4))); // (NaNs: a texel no kernel wrote shows)
    BP_TRY(hipMemset(b.u, 0xFF, texels * sizeof(float4)));
    {
        const RpBloomRun r = make_run(b, W, H, p, scale, from_state, max_blocks, 7);
        enqueue(r, tile, tail);
        *levels_out = r.pyr.L;
        *tail_start_out = tail ? rp_bloom_tail_start(r.pyr) : r.pyr.L + 1;
    }
    BP_TRY(hipGetLastError());
    BP_TRY(hipDeviceSynchronize());
    BP_TRY(hipMemcpy(d_out, b.d, texels * sizeof(float4), hipMemcpyDeviceToHost));
    BP_TRY(hipMemcpy(u_out, b.u, texels * sizeof(float4), hipMemcpyDeviceToHost));
    BP_TRY(hipMemcpy(image_out, b.out, npix * sizeof(uchar4), hipMemcpyDeviceToHost));
done:
    release(b);
    return rc;
}

// The stages of `stages` (bit 0: level 1, bit 1: the rest of the pyramid, bit 2: the composite; 8 alone: rp_k_expose, the manual
// auto-exposure call's one launch, on the same arrays) between two events, `reps` times after `warmup`: the median in microseconds.
// One whole run precedes the timed ones, so that a part finds the pyramid levels it reads.
int bp_time(const float *texels4, const unsigned char *fb, int W, int H, const RptrBloomParams *p, float scale, int tile, int tail, int max_blocks, int stages,
            int warmup, int reps, float *median_us) {
    if (!texels4 || !fb || !params_ok(p, W, H, max_blocks) || !median_us || reps < 1 || reps > 100000 || warmup < 0 || stages < 1 || stages > 8) return 2;
    int rc = 0;
    Buffers b;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<float> us;
    const size_t npix = size_t(W) * size_t(H);
    const RpBloomPyramid pyr = rp_bloom_pyramid(uint32_t(W), uint32_t(H), p->levels);
    const size_t texels = pyr.off[pyr.L + 1];
    BP_TRY(hipMalloc(&b.src, npix * sizeof(float4)));
    BP_TRY(hipMalloc(&b.fb, npix * sizeof(uchar4)));
    BP_TRY(hipMalloc(&b.out, npix * sizeof(uchar4)));
    BP_TRY(hipMalloc(&b.d, texels * sizeof(float4)));
    BP_TRY(hipMalloc(&b.u, texels * sizeof(float4)));
    BP_TRY(hipMemcpy(b.src, texels4, npix * sizeof(float4), hipMemcpyHostToDevice));
    BP_TRY(hipMemcpy(b.fb, fb, npix * sizeof(uchar4), hipMemcpyHostToDevice));
    BP_TRY(hipEventCreate(&e0));
    BP_TRY(hipEventCreate(&e1));
    {
        const RpBloomRun whole = make_run(b, W, H, p, scale, 0, max_blocks, 7);
        const RpBloomRun part = make_run(b, W, H, p, scale, 0, max_blocks, stages & 7);
        enqueue(whole, tile, tail);
        for (int k = 0; k < warmup + reps; ++k) {
            BP_TRY(hipEventRecord(e0, nullptr));
            if (stages == 8)
                hipLaunchKernelGGL(rp_k_expose, dim3(rp_bloom_grid(npix, unsigned(max_blocks))), dim3(256), 0, nullptr, part.comp.x);
            else
                enqueue(part, tile, tail);
            BP_TRY(hipEventRecord(e1, nullptr));
            BP_TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            BP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (k >= warmup) us.push_back(ms * 1000.0f);
        }
    }
    BP_TRY(hipGetLastError());
    std::sort(us.begin(), us.end());
    *median_us = us[us.size() / 2];
done:
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    release(b);
    return rc;
}
}
