// exposure_probe.hip -- TEST INFRASTRUCTURE: the meter of csrc/auto_exposure.h on a caller-supplied float4 array.
//
// ep_meter runs rp_k_meter and rp_k_meter_reduce -- the library's own kernels, nothing of them is restated here -- on `n` texels the
// caller chose: what a rendered frame cannot supply (NaN, infinities, negatives, denormals, exact bin edges, any length). The host-side
// constants of the reduce kernel's arguments (T, log2 key, the two adaptation factors) are filled as csrc/host_access.inl
// rptr_hip_auto_exposure fills them. combine = 0 launches rp_k_meter<false>, the instantiation the library launches; 1 the one with the
// wave-combine step, which only this file builds. ep_time_meter times either alone (tools/auto_exposure_timing.py;
// profiles/auto_exposure_notes.md).
//
// Built by tests/device_probes/exposure.py with the product's compiler flags: libexposure_probe.so. Not part of librptr_hip.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rptr_hip.h"
#include "auto_exposure.h"

#define EP_TRY(expr)                                                                                                                   \
    do {                                                                                                                               \
        const hipError_t e_ = (expr);                                                                                                  \
        if (e_ != hipSuccess) {                                                                                                        \
            fprintf(stderr, "exposure_probe: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);            \
            rc = 1;                                                                                                                    \
            goto done;                                                                                                                 \
        }                                                                                                                              \
    } while (0)

extern "C" {
// p: the call's parameters (source and the display fields are not used); exposure: RptrRenderParams.exposure; blocks: the meter's grid;
// state_in: NULL = no state since initialize, else the state the call starts from. Out: the state after the call and the RP_AE_WORDS
// words of the working histogram as the reduce kernel left them (all zero).
int ep_meter(const float *texels4, size_t n, const RptrAutoExposureParams *p, float exposure, int blocks, int combine, const RptrExposureState *state_in,
             RptrExposureState *state_out, uint32_t *hist_after) {
    if (!texels4 || !n || !p || !state_out || !hist_after || blocks < 1 || blocks > 65536) return 2;
    int rc = 0;
    float4 *d_src = nullptr;
    uint32_t *d_hist = nullptr;
    RptrExposureState *d_state = nullptr;
    RpMeterReduceArgs m;
    memset(&m, 0, sizeof(m));
    EP_TRY(hipMalloc(&d_src, n * sizeof(float4)));
    EP_TRY(hipMalloc(&d_hist, RP_AE_WORDS * sizeof(uint32_t)));
    EP_TRY(hipMalloc(&d_state, sizeof(RptrExposureState)));
    EP_TRY(hipMemcpy(d_src, texels4, n * sizeof(float4), hipMemcpyHostToDevice));
    EP_TRY(hipMemset(d_hist, 0, RP_AE_WORDS * sizeof(uint32_t)));
    EP_TRY(hipMemset(d_state, 0, sizeof(RptrExposureState)));
    if (state_in) EP_TRY(hipMemcpy(d_state, state_in, sizeof(RptrExposureState), hipMemcpyHostToDevice));
    m.hist = d_hist;
    m.state = d_state;
    for (int s = 0; s < 8; ++s) m.T[s] = std::log2(1.0 + ((double)s + 0.5) / 8.0);
    m.log2_key = std::log2((double)p->key);
    m.k_up = 1.0 - std::exp(-(double)p->dt * (double)p->speed_up);
    m.k_down = 1.0 - std::exp(-(double)p->dt * (double)p->speed_down);
    m.low_percentile = p->low_percentile;
    m.high_percentile = p->high_percentile;
    m.min_ev = p->min_ev;
    m.max_ev = p->max_ev;
    m.exposure = exposure;
    m.have_state = state_in ? 1 : 0;
    m.reset_history = p->reset_history;
    m.jump = p->dt == 0.0f ? 1 : 0;
    if (combine)
        rp_k_meter<true><<<unsigned(blocks), 256>>>(d_src, n, d_hist);
    else
        rp_k_meter<false><<<unsigned(blocks), 256>>>(d_src, n, d_hist);
    rp_k_meter_reduce<<<1, 256>>>(m);
    EP_TRY(hipGetLastError());
    EP_TRY(hipDeviceSynchronize());
    EP_TRY(hipMemcpy(state_out, d_state, sizeof(RptrExposureState), hipMemcpyDeviceToHost));
    EP_TRY(hipMemcpy(hist_after, d_hist, RP_AE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
done:
    (void)hipFree(d_src);
    (void)hipFree(d_hist);
    (void)hipFree(d_state);
    return rc;
}

// rp_k_meter alone, `reps` launches after `warmup`, each between two events: the median in microseconds. The histogram is cleared (a
// 1 KB fill, outside the events) before each launch.
int ep_time_meter(const float *texels4, size_t n, int blocks, int combine, int warmup, int reps, float *median_us) {
    if (!texels4 || !n || !median_us || blocks < 1 || blocks > 65536 || reps < 1 || reps > 100000 || warmup < 0) return 2;
    int rc = 0;
    float4 *d_src = nullptr;
    uint32_t *d_hist = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    std::vector<float> us;
    EP_TRY(hipMalloc(&d_src, n * sizeof(float4)));
    EP_TRY(hipMalloc(&d_hist, RP_AE_WORDS * sizeof(uint32_t)));
    EP_TRY(hipMemcpy(d_src, texels4, n * sizeof(float4), hipMemcpyHostToDevice));
    EP_TRY(hipEventCreate(&a));
    EP_TRY(hipEventCreate(&b));
    for (int k = 0; k < warmup + reps; ++k) {
        EP_TRY(hipMemsetAsync(d_hist, 0, RP_AE_WORDS * sizeof(uint32_t), nullptr));
        EP_TRY(hipEventRecord(a, nullptr));
        if (combine)
            rp_k_meter<true><<<unsigned(blocks), 256>>>(d_src, n, d_hist);
        else
            rp_k_meter<false><<<unsigned(blocks), 256>>>(d_src, n, d_hist);
        EP_TRY(hipEventRecord(b, nullptr));
        EP_TRY(hipEventSynchronize(b));
        float ms = 0.0f;
        EP_TRY(hipEventElapsedTime(&ms, a, b));
        if (k >= warmup) us.push_back(ms * 1000.0f);
    }
    EP_TRY(hipGetLastError());
    std::sort(us.begin(), us.end());
    *median_us = us[us.size() / 2];
done:
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipFree(d_src);
    (void)hipFree(d_hist);
    return rc;
}
}
