// k_shade_query.hip -- instantiations of the first shade of a radiance-query run (kernels.h rp_k_shade_query) for ONE gpu-program variant and ONE build of the shading arithmetic: -DRP_INST_VARIANT=0|1|2 -DRP_FAST_MATH=0|1 (dmath.h)
#include "launch.h"

#ifndef RP_INST_VARIANT
#error "build with -DRP_INST_VARIANT=<RPTR_VARIANT_*>"
#endif
#define RP_CAT2(a, b) a##b
#define RP_CAT(a, b) RP_CAT2(a, b)
#if RP_FAST_MATH
#define RP_LAUNCHER(stem) RP_CAT(RP_CAT(stem, fast_v), RP_INST_VARIANT)
#else
#define RP_LAUNCHER(stem) RP_CAT(RP_CAT(stem, ieee_v), RP_INST_VARIANT)
#endif

void RP_LAUNCHER(rp_launch_shade_query_)(const RpLaunch &l, bool lights, bool tex, bool table, const RpScene &sc, const RpFrame &f, const RpPathState &ps,
                                         const RpShadowRays &sq, const uint32_t *count_ptr, uint32_t *next_queue, uint32_t *next_count,
                                         uint32_t *shadow_count, RpCounters *ctr) {
    rp_pick(lights, [&](auto L) {
        rp_pick(tex, [&](auto X) {
            rp_pick(table, [&](auto T) {
                rp_launch_kernel(l, rp_k_shade_query<RP_INST_VARIANT, decltype(L)::value, decltype(X)::value, decltype(T)::value>, 256u, sc, f, ps, sq, count_ptr,
                                 next_queue, next_count, shadow_count, ctr);
            });
        });
    });
}
