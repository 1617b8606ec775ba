// occlusion_query.h -- occlusion queries (include/rptr_hip.h rptr_hip_trace_occlusion*): "does anything lie on this ray inside (t_min, t_max)?",
// one BIT per query. One launch per call: rp_k_trace_occlusion<ALPHA, SINGLE>, the any-hit traversal of a frame's shadow rays
// (dtraverse.h rp_wave_trace<ANY = true>: the first accepted hit ends the query, children are visited longest stretch first) over the query
// records, with the interval start of rp_k_trace (RPTR_RAY_EPSILON * |origin|) and the scene's own scheduling thresholds and pool size.
// ALPHA is the cutout rule (dshade.h rp_alpha_below_cutoff: deterministic, no random number); without it every triangle is opaque.
// Included by rptr_hip.hip only (one definition per kernel).
#pragma once
#include "kernels.h"

// How a finished query's bit reaches its word. The 32 queries of a word finish in different lanes at different steps of a persistent wave
// (lanes refill from later pools while others still walk), and the bits of skipped queries and those behind n belong to the caller: a
// blind store of the word is not possible. Pools are multiples of 64 consecutive queries, so a word is only ever written by one wave --
// the atomics order nothing between waves, they merge bits that arrive at different times into one word.
//   1 (the default: measured, profiles/occlusion_queries_notes.md)  the lanes that one refill retires (dtraverse.h) are grouped by word with
//     ballots and the group's first lane issues one OR (the hits) and one AND (the misses) for the word, or a plain store when the
//     group is the whole word. The bits of a group come from two
//     ballots when every lane of the group holds the query whose bit index is its own lane index modulo 32 (a wave that refills all its
//     lanes at once -- the first fill, rays that leave the scene at the root -- is dealt its queries that way), else they are collected
//     into scalar registers lane by lane (v_readlane).
//   0  every finished query issues one no-return vector atomic on its word: two instructions per step whatever the number of lanes, but
//     32 atomics on one address per word.
#ifndef RP_OCCLUSION_COMMIT
#define RP_OCCLUSION_COMMIT 1
#endif

// launch bounds as for the shadow-ray kernels of a frame (kernels.h rp_k_connect): the budget of RP_CONNECT_WAVES for scenes with one
// instance record, RP_TRAVERSE_WAVES for the two-level walk; the cutout instantiations, which carry the material and texture lookup of the
// alpha test through the walk, get the budget of the alpha-tested first extend of a radiance-query run (RP_QUERY_ALPHA_EXTEND_WAVES)
template <bool ALPHA, bool SINGLE>
__global__ __launch_bounds__(RP_TRAVERSE_BLOCK, (ALPHA ? RP_QUERY_ALPHA_EXTEND_WAVES : (SINGLE ? RP_CONNECT_WAVES : RP_TRAVERSE_WAVES))) void rp_k_trace_occlusion(
    RpScene sc, const RptrRenderRayQuery *queries, uint32_t n, uint32_t *bits, float alpha_cutoff, uint32_t *cursor, int *gstack) {
    uint32_t nn = 0, nt = 0;
    auto load = [&](uint32_t i, V3 &ro, V3 &rd, float &tmin, float &tmax) -> bool {
        const float4 *qp = reinterpret_cast<const float4 *>(queries + i);
        const float4 q0 = qp[0], q1 = qp[1];
        ro = v3(q0.x, q0.y, q0.z);
        rd = v3(q1.x, q1.y, q1.z);
        tmin = RPTR_RAY_EPSILON * len3(ro);             // the RQ_CLOSEST rule (kernels_misc.h rp_k_trace)
        tmax = __float_as_int(q0.w) < 0 ? -1.0f : q1.w; // mode < 0: skipped query, empty interval
        return true;
    };
    auto done = [&](uint32_t i, const RpHitRec &h) {
        const bool skip = queries[i].mode_or_data < 0; // the bit stays the caller's
        const bool hit = h.inst_idx >= 0;
#if RP_OCCLUSION_COMMIT == 0
        if (skip) return;
        uint32_t *word = bits + (i >> 5);
        const uint32_t bit = 1u << (i & 31u);
        if (hit)
            (void)__hip_atomic_fetch_or(word, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            (void)__hip_atomic_fetch_and(word, ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
        // (the lanes retired by this refill are the active ones: the ballots see nobody else)
        const uint32_t w = i >> 5, key = (i & 31u) | (hit ? 32u : 0u);
        const uint32_t lane = rp_lane_id();
        unsigned long long todo = __ballot(!skip);
        while (todo != 0ull) {
            const int leader = __ffsll(todo) - 1;
            const uint32_t lw = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
            const unsigned long long same = __ballot(!skip && w == lw);
            uint32_t set = 0u, all = 0u;
            if (__ballot(!skip && w == lw && (i & 31u) != (lane & 31u)) == 0ull) { // bit index == lane index modulo 32: no two lanes of the group collide
                const unsigned long long hits = __ballot(!skip && w == lw && hit);
                all = (uint32_t)same | (uint32_t)(same >> 32);
                set = (uint32_t)hits | (uint32_t)(hits >> 32);
            } else
                for (unsigned long long m = same; m != 0ull; m &= m - 1ull) {
                    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll(m) - 1);
                    const uint32_t b = 1u << (k & 31u);
                    all |= b;
                    set |= (k & 32u) ? b : 0u;
                }
            if (lane == (uint32_t)leader) {
                if (all == ~0u) // the whole word at once: nobody's bit to keep, and nothing of this word was or will be written by another step
                    bits[lw] = set;
                else if (set != 0u) (void)__hip_atomic_fetch_or(bits + lw, set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (all != ~0u && set != all) (void)__hip_atomic_fetch_and(bits + lw, ~(all & ~set), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            todo &= ~same;
        }
#endif
    };
    auto alpha = [&](uint32_t, int inst_idx, int, int geom, int prim, float u, float v) -> bool {
        return rp_alpha_below_cutoff(sc, inst_idx, geom, prim, u, v, alpha_cutoff);
    };
    if constexpr (ALPHA) // (one instantiation per kernel: each owns the LDS stacks)
        rp_wave_trace<true, false, RP_NODE_MIN_ANY, RP_REFILL_MIN_ANY, true, SINGLE>(sc, n, cursor, gstack, load, done, alpha, nn, nt);
    else
        rp_wave_trace<true, false, RP_NODE_MIN_ANY, RP_REFILL_MIN_ANY, false, SINGLE>(sc, n, cursor, gstack, load, done, RpNoAlpha(), nn, nt);
}
