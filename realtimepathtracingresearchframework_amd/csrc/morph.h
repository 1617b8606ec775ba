// morph.h -- morph targets (blend shapes): weights in, float positions and oct-encoded shading normals out (include/rptr_hip.h "morph
// targets"). The stage in front of the skinner (skin.h): it runs alone where a geometry has no skin, and with a skin it hands the morphed
// rest pose to exactly the operations of rp_k_skin. It shares the skinner's rest pose, output arrays (SceneCopy::dynpos / dynnrm),
// rejection rule and everything downstream.
//
// Data: rptr_hip_set_morph_targets transposes the sparse targets on the host, once, into a per-vertex CSR: offsets[n + 1], and entries
// sorted by (vertex, target). An entry is one float4 (dpos.xyz, the target index as bits) for a geometry without normals, two float4
// (the second: dnrm.xyz, 0) for one with normals. The order of a vertex's sum is therefore fixed -- ascending target index --, nothing is
// accumulated with atomics and the result does not depend on how lanes are scheduled.
//
// Arithmetic: binary32, every product and sum rounded on its own (-ffp-contract=off, RP_FAST_MATH = 0; the temporaries keep the
// association explicit). tests/morph_ref.py states the same operations in numpy float32, and the tests compare bit for bit.
//   p = rest_pos[i];  n = rp_dequantize_normal(rest_word[i])
//   for each entry (t, dpos, dnrm) of vertex i:  w = weight[t];  w == 0: the entry is skipped
//       p[c] = p[c] + w dpos[c];  n[c] = n[c] + w dnrm[c]
//   no skin: p' = p, q = n; when no entry was applied the word written is rest_word[i] itself (nothing is re-quantised)
//   skin:    B = blend, p' = place(B, p), q = cof(A) n with the sign rule (skin.h)
//   word = rp_quantize_normal(q) unless q is not finite or all zero (the previous word stays)
// All-zero weights therefore reproduce the rest pose bit for bit without a skin, and what rp_k_skin writes with one. Always from the
// rest pose, never from the previous output: nothing drifts.
#pragma once
#include "skin.h"

static_assert(sizeof(RptrMorphDelta) == 32, "RptrMorphDelta is 32 bytes");

// One lane per unrolled vertex. Loads: 8 bytes of offsets (two neighbouring dwords), 12 of rest position, 4 of rest normal word, 16 or
// 32 per entry as float4 and 4 of weight per entry (the table is small and shared by every lane: cache hits), with a skin what rp_k_skin
// loads; stores: 12 + 4 bytes. A vertex whose final position is not finite keeps position and normal and is counted in *rejected.
#ifndef RP_MORPH_CHUNK
#define RP_MORPH_CHUNK 4 // (measured against 1 and 8: profiles/morph_notes.md section 2)
#endif
template <bool SKIN, bool NORMALS>
__global__ __launch_bounds__(256) void rp_k_morph(const uint32_t *offsets, const float4 *entries, const float *weights, const uint4 *skin, const float *rest_pos,
                                                  const uint32_t *rest_nrm, const float4 *bones, uint32_t n, float *out_pos, uint32_t *out_nrm, uint32_t *rejected) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float p[3] = {rest_pos[3ull * i], rest_pos[3ull * i + 1], rest_pos[3ull * i + 2]};
        uint32_t word = 0;
        V3 nr = v3(0.0f, 0.0f, 0.0f);
        if (NORMALS) {
            word = rest_nrm[i];
            nr = rp_dequantize_normal(word);
        }
        bool applied = false;
        const uint64_t end = offsets[i + 1]; // (64-bit: e + k cannot wrap however close to 2^32 the entries come)
        // RP_MORPH_CHUNK entries are fetched before the first of them is applied: a lane's entries are contiguous (128 bytes hold four of
        // them with normals), its neighbour's lie a whole run away, so a line fetched for one entry must serve the next ones while it is
        // still in the vector L1 -- one entry per trip re-fetched every line up to four times (profiles/morph_notes.md section 2). The
        // loads past the end of the run are clamped to its last entry (a cache hit) and not applied; the sum's order is unchanged.
        for (uint64_t e = offsets[i]; e < end; e += RP_MORPH_CHUNK) {
            float4 a[RP_MORPH_CHUNK], b[RP_MORPH_CHUNK];
            float w[RP_MORPH_CHUNK];
#pragma unroll
            for (int k = 0; k < RP_MORPH_CHUNK; ++k) {
                const uint64_t ek = min(e + (uint64_t)k, end - 1);
                a[k] = entries[NORMALS ? 2 * ek : ek];
                if (NORMALS) b[k] = entries[2 * ek + 1];
            }
#pragma unroll
            for (int k = 0; k < RP_MORPH_CHUNK; ++k) w[k] = weights[__float_as_uint(a[k].w)];
#pragma unroll
            for (int k = 0; k < RP_MORPH_CHUNK; ++k) {
                if (e + (uint64_t)k >= end || w[k] == 0.0f) continue;
                applied = true;
                const float t[3] = {w[k] * a[k].x, w[k] * a[k].y, w[k] * a[k].z};
                p[0] = p[0] + t[0], p[1] = p[1] + t[1], p[2] = p[2] + t[2];
                if (NORMALS) {
                    const float u[3] = {w[k] * b[k].x, w[k] * b[k].y, w[k] * b[k].z};
                    nr.x = nr.x + u[0], nr.y = nr.y + u[1], nr.z = nr.z + u[2];
                }
            }
        }
        float B[12];
        if (SKIN) {
            rp_skin_blend(skin[i], bones, B);
            const float x = p[0], y = p[1], z = p[2];
            for (int r = 0; r < 3; ++r) p[r] = rp_place_coord(B + 4 * r, x, y, z);
        }
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
            atomicAdd(rejected, 1u);
            continue;
        }
        out_pos[3ull * i] = p[0], out_pos[3ull * i + 1] = p[1], out_pos[3ull * i + 2] = p[2];
        if (!NORMALS) continue;
        if (!SKIN && !applied) {
            out_nrm[i] = word;
            continue;
        }
        const V3 q = SKIN ? rp_skin_normal(B, nr) : nr;
        if (!rp_skin_normal_usable(q)) continue;
        out_nrm[i] = rp_quantize_normal(q);
    }
}
