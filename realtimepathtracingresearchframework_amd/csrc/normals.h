// normals.h -- recomputed shading normals: float positions in, oct-encoded normal words out (include/rptr_hip.h "recomputed normals").
// The missing half of rptr_hip_update_vertices[_device]: a cloth, fluid or soft-body solver writes the float vertex buffer and nothing
// knows the normals of the new shape; morph targets authored without normal deltas leave the rest normal in place. rp_k_face_normals and
// rp_k_group_normals make area-weighted smooth normals from the master copy's CURRENT positions into SceneCopy::dynnrm, the array the
// skinner and the morph stage write; everything downstream (rp_k_refit_normals, frame contexts, readback_skinned) is theirs.
//
// Data: vertices are unrolled, so the host says which corners are one smooth vertex (rptr_hip_set_normal_groups: one label per corner).
// The library renumbers the labels densely by first occurrence -- every RPTR_NORMAL_GROUP_FLAT corner becomes a group of its own -- and
// transposes them on the host, once, into a CSR: offsets[groups + 1] and members[3 * triangles], a group's member corners in ASCENDING
// UNROLLED VERTEX INDEX (the pattern of morph.h's per-vertex list). The order of a group's sum is therefore fixed, nothing is accumulated
// with atomics and the result does not depend on how lanes are scheduled.
//
// Arithmetic: binary32, every product, difference and sum rounded on its own (-ffp-contract=off, RP_FAST_MATH = 0; the temporaries keep
// the association explicit). tests/normals_ref.py states the same operations in numpy float32, and the tests compare bit for bit.
//   triangle t, corners p0 p1 p2 = positions[3t .. 3t+2]:  e1 = p1 - p0,  e2 = p2 - p0
//     f = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x)          (area-weighted, never normalised)
//   group with members c_0 < c_1 < ...:  n = f(c_0 / 3);  n = n + f(c_k / 3) for k = 1, 2, ...   (left to right)
//   flip: n = -n;   word = rp_quantize_normal(n) unless n is not finite or all zero (every corner of the group keeps its previous word)
// A triangle with two corners in one group is a member twice and contributes twice; a zero-area triangle contributes zeros. Weighting
// is by area only (angle weighting is out of scope).
//
// Two launches per geometry. The fused form -- every member's face normal computed in place from its 36 bytes of positions -- does the
// subtractions and the cross product once per corner instead of once per triangle and replaces one aligned 16-byte load per member by
// nine 4-byte ones at a 36-byte stride; profiles/normals_notes.md has the figures of both.
#pragma once
#include "skin.h"

// One lane per triangle: loads 36 bytes, stores 16 (w = 0).
__global__ __launch_bounds__(256) void rp_k_face_normals(const float *pos, uint32_t num_tris, float4 *face) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < num_tris; t += gridDim.x * blockDim.x) {
        const float *p = pos + 9ull * t;
        const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
        const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
        const float a[3] = {e1y * e2z, e1z * e2x, e1x * e2y};
        const float b[3] = {e1z * e2y, e1x * e2z, e1y * e2x};
        face[t] = make_float4(a[0] - b[0], a[1] - b[1], a[2] - b[2], 0.0f);
    }
}

// One lane per group: loads 8 bytes of offsets (two neighbouring dwords), per member 4 bytes of corner index and 16 of face normal;
// stores 4 bytes per member. A group is summed once however many corners share it, and a lane whose sum is unusable stores nothing.
#ifndef RP_NORMALS_CHUNK
#define RP_NORMALS_CHUNK 4 // members fetched before the first of them is added (the fetch shape of rp_k_morph)
#endif
__global__ __launch_bounds__(256) void rp_k_group_normals(const uint32_t *offsets, const uint32_t *members, const float4 *face, uint32_t num_groups, uint32_t flip,
                                                          uint32_t *out_nrm) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < num_groups; g += gridDim.x * blockDim.x) {
        const uint32_t begin = offsets[g], end = offsets[g + 1]; // (end <= 3 * triangles < 2^32: e + k below cannot wrap in 64 bits)
        if (begin >= end) continue;                              // (the host makes no empty group: this only guards the clamp below)
        V3 n = v3(0.0f, 0.0f, 0.0f);
        // RP_NORMALS_CHUNK members are fetched, then their face normals, before the first is added. The loads past the end of the list
        // are clamped to its last member (a cache hit) and not added: a list of any length works and the sum's order is unchanged.
        for (uint64_t e = begin; e < end; e += RP_NORMALS_CHUNK) {
            uint32_t c[RP_NORMALS_CHUNK];
            float4 f[RP_NORMALS_CHUNK];
#pragma unroll
            for (int k = 0; k < RP_NORMALS_CHUNK; ++k) c[k] = members[min(e + (uint64_t)k, (uint64_t)end - 1)];
#pragma unroll
            for (int k = 0; k < RP_NORMALS_CHUNK; ++k) f[k] = face[c[k] / 3u];
#pragma unroll
            for (int k = 0; k < RP_NORMALS_CHUNK; ++k) {
                if (e + (uint64_t)k >= end) continue;
                if (e + (uint64_t)k == begin) n = v3(f[k].x, f[k].y, f[k].z); // n = f(c_0 / 3)
                else n.x = n.x + f[k].x, n.y = n.y + f[k].y, n.z = n.z + f[k].z;
            }
        }
        if (flip) n = -n;
        if (!rp_skin_normal_usable(n)) continue;
        const uint32_t word = rp_quantize_normal(n);
        for (uint32_t e = begin; e < end; ++e) out_nrm[members[e]] = word;
    }
}
