// skin.h -- skinned meshes: bone matrices in, float positions and oct-encoded shading normals out (include/rptr_hip.h "skinned meshes").
//
// The reference animates "with a compute shader that writes the float vertex buffer" (render_vulkan.cpp:2834-2840) and ships the buffer,
// not the shader. rp_k_skin is that piece: linear blend skinning with up to four influences per UNROLLED vertex (three per triangle, the
// layout of SceneCopy::dynpos), from a rest pose the library keeps, into the master copy's dynpos and -- for geometries with normals --
// into dynnrm, the per-geometry array of skinned normal words. The refit carries the positions on as it always did (rp_k_refit_tris);
// rp_k_refit_normals, launched behind it for meshes that have such an array, carries the normal words into the shading records.
//
// Arithmetic: binary32, every product and sum rounded on its own (the library is built -ffp-contract=off; the temporaries below keep the
// association explicit whatever the flags), division and square root in their IEEE forms (dmath.h; this translation unit is built with
// RP_FAST_MATH = 0). tests/skin_ref.py states the same operations in numpy float32, and the tests compare bit for bit.
//   w_k     = float(weight[k]) / 65535.0f
//   B[r][c] = ((w0 M0[r][c] + w1 M1[r][c]) + w2 M2[r][c]) + w3 M3[r][c]
//   p'[r]   = (B[r][0] x + B[r][1] y) + (B[r][2] z + B[r][3])                    (the placement rule of rp_k_place_lights)
//   n'      = cof(A) n, A the 3x3 part of B, rows of cof(A): cross(A1, A2), cross(A2, A0), cross(A0, A1); negated when det A = A0 . C0 < 0
//   word    = quantize_normal(n') (librender/quantize.h:21-35: it divides by the L1 norm, so nothing is normalised first)
// cof(A) = det(A) inverse-transpose(A): the direction of the inverse-transpose normal without a division, and the sign flip undoes the
// factor det(A) of a mirroring bone. Always from the rest pose, never from the previous output: nothing drifts.
#pragma once
#include "dshade.h"

// the 16-byte record of include/rptr_hip.h as the kernel loads it: one uint4
//   x = bone[0] | bone[1] << 16, y = bone[2] | bone[3] << 16, z = weight[0] | weight[1] << 16, w = weight[2] | weight[3] << 16
static_assert(sizeof(RptrSkinVertex) == 16, "RptrSkinVertex is loaded as one uint4");

// librender/quantize.h:21-35 (scenes.quantize_normals restates it): n must be finite and not all zero
RP_DEV uint32_t rp_quantize_normal(V3 n) {
    const float nl1 = (fabsf(n.x) + fabsf(n.y)) + fabsf(n.z);
    float px = n.x / nl1, py = n.y / nl1;
    if (n.z <= 0.0f) {
        const float fx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float fy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = fx, py = fy;
    }
    px = px * 32768.0f, py = py * 32768.0f;
    const int ix = min(max(int(px), -0x7FFF), 0x7FFF), iy = min(max(int(py), -0x7FFF), 0x7FFF);
    return uint32_t(0x8000 + ix) | (uint32_t(0x8000 + iy) << 16);
}

// the compact rest normals of a geometry: the low halves of its qnrm_uv words (set_skin; also what dynnrm starts from)
__global__ __launch_bounds__(256) void rp_k_skin_rest_normals(const uint64_t *qnrm_uv, uint32_t *out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = uint32_t(qnrm_uv[i]);
}

// The steps of rp_k_skin as functions: rp_k_morph (morph.h) performs exactly these operations on a morphed rest pose.
// blended matrix of one skin record, B[4 r + c]
RP_DEV void rp_skin_blend(const uint4 s, const float4 *bones, float *B) {
    const uint32_t bone[4] = {s.x & 0xFFFFu, s.x >> 16, s.y & 0xFFFFu, s.y >> 16};
    const uint32_t wq[4] = {s.z & 0xFFFFu, s.z >> 16, s.w & 0xFFFFu, s.w >> 16};
    for (int k = 0; k < 4; ++k) {
        const float w = float(wq[k]) / 65535.0f;
        const float4 *m = bones + 3ull * min(bone[k], uint32_t(RPTR_MAX_BONES - 1)); // (set_skin checked the index: the clamp only guards the table)
        for (int r = 0; r < 3; ++r) {
            const float4 row = m[r];
            const float t[4] = {w * row.x, w * row.y, w * row.z, w * row.w};
            for (int c = 0; c < 4; ++c) B[4 * r + c] = k == 0 ? t[c] : B[4 * r + c] + t[c];
        }
    }
}
// cof(A) n, A the 3x3 part of B, negated under a mirroring blend
RP_DEV V3 rp_skin_normal(const float *B, const V3 n) {
    const V3 A0 = v3(B[0], B[1], B[2]), A1 = v3(B[4], B[5], B[6]), A2 = v3(B[8], B[9], B[10]);
    const V3 C0 = cross3(A1, A2), C1 = cross3(A2, A0), C2 = cross3(A0, A1);
    V3 q = v3(dot3(C0, n), dot3(C1, n), dot3(C2, n));
    if (dot3(A0, C0) < 0.0f) q = -q;
    return q;
}
// a normal the quantiser can take: finite and not all zero (otherwise the previous word stays)
RP_DEV bool rp_skin_normal_usable(const V3 q) {
    return isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && !(q.x == 0.0f && q.y == 0.0f && q.z == 0.0f);
}

// One lane per unrolled vertex. Loads: 16 bytes of skin record, 12 of rest position, 4 of rest normal word, and three float4 per bone
// (lanes of a wave share few bones: cache hits); stores: 12 + 4 bytes. rest_nrm / out_nrm NULL: a geometry without normals.
// A vertex whose new position is not finite keeps position and normal and is counted in *rejected; a normal that is not finite or all
// zero keeps its previous word.
__global__ __launch_bounds__(256) void rp_k_skin(const uint4 *skin, const float *rest_pos, const uint32_t *rest_nrm, const float4 *bones, uint32_t n, float *out_pos,
                                                 uint32_t *out_nrm, uint32_t *rejected) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float B[12];
        rp_skin_blend(skin[i], bones, B);
        const float x = rest_pos[3ull * i], y = rest_pos[3ull * i + 1], z = rest_pos[3ull * i + 2];
        float p[3];
        for (int r = 0; r < 3; ++r) p[r] = rp_place_coord(B + 4 * r, x, y, z);
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
            atomicAdd(rejected, 1u);
            continue;
        }
        out_pos[3ull * i] = p[0], out_pos[3ull * i + 1] = p[1], out_pos[3ull * i + 2] = p[2];
        if (!out_nrm) continue;
        const V3 q = rp_skin_normal(B, rp_dequantize_normal(rest_nrm[i]));
        if (!rp_skin_normal_usable(q)) continue;
        out_nrm[i] = rp_quantize_normal(q);
    }
}

// The skinned normal words into the shading records of BVH triangles [begin, begin + count) of one mesh: the low halves of qnu[0 / 2 / 4]
// (the uv halves stay). geom_nrm: per geometry of the mesh its dynnrm array, or NULL (never bound, or no normals: the record keeps what
// rp_make_shade_tri read from the qnrm_uv stream). Launched behind rp_k_refit_tris and behind the rp_k_build_shade_tris of a device rebuild.
__global__ __launch_bounds__(256) void rp_k_refit_normals(const RptrBvhTri *tris, RpShadeTri *shade, uint32_t begin, uint32_t count, const uint32_t *const *geom_nrm) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const RptrBvhTri &t = tris[begin + i];
        const uint32_t *nw = geom_nrm[t.geom];
        if (!nw) continue;
        nw += 3ull * t.prim;
        uint32_t *q = shade[begin + i].qnu;
        q[0] = nw[0], q[2] = nw[1], q[4] = nw[2];
    }
}
