// tlas_build.h -- moving instances: new transforms in the instance records, and the device-side rebuild of the top level.
//
// Stands in for what the reference does per frame with its instance list: default_update_tlas (vulkan/render_vulkan.cpp:1219-1321) makes
// a new top-level structure and builds it; request_tlas_operation(Rebuild | Refit) (:1323-1354) picks between a build and an update
// -> rptr_hip_set_tlas_policy.
//
// rptr_hip_update_instances stages transforms in a table (per scene instance: object_to_world, world_to_object); the next refit of a
// scene copy then
//   1. writes them into the copy's instance records (one thread per record: the up to `braid` records of an instance and, in a
//      flattened scene, the instance's own record behind the top-level ones all carry instance_id),
//   2. bounds every top-level record from its sub-root's box (rp_k_refit_instances, as for a deformed mesh),
//   3. RPTR_TLAS_REFIT: refits the top level on its topology; RPTR_TLAS_REBUILD: builds a new one over the record boxes with the
//      kernels of lbvh.h -- centroid bounds, Morton keys, radix sort, Karras hierarchy, 4-wide collapse with ONE record per leaf,
//      level lists -- and gives it boxes and encoding through the refit (rp_refit_node + rp_bvh4_encode). The records are NOT
//      permuted: a leaf names its record through the index bits of its sorted key (RpLbvhLeaves.named), so the record array a host
//      exports keeps the order set_scene gave it. The root stays node 0; the nodes live in [0, capacity) in front of every
//      bottom-level tree, capacity reserved by set_scene (host_bvh.inl).
// No step synchronises threads through memory inside a kernel (lbvh.h says why).
//
// Stack safety: the keys of a top-level build are RP_TLAS_AXIS_BITS bits per axis + the index bits, so the binary radix tree is at
// most that deep, the 4-wide tree half of it, and a traversal needs at most 3 stack entries per 4-wide level (and never more than
// records - 1). set_scene adds that bound to the bottom-level need and refuses the scene when the sum exceeds the traversal stack
// (rp_tlas_stack_bound below is the one statement of it, used by host_bvh.inl).
#pragma once
#include <algorithm>

#define RP_TLAS_AXIS_BITS 10 // Morton bits per axis of a top-level build: 1024^3 cells over the centroid bounds of the records

// worst-case traversal stack entries of ANY top level rp_tlas_rebuild can make over n records
static inline int rp_tlas_stack_bound(size_t n_records) {
    if (n_records < 2) return 0;
    int index_bits = 1;
    while ((1ull << index_bits) < (unsigned long long)n_records) ++index_bits;
    const int key_bits = 3 * std::min(RP_TLAS_AXIS_BITS, (64 - index_bits) / 3) + index_bits;
    const int levels4 = (key_bits - 1) / 2 + 1; // binary inner depths 0 .. key_bits - 1, 4-wide nodes at the even ones
    return (int)std::min<size_t>(n_records - 1, (size_t)3 * levels4);
}

// world_to_object of a row-major 3x4 object_to_world: host_state.h invert_affine operation for operation (cofactors in double, rounded
// once; the translation unit is compiled without contraction), so that a record written here equals the one set_scene makes bit for bit
RP_DEV void rp_invert_affine(const float m[12], float out[12]) {
    double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], hh = m[9], i = m[10];
    double A = e * i - f * hh, B = -(d * i - f * g), C = d * hh - e * g;
    double det = a * A + b * B + c * C;
    double id = 1.0 / det;
    double r[9] = {A * id, -(b * i - c * hh) * id, (b * f - c * e) * id, B * id, (a * i - c * g) * id, -(a * f - c * d) * id,
                   C * id, -(a * hh - b * g) * id, (a * e - b * d) * id};
    double tx = m[3], ty = m[7], tz = m[11];
    for (int k = 0; k < 3; ++k) {
        out[4 * k + 0] = (float)r[3 * k + 0];
        out[4 * k + 1] = (float)r[3 * k + 1];
        out[4 * k + 2] = (float)r[3 * k + 2];
        out[4 * k + 3] = (float)(-(r[3 * k + 0] * tx + r[3 * k + 1] * ty + r[3 * k + 2] * tz));
    }
}

// staging of a DEVICE-source update: rows [first, first + count) of the table (24 floats per instance: object_to_world, world_to_object)
// from `count` 3x4 matrices. A matrix that is not finite or has det == 0 (what the host-source call rejects) leaves its row as it was
// and is counted in *rejected (rptr_hip_get_option "instance_updates_rejected").
__global__ __launch_bounds__(256) void rp_k_stage_instance_transforms(const float *src12, uint32_t first, uint32_t count, float *table24, uint32_t *rejected) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        float m[12], inv[12];
        bool ok = true;
        for (int k = 0; k < 12; ++k) {
            m[k] = src12[12ull * i + k];
            ok = ok && isfinite(m[k]);
        }
        rp_invert_affine(m, inv);
        for (int k = 0; k < 12; ++k) ok = ok && isfinite(inv[k]); // (det == 0: 1 / det is infinite)
        if (!ok) {
            atomicAdd(rejected, 1u);
            continue;
        }
        float *row = table24 + 24ull * (first + i);
        for (int k = 0; k < 12; ++k) {
            row[k] = m[k];
            row[12 + k] = inv[k];
        }
    }
}

// the reserved top-level nodes as set_scene leaves the ones its tree does not use: empty and unreachable. A build starts from them, so
// that what lies behind the nodes of the new tree does not depend on the trees before it (the export is a function of the records)
__global__ __launch_bounds__(256) void rp_k_tlas_clear(RptrBvh4Node *nodes, float *node_box, uint32_t capacity) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < capacity; i += gridDim.x * blockDim.x) {
        RptrBvh4Node nd;
        __builtin_memset(&nd, 0, sizeof(nd));
        for (int k = 0; k < 4; ++k) nd.child[k] = RPTR_BVH4_EMPTY;
        nodes[i] = nd;
        for (int k = 0; k < 6; ++k) node_box[6ull * i + k] = 0.0f;
    }
}

// 1. the staged transforms into the instance records: one thread per record (top-level records AND a flattened scene's own records).
// The row of an instance nobody moved holds what set_scene put into its records: rewriting it changes nothing.
__global__ __launch_bounds__(256) void rp_k_update_instance_records(RptrBvhInstance *insts, uint32_t n_records, const float *table24, uint32_t n_instances) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_records; i += gridDim.x * blockDim.x) {
        const int id = insts[i].instance_id;
        if (id < 0 || (uint32_t)id >= n_instances) continue; // (the flat tree's identity record)
        const float *row = table24 + 24ull * (uint32_t)id;
        for (int k = 0; k < 12; ++k) {
            insts[i].object_to_world[k] = row[k];
            insts[i].world_to_object[k] = row[12 + k];
        }
    }
}

// 4. moving lights (rptr_hip_set_light_sources): the world-space vertices of every light from where its triangle is NOW -- the staged
// object_to_world of its instance applied to the object-space vertices, which are the registered ones for a static mesh and the copy's
// float positions (geom_dyn[geometry], 9 floats per triangle in unrolled order, NULL for a static geometry) for a deforming one. A
// device-side rebuild of the mesh's tree reorders the copy's TRIANGLES, never these positions, so `triangle` stays valid. One thread
// per light; only the 36 bytes of vertices of lights[i], i < n, are written: radiance stays, and so does the zeroed bin behind the
// array. The association is the one of collect_emitters (librender/lights.cpp:52-56, glm's mat4 * vec4), (m0 x + m1 y) + (m2 z + m3),
// every product and sum rounded to float (the translation unit is built without contraction; the temporaries below keep the
// association explicit whatever the flags), so a light placed with the transform set_scene received equals the host's bit for bit.
// Always from the object-space source, never from the previous placement: nothing drifts however many updates there were.
RP_DEV float rp_place_coord(const float *row, float x, float y, float z) {
    const float a = row[0] * x, b = row[1] * y, c = row[2] * z;
    const float ab = a + b, cd = c + row[3];
    return ab + cd;
}
__global__ __launch_bounds__(256) void rp_k_place_lights(RptrTriLightData *lights, const RptrLightSource *sources, uint32_t n, const float *table24,
                                                         const float *const *geom_dyn) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const RptrLightSource s = sources[i];
        float p[9];
        const float *dyn = geom_dyn[s.geometry];
        if (dyn)
            for (int k = 0; k < 9; ++k) p[k] = dyn[9ull * s.triangle + k];
        else
            for (int k = 0; k < 3; ++k) p[k] = s.v0[k], p[3 + k] = s.v1[k], p[6 + k] = s.v2[k];
        const float *m = table24 + 24ull * s.instance;
        float *out = lights[i].v0; // v0, v1, v2 lie back to back: 9 floats
        for (int v = 0; v < 3; ++v)
            for (int r = 0; r < 3; ++r) out[3 * v + r] = rp_place_coord(m + 4 * r, p[3 * v], p[3 * v + 1], p[3 * v + 2]);
    }
}
