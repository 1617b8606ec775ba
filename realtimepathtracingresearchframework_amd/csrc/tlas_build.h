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
