// surface_query.h -- surface queries (include/rptr_hip.h rptr_hip_trace_surface*): position, normals and material at a query ray's closest
// hit. Two launches per call: rp_k_trace_surface, a traversal of the rp_k_trace family that keeps the RAW hit (t, u, v, instance record, BVH
// triangle) in a 32-byte scratch record, and rp_k_surface<VARIANT, TEX>, one thread per query, which decodes it with the device functions
// the first shade of a frame uses (kernels.h rp_shade_body, stretch A) into the six 16-byte rows of an RptrSurfaceHit. The decode does not
// live in the traversal's `done`: with textures it needs the shade kernels' 120-odd VGPRs, the traversal kernels run at 77-96.
// Included by rptr_hip.hip only (one definition per kernel; compiled with the IEEE build of the shading arithmetic, dmath.h RP_FAST_MATH 0).
#pragma once
#include "kernels.h"

// the raw hit of one query: two 16-byte rows
struct alignas(16) RpRawHit {
    float t, u, v;
    int inst_idx; // index into RpScene::insts, -1 = miss
    int tri;      // index into RpScene::tris / RpScene::shade
    int _pad[3];
};
static_assert(sizeof(RpRawHit) == 32, "two 16-byte rows per query");
static_assert(sizeof(RptrSurfaceHit) == 96, "six 16-byte rows per query");

// what the decode needs of a frame's constants: the image-plane axes of the camera (host_frame.inl compute_view), the handle's frame size
// and RenderParams.pixel_radius for the first-hit footprint (pt_megakernel.glsl:341-352), SceneParams.normal_z_scale for the normal map
struct RpSurfaceFrame {
    float cam_du[3];
    int32_t width;
    float cam_dv[3];
    int32_t height;
    float pixel_radius;
    float normal_z_scale;
};

// ------------------------------------------------------------------ traversal: the interval is (0, t_max) as a rule of the instantiation
// (radiance queries: kernels.h rp_extend_body QUERY); records with mode_or_data < 0 get an empty interval and store nothing
template <bool SINGLE>
__global__ RP_TRAVERSE_BOUNDS void rp_k_trace_surface(RpScene sc, const RptrRenderRayQuery *queries, uint32_t n, RpRawHit *raw, uint32_t *cursor, int *gstack) {
    uint32_t nn = 0, nt = 0;
    auto load = [&](uint32_t i, V3 &ro, V3 &rd, float &tmin, float &tmax) -> bool {
        const float4 *qp = reinterpret_cast<const float4 *>(queries + i);
        const float4 q0 = qp[0], q1 = qp[1];
        ro = v3(q0.x, q0.y, q0.z);
        rd = v3(q1.x, q1.y, q1.z);
        tmin = 0.0f;
        tmax = __float_as_int(q0.w) < 0 ? -1.0f : q1.w; // mode < 0: skipped query, empty interval
        return true;
    };
    auto done = [&](uint32_t i, const RpHitRec &h) {
        if (queries[i].mode_or_data < 0) return;
        float4 *rp = reinterpret_cast<float4 *>(raw + i);
        rp[0] = make_float4(h.t, h.u, h.v, __int_as_float(h.inst_idx));
        rp[1] = make_float4(__int_as_float(h.tri), 0.0f, 0.0f, 0.0f);
    };
    // ray queries see opaque geometry
    rp_wave_trace<false, false, RP_NODE_MIN, RP_REFILL_MIN, false, SINGLE>(sc, n, cursor, gstack, load, done, RpNoAlpha(), nn, nt);
}

// ------------------------------------------------------------------ decode: kernels.h rp_shade_body from "hit attributes" to rp_unpack_material,
// for bounce 0, total_t 0 and throughput 1, without the VOLUME rule that moves the interaction point to the ray origin
RP_DEV void rp_store_surface_hit(RptrSurfaceHit *out, V3 p, float t, V3 gn, int inst_geom, V3 nn, int prim, V3 base, float roughness, V3 emit, float ior, V2 uv,
                                 int material_id, float metallic) {
    float4 *o = reinterpret_cast<float4 *>(out);
    o[0] = f4(p, t);
    o[1] = f4(gn, __int_as_float(inst_geom));
    o[2] = f4(nn, __int_as_float(prim));
    o[3] = f4(base, roughness);
    o[4] = f4(emit, ior);
    o[5] = make_float4(uv.x, uv.y, __int_as_float(material_id), metallic);
}
template <int VARIANT, bool TEX>
__global__ __launch_bounds__(256) void rp_k_surface(RpScene sc, RpSurfaceFrame f, const RptrRenderRayQuery *queries, const RpRawHit *raw, uint32_t n, RptrSurfaceHit *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 *qp = reinterpret_cast<const float4 *>(queries + i);
        const float4 q0 = qp[0], q1 = qp[1];
        if (__float_as_int(q0.w) < 0) continue; // mode_or_data < 0: the record stays untouched
        const float4 *rp = reinterpret_cast<const float4 *>(raw + i);
        const float4 hit4 = rp[0];
        const int hit_inst = __float_as_int(hit4.w);
        if (hit_inst < 0) { // the miss texels of the AOV images (pt_megakernel.glsl:482-487): albedo 0, roughness 1, ior 1
            rp_store_surface_hit(out + i, v3s(0.0f), -1.0f, v3s(0.0f), -1, v3s(0.0f), -1, v3s(0.0f), 1.0f, v3s(0.0f), 1.0f, v2(0.0f, 0.0f), -1, 0.0f);
            continue;
        }
        const uint32_t tri_index = uint32_t(__float_as_int(rp[1].x));
        const V3 ray_origin = xyz(q0), ray_dir = xyz(q1);
        // ---- hit attributes, pt_megakernel.glsl:495-572
        const float4 *sp = reinterpret_cast<const float4 *>(sc.shade + tri_index);
        const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
        const float4 *ip = reinterpret_cast<const float4 *>(sc.insts + hit_inst);
        const float4 r0 = ip[0], r1 = ip[1], r2 = ip[2];
        const int4 meta = *reinterpret_cast<const int4 *>(ip + 3);
        const int *tr = reinterpret_cast<const int *>(sc.tris + tri_index); // prim, geom: words 9 and 10 of the triangle record
        const int prim = tr[9], geom = tr[10];
        const uint32_t mword = __float_as_uint(s3.w);
        int material_id = int(mword & RP_SHADE_MATERIAL_MASK);
        if (meta.w & RP_INST_OWN_MATERIALS) material_id = rp_hit_material_id(sc.geoms[meta.y + geom], uint32_t(prim));
        const RptrBaseMaterial mp = sc.materials[material_id];
        const M3 n2w{v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z), v3(r2.x, r2.y, r2.z)};
        const uint64_t qa = uint64_t(__float_as_uint(s2.y)) | (uint64_t(__float_as_uint(s2.z)) << 32), qb = uint64_t(__float_as_uint(s2.w)) | (uint64_t(__float_as_uint(s3.x)) << 32),
                       qc = uint64_t(__float_as_uint(s3.y)) | (uint64_t(__float_as_uint(s3.z)) << 32);
        RpHit hit = rp_calc_hit_attributes(v3(s0.x, s0.y, s0.z), v3(s0.w, s1.x, s1.y), v3(s1.z, s1.w, s2.x), qa, qb, qc, (mword & RP_SHADE_HAS_NORMALS) != 0u,
                                           (mword & RP_SHADE_HAS_UVS) != 0u, material_id, hit4.x, hit4.y, hit4.z, n2w);
        hit.geo_normal = hit.geo_normal / len3(hit.geo_normal); // :578-580
        // :582-606, with the first-hit footprint of the camera's image-plane axes (:341-351)
        RpTexCoord tc = rp_texcoord(hit.uv);
        if (TEX) {
            const V3 dpdx = (ld3(f.cam_du) / float(f.width)) * f.pixel_radius, dpdy = (ld3(f.cam_dv) / float(f.height)) * f.pixel_radius;
            const M2 tex_fp = rp_dpdxy_to_footprint(ray_dir, dpdx, dpdy);
            tc = rp_hit_texcoord(hit.uv, tex_fp, ray_dir, hit.geo_normal, hit.tangent, hit.bitangent_l, hit.dist);
        }
        const V3 w_o = -ray_dir;
        const V3 ip_p = ray_origin + hit.dist * ray_dir;
        V3 gn = hit.geo_normal, nn = hit.normal;
        // (:624-668 below are the statements of kernels.h rp_shade_body, kept in step by hand: see the note there)
        // :624-633 (the VOLUME rule moves the megakernel's interaction point, not the surface: neither normal is flipped for it)
        if (dot3(w_o, gn) < 0.0f && (mp.flags & (RPTR_BASE_MATERIAL_VOLUME | RPTR_BASE_MATERIAL_ONESIDED)) == 0) {
            nn = -nn;
            gn = -gn;
        }
        // :634-654 normal mapping, bounce 0
        if (TEX && mp.normal_map != -1) {
            V3 t_y = norm3(cross3(hit.normal, hit.tangent));
            V3 t_x = cross3(t_y, hit.normal);
            t_x = t_x * len3(hit.tangent);
            t_y = t_y * hit.bitangent_l;
            const float4 tx = rp_texture_lod(sc, mp.normal_map, hit.uv, 0.0f); // :642-648
            V3 map_nrm = v3(2.0f * tx.x - 1.0f, 2.0f * tx.y - 1.0f, 1.0f * tx.z - 0.0f);
            map_nrm.z = rp_fsqrt(fmaxf(1.0f - map_nrm.x * map_nrm.x - map_nrm.y * map_nrm.y, 0.0f));
            const V3 t_z = f.normal_z_scale * nn;
            nn = norm3((t_x * map_nrm.x + t_y * map_nrm.y) + t_z * map_nrm.z);
        }
        // :656-668
        {
            const float nw = dot3(w_o, nn);
            const float gnw = dot3(w_o, gn);
            if (nw * gnw <= 0.0f) {
                const float blend = rp_fdiv(gnw, gnw - nw);
                nn = norm3(mix3(gn, nn, blend - RP_EPSILON));
            }
        }
        // ---- shade_base_material.glsl:14-31: the material at the hit
        RpMaterial mat;
        V3 emit;
        rp_unpack_material<VARIANT, TEX>(sc, mat, emit, mp, tc);
        rp_store_surface_hit(out + i, ip_p, hit.dist, gn, meta.y + geom, nn, prim, mat.base_color, mat.roughness, emit, mat.ior, hit.uv, material_id, mat.metallic);
    }
}
