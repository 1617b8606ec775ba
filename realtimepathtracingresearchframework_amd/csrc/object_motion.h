// object_motion.h -- object motion vectors (include/rptr_hip.h rptr_hip_object_motion): a pass over a FINISHED frame that rewrites the .xy
// half of its motion + jitter AOV texels where the pixel's representative ray hits a surface that moved since the previous frame. A frame
// itself projects the SAME world point through the previous and the current view (dshade.h rp_store_geometry_aovs, motion_vector = 0 as
// the reference); here the previous view gets the point where the surface WAS. Two launches per call, the shape of surface_query.h:
// rp_k_trace_pixels, a traversal of the rp_k_trace family whose `load` makes the ray of its pixel from the frame constants (no query
// buffer) and whose `done` keeps the raw hit in the 32-byte scratch record, and rp_k_object_motion, one thread per pixel slot, which
// decides from the staged transform rows and the changed-geometry marks whether the hit moved and stores the one word.
// Neither kernel synchronises threads through memory; nothing a frame launches is touched.
// Included by rptr_hip.hip only (one definition per kernel; compiled with the IEEE build of the arithmetic, dmath.h RP_FAST_MATH 0).
#pragma once
#include "surface_query.h"

// what the snapshot of the previous frame's state looks like on the device (host_state.h rptr_hip::ObjectMotion)
struct RpObjectMotionTables {
    const float *inst_xf;          // per scene instance 24 floats: object_to_world, world_to_object as the last refit applied them
    const float *prev_inst_xf;     // ... and as the previous frame saw them
    const uint32_t *record_geom;   // per geometry record (instance.geometry_base + triangle.geom): the global geometry it is about
    const uint32_t *geom_changed;  // per global geometry: != 0 when its positions were updated between the two frames
    const float *const *prev_pos;  // per global geometry: its previous float positions (9 per triangle, unrolled), NULL for a static one
    uint32_t num_instances;
    uint32_t any_geom_changed;     // some entry of geom_changed is set
};

// The representative ray of the pixel behind tiled slot `slot` (dshade.h rp_slot_to_local: a wave's 64 lanes are an 8 x 8 tile): kernels.h
// rp_primary_ray_ex with the pixel-filter draw replaced by its mean and no lens. `f` holds the constants of the frame the AOV images belong
// to: ONE frame (after a launch sequence of several the host launches nothing), so cam_* is its camera. world_size 1: local rows are
// frame rows.
RP_DEV void rp_representative_ray_of_pixel(const RpFrame &f, int lx, int ly, V3 &origin, V3 &dir) {
    V2 point = v2(float(lx) + 0.5f, float(ly) + 0.5f);
    point = v2(point.x / float(f.width), point.y / float(f.height));
    if (f.rp.enable_raster_taa != 0) point = point + rp_screen_jitter(f, f.frame_offset, f.frame_id) * 0.5f;
    const V3 du = ld3(f.cam_du), dv = ld3(f.cam_dv), tl = ld3(f.cam_dir_top_left);
    origin = ld3(f.cam_pos);
    dir = norm3_ieee(point.x * du + point.y * dv + tl);
}
RP_DEV bool rp_representative_ray(const RpFrame &f, uint32_t slot, int &lx, int &ly, V3 &origin, V3 &dir) {
    lx = ly = 0;
    if (!rp_slot_to_local(f, slot, lx, ly)) return false;
    rp_representative_ray_of_pixel(f, lx, ly, origin, dir);
    return true;
}

// ------------------------------------------------------------------ traversal: opaque geometry, interval (0, inf), as ray queries
template <bool SINGLE>
__global__ RP_TRAVERSE_BOUNDS void rp_k_trace_pixels(RpScene sc, RpFrame f, RpRawHit *raw, uint32_t *cursor, int *gstack) {
    uint32_t nn = 0, nt = 0;
    auto load = [&](uint32_t i, V3 &ro, V3 &rd, float &tmin, float &tmax) -> bool {
        int lx, ly;
        tmin = 0.0f;
        tmax = __builtin_inff();
        return rp_representative_ray(f, i, lx, ly, ro, rd);
    };
    auto done = [&](uint32_t i, const RpHitRec &h) {
        float4 *rp = reinterpret_cast<float4 *>(raw + i);
        rp[0] = make_float4(h.t, h.u, h.v, __int_as_float(h.inst_idx));
        rp[1] = make_float4(__int_as_float(h.tri), 0.0f, 0.0f, 0.0f);
    };
    rp_wave_trace<false, false, RP_NODE_MIN, RP_REFILL_MIN, false, SINGLE>(sc, uint32_t(f.npix_padded), cursor, gstack, load, done, RpNoAlpha(), nn, nt);
}

// ------------------------------------------------------------------ decode: one thread per pixel slot (the raw hits are read in the order
// the traversal wrote them; a wave is an 8 x 8 tile, so its lanes mostly share one instance row). Slots of the tile padding hold no hit
// record and are skipped before anything is read. What a pixel does NOT need it does not pay for: a miss reads its raw hit and nothing
// else, an unmoved hit the instance's meta row and the two object_to_world rows, and only a pixel that is rewritten makes its ray again;
// the triangle record and the geometry tables are read only in a frame interval in which some geometry's positions changed
// (tb.any_geom_changed, a launch constant).
__global__ __launch_bounds__(256) void rp_k_object_motion(RpScene sc, RpFrame f, RpObjectMotionTables tb, const RpRawHit *raw, uint32_t *rewritten) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool write = false;
    uint32_t word = 0u;
    int lx = 0, ly = 0;
    if (i < uint32_t(f.npix_padded) && rp_slot_to_local(f, i, lx, ly)) {
        const float4 *rp = reinterpret_cast<const float4 *>(raw + i);
        const float4 hit4 = rp[0];
        const int hit_inst = __float_as_int(hit4.w);
        if (hit_inst >= 0) {
            const int4 meta = *(reinterpret_cast<const int4 *>(sc.insts + hit_inst) + 3); // blas_root, geometry_base, instance_id, flags
            if (meta.z >= 0 && uint32_t(meta.z) < tb.num_instances) {
                const float4 *cur = reinterpret_cast<const float4 *>(tb.inst_xf + 24ull * uint32_t(meta.z));
                const float4 *prv = reinterpret_cast<const float4 *>(tb.prev_inst_xf + 24ull * uint32_t(meta.z));
                const float4 p0 = prv[0], p1 = prv[1], p2 = prv[2];
                bool moved = false;
                for (int k = 0; k < 3; ++k) {
                    const float4 a = cur[k], b = k == 0 ? p0 : k == 1 ? p1 : p2;
                    moved = moved || __float_as_uint(a.x) != __float_as_uint(b.x) || __float_as_uint(a.y) != __float_as_uint(b.y) ||
                            __float_as_uint(a.z) != __float_as_uint(b.z) || __float_as_uint(a.w) != __float_as_uint(b.w);
                }
                const float *prev_tri = nullptr; // the triangle's previous positions when its geometry's were updated
                if (tb.any_geom_changed != 0u) {
                    const int *tr = reinterpret_cast<const int *>(sc.tris + uint32_t(__float_as_int(rp[1].x))); // prim, geom: words 9 and 10
                    const uint32_t g = tb.record_geom[meta.y + tr[10]];
                    if (tb.geom_changed[g] != 0u) prev_tri = tb.prev_pos[g] + 9ull * uint32_t(tr[9]);
                }
                if (moved || prev_tri) {
                    V3 ray_origin, ray_dir;
                    rp_representative_ray_of_pixel(f, lx, ly, ray_origin, ray_dir);
                    const V3 x_cur = ray_origin + hit4.x * ray_dir;
                    V3 p_obj;
                    if (prev_tri) { // the deformed surface: where the hit's barycentrics were on the previous positions
                        const float *q = prev_tri;
                        const V3 a = v3(q[0], q[1], q[2]), b = v3(q[3], q[4], q[5]), c = v3(q[6], q[7], q[8]);
                        p_obj = ((1.0f - hit4.y - hit4.z) * a + hit4.y * b) + hit4.z * c;
                    } else
                        p_obj = rp_xform_point(cur[3], cur[4], cur[5], x_cur);
                    const V3 x_prev = rp_xform_point(p0, p1, p2, p_obj);
                    float rx, ry, rw, cx, cy, cw; // dshade.h rp_store_geometry_aovs, the reference view on x_prev
                    rp_project(f.view_ref, f.proj_ref, x_prev, rx, ry, rw);
                    rp_project(f.view, f.proj, x_cur, cx, cy, cw);
                    const float rd = fmaxf(rw, 0.0f), cd = fmaxf(cw, 0.0f);
                    word = rp_half4(rx / rd - cx / cd, ry / rd - cy / cd, 0.0f, 0.0f).x;
                    write = true;
                }
            }
        }
    }
    if (write) reinterpret_cast<uint32_t *>(f.aov_motion_jitter)[2u * uint32_t(ly * f.width + lx)] = word; // the .xy word; the jitter word stays
    // the pixels this call rewrote: one atomic per wave
    const unsigned long long mask = __ballot(write);
    if (mask != 0ull && int(rp_lane_id()) == __ffsll((long long)mask) - 1) atomicAdd(rewritten, (uint32_t)__popcll(mask));
}
