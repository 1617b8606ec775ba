// host_scene.inl -- rptr_hip_set_scene (static uploads, tree, refit tables, then every scene copy -- the master's and the frame contexts' --
// through scene_copy_build), vertex and instance updates, refit and the device rebuilds (one front half: lbvh_front_half)
// Part of the ONE translation unit rptr_hip.hip (included there, in this order: host_state.h, host_bvh.inl, host_scene.inl,
// host_frame.inl, host_access.inl, host_queries.inl, host_comm.h): the host runtime split along its seams; no symbol changed.
// ---- set_scene, step by step (each returns RPTR_OK or the error it reported through fail())
// what the reference host rejects or this build does not cover yet; sets uses_textures / uses_alpha
static int scene_validate(rptr_hip *h, const RptrSceneDesc *s) {
    {
        const std::string bad = validate_scene_tables(s);
        if (!bad.empty()) return fail(h, RPTR_E_INVALID, "%s", bad.c_str());
    }
    if (s->num_textures && !s->textures) return fail(h, RPTR_E_INVALID, "num_textures = %u but textures is NULL", s->num_textures);
    for (uint32_t t = 0; t < s->num_textures; ++t) {
        if (!s->textures[t].rgba8 || s->textures[t].width == 0 || s->textures[t].height == 0 || s->textures[t].width > 16384 || s->textures[t].height > 16384)
            return fail(h, RPTR_E_INVALID, "texture %u: bad size or NULL data", t);
        if (s->textures[t].mip_levels > 1u) { // at most the full chain down to 1 x 1
            uint32_t full = 1;
            for (uint32_t w = s->textures[t].width, hh = s->textures[t].height; w > 1 || hh > 1; w = std::max(1u, w / 2), hh = std::max(1u, hh / 2)) ++full;
            if (s->textures[t].mip_levels > full)
                return fail(h, RPTR_E_INVALID, "texture %u: %u mip levels, a %u x %u texture has at most %u", t, s->textures[t].mip_levels, s->textures[t].width,
                            s->textures[t].height, full);
        }
    }
    h->uses_textures = false;
    h->uses_alpha = false;
    h->tail_adaptive = 1 << 30; // the first frame of a scene shows the queue lengths of every bounce
    for (uint32_t m = 0; m < s->num_materials; ++m) {
        const RptrBaseMaterial &mat = s->materials[m];
        if (mat.normal_map != -1) h->uses_textures = true;
        if (mat.normal_map != -1 && (mat.normal_map < 0 || (uint32_t)mat.normal_map >= s->num_textures))
            return fail(h, RPTR_E_INVALID, "material %u: normal_map %d is not a texture of this scene (%u textures)", m, mat.normal_map, s->num_textures);
        if ((mat.flags & RPTR_BASE_MATERIAL_NOALPHA) == 0) h->uses_alpha = true; // alpha test of hit candidates (kernels.h ALPHA)
        const float vals[5] = {mat.base_color[0], mat.roughness, mat.specular, mat.metallic, mat.ior};
        for (float v : vals) {
            uint32_t u;
            memcpy(&u, &v, 4);
            if (u & RPTR_TEXTURED_PARAM_MASK) h->uses_textures = true;
            if ((u & RPTR_TEXTURED_PARAM_MASK) && RPTR_TEXTURE_ID(u) >= s->num_textures)
                return fail(h, RPTR_E_INVALID, "material %u: textured parameter refers to texture %u of %u", m, RPTR_TEXTURE_ID(u), s->num_textures);
        }
    }
    return RPTR_OK;
}
// textures (RGBA8, mip levels back to back) + the sRGB decode table
static int scene_upload_textures(rptr_hip *h, const RptrSceneDesc *s, RpTexture *&d_textures, float *&d_srgb_lut) {
    int rc;
    d_textures = nullptr;
    d_srgb_lut = nullptr;
    // paths through a scene with textures carry their texture footprint (kernels.h TEX; the tail kernel's textured instantiation also serves
    // alpha-tested scenes)
    if ((h->uses_textures || h->uses_alpha) && h->path_capacity)
        for (FrameCtx &c : h->ctx)
            if (!c.ps.footprint && (rc = dev_alloc(h, &c.ps.footprint, h->path_capacity, nullptr))) return rc;
    h->tex = decltype(h->tex)(); // dynamic textures (texture_mips.h): the host's copy of the records, and which textures an emissive material reads
    h->tex.cap_texels.assign(s->num_textures, 0);
    h->tex.emissive.assign(s->num_textures, 0);
    for (uint32_t m = 0; m < s->num_materials; ++m) { // (scene_validate checked every index)
        const RptrBaseMaterial &mat = s->materials[m];
        if (!(mat.emission_intensity > 0.0f)) continue;
        if (mat.normal_map != -1) h->tex.emissive[(size_t)mat.normal_map] = 1;
        const float vals[5] = {mat.base_color[0], mat.roughness, mat.specular, mat.metallic, mat.ior};
        for (float v : vals) {
            uint32_t u;
            memcpy(&u, &v, 4);
            if (u & RPTR_TEXTURED_PARAM_MASK) h->tex.emissive[RPTR_TEXTURE_ID(u)] = 1;
        }
    }
    {
        std::vector<RpTexture> &tex = h->tex.records;
        tex.assign(s->num_textures, RpTexture{});
        for (uint32_t t = 0; t < s->num_textures; ++t) {
            const RptrTextureDesc &td = s->textures[t];
            uchar4 *dt = nullptr;
            const uint32_t levels = td.mip_levels > 1u ? td.mip_levels : 1u;
            size_t n = 0; // the levels back to back, level l = max(1, w >> l) x max(1, h >> l) (vulkan/resource_utils.cpp:86-100)
            for (uint32_t l = 0, w = td.width, hh = td.height; l < levels; ++l, w = std::max(1u, w / 2), hh = std::max(1u, hh / 2)) n += (size_t)w * hh;
            if ((rc = dev_upload(h, &dt, n, td.rgba8, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
            tex[t].texels = dt;
            tex[t].width = (int)td.width;
            tex[t].height = (int)td.height;
            tex[t].srgb = td.srgb ? 1 : 0;
            tex[t].levels = (int)levels;
            h->tex.cap_texels[t] = n;
        }
        if ((rc = dev_upload(h, &d_textures, tex.size(), tex.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
        h->tex.d_records = d_textures;
        float lut[256];
        rp_srgb_decode_lut(lut);
        if ((rc = dev_upload(h, &d_srgb_lut, 256, lut, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    }
    return RPTR_OK;
}
// the quantised vertex streams, one allocation per stream (the float positions of deforming meshes belong to the scene copies: scene_copy_build)
static int scene_upload_vertex_streams(rptr_hip *h, const RptrSceneDesc *s, std::vector<const uint64_t *> &d_qpos, std::vector<const uint64_t *> &d_qnu) {
    int rc;
    d_qpos.assign(s->num_geometries, nullptr);
    d_qnu.assign(s->num_geometries, nullptr);
    for (uint32_t g = 0; g < s->num_geometries; ++g) {
        const RptrGeometryDesc &gd = s->geometries[g];
        uint64_t *dp = nullptr;
        if ((rc = dev_upload(h, &dp, (size_t)gd.num_tris * 3, gd.qpos, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
        d_qpos[g] = dp;
        if (gd.qnrm_uv && (gd.has_normals || gd.has_uvs)) {
            uint64_t *dn = nullptr;
            if ((rc = dev_upload(h, &dn, (size_t)gd.num_tris * 3, gd.qnrm_uv, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
            d_qnu[g] = dn;
        }
    }
    h->geom_tris.assign(s->num_geometries, 0);
    h->geom_mesh.assign(s->num_geometries, -1);
    for (uint32_t m = 0; m < s->num_meshes; ++m)
        for (uint32_t j = 0; j < s->meshes[m].num_geometries; ++j) {
            h->geom_tris[s->meshes[m].first_geometry + j] = s->geometries[s->meshes[m].first_geometry + j].num_tris;
            h->geom_mesh[s->meshes[m].first_geometry + j] = (int)m;
        }
    return RPTR_OK;
}
// what set_scene works out on the host and every scene copy is made from
struct SceneTables {
    std::vector<RpGeomRecord> geoms;  // per (parameterized mesh, geometry); dyn_pos is left NULL: a copy's records point at ITS positions
    std::vector<uint32_t> geom_index; // ... and the global geometry each record is about
    std::vector<int> pmesh_base;      // per parameterized mesh: its first record
    std::vector<uint32_t> blas_list;  // scene_refit_tables: the node lists and depth levels of the dynamic meshes' trees
    std::vector<std::array<uint2, RP_REFIT_LEVELS>> levels;
};
// geometry records per (parameterized mesh, geometry): instanced_geometry[] (render_vulkan.cpp:2748-2850)
static int scene_geometry_records(rptr_hip *h, const RptrSceneDesc *s, const std::vector<const uint64_t *> &d_qpos, const std::vector<const uint64_t *> &d_qnu, SceneTables &T) {
    int rc;
    T.geoms.clear();
    T.geom_index.clear();
    T.pmesh_base.assign(s->num_parameterized_meshes, 0);
    for (uint32_t p = 0; p < s->num_parameterized_meshes; ++p) {
        const RptrParameterizedMeshDesc &pm = s->parameterized_meshes[p];
        const RptrMeshDesc &mesh = s->meshes[pm.mesh];
        T.pmesh_base[p] = (int)T.geoms.size();
        size_t total_tris = 0;
        for (uint32_t j = 0; j < mesh.num_geometries; ++j) total_tris += s->geometries[mesh.first_geometry + j].num_tris;
        uint8_t *d_ids = nullptr;
        if (pm.tri_material_ids && (rc = dev_upload(h, &d_ids, total_tris, pm.tri_material_ids, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
        size_t prim_offset = 0;
        for (uint32_t j = 0; j < mesh.num_geometries; ++j) {
            const uint32_t gi = mesh.first_geometry + j;
            const RptrGeometryDesc &gd = s->geometries[gi];
            RpGeomRecord r;
            memset(&r, 0, sizeof(r));
            r.qpos = d_qpos[gi];
            r.qnrm_uv = d_qnu[gi];
            r.mat_ids = d_ids ? d_ids + prim_offset : nullptr;
            memcpy(r.scaling, gd.quantized_scaling, 12);
            memcpy(r.offset, gd.quantized_offset, 12);
            r.material_id = d_ids ? -1 - pm.material_offsets[j] : pm.material_offsets[j];
            r.flags = (gd.has_normals && d_qnu[gi] ? RP_GEOM_HAS_NORMALS : 0u) | (gd.has_uvs && d_qnu[gi] ? RP_GEOM_HAS_UVS : 0u) |
                      (mesh.dynamic & kMeshDeforms ? RP_GEOM_DYNAMIC : 0u);
            T.geoms.push_back(r);
            T.geom_index.push_back(gi);
            prim_offset += gd.num_tris;
        }
    }
    return RPTR_OK;
}
// the acceleration structure: per-mesh trees (host binned SAH, or the device's PLOC builder for large static sets), top level, encoding
static int scene_build_acceleration_structure(rptr_hip *h, const RptrSceneDesc *s, std::vector<const uint64_t *> &d_qpos, std::vector<RpGeomRecord> &geoms, HostBvh &B) {
    {
        // large static triangle sets are built on the device (csrc/ploc.h) from the vertex streams uploaded above
        std::vector<uint8_t> mat_alpha(s->num_materials, 0);
        for (uint32_t i = 0; i < s->num_materials; ++i) mat_alpha[i] = (s->materials[i].flags & RPTR_BASE_MATERIAL_NOALPHA) == 0 ? 1 : 0;
        DeviceBuildCtx ctx;
        ctx.d_qpos = &d_qpos;
        ctx.geoms = &geoms;
        ctx.min_tris = (size_t)h->opt.v[OPT_DEVICE_BUILD_MIN_TRIS];
        int device_failures = 0;
        std::string device_failure;
        ctx.build = [&](const std::vector<RpBuildSegment> &segs, uint32_t n, DeviceTree &out) {
            const bool ok = device_build_tree(h, segs, n, mat_alpha, out);
            if (!ok) { // the host builder takes over (same scene, seconds instead of a fraction of one): say so, and do not leave the
                       // message behind as the "last error" of a call that succeeds
                ++device_failures;
                device_failure = h->last_error;
                h->last_error.clear();
            }
            return ok;
        };
        const auto t_build = std::chrono::steady_clock::now();
        build_host_bvh(s, B, h->opt, &ctx);
        if (device_failures && h->opt.v[OPT_QUIET] == 0)
            fprintf(stderr, "rptr_hip: note: %d device-side BVH build(s) failed (%s); the host builder built those trees instead\n", device_failures,
                    device_failure.c_str());
        h->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();
        h->bvh_device_built = B.device_built;
        h->bvh_device_ms = B.device_ms;
    }
    {
        const int capacity = RP_LDS_STACK + RPTR_BVH_STACK_DEPTH;
        if (B.stack_need > capacity)
            return fail(h, RPTR_E_UNSUPPORTED, "the acceleration structure of this scene needs a traversal stack of %d entries (limit %d)",
                        B.stack_need, capacity);
    }
    return RPTR_OK;
}
// refit tables. The top level by height (children before parents) is the same for every scene copy: worked out and uploaded here
// (d_refit_list, d_refit_levels, refit_top_all). The depth levels of every dynamic mesh's tree differ per copy once a copy is rebuilt:
// worked out here, left in T, uploaded per copy (scene_copy_refit_tables).
static int scene_refit_tables(rptr_hip *h, SceneTables &T) {
    std::vector<uint32_t> refit_list;
    T.blas_list.assign(h->h_nodes.size(), 0u);
    T.levels.assign(h->meshes.size(), std::array<uint2, RP_REFIT_LEVELS>());
    // (the bottom-level trees of dynamic meshes are refitted bottom-up with arrival counters, lbvh.h rp_k_refit_up: per node its parent and the
    // number of its inner children)
    h->refit_levels_tlas.clear();
    h->has_dynamic = false;
    for (const MeshRt &mr : h->meshes) h->has_dynamic = h->has_dynamic || mr.dynamic;
    // depth levels of every dynamic mesh's tree (slot RP_REFIT_LEVELS - 1 - depth: ascending slot = deepest first)
    {
        const size_t nn = h->h_nodes.size();
        std::vector<int> height(nn, -1);
        std::vector<std::vector<uint32_t>> tlas_levels;
        // iterative post-order: height = 1 + max(height of inner children), 0 for nodes with leaf children only
        std::vector<std::pair<int, int>> st{{0, 0}};
        while (!st.empty()) {
            auto [n, phase] = st.back();
            st.pop_back();
            const RptrBvh4Node &nd = h->h_nodes[n];
            if (phase == 0) {
                st.push_back({n, 1});
                for (int k = 0; k < 4; ++k)
                    if (nd.child[k] >= 0) st.push_back({nd.child[k], 0});
            } else {
                int hgt = 0;
                for (int k = 0; k < 4; ++k)
                    if (nd.child[k] >= 0) hgt = std::max(hgt, height[nd.child[k]] + 1);
                height[n] = hgt;
                if ((size_t)hgt >= tlas_levels.size()) tlas_levels.resize(hgt + 1);
                tlas_levels[hgt].push_back((uint32_t)n | 0x80000000u);
            }
        }
        for (auto &lv : tlas_levels) {
            h->refit_levels_tlas.push_back({(uint32_t)refit_list.size(), (uint32_t)(refit_list.size() + lv.size())});
            refit_list.insert(refit_list.end(), lv.begin(), lv.end());
        }
        for (size_t m = 0; m < h->meshes.size(); ++m) {
            const MeshRt &mr = h->meshes[m];
            for (auto &l : T.levels[m]) l = make_uint2((uint32_t)mr.node_base, (uint32_t)mr.node_base);
            if (!mr.dynamic) continue;
            std::vector<std::vector<uint32_t>> by_depth;
            std::vector<std::pair<int, int>> bfs{{h->mesh_root[m], 0}};
            for (size_t at = 0; at < bfs.size(); ++at) {
                const auto [n, d] = bfs[at];
                if ((size_t)d >= by_depth.size()) by_depth.resize((size_t)d + 1);
                by_depth[(size_t)d].push_back((uint32_t)n);
                for (int k = 0; k < 4; ++k)
                    if (h->h_nodes[(size_t)n].child[k] >= 0) bfs.push_back({h->h_nodes[(size_t)n].child[k], d + 1});
            }
            if (by_depth.size() > RP_REFIT_LEVELS) return fail(h, RPTR_E_UNSUPPORTED, "mesh %zu: a tree of %zu levels (limit %d)", m, by_depth.size(), RP_REFIT_LEVELS);
            uint32_t at = (uint32_t)mr.node_base;
            for (int slot = 0; slot < RP_REFIT_LEVELS; ++slot) {
                const int d = RP_REFIT_LEVELS - 1 - slot;
                const uint32_t cnt = (size_t)d < by_depth.size() ? (uint32_t)by_depth[(size_t)d].size() : 0u;
                T.levels[m][(size_t)slot] = make_uint2(at, at + cnt);
                for (uint32_t k = 0; k < cnt; ++k) T.blas_list[at + k] = by_depth[(size_t)d][k];
                at += cnt;
            }
        }
    }
    int rc;
    if ((rc = dev_upload(h, &h->d_refit_list, refit_list.size(), refit_list.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    // the instance bounds and the (small) top-level levels of a refit share one launch (kernels.h rp_k_refit_top): every level is one
    // more dependent launch otherwise, and an animated frame pays for them whatever its size
    const uint32_t small = 4096;
    std::vector<uint2> lv;
    for (auto &l : h->refit_levels_tlas) lv.push_back(make_uint2(l[0], l[1]));
    h->refit_top_all = (size_t)h->num_tlas_insts <= 4 * small; // (only the records the top level refers to have bounds: a flattened tree's triangles name the others)
    for (auto &l : h->refit_levels_tlas) h->refit_top_all = h->refit_top_all && l[1] - l[0] <= small;
    h->d_refit_levels = nullptr;
    if (!lv.empty() && (rc = dev_upload(h, &h->d_refit_levels, lv.size(), lv.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    return RPTR_OK;
}
// the traversal's scheduling thresholds and pool size for this scene's trees (RpScene.node_min / refill_min / fetch_max)
static void scene_traversal_preset(rptr_hip *h) {
    // Scheduling thresholds of the traversal (dtraverse.h): a wave refills its idle lanes together once `refill_min` of them have finished,
    // and leaves a node phase for a leaf phase once fewer than `node_min` lanes are at inner nodes. The defaults (48 / 10) were tuned on the
    // height field; in a dense soup of overlapping primitive boxes -- the forest: 26 node visits per ray, node-phase lane utilisation 0.55
    // instead of 0.67, a quarter of the lane slots waiting for a refill -- 32 / 16 are 5 % faster (C4 5.89 -> 5.61 ms) and 1.4 % slower on the
    // height field (profiles/r03_notes.md section 7). The choice follows the tree: the surface-area cost of its largest bottom-level tree
    // (sum of the inner children's box areas over the root's: 11 for the height field, 92 for the flattened forest). RPTR_TRAVERSE_PRESET=
    // "node_min,refill_min" overrides (0,0 = the compile-time defaults).
    {
        double best_cost = 0.0;
        size_t best_tris = 0;
        auto half_area = [&](size_t n) {
            const std::array<float, 6> &b = h->h_node_box[n];
            const double dx = std::max(0.0f, b[3] - b[0]), dy = std::max(0.0f, b[4] - b[1]), dz = std::max(0.0f, b[5] - b[2]);
            return dx * dy + dy * dz + dz * dx;
        };
        for (size_t m = 0; m < h->meshes.size(); ++m) {
            const MeshRt &mr = h->meshes[m];
            // (a mesh without a tree of its own is part of the flattened tree, which lies first: counted once, for mesh 0)
            const size_t root = (size_t)h->mesh_root[m], count = (size_t)(mr.node_count > 0 ? mr.node_count : (m == 0 ? (int)h->flat_nodes : 0));
            const size_t tris_m = mr.tri_count > 0 ? (size_t)mr.tri_count : (m == 0 ? h->flat_tris : 0);
            if (!count || tris_m < best_tris || root >= h->h_nodes.size()) continue;
            const double a0 = half_area(root);
            if (!(a0 > 0.0)) continue;
            double sum = 0.0;
            for (size_t n = root; n < std::min(root + count, h->h_nodes.size()); ++n)
                for (int k = 0; k < 4; ++k)
                    if (h->h_nodes[n].child[k] >= 0) sum += half_area((size_t)h->h_nodes[n].child[k]);
            best_cost = sum / a0;
            best_tris = tris_m;
        }
        // ... times the same measure of the top level (all child boxes of its nodes, instance boxes included, over the scene's box: 1 for a
        // single instance, ~ 6 for the forest's 1001 overlapping instances: the two-level forest gains the same 5 %, 8.38 -> 7.95 ms)
        double tlas_cost = 1.0;
        if (h->num_tlas_nodes > 0 && h->num_tlas_insts > 1) {
            const double a0 = half_area(0);
            double sum = 0.0;
            for (int n = 0; n < h->num_tlas_nodes; ++n) {
                const RptrBvh4Node &nd = h->h_nodes[(size_t)n];
                for (int k = 0; k < 4; ++k) {
                    if (nd.child[k] == RPTR_BVH4_EMPTY) continue;
                    double d[3];
                    for (int a = 0; a < 3; ++a) d[a] = std::max(0.0, (double)((int)nd.qhi[a][k] - (int)nd.qlo[a][k])) * std::ldexp(1.0, (int)nd.exp[a] - 127);
                    sum += d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
                }
            }
            if (a0 > 0.0) tlas_cost = std::max(1.0, sum / a0);
        }
        best_cost *= tlas_cost;
        h->bvh_area_cost = best_cost;
        int node_min = 0, refill_min = 0;
        if (best_cost >= 24.0) { // (height fields: 10-12; the small forests of the tests: 29-35; C4: 90 flattened, 250-280 two-level)
            node_min = 16;
            refill_min = 32;
        }
        if (h->opt.v[OPT_TRAVERSE_NODE_MIN] >= 0) { // options "traverse_node_min" / "traverse_refill_min" (0, 0: the compile-time defaults)
            node_min = (int)h->opt.v[OPT_TRAVERSE_NODE_MIN];
            refill_min = (int)std::max(0ll, h->opt.v[OPT_TRAVERSE_REFILL_MIN]);
        }
        h->master.dscene.node_min = std::max(0, std::min(64, node_min));
        h->master.dscene.refill_min = std::max(0, std::min(64, refill_min));
        h->master.dscene.lds_top = h->opt.v[OPT_LDS_TOP] != 0 ? 1 : 0;
        // ... and the size of a wave's pool of queue entries (dtraverse.h RP_FETCH: 256, four tiles of the first queue): 384 for the trees
        // of the default preset -- one frame at a time 1.82 -> 1.76 ms, two in flight 1.45 -> 1.38 on C2, pipelined unchanged --, 256 for dense
        // ones (the forest loses 4 % with 384; profiles/r05_notes.md section 19)
        h->master.dscene.fetch_max = h->opt.v[OPT_TRAVERSE_FETCH] > 0 ? (int)std::max(64ll, h->opt.v[OPT_TRAVERSE_FETCH] / 64 * 64) : (best_cost >= 24.0 ? 0 : 384);
    }
}
// level tables + node lists of the dynamic meshes + per-mesh node counts (one set per scene copy: copies are rebuilt independently)
static int scene_copy_refit_tables(rptr_hip *h, const SceneTables &T, SceneCopy &sc) {
    int rc;
    sc.device_built.assign(h->meshes.size(), 0);
    sc.built_epoch.assign(h->meshes.size(), 0);
    sc.scratch = RpLbvhScratch();
    sc.blas_list = nullptr;
    sc.blas_levels = nullptr;
    sc.mesh_count = nullptr;
    sc.host_levels = T.levels;
    sc.levels_known.assign(h->meshes.size(), 1);
    release_scene_copy_host(sc);
    sc.pinned_levels.assign(h->meshes.size(), nullptr);
    sc.ev_levels.assign(h->meshes.size(), nullptr);
    sc.inst_version = h->inst_version;
    sc.tlas_rebuilt = false;
    sc.tlas_list = nullptr;
    sc.tlas_levels = nullptr;
    sc.tlas_count = nullptr;
    if (h->tlas_capacity > 0) { // the level lists of a top level this copy builds itself (tlas_build.h)
        if ((rc = dev_alloc(h, &sc.tlas_list, (size_t)h->tlas_capacity, &h->scene_allocs))) return rc;
        if ((rc = dev_alloc(h, &sc.tlas_levels, RP_REFIT_LEVELS, &h->scene_allocs))) return rc;
        if ((rc = dev_alloc(h, &sc.tlas_count, 1, &h->scene_allocs))) return rc;
    }
    if (!h->has_dynamic) return RPTR_OK;
    std::vector<int> counts;
    for (const MeshRt &mr : h->meshes) counts.push_back(mr.node_count);
    if ((rc = dev_upload(h, &sc.blas_list, T.blas_list.size(), T.blas_list.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    if ((rc = dev_upload(h, &sc.blas_levels, T.levels.size() * RP_REFIT_LEVELS, T.levels.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    if ((rc = dev_upload(h, &sc.mesh_count, counts.size(), counts.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    for (size_t m = 0; m < h->meshes.size(); ++m)
        if (h->meshes[m].dynamic) {
            if (hipHostMalloc((void **)&sc.pinned_levels[m], RP_REFIT_LEVELS * sizeof(uint2), hipHostMallocDefault) != hipSuccess)
                return fail(h, RPTR_E_NOMEM, "hipHostMalloc failed");
            HIP_TRY(h, hipEventCreateWithFlags(&sc.ev_levels[m], hipEventDisableTiming));
        }
    return RPTR_OK;
}
// the light buffer of one scene copy. Without registered light sources every copy reads the buffer set_scene uploaded. With them
// (rptr_hip_set_light_sources) the copy owns a buffer -- padded with the zeroed bin like the shared one, filled from `src` -- that its
// refits re-place (refit_scene_copy), and the table of its float positions the placement reads.
static int scene_copy_lights(rptr_hip *h, SceneCopy &sc, const RptrTriLightData *src) {
    int rc;
    sc.lights = nullptr;
    sc.geom_dyn = nullptr;
    sc.dscene.lights = h->d_lights_shared;
    if (!h->d_light_sources) return RPTR_OK;
    const size_t before = h->scene_allocs.size(), bytes_before = h->bytes_scene;
    const size_t light_pad = RPTR_BINNED_LIGHTS_BIN_MAX_SIZE + 1, n = (size_t)h->num_lights;
    std::vector<const float *> table(sc.dynpos.begin(), sc.dynpos.end());
    rc = dev_upload(h, &sc.lights, n, src, hipMemcpyDeviceToDevice, &h->scene_allocs, light_pad);
    if (!rc) rc = dev_upload(h, &sc.geom_dyn, table.size(), table.data(), hipMemcpyHostToDevice, &h->scene_allocs);
    h->light_allocs.insert(h->light_allocs.end(), h->scene_allocs.begin() + (long)before, h->scene_allocs.end());
    h->light_bytes += h->bytes_scene - bytes_before;
    if (rc) return rc;
    HIP_TRY(h, hipMemset(sc.lights + n, 0, light_pad * sizeof(RptrTriLightData)));
    sc.dscene.lights = sc.lights;
    return RPTR_OK;
}
// One scene copy (host_state.h SceneCopy), given where its contents come from: the master set (from == NULL) is filled from the host's
// arrays, a frame context's copy from the master's device buffers. Either way the copy owns the node array with its boxes (ONE array,
// top level first: 88 bytes per node), the instance bounds, records and staged transforms (a frame still rendering never sees an instance
// move), the float positions of the deforming meshes with their per-mesh tables, geometry records that point at THOSE positions, and its
// refit tables. Triangles, shading records and triangle bounds only change when a mesh deforms: the context copies of a scene whose
// instances move and nothing else share the master's. The master's shading records are made afterwards (build_shade_records); a
// context's copy takes them from there.
static int scene_copy_build(rptr_hip *h, const RptrSceneDesc *s, const SceneTables &T, SceneCopy &sc, const SceneCopy *from) {
    int rc;
    std::vector<void *> *const A = &h->scene_allocs;
    const hipMemcpyKind kind = from ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t nn = h->h_nodes.size(), nt = h->h_tris.size(), ni = h->h_insts.size();
    // the table rptr_hip_update_instances stages into: per instance object_to_world + world_to_object, as the records hold them
    std::vector<float> xf(from ? 0 : (size_t)24 * s->num_instances);
    for (size_t i = 0; i * 24 < xf.size(); ++i) {
        memcpy(&xf[24 * i], s->instances[i].transform, 48);
        invert_affine(s->instances[i].transform, &xf[24 * i + 12]);
    }
    const void *src_nodes = h->h_nodes.data(), *src_node_box = h->h_node_box.data(), *src_tris = h->h_tris.data(), *src_insts = h->h_insts.data(), *src_xf = xf.data();
    if (from) {
        sc.dscene = from->dscene; // (the static arrays are shared between all copies)
        src_nodes = from->nodes, src_node_box = from->node_box, src_tris = from->tris, src_insts = from->dscene.insts, src_xf = from->inst_xf;
    }
    if ((rc = dev_upload(h, &sc.nodes, nn, src_nodes, kind, A))) return rc;
    if ((rc = dev_upload(h, &sc.node_box, 6 * nn, src_node_box, kind, A))) return rc;
    if ((rc = dev_alloc(h, &sc.inst_box, 6 * ni, A))) return rc;
    RptrBvhInstance *insts = nullptr;
    if ((rc = dev_upload(h, &insts, ni, src_insts, kind, A))) return rc;
    if ((rc = dev_upload(h, &sc.inst_xf, (size_t)24 * s->num_instances, src_xf, kind, A))) return rc;
    sc.tri_box = nullptr;
    if (!from || h->has_dynamic) {
        if ((rc = dev_upload(h, &sc.tris, nt, src_tris, kind, A, 2))) return rc; // +2: a leaf is fetched as whole pairs
        if ((rc = from ? dev_upload(h, &sc.shade, nt, from->shade, kind, A, 1) : dev_alloc(h, &sc.shade, nt + 1, A))) return rc;
        if (h->has_dynamic && (rc = dev_alloc(h, &sc.tri_box, 6 * nt, A))) return rc;
    } else {
        sc.tris = from->tris;
        sc.shade = from->shade;
    }
    // ---- deforming meshes keep full-precision float positions next to the quantised stream, and a table of them per mesh
    sc.dynpos.assign(s->num_geometries, nullptr);
    sc.mesh_dirty.assign(s->num_meshes, 0);
    sc.mesh_dyn.assign(s->num_meshes, nullptr);
    sc.dynnrm.assign(s->num_geometries, nullptr); // (skinned normal words: made by rptr_hip_set_skin)
    sc.mesh_nrm.assign(s->num_meshes, nullptr);
    for (uint32_t m = 0; m < s->num_meshes; ++m) {
        const RptrMeshDesc &mesh = s->meshes[m];
        if (!(mesh.dynamic & kMeshDeforms)) continue;
        std::vector<const float *> table(mesh.num_geometries, nullptr);
        for (uint32_t j = 0; j < mesh.num_geometries; ++j) {
            const uint32_t gi = mesh.first_geometry + j;
            const RptrGeometryDesc &gd = s->geometries[gi];
            std::vector<float> pos(from ? 0 : (size_t)gd.num_tris * 9);
            for (size_t v = 0; 3 * v < pos.size(); ++v) dequantize_position(gd.qpos[v], gd.quantized_scaling, gd.quantized_offset, &pos[3 * v]);
            if ((rc = dev_upload(h, &sc.dynpos[gi], (size_t)gd.num_tris * 9, from ? (const void *)from->dynpos[gi] : pos.data(), kind, A))) return rc;
            table[j] = sc.dynpos[gi];
        }
        if ((rc = dev_upload(h, &sc.mesh_dyn[m], table.size(), table.data(), hipMemcpyHostToDevice, A))) return rc;
        sc.mesh_dirty[m] = 2;
    }
    std::vector<RpGeomRecord> geoms = T.geoms;
    for (size_t r = 0; r < geoms.size(); ++r) geoms[r].dyn_pos = sc.dynpos[T.geom_index[r]];
    RpGeomRecord *d_geoms = nullptr;
    if ((rc = dev_upload(h, &d_geoms, geoms.size(), geoms.data(), hipMemcpyHostToDevice, A))) return rc;
    sc.dscene.nodes = sc.nodes;
    sc.dscene.tris = sc.tris;
    sc.dscene.shade = sc.shade;
    sc.dscene.insts = insts;
    sc.dscene.geoms = d_geoms;
    sc.version = h->refit_version;
    if ((rc = scene_copy_lights(h, sc, from ? from->dscene.lights : h->d_lights_shared))) return rc;
    return scene_copy_refit_tables(h, T, sc);
}
// what build_host_bvh made becomes the handle's
static void scene_adopt_bvh(rptr_hip *h, HostBvh &B) {
    h->h_nodes = std::move(B.nodes);
    h->h_node_box = std::move(B.node_box);
    h->h_tris = std::move(B.tris);
    h->h_insts = std::move(B.insts);
    h->meshes = std::move(B.meshes);
    h->mesh_root = std::move(B.mesh_root);
    h->num_tlas_insts = B.num_tlas_insts;
    h->num_tlas_nodes = B.num_tlas_nodes;
    h->flat_tris = B.flat_tris;
    h->flat_nodes = B.flat_nodes;
    h->tlas_capacity = B.tlas_capacity;
    memcpy(h->scene_lo, B.scene_lo, 12);
    memcpy(h->scene_hi, B.scene_hi, 12);
    h->master.dscene.num_nodes = (uint32_t)h->h_nodes.size();
    h->master.dscene.flat_id_bias = B.flat_id_bias > 0 ? B.flat_id_bias : 1;
    h->master.dscene.single_instance = (h->num_tlas_insts == 1 && h->opt.v[OPT_SINGLE_INSTANCE] != 0) ? 1 : 0;
}
int rptr_hip_set_scene(rptr_hip_t *h, const RptrSceneDesc *s) {
    if (!h || !s) return fail(h, RPTR_E_INVALID, "NULL argument");
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (void *p : h->scene_allocs) {
        (void)hipFree(p);
    }
    h->scene_allocs.clear();
    h->light_bytes = 0;
    h->light_allocs.clear(); // (a new scene drops the light-source registration: its buffers went with the rest)
    h->d_light_sources = nullptr;
    h->d_lights_shared = nullptr;
    h->bytes_scene = 0;
    h->bytes_allocated = h->bytes_frame;
    h->have_scene = false;
    int rc;
    if ((rc = scene_validate(h, s))) return rc;
    // ---- the static data, shared by every scene copy: textures, vertex streams, per-triangle material ids (with the host side of the
    // geometry records that name them), materials, lights
    RpScene &ds = h->master.dscene;
    RpTexture *d_textures = nullptr;
    float *d_srgb_lut = nullptr;
    if ((rc = scene_upload_textures(h, s, d_textures, d_srgb_lut))) return rc;
    std::vector<const uint64_t *> d_qpos, d_qnu;
    if ((rc = scene_upload_vertex_streams(h, s, d_qpos, d_qnu))) return rc;
    SceneTables T;
    if ((rc = scene_geometry_records(h, s, d_qpos, d_qnu, T))) return rc;
    h->record_geometry = T.geom_index;
    h->om = decltype(h->om)(); // (object-motion tracking belongs to a scene: its buffers went with scene_allocs above)
    RptrBaseMaterial *d_mats = nullptr;
    RptrTriLightData *d_lights = nullptr;
    if ((rc = dev_upload(h, &d_mats, s->num_materials, s->materials, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    // light buffer padded with one zeroed bin (+1): sample_tri_lights may read light_id == bin_end
    const size_t light_pad = RPTR_BINNED_LIGHTS_BIN_MAX_SIZE + 1;
    if ((rc = dev_upload(h, &d_lights, s->num_lights, s->lights, hipMemcpyHostToDevice, &h->scene_allocs, light_pad))) return rc;
    HIP_TRY(h, hipMemset(d_lights + s->num_lights, 0, light_pad * sizeof(RptrTriLightData)));
    ds.materials = d_mats;
    ds.lights = h->d_lights_shared = d_lights;
    h->h_lights.assign(s->lights, s->lights + s->num_lights); // (what rptr_hip_set_light_sources checks a registration against)
    ds.num_lights = h->num_lights = (int)s->num_lights;
    ds.num_materials = h->num_materials = (int)s->num_materials;
    ds.num_textures = (int)s->num_textures;
    ds.textures = d_textures;
    ds.srgb_lut = d_srgb_lut;
    // ---- acceleration structure
    HostBvh B;
    if ((rc = scene_build_acceleration_structure(h, s, d_qpos, T.geoms, B))) return rc;
    scene_adopt_bvh(h, B);
    // ---- moving instances: which instances have top-level records of their own, which ones carry lights
    h->num_instances = s->num_instances;
    h->inst_movable.assign(s->num_instances, 0);
    for (int k = 0; k < h->num_tlas_insts; ++k)
        if (h->h_insts[(size_t)k].instance_id >= 0 && (uint32_t)h->h_insts[(size_t)k].instance_id < s->num_instances) h->inst_movable[(size_t)h->h_insts[(size_t)k].instance_id] = 1;
    {
        std::vector<char> pmesh_emissive(s->num_parameterized_meshes, 0);
        for (uint32_t p = 0; p < s->num_parameterized_meshes; ++p) {
            const RptrParameterizedMeshDesc &pm = s->parameterized_meshes[p];
            const RptrMeshDesc &mesh = s->meshes[pm.mesh];
            size_t off = 0;
            for (uint32_t j = 0; j < mesh.num_geometries; ++j) {
                const uint32_t nt = s->geometries[mesh.first_geometry + j].num_tris;
                for (uint32_t t = 0; t < (pm.tri_material_ids ? nt : std::min(nt, 1u)); ++t) // (validated: every id is a material of the scene)
                    if (s->materials[(size_t)pm.material_offsets[j] + (pm.tri_material_ids ? pm.tri_material_ids[off + t] : 0)].emission_intensity > 0.0f) pmesh_emissive[p] = 1;
                off += nt;
            }
        }
        h->inst_emissive.assign(s->num_instances, 0);
        for (uint32_t i = 0; i < s->num_instances; ++i) h->inst_emissive[i] = pmesh_emissive[s->instances[i].parameterized_mesh];
        h->inst_mesh.assign(s->num_instances, 0);
        h->scene_xf.assign((size_t)12 * s->num_instances, 0.0f);
        for (uint32_t i = 0; i < s->num_instances; ++i) {
            h->inst_mesh[i] = (int)s->parameterized_meshes[s->instances[i].parameterized_mesh].mesh;
            memcpy(&h->scene_xf[(size_t)12 * i], s->instances[i].transform, 48);
        }
        h->mesh_has_lights.assign(s->num_meshes, 0);
    }
    if ((rc = dev_alloc(h, &h->d_inst_rejected, 1, &h->scene_allocs))) return rc;
    HIP_TRY(h, hipMemset(h->d_inst_rejected, 0, sizeof(uint32_t)));
    // ---- skinned meshes: no binding survives a new scene, the bone table is identity again
    {
        h->skin = decltype(h->skin)();
        h->skin.geom_qnu = d_qnu;
        h->skin.geom_normals.assign(s->num_geometries, 0);
        for (uint32_t g = 0; g < s->num_geometries; ++g) h->skin.geom_normals[g] = s->geometries[g].has_normals && d_qnu[g] ? 1 : 0;
        h->skin.bound.assign(s->num_geometries, 0);
        h->skin.records.assign(s->num_geometries, nullptr);
        h->skin.rest_pos.assign(s->num_geometries, nullptr);
        h->skin.rest_nrm.assign(s->num_geometries, nullptr); // (the table itself is made by the first call that needs it: skin_bone_table)
        h->morph = decltype(h->morph)(); // morph targets (morph.h): host vectors only; the device arrays are made by set_morph_targets
        h->morph.bound.assign(s->num_geometries, 0);
        h->morph.num_targets.assign(s->num_geometries, 0);
        h->morph.offsets.assign(s->num_geometries, nullptr);
        h->morph.entries.assign(s->num_geometries, nullptr);
        h->morph.weights.assign(s->num_geometries, nullptr);
        h->morph.cap_entries.assign(s->num_geometries, 0);
        h->morph.cap_weights.assign(s->num_geometries, 0);
        h->normals = decltype(h->normals)(); // recomputed normals (normals.h): the device arrays are made by set_normal_groups
        h->normals.bound.assign(s->num_geometries, 0);
        h->normals.flip.assign(s->num_geometries, 0);
        h->normals.num_groups.assign(s->num_geometries, 0);
        h->normals.offsets.assign(s->num_geometries, nullptr);
        h->normals.members.assign(s->num_geometries, nullptr);
    }
    // ---- refit tables, then the master copy
    if ((rc = scene_refit_tables(h, T))) return rc;
    h->rebuild_epoch.assign(h->meshes.size(), 0);
    h->bvh_credit = 0;
    h->rebuild_cursor = 0;
    h->host_insts_stale = false;
    h->host_bvh_stale = false;
    h->master_refit_pending = false;
    if ((rc = scene_copy_build(h, s, T, h->master, nullptr))) return rc;
    scene_traversal_preset(h);
    // ---- one shading record per BVH triangle (dshade.h RpShadeTri), made on the device from what was just uploaded: per mesh with the
    // geometry records of the first parameterized mesh that uses it, or -- a flattened scene -- per triangle through the instance it names
    h->mesh_geometry_base.assign(s->num_meshes, -1);
    for (uint32_t p = s->num_parameterized_meshes; p-- > 0;) h->mesh_geometry_base[s->parameterized_meshes[p].mesh] = T.pmesh_base[p];
    if ((rc = build_shade_records(h, h->master, -1, h->stream))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // ---- dynamic scene (meshes that deform, or instances that move: RPTR_MESH_INSTANCES_MOVE) + frames in flight: every frame context
    // gets its own set of what a refit rewrites
    for (SceneCopy &sc : h->ctx_scene) release_scene_copy_host(sc);
    h->ctx_scene.clear();
    if ((h->has_dynamic || h->tlas_capacity > 0) && h->ctx.size() > 1) {
        h->ctx_scene.resize(h->ctx.size());
        for (SceneCopy &sc : h->ctx_scene)
            if ((rc = scene_copy_build(h, s, T, sc, &h->master))) return rc;
    }
    h->have_scene = true;
    // a new scene restarts accumulation (Shell::set_scene -> reset, libapp/shell.cpp:96-126)
    h->frame_offset += h->frame_id;
    h->frame_id = 0;
    return RPTR_OK;
}

// ---- object motion (object_motion.h, rptr_hip_track_object_motion): what an update does for the tracking BEFORE it stages anything, on
// the backend's stream. The first update after a submission keeps the staged transform table -- what the last submitted frame saw, as
// long as every update was refitted before that frame (rptr_hip_object_motion refuses otherwise) -- and clears the changed marks; the
// first update of a geometry's positions in that interval keeps those. geometry < 0: an instance update.
static int object_motion_before_update(rptr_hip *h, int geometry) {
    auto &om = h->om;
    if (!om.enabled) return RPTR_OK;
    if (!om.staged_since_submission) {
        if (h->num_instances)
            HIP_TRY(h, hipMemcpyAsync(om.prev_inst_xf, h->master.inst_xf, (size_t)96 * h->num_instances, hipMemcpyDeviceToDevice, h->stream));
        if (!om.geom_marked.empty()) HIP_TRY(h, hipMemsetAsync(om.d_geom_changed, 0, om.geom_marked.size() * sizeof(uint32_t), h->stream));
        std::fill(om.geom_marked.begin(), om.geom_marked.end(), 0);
        om.snapshot = true;
        om.snapshot_of = om.submissions;
        om.staged_since_submission = true;
    }
    if (geometry >= 0 && !om.geom_marked[(size_t)geometry]) {
        HIP_TRY(h, hipMemcpyAsync(om.prev_pos[(size_t)geometry], h->master.dynpos[(size_t)geometry], (size_t)h->geom_tris[(size_t)geometry] * 9 * sizeof(float),
                                  hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)(om.d_geom_changed + geometry), 1, 1, h->stream));
        om.geom_marked[(size_t)geometry] = 1;
    }
    return RPTR_OK;
}

static int update_vertices_common(rptr_hip_t *h, uint32_t geometry, const float *xyz, uint32_t num_vertices, bool device_src) {
    if (!h || !xyz) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "update_vertices before set_scene");
    if (h->ctx_scene.empty()) { // frames in flight read the master vertex buffer and tree
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    if (geometry >= h->master.dynpos.size() || !h->master.dynpos[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u does not belong to a dynamic mesh (RptrMeshDesc.dynamic)", geometry);
    if (num_vertices != 3u * h->geom_tris[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u has %u unrolled vertices, got %u", geometry, 3u * h->geom_tris[geometry], num_vertices);
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rc0 = object_motion_before_update(h, (int)geometry);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipMemcpyAsync(h->master.dynpos[geometry], xyz, (size_t)num_vertices * 12, device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              h->stream));
    if (!device_src) HIP_TRY(h, hipStreamSynchronize(h->stream)); // the host array is only borrowed for the call
    h->master.mesh_dirty[h->geom_mesh[geometry]] = 1;
    h->vertex_updates++;
    h->om.unrefitted = true; // (kept whether the tracking is on or not: it may be switched on between an update and its refit)
    return RPTR_OK;
}
int rptr_hip_update_vertices(rptr_hip_t *h, uint32_t geometry, const float *xyz, uint32_t num_vertices) {
    return update_vertices_common(h, geometry, xyz, num_vertices, false);
}
// the reference animates on the device (a compute shader writes float_vertex_buf, render_vulkan.cpp:2834-2840):
// same call with a DEVICE source, ordered on the backend's stream, no host synchronisation
int rptr_hip_update_vertices_device(rptr_hip_t *h, uint32_t geometry, const float *device_xyz, uint32_t num_vertices) {
    return update_vertices_common(h, geometry, device_xyz, num_vertices, true);
}

// ---- moving instances: new object-to-world transforms for scene instances [first, first + count), staged for the next refit
static int update_instances_common(rptr_hip_t *h, uint32_t first, uint32_t count, const float *xf12, bool device_src) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "update_instances before set_scene");
    if ((uint64_t)first + count > h->num_instances)
        return fail(h, RPTR_E_INVALID, "instances [%u, +%u) are outside the scene's %u instances", first, count, h->num_instances);
    if (count == 0) return RPTR_OK;
    if (!xf12) return fail(h, RPTR_E_INVALID, "NULL transforms");
    for (uint32_t i = first; i < first + count; ++i) {
        if (!h->inst_movable[i])
            return fail(h, RPTR_E_INVALID, "instance %u is baked into the flattened world-space tree and cannot move: set RPTR_MESH_INSTANCES_MOVE in "
                                           "RptrMeshDesc.dynamic of its mesh (or option flatten = 0) before set_scene", i);
        if (h->inst_emissive[i] && !h->d_light_sources)
            return fail(h, RPTR_E_UNSUPPORTED, "instance %u uses an emissive material: RptrSceneDesc.lights holds its triangles in world space and would go stale "
                                               "(register rptr_hip_set_light_sources first)", i);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<float> rows; // host source: the table rows, checked before anything is queued
    if (!device_src) {
        rows.resize((size_t)24 * count);
        for (uint32_t i = 0; i < count; ++i) {
            const float *m = xf12 + 12ull * i;
            float *row = &rows[(size_t)24 * i];
            memcpy(row, m, 48);
            invert_affine(m, row + 12);
            bool ok = true;
            for (int k = 0; k < 24; ++k) ok = ok && std::isfinite(row[k]); // (det == 0: 1 / det is infinite)
            if (!ok) return fail(h, RPTR_E_INVALID, "transform %u (instance %u) is not finite or singular", i, first + i);
        }
    }
    {
        const int rc0 = object_motion_before_update(h, -1);
        if (rc0) return rc0;
    }
    if (device_src)
        hipLaunchKernelGGL(rp_k_stage_instance_transforms, dim3(grid_for(h, count)), dim3(256), 0, h->stream, xf12, first, count, h->master.inst_xf, h->d_inst_rejected);
    else {
        HIP_TRY(h, hipMemcpyAsync(h->master.inst_xf + 24ull * first, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (pageable staging: the copy must be over before `rows` goes)
    }
    HIP_TRY(h, hipGetLastError());
    h->inst_version++;
    h->vertex_updates++; // (one counter for everything a refit has to pick up: rptr_hip_refit with frame contexts that own their sets)
    h->om.unrefitted = true;
    return RPTR_OK;
}
int rptr_hip_update_instances(rptr_hip_t *h, uint32_t first_instance, uint32_t count, const float *transforms12) {
    return update_instances_common(h, first_instance, count, transforms12, false);
}
int rptr_hip_update_instances_device(rptr_hip_t *h, uint32_t first_instance, uint32_t count, const float *device_transforms12) {
    return update_instances_common(h, first_instance, count, device_transforms12, true);
}
int rptr_hip_set_tlas_policy(rptr_hip_t *h, int mode) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (mode != RPTR_TLAS_REBUILD && mode != RPTR_TLAS_REFIT) return fail(h, RPTR_E_INVALID, "unknown top-level policy %d (0 = REBUILD, 1 = REFIT)", mode);
    h->tlas_policy = mode;
    return RPTR_OK;
}
int rptr_hip_tlas_rebuild_count(const rptr_hip_t *h, uint64_t *out_rebuilds) {
    if (!h || !out_rebuilds) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    *out_rebuilds = h->tlas_rebuilds;
    return RPTR_OK;
}

// ≙ BLAS update (VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE) of the dirty dynamic meshes + TLAS refit
// (render_vulkan.cpp:1323-1354, executed at the top of draw_frame :2165): topology is kept, triangles and all
// boxes are recomputed on the device, level by level from the leaves up.
extern "C++" {
// the shading records (dshade.h RpShadeTri) of one scene copy's triangles: of mesh `only_mesh`, or (-1) of every mesh
static int build_shade_records(rptr_hip *h, SceneCopy &sc, int only_mesh, hipStream_t st) {
    if (h->flat_tris && only_mesh < 0) // the world-space tree over the static instances' triangles: every triangle names its instance record
        hipLaunchKernelGGL(rp_k_build_shade_tris, dim3(grid_for(h, h->flat_tris)), dim3(256), 0, st, sc.dscene, sc.shade, 0u, (uint32_t)h->flat_tris, -1);
    for (size_t m = 0; m < h->meshes.size(); ++m) { // meshes with trees of their own (a mesh inside the flattened tree has none)
        const MeshRt &mr = h->meshes[m];
        if ((only_mesh >= 0 && (int)m != only_mesh) || mr.tri_count <= 0 || h->mesh_geometry_base[m] < 0) continue;
        hipLaunchKernelGGL(rp_k_build_shade_tris, dim3(grid_for(h, (size_t)mr.tri_count)), dim3(256), 0, st, sc.dscene, sc.shade, (uint32_t)mr.tri_base,
                           (uint32_t)mr.tri_count, h->mesh_geometry_base[m]);
    }
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}

// skinned meshes (skin.h): the skinned normal words of mesh m go into its shading records. A mesh none of whose geometries was ever bound
// (or has normals) launches nothing.
static void refit_mesh_normals(rptr_hip *h, SceneCopy &sc, size_t m, hipStream_t st) {
    const MeshRt &mr = h->meshes[m];
    if (m >= sc.mesh_nrm.size() || !sc.mesh_nrm[m] || mr.tri_count <= 0) return;
    hipLaunchKernelGGL(rp_k_refit_normals, dim3(grid_for(h, (size_t)mr.tri_count)), dim3(256), 0, st, sc.tris, sc.shade, (uint32_t)mr.tri_base, (uint32_t)mr.tri_count,
                       sc.mesh_nrm[m]);
}

// the depth levels of dynamic mesh m of one scene copy, deepest first: a launch per deep level, the shallow ones (at most 4^5 + ... + 1
// nodes) in the single-block kernel, which also does the instance bounds and the top level when `with_top`
static void refit_mesh_levels(rptr_hip *h, SceneCopy &sc, size_t m, hipStream_t st, bool with_top) {
    const MeshRt &mr = h->meshes[m];
    if (!sc.levels_known[m] && sc.ev_levels[m] && hipEventQuery(sc.ev_levels[m]) == hipSuccess) { // the read-back of a device-built tree's table has arrived
        memcpy(sc.host_levels[m].data(), sc.pinned_levels[m], RP_REFIT_LEVELS * sizeof(uint2));
        sc.levels_known[m] = 1;
    }
    const uint2 *dev_levels = sc.blas_levels + m * RP_REFIT_LEVELS;
    const int n_top = 6; // depths 0..5
    for (int slot = 0; slot < RP_REFIT_LEVELS - n_top; ++slot) {
        size_t work = (size_t)mr.node_capacity; // level size unknown to the host: any launch covers it (grid stride)
        if (sc.levels_known[m]) {
            work = sc.host_levels[m][(size_t)slot].y - sc.host_levels[m][(size_t)slot].x;
            if (!work) continue;
        }
        hipLaunchKernelGGL(rp_k_refit_level, dim3(grid_for(h, work, 4)), dim3(256), 0, st, sc.nodes, sc.node_box, sc.tri_box, nullptr, sc.blas_list, dev_levels + slot);
    }
    RptrBvhInstance *insts = const_cast<RptrBvhInstance *>(sc.dscene.insts);
    hipLaunchKernelGGL(rp_k_refit_top, dim3(1), dim3(1024), 0, st, sc.nodes, sc.node_box, sc.tri_box, sc.inst_box, sc.blas_list,
                       dev_levels + (RP_REFIT_LEVELS - n_top), n_top, h->d_refit_list, h->d_refit_levels, with_top ? (int)h->refit_levels_tlas.size() : 0, insts,
                       with_top ? (uint32_t)h->num_tlas_insts : 0u);
}

// work space of the device-side builds of one scene copy (lbvh.h RpLbvhScratch), for n primitives
static int lbvh_scratch(rptr_hip *h, SceneCopy &sc, size_t n, hipStream_t st) {
    RpLbvhScratch &w = sc.scratch;
    if (w.capacity < std::max<size_t>(n, 2)) { // first rebuild (of a set this large): work space for the largest dynamic mesh / the top level's records
        size_t cap = 2, cap_tris = 0; // (cap_tris: the triangle copies of the gather -- a top-level build gathers nothing)
        for (const MeshRt &x : h->meshes)
            if (x.dynamic) cap_tris = std::max<size_t>(cap_tris, (size_t)x.tri_count);
        cap = std::max(cap, cap_tris);
        if (h->tlas_capacity > 0) cap = std::max<size_t>(cap, (size_t)h->num_tlas_insts);
        // the work space is allocated into a local record and committed as a whole: a failure half way frees what it got (the rebuild is
        // retried with every refit, and a retry must not leak the earlier attempt's buffers while the device is short of memory)
        RpLbvhScratch t = w;
        std::vector<void *> got;
        auto fail_alloc = [&](int code) {
            for (void *p : got) (void)hipFree(p);
            return code;
        };
        auto alloc = [&](auto **out, size_t count) -> int {
            void *p = nullptr;
            const size_t bytes = std::max<size_t>(count, 1) * sizeof(**out);
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) return fail(h, RPTR_E_NOMEM, "hipMalloc(%zu) failed: %s (work space of a device-side BVH rebuild)", bytes, hipGetErrorString(e));
            got.push_back(p);
            *out = reinterpret_cast<std::remove_reference_t<decltype(**out)> *>(p);
            return RPTR_OK;
        };
        int rc;
        if ((rc = alloc(&t.keys_a, cap)) || (rc = alloc(&t.keys_b, cap))) return fail_alloc(rc);
        for (int **p : {&t.left, &t.right, &t.parent, &t.first, &t.last})
            if ((rc = alloc(p, cap))) return fail_alloc(rc);
        for (uint32_t **p : {&t.flag, &t.slot, &t.depth4})
            if ((rc = alloc(p, cap))) return fail_alloc(rc);
        if ((rc = alloc(&t.level_hist, RP_REFIT_LEVELS)) || (rc = alloc(&t.level_cursor, RP_REFIT_LEVELS)) || (rc = alloc(&t.tri_copy, cap_tris)) ||
            (rc = alloc(&t.tribox_copy, 6 * cap_tris)) || (rc = alloc(&t.bounds, 8)))
            return fail_alloc(rc);
        size_t sort_bytes = 0, scan_bytes = 0;
        (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, t.keys_a, t.keys_b, (int)cap, 0, 64, st);
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, t.flag, t.slot, (int)cap, st);
        t.cub_bytes = std::max(sort_bytes, scan_bytes) + 256;
        char *tmp = nullptr;
        if ((rc = alloc(&tmp, t.cub_bytes))) return fail_alloc(rc);
        t.cub_tmp = tmp;
        t.capacity = cap;
        for (void *p : got) { // committed: the scene owns the buffers now (an earlier, smaller work space stays until the next set_scene)
            h->scene_allocs.push_back(p);
        }
        w = t;
    }
    return RPTR_OK;
}

// bits that tell n primitives apart (the low bits of a sort key)
static int lbvh_index_bits(uint32_t n) {
    int bits = 1;
    while ((1ull << bits) < (unsigned long long)n) ++bits;
    return bits;
}
// the front half both device builds share (lbvh.h), over the n boxes of `box`: bounds -> keys -> sort -> hierarchy -> flags -> scan, with
// `after_hierarchy` (the bottom-level build's triangle gather) between hierarchy and flags. One primitive has no hierarchy: nothing runs.
template <class F>
static int lbvh_front_half(rptr_hip *h, RpLbvhScratch &w, const float *box, uint32_t n, int axis_bits, int leaf_size, hipStream_t st, F after_hierarchy) {
    if (n < 2) return RPTR_OK;
    const int g = grid_for(h, n);
    hipLaunchKernelGGL(rp_k_lbvh_reset, dim3(1), dim3(64), 0, st, w.bounds);
    hipLaunchKernelGGL(rp_k_lbvh_bounds, dim3(g), dim3(256), 0, st, box, n, w.bounds);
    hipLaunchKernelGGL(rp_k_lbvh_keys, dim3(g), dim3(256), 0, st, box, n, w.bounds, w.keys_a, lbvh_index_bits(n), axis_bits);
    size_t bytes = w.cub_bytes;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortKeys(w.cub_tmp, bytes, w.keys_a, w.keys_b, (int)n, 0, 64, st));
    hipLaunchKernelGGL(rp_k_lbvh_hierarchy, dim3(g), dim3(256), 0, st, w.keys_b, (int)n, w.left, w.right, w.parent, w.first, w.last);
    {
        const int rc = after_hierarchy();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(rp_k_lbvh_flags, dim3(g), dim3(256), 0, st, (int)n, w.parent, w.first, w.last, w.flag, w.depth4, leaf_size);
    bytes = w.cub_bytes;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, bytes, w.flag, w.slot, (int)n - 1, st));
    return RPTR_OK;
}

// device-side rebuild of the bottom-level tree of dynamic mesh m of one scene copy (lbvh.h), on stream `st`. The triangles of the mesh
// (current order) must hold the new vertices already (rp_k_refit_tris). Ends with the refit that gives the new topology its boxes.
static int lbvh_rebuild(rptr_hip *h, SceneCopy &sc, size_t m, hipStream_t st, bool with_top) {
    const MeshRt &mr = h->meshes[m];
    const uint32_t n = (uint32_t)mr.tri_count;
    {
        const int rc = lbvh_scratch(h, sc, n, st);
        if (rc) return rc;
    }
    RpLbvhScratch &w = sc.scratch;
    RptrBvhTri *tris = sc.tris + mr.tri_base;
    float *tri_box = sc.tri_box + 6ull * mr.tri_base;
    const int g = grid_for(h, n);
    {
        const int rc = lbvh_front_half(h, w, tri_box, n, 21, RP_LBVH_LEAF_TRIS, st, [&]() -> int { // the triangles and their boxes follow the sort
            HIP_TRY(h, hipMemcpyAsync(w.tri_copy, tris, (size_t)n * sizeof(RptrBvhTri), hipMemcpyDeviceToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(w.tribox_copy, tri_box, (size_t)n * 24, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(rp_k_lbvh_gather, dim3(g), dim3(256), 0, st, w.keys_b, n, w.tri_copy, w.tribox_copy, tris, tri_box, (1ull << lbvh_index_bits(n)) - 1ull);
            return RPTR_OK;
        });
        if (rc) return rc;
    }
    HIP_TRY(h, hipMemsetAsync(w.level_hist, 0, RP_REFIT_LEVELS * sizeof(uint32_t), st));
    hipLaunchKernelGGL(rp_k_lbvh_emit, dim3(g), dim3(256), 0, st, (int)n, w.left, w.right, w.first, w.last, w.flag, w.slot, w.depth4, mr.node_base, mr.tri_base, sc.nodes,
                       w.level_hist, sc.mesh_count + m, RpLbvhLeaves{RP_LBVH_LEAF_TRIS, nullptr, 0ull});
    uint2 *dev_levels = sc.blas_levels + m * RP_REFIT_LEVELS;
    hipLaunchKernelGGL(rp_k_lbvh_level_scan, dim3(1), dim3(64), 0, st, w.level_hist, (uint32_t)mr.node_base, dev_levels, w.level_cursor);
    hipLaunchKernelGGL(rp_k_lbvh_level_scatter, dim3(grid_for(h, (size_t)mr.node_capacity)), dim3(256), 0, st, sc.nodes, mr.node_base, sc.mesh_count + m, w.level_cursor,
                       sc.blas_list, 0u);
    // the host learns the level sizes when this copy has arrived; until then a refit launches every possible level
    sc.levels_known[m] = 0;
    HIP_TRY(h, hipMemcpyAsync(sc.pinned_levels[m], dev_levels, RP_REFIT_LEVELS * sizeof(uint2), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipEventRecord(sc.ev_levels[m], st));
    refit_mesh_levels(h, sc, m, st, with_top);
    HIP_TRY(h, hipGetLastError());
    sc.device_built[m] = 1;
    h->rebuilds_done++;
    return RPTR_OK;
}

// the top level of one scene copy by ITS OWN level lists (a device-built top level): boxes and encoding, deepest level first. The
// instance bounds must be current. Up to kTlasSingleBlock records the levels run in the one block of rp_k_refit_top (a block barrier per
// level instead of a launch); above it every level gets a launch. The break-even was ESTIMATED, not measured: 40 dependent launches cost
// about 40 x 5 us, one block of 1024 threads refits about 1000 nodes per pass, so the block wins while the tree has a few thousand nodes.
static const int kTlasSingleBlock = 8192;
static void tlas_refit_own(rptr_hip *h, SceneCopy &sc, hipStream_t st) {
    RptrBvhInstance *insts = const_cast<RptrBvhInstance *>(sc.dscene.insts);
    if (h->num_tlas_insts <= kTlasSingleBlock)
        hipLaunchKernelGGL(rp_k_refit_top, dim3(1), dim3(1024), 0, st, sc.nodes, sc.node_box, sc.tri_box, sc.inst_box, sc.blas_list, sc.blas_levels, 0, sc.tlas_list,
                           sc.tlas_levels, RP_REFIT_LEVELS, insts, 0u);
    else
        for (int slot = 0; slot < RP_REFIT_LEVELS; ++slot)
            hipLaunchKernelGGL(rp_k_refit_level, dim3(grid_for(h, (size_t)h->tlas_capacity, 4)), dim3(256), 0, st, sc.nodes, sc.node_box, sc.tri_box, sc.inst_box, sc.tlas_list,
                               sc.tlas_levels + slot);
}

// device-side rebuild of the top level of one scene copy over its instance records (tlas_build.h), on stream `st`. The instance bounds
// (sc.inst_box) must be current. Nodes [0, tlas_capacity) are rewritten; the records stay where they are.
static int tlas_rebuild(rptr_hip *h, SceneCopy &sc, hipStream_t st) {
    const uint32_t n = (uint32_t)h->num_tlas_insts;
    if ((size_t)std::max<uint32_t>(n, 1) > (size_t)h->tlas_capacity) return fail(h, RPTR_E_INVALID, "no top-level capacity for %u records", n);
    {
        const int rc = lbvh_scratch(h, sc, n, st);
        if (rc) return rc;
    }
    RpLbvhScratch &w = sc.scratch;
    const int g = grid_for(h, n);
    {
        const int rc = lbvh_front_half(h, w, sc.inst_box, n, RP_TLAS_AXIS_BITS, 1, st, [] { return RPTR_OK; });
        if (rc) return rc;
    }
    HIP_TRY(h, hipMemsetAsync(w.level_hist, 0, RP_REFIT_LEVELS * sizeof(uint32_t), st));
    hipLaunchKernelGGL(rp_k_tlas_clear, dim3(grid_for(h, (size_t)h->tlas_capacity)), dim3(256), 0, st, sc.nodes, sc.node_box, (uint32_t)h->tlas_capacity);
    hipLaunchKernelGGL(rp_k_lbvh_emit, dim3(g), dim3(256), 0, st, (int)n, w.left, w.right, w.first, w.last, w.flag, w.slot, w.depth4, 0, 0, sc.nodes, w.level_hist,
                       sc.tlas_count, RpLbvhLeaves{1, n >= 2 ? w.keys_b : nullptr, (1ull << lbvh_index_bits(n)) - 1ull});
    hipLaunchKernelGGL(rp_k_lbvh_level_scan, dim3(1), dim3(64), 0, st, w.level_hist, 0u, sc.tlas_levels, w.level_cursor);
    hipLaunchKernelGGL(rp_k_lbvh_level_scatter, dim3(grid_for(h, (size_t)h->tlas_capacity)), dim3(256), 0, st, sc.nodes, 0, sc.tlas_count, w.level_cursor, sc.tlas_list,
                       0x80000000u);
    sc.tlas_rebuilt = true;
    tlas_refit_own(h, sc, st); // (rp_refit_node rewrites the whole node: the depth the emit kernel parked in its padding goes)
    HIP_TRY(h, hipGetLastError());
    h->tlas_rebuilds++;
    return RPTR_OK;
}

// refits one copy of the mutable scene on stream `st`; all_dynamic: treat every dynamic mesh as changed. A mesh whose tree is older
// than the rebuild the policy asked for (rptr_hip_refit) is rebuilt instead of refitted. A rebuild that cannot start (no memory for its
// work space) is reported through *err -- the error text is in the handle -- and the mesh is refitted on its old topology instead, so
// that its boxes always match the new vertices; the rebuild is tried again with the next refit.
static bool refit_scene_copy(rptr_hip *h, SceneCopy &sc, bool all_dynamic, hipStream_t st, int *err) {
    bool any = all_dynamic && h->has_dynamic;
    const bool insts_moved = sc.inst_version != h->inst_version;
    any = any || insts_moved;
    for (size_t m = 0; m < h->meshes.size(); ++m) any = any || sc.mesh_dirty[m] == 1 || (h->meshes[m].dynamic && sc.built_epoch[m] != h->rebuild_epoch[m]);
    if (!any) return false;
    std::vector<size_t> todo;
    for (size_t m = 0; m < h->meshes.size(); ++m) {
        const MeshRt &mr = h->meshes[m];
        if (!mr.dynamic) continue;
        const bool rebuild = sc.built_epoch[m] != h->rebuild_epoch[m];
        if (!all_dynamic && !sc.mesh_dirty[m] && !rebuild) continue; // 1 = new vertices, 2 = dynamic but its triangle bounds were never written
        todo.push_back(m);
    }
    // staged instance transforms go into this copy's records first: everything below bounds the records from them
    if (insts_moved) {
        hipLaunchKernelGGL(rp_k_update_instance_records, dim3(grid_for(h, h->h_insts.size())), dim3(256), 0, st, const_cast<RptrBvhInstance *>(sc.dscene.insts),
                           (uint32_t)h->h_insts.size(), sc.inst_xf, h->num_instances);
        sc.inst_version = h->inst_version;
    }
    // registered light sources (rptr_hip_set_light_sources): this copy's lights go where their triangles are now -- behind the records'
    // update and the vertex copies (queued on this stream, or waited for by it), in front of every frame this copy renders next
    if (sc.lights && h->num_lights > 0) {
        bool place = insts_moved;
        for (size_t m : todo) place = place || h->mesh_has_lights[m];
        if (place)
            hipLaunchKernelGGL(rp_k_place_lights, dim3(grid_for(h, (size_t)h->num_lights)), dim3(256), 0, st, sc.lights, h->d_light_sources, (uint32_t)h->num_lights,
                               sc.inst_xf, sc.geom_dyn);
    }
    // moved instances under RPTR_TLAS_REBUILD get a new top level (where set_scene reserved room for one); a top level that was rebuilt
    // before is refitted by its own level lists, not the host's
    const bool rebuild_top = insts_moved && h->tlas_policy == RPTR_TLAS_REBUILD && h->tlas_capacity > 0 && h->num_tlas_insts > 0;
    const bool own_top = rebuild_top || sc.tlas_rebuilt;
    // the instance bounds and the top level ride in the single-block launch of the last mesh when they are small
    bool top_done = false;
    for (size_t k = 0; k < todo.size(); ++k) {
        const size_t m = todo[k];
        const MeshRt &mr = h->meshes[m];
        const bool with_top = h->refit_top_all && !own_top && k + 1 == todo.size();
        if (mr.tri_count)
            hipLaunchKernelGGL(rp_k_refit_tris, dim3(grid_for(h, (size_t)mr.tri_count)), dim3(256), 0, st, sc.tris, sc.tri_box, sc.shade, (uint32_t)mr.tri_base,
                               (uint32_t)mr.tri_count, sc.mesh_dyn[m]);
        refit_mesh_normals(h, sc, m, st);
        sc.mesh_dirty[m] = 0;
        if (sc.built_epoch[m] != h->rebuild_epoch[m]) {
            const int rc = lbvh_rebuild(h, sc, m, st, with_top);
            if (rc == RPTR_OK) {
                sc.built_epoch[m] = h->rebuild_epoch[m];
                (void)build_shade_records(h, sc, (int)m, st); // the rebuild reordered the mesh's triangles: its shading records follow
                refit_mesh_normals(h, sc, m, st);             // ... and they read the rest normals again: the skinned ones go back in
            } else {
                if (err && *err == RPTR_OK) *err = rc;
                refit_mesh_levels(h, sc, m, st, with_top);
            }
        } else
            refit_mesh_levels(h, sc, m, st, with_top);
        top_done = top_done || with_top;
    }
    if (!top_done && own_top) {
        RptrBvhInstance *insts = const_cast<RptrBvhInstance *>(sc.dscene.insts);
        const uint32_t ni = (uint32_t)h->num_tlas_insts;
        if (ni) hipLaunchKernelGGL(rp_k_refit_instances, dim3(grid_for(h, ni)), dim3(256), 0, st, sc.node_box, insts, sc.inst_box, ni);
        int rc = rebuild_top ? tlas_rebuild(h, sc, st) : RPTR_E_INVALID;
        if (rebuild_top && rc != RPTR_OK && err && *err == RPTR_OK) *err = rc; // (no memory for the work space: refitted instead, tried again next time)
        if (rc == RPTR_OK) top_done = true;
        else if (sc.tlas_rebuilt) {
            tlas_refit_own(h, sc, st);
            top_done = true;
        }
    }
    if (!top_done) { // instance bounds, then the top level
        RptrBvhInstance *insts = const_cast<RptrBvhInstance *>(sc.dscene.insts);
        const uint32_t ni = (uint32_t)h->num_tlas_insts;
        if (h->refit_top_all)
            hipLaunchKernelGGL(rp_k_refit_top, dim3(1), dim3(1024), 0, st, sc.nodes, sc.node_box, sc.tri_box, sc.inst_box, sc.blas_list, sc.blas_levels, 0,
                               h->d_refit_list, h->d_refit_levels, (int)h->refit_levels_tlas.size(), insts, ni);
        else {
            if (ni) hipLaunchKernelGGL(rp_k_refit_instances, dim3(grid_for(h, ni)), dim3(256), 0, st, sc.node_box, insts, sc.inst_box, ni);
            for (auto &lv : h->refit_levels_tlas)
                hipLaunchKernelGGL(rp_k_refit_nodes, dim3(grid_for(h, lv[1] - lv[0])), dim3(256), 0, st, sc.nodes, sc.node_box, sc.tri_box, sc.inst_box,
                                   h->d_refit_list, lv[0], lv[1]);
        }
    }
    return true;
}
} // extern "C++"

int rptr_hip_refit(rptr_hip_t *h) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "refit before set_scene");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->ctx_scene.empty()) { // frames in flight read the master set
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    h->om.unrefitted = false; // (object motion: what was staged reaches the next frame)
    // ---- the BVH policy: which dynamic meshes get a new tree instead of a refit (librender/render_params.glsl.h:61,90-93)
    {
        bool changed = false;
        for (size_t m = 0; m < h->meshes.size(); ++m) changed = changed || (h->meshes[m].dynamic && h->master.mesh_dirty[m] == 1);
        if (changed && h->bvh_force_rebuild) {
            for (size_t m = 0; m < h->meshes.size(); ++m)
                if (h->meshes[m].rebuildable && h->master.mesh_dirty[m] == 1) h->rebuild_epoch[m]++;
        } else if (changed && h->bvh_budget > 0) {
            // a budget of triangles per refit call: it is saved up until it covers the next mesh in turn (a mesh larger than the budget is
            // rebuilt every ceil(triangles / budget) calls), dynamic meshes take turns
            long long total = 0;
            std::vector<size_t> dyn;
            for (size_t m = 0; m < h->meshes.size(); ++m)
                if (h->meshes[m].rebuildable) {
                    dyn.push_back(m);
                    total += h->meshes[m].tri_count;
                }
            h->bvh_credit = std::min(h->bvh_credit + h->bvh_budget, std::max(total, h->bvh_budget));
            for (size_t tries = 0; tries < dyn.size() && !dyn.empty(); ++tries) {
                const size_t m = dyn[(size_t)h->rebuild_cursor % dyn.size()];
                if (h->bvh_credit < h->meshes[m].tri_count) break;
                h->bvh_credit -= h->meshes[m].tri_count;
                h->rebuild_epoch[m]++;
                h->rebuild_cursor = (h->rebuild_cursor + 1) % (int)dyn.size();
            }
        }
    }
    if (!h->ctx_scene.empty()) {
        // frames render from the contexts' own sets, which follow from the master's VERTICES when their next frame is submitted:
        // the master's tree is only needed by ray queries and the export, and is refitted when one of them asks for it
        if (h->vertex_updates != h->vertex_updates_refitted) { // (the dirty marks stay for the deferred refit of the master tree)
            h->vertex_updates_refitted = h->vertex_updates;
            h->master_refit_pending = true;
            h->host_bvh_stale = true;
            h->host_insts_stale = true;
            h->refit_version++;
        }
        return RPTR_OK;
    }
    int err = RPTR_OK;
    if (refit_scene_copy(h, h->master, false, h->stream, &err)) {
        HIP_TRY(h, hipGetLastError());
        h->host_bvh_stale = true;
        h->host_insts_stale = true;
        h->refit_version++; // the frame contexts' own sets follow when their next frame is submitted
        h->master.version = h->refit_version;
    }
    return err;
}

// the master set's tree after a deferred refit (see rptr_hip_refit)
static int ensure_master_tree(rptr_hip *h) {
    if (!h->master_refit_pending) return RPTR_OK;
    h->master_refit_pending = false;
    int err = RPTR_OK;
    if (refit_scene_copy(h, h->master, false, h->stream, &err)) HIP_TRY(h, hipGetLastError());
    h->master.version = h->refit_version;
    return err;
}

// ---- moving lights: the provenance of RptrSceneDesc.lights (include/rptr_hip.h)
// what the registration allocated goes: every copy reads the buffer set_scene uploaded again
static void drop_light_sources(rptr_hip *h) {
    h->bytes_scene -= std::min(h->light_bytes, h->bytes_scene);
    h->light_bytes = 0;
    for (void *p : h->light_allocs) {
        (void)hipFree(p);
        h->scene_allocs.erase(std::remove(h->scene_allocs.begin(), h->scene_allocs.end(), p), h->scene_allocs.end());
    }
    h->bytes_allocated = h->bytes_scene + h->bytes_frame;
    h->light_allocs.clear();
    h->d_light_sources = nullptr;
    h->master.lights = nullptr, h->master.geom_dyn = nullptr, h->master.dscene.lights = h->d_lights_shared;
    for (SceneCopy &sc : h->ctx_scene) sc.lights = nullptr, sc.geom_dyn = nullptr, sc.dscene.lights = h->d_lights_shared;
    std::fill(h->mesh_has_lights.begin(), h->mesh_has_lights.end(), 0);
}
// Allowed difference between a light as uploaded and the placement rule applied to its source, per coordinate, relative to
// S = |m0 x| + |m1 y| + |m2 z| + |m3|. One evaluation of (m0 x + m1 y) + (m2 z + m3) in float32 rounds three products (each within
// 2^-24 of itself, together within 2^-24 S), two inner sums (together within 2^-24 S, to first order) and the outer sum (within 2^-24 S):
// within 3 x 2^-24 S of the exact value, and a fused multiply-add only drops roundings. The host's evaluation and the one here: 6 x 2^-24 S
// = 0.375 x 2^-20 S. The bound leaves a margin of 2.7 over that; a light of another triangle or instance misses it by orders of magnitude.
static const double kLightSourceTolerance = 1.0 / 1048576.0; // 2^-20
int rptr_hip_set_light_sources(rptr_hip_t *h, const RptrLightSource *sources, uint32_t count) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "set_light_sources before set_scene");
    if ((sources == nullptr) != (count == 0)) return fail(h, RPTR_E_INVALID, "sources and count must both be given, or NULL and 0 to unregister");
    if (count && count != (uint32_t)h->num_lights) return fail(h, RPTR_E_INVALID, "%u light sources for a scene of %d lights", count, h->num_lights);
    std::vector<char> mesh_has_lights(h->mesh_has_lights.size(), 0);
    for (uint32_t i = 0; i < count; ++i) {
        const RptrLightSource &s = sources[i];
        if (s.instance >= h->num_instances) return fail(h, RPTR_E_INVALID, "light source %u: instance %u of %u", i, s.instance, h->num_instances);
        if (s.geometry >= h->geom_tris.size()) return fail(h, RPTR_E_INVALID, "light source %u: geometry %u of %zu", i, s.geometry, h->geom_tris.size());
        if (s.triangle >= h->geom_tris[s.geometry])
            return fail(h, RPTR_E_INVALID, "light source %u: triangle %u of geometry %u, which has %u", i, s.triangle, s.geometry, h->geom_tris[s.geometry]);
        if (h->geom_mesh[s.geometry] != h->inst_mesh[s.instance])
            return fail(h, RPTR_E_INVALID, "light source %u: geometry %u belongs to mesh %d, instance %u is one of mesh %d", i, s.geometry, h->geom_mesh[s.geometry],
                        s.instance, h->inst_mesh[s.instance]);
        const float *M = &h->scene_xf[(size_t)12 * s.instance];
        const float *src[3] = {s.v0, s.v1, s.v2}, *dst[3] = {h->h_lights[i].v0, h->h_lights[i].v1, h->h_lights[i].v2};
        for (int k = 0; k < 3; ++k)
            for (int r = 0; r < 3; ++r) {
                const float *m = M + 4 * r, *p = src[k];
                const float a = m[0] * p[0], b = m[1] * p[1], c = m[2] * p[2];
                const float ab = a + b, cd = c + m[3];
                const float placed = ab + cd;
                const double sum = std::fabs((double)m[0] * p[0]) + std::fabs((double)m[1] * p[1]) + std::fabs((double)m[2] * p[2]) + std::fabs((double)m[3]);
                if (!(std::fabs((double)placed - (double)dst[k][r]) <= kLightSourceTolerance * sum))
                    return fail(h, RPTR_E_INVALID, "light source %u: vertex %d coordinate %d of instance %u, geometry %u, triangle %u lands at %.9g, light %u has %.9g: "
                                                   "not where this light came from", i, k, r, s.instance, s.geometry, s.triangle, (double)placed, i, (double)dst[k][r]);
            }
        mesh_has_lights[(size_t)h->geom_mesh[s.geometry]] = 1;
    }
    // ---- checked: from here on the scene copies change, so nothing of the handle may still be rendering from them
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drop_light_sources(h);
    if (!count) return RPTR_OK;
    int rc;
    {
        const size_t before = h->scene_allocs.size(), bytes_before = h->bytes_scene;
        rc = dev_upload(h, &h->d_light_sources, count, sources, hipMemcpyHostToDevice, &h->scene_allocs);
        h->light_allocs.insert(h->light_allocs.end(), h->scene_allocs.begin() + (long)before, h->scene_allocs.end());
        h->light_bytes += h->bytes_scene - bytes_before;
    }
    // every copy starts from the lights as set_scene got them; its next refit that finds moved instances or new vertices re-places them.
    // (No copies are made for a scene that has none: rptr_hip_refit waits for the frames in flight when every context reads the master's.)
    if (!rc) rc = scene_copy_lights(h, h->master, h->d_lights_shared);
    for (SceneCopy &sc : h->ctx_scene)
        if (!rc) rc = scene_copy_lights(h, sc, h->d_lights_shared);
    if (rc) {
        const std::string why = h->last_error;
        drop_light_sources(h);
        h->last_error = why;
        return rc;
    }
    h->mesh_has_lights = mesh_has_lights;
    return RPTR_OK;
}
int rptr_hip_readback_lights(rptr_hip_t *h, RptrTriLightData *out, uint32_t count) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "readback_lights before set_scene");
    if (count != (uint32_t)h->num_lights) return fail(h, RPTR_E_INVALID, "room for %u lights, the scene has %d", count, h->num_lights);
    if (count && !out) return fail(h, RPTR_E_INVALID, "NULL argument");
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = ensure_master_tree(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (count) HIP_TRY(h, hipMemcpy(out, h->master.dscene.lights, (size_t)count * sizeof(RptrTriLightData), hipMemcpyDeviceToHost));
    return RPTR_OK;
}

// ---- skinned meshes (include/rptr_hip.h "skinned meshes", skin.h)
// the bone table (identity) and the counter of rejected vertices, made by the first set_skin / update_bones after a set_scene: a scene
// that is never skinned allocates what it always did
static int skin_rejected_counter(rptr_hip *h) { // (a geometry with morph targets and no skin needs only this)
    auto &sk = h->skin;
    if (!sk.d_rejected) {
        const int rc = dev_alloc(h, &sk.d_rejected, 1, &h->scene_allocs);
        if (rc) return rc;
        HIP_TRY(h, hipMemset(sk.d_rejected, 0, sizeof(uint32_t)));
    }
    return RPTR_OK;
}
static int skin_bone_table(rptr_hip *h) {
    int rc;
    auto &sk = h->skin;
    if (!sk.d_bones) {
        std::vector<float> identity((size_t)12 * RPTR_MAX_BONES, 0.0f);
        for (size_t b = 0; b < RPTR_MAX_BONES; ++b) identity[12 * b] = identity[12 * b + 5] = identity[12 * b + 10] = 1.0f;
        if ((rc = dev_upload(h, &sk.d_bones, identity.size(), identity.data(), hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    }
    return skin_rejected_counter(h);
}
// the rest pose of `geometry`, shared by the skinner and the morph stage: a device copy of its float positions now (`capture`; a binding
// call on a geometry that already has the other deformer bound keeps the one it has), the normal halves of its qnrm_uv words as uploaded,
// and -- for a geometry with normals -- the output array of normal words in the master and in every frame context's scene copy
static int skin_copy_normals(rptr_hip *h, SceneCopy &sc, uint32_t geometry);
// the normal half of it, which is all rptr_hip_set_normal_groups needs: the rest normal words and the output arrays of a geometry with normals
static int skin_rest_normals(rptr_hip *h, uint32_t geometry) {
    int rc;
    auto &sk = h->skin;
    const uint32_t n = 3u * h->geom_tris[geometry];
    if (!sk.geom_normals[geometry]) return RPTR_OK;
    if (!sk.rest_nrm[geometry]) {
        if ((rc = dev_alloc(h, &sk.rest_nrm[geometry], n, &h->scene_allocs))) return rc;
        if (n) hipLaunchKernelGGL(rp_k_skin_rest_normals, dim3(grid_for(h, n)), dim3(256), 0, h->stream, sk.geom_qnu[geometry], sk.rest_nrm[geometry], n);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if ((rc = skin_copy_normals(h, h->master, geometry))) return rc;
    for (SceneCopy &sc : h->ctx_scene)
        if ((rc = skin_copy_normals(h, sc, geometry))) return rc;
    return RPTR_OK;
}
static int skin_rest_pose(rptr_hip *h, uint32_t geometry, bool capture) {
    int rc;
    auto &sk = h->skin;
    const uint32_t n = 3u * h->geom_tris[geometry];
    if (!sk.rest_pos[geometry]) {
        if ((rc = dev_alloc(h, &sk.rest_pos[geometry], (size_t)n * 3, &h->scene_allocs))) return rc;
        capture = true;
    }
    if (capture) HIP_TRY(h, hipMemcpy(sk.rest_pos[geometry], h->master.dynpos[geometry], (size_t)n * 12, hipMemcpyDeviceToDevice));
    return skin_rest_normals(h, geometry);
}
// one scene copy's skinned normal words of `geometry` (made once, starting from the rest normals) and the table of its mesh
static int skin_copy_normals(rptr_hip *h, SceneCopy &sc, uint32_t geometry) {
    int rc;
    const size_t n = (size_t)h->geom_tris[geometry] * 3;
    if (!sc.dynnrm[geometry]) {
        uint32_t *d = nullptr;
        if ((rc = dev_upload(h, &d, n, h->skin.rest_nrm[geometry], hipMemcpyDeviceToDevice, &h->scene_allocs))) return rc;
        sc.dynnrm[geometry] = d;
    }
    const int m = h->geom_mesh[geometry];
    std::vector<const uint32_t *> table;
    for (size_t g = 0; g < h->geom_mesh.size(); ++g)
        if (h->geom_mesh[g] == m) table.push_back(sc.dynnrm[g]); // (a mesh's geometries are consecutive: the table's order is the mesh's)
    if (!sc.mesh_nrm[(size_t)m]) return dev_upload(h, &sc.mesh_nrm[(size_t)m], table.size(), table.data(), hipMemcpyHostToDevice, &h->scene_allocs);
    HIP_TRY(h, hipMemcpy(sc.mesh_nrm[(size_t)m], table.data(), table.size() * sizeof(table[0]), hipMemcpyHostToDevice));
    return RPTR_OK;
}
int rptr_hip_set_skin(rptr_hip_t *h, uint32_t geometry, const RptrSkinVertex *vertices, uint32_t num_vertices) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "set_skin before set_scene");
    if (geometry >= h->master.dynpos.size() || !h->master.dynpos[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u does not belong to a dynamic mesh (RptrMeshDesc.dynamic)", geometry);
    if ((vertices == nullptr) != (num_vertices == 0)) return fail(h, RPTR_E_INVALID, "vertices and num_vertices must both be given, or NULL and 0 to unbind");
    const uint32_t n = 3u * h->geom_tris[geometry];
    if (vertices) {
        if (num_vertices != n) return fail(h, RPTR_E_INVALID, "geometry %u has %u unrolled vertices, got %u", geometry, n, num_vertices);
        for (uint32_t v = 0; v < n; ++v) {
            uint32_t sum = 0;
            for (int k = 0; k < 4; ++k) {
                if (vertices[v].bone[k] >= RPTR_MAX_BONES)
                    return fail(h, RPTR_E_INVALID, "skin vertex %u: bone %u (influence %d) is outside the table of %d bones", v, (unsigned)vertices[v].bone[k], k, RPTR_MAX_BONES);
                sum += vertices[v].weight[k];
            }
            if (sum != 65535u) return fail(h, RPTR_E_INVALID, "skin vertex %u: its weights sum to %u, not 65535", v, sum);
        }
    }
    // ---- checked: from here on the scene copies change, so nothing of the handle may still be rendering from them
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto &sk = h->skin;
    if (!vertices) { // unbind: positions and normals stay as last written
        sk.bound[geometry] = 0;
        return RPTR_OK;
    }
    int rc;
    sk.bound[geometry] = 0;
    if ((rc = skin_bone_table(h))) return rc;
    if (!sk.records[geometry] && (rc = dev_alloc(h, &sk.records[geometry], n, &h->scene_allocs))) return rc;
    HIP_TRY(h, hipMemcpy(sk.records[geometry], vertices, (size_t)n * sizeof(RptrSkinVertex), hipMemcpyHostToDevice));
    if ((rc = skin_rest_pose(h, geometry, !h->morph.bound[geometry]))) return rc; // (morph targets bound: their rest pose is this one's too)
    sk.bound[geometry] = 1;
    return RPTR_OK;
}
static int update_bones_common(rptr_hip_t *h, uint32_t first, uint32_t count, const float *xf12, bool device_src) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "update_bones before set_scene");
    if ((uint64_t)first + count > RPTR_MAX_BONES) return fail(h, RPTR_E_INVALID, "bones [%u, +%u) are outside the table of %d bones", first, count, RPTR_MAX_BONES);
    if (count == 0) return RPTR_OK;
    if (!xf12) return fail(h, RPTR_E_INVALID, "NULL transforms");
    if (!device_src)
        for (uint32_t i = 0; i < count; ++i)
            for (int k = 0; k < 12; ++k)
                if (!std::isfinite(xf12[12ull * i + k])) return fail(h, RPTR_E_INVALID, "transform %u (bone %u) is not finite", i, first + i);
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const int rc0 = skin_bone_table(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipMemcpyAsync(h->skin.d_bones + 12ull * first, xf12, (size_t)count * 48, device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!device_src) HIP_TRY(h, hipStreamSynchronize(h->stream)); // the host array is only borrowed for the call
    return RPTR_OK;
}
int rptr_hip_update_bones(rptr_hip_t *h, uint32_t first_bone, uint32_t count, const float *transforms12) {
    return update_bones_common(h, first_bone, count, transforms12, false);
}
int rptr_hip_update_bones_device(rptr_hip_t *h, uint32_t first_bone, uint32_t count, const float *device_transforms12) {
    return update_bones_common(h, first_bone, count, device_transforms12, true);
}
// every bound geometry's positions (and normal words) from its rest pose and the bone table, on the backend's stream; then what
// rptr_hip_update_vertices_device does per geometry
int rptr_hip_skin(rptr_hip_t *h) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "skin before set_scene");
    auto &sk = h->skin;
    auto &mo = h->morph;
    if (std::find(sk.bound.begin(), sk.bound.end(), (char)1) == sk.bound.end() && std::find(mo.bound.begin(), mo.bound.end(), (char)1) == mo.bound.end())
        return fail(h, RPTR_E_INVALID, "skin: no geometry is bound (rptr_hip_set_skin, rptr_hip_set_morph_targets)");
    if (h->ctx_scene.empty()) { // frames in flight read the master vertex buffer and tree
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    for (size_t g = 0; g < sk.bound.size(); ++g) {
        if (!sk.bound[g] && !mo.bound[g]) continue;
        const int rc0 = object_motion_before_update(h, (int)g);
        if (rc0) return rc0;
        const uint32_t n = 3u * h->geom_tris[g];
        if (n && !mo.bound[g])
            hipLaunchKernelGGL(rp_k_skin, dim3(grid_for(h, n)), dim3(256), 0, h->stream, reinterpret_cast<const uint4 *>(sk.records[g]), sk.rest_pos[g], sk.rest_nrm[g],
                               reinterpret_cast<const float4 *>(sk.d_bones), n, h->master.dynpos[g], h->master.dynnrm[g], sk.d_rejected);
        else if (n) { // morph targets, alone or in front of the skin (morph.h)
            const bool skinned = sk.bound[g] != 0, normals = sk.geom_normals[g] != 0;
            const dim3 grid(grid_for(h, n)), block(256);
            const uint4 *rec = skinned ? reinterpret_cast<const uint4 *>(sk.records[g]) : nullptr;
            const float4 *bones = skinned ? reinterpret_cast<const float4 *>(sk.d_bones) : nullptr;
#define RP_MORPH_LAUNCH(S, N)                                                                                                                          \
    hipLaunchKernelGGL((rp_k_morph<S, N>), grid, block, 0, h->stream, (const uint32_t *)mo.offsets[g], (const float4 *)mo.entries[g], (const float *)mo.weights[g], rec, \
                       (const float *)sk.rest_pos[g], (const uint32_t *)sk.rest_nrm[g], bones, n, h->master.dynpos[g], h->master.dynnrm[g], sk.d_rejected)
            if (skinned && normals) RP_MORPH_LAUNCH(true, true);
            else if (skinned) RP_MORPH_LAUNCH(true, false);
            else if (normals) RP_MORPH_LAUNCH(false, true);
            else RP_MORPH_LAUNCH(false, false);
#undef RP_MORPH_LAUNCH
        }
        HIP_TRY(h, hipGetLastError());
        h->master.mesh_dirty[(size_t)h->geom_mesh[g]] = 1;
        h->vertex_updates++;
        h->om.unrefitted = true;
    }
    return RPTR_OK;
}
int rptr_hip_readback_skinned(rptr_hip_t *h, uint32_t geometry, float *xyz, uint32_t *normal_words, uint32_t num_vertices) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "readback_skinned before set_scene");
    if (geometry >= h->skin.bound.size() || (!h->skin.bound[geometry] && !h->morph.bound[geometry] && !h->normals.bound[geometry]))
        return fail(h, RPTR_E_INVALID, "geometry %u has no skin (rptr_hip_set_skin) and no morph targets (rptr_hip_set_morph_targets) and no normal groups "
                                       "(rptr_hip_set_normal_groups)", geometry);
    if (num_vertices != 3u * h->geom_tris[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u has %u unrolled vertices, got %u", geometry, 3u * h->geom_tris[geometry], num_vertices);
    if (normal_words && !h->master.dynnrm[geometry]) return fail(h, RPTR_E_INVALID, "geometry %u has no normals", geometry);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (xyz && num_vertices) HIP_TRY(h, hipMemcpy(xyz, h->master.dynpos[geometry], (size_t)num_vertices * 12, hipMemcpyDeviceToHost));
    if (normal_words && num_vertices) HIP_TRY(h, hipMemcpy(normal_words, h->master.dynnrm[geometry], (size_t)num_vertices * 4, hipMemcpyDeviceToHost));
    return RPTR_OK;
}

// ---- morph targets (include/rptr_hip.h "morph targets", morph.h)
int rptr_hip_set_morph_targets(rptr_hip_t *h, uint32_t geometry, const RptrMorphTargetDesc *targets, uint32_t num_targets) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "set_morph_targets before set_scene");
    if (geometry >= h->master.dynpos.size() || !h->master.dynpos[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u does not belong to a dynamic mesh (RptrMeshDesc.dynamic)", geometry);
    if ((targets == nullptr) != (num_targets == 0)) return fail(h, RPTR_E_INVALID, "targets and num_targets must both be given, or NULL and 0 to unbind");
    if (num_targets > RPTR_MAX_MORPH_TARGETS)
        return fail(h, RPTR_E_INVALID, "%u morph targets, a geometry takes at most %d (RPTR_MAX_MORPH_TARGETS)", num_targets, RPTR_MAX_MORPH_TARGETS);
    const uint32_t n = 3u * h->geom_tris[geometry];
    auto &sk = h->skin;
    auto &mo = h->morph;
    const bool normals = sk.geom_normals[geometry] != 0;
    // ---- the host's checks and the transposition: per vertex its entries in ascending target order (a counting sort over the targets in order)
    std::vector<uint32_t> offsets((size_t)n + 1, 0);
    std::vector<float> entries;
    if (targets) {
        uint64_t total = 0;
        std::vector<uint32_t> seen_in(n, UINT32_MAX); // the last target that named the vertex
        for (uint32_t t = 0; t < num_targets; ++t) {
            const RptrMorphTargetDesc &T = targets[t];
            if (!T.deltas && T.num_deltas) return fail(h, RPTR_E_INVALID, "morph target %u: NULL deltas with num_deltas %u", t, T.num_deltas);
            if (T._pad) return fail(h, RPTR_E_INVALID, "morph target %u: _pad of its descriptor is not zero", t);
            for (uint32_t d = 0; d < T.num_deltas; ++d) {
                const RptrMorphDelta &D = T.deltas[d];
                if (D.vertex >= n) return fail(h, RPTR_E_INVALID, "morph target %u, delta %u: vertex %u, geometry %u has %u unrolled vertices", t, d, D.vertex, geometry, n);
                if (seen_in[D.vertex] == t) return fail(h, RPTR_E_INVALID, "morph target %u, delta %u: vertex %u appears twice in the target", t, d, D.vertex);
                seen_in[D.vertex] = t;
                for (int c = 0; c < 3; ++c)
                    if (!std::isfinite(D.dpos[c]) || !std::isfinite(D.dnrm[c])) return fail(h, RPTR_E_INVALID, "morph target %u, delta %u: a component is not finite", t, d);
                if (D._pad) return fail(h, RPTR_E_INVALID, "morph target %u, delta %u: _pad is not zero", t, d);
                offsets[(size_t)D.vertex + 1]++;
            }
            total += T.num_deltas;
        }
        if (total > UINT32_MAX) return fail(h, RPTR_E_INVALID, "%llu morph deltas: the entries of a geometry must fit 32 bits", (unsigned long long)total);
        for (uint32_t v = 0; v < n; ++v) offsets[(size_t)v + 1] += offsets[v];
        const size_t per = normals ? 8 : 4; // floats per entry
        entries.assign((size_t)total * per, 0.0f);
        std::vector<uint32_t> cursor(offsets.begin(), offsets.end() - 1);
        for (uint32_t t = 0; t < num_targets; ++t)
            for (uint32_t d = 0; d < targets[t].num_deltas; ++d) {
                const RptrMorphDelta &D = targets[t].deltas[d];
                float *e = entries.data() + (size_t)cursor[D.vertex]++ * per;
                e[0] = D.dpos[0], e[1] = D.dpos[1], e[2] = D.dpos[2];
                std::memcpy(e + 3, &t, sizeof(t)); // the target index as bits
                if (normals) e[4] = D.dnrm[0], e[5] = D.dnrm[1], e[6] = D.dnrm[2];
            }
    }
    // ---- checked: from here on the scene copies change, so nothing of the handle may still be rendering from them
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!targets) { // unbind: positions and normals stay as last written
        mo.bound[geometry] = 0;
        return RPTR_OK;
    }
    int rc;
    const bool capture = !sk.bound[geometry] && !mo.bound[geometry]; // (either deformer bound: the rest pose is the one it captured)
    mo.bound[geometry] = 0;
    if ((rc = skin_rejected_counter(h))) return rc;
    if (!mo.offsets[geometry] && (rc = dev_alloc(h, &mo.offsets[geometry], (size_t)n + 1, &h->scene_allocs))) return rc;
    const size_t n_entries = entries.size() / 4; // float4s
    if (!mo.entries[geometry] || mo.cap_entries[geometry] < n_entries) {
        if ((rc = dev_alloc(h, &mo.entries[geometry], n_entries, &h->scene_allocs))) return rc;
        mo.cap_entries[geometry] = n_entries;
    }
    if (!mo.weights[geometry] || mo.cap_weights[geometry] < num_targets) {
        if ((rc = dev_alloc(h, &mo.weights[geometry], num_targets, &h->scene_allocs))) return rc;
        mo.cap_weights[geometry] = num_targets;
    }
    HIP_TRY(h, hipMemcpy(mo.offsets[geometry], offsets.data(), offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_entries) HIP_TRY(h, hipMemcpy(mo.entries[geometry], entries.data(), entries.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(mo.weights[geometry], 0, (size_t)num_targets * sizeof(float)));
    if ((rc = skin_rest_pose(h, geometry, capture))) return rc;
    mo.num_targets[geometry] = num_targets;
    mo.bound[geometry] = 1;
    return RPTR_OK;
}
static int update_morph_weights_common(rptr_hip_t *h, uint32_t geometry, uint32_t first, uint32_t count, const float *weights, bool device_src) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "update_morph_weights before set_scene");
    auto &mo = h->morph;
    if (geometry >= mo.bound.size() || !mo.bound[geometry]) return fail(h, RPTR_E_INVALID, "geometry %u has no morph targets (rptr_hip_set_morph_targets)", geometry);
    if ((uint64_t)first + count > mo.num_targets[geometry])
        return fail(h, RPTR_E_INVALID, "morph weights [%u, +%u) are outside the %u targets of geometry %u", first, count, mo.num_targets[geometry], geometry);
    if (count == 0) return RPTR_OK;
    if (!weights) return fail(h, RPTR_E_INVALID, "NULL weights");
    if (!device_src)
        for (uint32_t i = 0; i < count; ++i)
            if (!std::isfinite(weights[i])) return fail(h, RPTR_E_INVALID, "morph weight %u (target %u) is not finite", i, first + i);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(mo.weights[geometry] + first, weights, (size_t)count * sizeof(float), device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!device_src) HIP_TRY(h, hipStreamSynchronize(h->stream)); // the host array is only borrowed for the call
    return RPTR_OK;
}
int rptr_hip_update_morph_weights(rptr_hip_t *h, uint32_t geometry, uint32_t first_target, uint32_t count, const float *weights) {
    return update_morph_weights_common(h, geometry, first_target, count, weights, false);
}
int rptr_hip_update_morph_weights_device(rptr_hip_t *h, uint32_t geometry, uint32_t first_target, uint32_t count, const float *device_weights) {
    return update_morph_weights_common(h, geometry, first_target, count, device_weights, true);
}

// ---- recomputed normals (include/rptr_hip.h "recomputed normals", normals.h)
int rptr_hip_set_normal_groups(rptr_hip_t *h, uint32_t geometry, const uint32_t *group, uint32_t num_vertices, uint32_t flags) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "set_normal_groups before set_scene");
    if (geometry >= h->master.dynpos.size() || !h->master.dynpos[geometry])
        return fail(h, RPTR_E_INVALID, "geometry %u does not belong to a dynamic mesh (RptrMeshDesc.dynamic)", geometry);
    if (!h->skin.geom_normals[geometry]) return fail(h, RPTR_E_INVALID, "geometry %u has no normals: there are no normal words to recompute", geometry);
    if ((group == nullptr) != (num_vertices == 0)) return fail(h, RPTR_E_INVALID, "group and num_vertices must both be given, or NULL and 0 to unbind");
    if (flags & ~RPTR_NORMALS_FLIP) return fail(h, RPTR_E_INVALID, "unknown flag bits 0x%x (RPTR_NORMALS_FLIP is the only flag)", flags & ~RPTR_NORMALS_FLIP);
    const uint32_t n = 3u * h->geom_tris[geometry];
    if (group && num_vertices != n) return fail(h, RPTR_E_INVALID, "geometry %u has %u unrolled vertices, got %u", geometry, n, num_vertices);
    // ---- the labels renumbered densely by first occurrence (every FLAT corner a group of its own), then transposed: per group its
    // member corners in ascending order (a counting sort over the corners in order)
    std::vector<uint32_t> offsets, members;
    uint32_t num_groups = 0;
    if (group) {
        std::vector<uint32_t> dense(n);
        std::unordered_map<uint32_t, uint32_t> id_of;
        id_of.reserve(n);
        for (uint32_t v = 0; v < n; ++v) {
            if (group[v] == RPTR_NORMAL_GROUP_FLAT) {
                dense[v] = num_groups++;
                continue;
            }
            const auto it = id_of.emplace(group[v], num_groups);
            if (it.second) ++num_groups;
            dense[v] = it.first->second;
        }
        offsets.assign((size_t)num_groups + 1, 0);
        for (uint32_t v = 0; v < n; ++v) offsets[(size_t)dense[v] + 1]++;
        for (uint32_t g = 0; g < num_groups; ++g) offsets[(size_t)g + 1] += offsets[g];
        members.resize(n);
        std::vector<uint32_t> cursor(offsets.begin(), offsets.end() - 1);
        for (uint32_t v = 0; v < n; ++v) members[cursor[dense[v]]++] = v;
    }
    // ---- checked: from here on the scene copies change, so nothing of the handle may still be rendering from them
    HIP_TRY(h, hipSetDevice(h->device));
    {
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto &nm = h->normals;
    if (!group) { // unbind: the normals stay as last written
        nm.bound[geometry] = 0;
        return RPTR_OK;
    }
    int rc;
    nm.bound[geometry] = 0;
    if (!nm.offsets[geometry] && (rc = dev_alloc(h, &nm.offsets[geometry], (size_t)n + 1, &h->scene_allocs))) return rc; // (at most one group per corner)
    if (!nm.members[geometry] && (rc = dev_alloc(h, &nm.members[geometry], n, &h->scene_allocs))) return rc;
    if (!nm.d_face || nm.cap_face < h->geom_tris[geometry]) {
        if ((rc = dev_alloc(h, &nm.d_face, h->geom_tris[geometry], &h->scene_allocs))) return rc;
        nm.cap_face = h->geom_tris[geometry];
    }
    HIP_TRY(h, hipMemcpy(nm.offsets[geometry], offsets.data(), offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n) HIP_TRY(h, hipMemcpy(nm.members[geometry], members.data(), members.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((rc = skin_rest_normals(h, geometry))) return rc; // dynnrm in every scene copy, from the uploaded words, and the mesh's table
    nm.num_groups[geometry] = num_groups;
    nm.flip[geometry] = (flags & RPTR_NORMALS_FLIP) ? 1 : 0;
    nm.bound[geometry] = 1;
    return RPTR_OK;
}
// every bound geometry's normal words from the master copy's current positions, on the backend's stream; then what
// rptr_hip_update_vertices_device does per geometry
int rptr_hip_recompute_normals(rptr_hip_t *h) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "recompute_normals before set_scene");
    auto &nm = h->normals;
    if (std::find(nm.bound.begin(), nm.bound.end(), (char)1) == nm.bound.end())
        return fail(h, RPTR_E_INVALID, "recompute_normals: no geometry is bound (rptr_hip_set_normal_groups)");
    if (h->ctx_scene.empty()) { // frames in flight read the master vertex buffer and tree
        int rc0 = drain(h);
        if (rc0) return rc0;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    for (size_t g = 0; g < nm.bound.size(); ++g) {
        if (!nm.bound[g]) continue;
        const int rc0 = object_motion_before_update(h, (int)g);
        if (rc0) return rc0;
        const uint32_t tris = h->geom_tris[g];
        if (tris) {
            hipLaunchKernelGGL(rp_k_face_normals, dim3(grid_for(h, tris)), dim3(256), 0, h->stream, (const float *)h->master.dynpos[g], tris, nm.d_face);
            hipLaunchKernelGGL(rp_k_group_normals, dim3(grid_for(h, nm.num_groups[g])), dim3(256), 0, h->stream, (const uint32_t *)nm.offsets[g],
                               (const uint32_t *)nm.members[g], (const float4 *)nm.d_face, nm.num_groups[g], (uint32_t)nm.flip[g], h->master.dynnrm[g]);
        }
        HIP_TRY(h, hipGetLastError());
        h->master.mesh_dirty[(size_t)h->geom_mesh[g]] = 1;
        h->vertex_updates++;
        h->om.unrefitted = true;
    }
    return RPTR_OK;
}

// ---- dynamic textures (include/rptr_hip.h "dynamic textures", texture_mips.h)
void rptr_hip_srgb_decode_table(float out256[256]) {
    if (out256) rp_srgb_decode_lut(out256);
}
// levels of the full chain of a w x h texture, down to 1 x 1
static uint32_t texture_full_levels(uint32_t w, uint32_t hh) {
    uint32_t full = 1;
    for (; w > 1 || hh > 1; w = std::max(1u, w / 2), hh = std::max(1u, hh / 2)) ++full;
    return full;
}
// texels in front of `level` in a texture's storage (the levels lie back to back); lw x lh: that level's size
static size_t texture_level_offset(uint32_t w, uint32_t hh, uint32_t level, uint32_t *lw, uint32_t *lh) {
    size_t at = 0;
    for (uint32_t l = 0; l < level; ++l, w = std::max(1u, w / 2), hh = std::max(1u, hh / 2)) at += (size_t)w * hh;
    *lw = w, *lh = hh;
    return at;
}
// what every call checks first: the handle, the scene, the index
static int texture_call_checks(const rptr_hip *ch, const char *what, uint32_t texture) {
    rptr_hip *h = const_cast<rptr_hip *>(ch); // (fail only writes the message)
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "%s before set_scene", what);
    if (texture >= h->tex.records.size()) return fail(h, RPTR_E_INVALID, "%s: texture %u is not a texture of this scene (%zu textures)", what, texture, h->tex.records.size());
    return RPTR_OK;
}
static int update_texture_common(rptr_hip_t *h, uint32_t texture, const uint8_t *rgba8, size_t n_bytes, uint32_t flags, bool device_src) {
    int rc;
    if ((rc = texture_call_checks(h, "update_texture", texture))) return rc;
    if (flags & ~RPTR_TEXTURE_GENERATE_MIPS)
        return fail(h, RPTR_E_INVALID, "update_texture: unknown flag bits 0x%x (RPTR_TEXTURE_GENERATE_MIPS is the only flag)", flags & ~RPTR_TEXTURE_GENERATE_MIPS);
    const bool generate = (flags & RPTR_TEXTURE_GENERATE_MIPS) != 0;
    RpTexture rec = h->tex.records[texture];
    const uint32_t w = (uint32_t)rec.width, hh = (uint32_t)rec.height;
    const size_t texels0 = (size_t)w * hh;
    if (!rgba8 && (n_bytes != 0 || !generate))
        return fail(h, RPTR_E_INVALID, "update_texture: texture %u: NULL texels keep level 0, which only (NULL, 0, RPTR_TEXTURE_GENERATE_MIPS) asks for", texture);
    if (rgba8 && n_bytes != 4 * texels0)
        return fail(h, RPTR_E_INVALID, "update_texture: texture %u is %u x %u: level 0 has %zu bytes, got %zu", texture, w, hh, 4 * texels0, n_bytes);
    if (h->tex.emissive[texture])
        return fail(h, RPTR_E_UNSUPPORTED, "update_texture: texture %u is read by a material with emission_intensity > 0: RptrSceneDesc.lights carry the radiance the "
                                           "host prepared from it, and next-event estimation would disagree with what paths see", texture);
    // ---- checked: every scene copy reads these texels, so nothing of the handle may still be rendering
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;
    const uint32_t full = texture_full_levels(w, hh);
    if (generate && rec.srgb && !h->tex.d_thresholds) {
        float lut[256], thr[256];
        rp_srgb_decode_lut(lut);
        rp_srgb_thresholds(lut, thr);
        if ((rc = dev_upload(h, &h->tex.d_thresholds, 256, thr, hipMemcpyHostToDevice, &h->scene_allocs))) return rc;
    }
    uint32_t lw, lh;
    const size_t need = generate ? texture_level_offset(w, hh, full, &lw, &lh) : texels0;
    if (need > h->tex.cap_texels[texture]) { // the first call that needs more room than set_scene allocated: one allocation for the full chain
        uchar4 *bigger = nullptr, *old = const_cast<uchar4 *>(rec.texels);
        if ((rc = dev_alloc(h, &bigger, need, &h->scene_allocs))) return rc;
        HIP_TRY(h, hipMemcpyAsync(bigger, old, texels0 * sizeof(uchar4), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (and whatever was queued in front of it: nothing reads the old block any more)
        (void)hipFree(old);
        h->scene_allocs.erase(std::remove(h->scene_allocs.begin(), h->scene_allocs.end(), (void *)old), h->scene_allocs.end());
        h->bytes_scene -= std::min(h->bytes_scene, std::max<size_t>(h->tex.cap_texels[texture], 1) * sizeof(uchar4));
        h->bytes_allocated = h->bytes_scene + h->bytes_frame;
        rec.texels = bigger;
        rec.levels = 1; // (only level 0 was carried over)
        h->tex.cap_texels[texture] = need;
        h->tex.records[texture] = rec;
        hipLaunchKernelGGL(rp_k_set_texture_record, dim3(1), dim3(64), 0, h->stream, h->tex.d_records + texture, rec); // the old block is gone: at once
        HIP_TRY(h, hipGetLastError());
    }
    uchar4 *level0 = const_cast<uchar4 *>(rec.texels);
    if (rgba8) {
        HIP_TRY(h, hipMemcpyAsync(level0, rgba8, n_bytes, device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        if (!device_src) HIP_TRY(h, hipStreamSynchronize(h->stream)); // the host array is only borrowed for the call
    }
    if (generate) { // level l + 1 from the quantised level l: one launch per level, in stream order
        uchar4 *src = level0;
        for (uint32_t l = 0, sw = w, sh = hh; l + 1 < full; ++l) {
            uchar4 *dst = src + (size_t)sw * sh;
            const uint32_t dw = std::max(1u, sw / 2), dh = std::max(1u, sh / 2);
            const bool pair = (sw & 1u) == 0 && ((uintptr_t)src & 7u) == 0;
            const dim3 grid(grid_for(h, (size_t)dw * dh));
            if (pair)
                hipLaunchKernelGGL(rp_k_mip_level<true>, grid, dim3(256), 0, h->stream, (const uchar4 *)src, dst, sw, sh, (uint32_t)rec.srgb, h->master.dscene.srgb_lut,
                                   (const float *)h->tex.d_thresholds);
            else
                hipLaunchKernelGGL(rp_k_mip_level<false>, grid, dim3(256), 0, h->stream, (const uchar4 *)src, dst, sw, sh, (uint32_t)rec.srgb, h->master.dscene.srgb_lut,
                                   (const float *)h->tex.d_thresholds);
            src = dst, sw = dw, sh = dh;
        }
    }
    // the record every scene copy reads, patched in place behind the texels: without the flag the texture is level 0 only, so no stale level
    // is ever sampled. Frames submitted from here on wait for the backend's stream (follow_master_scene), query runs are queued behind it
    // (on_callers_stream).
    rec.levels = generate ? (int)full : 1;
    hipLaunchKernelGGL(rp_k_set_texture_record, dim3(1), dim3(64), 0, h->stream, h->tex.d_records + texture, rec);
    HIP_TRY(h, hipGetLastError());
    h->tex.records[texture] = rec;
    return RPTR_OK;
}
int rptr_hip_update_texture(rptr_hip_t *h, uint32_t texture, const uint8_t *rgba8, size_t n_bytes, uint32_t flags) {
    return update_texture_common(h, texture, rgba8, n_bytes, flags, false);
}
int rptr_hip_update_texture_device(rptr_hip_t *h, uint32_t texture, const uint8_t *device_rgba8, size_t n_bytes, uint32_t flags) {
    return update_texture_common(h, texture, device_rgba8, n_bytes, flags, true);
}
int rptr_hip_texture_levels(const rptr_hip_t *h, uint32_t texture, uint32_t *out_levels) {
    int rc;
    if ((rc = texture_call_checks(h, "texture_levels", texture))) return rc;
    if (!out_levels) return fail(const_cast<rptr_hip *>(h), RPTR_E_INVALID, "NULL argument");
    *out_levels = (uint32_t)h->tex.records[texture].levels;
    return RPTR_OK;
}
// one level as the device holds it, behind whatever was queued on the backend's stream
int rptr_hip_readback_texture(rptr_hip_t *h, uint32_t texture, uint32_t level, uint8_t *rgba8, size_t n_bytes) {
    int rc;
    if ((rc = texture_call_checks(h, "readback_texture", texture))) return rc;
    const RpTexture &rec = h->tex.records[texture];
    if (level >= (uint32_t)rec.levels) return fail(h, RPTR_E_INVALID, "readback_texture: texture %u has %d levels, level %u is not one of them", texture, rec.levels, level);
    uint32_t lw, lh;
    const size_t at = texture_level_offset((uint32_t)rec.width, (uint32_t)rec.height, level, &lw, &lh);
    if (!rgba8 || n_bytes != 4 * (size_t)lw * lh)
        return fail(h, RPTR_E_INVALID, "readback_texture: level %u of texture %u is %u x %u: %zu bytes, got %zu%s", level, texture, lw, lh, 4 * (size_t)lw * lh, n_bytes,
                    rgba8 ? "" : " and a NULL array");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(rgba8, rec.texels + at, n_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RPTR_OK;
}
