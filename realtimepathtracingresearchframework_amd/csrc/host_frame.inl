// host_frame.inl -- a frame: camera basis, the bounce schedule of the path pipeline (queue_path_bounces: the ONE place that launches the path
// stages, for frames and for radiance-query runs), submitting a launch sequence (render_batch_impl and its steps), radiance-query runs
// (radiance_queries_on), collecting a frame (finish_frame), wait / render / stats
// Part of the ONE translation unit rptr_hip.hip (included there, in this order: host_state.h, host_bvh.inl, host_scene.inl,
// host_frame.inl, host_access.inl, host_queries.inl, host_comm.h): the host runtime split along its seams; no symbol changed.
// host part of a3: vulkan/render_vulkan.cpp:2880-2896
static void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - b[1] * a[2];
    o[1] = a[2] * b[0] - b[2] * a[0];
    o[2] = a[0] * b[1] - b[0] * a[1];
}
static void compute_view(const RptrCamera &c, int W, int H, RpFrame &f) {
    auto normalize = [](float v[3]) {
        float inv = 1.0f / sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        v[0] *= inv;
        v[1] *= inv;
        v[2] *= inv;
    };
    const float plane_y = 2.f * tanf((0.5f * c.fovy) * 0.01745329251994329576923690768489f);
    const float aspect = static_cast<float>(W) / H;
    const float plane_x = plane_y * aspect;
    float du[3], dv[3];
    cross3(c.dir, c.up, du);
    normalize(du);
    for (int k = 0; k < 3; ++k) du[k] *= plane_x;
    cross3(du, c.dir, dv);
    normalize(dv);
    for (int k = 0; k < 3; ++k) dv[k] = -dv[k] * plane_y;
    for (int k = 0; k < 3; ++k) {
        f.cam_pos[k] = c.pos[k];
        f.cam_du[k] = du[k];
        f.cam_dv[k] = dv[k];
        f.cam_dir_top_left[k] = c.dir[k] - 0.5f * du[k] - 0.5f * dv[k];
    }
}

// x / y / w rows of VP (render_vulkan.cpp:2926-2931): inverse of the camera-to-world matrix with columns cross(dir, up), up, -dir,
// pos; glm::infinitePerspective(radians(fovy), aspect, 0.5f) contributes P00 and P11 (GLM's published formulas)
static void compute_view_projection(const RptrCamera &c, int W, int H, float view[12], float proj[2]) {
    auto dot = [](const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    float cx[3], cz[3] = {-c.dir[0], -c.dir[1], -c.dir[2]}, r[3][3];
    cross3(c.dir, c.up, cx);
    cross3(c.up, cz, r[0]);
    cross3(cz, cx, r[1]);
    cross3(cx, c.up, r[2]);
    const float inv_det = 1.0f / dot(cx, r[0]);
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) r[k][j] *= inv_det;
        view[4 * k + 0] = r[k][0];
        view[4 * k + 1] = r[k][1];
        view[4 * k + 2] = r[k][2];
        view[4 * k + 3] = -dot(r[k], c.pos);
    }
    const float z_near = 0.5f, aspect = static_cast<float>(W) / H;
    const float range = tanf((c.fovy * 0.01745329251994329576923690768489f) / 2.0f) * z_near;
    const float left = -range * aspect, right = range * aspect, bottom = -range, top = range;
    proj[0] = (2.0f * z_near) / (right - left);
    proj[1] = (2.0f * z_near) / (top - bottom);
}

extern "C++" {
// Which instantiations of the path stages a launch sequence runs, and where it hands over to the tail kernel
struct PathKernelFlags {
    bool lights;    // light-sampling code: without emissive triangles and with all NEE probability on the sun that branch is dead code
    bool table_rng; // the general instantiations: a table point set, a screen jitter (raster TAA) or a lens (aperture_radius > 0) -- the shipped path carries none
    bool single;    // the top level holds one instance record
    bool full;      // the tail kernel's one instantiation for textured and alpha-tested scenes
    bool fast_math;
};
static PathKernelFlags path_kernel_flags(const rptr_hip *h, const RpScene &scene, const RpFrame &f) {
    PathKernelFlags k;
    k.lights = (h->num_lights > 0 && !h->lights_disabled) || f.sp.sun_radiance[3] < 1.0f;
    k.table_rng = h->rng_variant != RPTR_RNG_VARIANT_UNIFORM || h->params.enable_raster_taa != 0 || f.rp.aperture_radius > 0.0f;
    k.single = scene.single_instance != 0; // (the same in every copy: set_scene decides it before it copies the master's RpScene, nothing writes it later)
    k.full = h->uses_textures || h->uses_alpha;
    k.fast_math = h->opt.v[OPT_FAST_MATH] != 0;
    return k;
}
// the bounce at which the tail kernel takes over (kernels.h rp_k_tail; max_path_depth: never); counting keeps the stand-alone kernels
static int tail_hand_over(const rptr_hip *h, bool count_traversal) {
    const int depth = h->params.max_path_depth;
    if (h->tail_mode == 0 || count_traversal) return depth;
    return std::max(1, std::min(depth, h->tail_mode > 0 ? h->tail_mode : h->tail_adaptive));
}

// Where the launches of one submission put their timing spans: the context's event pool (from `cursor` on) and span list
struct StageTimer {
    FrameCtx *c;
    size_t cursor;
    int level; // stage_timing: 1 times kind 0 (closest-hit traversal) only, 2 every kind (host_state.h Span)
};
// (stream, kind, grid) -> the launch. When the level times this kind its start / stop events ride on the dispatch packet itself
// (launch.h rp_launch_kernel), no extra barrier packets in the queue -- the command processor's packet rate is what bounds small frames
// (profiles/r01_notes.md). timer == NULL: never timed.
static RpLaunch timed_launch(StageTimer *t, hipStream_t st, int kind, dim3 grid) {
    RpLaunch l = {grid, st, nullptr, nullptr};
    if (t && (t->level >= 2 || (t->level == 1 && kind == 0))) {
        l.start = next_event(*t->c, t->cursor);
        l.stop = next_event(*t->c, t->cursor);
        t->c->spans.push_back({l.start, l.stop, kind});
    }
    return l;
}

// One batch of paths through the pipeline: extend -> shade -> connect per bounce, then the tail launch. What differs between a frame
// (render_batch_impl) and a radiance-query run (radiance_queries_on):
struct PathRun {
    FrameCtx *c;          // whose path state, queues, counters and stack scratch are used
    const RpScene *scene; // the scene copy that is traced
    const RpFrame *f;     // (f->batch_spp sizes the first bounce's queue)
    int variant;
    hipStream_t stream;
    hipStream_t side;     // NULL: connect on `stream` with c->gstack; otherwise on this stream with c->gstack_side, next to the following extend
    int grids[4];         // traversal_grid kinds: first extend, later extends, connect, connect of a single-instance scene
    int grid_shade, grid_tail;
    bool count_traversal;
    int tail_from;             // the bounce the tail kernel takes over at (tail_hand_over)
    const RpQueries *queries;  // non-NULL: bounce 0 traces and shades the rays of the query buffer; NULL: the camera's
    StageTimer *timer;         // NULL: no timing spans
};
struct BounceLaunches {
    int extend = 0, connect = 0;
};
static int queue_path_bounces(rptr_hip *h, const PathRun &run, BounceLaunches &launched) {
    FrameCtx &c = *run.c;
    const RpScene &scene = *run.scene;
    const RpFrame &f = *run.f;
    const PathKernelFlags k = path_kernel_flags(h, scene, f);
    const bool alpha = h->uses_alpha, tex = h->uses_textures;
    HIP_TRY(h, hipMemsetAsync(c.counters, 0, sizeof(RpCounters), run.stream));
    // the first bounce's queue is the identity over the batch's path ids and is not stored (kernels.h)
    const uint32_t first_count = (uint32_t)((size_t)f.batch_spp * h->npix_padded);
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)&c.counters->bounce[0].queue_count, (int)first_count, 1, run.stream));
    for (int b = 0; b < h->params.max_path_depth; ++b) {
        const int in = b & 1, out = in ^ 1;
        RpBounceCounters *bc = &c.counters->bounce[b];
        const uint32_t *in_queue = b == 0 ? nullptr : c.queue[in];
        if (b == run.tail_from) { // the late bounces in one launch (kernels.h rp_k_tail)
            if (run.side && b > 0) HIP_TRY(h, hipStreamWaitEvent(run.stream, c.ev_side, 0)); // join: connect(b-1) on the side stream
            rp_launch_tail(run.variant, k.fast_math, timed_launch(run.timer, run.stream, 3, (unsigned)run.grid_tail), k.lights, k.full, k.single, k.table_rng, scene, f, c.ps,
                           c.sq, (const uint32_t *)c.queue[in], c.counters, b, c.gstack);
            break;
        }
        const RpLaunch l_extend = timed_launch(run.timer, run.stream, 0, (unsigned)run.grids[b == 0 ? 0 : 1]);
        if (b == 0 && run.queries)
            rp_launch_extend_query(l_extend, alpha, k.single, k.table_rng, scene, f, c.ps, *run.queries, bc, c.counters, c.gstack);
        else
            rp_launch_extend(l_extend, run.count_traversal, b == 0, alpha, k.single, k.table_rng, scene, f, c.ps, in_queue, bc, c.counters, c.gstack);
        launched.extend++;
        if (run.side && b > 0) HIP_TRY(h, hipStreamWaitEvent(run.stream, c.ev_side, 0)); // join: connect(b-1) wrote illum, frees the shadow queue
        const RpLaunch l_shade = timed_launch(run.timer, run.stream, 2, (unsigned)run.grid_shade);
        if (b == 0 && run.queries)
            rp_launch_shade_query(run.variant, k.fast_math, l_shade, k.lights, tex, k.table_rng, scene, f, c.ps, c.sq, (const uint32_t *)&bc->queue_count, c.queue[out],
                                  &c.counters->bounce[b + 1].queue_count, &bc->shadow_count, c.counters);
        else
            rp_launch_shade(run.variant, k.fast_math, l_shade, b == 0, k.lights, tex, k.table_rng, scene, f, c.ps, c.sq, in_queue, (const uint32_t *)&bc->queue_count,
                            c.queue[out], &c.counters->bounce[b + 1].queue_count, &bc->shadow_count, c.counters);
        if (run.side) { // fork: the side stream sees shade(b)
            HIP_TRY(h, hipEventRecord(c.ev_fork, run.stream));
            HIP_TRY(h, hipStreamWaitEvent(run.side, c.ev_fork, 0));
        }
        rp_launch_connect(timed_launch(run.timer, run.side ? run.side : run.stream, 1, (unsigned)run.grids[k.single ? 3 : 2]), run.count_traversal, alpha, k.single, scene, f,
                          c.ps, c.sq, bc, c.counters, run.side ? c.gstack_side : c.gstack);
        if (run.side) HIP_TRY(h, hipEventRecord(c.ev_side, run.side));
        launched.connect++;
    }
    if (run.side) HIP_TRY(h, hipStreamWaitEvent(run.stream, c.ev_side, 0)); // the last connect
    return RPTR_OK;
}

static void add_counters(RpCounters &dst, const RpCounters &c) {
    dst.rays_closest += c.rays_closest;
    dst.rays_shadow += c.rays_shadow;
    dst.nodes += c.nodes;
    dst.tris += c.tris;
    dst.nodes_shadow += c.nodes_shadow;
    dst.tris_shadow += c.tris_shadow;
    dst.hits_shaded += c.hits_shaded;
}

// read-backs of the image get, from here on, the one frame `which` of this context's batch produced (its context keeps a copy)
static void note_output(rptr_hip *h, FrameCtx &c, int which) {
    h->finished_serial++; // (a denoised image made from the frame waited for before is stale now: host_access.inl)
    if (h->ctx.size() > 1) {
        h->output_ctx = (int)(&c - h->ctx.data());
        h->output_index = std::max(which, 0);
        h->output_overwritten = false;
    }
}

// waits for the frame in flight on `c` and turns its events / counters into RptrStats
// `which`: the frame of the batch that is being collected (-1: all of them, stats dropped)
static int finish_frame(rptr_hip *h, FrameCtx &c, RptrStats *out_stats, int which = -1) {
    if (!c.pending) return fail(h, RPTR_E_INVALID, "no frame in flight on this context");
    const uint32_t all = c.batch_n >= 32 ? ~0u : ((1u << c.batch_n) - 1u);
    if (c.synced) { // a later frame of a batch whose end has been awaited already
        RptrStats st = c.batch_stats;
        st.spp = c.batch_spp_after[std::max(which, 0)];
        h->stats = st;
        if (out_stats) *out_stats = st;
        c.collected |= which < 0 ? all : (1u << which);
        if (c.collected == all) c.pending = false;
        note_output(h, c, which);
        return RPTR_OK;
    }
    // work queued on the backend's stream from here on (tile copies, read-backs) sees this frame: the host has waited for its end, so
    // nothing needs to be queued there. (A join on the backend's stream would sit in a hardware queue that it may share with another frame
    // context, behind that context's frame, and hold up the next frame's dependency event until that frame ends.)
    HIP_TRY(h, hipEventSynchronize(c.ev_end));
    c.synced = true;
    c.collected |= which < 0 ? all : (1u << which);
    if (c.collected == all) c.pending = false;
#ifdef RP_PROF
    {
        unsigned long long pr[16];
        HIP_TRY(h, rp_prof_exchange(pr)); // (the counters of the traversal kernels live in k_extend.hip's copy of rp_prof)
        fprintf(stderr, "[RP_PROF] node-phase cycles %llu wave-iters %llu lane-iters %llu phases %llu leaf-cycles %llu | cyc/wave-iter %.1f util %.3f iters/phase %.2f leafcyc/phase %.1f\n",
                pr[0], pr[1], pr[2], pr[3], pr[4], double(pr[0]) / double(pr[1] ? pr[1] : 1), double(pr[2]) / (64.0 * double(pr[1] ? pr[1] : 1)),
                double(pr[1]) / double(pr[3] ? pr[3] : 1), double(pr[4]) / double(pr[3] ? pr[3] : 1));
        fprintf(stderr, "[RP_PROF] lost lane-iterations: idle-at-entry %.3f leaf-at-entry %.3f dropped-out %.3f (fractions of 64*wave-iters)\n",
                double(pr[5]) / (64.0 * double(pr[1] ? pr[1] : 1)), double(pr[6]) / (64.0 * double(pr[1] ? pr[1] : 1)),
                double(pr[7]) / (64.0 * double(pr[1] ? pr[1] : 1)));
        fprintf(stderr, "[RP_PROF] time: node %.3g leaf %.3g refill+done %.3g | per phase: tri lanes %.2f (in %.2f of phases) instance lanes %.2f (in %.2f of phases)\n",
                double(pr[0]), double(pr[4]), double(pr[8]), double(pr[9]) / double(pr[3] ? pr[3] : 1), double(pr[11]) / double(pr[3] ? pr[3] : 1),
                double(pr[10]) / double(pr[3] ? pr[3] : 1), double(pr[12]) / double(pr[3] ? pr[3] : 1));
        fprintf(stderr, "[RP_PROF] leaf items: %llu triangle leaves, %llu instance entries (lane counts; per ray: divide by the frame's ray count)\n", pr[9], pr[10]);
        fprintf(stderr, "[RP_PROF] node iterations on the generic stack path (some lane within 3 entries of the end of its LDS stack): %.4f\n",
                double(pr[13]) / double(pr[1] ? pr[1] : 1));
    }
#endif
    RptrStats &st = h->stats;
    memset(&st, 0, sizeof(st));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c.ev_begin, c.ev_end);
    st.render_time_ms = ms;
    for (const Span &sp : c.spans) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, sp.a, sp.b);
        if (sp.kind == 0) st.extend_time_ms += t;
        else if (sp.kind == 1) st.connect_time_ms += t;
        else {
            st.shade_time_ms += t;
            if (sp.kind == 2) st.shade_only_time_ms += t;
            else if (sp.kind == 3) st.tail_time_ms += t;
            else if (sp.kind == 4) st.resolve_time_ms += t;
        }
    }
    RpCounters tot = c.earlier_batches;
    if (h->local_rows > 0) add_counters(tot, *c.host_counters);
    st.rays_closest = tot.rays_closest;
    st.rays_shadow = tot.rays_shadow;
    st.nodes_visited = tot.nodes + tot.nodes_shadow;
    st.tris_tested = tot.tris + tot.tris_shadow;
    st.nodes_closest = tot.nodes;
    st.tris_closest = tot.tris;
    st.hits_shaded = tot.hits_shaded;
    st.launches_extend = c.launches_extend;
    st.launches_connect = c.launches_connect;
    st.device_bytes_allocated = h->bytes_allocated;
    if (c.batch_n > 1) { // the frames of a batch share its launches: each reports an equal share
        const float inv = 1.0f / float(c.batch_n);
        st.render_time_ms *= inv;
        st.extend_time_ms *= inv;
        st.connect_time_ms *= inv;
        st.shade_time_ms *= inv;
        st.shade_only_time_ms *= inv;
        st.tail_time_ms *= inv;
        st.resolve_time_ms *= inv;
        for (uint64_t *v : {&st.rays_closest, &st.rays_shadow, &st.nodes_visited, &st.tris_tested, &st.hits_shaded, &st.nodes_closest, &st.tris_closest})
            *v /= (uint64_t)c.batch_n;
    }
    c.batch_stats = st;
    st.spp = c.batch_spp_after[std::max(which, 0)];
    note_output(h, c, which);
    h->aov_ctx = (int)(&c - h->ctx.data());
    h->aov_overwritten = false;
    if (h->local_rows > 0) {
        // where the next frame hands over to the tail kernel: the first bounce whose queue was short in this frame. Queue
        // lengths are known up to the bounce the tail took over at (it does not publish its block-local lists), so the
        // hand-over moves later by one bounce per frame at most
        const int depth = h->params.max_path_depth, used = std::min(c.tail_from, depth);
        int next = depth;
        for (int b = 1; b <= std::min(used, depth - 1); ++b)
            if (c.host_counters->bounce[b].queue_count <= (uint32_t)h->tail_threshold) {
                next = b;
                break;
            }
        if (next == depth && used < depth) // the tail's own queue was long: one bounce later, or (far too long) a frame without a tail to see all queues again
            next = c.host_counters->bounce[used].queue_count > 4u * (uint32_t)h->tail_threshold ? depth : std::min(depth, used + 1);
        h->tail_adaptive = next;
    }
    if (out_stats) *out_stats = st;
    return RPTR_OK;
}

// every frame in flight is waited for (its stats are dropped): before anything that touches shared state
static int drain(rptr_hip *h) {
    for (FrameCtx &c : h->ctx)
        if (c.pending) {
            int rc = finish_frame(h, c, nullptr);
            if (rc) return rc;
        }
    return RPTR_OK;
}
} // extern "C++"

int rptr_hip_render_async(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp, int reset_accumulation, int count_traversal,
                          uint64_t *out_ticket) {
    return rptr_hip_render_batch_async(h, camera, variant, spp, 1, reset_accumulation, 0, count_traversal, out_ticket);
}

extern "C++" {
static int render_batch_impl(rptr_hip_t *h, const RptrCamera *camera, bool per_frame_cameras, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                             int count_traversal, uint64_t *out_tickets);
}
int rptr_hip_render_batch_async(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                                int count_traversal, uint64_t *out_tickets) {
    return render_batch_impl(h, camera, false, variant, spp, n_frames, reset_first, reset_rest, count_traversal, out_tickets);
}
int rptr_hip_render_batch_cameras_async(rptr_hip_t *h, const RptrCamera *cameras, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                                        int count_traversal, uint64_t *out_tickets) {
    return render_batch_impl(h, cameras, n_frames > 1, variant, spp, n_frames, reset_first, reset_rest, count_traversal, out_tickets);
}

extern "C++" {
// camera: ONE camera for all frames of the sequence, or (per_frame_cameras) n_frames of them
// what a render call may ask of this handle (RPTR_E_INVALID with the reason otherwise)
static int check_render_arguments(rptr_hip_t *h, const RptrCamera *camera, bool per_frame_cameras, int variant, int spp, int n_frames) {
    if (!h || !camera) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (n_frames < 1) return fail(h, RPTR_E_INVALID, "n_frames must be >= 1");
    if (per_frame_cameras && n_frames > RP_BATCH_CAMS)
        return fail(h, RPTR_E_INVALID, "a launch sequence holds at most %d frames with cameras of their own", RP_BATCH_CAMS);
    if (n_frames > 1) {
        if (h->ctx.size() < 2) return fail(h, RPTR_E_INVALID, "batches of frames need frames_in_flight >= 2 (every frame of a batch keeps its own image)");
        if (n_frames > h->max_batch_frames) return fail(h, RPTR_E_INVALID, "a batch holds at most %d frames (option \"max_batch_frames\", read by rptr_hip_initialize)", h->max_batch_frames);
        if (n_frames * spp > h->max_batch_spp)
            return fail(h, RPTR_E_INVALID, "%d frames of %d samples do not fit the %d sample slots in flight (RPTR_PATH_BUDGET_MB)", n_frames, spp, h->max_batch_spp);
        if (h->freeze_frame) return fail(h, RPTR_E_INVALID, "a frozen frame cannot be batched with others");
    }
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "render before set_scene");
    if (h->width == 0) return fail(h, RPTR_E_INVALID, "render before initialize");
    if (variant != RPTR_VARIANT_GLTF && variant != RPTR_VARIANT_SIMPLE && variant != RPTR_VARIANT_GLTF_TRANSMISSION)
        return fail(h, RPTR_E_INVALID, "unknown variant %d", variant);
    if (spp < 1) return fail(h, RPTR_E_INVALID, "spp must be >= 1");
    // the thin lens (kernels.h rp_primary_ray_ex); aperture_radius == 0 checks nothing: hosts pass whatever focus_distance they like
    if (!(h->params.aperture_radius >= 0.0f) || !std::isfinite(h->params.aperture_radius))
        return fail(h, RPTR_E_INVALID, "aperture_radius must be finite and >= 0 (is %g)", (double)h->params.aperture_radius);
    if (h->params.aperture_radius > 0.0f && (!std::isfinite(h->params.focus_distance) || !(h->params.focus_distance > 0.0f)))
        return fail(h, RPTR_E_INVALID, "focus_distance must be finite and > 0 with aperture_radius > 0 (is %g)", (double)h->params.focus_distance);
    // reprojection_mode 2 (realtime_resolve.h) covers one frame per call on one device with the AOV images
    if (h->params.reprojection_mode == 2) {
        if (h->world > 1)
            return fail(h, RPTR_E_UNSUPPORTED, "reprojection_mode 2 needs world_size 1: the history of a stripe's edge pixels belongs to other ranks");
        if (n_frames > 1) return fail(h, RPTR_E_UNSUPPORTED, "reprojection_mode 2 renders one frame per call: batches of %d frames are not supported", n_frames);
        if (!h->aovs) return fail(h, RPTR_E_UNSUPPORTED, "reprojection_mode 2 reads the motion and normal + depth AOV images: option \"aovs\" is 0");
        if (h->params.spp_accumulation_window < 1) return fail(h, RPTR_E_INVALID, "reprojection_mode 2 needs spp_accumulation_window >= 1");
    }
    if (h->opt.v[OPT_TAA] != 0 && h->params.reprojection_mode != 0) {
        if (h->params.reprojection_mode != 2) return fail(h, RPTR_E_UNSUPPORTED, "option \"taa\" runs with reprojection_mode 2 only");
        if (h->params.render_upscale_factor != 1)
            return fail(h, RPTR_E_UNSUPPORTED, "option \"taa\" needs render_upscale_factor 1 (the frame buffer has the render resolution)");
    }
    return RPTR_OK;
}
// the frame constants of a launch sequence (RpFrame: render / scene / lighting parameters, the camera basis of frame 0 and -- per_frame_cameras --
// of every frame, the AOV view of the last frame, tiling and divisors, light bins, alpha test and point set); frame_id / sample bookkeeping is
// the caller's. note_view: the last camera becomes the previous view of the next frame's motion vectors (a frame's does, a query run's does not)
static void fill_frame_constants(rptr_hip_t *h, FrameCtx &c, const RptrCamera *camera, bool per_frame_cameras, int variant, int spp, int n_frames, int reset_rest, bool note_view,
                                 RpFrame &f) {
    memset(&f, 0, sizeof(f));
    f.rp = h->params;
    f.sp = h->scene_params;
    f.lc = h->lighting;
    compute_view(camera[0], h->width, h->height, f);
    if (per_frame_cameras) { // every frame of the sequence looks through its own camera (kernels.h rp_primary_ray_ex: the general instantiation)
        f.per_frame_cams = 1;
        for (int k = 0; k < n_frames; ++k) {
            RpFrame t;
            compute_view(camera[k], h->width, h->height, t);
            memcpy(f.cams[k].pos, t.cam_pos, sizeof(t.cam_pos));
            memcpy(f.cams[k].du, t.cam_du, sizeof(t.cam_du));
            memcpy(f.cams[k].dv, t.cam_dv, sizeof(t.cam_dv));
            memcpy(f.cams[k].dir_top_left, t.cam_dir_top_left, sizeof(t.cam_dir_top_left));
        }
    }
    {
        // the AOV images are those of the LAST frame of the sequence: its view, and as VP_reference the view of the frame before it (the
        // previous submission's last camera when the sequence is one frame)
        const RptrCamera &last = camera[per_frame_cameras ? n_frames - 1 : 0];
        const RptrCamera &before = n_frames > 1 ? camera[per_frame_cameras ? n_frames - 2 : 0] : (h->have_prev_camera ? h->prev_camera : last);
        compute_view_projection(last, h->width, h->height, f.view, f.proj);
        compute_view_projection(before, h->width, h->height, f.view_ref, f.proj_ref);
        memcpy(f.aov_cam_pos, last.pos, sizeof(f.aov_cam_pos));
        if (note_view) {
            h->prev_camera = last;
            h->have_prev_camera = true;
        }
    }
    f.aov_albedo_roughness = c.aov[0];
    f.aov_normal_depth = c.aov[1];
    f.aov_motion_jitter = c.aov[2];
    f.frame_offset = h->frame_offset;
    f.batch_frames = n_frames;
    f.frame_spp = spp;
    f.batch_reset = reset_rest ? 1 : 0;
    f.div_frame_spp = rp_make_div((uint32_t)spp);
    f.out_stride = (size_t)h->width * (size_t)std::max(h->local_rows, 1);
    f.variant = variant;
    f.width = h->width;
    f.height = h->height;
    f.local_rows = h->local_rows;
    f.tiles_x = h->tiles_x;
    f.tiles_y = h->tiles_y;
    f.npix_padded = h->npix_padded;
    f.rank = h->rank;
    f.world = h->world;
    f.stripe_rows = h->stripe_rows;
    f.div_npix_padded = rp_make_div((uint32_t)h->npix_padded);
    f.div_tiles_x = rp_make_div((uint32_t)(h->tiles_x / RP_TILE_BLOCK));
    f.div_stripe_rows = rp_make_div((uint32_t)h->stripe_rows);
    f.div_width = rp_make_div((uint32_t)h->width);
    f.num_bins = (h->num_lights + (h->lighting.bin_size - 1)) / h->lighting.bin_size;
    if (h->lights_disabled || h->num_lights == 0) { // LIGHT_SAMPLING_VARIANT_NONE (rendering/mc/nee.glsl:12-14): every NEE sample goes to the sun
        // the adapter hands sun_radiance.w = 1 with this variant (vulkan/render_sky.cpp:67-70: light_count is 0 without the binned-lights
        // extension); emitters that are HIT keep their full weight: pdf of picking them = (1 - 1) / (bins x solid angle) with a bin count
        // that must not be zero for that product to be 0 rather than NaN.
        // A scene without lights gets the same rule whatever sun weight scene_params carries (the same file hands w = 1 when light_count
        // == 0): with a weight below 1 the light-sampling kernels would choose bin -1 of 0 and read in front of the light table
        f.num_bins = std::max(f.num_bins, 1);
        f.sp.sun_radiance[3] = 1.0f;
    }
    // north_star's regrouping of rays by material lives INSIDE the shade kernel's LDS compaction (kernels.h rp_shade_body, RPTR_REGROUP=1):
    // measured on C3 with 48 textured materials it costs 6 % of the shade time and gains nothing (every material runs the same BSDF code),
    // so it is off unless asked for. The separate counting-sort pass of rounds 1-2 (rp_k_sort_*: three launches per bounce, one frame
    // context only, 0.4 ms per frame) lost on every configuration and is gone (profiles/r03_notes.md section 6).
    f.regroup_materials = h->opt.v[OPT_REGROUP] != 0 ? 1 : 0;
    f.alpha_test = h->uses_alpha ? 1 : 0;
    f.rng_variant = h->rng_variant;
    f.rng_table = h->rng_table;
}
// ---- the steps of render_batch_impl, in the order it takes them
// reprojection_mode 2: the images of realtime_resolve.h, made by the first frame that needs them
static int ensure_realtime_images(rptr_hip_t *h, bool taa) {
    const size_t npix = (size_t)h->width * (size_t)h->local_rows;
    int rc = RPTR_OK;
    if (!h->rt.cur) {
        if ((rc = dev_alloc(h, &h->rt.cur, npix, nullptr)) || (rc = dev_alloc(h, &h->rt.accum_other, npix, nullptr)) ||
            (rc = dev_alloc(h, &h->rt.nd[0], npix, nullptr)) || (rc = dev_alloc(h, &h->rt.nd[1], npix, nullptr)))
            return rc;
        h->rt.chain = false;
    }
    if (taa && !h->rt.fb_pre) {
        if ((rc = dev_alloc(h, &h->rt.fb_pre, npix, nullptr)) || (rc = dev_alloc(h, &h->rt.fb_other, npix, nullptr))) return rc;
    }
    return RPTR_OK;
}
// The traversal grids of the frame submitted on `c`, and whether its shadow rays go to the side stream, for the frames of this handle that
// will share the GPU with it: those still in flight on the device (up to the most that can run side by side). A frame alone gets the full
// grids (and, when the library chose side streams, its side stream); counted frames are launched as frames side by side are.
static void plan_frame_grids(rptr_hip_t *h, FrameCtx &c, int count_traversal, int grids[4], bool *side) {
    int concurrency = 1;
    for (FrameCtx &o : h->ctx)
        if (concurrency < h->max_concurrency && &o != &c && o.pending && !o.synced && hipEventQuery(o.ev_end) != hipSuccess) ++concurrency;
    const bool alone = concurrency == 1;
    *side = c.side != nullptr && !(h->side_only_alone && !alone);
    if (count_traversal) concurrency = h->max_concurrency;
    for (int kind = 0; kind < 4; ++kind) h->last_grids[kind] = grids[kind] = traversal_grid(h, kind, concurrency);
}
// The context's scene follows the master, behind whatever the caller queued on the backend's stream
static int follow_master_scene(rptr_hip_t *h, FrameCtx &c, SceneCopy &scn) {
    const bool follow = !h->ctx_scene.empty() && scn.version != h->refit_version;
    if (follow) {
        // this context's own vertices follow the master set: the copy of the float positions is queued on the backend's stream,
        // behind the caller's updates (this context is idle, the others keep rendering from their own sets)
        for (size_t gi = 0; gi < scn.dynpos.size(); ++gi)
            if (scn.dynpos[gi])
                HIP_TRY(h, hipMemcpyAsync(scn.dynpos[gi], h->master.dynpos[gi], (size_t)h->geom_tris[gi] * 9 * sizeof(float), hipMemcpyDeviceToDevice,
                                          h->stream));
        for (size_t gi = 0; gi < scn.dynnrm.size(); ++gi) // ... with the skinned normal words of the geometries that have them (skin.h)
            if (scn.dynnrm[gi])
                HIP_TRY(h, hipMemcpyAsync(scn.dynnrm[gi], h->master.dynnrm[gi], (size_t)h->geom_tris[gi] * 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                          h->stream));
        if (scn.inst_version != h->inst_version && h->num_instances) // ... and so do the staged instance transforms (rptr_hip_update_instances)
            HIP_TRY(h, hipMemcpyAsync(scn.inst_xf, h->master.inst_xf, (size_t)96 * h->num_instances, hipMemcpyDeviceToDevice, h->stream));
    }
    // whatever the caller queued on the backend's stream (vertex updates, the copy above) comes first. When that stream has nothing
    // unfinished there is nothing to wait for, and no event is recorded: an event on a stream that shares its hardware queue with another
    // frame context completes only after that context's frame, and would serialise the frames in flight.
    if (h->ctx.size() > 1 && hipStreamQuery(h->stream) != hipSuccess) {
        HIP_TRY(h, hipEventRecord(c.ev_dep, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(c.stream, c.ev_dep, 0));
    }
    if (follow) { // ... and its tree is refitted on its OWN stream: the refits of different contexts run side by side
        int err = RPTR_OK;
        (void)refit_scene_copy(h, scn, true, c.stream, &err);
        scn.version = h->refit_version;
        // a rebuild that could not start (no memory for its work space): the tree was refitted on its old topology, so this context is
        // consistent and the frame is rendered on it; the next refit tries again. The caller can tell: rptr_hip_bvh_rebuild_count does not
        // advance, and the failures are counted (rptr_hip_get_option(h, "bvh_rebuild_failures"))
        if (err != RPTR_OK) h->rebuild_failures++;
    }
    return RPTR_OK;
}
// The resolve of one internal batch and, in reprojection_mode 2 after the
// frame's last batch (spp: the frame's), the reprojection and TAA passes; resolves run in submission order across the contexts
static int queue_resolve(rptr_hip_t *h, FrameCtx &c, const RpFrame &f, StageTimer *timer, bool realtime, bool last_batch, int spp, bool taa_now) {
    const bool multi = h->ctx.size() > 1;
    // resolves fold into one history buffer: they run in submission order across the contexts
    if (multi && h->last_resolved && h->last_resolved != c.ev_resolved) HIP_TRY(h, hipStreamWaitEvent(c.stream, h->last_resolved, 0));
    const RpLaunch l_resolve = timed_launch(timer, c.stream, 4, (unsigned)grid_for(h, (size_t)h->width * h->local_rows));
    if (!realtime)
        rp_launch_kernel(l_resolve, rp_k_resolve, 256u, f, c.ps, h->accum, h->fb, c.out_accum, c.out_fb);
    else // the mean of this frame's samples (kernels_misc.h), then, after its last batch, the reprojection (and TAA) passes
        rp_launch_kernel(l_resolve, rp_k_resolve, 256u, f, c.ps, h->rt.cur, (uchar4 *)nullptr, (float4 *)nullptr, (uchar4 *)nullptr);
    if (realtime && last_batch) {
        RpReprojectArgs ra;
        ra.cur = h->rt.cur;
        ra.nd = c.aov[1];
        ra.mj = c.aov[2];
        ra.hist = h->accum;
        ra.hist_nd = h->rt.nd[h->rt.parity];
        ra.accum = h->rt.accum_other;
        ra.out_nd = h->rt.nd[h->rt.parity ^ 1];
        ra.fb = taa_now ? h->rt.fb_pre : h->fb;
        ra.fb_keep = h->fb;
        ra.out_accum = c.out_accum;
        ra.out_fb = c.out_fb; // (with TAA, rp_k_taa overwrites it with the frame after the pass)
        ra.min_sample_weight = 1.0f / float(h->params.spp_accumulation_window);
        ra.sample_batch_size = spp;
        ra.use_history = (f.frame_id > 0 && h->rt.chain) ? 1 : 0;
        const dim3 tiles((unsigned)((h->width + RP_RT_TILE - 1) / RP_RT_TILE), (unsigned)((h->local_rows + RP_RT_TILE - 1) / RP_RT_TILE));
        rp_launch_kernel(timed_launch(timer, c.stream, 4, tiles), rp_k_reproject, 64u, f, ra);
        std::swap(h->accum, h->rt.accum_other);
        h->rt.parity ^= 1;
        if (taa_now) {
            rp_launch_kernel(timed_launch(timer, c.stream, 4, tiles), rp_k_taa, 64u, f, (const uchar4 *)h->rt.fb_pre, (const uchar4 *)h->fb, (const uint2 *)c.aov[2],
                             h->rt.fb_other, c.out_fb);
            std::swap(h->fb, h->rt.fb_other);
        }
    }
    if (multi) { // (the resolve also kept a copy of the image this frame produced: the next frame's resolve overwrites the shared buffers)
        HIP_TRY(h, hipEventRecord(c.ev_resolved, c.stream));
        h->last_resolved = c.ev_resolved;
    }
    return RPTR_OK;
}
// The counters of one internal batch come back to the host; between batches the host waits for them
static int read_back_counters(rptr_hip_t *h, FrameCtx &c, bool more_batches) {
    HIP_TRY(h, hipMemcpyAsync(c.host_counters, c.counters, sizeof(RpCounters), hipMemcpyDeviceToHost, c.stream));
    // the host copy above must land before the next batch's memset: batches are few, sync here
    if (more_batches) {
        HIP_TRY(h, hipStreamSynchronize(c.stream));
        add_counters(c.earlier_batches, *c.host_counters);
        memset(c.host_counters, 0, sizeof(RpCounters));
    }
    return RPTR_OK;
}
// The end of the submission: the sample counts of a batch's frames, the end event, the tickets
static int close_submission(rptr_hip_t *h, FrameCtx &c, int spp, int n_frames, int reset_rest, bool realtime, uint32_t frame_id_before, uint64_t *out_tickets) {
    c.batch_spp_after[0] = h->accumulated_spp;
    if (n_frames > 1) { // begin_frame / end_frame of every frame of the batch (kernels: dshade.h rp_slot_frame)
        for (int k = 0; k < n_frames; ++k) {
            if (k > 0 && reset_rest) {
                h->frame_offset += h->frame_id;
                h->frame_id = 0;
            }
            h->frame_id += (uint32_t)spp;
            h->accumulated_spp = (int)h->frame_id;
            c.batch_spp_after[k] = h->accumulated_spp;
        }
    }
    h->rt.chain = realtime; // what this frame left is the next frame's history in mode 2 only
    HIP_TRY(h, hipEventRecord(c.ev_end, c.stream));
    HIP_TRY(h, hipGetLastError());
    if (h->freeze_frame) h->frame_id = frame_id_before; // end_frame, render_vulkan.cpp:2152-2154: the next frame repeats these samples
    c.spp_after = h->accumulated_spp;
    c.pending = true;
    c.synced = false;
    c.collected = 0;
    c.batch_n = n_frames;
    c.ticket = h->next_ticket;
    h->next_ticket += (uint64_t)n_frames;
    if (out_tickets)
        for (int k = 0; k < n_frames; ++k) out_tickets[k] = c.ticket + (uint64_t)k;
    return RPTR_OK;
}

static int render_batch_impl(rptr_hip_t *h, const RptrCamera *camera, bool per_frame_cameras, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                             int count_traversal, uint64_t *out_tickets) {
    int rc = check_render_arguments(h, camera, per_frame_cameras, variant, spp, n_frames);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    FrameCtx &c = h->ctx[(size_t)h->next_ctx];
    if (c.pending)
        return fail(h, RPTR_E_INVALID, "all %zu frames in flight are busy: rptr_hip_wait for ticket %llu first", h->ctx.size(),
                    (unsigned long long)c.ticket);
    h->next_ctx = (h->next_ctx + 1) % (int)h->ctx.size();
    if (h->ctx.size() > 1) { // this context's images are about to be rewritten: what was queued on the backend's stream so far still sees the old
                             // ones (ev_dep, follow_master_scene), a read-back issued after this submission would not
        if ((int)(&c - h->ctx.data()) == h->output_ctx) h->output_overwritten = true;
        if ((int)(&c - h->ctx.data()) == h->aov_ctx) h->aov_overwritten = true;
    }
    // begin_frame: render_vulkan.cpp:1937-1941
    if (reset_first) {
        if (!h->freeze_frame) h->frame_offset += h->frame_id;
        h->frame_id = 0;
    }
    const uint32_t frame_id_before = h->frame_id;
    const bool realtime = h->params.reprojection_mode == 2 && h->local_rows > 0;
    const bool taa = realtime && h->opt.v[OPT_TAA] != 0;
    if (realtime && (rc = ensure_realtime_images(h, taa))) return rc;
    RpFrame f;
    fill_frame_constants(h, c, camera, per_frame_cameras, variant, spp, n_frames, reset_rest, true, f);
    f.frame_id = h->frame_id; // the whole call is one frame of the reference (its batch_spp = spp), whatever the internal batches
    c.spans.clear();
    StageTimer timer = {&c, 0, h->stage_timing};
    SceneCopy &scn = h->ctx_scene.empty() ? h->master : h->ctx_scene[(size_t)(&c - h->ctx.data())];
    PathRun run = {};
    run.c = &c;
    run.scene = &scn.dscene;
    run.f = &f;
    run.variant = variant;
    run.stream = c.stream;
    bool side = false;
    plan_frame_grids(h, c, count_traversal, run.grids, &side);
    run.side = side ? c.side : nullptr;
    run.grid_shade = grid_for(h, h->path_capacity);
    run.grid_tail = h->tail_blocks;
    run.count_traversal = count_traversal != 0;
    run.timer = &timer;
    if ((rc = follow_master_scene(h, c, scn))) return rc;
    if (c.gather_pending) { // the image this context produced last is still being sent to rank 0 (host_comm.h)
        HIP_TRY(h, hipStreamWaitEvent(c.stream, c.ev_gather, 0));
        c.gather_pending = false;
    }
    HIP_TRY(h, hipEventRecord(c.ev_begin, c.stream));
    BounceLaunches launched;
    memset(&c.earlier_batches, 0, sizeof(c.earlier_batches));
    memset(c.host_counters, 0, sizeof(RpCounters));
    int remaining = spp * n_frames; // (n_frames > 1: one internal batch holds them all, checked above)
    while (remaining > 0) {
        const int batch = std::min(remaining, h->max_batch_spp);
        f.sample_base = h->frame_id;
        f.batch_spp = batch;
        if (h->local_rows > 0) {
            c.tail_from = run.tail_from = tail_hand_over(h, run.count_traversal);
            if ((rc = queue_path_bounces(h, run, launched))) return rc;
            // process_taa.cpp:92 reads frame_id after end_frame: this call's samples included
            const bool taa_now = taa && frame_id_before + (uint32_t)spp > 1u;
            if ((rc = queue_resolve(h, c, f, &timer, realtime, remaining - batch == 0, spp, taa_now))) return rc;
            if ((rc = read_back_counters(h, c, remaining - batch > 0))) return rc;
        }
        // end_frame: render_vulkan.cpp:2152-2154
        if (n_frames == 1) {
            h->accumulated_spp = int(h->frame_id) + batch;
            h->frame_id += (uint32_t)batch;
        }
        remaining -= batch;
    }
    c.launches_extend = launched.extend;
    c.launches_connect = launched.connect;
    if (h->om.enabled) { // object motion: the frame constants stay with the context, the interval of staged updates ends
        c.last_frame = f;
        c.last_submission = ++h->om.submissions;
        h->om.dirty[1] = h->om.dirty[0];
        h->om.dirty[0] = h->om.unrefitted;
        h->om.staged_since_submission = false;
        h->om.last_frames = n_frames;
    }
    return close_submission(h, c, spp, n_frames, reset_rest, realtime, frame_id_before, out_tickets);
}
} // extern "C++"

extern "C++" {
// ---- radiance queries (kernels.h RpQueries): the path pipeline on the rays of a query buffer instead of the camera's
// (RenderBackend::render_ray_queries with a path-tracing variant: render_vulkan.cpp:1867-1876, 2961-3059)
// Queues the run on `st` for DEVICE buffers. The caller has begun a query run (host_queries.inl begin_query_run: what is borrowed from
// context 0); everything a frame owns is left alone (accumulation and frame buffers, AOV images, frame_id, frame_offset, the previous view,
// the last frame's statistics and hand-over bounce).
// The virtual image (width = the frame's, query q = pixel (q mod W, q div W)) is walked in slices of at most the frame's rows, the samples
// of a slice in batches of at most the context's sample slots; a path's result is a function of its query and sample index alone, so
// neither shows in the results. Sample s runs as a one-sample frame at that point of the accumulation would: sample_index = frame_id =
// first_sample + s (frame_id seeds the alpha test of shadow rays and the blue-noise point set) -- one call of k samples and k calls of one
// give the same bits.
// totals != NULL: the ray counters of every batch are added to it (the host waits for each batch); NULL: nothing is waited for.
// fresh (a probe run, host_queries.inl): the fold into `dr` counts from 0 instead of first_sample -- the mean of this run's samples alone.
static int radiance_queries_on(rptr_hip_t *h, const RptrRenderRayQuery *dq, int n, const RptrCamera *camera, int variant, int spp, int first_sample, float4 *dr,
                               hipStream_t st, RpCounters *totals, bool fresh = false) {
    if (n == 0) return RPTR_OK;
    FrameCtx &c = h->ctx[0];
    RpFrame f;
    fill_frame_constants(h, c, camera, false, variant, 1, 1, 0, false, f);
    f.rp.aperture_radius = 0.0f; // a query's own origin and direction replace the camera ray, lens included (raygen.rgen:162-168): the same kernels, the same bits
    f.aov_albedo_roughness = f.aov_normal_depth = f.aov_motion_jitter = nullptr;
    const int slice_rows = h->local_rows; // (world_size 1: the frame's height)
    f.world = 1;
    f.stripe_rows = slice_rows;
    f.div_stripe_rows = rp_make_div((uint32_t)slice_rows);
    const RpQueries rq = {dq, (uint32_t)n, fresh ? RP_QUERIES_FRESH | (uint32_t)first_sample : 0u};
    PathRun run = {};
    run.c = &c;
    run.scene = &h->master.dscene;
    run.f = &f;
    run.variant = variant;
    run.stream = st;
    for (int kind = 0; kind < 4; ++kind) run.grids[kind] = traversal_grid(h, kind, 1); // (nothing else of this handle is on the GPU: the grids of a frame alone)
    run.grid_shade = grid_for(h, h->path_capacity);
    run.grid_tail = h->tail_blocks;
    run.tail_from = tail_hand_over(h, false);
    run.queries = &rq;
    BounceLaunches launched; // (a frame's statistic: dropped)
    const long long total_rows = ((long long)n + h->width - 1) / h->width;
    for (long long row0 = 0; row0 < total_rows; row0 += slice_rows) {
        f.rank = (int)(row0 / slice_rows);
        f.local_rows = (int)std::min<long long>(slice_rows, total_rows - row0);
        for (int done = 0; done < spp;) {
            const int batch = std::min(spp - done, h->max_batch_spp);
            f.sample_base = (uint32_t)(first_sample + done);
            f.frame_id = f.sample_base;
            f.batch_spp = batch;
            f.batch_frames = batch; // one "frame" per sample slot (dshade.h rp_slot_frame): frame_id = sample_index
            const int rc = queue_path_bounces(h, run, launched);
            if (rc) return rc;
            hipLaunchKernelGGL(rp_k_resolve_queries, dim3(grid_for(h, (size_t)h->width * (size_t)f.local_rows)), dim3(256), 0, st, f, c.ps, rq, dr);
            HIP_TRY(h, hipGetLastError());
            if (totals) {
                HIP_TRY(h, hipMemcpyAsync(c.host_counters, c.counters, sizeof(RpCounters), hipMemcpyDeviceToHost, st));
                HIP_TRY(h, hipStreamSynchronize(st));
                add_counters(*totals, *c.host_counters);
            }
            done += batch;
        }
    }
    return RPTR_OK;
}
} // extern "C++"

int rptr_hip_wait(rptr_hip_t *h, uint64_t ticket, RptrStats *out_stats) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    for (FrameCtx &c : h->ctx)
        if (c.pending && ticket >= c.ticket && ticket < c.ticket + (uint64_t)c.batch_n) {
            const int which = (int)(ticket - c.ticket);
            if (c.collected & (1u << which)) break; // waited for already
            return finish_frame(h, c, out_stats, which);
        }
    return fail(h, RPTR_E_INVALID, "ticket %llu is not in flight", (unsigned long long)ticket);
}

int rptr_hip_render(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp, int reset_accumulation, int count_traversal,
                    RptrStats *out_stats) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    int rc = drain(h); // a synchronous frame goes behind whatever is still in flight
    if (rc) return rc;
    uint64_t ticket = 0;
    if ((rc = rptr_hip_render_async(h, camera, variant, spp, reset_accumulation, count_traversal, &ticket))) return rc;
    return rptr_hip_wait(h, ticket, out_stats);
}

int rptr_hip_stats(const rptr_hip_t *h, RptrStats *out) {
    if (!h || !out) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    *out = h->stats;
    return RPTR_OK;
}

