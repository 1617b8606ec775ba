// host_queries.inl -- ray queries, four kinds behind ten entry points: closest hits (rptr_hip_trace, _trace_counted, _trace_device,
// _render_ray_queries), path-traced radiance (rptr_hip_trace_radiance, _trace_radiance_device, _render_radiance_queries; the run itself is
// host_frame.inl radiance_queries_on), surface records (rptr_hip_trace_surface, _trace_surface_device) and occlusion bits
// (rptr_hip_trace_occlusion, _trace_occlusion_device); and the irradiance probes built on the radiance kind (probes.h:
// rptr_hip_trace_probes, _trace_probes_device, their two stages). What the kinds share stands here once: the run preamble, the borrowed
// pool cursor, the staging of host arrays, the budget of the backend's own buffers, the checks.
// Part of the ONE translation unit rptr_hip.hip (included there after host_access.inl).
extern "C++" {
// A query run borrows context 0 and nothing a frame owns: the traversals take its stack scratch and, as their pool cursor, its
// counters->bounce[0].cursor_extend (borrowed_cursor); a radiance run takes its path state, queues and counters as well. So the frames in
// flight are drained first, and a run never overlaps a frame. Every entry point starts here, after its argument checks.
static int begin_query_run(rptr_hip *h) {
    int rc = drain(h);
    if (rc || (rc = ensure_master_tree(h))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return RPTR_OK;
}
// the pool cursor of a traversal over queries, set to zero on `st` ahead of the launch that follows
static uint32_t *borrowed_cursor(rptr_hip *h, hipStream_t st) {
    uint32_t *cursor = &h->ctx[0].counters->bounce[0].cursor_extend;
    hipLaunchKernelGGL(rp_k_reset_u32, dim3(1), dim3(1), 0, st, cursor);
    return cursor;
}
// the device buffers of rptr_hip_enable_ray_queries hold rq_capacity queries and results
static int check_query_budget(rptr_hip *h, int n) {
    if ((size_t)n > h->rq_capacity) return fail(h, RPTR_E_INVALID, "%d ray queries exceed the budget of %zu (rptr_hip_enable_ray_queries)", n, h->rq_capacity);
    return RPTR_OK;
}
// queue(st) on the stream the caller named (NULL: the backend's). A stream of the caller's sees the scene uploads / refits queued on the
// backend's, and later frames see what was queued
template <class F>
static int on_callers_stream(rptr_hip *h, void *hip_stream, F &&queue) {
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (st == h->stream) return queue(st);
    hipEvent_t e;
    HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    (void)hipEventRecord(e, h->stream);
    (void)hipStreamWaitEvent(st, e, 0);
    const int rc = queue(st);
    (void)hipEventRecord(e, st);
    (void)hipStreamWaitEvent(h->stream, e, 0);
    (void)hipEventDestroy(e);
    return rc;
}
// Host arrays of a run: every span gets a device copy, the SPAN_UP ones are uploaded, queue(stream, spans) queues the run on the backend's
// stream (spans[i].dev: the copies), the SPAN_DOWN ones come back and the stream is waited for. Results go both ways: the slots of
// skipped queries keep what the caller put there. A span without a host pointer is an optional array left out: its dev stays NULL.
enum { SPAN_UP = 1, SPAN_DOWN = 2 };
struct HostSpan {
    void *host;
    size_t bytes;
    int dir;
    void *dev;
};
template <class F>
static int run_on_host_arrays(rptr_hip *h, const char *what, HostSpan *spans, int count, F &&queue) {
    int rc = RPTR_OK;
    for (int i = 0; i < count && !rc; ++i)
        if (spans[i].host && hipMalloc(&spans[i].dev, spans[i].bytes) != hipSuccess) {
            spans[i].dev = nullptr;
            rc = fail(h, RPTR_E_NOMEM, "hipMalloc failed");
        }
    for (int i = 0; i < count && !rc; ++i)
        if (spans[i].dev && (spans[i].dir & SPAN_UP) && hipMemcpyAsync(spans[i].dev, spans[i].host, spans[i].bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
            rc = fail(h, RPTR_E_HIP, "upload failed");
    if (!rc) rc = queue(h->stream, spans);
    if (!rc) {
        bool ok = true;
        for (int i = 0; i < count && ok; ++i)
            if (spans[i].dev && (spans[i].dir & SPAN_DOWN)) ok = hipMemcpyAsync(spans[i].host, spans[i].dev, spans[i].bytes, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
        if (!ok || hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = fail(h, RPTR_E_HIP, "%s failed", what);
    }
    if (rc) (void)hipStreamSynchronize(h->stream); // nothing of the run may still use the buffers freed below
    for (int i = 0; i < count; ++i) (void)hipFree(spans[i].dev);
    return rc;
}

// ---- closest hits (RQ_CLOSEST): rp_k_trace over DEVICE buffers, asynchronously on `st`. dv != NULL: nodes and triangles visited per query;
// dt != NULL: explicit interval starts; any_hit: the shadow-ray traversal
static int closest_queries_on(rptr_hip *h, const RptrRenderRayQuery *dq, int n, float4 *dr, hipStream_t st, uint2 *dv, const float *dt, bool any_hit) {
    if (n == 0) return RPTR_OK;
    uint32_t *cursor = borrowed_cursor(h, st);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(h->persistent_blocks), dim3(RP_TRAVERSE_BLOCK), 0, st, h->master.dscene, dq, (uint32_t)n, dr, cursor, h->ctx[0].gstack, dv, dt);
    };
    rp_pick(h->master.dscene.single_instance != 0, [&](auto S) {
        if (any_hit)
            launch(rp_k_trace<true, true, decltype(S)::value>);
        else if (dv)
            launch(rp_k_trace<true, false, decltype(S)::value>);
        else
            launch(rp_k_trace<false, false, decltype(S)::value>);
    });
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}
static int check_closest_arguments(rptr_hip *h, const void *queries, int n, const void *out4) {
    if (!h || !queries || !out4 || n < 0) return fail(h, RPTR_E_INVALID, "bad argument");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "trace before set_scene");
    if (!h->ctx[0].gstack) return fail(h, RPTR_E_INVALID, "trace before initialize");
    return RPTR_OK;
}
} // extern "C++"

int rptr_hip_trace(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, float *out4) {
    return rptr_hip_trace_counted(h, queries, n, out4, nullptr, nullptr, 0);
}

int rptr_hip_trace_counted(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, float *out4, uint32_t *visits2, const float *tmin, int any_hit) {
    int rc = check_closest_arguments(h, queries, n, out4);
    if (rc || (rc = begin_query_run(h)) || n == 0) return rc;
    HostSpan spans[4] = {{const_cast<RptrRenderRayQuery *>(queries), (size_t)n * sizeof(RptrRenderRayQuery), SPAN_UP, nullptr},
                         {out4, (size_t)n * sizeof(float4), SPAN_UP | SPAN_DOWN, nullptr},
                         {visits2, (size_t)n * sizeof(uint2), SPAN_DOWN, nullptr},
                         {const_cast<float *>(tmin), (size_t)n * sizeof(float), SPAN_UP, nullptr}};
    return run_on_host_arrays(h, "trace kernel", spans, 4, [&](hipStream_t st, const HostSpan *s) {
        return closest_queries_on(h, (const RptrRenderRayQuery *)s[0].dev, n, (float4 *)s[1].dev, st, (uint2 *)s[2].dev, (const float *)s[3].dev, any_hit != 0);
    });
}

int rptr_hip_trace_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, float *device_out4, void *hip_stream) {
    int rc = check_closest_arguments(h, device_queries, n, device_out4);
    if (rc || (rc = begin_query_run(h))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) {
        return closest_queries_on(h, device_queries, n, reinterpret_cast<float4 *>(device_out4), st, nullptr, nullptr, false);
    });
}

int rptr_hip_enable_ray_queries(rptr_hip_t *h, int max_queries, int max_queries_per_pixel, void **out_device_queries, void **out_device_results) {
    if (!h || max_queries < 0 || max_queries_per_pixel < 0) return fail(h, RPTR_E_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // vulkan/render_vulkan.cpp:430-455: max(fixed budget, per-pixel budget x frame size) queries of 32 bytes, as many float4 results
    const size_t want = std::max<size_t>((size_t)max_queries, (size_t)h->width * (size_t)h->height * (size_t)max_queries_per_pixel);
    if (want > h->rq_capacity) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->rq_queries) (void)hipFree(h->rq_queries);
        if (h->rq_results) (void)hipFree(h->rq_results);
        h->rq_queries = nullptr;
        h->rq_results = nullptr;
        h->rq_capacity = 0;
        if (hipMalloc((void **)&h->rq_queries, want * sizeof(RptrRenderRayQuery)) != hipSuccess || hipMalloc((void **)&h->rq_results, want * sizeof(float4)) != hipSuccess) {
            if (h->rq_queries) (void)hipFree(h->rq_queries);
            h->rq_queries = nullptr;
            return fail(h, RPTR_E_NOMEM, "hipMalloc of the ray query buffers (%zu queries) failed", want);
        }
        h->rq_capacity = want;
    }
    if (out_device_queries) *out_device_queries = h->rq_queries;
    if (out_device_results) *out_device_results = h->rq_results;
    return RPTR_OK;
}

int rptr_hip_render_ray_queries(rptr_hip_t *h, int num_queries) {
    if (!h || num_queries < 0) return fail(h, RPTR_E_INVALID, "bad argument");
    const int rc = check_query_budget(h, num_queries);
    return rc ? rc : rptr_hip_trace_device(h, h->rq_queries, num_queries, reinterpret_cast<float *>(h->rq_results), nullptr);
}

extern "C++" {
// ---- the kinds that take a camera and a variant (radiance, surface). The arguments come first: they need neither a handle nor a device.
// missing_buffer: the kind's own rule, NULL when its buffers pass, else what to call the fault
static int check_camera_queries(rptr_hip_t *h, const char *kind, int n, const RptrCamera *camera, int variant, const char *missing_buffer) {
    if (!camera) return fail(h, RPTR_E_INVALID, "%s: NULL camera (its image-plane axes size the texture footprint)", kind);
    if (n < 0) return fail(h, RPTR_E_INVALID, "%s: n must be >= 0", kind);
    if (missing_buffer) return fail(h, RPTR_E_INVALID, "%s: %s", kind, missing_buffer);
    if (variant != RPTR_VARIANT_GLTF && variant != RPTR_VARIANT_SIMPLE && variant != RPTR_VARIANT_GLTF_TRANSMISSION)
        return fail(h, RPTR_E_INVALID, "%s: unknown variant %d", kind, variant);
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "%s before set_scene", kind);
    if (h->width == 0 || h->ctx.empty() || !h->ctx[0].gstack) return fail(h, RPTR_E_INVALID, "%s before initialize", kind);
    if (h->world > 1) return fail(h, RPTR_E_UNSUPPORTED, "%s need world_size 1: queries are not striped over the ranks", kind);
    return RPTR_OK;
}

// ---- radiance queries: the path-tracing variants of RenderBackend::render_ray_queries (host_frame.inl radiance_queries_on;
// render_vulkan.cpp:1867-1876, 2961-3059). NULL buffers pass when there is nothing to trace.
static int check_radiance_arguments(rptr_hip_t *h, const void *queries, int n, const RptrCamera *camera, int variant, int samples_per_query, int first_sample,
                                    const void *out4) {
    if (samples_per_query < 1) return fail(h, RPTR_E_INVALID, "samples_per_query must be >= 1");
    if (first_sample < 0) return fail(h, RPTR_E_INVALID, "first_sample must be >= 0");
    if ((long long)first_sample + samples_per_query > 0x7fffffffll) return fail(h, RPTR_E_INVALID, "first_sample + samples_per_query overflows");
    return check_camera_queries(h, "radiance queries", n, camera, variant, n > 0 && (!queries || !out4) ? "NULL query or result buffer" : nullptr);
}
} // extern "C++"

int rptr_hip_trace_radiance(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrCamera *camera, int variant, int samples_per_query, int first_sample,
                            float *out4, RptrStats *out_stats) {
    int rc = check_radiance_arguments(h, queries, n, camera, variant, samples_per_query, first_sample, out4);
    if (rc || (rc = begin_query_run(h))) return rc;
    if (out_stats) memset(out_stats, 0, sizeof(*out_stats));
    if (n == 0) return RPTR_OK;
    RpCounters tot;
    memset(&tot, 0, sizeof(tot));
    HostSpan spans[2] = {{const_cast<RptrRenderRayQuery *>(queries), (size_t)n * sizeof(RptrRenderRayQuery), SPAN_UP, nullptr},
                         {out4, (size_t)n * sizeof(float4), SPAN_UP | SPAN_DOWN, nullptr}}; // (up whatever first_sample is: the old means, and the skipped slots)
    rc = run_on_host_arrays(h, "radiance query kernels", spans, 2, [&](hipStream_t st, const HostSpan *s) {
        return radiance_queries_on(h, (const RptrRenderRayQuery *)s[0].dev, n, camera, variant, samples_per_query, first_sample, (float4 *)s[1].dev, st, &tot);
    });
    if (!rc && out_stats) {
        out_stats->rays_closest = tot.rays_closest;
        out_stats->rays_shadow = tot.rays_shadow;
        out_stats->hits_shaded = tot.hits_shaded;
        out_stats->spp = first_sample + samples_per_query;
        out_stats->device_bytes_allocated = h->bytes_allocated;
    }
    return rc;
}

int rptr_hip_trace_radiance_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, const RptrCamera *camera, int variant, int samples_per_query,
                                   int first_sample, float *device_out4, void *hip_stream) {
    int rc = check_radiance_arguments(h, device_queries, n, camera, variant, samples_per_query, first_sample, device_out4);
    if (rc || (rc = begin_query_run(h))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) {
        return radiance_queries_on(h, device_queries, n, camera, variant, samples_per_query, first_sample, reinterpret_cast<float4 *>(device_out4), st, nullptr);
    });
}

int rptr_hip_render_radiance_queries(rptr_hip_t *h, int num_queries, const RptrCamera *camera, int variant, int samples_per_query, int first_sample) {
    if (!h || num_queries < 0) return fail(h, RPTR_E_INVALID, "bad argument");
    const int rc = check_query_budget(h, num_queries);
    return rc ? rc
              : rptr_hip_trace_radiance_device(h, h->rq_queries, num_queries, camera, variant, samples_per_query, first_sample, reinterpret_cast<float *>(h->rq_results), nullptr);
}

// ---- surface queries (surface_query.h): the raw closest hits into the handle's scratch, then the decode into RptrSurfaceHit records.
// NULL buffers never pass.
extern "C++" {
static int check_surface_arguments(rptr_hip_t *h, bool have_queries, int n, const RptrCamera *camera, int variant, const void *out) {
    return check_camera_queries(h, "surface queries", n, camera, variant, !have_queries || !out ? "NULL query or output buffer" : nullptr);
}
// the scratch holds the largest n seen: a run of no more queries than an earlier one allocates nothing
static int surface_scratch(rptr_hip_t *h, int n) {
    if ((size_t)n <= h->sq_capacity) return RPTR_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (an earlier run -- on a caller's stream too: the backend's is ordered behind it -- may still use the old one)
    if (h->sq_raw) (void)hipFree(h->sq_raw);
    h->sq_raw = nullptr;
    h->sq_capacity = 0;
    if (hipMalloc(&h->sq_raw, (size_t)n * sizeof(RpRawHit)) != hipSuccess) {
        h->sq_raw = nullptr;
        return fail(h, RPTR_E_NOMEM, "hipMalloc of the surface-query scratch (%d queries) failed", n);
    }
    h->sq_capacity = (size_t)n;
    return RPTR_OK;
}
// queues the two launches on `st` for DEVICE buffers
static int surface_queries_on(rptr_hip_t *h, const RptrRenderRayQuery *dq, int n, const RptrCamera *camera, int variant, RptrSurfaceHit *dout, hipStream_t st) {
    if (n == 0) return RPTR_OK;
    RpFrame view;
    compute_view(*camera, h->width, h->height, view);
    RpSurfaceFrame f;
    memset(&f, 0, sizeof(f));
    memcpy(f.cam_du, view.cam_du, sizeof(f.cam_du));
    memcpy(f.cam_dv, view.cam_dv, sizeof(f.cam_dv));
    f.width = h->width;
    f.height = h->height;
    f.pixel_radius = h->params.pixel_radius;
    f.normal_z_scale = h->scene_params.normal_z_scale;
    RpRawHit *raw = static_cast<RpRawHit *>(h->sq_raw);
    const RpScene &sc = h->master.dscene;
    uint32_t *cursor = borrowed_cursor(h, st);
    rp_pick(sc.single_instance != 0, [&](auto S) {
        hipLaunchKernelGGL((rp_k_trace_surface<decltype(S)::value>), dim3(h->persistent_blocks), dim3(RP_TRAVERSE_BLOCK), 0, st, sc, dq, (uint32_t)n, raw, cursor, h->ctx[0].gstack);
    });
    // TEX as the frame's kernels select theirs: no material of the scene reads a texture -> the instantiation without sampling code
    const dim3 grid((unsigned)grid_for(h, (size_t)n));
    rp_pick(h->uses_textures, [&](auto T) {
        constexpr bool tex = decltype(T)::value;
        if (variant == RPTR_VARIANT_SIMPLE)
            hipLaunchKernelGGL((rp_k_surface<RPTR_VARIANT_SIMPLE, tex>), grid, dim3(256), 0, st, sc, f, dq, (const RpRawHit *)raw, (uint32_t)n, dout);
        else if (variant == RPTR_VARIANT_GLTF_TRANSMISSION)
            hipLaunchKernelGGL((rp_k_surface<RPTR_VARIANT_GLTF_TRANSMISSION, tex>), grid, dim3(256), 0, st, sc, f, dq, (const RpRawHit *)raw, (uint32_t)n, dout);
        else
            hipLaunchKernelGGL((rp_k_surface<RPTR_VARIANT_GLTF, tex>), grid, dim3(256), 0, st, sc, f, dq, (const RpRawHit *)raw, (uint32_t)n, dout);
    });
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}
}

int rptr_hip_trace_surface(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrCamera *camera, int variant, RptrSurfaceHit *out) {
    int rc = check_surface_arguments(h, queries != nullptr, n, camera, variant, out);
    if (rc || (rc = begin_query_run(h)) || n == 0 || (rc = surface_scratch(h, n))) return rc;
    HostSpan spans[2] = {{const_cast<RptrRenderRayQuery *>(queries), (size_t)n * sizeof(RptrRenderRayQuery), SPAN_UP, nullptr},
                         {out, (size_t)n * sizeof(RptrSurfaceHit), SPAN_UP | SPAN_DOWN, nullptr}};
    return run_on_host_arrays(h, "surface query kernels", spans, 2, [&](hipStream_t st, const HostSpan *s) {
        return surface_queries_on(h, (const RptrRenderRayQuery *)s[0].dev, n, camera, variant, (RptrSurfaceHit *)s[1].dev, st);
    });
}

int rptr_hip_trace_surface_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, const RptrCamera *camera, int variant, RptrSurfaceHit *device_out,
                                  void *hip_stream) {
    int rc = check_surface_arguments(h, true, n, camera, variant, device_out);
    if (rc) return rc;
    if (!device_queries) { // the query buffer of rptr_hip_enable_ray_queries
        if ((rc = check_query_budget(h, n))) return rc;
        device_queries = h->rq_queries;
    }
    if ((rc = begin_query_run(h)) || n == 0 || (rc = surface_scratch(h, n))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) { return surface_queries_on(h, device_queries, n, camera, variant, device_out, st); });
}

// ---- occlusion queries (occlusion_query.h): one any-hit traversal, one bit per query merged into the caller's words. NULL buffers pass
// when there is nothing to trace.
void rptr_hip_occlusion_defaults(RptrOcclusionParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->alpha_cutoff = 0.5f;
}

extern "C++" {
// the arguments come first: they need neither a handle nor a device. `p` is never NULL here (the entry points pass the defaults)
static int check_occlusion_arguments(rptr_hip_t *h, bool have_queries, int n, const RptrOcclusionParams &p, const void *bits) {
    const char *kind = "occlusion queries";
    if (n < 0) return fail(h, RPTR_E_INVALID, "%s: n must be >= 0", kind);
    if (n > 0 && (!have_queries || !bits)) return fail(h, RPTR_E_INVALID, "%s: NULL query or result buffer", kind);
    if (p.reserved[0] != 0u || p.reserved[1] != 0u) return fail(h, RPTR_E_INVALID, "%s: reserved words must be 0", kind);
    if ((p.flags & ~RPTR_OCCLUSION_ALPHA_CUTOUT) != 0u) return fail(h, RPTR_E_INVALID, "%s: unknown flag bits 0x%x", kind, p.flags & ~RPTR_OCCLUSION_ALPHA_CUTOUT);
    if ((p.flags & RPTR_OCCLUSION_ALPHA_CUTOUT) != 0u && !(std::isfinite(p.alpha_cutoff) && p.alpha_cutoff > 0.0f && p.alpha_cutoff <= 1.0f))
        return fail(h, RPTR_E_INVALID, "%s: alpha_cutoff must be finite and in (0, 1]", kind);
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "%s before set_scene", kind);
    if (h->ctx.empty() || !h->ctx[0].gstack) return fail(h, RPTR_E_INVALID, "%s before initialize", kind);
    return RPTR_OK;
}
// queues the launch on `st` for DEVICE buffers. The cutout instantiation only where it can differ: the flag is set AND the scene has
// alpha-tested materials (what RpFrame::alpha_test is derived from); grids as a frame's shadow-ray launches alone on the GPU choose theirs
static int occlusion_queries_on(rptr_hip_t *h, const RptrRenderRayQuery *dq, int n, const RptrOcclusionParams &p, uint32_t *bits, hipStream_t st) {
    if (n == 0) return RPTR_OK;
    const RpScene &sc = h->master.dscene;
    const bool cutout = (p.flags & RPTR_OCCLUSION_ALPHA_CUTOUT) != 0u && h->uses_alpha;
    const float cutoff = p.alpha_cutoff;
    uint32_t *cursor = borrowed_cursor(h, st);
    rp_pick(cutout, [&](auto A) {
        rp_pick(sc.single_instance != 0, [&](auto S) {
            constexpr bool alpha = decltype(A)::value, single = decltype(S)::value;
            const int blocks = alpha ? h->persistent_blocks : h->connect_blocks[single ? 1 : 0];
            hipLaunchKernelGGL((rp_k_trace_occlusion<alpha, single>), dim3(blocks), dim3(RP_TRAVERSE_BLOCK), 0, st, sc, dq, (uint32_t)n, bits, cutoff, cursor, h->ctx[0].gstack);
        });
    });
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}
static RptrOcclusionParams occlusion_params_or_defaults(const RptrOcclusionParams *params) {
    RptrOcclusionParams p;
    rptr_hip_occlusion_defaults(&p);
    return params ? *params : p;
}
}

int rptr_hip_trace_occlusion(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrOcclusionParams *params, uint32_t *out_bits) {
    const RptrOcclusionParams p = occlusion_params_or_defaults(params);
    int rc = check_occlusion_arguments(h, queries != nullptr, n, p, out_bits);
    if (rc || n == 0 || (rc = begin_query_run(h))) return rc;
    HostSpan spans[2] = {{const_cast<RptrRenderRayQuery *>(queries), (size_t)n * sizeof(RptrRenderRayQuery), SPAN_UP, nullptr},
                         {out_bits, ((size_t)n + 31) / 32 * sizeof(uint32_t), SPAN_UP | SPAN_DOWN, nullptr}}; // (up: the bits of skipped queries and those behind n)
    return run_on_host_arrays(h, "occlusion query kernel", spans, 2, [&](hipStream_t st, const HostSpan *s) {
        return occlusion_queries_on(h, (const RptrRenderRayQuery *)s[0].dev, n, p, (uint32_t *)s[1].dev, st);
    });
}

int rptr_hip_trace_occlusion_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, const RptrOcclusionParams *params, uint32_t *device_out_bits,
                                    void *hip_stream) {
    const RptrOcclusionParams p = occlusion_params_or_defaults(params);
    int rc = check_occlusion_arguments(h, true, n, p, device_out_bits);
    if (rc || n == 0) return rc;
    if (!device_queries) { // the query buffer of rptr_hip_enable_ray_queries
        if ((rc = check_query_budget(h, n))) return rc;
        device_queries = h->rq_queries;
    }
    if ((rc = begin_query_run(h))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) { return occlusion_queries_on(h, device_queries, n, p, device_out_bits, st); });
}

// ---- irradiance probes (probes.h): per run of whole probes the ray kernel, a radiance-query run with the fresh fold, the projection.
void rptr_hip_probe_defaults(RptrProbeParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->rays_per_probe = 128u;
    out->samples_per_ray = 1u;
    out->rotation[0] = out->rotation[4] = out->rotation[8] = 1.0f;
    out->blend = 1.0f;
    out->t_max = 1e20f;
}

int rptr_hip_probe_directions(uint32_t K, float *out3K) {
    if (K < 1u || K > RPTR_PROBE_MAX_RAYS) return fail(nullptr, RPTR_E_INVALID, "probe directions: K = %u is outside 1 .. %u", K, RPTR_PROBE_MAX_RAYS);
    if (!out3K) return fail(nullptr, RPTR_E_INVALID, "probe directions: NULL output");
    const double g = (std::sqrt(5.0) - 1.0) / 2.0, two_pi = 2.0 * 3.14159265358979323846;
    for (uint32_t k = 0; k < K; ++k) {
        const double z = 1.0 - (2.0 * (double)k + 1.0) / (double)K;
        const double kg = (double)k * g;
        const double phi = two_pi * (kg - std::floor(kg));
        const double r = std::sqrt(std::max(0.0, 1.0 - z * z));
        out3K[3 * k] = (float)(r * std::cos(phi));
        out3K[3 * k + 1] = (float)(r * std::sin(phi));
        out3K[3 * k + 2] = (float)z;
    }
    return RPTR_OK;
}

extern "C++" {
static RptrProbeParams probe_params_or_defaults(const RptrProbeParams *params) {
    RptrProbeParams p;
    rptr_hip_probe_defaults(&p);
    return params ? *params : p;
}
// the params alone: they need neither a handle nor a device. `p` is never NULL here (the entry points pass the defaults)
static int check_probe_params(rptr_hip_t *h, const RptrProbeParams &p) {
    const char *kind = "probes";
    if (p.rays_per_probe < 1u || p.rays_per_probe > RPTR_PROBE_MAX_RAYS)
        return fail(h, RPTR_E_INVALID, "%s: rays_per_probe = %u is outside 1 .. %u", kind, p.rays_per_probe, RPTR_PROBE_MAX_RAYS);
    if (p.samples_per_ray < 1u) return fail(h, RPTR_E_INVALID, "%s: samples_per_ray must be >= 1", kind);
    if (p.sample_index < 0) return fail(h, RPTR_E_INVALID, "%s: sample_index must be >= 0", kind);
    if ((unsigned long long)p.sample_index + p.samples_per_ray > 0x7fffffffull) return fail(h, RPTR_E_INVALID, "%s: sample_index + samples_per_ray overflows", kind);
    if (p.flags != 0u) return fail(h, RPTR_E_INVALID, "%s: unknown flag bits 0x%x", kind, p.flags);
    if (p.reserved[0] != 0u || p.reserved[1] != 0u || p.reserved[2] != 0u) return fail(h, RPTR_E_INVALID, "%s: reserved words must be 0", kind);
    if (!(std::isfinite(p.blend) && p.blend > 0.0f && p.blend <= 1.0f)) return fail(h, RPTR_E_INVALID, "%s: blend must be finite and in (0, 1]", kind);
    if (!(std::isfinite(p.clamp) && p.clamp >= 0.0f)) return fail(h, RPTR_E_INVALID, "%s: clamp must be finite and >= 0", kind);
    if (!(p.t_max > 0.0f)) return fail(h, RPTR_E_INVALID, "%s: t_max must be > 0", kind);
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(p.rotation[i])) return fail(h, RPTR_E_INVALID, "%s: rotation[%d] is not finite", kind, i);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double dot = 0.0;
            for (int k = 0; k < 3; ++k) dot += (double)p.rotation[3 * r + k] * (double)p.rotation[3 * c + k];
            if (!(std::fabs(dot - (r == c ? 1.0 : 0.0)) <= 1e-3))
                return fail(h, RPTR_E_INVALID, "%s: rotation is not orthonormal: (R R^T)[%d][%d] = %g", kind, r, c, dot);
        }
    return RPTR_OK;
}
static RpProbeConst probe_constants(const RptrProbeParams &p) {
    RpProbeConst c;
    memcpy(c.rot, p.rotation, sizeof(c.rot));
    c.t_max = p.t_max;
    c.clamp = p.clamp;
    c.blend = p.blend;
    c.weight = (float)(4.0 * 3.14159265358979323846 / (double)p.rays_per_probe);
    c.K = p.rays_per_probe;
    return c;
}
// the direction table of K on the device: computed and uploaded when K changes, kept otherwise
static int probe_table(rptr_hip_t *h, uint32_t K) {
    if (h->pb_dirs && h->pb_dirs_K == K) return RPTR_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (an earlier run -- on a caller's stream too: the backend's is ordered behind it -- may still read the old table)
    if (!h->pb_dirs && hipMalloc((void **)&h->pb_dirs, (size_t)RPTR_PROBE_MAX_RAYS * 3 * sizeof(float)) != hipSuccess) {
        h->pb_dirs = nullptr;
        return fail(h, RPTR_E_NOMEM, "hipMalloc of the probe direction table failed");
    }
    std::vector<float> table((size_t)K * 3);
    const int rc = rptr_hip_probe_directions(K, table.data());
    if (rc) return rc;
    h->pb_dirs_K = 0;
    HIP_TRY(h, hipMemcpy(h->pb_dirs, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    h->pb_dirs_K = K;
    return RPTR_OK;
}
// 48 bytes per ray: the records of `rays` rays, then their values; holds the largest run seen
static int probe_scratch(rptr_hip_t *h, size_t rays) {
    if (rays <= h->pb_capacity) return RPTR_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->pb_scratch) (void)hipFree(h->pb_scratch);
    h->pb_scratch = nullptr;
    h->pb_capacity = 0;
    h->pb_last_rays = 0;
    if (hipMalloc(&h->pb_scratch, rays * 48) != hipSuccess) {
        h->pb_scratch = nullptr;
        return fail(h, RPTR_E_NOMEM, "hipMalloc of the probe scratch (%zu rays) failed", rays);
    }
    h->pb_capacity = rays;
    return RPTR_OK;
}
static int probe_rays_on(rptr_hip_t *h, const float *dpos, uint32_t n_probes, const RpProbeConst &c, RptrRenderRayQuery *dq, hipStream_t st) {
    const uint32_t n_rays = n_probes * c.K;
    hipLaunchKernelGGL(rp_k_probe_rays, dim3((unsigned)grid_for(h, n_rays)), dim3(256), 0, st, dpos, n_rays, c, (const float *)h->pb_dirs, reinterpret_cast<float4 *>(dq));
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}
static int probe_project_on(rptr_hip_t *h, const float4 *dvalues, uint32_t n_probes, const float *dpos, const RpProbeConst &c, float *dcoeffs, hipStream_t st) {
    // one wave per probe, four to a block
    hipLaunchKernelGGL(rp_k_probe_project, dim3((unsigned)grid_for(h, (size_t)n_probes * 64)), dim3(256), 0, st, dvalues, dpos, n_probes, c, (const float *)h->pb_dirs,
                       reinterpret_cast<float4 *>(dcoeffs));
    HIP_TRY(h, hipGetLastError());
    return RPTR_OK;
}
static int check_probe_stage(rptr_hip_t *h, const char *stage, uint32_t n_probes, const RptrProbeParams &p, const char *missing_buffer) {
    int rc = check_probe_params(h, p);
    if (rc) return rc;
    if (n_probes > 0 && missing_buffer) return fail(h, RPTR_E_INVALID, "probes: %s: %s", stage, missing_buffer);
    if ((unsigned long long)n_probes * p.rays_per_probe > 0x7fffffffull)
        return fail(h, RPTR_E_INVALID, "probes: %s: %u probes x %u rays exceed 2^31 - 1 rays", stage, n_probes, p.rays_per_probe);
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    return RPTR_OK;
}
static uint32_t probes_per_run(const RptrProbeParams &p) {
    const uint32_t R = p.max_run_rays ? p.max_run_rays : (1u << 22);
    return std::max(1u, R / p.rays_per_probe);
}
static int check_probe_arguments(rptr_hip_t *h, const void *positions, uint32_t n_probes, const RptrCamera *camera, int variant, const RptrProbeParams &p,
                                 const void *coeffs) {
    const int rc = check_probe_params(h, p); // (the arguments come first: they need neither a handle nor a device; the handle: check_camera_queries)
    if (rc) return rc;
    if (n_probes > 0x7fffffffu) return fail(h, RPTR_E_INVALID, "probes: n_probes = %u is too large", n_probes);
    return check_camera_queries(h, "probes", (int)n_probes, camera, variant, n_probes > 0 && (!positions || !coeffs) ? "NULL position or coefficient buffer" : nullptr);
}
// queues every run of the call on `st` for DEVICE buffers; the scratch holds a run
static int probes_on(rptr_hip_t *h, const float *dpos, uint32_t n_probes, const RptrCamera *camera, int variant, const RptrProbeParams &p, float *dcoeffs, hipStream_t st,
                     RpCounters *totals) {
    const RpProbeConst c = probe_constants(p);
    const uint32_t per_run = probes_per_run(p);
    RptrRenderRayQuery *records = static_cast<RptrRenderRayQuery *>(h->pb_scratch);
    float4 *values = reinterpret_cast<float4 *>(static_cast<char *>(h->pb_scratch) + h->pb_capacity * 32);
    for (uint32_t p0 = 0; p0 < n_probes; p0 += per_run) {
        const uint32_t np = std::min(per_run, n_probes - p0);
        const int n_rays = (int)(np * c.K);
        int rc = probe_rays_on(h, dpos + 3ull * p0, np, c, records, st);
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(values, 0, (size_t)n_rays * sizeof(float4), st)); // (the rays of skipped probes read 0)
        if ((rc = radiance_queries_on(h, records, n_rays, camera, variant, (int)p.samples_per_ray, p.sample_index, values, st, totals, true))) return rc;
        if ((rc = probe_project_on(h, values, np, dpos + 3ull * p0, c, dcoeffs + 36ull * p0, st))) return rc;
        h->pb_last_rays = (size_t)n_rays;
    }
    return RPTR_OK;
}
static size_t probe_run_rays(uint32_t n_probes, const RptrProbeParams &p) { return (size_t)std::min(n_probes, probes_per_run(p)) * p.rays_per_probe; }
} // extern "C++"

int rptr_hip_probe_rays_device(rptr_hip_t *h, const float *device_positions3, uint32_t n_probes, const RptrProbeParams *params, RptrRenderRayQuery *device_queries,
                               void *hip_stream) {
    const RptrProbeParams p = probe_params_or_defaults(params);
    int rc = check_probe_stage(h, "ray stage", n_probes, p, !device_positions3 || !device_queries ? "NULL position or record buffer" : nullptr);
    if (rc || n_probes == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = probe_table(h, p.rays_per_probe))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) { return probe_rays_on(h, device_positions3, n_probes, probe_constants(p), device_queries, st); });
}

int rptr_hip_probe_project_device(rptr_hip_t *h, const float *device_values4, uint32_t n_probes, const float *device_positions3, const RptrProbeParams *params,
                                  float *device_coeffs36, void *hip_stream) {
    const RptrProbeParams p = probe_params_or_defaults(params);
    int rc = check_probe_stage(h, "projection stage", n_probes, p, !device_values4 || !device_coeffs36 ? "NULL value or coefficient buffer" : nullptr);
    if (rc || n_probes == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = probe_table(h, p.rays_per_probe))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) {
        return probe_project_on(h, reinterpret_cast<const float4 *>(device_values4), n_probes, device_positions3, probe_constants(p), device_coeffs36, st);
    });
}

int rptr_hip_trace_probes(rptr_hip_t *h, const float *positions3, uint32_t n_probes, const RptrCamera *camera, int variant, const RptrProbeParams *params, float *coeffs36,
                          RptrStats *out_stats) {
    const RptrProbeParams p = probe_params_or_defaults(params);
    int rc = check_probe_arguments(h, positions3, n_probes, camera, variant, p, coeffs36);
    if (rc || n_probes == 0) return rc;
    if ((rc = begin_query_run(h)) || (rc = probe_table(h, p.rays_per_probe)) || (rc = probe_scratch(h, probe_run_rays(n_probes, p)))) return rc;
    if (out_stats) memset(out_stats, 0, sizeof(*out_stats));
    RpCounters tot;
    memset(&tot, 0, sizeof(tot));
    HostSpan spans[2] = {{const_cast<float *>(positions3), (size_t)n_probes * 3 * sizeof(float), SPAN_UP, nullptr},
                         {coeffs36, (size_t)n_probes * 36 * sizeof(float), SPAN_UP | SPAN_DOWN, nullptr}}; // (up: skipped probes, blend < 1)
    rc = run_on_host_arrays(h, "probe kernels", spans, 2, [&](hipStream_t st, const HostSpan *s) {
        return probes_on(h, (const float *)s[0].dev, n_probes, camera, variant, p, (float *)s[1].dev, st, &tot);
    });
    if (!rc && out_stats) {
        out_stats->rays_closest = tot.rays_closest;
        out_stats->rays_shadow = tot.rays_shadow;
        out_stats->hits_shaded = tot.hits_shaded;
        out_stats->spp = (int)p.samples_per_ray;
        out_stats->device_bytes_allocated = h->bytes_allocated;
    }
    return rc;
}

int rptr_hip_trace_probes_device(rptr_hip_t *h, const float *device_positions3, uint32_t n_probes, const RptrCamera *camera, int variant, const RptrProbeParams *params,
                                 float *device_coeffs36, void *hip_stream) {
    const RptrProbeParams p = probe_params_or_defaults(params);
    int rc = check_probe_arguments(h, device_positions3, n_probes, camera, variant, p, device_coeffs36);
    if (rc || n_probes == 0) return rc;
    if ((rc = begin_query_run(h)) || (rc = probe_table(h, p.rays_per_probe)) || (rc = probe_scratch(h, probe_run_rays(n_probes, p)))) return rc;
    return on_callers_stream(h, hip_stream, [&](hipStream_t st) { return probes_on(h, device_positions3, n_probes, camera, variant, p, device_coeffs36, st, nullptr); });
}

int rptr_hip_readback_probe_rays(rptr_hip_t *h, float *out4, size_t n_rays) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!out4 && n_rays > 0) return fail(h, RPTR_E_INVALID, "readback_probe_rays: NULL output");
    if (!h->pb_scratch || h->pb_last_rays == 0) return fail(h, RPTR_E_INVALID, "readback_probe_rays: no probe run yet");
    if (n_rays > h->pb_last_rays) return fail(h, RPTR_E_INVALID, "readback_probe_rays: %zu rays asked for, the last run had %zu", n_rays, h->pb_last_rays);
    if (n_rays == 0) return RPTR_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out4, static_cast<char *>(h->pb_scratch) + h->pb_capacity * 32, n_rays * sizeof(float4), hipMemcpyDeviceToHost));
    return RPTR_OK;
}

// ---- object motion (object_motion.h): the tracking of the previous frame's state, and the pass over the last submitted frame's
// motion + jitter AOV image. The pass is a query run over the master set -- after the checks below that set holds what the frame saw.
int rptr_hip_track_object_motion(rptr_hip_t *h, int enable) {
    const char *who = "rptr_hip_track_object_motion";
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "%s before set_scene", who);
    if (h->world > 1) return fail(h, RPTR_E_UNSUPPORTED, "%s needs world_size 1", who);
    auto &om = h->om;
    if (!enable) { // (the buffers stay until the next set_scene: switching it on again allocates nothing)
        om.enabled = false;
        return RPTR_OK;
    }
    if (om.enabled) return RPTR_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (!om.d_rewritten) {
        std::vector<void *> *const A = &h->scene_allocs;
        const size_t ng = h->master.dynpos.size();
        if ((rc = dev_alloc(h, &om.prev_inst_xf, (size_t)24 * h->num_instances, A))) return rc;
        om.prev_pos.assign(ng, nullptr);
        for (size_t g = 0; g < ng; ++g)
            if (h->master.dynpos[g] && (rc = dev_alloc(h, &om.prev_pos[g], (size_t)h->geom_tris[g] * 9, A))) return rc;
        std::vector<const float *> table(om.prev_pos.begin(), om.prev_pos.end());
        if ((rc = dev_upload(h, &om.d_prev_pos, table.size(), table.data(), hipMemcpyHostToDevice, A))) return rc;
        if ((rc = dev_upload(h, &om.d_record_geom, h->record_geometry.size(), h->record_geometry.data(), hipMemcpyHostToDevice, A))) return rc;
        if ((rc = dev_alloc(h, &om.d_geom_changed, ng, A))) return rc;
        if ((rc = dev_alloc(h, &om.d_rewritten, 1, A))) return rc;
        om.geom_marked.assign(ng, 0);
    }
    om.submissions = 0;
    om.snapshot = om.counted = om.staged_since_submission = om.dirty[0] = om.dirty[1] = false;
    om.last_frames = 1;
    for (FrameCtx &c : h->ctx) c.last_submission = 0;
    om.enabled = true;
    return RPTR_OK;
}

int rptr_hip_object_motion(rptr_hip_t *h) {
    const char *who = "rptr_hip_object_motion";
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "%s before set_scene", who);
    auto &om = h->om;
    if (!om.enabled) return fail(h, RPTR_E_INVALID, "%s: the previous frame's state is not tracked (rptr_hip_track_object_motion after set_scene)", who);
    if (h->world > 1) return fail(h, RPTR_E_UNSUPPORTED, "%s needs world_size 1", who);
    if (h->width != 0 && !h->aovs) return fail(h, RPTR_E_UNSUPPORTED, "%s rewrites the motion + jitter AOV image: option \"aovs\" is 0", who);
    if (om.unrefitted && om.staged_since_submission)
        return fail(h, RPTR_E_INVALID, "%s: updates are staged and not refitted: the tables no longer hold what the last frame saw (call it before the next "
                                       "update_instances / update_vertices)", who);
    if (om.staged_since_submission)
        return fail(h, RPTR_E_INVALID, "%s: updates were staged after the last frame's submission: the tables no longer hold what that frame saw (call it "
                                       "before the next update_instances / update_vertices)", who);
    if (om.dirty[0] || om.dirty[1])
        return fail(h, RPTR_E_INVALID, "%s: the last frame or the one before it was submitted while staged updates awaited rptr_hip_refit: what it saw is "
                                       "not what was staged", who);
    // frames in flight are waited for, oldest first: the frame waited for last is the one submitted last
    for (;;) {
        FrameCtx *first = nullptr;
        for (FrameCtx &c : h->ctx)
            if (c.pending && (!first || c.ticket < first->ticket)) first = &c;
        if (!first) break;
        const int rc = finish_frame(h, *first, nullptr);
        if (rc) return rc;
    }
    int rc;
    if ((rc = check_finished_frame_with_aovs(h, who, "call it", "the motion + jitter AOV image", false))) return rc;
    const FrameCtx &ac = h->ctx[(size_t)h->aov_ctx];
    if (om.submissions == 0 || ac.last_submission != om.submissions)
        return fail(h, RPTR_E_INVALID, "%s: no frame has been submitted since the tracking was switched on", who);
    om.counted = false;
    // nothing moved: a launch sequence of several frames (objects cannot move inside one), nothing staged between the previous frame and
    // this one, or no previous frame since the tracking was switched on
    if (om.last_frames > 1 || !om.snapshot || om.snapshot_of < 1 || om.snapshot_of + 1 != om.submissions) return RPTR_OK;
    if ((rc = begin_query_run(h)) || (rc = surface_scratch(h, h->npix_padded))) return rc;
    const RpFrame &f = ac.last_frame;
    const RpScene &sc = h->master.dscene;
    RpObjectMotionTables tb;
    tb.inst_xf = h->master.inst_xf;
    tb.prev_inst_xf = om.prev_inst_xf;
    tb.record_geom = om.d_record_geom;
    tb.geom_changed = om.d_geom_changed;
    tb.prev_pos = om.d_prev_pos;
    tb.num_instances = h->num_instances;
    tb.any_geom_changed = std::find(om.geom_marked.begin(), om.geom_marked.end(), (char)1) != om.geom_marked.end() ? 1u : 0u;
    RpRawHit *raw = static_cast<RpRawHit *>(h->sq_raw);
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemsetAsync(om.d_rewritten, 0, sizeof(uint32_t), st));
    uint32_t *cursor = borrowed_cursor(h, st);
    rp_pick(sc.single_instance != 0, [&](auto S) {
        hipLaunchKernelGGL((rp_k_trace_pixels<decltype(S)::value>), dim3(h->persistent_blocks), dim3(RP_TRAVERSE_BLOCK), 0, st, sc, f, raw, cursor, h->ctx[0].gstack);
    });
    hipLaunchKernelGGL(rp_k_object_motion, dim3(((unsigned)h->npix_padded + 255u) / 256u), dim3(256), 0, st, sc, f, tb, (const RpRawHit *)raw, om.d_rewritten);
    HIP_TRY(h, hipGetLastError());
    om.counted = true;
    return RPTR_OK;
}
