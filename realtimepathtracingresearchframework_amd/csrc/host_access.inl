// host_access.inl -- everything else a host reaches through the handle: BVH policy, freeze frame, point sets, stage timing, the option calls, frame buffer / tile /
// AOV read-backs (last_finished_image: which image they mean), the denoiser, the exported tree (ray queries: host_queries.inl)
// Part of the ONE translation unit rptr_hip.hip (included there, in this order: host_state.h, host_bvh.inl, host_scene.inl,
// host_frame.inl, host_access.inl, host_queries.inl, host_comm.h): the host runtime split along its seams; no symbol changed.
int rptr_hip_set_bvh_policy(rptr_hip_t *h, int force_bvh_rebuild, int rebuild_triangle_budget) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (rebuild_triangle_budget < 0) return fail(h, RPTR_E_INVALID, "rebuild_triangle_budget must be >= 0");
    h->bvh_force_rebuild = force_bvh_rebuild != 0;
    h->bvh_budget = rebuild_triangle_budget;
    return RPTR_OK;
}

int rptr_hip_bvh_rebuild_count(const rptr_hip_t *h, uint64_t *out_rebuilds) {
    if (!h || !out_rebuilds) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    *out_rebuilds = h->rebuilds_done;
    return RPTR_OK;
}

int rptr_hip_set_freeze_frame(rptr_hip_t *h, int freeze_frame) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    h->freeze_frame = freeze_frame != 0;
    return RPTR_OK;
}

int rptr_hip_set_rng_variant(rptr_hip_t *h, int rng_variant, const void *table, size_t table_bytes) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (rng_variant < RPTR_RNG_VARIANT_UNIFORM || rng_variant > RPTR_RNG_VARIANT_Z_SBL)
        return fail(h, RPTR_E_INVALID, "rng_variant %d (0 uniform, 1 blue noise, 2 Sobol, 3 Z-Sobol)", rng_variant);
    size_t need = 0;
    if (rng_variant == RPTR_RNG_VARIANT_BN) need = RPTR_BN_TABLE_MIN_BYTES;
    if (rng_variant == RPTR_RNG_VARIANT_SOBOL || rng_variant == RPTR_RNG_VARIANT_Z_SBL) need = RPTR_SOBOL_TABLE_BYTES;
    if (need && (!table || table_bytes < need))
        return fail(h, RPTR_E_INVALID, "rng_variant %d needs a table of %zu bytes (got %zu)", rng_variant, need, table ? table_bytes : (size_t)0);
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->rng_table) {
        (void)hipFree(h->rng_table);
        h->rng_table = nullptr;
    }
    if (need) {
        HIP_TRY(h, hipMalloc((void **)&h->rng_table, need));
        HIP_TRY(h, hipMemcpy(h->rng_table, table, need, hipMemcpyHostToDevice));
        for (FrameCtx &c : h->ctx) // the alpha-test generator of closest-hit queries gets its own slot in the path state
            if (!c.ps.alpha_rng && h->path_capacity && (rc = dev_alloc(h, &c.ps.alpha_rng, h->path_capacity, nullptr))) return rc;
    }
    h->rng_variant = rng_variant;
    return RPTR_OK;
}

int rptr_hip_set_stage_timing(rptr_hip_t *h, int level) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (level < 0 || level > 2) return fail(h, RPTR_E_INVALID, "stage timing level %d (0 none, 1 extend only, 2 all stages)", level);
    h->opt.v[OPT_STAGE_TIMING] = level;
    h->stage_timing = level;
    return RPTR_OK;
}

// ---- options (the table at the top of this file)
int rptr_hip_set_option(rptr_hip_t *h, const char *key, int64_t value) {
    const int k = find_option(key);
    if (k < 0) return fail(h, RPTR_E_INVALID, "rptr_hip_set_option: unknown option \"%s\"", key ? key : "(null)");
    if (value < g_opt_desc[k].lo || value > g_opt_desc[k].hi)
        return fail(h, RPTR_E_INVALID, "rptr_hip_set_option: %s = %lld is outside [%lld, %lld]", key, (long long)value, g_opt_desc[k].lo, g_opt_desc[k].hi);
    if (!h) { // the process default: what new handles (and the handle-less rptr_hip_build_bvh_host) start from
        set_process_default_option(k, value);
        return RPTR_OK;
    }
    if (h->opt.from_env[k]) return RPTR_OK; // the environment variable of this option is set: the experimenter's override stands (rptr_hip_get_option tells)
    h->opt.v[k] = value;
    sync_options(h);
    return RPTR_OK;
}
int rptr_hip_get_option(const rptr_hip_t *h, const char *key, int64_t *out_value) {
    if (h && key && out_value && !strcmp(key, "bvh_rebuild_failures")) { // (read-only: a counter, not a switch)
        *out_value = (int64_t)h->rebuild_failures;
        return RPTR_OK;
    }
    if (h && key && out_value && !strcmp(key, "instance_updates_rejected")) { // (read-only: matrices rptr_hip_update_instances_device skipped
        uint32_t n = 0;                                                       // since set_scene; waits for the backend's stream)
        if (h->have_scene && h->d_inst_rejected) {
            if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
                hipMemcpy(&n, h->d_inst_rejected, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(nullptr, RPTR_E_HIP, "reading the counter failed");
        }
        *out_value = (int64_t)n;
        return RPTR_OK;
    }
    if (h && key && out_value && !strcmp(key, "skin_vertices_rejected")) { // (read-only: vertices rptr_hip_skin left alone because their new position
        uint32_t n = 0;                                                    // was not finite, since set_scene; waits for the backend's stream)
        if (h->have_scene && h->skin.d_rejected) {
            if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
                hipMemcpy(&n, h->skin.d_rejected, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(nullptr, RPTR_E_HIP, "reading the counter failed");
        }
        *out_value = (int64_t)n;
        return RPTR_OK;
    }
    if (h && key && out_value && !strcmp(key, "object_motion_pixels")) { // (read-only: pixels the last rptr_hip_object_motion rewrote; waits for the
        uint32_t n = 0;                                                  // backend's stream)
        if (h->have_scene && h->om.d_rewritten && h->om.counted) {
            if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
                hipMemcpy(&n, h->om.d_rewritten, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(nullptr, RPTR_E_HIP, "reading the counter failed");
        }
        *out_value = (int64_t)n;
        return RPTR_OK;
    }
    if (h && key && out_value && !strcmp(key, "sample_slots")) { // (read-only: the sample slots a frame context holds once initialize has sized
        *out_value = (int64_t)h->max_batch_spp;                  // the path state -- "max_batch_spp" or what the budget allows; 0 before initialize)
        return RPTR_OK;
    }
    if (h && key && out_value) { // (read-only: the persistent traversal grids initialize sized, in blocks of RP_TRAVERSE_BLOCK threads; 0 before it)
        const struct { const char *key; int64_t v; } grids[] = {
            {"traversal_resident_blocks", (int64_t)h->num_cus * h->resident_per_cu[0]}, // first closest-hit kernel: blocks that fit at once
            {"traversal_grid_alone", h->resident_per_cu[0] ? traversal_grid(h, 0, 1) : 0},  // ... its grid in a frame alone on the GPU
            {"traversal_grid_shared", h->resident_per_cu[0] ? traversal_grid(h, 0, h->max_concurrency) : 0}, // ... beside the most frames
            {"traversal_stack_blocks", h->ctx.empty() ? 0 : (int64_t)(h->ctx[0].gstack_threads / RP_TRAVERSE_BLOCK)}, // the stack scratch
            {"traversal_concurrency", h->max_concurrency}, // frames that can run side by side: min(frame contexts, hardware queues)
            {"last_traversal_grid", h->last_grids[0]},     // the first closest-hit grid of the last submitted frame
        };
        for (const auto &g : grids)
            if (!strcmp(key, g.key)) {
                *out_value = g.v;
                return RPTR_OK;
            }
    }
    const int k = find_option(key);
    if (k < 0 || !out_value) return fail(nullptr, RPTR_E_INVALID, "rptr_hip_get_option: unknown option \"%s\" or NULL result", key ? key : "(null)");
    *out_value = h ? h->opt.v[k] : effective_default_options().v[k];
    return RPTR_OK;
}
int rptr_hip_option_count(void) { return OPT_PUBLIC_COUNT; }
const char *rptr_hip_option_name(int index) { return index >= 0 && index < OPT_PUBLIC_COUNT ? g_opt_desc[index].key : nullptr; }

int rptr_hip_get_framebuffer_size(const rptr_hip_t *h, uint32_t out_whc[3]) {
    if (!h || !out_whc) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    out_whc[0] = (uint32_t)h->width;
    out_whc[1] = (uint32_t)h->height;
    out_whc[2] = 4;
    return RPTR_OK;
}

int rptr_hip_tile_rows(const rptr_hip_t *h, int rank, int32_t *first_and_count, int cap) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    const int n_stripes = (h->height + h->stripe_rows - 1) / h->stripe_rows;
    int n = 0;
    for (int s = rank; s < n_stripes; s += h->world) {
        if (first_and_count && n < cap) {
            first_and_count[2 * n] = s * h->stripe_rows;
            first_and_count[2 * n + 1] = std::min(h->stripe_rows, h->height - s * h->stripe_rows);
        }
        ++n;
    }
    return n;
}

int rptr_hip_local_pixel_count(const rptr_hip_t *h, uint64_t *out_pixels) {
    if (!h || !out_pixels) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    *out_pixels = (uint64_t)h->width * (uint64_t)h->local_rows;
    return RPTR_OK;
}

// The last finished image: what read-backs, the denoiser and the gather (host_comm.h) refer to. One frame at a time it is the handle's
// accumulation buffer and RGBA8 frame; with frames in flight the context of the frame that was waited for last keeps a copy (one per
// frame of a launch sequence; `back` steps that many frames back in it). Refused while a newer frame on that context rewrites it.
static int last_finished_image(rptr_hip *h, const float4 **accum, const uchar4 **fb, int back = 0) {
    if (h->output_overwritten)
        return fail(h, RPTR_E_INVALID, "the image of the last waited frame is being overwritten by a newer frame in flight on the same frame context: "
                                       "read back before submitting that frame, or rptr_hip_wait for it first");
    const FrameCtx *c = h->output_ctx >= 0 ? &h->ctx[(size_t)h->output_ctx] : nullptr;
    if (!c) {
        if (accum) *accum = h->accum;
        if (fb) *fb = h->fb;
        return RPTR_OK;
    }
    const size_t at = (size_t)(h->output_index - back) * ((size_t)h->width * (size_t)std::max(h->local_rows, 1));
    if (accum) *accum = c->out_accum + at;
    if (fb) *fb = c->out_fb + at;
    return RPTR_OK;
}

int rptr_hip_copy_tile_to_device(rptr_hip_t *h, void *device_dst, size_t n_bytes) {
    if (!h || !device_dst) return fail(h, RPTR_E_INVALID, "NULL argument");
    const size_t need = (size_t)h->width * h->local_rows * sizeof(float4);
    if (n_bytes < need) return fail(h, RPTR_E_INVALID, "destination too small: %zu < %zu", n_bytes, need);
    const float4 *src = nullptr;
    const int rc = last_finished_image(h, &src, nullptr);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (need) HIP_TRY(h, hipMemcpyAsync(device_dst, src, need, hipMemcpyDeviceToDevice, h->stream));
    return RPTR_OK;
}

extern "C++" {
template <class T>
static int readback_rows(rptr_hip *h, const T *dev_local, T *host_full, size_t n_elems_host) {
    const size_t need = (size_t)h->width * h->height;
    if (n_elems_host < need) return fail(h, RPTR_E_INVALID, "read-back buffer too small");
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<T> tmp((size_t)h->width * std::max(h->local_rows, 1));
    if (h->local_rows)
        HIP_TRY(h, hipMemcpyAsync(tmp.data(), dev_local, (size_t)h->width * h->local_rows * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int n_stripes = (h->height + h->stripe_rows - 1) / h->stripe_rows;
    int local_row = 0;
    for (int s = h->rank; s < n_stripes; s += h->world) {
        const int first = s * h->stripe_rows, cnt = std::min(h->stripe_rows, h->height - first);
        memcpy(host_full + (size_t)first * h->width, tmp.data() + (size_t)local_row * h->width, (size_t)cnt * h->width * sizeof(T));
        local_row += cnt;
    }
    return RPTR_OK;
}
} // extern "C++"

int rptr_hip_readback_f32(rptr_hip_t *h, float *rgba, size_t n_floats) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    const float4 *src = nullptr;
    const int rc = last_finished_image(h, &src, nullptr);
    return rc ? rc : readback_rows<float4>(h, src, reinterpret_cast<float4 *>(rgba), n_floats / 4);
}
int rptr_hip_readback_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    const uchar4 *src = nullptr;
    int rc = last_finished_image(h, nullptr, &src);
    if (rc) return rc;
    if (h->params.render_upscale_factor != 2) return readback_rows<uchar4>(h, src, reinterpret_cast<uchar4 *>(rgba), n_bytes / 4);
    // render_upscale_factor == 2 (process_samples.comp:192-197): the frame buffer has twice the render resolution, every rendered
    // pixel fills a 2x2 block. Replicated here, on the way out (rows of other ranks stay untouched, as in the 1:1 read-back).
    const size_t W = (size_t)h->width, H = (size_t)h->height;
    if (n_bytes / 4 < 4 * W * H) return fail(h, RPTR_E_INVALID, "read-back buffer too small for the 2x upscaled frame buffer");
    std::vector<uchar4> lo(W * H);
    const uchar4 *big = reinterpret_cast<const uchar4 *>(rgba);
    for (size_t y = 0; y < H; ++y) // keep what the caller's buffer holds for rows this rank does not own
        for (size_t x = 0; x < W; ++x) lo[y * W + x] = big[(2 * y) * (2 * W) + 2 * x];
    if ((rc = readback_rows<uchar4>(h, src, lo.data(), lo.size()))) return rc;
    uchar4 *out = reinterpret_cast<uchar4 *>(rgba);
    for (size_t y = 0; y < H; ++y)
        for (size_t x = 0; x < W; ++x) {
            const uchar4 px = lo[y * W + x];
            out[(2 * y) * (2 * W) + 2 * x] = out[(2 * y) * (2 * W) + 2 * x + 1] = out[(2 * y + 1) * (2 * W) + 2 * x] = out[(2 * y + 1) * (2 * W) + 2 * x + 1] = px;
        }
    return RPTR_OK;
}

int rptr_hip_readback_aov(rptr_hip_t *h, int aov_index, uint16_t *rgba16f, size_t n_halfs) {
    if (!h || !rgba16f) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (aov_index < 0 || aov_index >= 3) return fail(h, RPTR_E_INVALID, "AOV index %d (0 albedo+roughness, 1 normal+depth, 2 motion+jitter)", aov_index);
    if (h->aov_overwritten)
        return fail(h, RPTR_E_INVALID, "the AOV images of the last finished frame are being overwritten by a newer frame in flight on the same frame "
                                       "context: read back before submitting that frame, or rptr_hip_wait for it first");
    const FrameCtx &c = h->ctx[(size_t)h->aov_ctx];
    if (!c.aov[aov_index]) return fail(h, RPTR_E_INVALID, "AOV images are switched off (RPTR_AOVS=0) or initialize() has not run");
    return readback_rows<uint2>(h, c.aov[aov_index], reinterpret_cast<uint2 *>(rgba16f), n_halfs / 4);
}

// ---- what the calls that work on the last finished frame and its AOV images (the denoiser, the temporal upscaler) ask of the handle:
// one device, the AOV images on, a frame finished, its images not being overwritten by a frame in flight, and the AOV images those of
// the frame waited for last. `who`: the entry point; `verb`: what the host is told to do earlier; `reads`: the AOV images it needs
// (NULL: none, option "aovs" may be 0); at_render_resolution: the call's images have the render resolution, so render_upscale_factor 2 is refused
extern "C++" {
static int check_finished_frame_with_aovs(rptr_hip *h, const char *who, const char *verb, const char *reads, bool at_render_resolution) {
    if (h->world > 1) return fail(h, RPTR_E_UNSUPPORTED, "%s needs world_size 1: the taps of a stripe's pixels lie in other ranks' rows", who);
    if (h->width == 0) return fail(h, RPTR_E_INVALID, "%s before initialize", who);
    if (reads && !h->aovs) return fail(h, RPTR_E_UNSUPPORTED, "%s reads %s: option \"aovs\" is 0", who, reads);
    if (at_render_resolution && h->params.render_upscale_factor == 2)
        return fail(h, RPTR_E_UNSUPPORTED, "%s needs render_upscale_factor 1 (its RGBA8 image has the render resolution)", who);
    if (h->finished_serial == 0) return fail(h, RPTR_E_INVALID, "%s before a frame has finished (render, or wait for a ticket, first)", who);
    if (h->output_overwritten || h->aov_overwritten)
        return fail(h, RPTR_E_INVALID, "%s: the images of the last waited frame are being overwritten by a newer frame in flight on the same frame context: "
                                       "%s before submitting that frame, or rptr_hip_wait for it first", who, verb);
    const FrameCtx &ac = h->ctx[(size_t)h->aov_ctx];
    if (h->output_ctx >= 0 && (h->output_ctx != h->aov_ctx || h->output_index != ac.batch_n - 1))
        return fail(h, RPTR_E_INVALID, "%s: the AOV images belong to the last frame of the launch sequence finished last, the frame waited "
                                       "for last is another one", who);
    return RPTR_OK;
}
}

// ---- the denoiser (denoise.h): the last finished frame through prepare, `iterations` a-trous passes and finish, on the backend's stream
void rptr_hip_denoise_defaults(RptrDenoiseParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->iterations = 5;
    out->sigma_luminance = 4.0f;
    out->sigma_depth = 1.0f;
    out->normal_power_log2 = 7;
    out->demodulate_albedo = 1;
}

// What the two denoise calls share: the five spatial parameters (the leading fields of both parameter structs) and their checks, ...
extern "C++" {
template <class To, class From> static void copy_spatial_params(To &to, const From &from) {
    to.iterations = from.iterations;
    to.sigma_luminance = from.sigma_luminance;
    to.sigma_depth = from.sigma_depth;
    to.normal_power_log2 = from.normal_power_log2;
    to.demodulate_albedo = from.demodulate_albedo;
}
static int check_denoise_params(rptr_hip *h, const char *who, const RptrDenoiseParams &p) {
    if (p.iterations < 1 || p.iterations > 5) return fail(h, RPTR_E_INVALID, "%s: iterations = %d is outside [1, 5]", who, p.iterations);
    if (!(p.sigma_luminance > 0.0f) || !std::isfinite(p.sigma_luminance) || !(p.sigma_depth > 0.0f) || !std::isfinite(p.sigma_depth))
        return fail(h, RPTR_E_INVALID, "%s: sigma_luminance and sigma_depth must be finite and > 0 (are %g, %g)", who, (double)p.sigma_luminance,
                    (double)p.sigma_depth);
    if (p.normal_power_log2 < 0 || p.normal_power_log2 > 8)
        return fail(h, RPTR_E_INVALID, "%s: normal_power_log2 = %d is outside [0, 8]", who, p.normal_power_log2);
    if (p.demodulate_albedo != 0 && p.demodulate_albedo != 1) return fail(h, RPTR_E_INVALID, "%s: demodulate_albedo must be 0 or 1", who);
    return RPTR_OK;
}
// ... the denoiser's images (made by the first call of either) and the kernels' arguments for the last finished frame, ...
static int denoise_args(rptr_hip *h, const RptrDenoiseParams &p, RpDenoiseArgs &a) {
    int rc;
    const FrameCtx &ac = h->ctx[(size_t)h->aov_ctx];
    const size_t npix = (size_t)h->width * (size_t)h->height;
    if (!h->dn.out_u8) {
        if ((rc = dev_alloc(h, &h->dn.ev[0], npix, nullptr)) || (rc = dev_alloc(h, &h->dn.ev[1], npix, nullptr)) || (rc = dev_alloc(h, &h->dn.ndz, npix, nullptr)) ||
            (rc = dev_alloc(h, &h->dn.gz, npix, nullptr)) || (rc = dev_alloc(h, &h->dn.out_f32, npix, nullptr)) || (rc = dev_alloc(h, &h->dn.out_u8, npix, nullptr)))
            return rc;
    }
    memset(&a, 0, sizeof(a));
    if ((rc = last_finished_image(h, &a.accum, &a.fb))) return rc; // (world_size 1: an image is the whole frame, npix pixels)
    a.albedo = ac.aov[0];
    a.nd = ac.aov[1];
    a.ndz = h->dn.ndz;
    a.gz = h->dn.gz;
    a.out_f32 = h->dn.out_f32;
    a.out_u8 = h->dn.out_u8;
    a.width = h->width;
    a.height = h->height;
    a.sigma_luminance = p.sigma_luminance;
    a.sigma_depth = p.sigma_depth;
    a.normal_power_log2 = p.normal_power_log2;
    a.demodulate = p.demodulate_albedo;
    a.output_channel = h->params.output_channel;
    a.tone_mapping_mode = h->params.early_tone_mapping_mode;
    a.exposure_scale = (float)std::exp2((double)h->params.exposure);
    return RPTR_OK;
}
static dim3 denoise_tiles(const rptr_hip *h) {
    const unsigned T = RP_DN_TILE;
    return dim3(((unsigned)h->width + T - 1) / T, ((unsigned)h->height + T - 1) / T);
}
// ... and the launches after prepare (or after rp_k_denoise_temporal in its place): the passes and finish
static int denoise_filter_and_finish(rptr_hip *h, const RpDenoiseArgs &a, int iterations) {
    const unsigned T = RP_DN_TILE;
    const dim3 tiles = denoise_tiles(h);
    const size_t npix = (size_t)h->width * (size_t)h->height;
    for (int i = 0; i < iterations; ++i) {
        const int s = 1 << i;
        const float4 *in = h->dn.ev[i & 1];
        float4 *out = h->dn.ev[(i & 1) ^ 1];
        if (s == 1)
            rp_launch_kernel(RpLaunch{tiles, h->stream, nullptr, nullptr}, rp_k_denoise_pass<1>, 256u, a, in, out, s);
        else if (s == 2)
            rp_launch_kernel(RpLaunch{tiles, h->stream, nullptr, nullptr}, rp_k_denoise_pass<2>, 256u, a, in, out, s);
        else { // tiles of the s x s sub-lattices: each has at most ceil(W / s) x ceil(H / s) pixels
            const unsigned us = (unsigned)s;
            const dim3 lattice(us * ((((unsigned)h->width + us - 1) / us + T - 1) / T), us * ((((unsigned)h->height + us - 1) / us + T - 1) / T));
            rp_launch_kernel(RpLaunch{lattice, h->stream, nullptr, nullptr}, rp_k_denoise_pass<0>, 256u, a, in, out, s);
        }
    }
    rp_launch_kernel(RpLaunch{dim3((unsigned)grid_for(h, npix)), h->stream, nullptr, nullptr}, rp_k_denoise_finish, 256u, a, (const float4 *)h->dn.ev[iterations & 1]);
    HIP_TRY(h, hipGetLastError());
    h->dn.serial = h->finished_serial;
    return RPTR_OK;
}
} // extern "C++"

int rptr_hip_denoise(rptr_hip_t *h, const RptrDenoiseParams *p) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!p) return fail(h, RPTR_E_INVALID, "rptr_hip_denoise: NULL parameters");
    int rc;
    if ((rc = check_denoise_params(h, "rptr_hip_denoise", *p))) return rc;
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(h, RPTR_E_INVALID, "rptr_hip_denoise: RptrDenoiseParams.reserved must be 0");
    if ((rc = check_finished_frame_with_aovs(h, "rptr_hip_denoise", "denoise", "the albedo and normal + depth AOV images", true))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    RpDenoiseArgs a;
    if ((rc = denoise_args(h, *p, a))) return rc;
    rp_launch_kernel(RpLaunch{denoise_tiles(h), h->stream, nullptr, nullptr}, rp_k_denoise_prepare, 256u, a, h->dn.ev[0]);
    return denoise_filter_and_finish(h, a, p->iterations);
}

// ---- the temporal denoiser (denoise_temporal.h): rp_k_denoise_temporal in prepare's place -- it blends the frame with the history the
// previous call left, along the motion AOV, and leaves the next call's -- then the same passes and finish
void rptr_hip_denoise_temporal_defaults(RptrDenoiseTemporalParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    RptrDenoiseParams sp;
    rptr_hip_denoise_defaults(&sp);
    copy_spatial_params(*out, sp);
    out->alpha_color = 0.2f;
    out->alpha_moments = 0.2f;
    out->normal_threshold = 0.9f;
    out->depth_tolerance = 0.1f;
}

int rptr_hip_denoise_temporal(rptr_hip_t *h, const RptrDenoiseTemporalParams *p) {
    const char *who = "rptr_hip_denoise_temporal";
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    RptrDenoiseTemporalParams defaults;
    rptr_hip_denoise_temporal_defaults(&defaults);
    if (!p) p = &defaults;
    RptrDenoiseParams sp; // the five spatial parameters
    memset(&sp, 0, sizeof(sp));
    copy_spatial_params(sp, *p);
    int rc;
    if ((rc = check_denoise_params(h, who, sp))) return rc;
    if (!(p->alpha_color > 0.0f && p->alpha_color <= 1.0f) || !(p->alpha_moments > 0.0f && p->alpha_moments <= 1.0f))
        return fail(h, RPTR_E_INVALID, "%s: alpha_color and alpha_moments must be in (0, 1] (are %g, %g)", who, (double)p->alpha_color, (double)p->alpha_moments);
    if (!(p->normal_threshold >= -1.0f && p->normal_threshold <= 1.0f))
        return fail(h, RPTR_E_INVALID, "%s: normal_threshold = %g is outside [-1, 1]", who, (double)p->normal_threshold);
    if (!(p->depth_tolerance >= 0.0f) || !std::isfinite(p->depth_tolerance))
        return fail(h, RPTR_E_INVALID, "%s: depth_tolerance must be finite and >= 0 (is %g)", who, (double)p->depth_tolerance);
    if (p->reset_history != 0 && p->reset_history != 1) return fail(h, RPTR_E_INVALID, "%s: reset_history must be 0 or 1", who);
    for (int r : p->reserved)
        if (r) return fail(h, RPTR_E_INVALID, "%s: RptrDenoiseTemporalParams.reserved must be 0", who);
    if ((rc = check_finished_frame_with_aovs(h, who, "denoise", "the albedo, normal + depth and motion + jitter AOV images", true))) return rc;
    const FrameCtx &ac = h->ctx[(size_t)h->aov_ctx];
    HIP_TRY(h, hipSetDevice(h->device));
    RpDenoiseArgs a;
    if ((rc = denoise_args(h, sp, a))) return rc;
    const size_t npix = (size_t)h->width * (size_t)h->height;
    if (!h->dt.hndz[1]) {
        for (int k = 0; k < 2; ++k)
            if ((rc = dev_alloc(h, &h->dt.he[k], npix, nullptr)) || (rc = dev_alloc(h, &h->dt.hm[k], npix, nullptr)) || (rc = dev_alloc(h, &h->dt.hndz[k], npix, nullptr)))
                return rc;
        h->dt.cur = 0;
        h->dt.have = false;
    }
    const int in = h->dt.cur, out = in ^ 1;
    RpDenoiseTemporalArgs t;
    memset(&t, 0, sizeof(t));
    t.mj = ac.aov[2];
    t.he_in = h->dt.he[in];
    t.hm_in = h->dt.hm[in];
    t.hndz_in = h->dt.hndz[in];
    t.he_out = h->dt.he[out];
    t.hm_out = h->dt.hm[out];
    t.hndz_out = h->dt.hndz[out];
    t.alpha_color = p->alpha_color;
    t.alpha_moments = p->alpha_moments;
    t.normal_threshold = p->normal_threshold;
    t.depth_tolerance = p->depth_tolerance;
    t.have_history = (h->dt.have && !p->reset_history && h->dt.demodulate == p->demodulate_albedo) ? 1 : 0;
    rp_launch_kernel(RpLaunch{denoise_tiles(h), h->stream, nullptr, nullptr}, rp_k_denoise_temporal, 256u, a, t, h->dn.ev[0]);
    h->dt.cur = out;
    h->dt.have = true;
    h->dt.demodulate = p->demodulate_albedo;
    return denoise_filter_and_finish(h, a, p->iterations);
}

int rptr_hip_readback_denoise_history_f32(rptr_hip_t *h, float *rgba, size_t n_floats) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (!h->dt.have) return fail(h, RPTR_E_INVALID, "no denoise history: call rptr_hip_denoise_temporal first");
    return readback_rows<float4>(h, h->dt.he[h->dt.cur], reinterpret_cast<float4 *>(rgba), n_floats / 4);
}

extern "C++" {
static int check_denoised(rptr_hip *h) {
    if (!h->dn.out_u8 || h->dn.serial == 0) return fail(h, RPTR_E_INVALID, "no denoised image: call rptr_hip_denoise_temporal or rptr_hip_denoise first");
    if (h->dn.serial != h->finished_serial)
        return fail(h, RPTR_E_INVALID, "the denoised image is stale: a later frame has finished since the denoise call ran; call it again for that frame");
    return RPTR_OK;
}
}
int rptr_hip_readback_denoised_f32(rptr_hip_t *h, float *rgba, size_t n_floats) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    const int rc = check_denoised(h);
    return rc ? rc : readback_rows<float4>(h, h->dn.out_f32, reinterpret_cast<float4 *>(rgba), n_floats / 4);
}
int rptr_hip_readback_denoised_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    const int rc = check_denoised(h);
    return rc ? rc : readback_rows<uchar4>(h, h->dn.out_u8, reinterpret_cast<uchar4 *>(rgba), n_bytes / 4);
}

// ---- temporal 2x upscaling (taa_upscale.h): the last finished frame and the previous call's output into a display-size image
void rptr_hip_taa_upscale_defaults(RptrTaaUpscaleParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->factor = 2;
}

int rptr_hip_taa_upscale(rptr_hip_t *h, const RptrTaaUpscaleParams *p) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    RptrTaaUpscaleParams defaults;
    rptr_hip_taa_upscale_defaults(&defaults);
    if (!p) p = &defaults;
    if (p->factor != 2) return fail(h, RPTR_E_INVALID, "rptr_hip_taa_upscale: factor = %d (2 is the one supported)", p->factor);
    if (p->reset_history != 0 && p->reset_history != 1) return fail(h, RPTR_E_INVALID, "rptr_hip_taa_upscale: reset_history must be 0 or 1");
    if (p->reserved[0] || p->reserved[1]) return fail(h, RPTR_E_INVALID, "rptr_hip_taa_upscale: RptrTaaUpscaleParams.reserved must be 0");
    int rc;
    if ((rc = check_finished_frame_with_aovs(h, "rptr_hip_taa_upscale", "upscale", "the motion + jitter AOV image", false))) return rc;
    const FrameCtx &ac = h->ctx[(size_t)h->aov_ctx];
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t npix = (size_t)h->width * (size_t)h->height;
    if (!h->up.img[0]) {
        if ((rc = dev_alloc(h, &h->up.img[0], 4 * npix, nullptr)) || (rc = dev_alloc(h, &h->up.img[1], 4 * npix, nullptr))) return rc;
        h->up.cur = 0;
        h->up.have = false;
    }
    const uchar4 *pre = nullptr;
    if ((rc = last_finished_image(h, nullptr, &pre))) return rc; // (world_size 1: an image is the whole frame)
    uchar4 *out = h->up.img[h->up.cur ^ 1];
    if (p->reset_history || !h->up.have)
        rp_launch_kernel(RpLaunch{dim3((unsigned)grid_for(h, 4 * npix)), h->stream, nullptr, nullptr}, rp_k_upscale_replicate, 256u, h->width, h->height, pre, out);
    else {
        const unsigned T = RP_TAA_TILE;
        const dim3 tiles((2u * (unsigned)h->width + T - 1) / T, (2u * (unsigned)h->height + T - 1) / T);
        rp_launch_kernel(RpLaunch{tiles, h->stream, nullptr, nullptr}, rp_k_taa_upscale, 64u, h->width, h->height, pre, (const uchar4 *)h->up.img[h->up.cur],
                         (const uint2 *)ac.aov[2], out);
    }
    HIP_TRY(h, hipGetLastError());
    h->up.cur ^= 1;
    h->up.have = true;
    return RPTR_OK;
}

int rptr_hip_readback_upscaled_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (!h->up.have) return fail(h, RPTR_E_INVALID, "no upscaled image: call rptr_hip_taa_upscale first");
    const size_t need = 16 * (size_t)h->width * (size_t)h->height;
    if (n_bytes < need) return fail(h, RPTR_E_INVALID, "read-back buffer too small for the upscaled image: %zu < %zu bytes", n_bytes, need);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(rgba, h->up.img[h->up.cur], need, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RPTR_OK;
}

// ---- auto-exposure (auto_exposure.h): meter the last finished frame or the denoiser's image, adapt the ev on the device, expose
void rptr_hip_auto_exposure_defaults(RptrAutoExposureParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->mode = 1;
    out->tone_mapping_mode = -1;
    out->key = 0.18f;
    out->low_percentile = 0.5f;
    out->high_percentile = 0.95f;
    out->min_ev = -8.0f;
    out->max_ev = 8.0f;
    out->speed_up = 1.0f;
    out->speed_down = 3.0f;
    out->white_balance[0] = out->white_balance[1] = out->white_balance[2] = 1.0f;
}

// What the display passes (auto-exposure, bloom) share: the checks of the fields both parameter structs have, ...
extern "C++" {
static int check_display_fields(rptr_hip *h, const char *who, int source, int tone_mapping_mode, const float white_balance[3]) {
    if (source != 0 && source != 1) return fail(h, RPTR_E_INVALID, "%s: source = %d (0: the frame, 1: the denoised image)", who, source);
    if (tone_mapping_mode < -1 || tone_mapping_mode > 2) return fail(h, RPTR_E_INVALID, "%s: tone_mapping_mode = %d is outside [-1, 2]", who, tone_mapping_mode);
    for (int k = 0; k < 3; ++k)
        if (!(white_balance[k] > 0.0f) || !std::isfinite(white_balance[k])) return fail(h, RPTR_E_INVALID, "%s: white_balance gains must be finite and > 0", who);
    return RPTR_OK;
}
// ... what they ask of the finished frame (and of the denoised image, source 1); selects the device, ...
static int check_display_frame(rptr_hip *h, const char *who, int source) {
    int rc;
    if ((rc = check_finished_frame_with_aovs(h, who, "expose", source == 1 ? "the denoised image, made from the AOV images" : nullptr, true))) return rc;
    if (source == 1 && (rc = check_denoised(h))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return RPTR_OK;
}
// ... and the display kernel's arguments for the last finished frame, all but the scale. *copied: output_channel != 0, an AOV view -- `out`
// has been given the frame's RGBA8 as it is (the denoiser's rule) and there is nothing to launch.
static int display_args(rptr_hip *h, int source, int tone_mapping_mode, const float white_balance[3], uchar4 *out, RpExposeArgs &x, bool *copied) {
    int rc;
    const size_t npix = (size_t)h->width * (size_t)h->height;
    const float4 *accum = nullptr;
    const uchar4 *fb = nullptr;
    if ((rc = last_finished_image(h, &accum, &fb))) return rc; // (world_size 1: an image is the whole frame, npix pixels)
    *copied = h->params.output_channel != 0;
    if (*copied) {
        HIP_TRY(h, hipMemcpyAsync(out, fb, npix * sizeof(uchar4), hipMemcpyDeviceToDevice, h->stream));
        return RPTR_OK;
    }
    memset(&x, 0, sizeof(x));
    x.src = source == 1 ? h->dn.out_f32 : accum;
    x.fb = fb;
    x.out = out;
    x.npix = npix;
    x.tone_mapping_mode = tone_mapping_mode;
    x.balance = (white_balance[0] != 1.0f || white_balance[1] != 1.0f || white_balance[2] != 1.0f) ? 1 : 0;
    for (int k = 0; k < 3; ++k) x.gains[k] = white_balance[k];
    return RPTR_OK;
}
static float manual_exposure_scale(const rptr_hip *h) { return (float)std::exp2((double)(h->params.exposure + 0.0f)); }
}

int rptr_hip_auto_exposure(rptr_hip_t *h, const RptrAutoExposureParams *p) {
    const char *who = "rptr_hip_auto_exposure";
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    RptrAutoExposureParams defaults;
    rptr_hip_auto_exposure_defaults(&defaults);
    if (!p) p = &defaults;
    int rc;
    if ((rc = check_display_fields(h, who, p->source, p->tone_mapping_mode, p->white_balance))) return rc;
    if (p->mode != 0 && p->mode != 1) return fail(h, RPTR_E_INVALID, "%s: mode = %d (0: manual, 1: meter and adapt)", who, p->mode);
    if (p->reset_history != 0 && p->reset_history != 1) return fail(h, RPTR_E_INVALID, "%s: reset_history must be 0 or 1", who);
    if (!(p->key > 0.0f) || !std::isfinite(p->key)) return fail(h, RPTR_E_INVALID, "%s: key must be finite and > 0 (is %g)", who, (double)p->key);
    if (!(p->low_percentile >= 0.0f && p->low_percentile < 1.0f) || !(p->high_percentile > p->low_percentile && p->high_percentile <= 1.0f))
        return fail(h, RPTR_E_INVALID, "%s: the percentiles must satisfy 0 <= low < high <= 1 (are %g, %g)", who, (double)p->low_percentile, (double)p->high_percentile);
    if (!std::isfinite(p->min_ev) || !std::isfinite(p->max_ev) || !(p->min_ev <= p->max_ev))
        return fail(h, RPTR_E_INVALID, "%s: min_ev and max_ev must be finite, min_ev <= max_ev (are %g, %g)", who, (double)p->min_ev, (double)p->max_ev);
    if (!(p->speed_up >= 0.0f) || !std::isfinite(p->speed_up) || !(p->speed_down >= 0.0f) || !std::isfinite(p->speed_down))
        return fail(h, RPTR_E_INVALID, "%s: speed_up and speed_down must be finite and >= 0 (are %g, %g)", who, (double)p->speed_up, (double)p->speed_down);
    if (!(p->dt >= 0.0f) || !std::isfinite(p->dt)) return fail(h, RPTR_E_INVALID, "%s: dt must be finite and >= 0 (is %g)", who, (double)p->dt);
    if (p->reserved) return fail(h, RPTR_E_INVALID, "%s: RptrAutoExposureParams.reserved must be 0", who);
    if ((rc = check_display_frame(h, who, p->source))) return rc;
    const size_t npix = (size_t)h->width * (size_t)h->height;
    if (!h->ae.out_u8) {
        if ((rc = dev_alloc(h, &h->ae.hist, RP_AE_WORDS, nullptr)) || (rc = dev_alloc(h, &h->ae.state, 1, nullptr)) || (rc = dev_alloc(h, &h->ae.out_u8, npix, nullptr))) {
            h->ae = decltype(h->ae)(); // (what was allocated stays on the handle's list and is freed with it)
            return rc;
        }
        HIP_TRY(h, hipMemsetAsync(h->ae.hist, 0, RP_AE_WORDS * sizeof(uint32_t), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->ae.state, 0, sizeof(RptrExposureState), h->stream));
    }
    RpExposeArgs x;
    bool copied = false;
    if ((rc = display_args(h, p->source, p->tone_mapping_mode, p->white_balance, h->ae.out_u8, x, &copied))) return rc;
    if (copied) {
        h->ae.serial = h->finished_serial;
        return RPTR_OK;
    }
    const RpLaunch one{dim3(1), h->stream, nullptr, nullptr};
    const RpLaunch per_pixel{dim3((unsigned)grid_for(h, npix)), h->stream, nullptr, nullptr};
    if (p->mode == 1) {
        RpMeterReduceArgs m;
        memset(&m, 0, sizeof(m));
        m.hist = h->ae.hist;
        m.state = h->ae.state;
        for (int s = 0; s < 8; ++s) m.T[s] = std::log2(1.0 + ((double)s + 0.5) / 8.0);
        m.log2_key = std::log2((double)p->key);
        m.k_up = 1.0 - std::exp(-(double)p->dt * (double)p->speed_up);
        m.k_down = 1.0 - std::exp(-(double)p->dt * (double)p->speed_down);
        m.low_percentile = p->low_percentile;
        m.high_percentile = p->high_percentile;
        m.min_ev = p->min_ev;
        m.max_ev = p->max_ev;
        m.exposure = h->params.exposure;
        m.have_state = h->ae.have_state ? 1 : 0;
        m.reset_history = p->reset_history;
        m.jump = p->dt == 0.0f ? 1 : 0;
        // (four blocks per CU: at most 1024 x 256 global adds on 256 CUs, whatever the image size)
        rp_launch_kernel(RpLaunch{dim3((unsigned)grid_for(h, npix, 4)), h->stream, nullptr, nullptr}, rp_k_meter<false>, 256u, x.src, npix, h->ae.hist);
        rp_launch_kernel(one, rp_k_meter_reduce, 256u, m);
        h->ae.have_state = true;
        x.state = h->ae.state;
    } else
        x.scale = manual_exposure_scale(h);
    rp_launch_kernel(per_pixel, rp_k_expose, 256u, x);
    HIP_TRY(h, hipGetLastError());
    h->ae.serial = h->finished_serial;
    return RPTR_OK;
}

int rptr_hip_readback_exposed_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (!h->ae.out_u8 || h->ae.serial == 0) return fail(h, RPTR_E_INVALID, "no exposed image: call rptr_hip_auto_exposure first");
    if (h->ae.serial != h->finished_serial)
        return fail(h, RPTR_E_INVALID, "the exposed image is stale: a later frame has finished since rptr_hip_auto_exposure ran; call it again for that frame");
    return readback_rows<uchar4>(h, h->ae.out_u8, reinterpret_cast<uchar4 *>(rgba), n_bytes / 4);
}

int rptr_hip_readback_exposure_state(rptr_hip_t *h, RptrExposureState *out) {
    if (!h || !out) return fail(h, RPTR_E_INVALID, "NULL argument");
    if (!h->ae.have_state) return fail(h, RPTR_E_INVALID, "no exposure state: call rptr_hip_auto_exposure with mode 1 first");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, h->ae.state, sizeof(*out), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RPTR_OK;
}

// ---- bloom (bloom.h): the part of the exposed image above a threshold down a pyramid, back up, and added in front of the tone map
void rptr_hip_bloom_defaults(RptrBloomParams *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->tone_mapping_mode = -1;
    out->threshold = 1.0f;
    out->knee = 0.5f;
    out->clamp = 16.0f;
    out->intensity = 0.2f;
    out->scatter = 0.7f;
    out->white_balance[0] = out->white_balance[1] = out->white_balance[2] = 1.0f;
}

int rptr_hip_bloom(rptr_hip_t *h, const RptrBloomParams *p) {
    const char *who = "rptr_hip_bloom";
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    RptrBloomParams defaults;
    rptr_hip_bloom_defaults(&defaults);
    if (!p) p = &defaults;
    int rc;
    if ((rc = check_display_fields(h, who, p->source, p->tone_mapping_mode, p->white_balance))) return rc;
    if (p->exposure_mode != 0 && p->exposure_mode != 1) return fail(h, RPTR_E_INVALID, "%s: exposure_mode = %d (0: manual, 1: the metered state)", who, p->exposure_mode);
    if (p->levels < 0 || p->levels > RPTR_BLOOM_MAX_LEVELS) return fail(h, RPTR_E_INVALID, "%s: levels = %d is outside [0, %d]", who, p->levels, RPTR_BLOOM_MAX_LEVELS);
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold) || !(p->knee >= 0.0f) || !std::isfinite(p->knee))
        return fail(h, RPTR_E_INVALID, "%s: threshold and knee must be finite and >= 0 (are %g, %g)", who, (double)p->threshold, (double)p->knee);
    if (!(p->clamp > 0.0f) || !std::isfinite(p->clamp)) return fail(h, RPTR_E_INVALID, "%s: clamp must be finite and > 0 (is %g)", who, (double)p->clamp);
    if (!(p->intensity >= 0.0f) || !std::isfinite(p->intensity)) return fail(h, RPTR_E_INVALID, "%s: intensity must be finite and >= 0 (is %g)", who, (double)p->intensity);
    if (!(p->scatter >= 0.0f && p->scatter <= 1.0f)) return fail(h, RPTR_E_INVALID, "%s: scatter = %g is outside [0, 1]", who, (double)p->scatter);
    for (int r : p->reserved)
        if (r) return fail(h, RPTR_E_INVALID, "%s: RptrBloomParams.reserved must be 0", who);
    if (p->exposure_mode == 1 && !h->ae.have_state)
        return fail(h, RPTR_E_INVALID, "%s: exposure_mode 1 reads the exposure state: call rptr_hip_auto_exposure with mode 1 first", who);
    if ((rc = check_display_frame(h, who, p->source))) return rc;
    const size_t npix = (size_t)h->width * (size_t)h->height;
    if (!h->bl.out_u8) {
        const RpBloomPyramid all = rp_bloom_pyramid((uint32_t)h->width, (uint32_t)h->height, RP_BLOOM_MAX_LEVELS);
        const size_t texels = all.off[all.L + 1];
        if ((rc = dev_alloc(h, &h->bl.d, texels, nullptr)) || (rc = dev_alloc(h, &h->bl.u, texels, nullptr)) || (rc = dev_alloc(h, &h->bl.out_u8, npix, nullptr))) {
            h->bl = decltype(h->bl)(); // (what was allocated stays on the handle's list and is freed with it)
            return rc;
        }
    }
    RpBloomRun r;
    memset(&r, 0, sizeof(r));
    bool copied = false;
    if ((rc = display_args(h, p->source, p->tone_mapping_mode, p->white_balance, h->bl.out_u8, r.comp.x, &copied))) return rc;
    h->bl.levels = 0;
    h->bl.asked = p->levels;
    if (!copied) {
        const bool metered = p->exposure_mode == 1;
        const float scale = metered ? 0.0f : manual_exposure_scale(h);
        r.pyr = rp_bloom_pyramid((uint32_t)h->width, (uint32_t)h->height, p->levels);
        r.pf = rp_bloom_prefilter_args(metered ? h->ae.state : nullptr, scale, p->threshold, p->knee, p->clamp);
        r.comp.x.state = metered ? h->ae.state : nullptr;
        r.comp.x.scale = scale;
        r.comp.W = h->width;
        r.comp.H = h->height;
        r.comp.gain = rp_bloom_gain(p->intensity, p->scatter, r.pyr.L);
        r.comp.add = p->intensity != 0.0f ? 1 : 0;
        r.d = h->bl.d;
        r.u = h->bl.u;
        r.scatter = p->scatter;
        r.max_blocks = (unsigned)h->num_cus * 8u;
        r.stages = 7;
        rp_bloom_enqueue<RP_BLOOM_SHIP_TILE != 0, RP_BLOOM_SHIP_TAIL != 0>(r, h->stream); // (which forms, and why: profiles/bloom_notes.md)
        HIP_TRY(h, hipGetLastError());
        h->bl.levels = r.pyr.L;
    }
    h->bl.serial = h->finished_serial;
    return RPTR_OK;
}

extern "C++" {
static int check_bloomed(rptr_hip *h) {
    if (!h->bl.out_u8 || h->bl.serial == 0) return fail(h, RPTR_E_INVALID, "no bloomed image: call rptr_hip_bloom first");
    if (h->bl.serial != h->finished_serial)
        return fail(h, RPTR_E_INVALID, "the bloomed image is stale: a later frame has finished since rptr_hip_bloom ran; call it again for that frame");
    return RPTR_OK;
}
}
int rptr_hip_readback_bloomed_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    const int rc = check_bloomed(h);
    return rc ? rc : readback_rows<uchar4>(h, h->bl.out_u8, reinterpret_cast<uchar4 *>(rgba), n_bytes / 4);
}

int rptr_hip_bloom_levels(const rptr_hip_t *h, uint32_t *out_levels) {
    if (!h || !out_levels) return fail(nullptr, RPTR_E_INVALID, "NULL argument");
    if (!h->bl.out_u8 || h->bl.serial == 0) return fail(nullptr, RPTR_E_INVALID, "no bloomed image: call rptr_hip_bloom first");
    *out_levels = (uint32_t)h->bl.levels;
    return RPTR_OK;
}

int rptr_hip_readback_bloom_level_f32(rptr_hip_t *h, int which, uint32_t level, float *rgba, size_t n_floats) {
    if (!h || !rgba) return fail(h, RPTR_E_INVALID, "NULL argument");
    int rc;
    if ((rc = check_bloomed(h))) return rc;
    if (which != 0 && which != 1) return fail(h, RPTR_E_INVALID, "rptr_hip_readback_bloom_level_f32: which = %d (0: the down pyramid d, 1: the up pyramid u)", which);
    if (level < 1 || level > (uint32_t)h->bl.levels)
        return fail(h, RPTR_E_INVALID, "rptr_hip_readback_bloom_level_f32: level %u is outside 1 .. %d, the levels of the last call", level, h->bl.levels);
    const RpBloomPyramid pyr = rp_bloom_pyramid((uint32_t)h->width, (uint32_t)h->height, h->bl.asked);
    const size_t texels = (size_t)pyr.w[level] * pyr.h[level];
    if (n_floats / 4 < texels) return fail(h, RPTR_E_INVALID, "read-back buffer too small for level %u: %zu < %zu floats", level, n_floats, 4 * texels);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(rgba, (which ? h->bl.u : h->bl.d) + pyr.off[level], texels * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RPTR_OK;
}

int rptr_hip_set_light_sampling_variant(rptr_hip_t *h, int variant) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (variant != 0 && variant != 1) return fail(h, RPTR_E_INVALID, "unknown light sampling variant %d (0 = NONE, 1 = RIS)", variant);
    h->lights_disabled = variant == 0;
    return RPTR_OK;
}

int rptr_hip_build_bvh_host(const RptrSceneDesc *scene, void *nodes, size_t *n_nodes, void *tris, size_t *n_tris, void *instances,
                            size_t *n_instances, int32_t *out_stack_need) {
    if (!scene) return fail(nullptr, RPTR_E_INVALID, "NULL scene");
    {
        const std::string bad = validate_scene_tables(scene);
        if (!bad.empty()) return fail(nullptr, RPTR_E_INVALID, "%s", bad.c_str());
    }
    HostBvh B;
    build_host_bvh(scene, B, effective_default_options());
    if (nodes && n_nodes && *n_nodes >= B.nodes.size()) memcpy(nodes, B.nodes.data(), B.nodes.size() * sizeof(RptrBvh4Node));
    if (tris && n_tris && *n_tris >= B.tris.size()) memcpy(tris, B.tris.data(), B.tris.size() * sizeof(RptrBvhTri));
    if (instances && n_instances && *n_instances >= B.insts.size()) memcpy(instances, B.insts.data(), B.insts.size() * sizeof(RptrBvhInstance));
    if (n_nodes) *n_nodes = B.nodes.size();
    if (n_tris) *n_tris = B.tris.size();
    if (n_instances) *n_instances = B.insts.size();
    if (out_stack_need) *out_stack_need = B.stack_need;
    return RPTR_OK;
}

int rptr_hip_export_bvh(rptr_hip_t *h, void *nodes, size_t *n_nodes, void *tris, size_t *n_tris, void *instances, size_t *n_instances) {
    if (!h) return fail(nullptr, RPTR_E_INVALID, "NULL handle");
    if (!h->have_scene) return fail(h, RPTR_E_INVALID, "export before set_scene");
    {
        int rc0 = ensure_master_tree(h);
        if (rc0) return rc0;
    }
    if (h->host_bvh_stale) { // a refit happened on the device: refresh the host mirror first
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipMemcpy(h->h_nodes.data(), h->master.dscene.nodes, h->h_nodes.size() * sizeof(RptrBvh4Node), hipMemcpyDeviceToHost));
        if (!h->h_tris.empty()) HIP_TRY(h, hipMemcpy(h->h_tris.data(), h->master.dscene.tris, h->h_tris.size() * sizeof(RptrBvhTri), hipMemcpyDeviceToHost));
        if (h->host_insts_stale && !h->h_insts.empty()) // (instances moved: rptr_hip_update_instances)
            HIP_TRY(h, hipMemcpy(h->h_insts.data(), h->master.dscene.insts, h->h_insts.size() * sizeof(RptrBvhInstance), hipMemcpyDeviceToHost));
        h->host_insts_stale = false;
        h->host_bvh_stale = false;
    }
    if (nodes && n_nodes && *n_nodes >= h->h_nodes.size()) memcpy(nodes, h->h_nodes.data(), h->h_nodes.size() * sizeof(RptrBvh4Node));
    if (tris && n_tris && *n_tris >= h->h_tris.size()) memcpy(tris, h->h_tris.data(), h->h_tris.size() * sizeof(RptrBvhTri));
    if (instances && n_instances && *n_instances >= h->h_insts.size())
        memcpy(instances, h->h_insts.data(), h->h_insts.size() * sizeof(RptrBvhInstance));
    if (n_nodes) *n_nodes = h->h_nodes.size();
    if (n_tris) *n_tris = h->h_tris.size();
    if (n_instances) *n_instances = h->h_insts.size();
    return RPTR_OK;
}

