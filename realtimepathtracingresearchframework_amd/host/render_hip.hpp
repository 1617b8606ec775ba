// render_hip.hpp -- C++ host class over the C ABI, shaped like the reference's
// `struct RenderBackend` (librender/render_backend.h:68-116) so that the adapter a
// maintainer adds on the reference side is a thin subclass shim:
// same method names, same argument meaning, same error convention (failures throw
// a std::runtime_error like `logged_exception`, util/error_io.h:27-29; read-backs
// return the element count or 0, render_vulkan.cpp:2256-2275; configure_for
// returns bool). glm-free: vectors are float[3].
#pragma once
#include "../../include/rptr_hip.h"

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace rptr {

static_assert(sizeof(RptrOcclusionParams) == 16, "RptrOcclusionParams: flags, alpha_cutoff, two reserved words (include/rptr_hip.h)");
static_assert(sizeof(RptrProbeParams) == 80, "RptrProbeParams: four words, the rotation, blend / clamp / t_max, max_run_rays, three reserved words (include/rptr_hip.h)");
static_assert(sizeof(RptrDenoiseTemporalParams) == 64, "RptrDenoiseTemporalParams: ten parameters and six reserved words (include/rptr_hip.h)");
static_assert(sizeof(RptrTaaUpscaleParams) == 16, "RptrTaaUpscaleParams: factor, reset_history, two reserved words (include/rptr_hip.h)");
static_assert(sizeof(RptrBloomParams) == 64, "RptrBloomParams: four switches, five parameters, three gains, four reserved words (include/rptr_hip.h)");
static_assert(sizeof(RptrSurfaceHit) == 96, "RptrSurfaceHit: six 16-byte rows per surface query (include/rptr_hip.h)");

struct RenderStats { // librender/render_backend.h:15-24
    float render_time = 0;
    float rays_per_second = 0;
    int spp = 0;
    short frame_stats_delay = 0;
    bool has_valid_frame_stats = true;
    size_t total_device_bytes_allocated = 0;
};

struct RenderCameraParams { // librender/render_backend.h:26-31
    float pos[3], dir[3], up[3];
    float fovy;
};

struct RenderConfiguration { // librender/render_backend.h:33-40
    RenderCameraParams camera;
    double time = 0.0;
    int active_variant = 0;
    bool reset_accumulation = false;
    bool freeze_frame = false;
    int active_swap_buffer_count = -1; // :37: > 0 limits the frames in flight (the application sets 1 when it renders synchronously, app.cpp:386-389)
};

// util/display/render_graphic.h: `CommandStream*` is what the application hands to begin_frame / draw_frame / end_frame -- the display's
// stream (asynchronous: the frame is queued, up to MAX_SWAP_BUFFERS of them are in flight, statistics lag frame_stats_delay frames) or
// nullptr (synchronous, app.cpp:385-389). Here a frame's launches go to the HIP streams of the library's frame contexts, so the type only
// carries the distinction.
struct CommandStream {};

// The RenderBackendOptions (render_params.glsl.h:74-99) that are switches of the HOST class alone, not keys of the library's option table.
// enable_raytraced_dof: false hands the library aperture_radius = 0 and focal_length = 0 whatever `params` says (render_vulkan.cpp:2945-2947);
// `params` itself stays the caller's.
struct RenderBackendOptions {
    bool enable_raytraced_dof = true;
};

class RenderHip {
public:
    // public data members the app mutates directly (render_backend.h:69-76)
    RptrRenderParams params;
    RenderBackendOptions options;
    RptrLightSamplingConfig lighting_params;
    RenderCameraParams camera;
    bool reset_accumulation = false;
    bool freeze_frame = false;

    static const int MAX_SWAP_BUFFERS = 2; // util/display/render_graphic.h:19

    // frames_in_flight: the library's frame contexts. The reference's backend owns MAX_SWAP_BUFFERS sets of per-frame resources whatever the
    // application does with them (vulkan/render_vulkan.h:128-131); so does this one by default: draw_frame(cmd_stream != nullptr) then has
    // two frames in flight, draw_frame(nullptr) renders one at a time on the same handle.
    // create_flags: RPTR_CREATE_*. 0 (an embedded plugin): the library touches nothing outside its handle; a host that owns its process
    // (bin/rptr_hip) passes RPTR_CREATE_SET_HW_QUEUES so that every frame context's stream gets a hardware queue (INTEGRATION.md "Hardware queues").
    explicit RenderHip(int device_ordinal = 0, int rank = 0, int world_size = 1, int stripe_rows = 32, void *hip_stream = nullptr,
                       int frames_in_flight = MAX_SWAP_BUFFERS, uint32_t create_flags = 0u) {
        RptrCreateInfo info{device_ordinal, rank, world_size, stripe_rows, hip_stream, frames_in_flight, RPTR_HIP_ABI_VERSION, create_flags, 0u};
        int rc = rptr_hip_create(&info, &h_);
        if (rc != RPTR_OK) throw std::runtime_error(std::string("rptr_hip_create: ") + rptr_hip_last_error(nullptr));
        contexts_ = frames_in_flight < 1 ? 1 : (frames_in_flight > 16 ? 16 : frames_in_flight);
        params = RptrRenderParams{1, RPTR_MAX_PATH_DEPTH, RPTR_DEFAULT_RR_PATH_DEPTH, 0, 0.f, 2.5f, 1.f, 4.f, 0, 0, 0.f, -1, 0, 8, 0, 1, 35.f, 0, 0, 0};
        lighting_params = RptrLightSamplingConfig{0.f, 16, 15.f, 0.f};
    }
    ~RenderHip() { rptr_hip_destroy(h_); }
    RenderHip(const RenderHip &) = delete;
    RenderHip &operator=(const RenderHip &) = delete;

    std::string name() const { return rptr_hip_name(); }
    std::vector<std::string> variant_names() const { return {"wavefront-gltf", "wavefront-diffuse", "wavefront-gltf-transmission"}; }

    // library options (include/rptr_hip.h "Options"): per-handle switches that take effect at initialize / set_scene / the next frame
    void set_option(const char *key, int64_t value) { check(rptr_hip_set_option(h_, key, value)); }
    int64_t get_option(const char *key) const {
        int64_t v = 0;
        check(rptr_hip_get_option(h_, key, &v));
        return v;
    }
    void initialize(const int fb_width, const int fb_height) {
        flush_pipeline();
        check(rptr_hip_initialize(h_, fb_width, fb_height));
    }
    // set_scene(const Scene&): the adapter flattens Scene into RptrSceneDesc
    void set_scene(const RptrSceneDesc &scene) {
        flush_pipeline();
        check(rptr_hip_set_scene(h_, &scene));
    }
    // update_config(SceneConfig): the adapter runs the reference's Hosek fit and passes the result
    void update_config(const RptrSceneParams &scene_params) { scene_params_ = scene_params; have_scene_params_ = true; }
    // dynamic meshes: float positions of one geometry (3 per unrolled vertex), then BLAS update + TLAS refit
    void update_vertices(uint32_t geometry, const float *xyz, uint32_t num_vertices) { check(rptr_hip_update_vertices(h_, geometry, xyz, num_vertices)); }
    void update_vertices_device(uint32_t geometry, const float *device_xyz, uint32_t num_vertices) {
        check(rptr_hip_update_vertices_device(h_, geometry, device_xyz, num_vertices));
    }
    void refit() { check(rptr_hip_refit(h_)); }
    // moving instances: `count` row-major 3x4 object-to-world transforms for scene instances [first, first + count), applied by the next refit
    void update_instances(uint32_t first, uint32_t count, const float *transforms12) { check(rptr_hip_update_instances(h_, first, count, transforms12)); }
    void update_instances_device(uint32_t first, uint32_t count, const float *device_transforms12) {
        check(rptr_hip_update_instances_device(h_, first, count, device_transforms12));
    }
    void set_tlas_policy(int mode) { check(rptr_hip_set_tlas_policy(h_, mode)); } // RPTR_TLAS_REBUILD | RPTR_TLAS_REFIT
    uint64_t tlas_rebuild_count() const {
        uint64_t n = 0;
        rptr_hip_tlas_rebuild_count(h_, &n);
        return n;
    }
    // moving lights: where every entry of RptrSceneDesc.lights came from (lights.hpp collect_light_sources / prepare_lights), one record
    // per light; afterwards emissive instances may move and refit() re-places the lights. An empty vector unregisters; set_scene never
    // registers on its own and a new set_scene drops the registration.
    void set_light_sources(const std::vector<RptrLightSource> &sources) {
        flush_pipeline();
        check(rptr_hip_set_light_sources(h_, sources.empty() ? nullptr : sources.data(), (uint32_t)sources.size()));
    }
    // the master scene copy's light buffer after all pending work (num_lights: RptrSceneDesc.num_lights of the scene)
    std::vector<RptrTriLightData> readback_lights(uint32_t num_lights) {
        std::vector<RptrTriLightData> out(num_lights);
        check(rptr_hip_readback_lights(h_, out.data(), num_lights));
        return out;
    }
    // skinned meshes: one RptrSkinVertex per unrolled vertex binds a geometry of a dynamic mesh (its rest pose: the positions it has now;
    // an empty vector unbinds); bone matrices are row-major 3x4, rest to posed object space; skin() writes positions and shading normals
    // of every bound geometry on the device, refit() follows as after update_vertices
    void set_skin(uint32_t geometry, const std::vector<RptrSkinVertex> &vertices) {
        flush_pipeline();
        check(rptr_hip_set_skin(h_, geometry, vertices.empty() ? nullptr : vertices.data(), (uint32_t)vertices.size()));
    }
    void update_bones(uint32_t first, uint32_t count, const float *transforms12) { check(rptr_hip_update_bones(h_, first, count, transforms12)); }
    void update_bones_device(uint32_t first, uint32_t count, const float *device_transforms12) {
        check(rptr_hip_update_bones_device(h_, first, count, device_transforms12));
    }
    // morph targets: the stage in front of the skinner. One vector of RptrMorphDelta per target (sparse: the unrolled vertices the target
    // moves, each at most once; a target may be empty); the weights start at zero; no targets at all unbinds. skin() runs both deformers.
    void set_morph_targets(uint32_t geometry, const std::vector<std::vector<RptrMorphDelta>> &targets) {
        flush_pipeline();
        std::vector<RptrMorphTargetDesc> descs(targets.size());
        for (size_t t = 0; t < targets.size(); ++t) descs[t] = RptrMorphTargetDesc{targets[t].empty() ? nullptr : targets[t].data(), (uint32_t)targets[t].size(), 0u};
        check(rptr_hip_set_morph_targets(h_, geometry, descs.empty() ? nullptr : descs.data(), (uint32_t)descs.size()));
    }
    void update_morph_weights(uint32_t geometry, uint32_t first_target, uint32_t count, const float *weights) {
        check(rptr_hip_update_morph_weights(h_, geometry, first_target, count, weights));
    }
    void update_morph_weights_device(uint32_t geometry, uint32_t first_target, uint32_t count, const float *device_weights) {
        check(rptr_hip_update_morph_weights_device(h_, geometry, first_target, count, device_weights));
    }
    void skin() { check(rptr_hip_skin(h_)); }
    // recomputed normals: one label per UNROLLED vertex (corners with the same label share a normal; RPTR_NORMAL_GROUP_FLAT: the face
    // normal; host/normal_groups.hpp welds a mesh that has no index buffer); no labels at all unbinds. recompute_normals() goes between
    // update_vertices* / skin() and refit().
    void set_normal_groups(uint32_t geometry, const std::vector<uint32_t> &groups, bool flip = false) {
        flush_pipeline();
        check(rptr_hip_set_normal_groups(h_, geometry, groups.empty() ? nullptr : groups.data(), (uint32_t)groups.size(), flip && !groups.empty() ? RPTR_NORMALS_FLIP : 0u));
    }
    void recompute_normals() { check(rptr_hip_recompute_normals(h_)); }
    // dynamic textures: new level-0 texels (n_bytes == 4 * width * height as set_scene received them; nullptr, 0 keeps level 0), and with
    // generate_mips the full chain made on the device. Returns false, nothing changed, for a texture an emissive material reads
    // (RPTR_E_UNSUPPORTED: the scene's lights were made from it); every other refusal throws. Waits for the frames in flight.
    bool update_texture(uint32_t texture, const uint8_t *rgba8, size_t n_bytes, bool generate_mips = true) {
        flush_pipeline();
        const int rc = rptr_hip_update_texture(h_, texture, rgba8, n_bytes, generate_mips ? RPTR_TEXTURE_GENERATE_MIPS : 0u);
        if (rc == RPTR_E_UNSUPPORTED) return false;
        check(rc);
        return true;
    }
    bool update_texture_device(uint32_t texture, const uint8_t *device_rgba8, size_t n_bytes, bool generate_mips = true) { // (ordered on the backend's stream)
        flush_pipeline();
        const int rc = rptr_hip_update_texture_device(h_, texture, device_rgba8, n_bytes, generate_mips ? RPTR_TEXTURE_GENERATE_MIPS : 0u);
        if (rc == RPTR_E_UNSUPPORTED) return false;
        check(rc);
        return true;
    }
    uint32_t texture_levels(uint32_t texture) const {
        uint32_t n = 0;
        check(rptr_hip_texture_levels(h_, texture, &n));
        return n;
    }
    // one level of a texture whose level 0 is width x height: max(1, width >> level) x max(1, height >> level) RGBA8 texels, row 0 first
    std::vector<uint8_t> readback_texture(uint32_t texture, uint32_t level, uint32_t width, uint32_t height) {
        const uint32_t w = level < 32 && (width >> level) ? width >> level : 1u, h = level < 32 && (height >> level) ? height >> level : 1u;
        std::vector<uint8_t> out((size_t)4 * w * h);
        check(rptr_hip_readback_texture(h_, texture, level, out.data(), out.size()));
        return out;
    }
    // the master copy's positions (3 floats per vertex) and, when `normal_words` is given, normal words of a bound geometry
    std::vector<float> readback_skinned(uint32_t geometry, uint32_t num_vertices, std::vector<uint32_t> *normal_words = nullptr) {
        std::vector<float> xyz((size_t)num_vertices * 3);
        if (normal_words) normal_words->assign(num_vertices, 0u);
        check(rptr_hip_readback_skinned(h_, geometry, xyz.data(), normal_words ? normal_words->data() : nullptr, num_vertices));
        return xyz;
    }
    // RenderBackendOptions (render_params.glsl.h:56-93): the point set with the table its render extension uploads, and the BVH policy
    void set_rng_variant(int rng_variant, const std::vector<uint32_t> &table = {}) {
        check(rptr_hip_set_rng_variant(h_, rng_variant, table.empty() ? nullptr : table.data(), table.size() * sizeof(uint32_t)));
    }
    void set_bvh_policy(bool force_bvh_rebuild, int rebuild_triangle_budget) {
        check(rptr_hip_set_bvh_policy(h_, force_bvh_rebuild ? 1 : 0, rebuild_triangle_budget));
    }
    bool configure_for(int variant_idx) {
        if (variant_idx != RPTR_VARIANT_GLTF && variant_idx != RPTR_VARIANT_SIMPLE && variant_idx != RPTR_VARIANT_GLTF_TRANSMISSION) return false;
        variant_ = variant_idx;
        return true;
    }

    // ---- the reference's frame loop (app.cpp:453-469): begin_frame -> draw_frame -> end_frame with the application's CommandStream*.
    // cmd_stream != nullptr: the frame is SUBMITTED (rptr_hip_render_async, this frame's camera) and the call returns; at most
    // active_swap_buffer_count (<= MAX_SWAP_BUFFERS <= the handle's frame contexts) frames are in flight: begin_frame of frame i + 2 waits for
    // frame i -- as RenderVulkan::begin_frame waits for the render-done event of the swap index it is about to reuse
    // (vulkan/render_vulkan.cpp:1953-1972) -- and takes frame i's timings, so stats() lags frame_stats_delay = 2 frames (:2229-2243).
    // cmd_stream == nullptr: synchronous -- everything in flight is finished first, stats() is this frame's.
    // Read-backs return the newest frame: they wait for everything in flight (the reference's read-back goes through the synchronous
    // command stream of the same queue, :2256-2275).
    void begin_frame(CommandStream *cmd_stream, const RenderConfiguration &config) {
        begin_frame(config);
        int active = config.active_swap_buffer_count > 0 ? config.active_swap_buffer_count : MAX_SWAP_BUFFERS;
        active = active < contexts_ ? active : contexts_;
        if (active > MAX_SWAP_BUFFERS) active = MAX_SWAP_BUFFERS;
        if (!cmd_stream || active != active_swap_) flush_pipeline(); // (a change of depth: start from an empty ring)
        active_swap_ = cmd_stream ? active : 1;
        swap_index_ = (swap_index_ + 1) % active_swap_;
        wait_slot(swap_index_); // the frame that used this swap index: done by now or waited for, its timings are the stats of this frame
    }
    void draw_frame(CommandStream *cmd_stream, int variant_idx) {
        if (variant_idx >= 0 && !configure_for(variant_idx)) throw std::runtime_error("rptr_hip: unknown variant");
        if (!cmd_stream) {
            draw_frame(0);
            asynchronous_ = false;
            return;
        }
        push_state();
        const RptrCamera cam = abi_camera();
        check(rptr_hip_render_async(h_, &cam, variant_, batch_spp(0), reset_accumulation ? 1 : 0, 0, &ticket_[swap_index_]));
        pending_[swap_index_] = true;
        slot_reset_[swap_index_] = reset_accumulation;
        slot_dt_[swap_index_] = frame_dt_;
        asynchronous_ = true;
        count_frame(batch_spp(0));
    }
    void end_frame(CommandStream * /*cmd_stream*/, int /*variant_idx*/) {} // process_samples is sequenced inside the frame's own launch sequence
    void flush_pipeline() { // RenderBackend::flush_pipeline (vulkan/render_vulkan.cpp:2245-2248): nothing in flight afterwards
        for (int k = 1; k <= MAX_SWAP_BUFFERS; ++k) { // oldest first: the newest frame is the one waited for last (what read-backs return)
            wait_slot((swap_index_ + k) % MAX_SWAP_BUFFERS);
        }
    }

    void begin_frame(const RenderConfiguration &config) { // render_backend.cpp:17-23
        camera = config.camera;
        reset_accumulation = config.reset_accumulation;
        freeze_frame = config.freeze_frame;
        configure_for(config.active_variant);
        frame_dt_ = have_time_ && config.time > last_time_ ? float(config.time - last_time_) : 0.0f; // (auto_exposure_every_frame)
        last_time_ = config.time;
        have_time_ = true;
    }
    void draw_frame(int spp = 0) { // synchronous
        flush_pipeline();
        push_state();
        const RptrCamera cam = abi_camera();
        check(rptr_hip_render(h_, &cam, variant_, batch_spp(spp), reset_accumulation ? 1 : 0, 0, &last_));
        ++stats_serial_;
        frame_collected(reset_accumulation, frame_dt_);
        count_frame(batch_spp(spp));
        asynchronous_ = false;
    }
    // frames in flight: begin_frame + asynchronous draw_frame, collected with wait(ticket)
    // ---- explicit tickets (hosts that schedule deeper than the reference's two swap buffers: render_group.hpp, bin/rptr_hip --frames-in-flight)
    uint64_t render_async(const RenderConfiguration &config, int spp = 0) {
        begin_frame(config);
        push_state();
        const RptrCamera cam = abi_camera();
        uint64_t ticket = 0;
        check(rptr_hip_render_async(h_, &cam, variant_, batch_spp(spp), reset_accumulation ? 1 : 0, 0, &ticket));
        count_frame(batch_spp(spp));
        return ticket;
    }
    // several frames of the same view in ONE launch sequence (rptr_hip_render_batch_async): tickets[k] is frame k's
    std::vector<uint64_t> render_batch_async(const RenderConfiguration &config, int spp, int n_frames, bool reset_rest = true) {
        begin_frame(config);
        push_state();
        const RptrCamera cam = abi_camera();
        std::vector<uint64_t> tickets((size_t)n_frames, 0);
        check(rptr_hip_render_batch_async(h_, &cam, variant_, batch_spp(spp), n_frames, reset_accumulation ? 1 : 0, reset_rest ? 1 : 0, 0, tickets.data()));
        for (int k = 0; k < n_frames; ++k) {
            count_frame(batch_spp(spp));
            if (k + 1 < n_frames) reset_accumulation = reset_rest;
        }
        reset_accumulation = false;
        return tickets;
    }
    // ... with a camera per frame (rptr_hip_render_batch_cameras_async): the application moves the camera every frame (app.cpp:350-469);
    // configs[k] is frame k's RenderConfiguration (camera; variant / freeze of configs[0]; reset_accumulation of configs[0] for frame 0,
    // reset_rest for the others -- a moved camera restarts the accumulation)
    std::vector<uint64_t> render_batch_cameras_async(const RenderConfiguration *configs, int n_frames, int spp = 0, bool reset_rest = true) {
        begin_frame(configs[0]);
        push_state();
        std::vector<RptrCamera> cams((size_t)n_frames);
        for (int k = 0; k < n_frames; ++k) {
            camera = configs[k].camera;
            cams[(size_t)k] = abi_camera();
        }
        std::vector<uint64_t> tickets((size_t)n_frames, 0);
        check(rptr_hip_render_batch_cameras_async(h_, cams.data(), variant_, batch_spp(spp), n_frames, reset_accumulation ? 1 : 0, reset_rest ? 1 : 0, 0, tickets.data()));
        for (int k = 0; k < n_frames; ++k) {
            count_frame(batch_spp(spp));
            if (k + 1 < n_frames) reset_accumulation = reset_rest;
        }
        reset_accumulation = false;
        return tickets;
    }
    RenderStats wait(uint64_t ticket) {
        check(rptr_hip_wait(h_, ticket, &last_));
        ++stats_serial_;
        RenderStats s = stats();
        s.spp = last_.spp; // (the waited frame's own count)
        s.frame_stats_delay = 0;
        return s;
    }
    void end_frame() {} // process_samples is sequenced inside draw_frame on the same stream
    RenderStats render(const RenderConfiguration &config, int spp = 0) {
        begin_frame(config);
        draw_frame(spp);
        end_frame();
        return stats();
    }
    // render_vulkan.cpp:2229-2243: the timings of the frame whose swap buffers this frame took over (asynchronous: frame_stats_delay frames
    // ago), spp = samples accumulated INCLUDING the frame just submitted (:2152-2154). rays_per_second is filled here; the reference leaves -1
    RenderStats stats() const {
        RenderStats s;
        s.render_time = last_.render_time_ms;
        s.has_valid_frame_stats = last_.render_time_ms != 0.0f;
        s.rays_per_second = s.has_valid_frame_stats ? float(double(last_.rays_closest + last_.rays_shadow) / (last_.render_time_ms * 1e-3)) : -1.f;
        s.frame_stats_delay = short(asynchronous_ ? active_swap_ : 0);
        s.spp = accumulated_spp_;
        s.total_device_bytes_allocated = (size_t)last_.device_bytes_allocated;
        return s;
    }
    uint64_t rays_of_last_stats() const { return last_.rays_closest + last_.rays_shadow; }
    uint64_t stats_serial() const { return stats_serial_; } // grows whenever stats() starts to describe another frame

    void get_framebuffer_size(uint32_t whc[3]) const { check(rptr_hip_get_framebuffer_size(h_, whc)); }
    size_t readback_framebuffer(size_t buffer_size, float *buffer) { // RGBA32F accumulation buffer
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        flush_pipeline();
        check(rptr_hip_readback_f32(h_, buffer, buffer_size));
        return need;
    }
    size_t readback_framebuffer(size_t buffer_size, unsigned char *buffer) { // sRGB RGBA8
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        flush_pipeline();
        check(rptr_hip_readback_u8(h_, buffer, buffer_size));
        return need;
    }

    // The denoiser (include/rptr_hip.h rptr_hip_denoise): the frame the read-backs return -- everything in flight is finished first --
    // into images of its own; the frame's images, its history and the statistics stay as they are. Asynchronous on the backend's stream.
    static RptrDenoiseParams denoise_defaults() {
        RptrDenoiseParams p;
        rptr_hip_denoise_defaults(&p);
        return p;
    }
    void denoise(const RptrDenoiseParams &p) {
        flush_pipeline();
        check(rptr_hip_denoise(h_, &p));
    }
    size_t readback_denoised(size_t buffer_size, float *buffer) { // RGBA32F
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        if (denoise_temporal_every_frame_) flush_pipeline(); // (the frames in flight are collected, and denoised, first)
        check(rptr_hip_readback_denoised_f32(h_, buffer, buffer_size));
        return need;
    }
    size_t readback_denoised(size_t buffer_size, unsigned char *buffer) { // sRGB RGBA8
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        if (denoise_temporal_every_frame_) flush_pipeline(); // (the frames in flight are collected, and denoised, first)
        check(rptr_hip_readback_denoised_u8(h_, buffer, buffer_size));
        return need;
    }

    // The temporal denoiser (include/rptr_hip.h rptr_hip_denoise_temporal): the frame the read-backs return -- everything in flight is
    // finished first -- blended with the history the previous call left, into the denoiser's images (readback_denoised); one call per
    // frame, p.reset_history = 1 for a frame that does not follow the previous call's (a restarted accumulation, a skipped frame).
    static RptrDenoiseTemporalParams denoise_temporal_defaults() {
        RptrDenoiseTemporalParams p;
        rptr_hip_denoise_temporal_defaults(&p);
        return p;
    }
    void denoise_temporal(const RptrDenoiseTemporalParams &p) {
        flush_pipeline();
        check(rptr_hip_denoise_temporal(h_, &p));
    }
    // ... or with every frame of the reference's loop, as upscale_every_frame below: issued when the frame it belongs to has been
    // collected, with `p` and reset_history = that frame's reset_accumulation.
    void denoise_temporal_every_frame(bool on, const RptrDenoiseTemporalParams &p = denoise_temporal_defaults()) {
        denoise_temporal_every_frame_ = on;
        denoise_temporal_params_ = p;
    }
    size_t readback_denoise_history(size_t buffer_size, float *buffer) { // RGBA32F: the blended demodulated colour, the history length
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        if (denoise_temporal_every_frame_) flush_pipeline();
        check(rptr_hip_readback_denoise_history_f32(h_, buffer, buffer_size));
        return need;
    }

    // Temporal 2x upscaling (include/rptr_hip.h rptr_hip_taa_upscale): the frame the read-backs return -- everything in flight is finished
    // first -- and the previous call's output into a display-size image of its own; the frame's images and histories stay as they are.
    // Asynchronous on the backend's stream. p.reset_history = 1 for the frame that restarted the accumulation.
    static RptrTaaUpscaleParams taa_upscale_defaults() {
        RptrTaaUpscaleParams p;
        rptr_hip_taa_upscale_defaults(&p);
        return p;
    }
    void taa_upscale(const RptrTaaUpscaleParams &p) {
        flush_pipeline();
        check(rptr_hip_taa_upscale(h_, &p));
    }
    // Auto-exposure (include/rptr_hip.h rptr_hip_auto_exposure): the frame the read-backs return -- everything in flight is finished first
    // -- or its denoised image (p.source = 1) is metered, the exposure value adapts on the device, and a display-ready RGBA8 image of its
    // own is written; nothing else is touched. Asynchronous on the backend's stream. `params.exposure`, as it is now, is added to the
    // metered value.
    static RptrAutoExposureParams auto_exposure_defaults() {
        RptrAutoExposureParams p;
        rptr_hip_auto_exposure_defaults(&p);
        return p;
    }
    void auto_exposure(const RptrAutoExposureParams &p) {
        flush_pipeline();
        push_state();
        check(rptr_hip_auto_exposure(h_, &p));
        if (p.mode == 1) ++exposure_calls_;
    }
    // ... or with every frame of the reference's loop, as upscale_every_frame below (after that frame's temporal denoise when both are on:
    // p.source = 1 then meters its result), with `p`, reset_history = that frame's reset_accumulation and dt = the frame's time step,
    // RenderConfiguration::time minus the previous frame's (0, a jump to the target, for the first frame and for a clock that stands)
    void auto_exposure_every_frame(bool on, const RptrAutoExposureParams &p = auto_exposure_defaults()) {
        auto_exposure_every_frame_ = on;
        auto_exposure_params_ = p;
    }
    size_t readback_exposed(size_t buffer_size, unsigned char *buffer) { // sRGB RGBA8
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        if (auto_exposure_every_frame_) flush_pipeline(); // (the frames in flight are collected, and exposed, first)
        check(rptr_hip_readback_exposed_u8(h_, buffer, buffer_size));
        return need;
    }
    // newest = false: what the call of the frame collected last left -- under a command stream that frame is frame_stats_delay frames
    // behind, like stats(); nothing in flight is waited for (exposure_state_ready(): such a call has run)
    RptrExposureState readback_exposure_state(bool newest = true) {
        if (auto_exposure_every_frame_ && newest) flush_pipeline();
        RptrExposureState st;
        check(rptr_hip_readback_exposure_state(h_, &st));
        return st;
    }
    bool exposure_state_ready() const { return exposure_calls_ > 0; }
    // Bloom (include/rptr_hip.h rptr_hip_bloom): glare for the frame the read-backs return -- everything in flight is finished first -- or
    // its denoised image (p.source = 1), into an RGBA8 image of its own; nothing else is touched. Asynchronous on the backend's stream.
    // p.exposure_mode = 1 uses the scale the last metering auto_exposure() left on the device (call order: auto_exposure, bloom, present);
    // 0 uses `params.exposure` as it is now.
    static RptrBloomParams bloom_defaults() {
        RptrBloomParams p;
        rptr_hip_bloom_defaults(&p);
        return p;
    }
    void bloom(const RptrBloomParams &p) {
        flush_pipeline();
        push_state();
        check(rptr_hip_bloom(h_, &p));
    }
    size_t readback_bloomed(size_t buffer_size, unsigned char *buffer) { // sRGB RGBA8
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        check(rptr_hip_readback_bloomed_u8(h_, buffer, buffer_size));
        return need;
    }
    uint32_t bloom_levels() {
        uint32_t n = 0;
        check(rptr_hip_bloom_levels(h_, &n));
        return n;
    }
    // Object motion (include/rptr_hip.h rptr_hip_object_motion): track_object_motion after set_scene; object_motion after the frame that
    // followed update_* + refit and before denoise_temporal / taa_upscale -- everything in flight is finished first. Returns the pixels
    // whose motion vector was rewritten (waits for the pass).
    void track_object_motion(bool enable = true) { check(rptr_hip_track_object_motion(h_, enable ? 1 : 0)); }
    int64_t object_motion() {
        flush_pipeline();
        check(rptr_hip_object_motion(h_));
        int64_t n = 0;
        check(rptr_hip_get_option(h_, "object_motion_pixels", &n));
        return n;
    }
    // ... or with every frame of the reference's loop (begin_frame / draw_frame with or without a command stream), issued when the frame
    // it belongs to has been collected -- begin_frame's wait for the swap index it reuses, flush_pipeline, the synchronous draw_frame --
    // with reset_history = that frame's reset_accumulation. Frames collected through wait(ticket) are the host's to upscale.
    void upscale_every_frame(bool on) { upscale_every_frame_ = on; }
    size_t readback_upscaled(size_t buffer_size, unsigned char *buffer) { // sRGB RGBA8, twice the width and height
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 16;
        if (buffer_size < need) return 0;
        if (upscale_every_frame_) flush_pipeline();
        check(rptr_hip_readback_upscaled_u8(h_, buffer, buffer_size));
        return need;
    }

    // RenderGraphic::readback_aov (util/display/render_graphic.h:12-17,40): RGBA16F, the reference's AOVBufferIndex order
    enum AOVBufferIndex { AOVAlbedoRoughnessIndex = 0, AOVNormalDepthIndex, AOVMotionJitterIndex, AOVBufferCount };
    size_t readback_aov(AOVBufferIndex aov_index, size_t buffer_size, uint16_t *buffer, bool /*force_refresh*/ = false) {
        uint32_t whc[3];
        get_framebuffer_size(whc);
        const size_t need = size_t(whc[0]) * whc[1] * 4;
        if (buffer_size < need) return 0;
        flush_pipeline();
        check(rptr_hip_readback_aov(h_, int(aov_index), buffer, buffer_size));
        return need;
    }

    // enable_ray_queries / render_ray_queries with RQ_CLOSEST (render_backend.h:101-102; vulkan/render_vulkan.cpp:430-455,1867-1876): the
    // queries live in a DEVICE buffer the backend owns (ray_query_buffer), other device code fills it, the results land in
    // ray_result_buffer. ray_query_buffer() / ray_result_buffer() are the device addresses.
    void enable_ray_queries(const int max_queries, const int max_queries_per_pixel = 0) {
        check(rptr_hip_enable_ray_queries(h_, max_queries, max_queries_per_pixel, &ray_query_buffer_, &ray_result_buffer_));
    }
    void *ray_query_buffer() const { return ray_query_buffer_; }
    void *ray_result_buffer() const { return ray_result_buffer_; }
    bool render_ray_queries(int num_queries) { // the RQ_CLOSEST program: hit records (the reference's params / variant select nothing for it)
        if (!ray_query_buffer_) return false;
        check(rptr_hip_render_ray_queries(h_, num_queries));
        return true;
    }
    // RenderBackend::render_ray_queries(num_queries, params, variant_idx, ...) with a path-tracing variant (render_vulkan.cpp:2961-3059):
    // the path tracer runs on the query rays and ray_result_buffer receives (radiance.rgb, alpha) -- the mean over samples_per_query
    // samples from first_sample on (the reference: one sample, from 0). `camera` supplies the image-plane axes of the texture footprint,
    // as the reference's view does. An index that is no RPTR_VARIANT_* gpu program is refused (the RQ_CLOSEST program has the overload above).
    // render_params become the handle's RenderParams (rptr_hip_set_params): later frames render with them too.
    bool render_ray_queries(int num_queries, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera, int samples_per_query = 1,
                            int first_sample = 0) {
        if (!ray_query_buffer_) return false;
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_render_radiance_queries(h_, num_queries, &cam, variant_idx, samples_per_query, first_sample));
        return true;
    }
    // ... over HOST arrays (results4 is read as well as written: old means for first_sample > 0, slots of skipped queries)
    bool render_ray_queries(const RptrRenderRayQuery *queries, int num_queries, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera,
                            float *results4, int samples_per_query = 1, int first_sample = 0) {
        if (num_queries < 0) return false;
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_trace_radiance(h_, queries, num_queries, &cam, variant_idx, samples_per_query, first_sample, results4, nullptr));
        return true;
    }
    // Surface queries (include/rptr_hip.h rptr_hip_trace_surface): one RptrSurfaceHit per query -- position, normals and material at the closest
    // hit, decoded as the first shade of a frame decodes it for the AOV images; a miss has t = -1. `camera` supplies the image-plane axes of the
    // texture footprint, render_params become the handle's (pixel_radius sizes the footprint). Over the query buffer of enable_ray_queries
    // into a DEVICE buffer of the caller's, asynchronously on `hip_stream` (nullptr: the backend's) ...
    bool render_surface_queries(int num_queries, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera, RptrSurfaceHit *device_results,
                                void *hip_stream = nullptr) {
        if (!ray_query_buffer_) return false;
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_trace_surface_device(h_, nullptr, num_queries, &cam, variant_idx, device_results, hip_stream));
        return true;
    }
    // ... and over HOST arrays, synchronously (results is read as well as written: the slots of skipped queries are preserved)
    bool render_surface_queries(const RptrRenderRayQuery *queries, int num_queries, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera,
                                RptrSurfaceHit *results) {
        if (num_queries < 0) return false;
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_trace_surface(h_, queries, num_queries, &cam, variant_idx, results));
        return true;
    }
    // Occlusion queries (include/rptr_hip.h rptr_hip_trace_occlusion): one BIT per query, bit q & 31 of word q >> 5, 1 = something lies on the
    // ray inside (t_min, t_max). alpha_cutoff <= 0: every triangle is opaque; in (0, 1]: the cutout rule. Skipped queries and the bits behind
    // num_queries keep what the words held. Over the query buffer of enable_ray_queries into a DEVICE buffer of ceil(num_queries / 32) words
    // of the caller's, asynchronously on `hip_stream` (nullptr: the backend's) ...
    bool render_occlusion_queries(int num_queries, uint32_t *device_bits, float alpha_cutoff = 0.0f, void *hip_stream = nullptr) {
        if (!ray_query_buffer_) return false;
        const RptrOcclusionParams p = occlusion_params(alpha_cutoff);
        check(rptr_hip_trace_occlusion_device(h_, nullptr, num_queries, &p, device_bits, hip_stream));
        return true;
    }
    // ... and over HOST arrays, synchronously (bits is read as well as written)
    bool render_occlusion_queries(const RptrRenderRayQuery *queries, int num_queries, uint32_t *bits, float alpha_cutoff = 0.0f) {
        if (num_queries < 0) return false;
        const RptrOcclusionParams p = occlusion_params(alpha_cutoff);
        check(rptr_hip_trace_occlusion(h_, queries, num_queries, &p, bits));
        return true;
    }
    // Irradiance probes (include/rptr_hip.h rptr_hip_trace_probes): 3 floats of position per probe in, 36 floats out -- coeffs[p][i][ch], the
    // L2 SH coefficients of the radiance arriving at the probe, channels r, g, b and alpha (visibility of geometry). params: nullptr = the
    // defaults of rptr_hip_probe_defaults; a per-frame loop sets rotation, sample_index and blend. `camera` supplies the image-plane axes of
    // the texture footprint, render_params become the handle's. Over DEVICE buffers of the caller's, asynchronously on `hip_stream`
    // (nullptr: the backend's) ...
    bool trace_probes(const float *device_positions3, uint32_t num_probes, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera,
                      const RptrProbeParams *params, float *device_coeffs36, void *hip_stream) {
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_trace_probes_device(h_, device_positions3, num_probes, &cam, variant_idx, params, device_coeffs36, hip_stream));
        return true;
    }
    // ... and over HOST arrays, synchronously (coeffs36 is read as well as written: skipped probes keep theirs, blend < 1 blends into them)
    bool trace_probes(const float *positions3, uint32_t num_probes, const RptrRenderParams &render_params, int variant_idx, const RenderCameraParams &camera,
                      const RptrProbeParams *params, float *coeffs36) {
        check(rptr_hip_set_params(h_, &render_params, nullptr, nullptr));
        const RptrCamera cam = to_abi(camera);
        check(rptr_hip_trace_probes(h_, positions3, num_probes, &cam, variant_idx, params, coeffs36, nullptr));
        return true;
    }
    // convenience over HOST arrays (tests, tools): rptr_hip_trace uploads, traces, reads back
    bool render_ray_queries(const RptrRenderRayQuery *queries, int num_queries, float *results4) {
        if (num_queries < 0) return false;
        // (rptr_hip_trace sizes its own staging: the budget of enable_ray_queries only bounds the device buffers)
        check(rptr_hip_trace(h_, queries, num_queries, results4));
        return true;
    }
    // RenderBackendOptions::light_sampling_variant (rendering/mc/light_sampling.h:11-20): 0 NONE, 1 RIS; light_sampling_bucket_count is
    // LightSamplingConfig::bin_size, at most RPTR_BINNED_LIGHTS_BIN_MAX_SIZE (set_params refuses more)
    void set_light_sampling_variant(int variant) { check(rptr_hip_set_light_sampling_variant(h_, variant)); }
    rptr_hip_t *handle() { return h_; }

private:
    static RptrOcclusionParams occlusion_params(float alpha_cutoff) {
        RptrOcclusionParams p;
        rptr_hip_occlusion_defaults(&p);
        if (alpha_cutoff > 0.0f) {
            p.flags = RPTR_OCCLUSION_ALPHA_CUTOUT;
            p.alpha_cutoff = alpha_cutoff;
        }
        return p;
    }
    static RptrCamera to_abi(const RenderCameraParams &c) {
        RptrCamera cam{};
        for (int k = 0; k < 3; ++k) {
            cam.pos[k] = c.pos[k];
            cam.dir[k] = c.dir[k];
            cam.up[k] = c.up[k];
        }
        cam.fovy = c.fovy;
        return cam;
    }
    void check(int rc) const {
        if (rc != RPTR_OK) throw std::runtime_error(std::string("rptr_hip: ") + rptr_hip_last_error(h_));
    }
    void wait_slot(int i) {
        if (!pending_[i]) return;
        pending_[i] = false;
        // (a library call that needs the device to itself -- set_scene, ray queries over host arrays, a vertex update of a scene without
        // per-context copies -- has finished every frame in flight already: such a ticket is "not in flight" any more, its timings are gone)
        const int rc = rptr_hip_wait(h_, ticket_[i], &last_);
        if (rc == RPTR_OK) {
            ++stats_serial_;
            frame_collected(slot_reset_[i], slot_dt_[i]);
        }
        if (rc != RPTR_OK && !(rc == RPTR_E_INVALID && std::string(rptr_hip_last_error(h_)).find("not in flight") != std::string::npos)) check(rc);
    }
    // upscale_every_frame, denoise_temporal_every_frame, auto_exposure_every_frame: the calls that belong to the frame just collected
    void frame_collected(bool restarted, float dt) {
        if (denoise_temporal_every_frame_) {
            RptrDenoiseTemporalParams p = denoise_temporal_params_;
            p.reset_history = restarted ? 1 : 0;
            check(rptr_hip_denoise_temporal(h_, &p));
        }
        if (auto_exposure_every_frame_) {
            RptrAutoExposureParams p = auto_exposure_params_;
            p.reset_history = restarted ? 1 : 0;
            p.dt = dt;
            check(rptr_hip_auto_exposure(h_, &p));
            if (p.mode == 1) ++exposure_calls_;
        }
        if (!upscale_every_frame_) return;
        RptrTaaUpscaleParams p = taa_upscale_defaults();
        p.reset_history = restarted ? 1 : 0;
        check(rptr_hip_taa_upscale(h_, &p));
    }
    RptrRenderParams effective_params(RptrRenderParams p) const { // what the library is handed: `options` applied to a copy
        if (!options.enable_raytraced_dof) p.aperture_radius = p.focal_length = 0.f;
        return p;
    }
    int batch_spp(int spp) const { return spp > 0 ? spp : (params.batch_spp > 0 ? params.batch_spp : 1); }
    void push_state() { // RenderBackend::begin_frame "update params" (render_backend.cpp:17-23): the public members as they are NOW
        const RptrRenderParams pushed = effective_params(params);
        check(rptr_hip_set_params(h_, &pushed, have_scene_params_ ? &scene_params_ : nullptr, &lighting_params));
        check(rptr_hip_set_freeze_frame(h_, freeze_frame ? 1 : 0));
    }
    RptrCamera abi_camera() const {
        RptrCamera cam;
        for (int k = 0; k < 3; ++k) {
            cam.pos[k] = camera.pos[k];
            cam.dir[k] = camera.dir[k];
            cam.up[k] = camera.up[k];
        }
        cam.fovy = camera.fovy;
        return cam;
    }
    void count_frame(int spp) { // begin_frame / end_frame bookkeeping (render_vulkan.cpp:1937-1941,2152-2154), as the library keeps it
        if (reset_accumulation) frame_id_ = 0;
        accumulated_spp_ = int(frame_id_) + spp;
        if (!freeze_frame) frame_id_ += (uint32_t)spp;
        reset_accumulation = false;
    }
    rptr_hip_t *h_ = nullptr;
    int contexts_ = 1, active_swap_ = 1, swap_index_ = 0;
    uint64_t ticket_[MAX_SWAP_BUFFERS] = {0, 0};
    bool pending_[MAX_SWAP_BUFFERS] = {false, false};
    bool slot_reset_[MAX_SWAP_BUFFERS] = {false, false}; // reset_accumulation of the frame submitted on each swap index
    bool upscale_every_frame_ = false;
    bool denoise_temporal_every_frame_ = false;
    RptrDenoiseTemporalParams denoise_temporal_params_{};
    bool auto_exposure_every_frame_ = false;
    RptrAutoExposureParams auto_exposure_params_{};
    uint64_t exposure_calls_ = 0; // metering calls issued through this object (exposure_state_ready)
    float slot_dt_[MAX_SWAP_BUFFERS] = {0.f, 0.f}; // the time step of the frame submitted on each swap index ...
    float frame_dt_ = 0.f;                          // ... and of the frame begin_frame saw last: its RenderConfiguration::time minus the previous one's
    double last_time_ = 0.0;
    bool have_time_ = false;
    bool asynchronous_ = false;
    uint32_t frame_id_ = 0;
    uint64_t stats_serial_ = 0;
    int accumulated_spp_ = 0;
    RptrSceneParams scene_params_{};
    bool have_scene_params_ = false;
    int variant_ = RPTR_VARIANT_GLTF;
    void *ray_query_buffer_ = nullptr, *ray_result_buffer_ = nullptr;
    RptrStats last_{};
};

// ≙ struct RaytraceBackend (librender/raytrace_backend.h:13-19; libdatacapture's trace_ray over host arrays): closest-hit queries through
// rptr_hip_trace. The adapter on the reference's side converts rt_datacapture::RayQuery {origin, dir, t_max} to RptrRenderRayQuery
// (mode_or_data = 0) and RaytraceResults from the float4 rows (barycentrics, instance + geometry index, primitive index).
class RaytraceHip {
public:
    explicit RaytraceHip(int device_ordinal = 0) : backend_(device_ordinal, 0, 1, 32, nullptr, 1) { backend_.initialize(8, 8); } // (queries need no frame, the stack scratch does)
    std::string name() const { return std::string(rptr_hip_name()) + " (ray queries)"; }
    void set_scene(const RptrSceneDesc &scene) { backend_.set_scene(scene); }
    // returns the number of queries traced; results4: 4 floats per query in rt_intersect.comp's layout, miss = (-1, -1, bits(-1), bits(-1))
    int trace_ray(const RptrRenderRayQuery *queries, int num_queries, float *results4) {
        return backend_.render_ray_queries(queries, num_queries, results4) ? num_queries : 0;
    }
    RenderHip &backend() { return backend_; }

private:
    RenderHip backend_;
};

} // namespace rptr
