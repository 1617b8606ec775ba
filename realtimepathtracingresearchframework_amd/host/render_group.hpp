// render_group.hpp -- one host process driving several GPUs: N `RenderHip` backends (one per device, rank i of N) that share a frame
// by screen stripes, plus the library's gather of tile radiance to rank 0 (include/rptr_hip.h "multi-GPU": rptr_hip_comm_init_all /
// rptr_hip_gather_all -- grouped ncclSend / ncclRecv over xGMI, or peer copies when handles share a device).
// Shaped like one RenderBackend: the application calls set_scene / render / readback once, the group fans out. No reference
// counterpart (the reference renders on one physical device, vulkan/render_vulkan_extensions.cpp:77-82); partitioning per SURVEY 8e.
#pragma once
#include "render_hip.hpp"

#include <memory>
#include <vector>

namespace rptr {

class RenderGroup {
public:
    // devices: HIP ordinals, one rank each (the same ordinal may appear several times: a test rig on one GPU)
    RenderGroup(const std::vector<int> &devices, int stripe_rows = 8, int frames_in_flight = RenderHip::MAX_SWAP_BUFFERS, uint32_t create_flags = 0u) {
        const int n = (int)devices.size();
        if (n < 1) throw std::runtime_error("RenderGroup: no devices");
        for (int i = 0; i < n; ++i) ranks_.emplace_back(new RenderHip(devices[(size_t)i], i, n, stripe_rows, nullptr, frames_in_flight, create_flags));
    }
    int size() const { return (int)ranks_.size(); }
    RenderHip &rank(int i) { return *ranks_[(size_t)i]; }
    std::string name() const { return ranks_[0]->name() + " x" + std::to_string(size()); }

    void initialize(int fb_width, int fb_height) {
        width_ = fb_width;
        height_ = fb_height;
        for (auto &r : ranks_) r->initialize(fb_width, fb_height);
        if (size() > 1) { // (a communicator's buffers are frame-sized: it is made again after every initialize)
            std::vector<rptr_hip_t *> hs;
            for (auto &r : ranks_) hs.push_back(r->handle());
            if (rptr_hip_comm_init_all(hs.data(), size()) != RPTR_OK) throw std::runtime_error(std::string("rptr_hip_comm_init_all: ") + last_error());
        }
    }
    void set_scene(const RptrSceneDesc &scene) { // every GPU holds a replica of the scene
        for (auto &r : ranks_) r->set_scene(scene);
    }
    void update_config(const RptrSceneParams &sp) {
        for (auto &r : ranks_) r->update_config(sp);
    }
    void set_params(const RptrRenderParams &p, const RptrLightSamplingConfig &l) {
        for (auto &r : ranks_) {
            r->params = p;
            r->lighting_params = l;
        }
    }
    void update_vertices(uint32_t geometry, const float *xyz, uint32_t num_vertices) {
        for (auto &r : ranks_) r->update_vertices(geometry, xyz, num_vertices);
    }
    void refit() {
        for (auto &r : ranks_) r->refit();
    }
    void update_instances(uint32_t first, uint32_t count, const float *transforms12) { // every GPU holds the whole scene
        for (auto &r : ranks_) r->update_instances(first, count, transforms12);
    }
    // (device memory belongs to one GPU: rank k reads device_transforms12[k])
    void update_instances_device(uint32_t first, uint32_t count, const std::vector<const float *> &device_transforms12) {
        for (size_t k = 0; k < ranks_.size(); ++k) ranks_[k]->update_instances_device(first, count, device_transforms12.at(k));
    }
    void set_tlas_policy(int mode) {
        for (auto &r : ranks_) r->set_tlas_policy(mode);
    }
    uint64_t tlas_rebuild_count() const { // over every GPU
        uint64_t n = 0;
        for (auto &r : ranks_) n += r->tlas_rebuild_count();
        return n;
    }
    void set_light_sources(const std::vector<RptrLightSource> &sources) { // every GPU holds the whole scene: every rank is registered
        for (auto &r : ranks_) r->set_light_sources(sources);
    }
    std::vector<RptrTriLightData> readback_lights(uint32_t num_lights) { return ranks_[0]->readback_lights(num_lights); } // (the ranks' buffers are equal)
    void set_skin(uint32_t geometry, const std::vector<RptrSkinVertex> &vertices) { // every GPU holds the whole scene: every rank is bound
        for (auto &r : ranks_) r->set_skin(geometry, vertices);
    }
    void update_bones(uint32_t first, uint32_t count, const float *transforms12) {
        for (auto &r : ranks_) r->update_bones(first, count, transforms12);
    }
    // (device memory belongs to one GPU: rank k reads device_transforms12[k])
    void update_bones_device(uint32_t first, uint32_t count, const std::vector<const float *> &device_transforms12) {
        for (size_t k = 0; k < ranks_.size(); ++k) ranks_[k]->update_bones_device(first, count, device_transforms12.at(k));
    }
    void skin() {
        for (auto &r : ranks_) r->skin();
    }
    void set_morph_targets(uint32_t geometry, const std::vector<std::vector<RptrMorphDelta>> &targets) { // every rank is bound
        for (auto &r : ranks_) r->set_morph_targets(geometry, targets);
    }
    void update_morph_weights(uint32_t geometry, uint32_t first_target, uint32_t count, const float *weights) {
        for (auto &r : ranks_) r->update_morph_weights(geometry, first_target, count, weights);
    }
    // (device memory belongs to one GPU: rank k reads device_weights[k])
    void update_morph_weights_device(uint32_t geometry, uint32_t first_target, uint32_t count, const std::vector<const float *> &device_weights) {
        for (size_t k = 0; k < ranks_.size(); ++k) ranks_[k]->update_morph_weights_device(geometry, first_target, count, device_weights.at(k));
    }
    void set_normal_groups(uint32_t geometry, const std::vector<uint32_t> &groups, bool flip = false) { // every rank is bound
        for (auto &r : ranks_) r->set_normal_groups(geometry, groups, flip);
    }
    void recompute_normals() {
        for (auto &r : ranks_) r->recompute_normals();
    }
    // dynamic textures: every GPU holds the whole scene, so every rank is updated (false: refused as emissive, on every rank alike)
    bool update_texture(uint32_t texture, const uint8_t *rgba8, size_t n_bytes, bool generate_mips = true) {
        bool done = true;
        for (auto &r : ranks_) done = r->update_texture(texture, rgba8, n_bytes, generate_mips) && done;
        return done;
    }
    uint32_t texture_levels(uint32_t texture) const { return ranks_[0]->texture_levels(texture); } // (the ranks' textures are equal)
    std::vector<uint8_t> readback_texture(uint32_t texture, uint32_t level, uint32_t width, uint32_t height) {
        return ranks_[0]->readback_texture(texture, level, width, height);
    }
    std::vector<float> readback_skinned(uint32_t geometry, uint32_t num_vertices, std::vector<uint32_t> *normal_words = nullptr) { // (the ranks' buffers are equal)
        return ranks_[0]->readback_skinned(geometry, num_vertices, normal_words);
    }
    void set_rng_variant(int rng_variant, const std::vector<uint32_t> &table = {}) {
        for (auto &r : ranks_) r->set_rng_variant(rng_variant, table);
    }
    void set_bvh_policy(bool force_bvh_rebuild, int rebuild_triangle_budget) {
        for (auto &r : ranks_) r->set_bvh_policy(force_bvh_rebuild, rebuild_triangle_budget);
    }
    void set_option(const char *key, int64_t value) { // before initialize / set_scene (include/rptr_hip.h "Options")
        for (auto &r : ranks_) r->set_option(key, value);
    }
    int64_t get_option(const char *key) const { // the smallest value over the ranks (limits: "sample_slots")
        int64_t v = ranks_[0]->get_option(key);
        for (auto &r : ranks_) v = std::min(v, r->get_option(key));
        return v;
    }
    // The reference's frame loop (app.cpp:453-469) on ONE device: begin_frame / draw_frame / end_frame with the application's CommandStream*
    // (render_hip.hpp: non-null = submitted, two frames in flight, statistics two frames late). A group of several devices renders such a
    // frame synchronously (its gather follows the frame).
    RenderStats frame(CommandStream *cmd_stream, const RenderConfiguration &config) {
        if (size() > 1 || !cmd_stream) {
            const RenderStats s = render(config);
            if (denoise_temporal_every_frame_) denoise_temporal(config.reset_accumulation);
            if (auto_exposure_every_frame_) { // (render() collects through tickets: the call is this loop's to issue, as the two around it)
                RptrAutoExposureParams p = auto_exposure_params_;
                p.reset_history = config.reset_accumulation ? 1 : 0;
                p.dt = have_time_ && config.time > last_time_ ? float(config.time - last_time_) : 0.0f;
                auto_exposure(p);
            }
            last_time_ = config.time;
            have_time_ = true;
            if (upscale_every_frame_) taa_upscale(config.reset_accumulation);
            return s;
        }
        RenderHip &r = *ranks_[0];
        r.begin_frame(cmd_stream, config);
        r.draw_frame(cmd_stream, config.active_variant);
        r.end_frame(cmd_stream, config.active_variant);
        const RenderStats s = r.stats();
        if (s.has_valid_frame_stats && r.stats_serial() != counted_serial_) { // (the timings of the frame two submissions ago: counted once)
            rays_ += double(r.rays_of_last_stats());
            counted_serial_ = r.stats_serial();
        }
        return s;
    }
    void flush_pipeline() {
        for (auto &r : ranks_) r->flush_pipeline();
    }
    // one frame on all GPUs: every rank renders its stripes (asynchronously, side by side), then the tiles are gathered to rank 0
    RenderStats render(const RenderConfiguration &config, int spp = 0) {
        std::vector<uint64_t> tickets;
        for (auto &r : ranks_) tickets.push_back(r->render_async(config, spp));
        RenderStats total{};
        for (size_t i = 0; i < ranks_.size(); ++i) {
            const RenderStats s = ranks_[i]->wait(tickets[i]);
            total.render_time = std::max(total.render_time, s.render_time);
            rays_ += s.has_valid_frame_stats ? double(s.rays_per_second) * s.render_time * 1e-3 : 0.0;
            total.spp = s.spp;
            total.total_device_bytes_allocated += s.total_device_bytes_allocated;
        }
        if (size() > 1) {
            std::vector<rptr_hip_t *> hs;
            for (auto &r : ranks_) hs.push_back(r->handle());
            if (rptr_hip_gather_all(hs.data(), size()) != RPTR_OK) throw std::runtime_error(std::string("rptr_hip_gather_all: ") + last_error());
        }
        return total;
    }
    // The pipelined schedule (what bench.py measures): a launch sequence of `n_frames` frames is queued on every GPU and collected later,
    // while others are in flight (the group's frames_in_flight contexts). collect() waits for the sequence's frames in order, gathers them
    // to rank 0 in ONE collective (rptr_hip_gather_all_batch: the frames of a sequence finish together and lie behind each other in every
    // rank's images; per_frame_gather = true: one collective per frame, as rounds 2-3 did) and returns one RenderStats per frame
    // (render_time: the slowest rank's share of the sequence). readback_framebuffer(.., frame) then reads frame k of that sequence.
    struct Sequence {
        std::vector<std::vector<uint64_t>> tickets; // [rank][frame]
        int frames = 0;
    };
    Sequence submit(const RenderConfiguration &config, int spp, int n_frames, bool reset_rest = true) {
        Sequence q;
        q.frames = n_frames;
        for (auto &r : ranks_) q.tickets.push_back(n_frames > 1 ? r->render_batch_async(config, spp, n_frames, reset_rest) : std::vector<uint64_t>{r->render_async(config, spp)});
        return q;
    }
    // ... with a camera per frame: configs[k] is frame k's (rptr_hip_render_batch_cameras_async; the application's loop may move the camera
    // every frame, app.cpp:350-469)
    Sequence submit(const std::vector<RenderConfiguration> &configs, int spp, bool reset_rest = true) {
        Sequence q;
        q.frames = (int)configs.size();
        for (auto &r : ranks_)
            q.tickets.push_back(q.frames > 1 ? r->render_batch_cameras_async(configs.data(), q.frames, spp, reset_rest) : std::vector<uint64_t>{r->render_async(configs[0], spp)});
        return q;
    }
    // one frame of a sequence at a time (hosts that act between the frames: an image per keyframe): the tickets of frame k on every rank,
    // the gather when it is the sequence's last (all its frames in one collective)
    RenderStats collect_frame(const Sequence &q, int k) {
        RenderStats total{};
        total.has_valid_frame_stats = false;
        for (size_t i = 0; i < ranks_.size(); ++i) {
            const RenderStats s = ranks_[i]->wait(q.tickets[i][(size_t)k]);
            total.render_time = std::max(total.render_time, s.render_time);
            total.has_valid_frame_stats = total.has_valid_frame_stats || s.has_valid_frame_stats;
            rays_ += s.has_valid_frame_stats ? double(s.rays_per_second) * s.render_time * 1e-3 : 0.0;
            total.spp = s.spp;
            total.total_device_bytes_allocated += s.total_device_bytes_allocated;
        }
        if (size() > 1 && k == q.frames - 1) {
            std::vector<rptr_hip_t *> hs;
            for (auto &r : ranks_) hs.push_back(r->handle());
            if (rptr_hip_gather_all_batch(hs.data(), size(), q.frames) != RPTR_OK) throw std::runtime_error(std::string("rptr_hip_gather_all_batch: ") + last_error());
        }
        return total;
    }
    std::vector<RenderStats> collect(const Sequence &q, bool per_frame_gather = false) {
        std::vector<RenderStats> out;
        for (int k = 0; k < q.frames; ++k) {
            RenderStats total{};
            for (size_t i = 0; i < ranks_.size(); ++i) {
                const RenderStats s = ranks_[i]->wait(q.tickets[i][(size_t)k]);
                total.render_time = std::max(total.render_time, s.render_time);
                total.has_valid_frame_stats = total.has_valid_frame_stats || s.has_valid_frame_stats;
                rays_ += s.has_valid_frame_stats ? double(s.rays_per_second) * s.render_time * 1e-3 : 0.0;
                total.spp = s.spp;
                total.total_device_bytes_allocated += s.total_device_bytes_allocated;
            }
            if (size() > 1 && (per_frame_gather || k == q.frames - 1)) {
                std::vector<rptr_hip_t *> hs;
                for (auto &r : ranks_) hs.push_back(r->handle());
                if (rptr_hip_gather_all_batch(hs.data(), size(), per_frame_gather ? 1 : q.frames) != RPTR_OK)
                    throw std::runtime_error(std::string("rptr_hip_gather_all_batch: ") + last_error());
            }
            out.push_back(total);
        }
        return out;
    }
    // frame k (0 = the oldest) of the sequence collected last, assembled on rank 0
    size_t readback_framebuffer(size_t buffer_size, float *buffer, int frame) {
        if (size() == 1) return 0; // (one rank: the frames of a sequence are read through the rank's own tickets)
        const size_t need = (size_t)width_ * height_ * 4;
        if (buffer_size < need) return 0;
        if (rptr_hip_readback_gathered_frame_f32(ranks_[0]->handle(), frame, buffer, buffer_size) != RPTR_OK) throw std::runtime_error(std::string("readback: ") + last_error());
        return need;
    }
    double rays_traced() const { return rays_; }
    // the full frame (RGBA32F accumulation buffer) on the host: rank 0's assembled frame
    size_t readback_framebuffer(size_t buffer_size, float *buffer) {
        if (size() == 1) return ranks_[0]->readback_framebuffer(buffer_size, buffer);
        const size_t need = (size_t)width_ * height_ * 4;
        if (buffer_size < need) return 0;
        if (rptr_hip_readback_gathered_f32(ranks_[0]->handle(), buffer, buffer_size) != RPTR_OK) throw std::runtime_error(std::string("readback: ") + last_error());
        return need;
    }
    // 8-bit frame buffer / AOV images: every rank fills in its own rows (the read-backs leave the other rows untouched)
    size_t readback_framebuffer(size_t buffer_size, unsigned char *buffer) {
        size_t n = 0;
        for (auto &r : ranks_) n = r->readback_framebuffer(buffer_size, buffer);
        return n;
    }
    // the denoiser works on one GPU's whole frame (rptr_hip_denoise refuses world_size > 1: a stripe's taps lie in other ranks' rows)
    void denoise(const RptrDenoiseParams &p) { ranks_[0]->denoise(p); }
    size_t readback_denoised(size_t buffer_size, float *buffer) { return ranks_[0]->readback_denoised(buffer_size, buffer); }
    size_t readback_denoised(size_t buffer_size, unsigned char *buffer) { return ranks_[0]->readback_denoised(buffer_size, buffer); }
    // ... and so does the temporal denoiser (rptr_hip_denoise_temporal refuses world_size > 1); its result is read with readback_denoised
    void denoise_temporal(const RptrDenoiseTemporalParams &p) { ranks_[0]->denoise_temporal(p); }
    void denoise_temporal(bool reset_history) {
        RptrDenoiseTemporalParams p = denoise_temporal_params_;
        p.reset_history = reset_history ? 1 : 0;
        denoise_temporal(p);
    }
    // with every frame of frame(), as upscale_every_frame below; for one device only
    void denoise_temporal_every_frame(bool on, const RptrDenoiseTemporalParams &p = RenderHip::denoise_temporal_defaults()) {
        if (on && size() > 1) throw std::runtime_error("denoise_temporal_every_frame needs one device (rptr_hip_denoise_temporal refuses world_size > 1)");
        denoise_temporal_every_frame_ = on;
        denoise_temporal_params_ = p;
        ranks_[0]->denoise_temporal_every_frame(on, p);
    }
    size_t readback_denoise_history(size_t buffer_size, float *buffer) { return ranks_[0]->readback_denoise_history(buffer_size, buffer); }
    // auto-exposure meters one GPU's whole frame as well (rptr_hip_auto_exposure refuses world_size > 1)
    void auto_exposure(const RptrAutoExposureParams &p) { ranks_[0]->auto_exposure(p); }
    // with every frame of frame(), as upscale_every_frame below (RenderHip issues it in both of its loops); for one device only
    void auto_exposure_every_frame(bool on, const RptrAutoExposureParams &p = RenderHip::auto_exposure_defaults()) {
        if (on && size() > 1) throw std::runtime_error("auto_exposure_every_frame needs one device (rptr_hip_auto_exposure refuses world_size > 1)");
        auto_exposure_every_frame_ = on;
        auto_exposure_params_ = p;
        ranks_[0]->auto_exposure_every_frame(on, p);
    }
    size_t readback_exposed(size_t buffer_size, unsigned char *buffer) { return ranks_[0]->readback_exposed(buffer_size, buffer); }
    RptrExposureState readback_exposure_state(bool newest = true) { return ranks_[0]->readback_exposure_state(newest); }
    bool exposure_state_ready() const { return ranks_[0]->exposure_state_ready(); }
    // bloom works on one GPU's whole frame as well (rptr_hip_bloom refuses world_size > 1)
    void bloom(const RptrBloomParams &p) { ranks_[0]->bloom(p); }
    size_t readback_bloomed(size_t buffer_size, unsigned char *buffer) { return ranks_[0]->readback_bloomed(buffer_size, buffer); }
    // temporal 2x upscaling works on one GPU's whole frame as well (rptr_hip_taa_upscale refuses world_size > 1)
    void taa_upscale(const RptrTaaUpscaleParams &p) { ranks_[0]->taa_upscale(p); }
    void taa_upscale(bool reset_history) {
        RptrTaaUpscaleParams p = RenderHip::taa_upscale_defaults();
        p.reset_history = reset_history ? 1 : 0;
        taa_upscale(p);
    }
    // with every frame of frame(): the command-stream loop upscales as it collects (render_hip.hpp), a synchronous frame right after it
    void upscale_every_frame(bool on) {
        upscale_every_frame_ = on;
        ranks_[0]->upscale_every_frame(on);
    }
    size_t readback_upscaled(size_t buffer_size, unsigned char *buffer) { return ranks_[0]->readback_upscaled(buffer_size, buffer); }
    // object motion works on one GPU's whole frame as well (rptr_hip_object_motion refuses world_size > 1)
    void track_object_motion(bool enable = true) { ranks_[0]->track_object_motion(enable); }
    int64_t object_motion() { return ranks_[0]->object_motion(); }
    size_t readback_aov(RenderHip::AOVBufferIndex aov, size_t buffer_size, uint16_t *buffer) {
        size_t n = 0;
        for (auto &r : ranks_) n = r->readback_aov(aov, buffer_size, buffer);
        return n;
    }
    float mean_gather_ms() {
        uint64_t n = 0;
        float ms = 0.f;
        if (size() > 1) (void)rptr_hip_comm_stats(ranks_[0]->handle(), &n, &ms);
        return ms;
    }

private:
    std::string last_error() {
        for (auto &r : ranks_) {
            const char *e = rptr_hip_last_error(r->handle());
            if (e && *e) return e;
        }
        return rptr_hip_last_error(nullptr);
    }
    std::vector<std::unique_ptr<RenderHip>> ranks_;
    int width_ = 0, height_ = 0;
    double rays_ = 0.0;
    uint64_t counted_serial_ = 0;
    bool upscale_every_frame_ = false;
    bool denoise_temporal_every_frame_ = false;
    RptrDenoiseTemporalParams denoise_temporal_params_ = RenderHip::denoise_temporal_defaults();
    bool auto_exposure_every_frame_ = false;
    RptrAutoExposureParams auto_exposure_params_ = RenderHip::auto_exposure_defaults();
    double last_time_ = 0.0; // RenderConfiguration::time of the previous synchronous frame(): the next one's time step
    bool have_time_ = false;
};

} // namespace rptr
