// rptr_cli.cpp -- the reference's headless run modes through the C ABI (binary: bin/rptr_hip):
//
//   <scene> = the reference's .vks file (textures in <name>_textures/) or the flat dump scenes.py writes (.rpsc)
//   rptr_hip <scene> --validation <prefix> [--validation-spp n] [--img w h] [--pfm] [--denoise iterations | --denoise-temporal iterations | --taa-upscale] [--auto-exposure] [--bloom intensity]
//   rptr_hip <scene.rpsc> --profiling <csv prefix> [--profiling-fps f] [--profiling-img <prefix>] [--profiling-frames n]
//            [--animate-wave amplitude kx] [--recompute-normals] [--synchronous] [--fly-through] [--frames-in-flight n [--frames-per-launch b]]
//   common:  [--eye x y z] [--center x y z] [--up x y z] [--fov deg] [--variant gltf|diffuse|gltf-transmission] [--batch-spp k] [--every-frame] [--generate-mips]
//            [--config file.ini]... [--keyframe [<seconds>:]file.ini]... [--camera n] [--freeze-frame] [--upscale n] [--backend hip]
//            [--sky-data <dir with the Hosek-Wilkie data headers>]   (Sun settings of the .ini files refit the sky: host/sky_fit.hpp; also RPTR_SKY_DATA)
//            [--rng-variant uniform|bn|sobol|z-sobol] [--bn-table bn_tables.h|BNData.u32] [--force-bvh-rebuild] [--rebuild-triangle-budget n]
//            [--devices n | --devices a,b,c] [--stripe-rows r]
//
// --config / --keyframe read the reference's .ini files (ini_config.hpp); in profiling mode every keyframe is held for its length
// (default 1 s of animation time = --profiling-fps frames) and the accumulation restarts when the keyframe changes.
// --devices: one process, several GPUs (render_group.hpp): the frame is cut into stripes of --stripe-rows rows, stripe s -> device
// s % n, tile radiance gathered to the first device with the library's RCCL gather (peer copies when a device is listed twice).
//
// Flag names, file names and the CSV header are the reference's (cmdline.cpp:10-104,296-474; libapp/app_state.cpp:218-255,
// 291-322,464-498; libapp/benchmark_info.cpp:69-124; util/write_image.cpp:34-64):
//  * validation mode renders at time 0, one frame = params.batch_spp samples, accumulates until --validation-spp and writes
//    the float accumulation buffer as <prefix>_%04d.pfm (accumulated spp in the name); n < 1 = after every frame;
//  * profiling mode advances time by 1/fps per frame (non-realtime), appends one CSV row per frame to <prefix>.csv with the
//    header frames_total,keyframe,frames_accumulated,render_time_ms,app_time_ms, and writes <img prefix>_%04d.pfm once per
//    second of animation time. The run ends at its last keyframe (--keyframe [len:]file.ini ...); without keyframes the reference
//    stops after its first frame (imstate.cpp:890-898) and so does this host unless --profiling-count n (its own flag) asks for n
//    frames, a keyframe then being one second. --profiling-frames is the reference's old spelling of --profiling-fps.
//    The loop is the reference's (app.cpp:453-469): begin_frame / draw_frame / end_frame with a command stream -- two frames in flight,
//    render_time_ms of a row = the statistics the backend has at that point, i.e. of the frame two submissions earlier
//    (RenderStats::frame_stats_delay, vulkan/render_vulkan.cpp:2229-2243) -- unless --synchronous (the application's "force synchronous
//    rendering": cmd_stream = nullptr) is given. --frames-in-flight n [--frames-per-launch b] (this host's) queues deeper than the reference's
//    two swap buffers: launch sequences of b frames, each frame with its own camera, n sequences in flight -- bench.py's schedule;
//    keyframes and --fly-through (this host's: the camera path of bench.py, yaw 0.002 rad and 2 cm sideways per frame, 64 views around the scene's own, a
//    moved camera restarts the accumulation) work in every schedule.
//  * --animate-wave a k (profiling mode, scenes whose mesh 0 is dynamic): y = y0 + a sin(k x + 2 pi t) on geometry 0 before
//    every frame, followed by rptr_hip_refit -- SURVEY 8d C5 (the reference animates with a compute shader,
//    render_vulkan.cpp:2834-2840; per-frame BLAS update + TLAS refit :1323-1354).
//  * --skin <file> --bones <file> (profiling and data-capture mode, scenes whose mesh 0 is dynamic): the skin file holds raw
//    RptrSkinVertex records (16 bytes per unrolled vertex) for geometry first_geometry of mesh 0, the bones file two uint32 (frames,
//    bones) and frames x bones x 12 float32. Frame k of the run stages the bones of frame k mod frames, skins on the device
//    (rptr_hip_skin) and refits before it renders; positions AND shading normals follow. One flag without the other, --animate-wave
//    beside them, a mesh 0 that is not dynamic or a file of the wrong size: exit code 2 before a device is touched.
//  * --morph <file> --morph-weights <file> (the same modes, alone or together with --skin --bones): the morph file holds uint32 targets,
//    then per target uint32 deltas and that many 32-byte RptrMorphDelta records, for geometry first_geometry of mesh 0; the weights file
//    two uint32 (frames, targets) and frames x targets float32. Frame k stages the weights of frame k mod frames, then skins (the morph
//    stage runs in front of the skin) and refits. One flag without the other, a size mismatch, a target count that differs between the
//    two files or a static mesh 0: exit code 2 before a device is touched.
//  * --recompute-normals (with --animate-wave, --skin --bones or --morph --morph-weights): the written geometry -- first_geometry of mesh
//    0, which must have normals -- is welded at its rest pose (host/normal_groups.hpp: corners with bitwise equal positions and equal
//    normal words are one smooth vertex) and bound with rptr_hip_set_normal_groups; rptr_hip_recompute_normals runs before every refit,
//    so the shading normals follow the wave (or replace what the skinner wrote: morph targets without normal deltas). Without one of
//    those flags nothing writes vertices: exit code 2 before a device is touched.
//  * --generate-mips: after set_scene, every texture that came with level 0 only gets its full mip chain on the device
//    (rptr_hip_update_texture(t, NULL, 0, RPTR_TEXTURE_GENERATE_MIPS): include/rptr_hip.h "dynamic textures"). One line per such texture on
//    stdout: "generate-mips: texture t w x h -> n levels", or "generate-mips: texture t w x h skipped (emissive)" for a texture a material
//    with emission_intensity > 0 reads (the scene's lights were made from it: the library refuses).
//  * data-capture mode (--data-capture <prefix> [--data-capture-spp n] [--data-capture-no-rgba] [--data-capture-no-aovs]
//    [--data-capture-albedo-roughness|-normal-depth|-motion]) stores the accumulation buffer and the chosen AOV images of every
//    keyframe as <prefix>_%04d_{rgba,albedo_roughness,normal_depth,motion_jitter}.exr (libapp/app_state.cpp:499-531).
// Images: --exr (default, as in the reference), --pfm, --png (write_image.hpp).
// The scene comes from a dump file (scene_dump.hpp) instead of a .vks (python -m ...vks converts).
#include "ini_config.hpp"
#include "normal_groups.hpp"
#include "render_group.hpp"
#include "scene_dump.hpp"
#include "sky_fit.hpp"
#include "vks_reader.hpp"
#include "write_image.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <dlfcn.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

enum OutputFormat { FORMAT_EXR, FORMAT_PFM, FORMAT_PNG }; // cmdline.cpp:450-460: EXR is the default

// BasicApplicationState::save_framebuffer (libapp/app_state.cpp:341-438): the float accumulation buffer as EXR / PFM, the 8-bit
// frame buffer as PNG, under <prefix>_<number> (+ suffix)
// --denoise <iterations> (this host's; the reference's enable_denoising links Open Image Denoise): the images written are the denoised ones
// (include/rptr_hip.h rptr_hip_denoise with the library's defaults and that many passes); 0: the frame's own, as without the flag
static int g_denoise_iterations = 0;
// --taa-upscale (this host's): every frame goes through rptr_hip_taa_upscale as it is collected, and the RGBA8 images written (--png)
// are the upscaled ones, at twice --img; the history restarts with the frames that restart the accumulation (the first one, a new
// keyframe, moved geometry, a moved camera unless the history is reprojected). The float images stay the frame's own. Not with --denoise.
static bool g_taa_upscale = false;
// --object-motion (this host's): plays the animated transforms of a .vks file (numFrames > 1) -- frame k of the run gets the file's frame
// k mod numFrames through update_instances + refit -- and runs rptr_hip_object_motion after every frame, in front of --denoise-temporal /
// --taa-upscale (profiling mode, one frame at a time) or of the captured images (--data-capture: one capture per frame of the file).
// Refused with anything else: without a consumer or a capture nothing reads the rewritten motion image.
static bool g_object_motion = false;
// --denoise-temporal <iterations> (this host's): every frame goes through rptr_hip_denoise_temporal as it is collected (the library's
// defaults and that many passes; one frame per launch sequence), the history restarting with the frames that restart the accumulation,
// and the images written are the denoised ones. Not with --denoise, --taa-upscale or several devices.
static int g_denoise_temporal_iterations = 0;
static RptrDenoiseTemporalParams denoise_temporal_params() {
    RptrDenoiseTemporalParams p = rptr::RenderHip::denoise_temporal_defaults();
    p.iterations = g_denoise_temporal_iterations;
    return p;
}
static void denoise_temporal(rptr::RenderGroup &backend, bool reset_history) {
    RptrDenoiseTemporalParams p = denoise_temporal_params();
    p.reset_history = reset_history ? 1 : 0;
    backend.denoise_temporal(p);
}
// --auto-exposure (this host's; .ini: Tonemapping "auto exposure" = 1, "exposure key", "white balance"): every frame -- in a validation run
// every image written -- goes through rptr_hip_auto_exposure as it is collected, after --denoise / --denoise-temporal (whose image it then
// meters: source 1), with the configuration's tone mapping operator, dt = the animation time step and the history restarted with the
// accumulation; the RGBA8 images written (--png) are the exposed ones, the float images stay what they were, and the frame log on stdout
// gets a line "auto-exposure: frame n ev e target t" per frame. Not with --taa-upscale (the upscaler reads the frame's own RGBA8) or
// several devices.
static bool g_auto_exposure = false;
static RptrAutoExposureParams g_auto_exposure_params;
static const char *auto_exposure_refusal(size_t n_devices) {
    if (!g_auto_exposure) return nullptr;
    if (g_taa_upscale) return "--auto-exposure and --taa-upscale cannot be combined: the upscaler reads the frame's own RGBA8 image, not the exposed one\n";
    if (n_devices > 1) return "--auto-exposure needs one device (rptr_hip_auto_exposure refuses world_size > 1)\n";
    return nullptr;
}
static void print_exposure(const RptrExposureState &st, int frame) {
    std::printf("auto-exposure: frame %d ev %.6f target %.6f\n", frame, st.ev, st.target_ev);
}
static void auto_exposure(rptr::RenderGroup &backend, bool reset_history, float dt, int frame) {
    RptrAutoExposureParams p = g_auto_exposure_params;
    p.reset_history = reset_history ? 1 : 0;
    p.dt = dt;
    backend.auto_exposure(p);
    print_exposure(backend.readback_exposure_state(), frame);
}
// --bloom <intensity> (this host's): every RGBA8 image written (--png) goes through rptr_hip_bloom with the library's defaults and that
// intensity, behind --denoise / --denoise-temporal (source 1) and --auto-exposure, whose metered scale it then reads on the device
// (exposure_mode 1) and whose white balance it shares; without --auto-exposure the configuration's exposure counts (exposure_mode 0). The
// tone mapping operator is the configuration's. Not with --taa-upscale or several devices.
static bool g_bloom = false;
static RptrBloomParams g_bloom_params;
static float g_bloom_intensity = 0.f;
static const char *bloom_refusal(size_t n_devices) {
    if (!g_bloom) return nullptr;
    if (g_taa_upscale) return "--bloom and --taa-upscale cannot be combined: bloom works on the frame at render resolution\n";
    if (n_devices > 1) return "--bloom needs one device (rptr_hip_bloom refuses world_size > 1)\n";
    return nullptr;
}
static void save_image(rptr::RenderGroup &backend, OutputFormat format, const std::string &prefix, int number, const std::string &suffix, int width, int height,
                       std::vector<float> &img, bool expose_now = false) {
    char name[32];
    std::snprintf(name, sizeof(name), "_%04d", number);
    const std::string base = prefix + name + suffix;
    bool ok = false;
    if (g_denoise_iterations > 0) {
        RptrDenoiseParams dp = rptr::RenderHip::denoise_defaults();
        dp.iterations = g_denoise_iterations;
        backend.denoise(dp);
    }
    const bool denoised = g_denoise_iterations > 0 || g_denoise_temporal_iterations > 0;
    // (expose_now: a validation run's still image, metered as it is written -- no adaptation; with --denoise the denoised image exists
    // only from here on, so the frame loops leave the call to this function as well)
    if (g_auto_exposure && (expose_now || g_denoise_iterations > 0)) auto_exposure(backend, true, 0.f, number);
    if (format == FORMAT_PNG && g_bloom) { // (behind the exposure call above, or the frame loop's: the state it reads is that frame's)
        std::vector<unsigned char> rgba8((size_t)width * height * 4);
        backend.bloom(g_bloom_params);
        if (backend.readback_bloomed(rgba8.size(), rgba8.data()) != rgba8.size()) throw std::runtime_error("read-back failed");
        ok = rptr::write_png(base, (unsigned)width, (unsigned)height, 4, rgba8.data());
    } else if (format == FORMAT_PNG && g_auto_exposure) {
        std::vector<unsigned char> rgba8((size_t)width * height * 4);
        if (backend.readback_exposed(rgba8.size(), rgba8.data()) != rgba8.size()) throw std::runtime_error("read-back failed");
        ok = rptr::write_png(base, (unsigned)width, (unsigned)height, 4, rgba8.data());
    } else if (format == FORMAT_PNG && g_taa_upscale) {
        std::vector<unsigned char> rgba8((size_t)width * height * 16);
        if (backend.readback_upscaled(rgba8.size(), rgba8.data()) != rgba8.size()) throw std::runtime_error("read-back failed");
        ok = rptr::write_png(base, 2u * (unsigned)width, 2u * (unsigned)height, 4, rgba8.data());
    } else if (format == FORMAT_PNG) {
        std::vector<unsigned char> rgba8((size_t)width * height * 4);
        if ((denoised ? backend.readback_denoised(rgba8.size(), rgba8.data()) : backend.readback_framebuffer(rgba8.size(), rgba8.data())) != rgba8.size())
            throw std::runtime_error("read-back failed");
        ok = rptr::write_png(base, (unsigned)width, (unsigned)height, 4, rgba8.data());
    } else {
        if ((denoised ? backend.readback_denoised(img.size(), img.data()) : backend.readback_framebuffer(img.size(), img.data())) != img.size())
            throw std::runtime_error("read-back failed");
        ok = format == FORMAT_PFM ? rptr::write_pfm(base, (unsigned)width, (unsigned)height, 4, img.data())
                                  : rptr::write_exr<float>(base, (unsigned)width, (unsigned)height, 4, img.data());
    }
    if (!ok) throw std::runtime_error("cannot write " + base);
}
// BasicApplicationState::save_aov_exr (libapp/app_state.cpp:441-462): an AOV image as a HALF EXR
static void save_aov(rptr::RenderGroup &backend, rptr::RenderHip::AOVBufferIndex aov, const std::string &base, int width, int height) {
    std::vector<uint16_t> half((size_t)width * height * 4);
    if (backend.readback_aov(aov, half.size(), half.data()) != half.size()) throw std::runtime_error("AOV read-back failed");
    if (!rptr::write_exr<uint16_t>(base, (unsigned)width, (unsigned)height, 4, half.data())) throw std::runtime_error("cannot write " + base + ".exr");
}

// package data (data/) sits next to librptr_hip.so: the directory of the library this program is linked against
static std::string data_dir() {
    if (const char *e = std::getenv("RPTR_DATA_DIR")) return e;
    Dl_info info;
    if (dladdr((const void *)&rptr_hip_name, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        const size_t k = p.rfind('/');
        return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/data";
    }
    return "data";
}

// a scene file: the reference's own .vks (with its _textures directory), or the flat dump of scenes.py
static rptr::vks::LoadParams g_load; // --remove-first-lods, --instance-pruning, --small-deformation, --ignore-animation, --ignore-textures, --load-specularity (SceneLoaderParams::PerFile)
static rptr::SceneDump load_one_scene(const std::string &path) {
    const size_t n = path.size();
    if (n >= 4 && path.compare(n - 4, 4, ".vks") == 0) return rptr::vks::read_scene(path, data_dir(), g_load);
    return rptr::SceneDump::load(path);
}
// `<scene_file> [<scene_file>...]` (Scene::Scene(fnames, ...), librender/scene.cpp:50-69): every further file is appended to the first --
// meshes, parameterized meshes, instances, materials, textures, indices shifted; camera and parameters are the first file's -- then
// `--deduplicate-scene` merges equal meshes / materials / textures and drops what nothing refers to (Scene::deduplicate + garbage_collect),
// and the emitters are collected and binned again over the whole scene (librender/lights.cpp through host/lights.hpp).
static std::vector<std::string> g_more_scenes;
static bool g_deduplicate = false, g_merge_partitions = false; // --deduplicate-scene, --merge-partition-instances (SceneLoaderParams)
static rptr::SceneDump load_scene(const std::string &path) {
    auto one = [&](const std::string &file) {
        rptr::SceneDump d = load_one_scene(file);
        if (g_merge_partitions) {
            const size_t n = d.merge_partition_instances();
            if (n) std::printf("%s: merged %zu partition instances\n", file.c_str(), n);
        }
        return d;
    };
    rptr::SceneDump s = one(path);
    for (const std::string &more : g_more_scenes) s.append(one(more));
    if (g_deduplicate) {
        const rptr::SceneDump::DedupStats st = s.deduplicate();
        if (st.meshes) std::printf("Duplicate geometry detected! Removed %zu meshes\n", st.meshes);
        if (st.materials) std::printf("Removed %zu unused materials\n", st.materials);
        if (st.textures) std::printf("Removed %zu unused textures\n", st.textures);
    }
    if (!g_more_scenes.empty() || g_deduplicate || g_merge_partitions) rptr::lights::prepare_lights(s);
    return s;
}

// the float positions of a geometry at rest, 3 per unrolled vertex (librender/dequantize.glsl:8-21): what set_scene puts into a dynamic
// mesh's vertex buffer
static std::vector<float> rest_positions(const RptrGeometryDesc &g) {
    std::vector<float> rest((size_t)g.num_tris * 9);
    for (size_t v = 0; v < (size_t)g.num_tris * 3; ++v) {
        const uint64_t w = g.qpos[v];
        rest[3 * v + 0] = float(uint32_t(w) & 0x1FFFFFu) * g.quantized_scaling[0] + g.quantized_offset[0];
        rest[3 * v + 1] = float(uint32_t(w >> 21) & 0x1FFFFFu) * g.quantized_scaling[1] + g.quantized_offset[1];
        rest[3 * v + 2] = float(uint32_t(w >> 42) & 0x1FFFFFu) * g.quantized_scaling[2] + g.quantized_offset[2];
    }
    return rest;
}

int main(int argc, char **argv) {
    std::string scene_path, validation_prefix, csv_prefix, profiling_img_prefix, capture_prefix;
    OutputFormat format = FORMAT_EXR;
    bool data_capture = false, capture_rgba = true, capture_albedo = true, capture_normal = true, capture_motion = true; // DataCaptureConfig, libapp/shell.h
    bool have_profiling_options = false, want_help = false;
    float capture_fps = 60.f;
    int capture_spp = 1;
    int target_spp = 1, width = 256, height = 256, variant = RPTR_VARIANT_GLTF, batch_spp = 1, profiling_frames = 1; // without keyframes the reference's profiling run ends after its first frame (imstate.cpp:890-898)
    float profiling_fps = 60.f, wave_amp = 0.f, wave_k = 0.f;
    float eye[3], center[3], up[3] = {0, 1, 0}, fov = 0.f;
    bool every_frame = false, describe = false, validation = false, profiling = false, got_eye = false, got_center = false, got_up = false;
    bool freeze_frame = false, got_batch_spp = false, got_variant = false;
    int rng_variant = -1, force_bvh_rebuild = -1, rebuild_triangle_budget = -1; // -1: as the configuration files say
    std::string bn_table_path, dump_scene_path, sky_data;
    std::string skin_path, bones_path; // --skin / --bones: a skinned mesh 0 (rptr_hip_set_skin / update_bones / skin)
    std::string morph_path, morph_weights_path; // --morph / --morph-weights: morph targets on mesh 0 (rptr_hip_set_morph_targets / update_morph_weights)
    bool generate_mips = false;     // --generate-mips: the full mip chain, made on the device, for every texture that has level 0 only
    bool recompute_normals = false; // --recompute-normals: rptr_hip_set_normal_groups on the written geometry, recompute_normals before every refit
    bool got_frames_per_launch = false;
    int upscale = 0, stripe_rows = 8, frames_in_flight = 0, frames_per_launch = 1; // frames_in_flight 0: the reference's loop (two swap buffers)
    bool synchronous = false, fly_through = false;
    std::vector<int> devices{0};
    std::vector<std::string> config_inis;
    struct Keyframe {
        std::string ini;
        double hold;
    };
    std::vector<Keyframe> keyframes;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](int k) {
            if (i + k >= argc) {
                std::fprintf(stderr, "%s needs %d argument(s)\n", a.c_str(), k);
                std::exit(2);
            }
        };
        auto vec3 = [&](float *v) {
            need(3);
            for (int k = 0; k < 3; ++k) v[k] = (float)std::atof(argv[++i]);
        };
        if (a == "--validation") { need(1); validation_prefix = argv[++i]; validation = true; }
        else if (a == "--validation-spp") { need(1); target_spp = std::atoi(argv[++i]); }
        else if (a == "--profiling") { need(1); csv_prefix = argv[++i]; profiling = true; }
        else if (a == "--profiling-fps") { need(1); profiling_fps = (float)std::atof(argv[++i]); if (profiling_fps <= 1) profiling_fps = 1; have_profiling_options = true; }
        else if (a == "--profiling-img") { need(1); profiling_img_prefix = argv[++i]; have_profiling_options = true; }
        else if (a == "--benchmark-file") { std::fprintf(stderr, "--benchmark-file <name>.csv is now --profiling <name>\n"); return 2; } // cmdline.cpp:409-413
        else if (a == "--profiling-frames") { // the reference's old spelling of --profiling-fps (cmdline.cpp:397-403)
            need(1); profiling_fps = (float)std::atof(argv[++i]); if (profiling_fps <= 1) profiling_fps = 1; have_profiling_options = true; }
        else if (a == "--frames-in-flight") { need(1); frames_in_flight = std::max(1, std::min(16, std::atoi(argv[++i]))); }   // (this host's: the pipelined schedule of bench.py)
        else if (a == "--frames-per-launch") { need(1); frames_per_launch = std::max(1, std::min(8, std::atoi(argv[++i]))); got_frames_per_launch = true; }
        else if (a == "--synchronous") synchronous = true;   // AppState::synchronous_rendering ("force synchronous rendering", libapp/app_state.cpp:145)
        else if (a == "--fly-through") fly_through = true;   // (this host's: bench.py's camera path)
        else if (a == "--profiling-count") { need(1); profiling_frames = std::atoi(argv[++i]); have_profiling_options = true; } // (this host's: frames of a run without keyframes)
        else if (a == "--animate-wave") { need(2); wave_amp = (float)std::atof(argv[++i]); wave_k = (float)std::atof(argv[++i]); }
        else if (a == "--skin") { need(1); skin_path = argv[++i]; }
        else if (a == "--bones") { need(1); bones_path = argv[++i]; }
        else if (a == "--morph") { need(1); morph_path = argv[++i]; }
        else if (a == "--morph-weights") { need(1); morph_weights_path = argv[++i]; }
        else if (a == "--recompute-normals") recompute_normals = true;
        else if (a == "--generate-mips") generate_mips = true;
        else if (a == "--denoise") { need(1); g_denoise_iterations = std::atoi(argv[++i]); if (g_denoise_iterations < 1 || g_denoise_iterations > 5) { std::fprintf(stderr, "--denoise takes 1..5 iterations\n"); return 2; } }
        else if (a == "--denoise-temporal") { need(1); g_denoise_temporal_iterations = std::atoi(argv[++i]); if (g_denoise_temporal_iterations < 1 || g_denoise_temporal_iterations > 5) { std::fprintf(stderr, "--denoise-temporal takes 1..5 iterations\n"); return 2; } }
        else if (a == "--taa-upscale") g_taa_upscale = true;
        else if (a == "--auto-exposure") g_auto_exposure = true;
        else if (a == "--bloom") { need(1); g_bloom = true; g_bloom_intensity = (float)std::atof(argv[++i]); if (!(g_bloom_intensity >= 0.f) || !std::isfinite(g_bloom_intensity)) { std::fprintf(stderr, "--bloom takes an intensity >= 0\n"); return 2; } }
        else if (a == "--object-motion") g_object_motion = true;
        else if (a == "--img") { need(2); width = std::atoi(argv[++i]); height = std::atoi(argv[++i]); }
        else if (a == "--eye") { vec3(eye); got_eye = true; }
        else if (a == "--center") { vec3(center); got_center = true; }
        else if (a == "--up") { vec3(up); got_up = true; }
        else if (a == "--fov") { need(1); fov = (float)std::atof(argv[++i]); }
        else if (a == "--batch-spp") { need(1); batch_spp = std::atoi(argv[++i]); got_batch_spp = true; }
        else if (a == "--config") { need(1); config_inis.push_back(argv[++i]); }
        else if (a == "--keyframe" || a == "--frame") { // [<length>:]<file> (cmdline.cpp:319-334; --frame: the old spelling)
            need(1);
            std::string v = argv[++i];
            double hold = 1.0;
            const size_t colon = v.find(':');
            if (colon != std::string::npos && colon > 0) {
                char *end = nullptr;
                const double len = std::strtod(v.c_str(), &end);
                if (end == v.c_str() + colon) {
                    hold = len;
                    v.erase(0, colon + 1);
                }
            }
            keyframes.push_back({v, hold});
        }
        else if (a == "--camera") { need(1); ++i; } // an index beyond the scene's cameras leaves the default view (libapp/scene_state.cpp:45-50); the scene file holds one
        else if (a == "--upscale") { need(1); upscale = std::max(1, std::atoi(argv[++i])); }
        else if (a == "--sky-data") { need(1); sky_data = argv[++i]; }
        else if (a == "--stripe-rows") { need(1); stripe_rows = std::atoi(argv[++i]); }
        else if (a == "--devices") { // a count (devices 0..n-1) or a comma-separated list of HIP ordinals
            need(1);
            const std::string v = argv[++i];
            devices.clear();
            if (v.find(',') == std::string::npos) {
                for (int d = 0; d < std::max(1, std::atoi(v.c_str())); ++d) devices.push_back(d);
            } else {
                size_t at = 0;
                while (at <= v.size()) {
                    const size_t comma = v.find(',', at);
                    devices.push_back(std::atoi(v.substr(at, comma == std::string::npos ? std::string::npos : comma - at).c_str()));
                    if (comma == std::string::npos) break;
                    at = comma + 1;
                }
            }
        }
        else if (a == "--variant") { need(1); const char *v = argv[++i]; variant = std::strcmp(v, "diffuse") == 0 ? RPTR_VARIANT_SIMPLE : std::strcmp(v, "gltf-transmission") == 0 ? RPTR_VARIANT_GLTF_TRANSMISSION : RPTR_VARIANT_GLTF; got_variant = true; }
        else if (a == "--every-frame") every_frame = true;
        else if (a == "--remove-first-lods") { need(1); g_load.remove_first_lods = std::max(0, std::atoi(argv[++i])); }
        else if (a == "--instance-pruning") { need(1); g_load.instance_pruning_probability = (float)std::atof(argv[++i]); }
        else if (a == "--small-deformation") g_load.small_deformation = true;
        else if (a == "--ignore-animation") g_load.ignore_animation = true;
        else if (a == "--ignore-textures") g_load.ignore_textures = true;
        else if (a == "--load-specularity") g_load.load_specularity = true;
        else if (a == "--dump-scene") { need(1); dump_scene_path = argv[++i]; describe = true; } // --describe + the scene as read, in the flat layout
        else if (a == "--describe") describe = true; // load the scene, print what was read, do not render
        else if (a == "--pfm") format = FORMAT_PFM;
        else if (a == "--exr") format = FORMAT_EXR;
        else if (a == "--png") format = FORMAT_PNG;
        else if (a == "--data-capture") { need(1); capture_prefix = argv[++i]; data_capture = true; }
        else if (a == "--data-capture-spp") { need(1); capture_spp = std::max(1, std::atoi(argv[++i])); }
        else if (a == "--data-capture-fps") { need(1); capture_fps = std::max(1.0f, (float)std::atof(argv[++i])); }
        else if (a == "--data-capture-no-rgba") capture_rgba = false; // cmdline.cpp:432-452
        else if (a == "--data-capture-no-aovs") capture_albedo = capture_normal = capture_motion = false;
        else if (a == "--data-capture-albedo-roughness") capture_albedo = true;
        else if (a == "--data-capture-normal-depth") capture_normal = true;
        else if (a == "--data-capture-motion") capture_motion = true;
        else if (a == "--vulkan-device") { need(1); devices.assign(1, std::atoi(argv[++i])); } // ProgramArgs::device_override: here the HIP ordinal
        else if (a == "--resource-dir") { need(1); ++i; }      // (shader / resource search path of the reference's backends: nothing to find here)
        else if (a == "--merge-partition-instances") g_merge_partitions = true; // SceneLoaderParams::PerFile::merge_partition_instances, librender/scene.cpp:757-797
        else if (a == "--deduplicate-scene") g_deduplicate = true; // Scene::deduplicate + garbage_collect: less memory, same image
        else if (a == "-h" || a == "--help") want_help = true;
        else if (a == "--backend") { // cmdline.cpp:363-376: the last one wins; this binary hosts one
            need(1);
            const std::string b = argv[++i];
            if (b != "hip" && b != "rptr_hip") { std::fprintf(stderr, "unknown backend %s (available: hip)\n", b.c_str()); return 2; }
        }
        else if (a == "--freeze-frame") freeze_frame = true;
        else if (a == "--rng-variant") { // RenderBackendOptions::rng_variant (render_params.glsl.h:34-43,76)
            need(1);
            rng_variant = rptr::rng_variant_from_name(argv[++i]);
            if (rng_variant < 0) { std::fprintf(stderr, "unknown point set %s (uniform, bn, sobol, z-sobol)\n", argv[i]); return 2; }
        }
        else if (a == "--bn-table") { need(1); bn_table_path = argv[++i]; }
        else if (a == "--force-bvh-rebuild") force_bvh_rebuild = 1;
        else if (a == "--rebuild-triangle-budget") { need(1); rebuild_triangle_budget = std::atoi(argv[++i]); }
        else if (a == "--disable-ui") {}
        else if (a[0] != '-') {
            if (scene_path.empty()) scene_path = a;
            else g_more_scenes.push_back(a);
        }
        else {
            // cmdline.cpp:226-259: the single-dash arguments of old versions get a pointer to their successors
            static const char *old_backends[] = {"-vulkan", "-embree", "-dxr", "-optix", "-metal"};
            static const char *old_args[] = {"-img", "-config", "-validation", "-eye", "-center", "-up", "-fov", "-camera", "-spp", "-profiling-frames"};
            for (const char *o : old_backends)
                if (a == o) std::fprintf(stderr, "%s used to be a command line argument that selects a rendering backend: use --backend <BACKEND> (optional)\n", o);
            for (const char *o : old_args)
                if (a == o) std::fprintf(stderr, "%s used to be a command line argument: long-form arguments take double dashes now (-%s)\n", o, o);
            std::fprintf(stderr, "Unknown argument: %s\n", a.c_str());
            return 2;
        }
    }
    if (describe && !scene_path.empty()) {
        try {
            const rptr::SceneDump s = load_scene(scene_path);
            if (!dump_scene_path.empty()) s.save(dump_scene_path);
            unsigned long long tris = 0, qsum = 0;
            for (size_t i = 0; i < s.geometries.size(); ++i) {
                tris += s.geometries[i].num_tris;
                for (uint64_t q : s.qpos[i]) qsum += q & 0xFFFFFFull;
            }
            std::printf("geometries %zu meshes %zu parameterized_meshes %zu instances %zu materials %zu lights %zu triangles %llu qsum %llu fovy %.6f "
                        "max_path_depth %d bin_size %d sun_w %.6f\n",
                        s.geometries.size(), s.meshes.size(), s.pmeshes.size(), s.instances.size(), s.materials.size(), s.lights.size(), tris, qsum,
                        s.camera.fovy, s.render_params.max_path_depth, s.lighting.bin_size, s.scene_params.sun_radiance[3]);
            if (!config_inis.empty() || !keyframes.empty()) { // ... and what the configuration files make of it
                rptr::HostConfig c;
                c.params = s.render_params;
                c.lighting = s.lighting;
                c.camera = s.camera;
                for (const std::string &ini : config_inis) rptr::load_config(ini, c);
                std::printf("config target_spp %d batch_spp %d max_path_depth %d rr_path_depth %d glossy_only %d exposure %.6f tonemap %d output_channel %d "
                            "output_moment %d bin_size %d variant %d rng_variant %d force_bvh_rebuild %d rebuild_triangle_budget %d bump_scale %.6f sun_changed %d reprojection_mode %d raster_taa %d upscale %d "
                            "cam_pos %.6f %.6f %.6f cam_dir %.6f %.6f %.6f\n",
                            c.target_spp, c.params.batch_spp, c.params.max_path_depth, c.params.rr_path_depth, c.params.glossy_only_mode, c.params.exposure,
                            c.params.early_tone_mapping_mode, c.params.output_channel, c.params.output_moment, c.lighting.bin_size, c.variant, c.rng_variant, c.force_bvh_rebuild,
                            c.rebuild_triangle_budget, c.bump_scale, c.sun_changed ? 1 : 0, c.params.reprojection_mode, c.params.enable_raster_taa, c.params.render_upscale_factor, c.camera.pos[0], c.camera.pos[1], c.camera.pos[2], c.camera.dir[0],
                            c.camera.dir[1], c.camera.dir[2]);
                for (const Keyframe &k : keyframes) {
                    rptr::HostConfig kc = c;
                    const int blocks = rptr::load_config(k.ini, kc);
                    std::printf("keyframe hold %.6f blocks %d exposure %.6f cam_pos %.6f %.6f %.6f\n", k.hold, blocks, kc.params.exposure, kc.camera.pos[0],
                                kc.camera.pos[1], kc.camera.pos[2]);
                }
            }
            return 0;
        } catch (const std::exception &e) {
            std::fprintf(stderr, "rptr_hip: %s\n", e.what());
            return 3;
        }
    }
    if (validation && target_spp < 1) { // "< 1: write after every frame" -- needs an end here: one frame
        every_frame = true;
        target_spp = 1;
    }
    if (have_profiling_options && !profiling) { // cmdline.cpp:489-494
        std::fprintf(stderr, "got profiling automation options without profiling mode, enable it using --profiling <stats>\n");
        return 2;
    }
    if (g_taa_upscale && g_denoise_iterations > 0) {
        std::fprintf(stderr, "--taa-upscale and --denoise cannot be combined: the denoised image has the render resolution, the upscaler reads the frame's own\n");
        return 2;
    }
    if (g_denoise_temporal_iterations > 0 && g_denoise_iterations > 0) {
        std::fprintf(stderr, "--denoise-temporal and --denoise cannot be combined: both write the denoised images, choose one\n");
        return 2;
    }
    if (g_denoise_temporal_iterations > 0 && g_taa_upscale) {
        std::fprintf(stderr, "--denoise-temporal and --taa-upscale cannot be combined: the denoised image has the render resolution, the upscaler reads the frame's own\n");
        return 2;
    }
    if (g_denoise_temporal_iterations > 0 && devices.size() > 1) {
        std::fprintf(stderr, "--denoise-temporal needs one device (rptr_hip_denoise_temporal refuses world_size > 1)\n");
        return 2;
    }
    if (g_taa_upscale && devices.size() > 1) {
        std::fprintf(stderr, "--taa-upscale needs one device (rptr_hip_taa_upscale refuses world_size > 1)\n");
        return 2;
    }
    if (const char *why = auto_exposure_refusal(devices.size())) {
        std::fputs(why, stderr);
        return 2;
    }
    if (const char *why = bloom_refusal(devices.size())) {
        std::fputs(why, stderr);
        return 2;
    }
    if (g_object_motion) {
        const size_t n = scene_path.size();
        const char *why = nullptr;
        if (devices.size() > 1) why = "needs one device (rptr_hip_object_motion refuses world_size > 1)";
        else if (validation) why = "needs --data-capture or --profiling: a validation run accumulates one still scene";
        else if (!data_capture && !g_taa_upscale && g_denoise_temporal_iterations == 0)
            why = "needs --denoise-temporal, --taa-upscale or --data-capture: nothing else reads the rewritten motion image";
        else if (n < 4 || scene_path.compare(n - 4, 4, ".vks") != 0 || !g_more_scenes.empty() || g_load.ignore_animation)
            why = "plays the animated transforms of ONE .vks file (not with --ignore-animation)";
        else if (data_capture && !keyframes.empty()) why = "captures one image set per frame of the file: not with --keyframe";
        else if (wave_amp != 0.f || freeze_frame) why = "cannot be combined with --animate-wave or --freeze-frame";
        if (why) {
            std::fprintf(stderr, "--object-motion %s\n", why);
            return 2;
        }
    }
    if (!skin_path.empty() || !bones_path.empty()) {
        const char *why = nullptr;
        if (skin_path.empty() || bones_path.empty()) why = "go together: the influences of mesh 0's vertices and the bone matrices of every frame";
        else if (wave_amp != 0.f) why = "cannot be combined with --animate-wave: both write the vertices of mesh 0";
        else if (validation) why = "need --profiling or --data-capture: a validation run accumulates one still scene";
        if (why) {
            std::fprintf(stderr, "--skin and --bones %s\n", why);
            return 2;
        }
    }
    if (!morph_path.empty() || !morph_weights_path.empty()) {
        const char *why = nullptr;
        if (morph_path.empty() || morph_weights_path.empty()) why = "go together: the targets of mesh 0's vertices and the weights of every frame";
        else if (wave_amp != 0.f) why = "cannot be combined with --animate-wave: both write the vertices of mesh 0";
        else if (validation) why = "need --profiling or --data-capture: a validation run accumulates one still scene";
        if (why) {
            std::fprintf(stderr, "--morph and --morph-weights %s\n", why);
            return 2;
        }
    }
    if (recompute_normals) {
        const char *why = nullptr;
        if (wave_amp == 0.f && skin_path.empty() && morph_path.empty()) why = "needs --animate-wave, --skin --bones or --morph --morph-weights: nothing else writes the vertices of mesh 0";
        else if (wave_amp != 0.f && !profiling) why = "with --animate-wave needs --profiling: the wave runs in profiling mode only";
        if (why) {
            std::fprintf(stderr, "--recompute-normals %s\n", why);
            return 2;
        }
    }
    if (want_help) scene_path.clear(); // prints the usage
    if (scene_path.empty() || (int)validation + (int)profiling + (int)data_capture != 1 || batch_spp < 1 || width < 1 || height < 1 || (profiling && profiling_frames < 1)) {
        std::fprintf(stderr, "usage: rptr_hip <scene.rpsc> (--validation <prefix> [--validation-spp n] | --profiling <csv prefix> [--profiling-fps f] "
                             "[--profiling-img <prefix>] [--keyframe [len:]file.ini ...] [--profiling-count n] [--synchronous] [--fly-through] [--frames-in-flight n [--frames-per-launch b]] [--animate-wave a k [--recompute-normals]]) [--img w h] [--denoise iterations | --denoise-temporal iterations | --taa-upscale] [--auto-exposure] [--bloom intensity] [--object-motion] [--generate-mips] [--eye x y z] [--center x y z] "
                             "[--up x y z] [--fov deg] [--variant gltf|diffuse] [--batch-spp k] [--every-frame] [--exr|--pfm|--png] [--config file.ini ...] [--sky-data <dir of the Hosek-Wilkie data headers>]\n"
                             "       rptr_hip <scene.rpsc> --data-capture <prefix> [--data-capture-spp n] [--data-capture-no-rgba] [--data-capture-no-aovs] "
                             "[--data-capture-albedo-roughness] [--data-capture-normal-depth] [--data-capture-motion] [--keyframe ...]   (EXR images per keyframe)\n"
                             "       <scene.vks>: [--remove-first-lods n] [--instance-pruning p] [--small-deformation] [--ignore-animation] [--ignore-textures] "
                             "[--load-specularity] [--dump-scene out.rpsc]\n"
                             "       <scene_file> [<scene_file>...] [--deduplicate-scene] [--merge-partition-instances]\n"
                             "validation, profiling and data-capture mode are mutually exclusive (cmdline.cpp:479-486)\n");
        return 2;
    }
    try {
        rptr::SceneDump scene = load_scene(scene_path);
        // ---- configuration: the scene file's state, then every --config in order, then the command line (main.cpp:121-149, app.cpp:204-213)
        rptr::HostConfig base;
        base.params = scene.render_params;
        base.lighting = scene.lighting;
        base.camera = scene.camera;
        for (const std::string &ini : config_inis) {
            std::printf("Loading config from %s\n", ini.c_str());
            rptr::load_config(ini, base);
        }
        std::vector<rptr::HostConfig> frames; // one per keyframe (profiling mode); empty = the base configuration throughout
        std::vector<double> holds;
        for (const Keyframe &k : keyframes) {
            std::printf("Loading config from %s\n", k.ini.c_str());
            const std::vector<rptr::IniBlock> blocks = rptr::parse_ini(k.ini);
            // every [Application] block of a keyframe file that changes the state is a keyframe; a static file is held for `hold` seconds
            rptr::HostConfig state = frames.empty() ? base : frames.back();
            for (const rptr::IniBlock &b : blocks) rptr::apply_ini_object(b.root, state);
            frames.push_back(state);
            holds.push_back(k.hold);
        }
        // the sky of a scene state (update_config -> update_sky_light, vulkan/render_sky.cpp:25-72): fitted here when a configuration names
        // Sun settings and the Hosek-Wilkie data headers are at hand (--sky-data / RPTR_SKY_DATA; host/sky_fit.hpp)
        rptr::SkyTables sky_tables;
        bool have_sky = false;
        if (sky_data.empty() && std::getenv("RPTR_SKY_DATA")) sky_data = std::getenv("RPTR_SKY_DATA");
        if (!sky_data.empty()) {
            std::string err;
            have_sky = rptr::load_sky_tables(sky_data, sky_tables, err);
            if (!have_sky) throw std::runtime_error("--sky-data: " + err);
            if (!err.empty()) std::fprintf(stderr, "note: %s\n", err.c_str());
        }
        const RptrSceneParams file_sky = scene.scene_params;
        auto sky_of = [&](rptr::HostConfig &c) { // the scene parameters of one state; reference defaults where no file named a value
            RptrSceneParams sp = file_sky;
            if (c.bump_scale > 0.f) sp.normal_z_scale = 1.0f / c.bump_scale; // render_vulkan.cpp:2954-2959
            if (!c.sun_changed) return sp;
            if (!have_sky) {
                const char *note = "Sun settings (height / angle / turbidity / Color) need the Hosek-Wilkie data headers (--sky-data <dir> / RPTR_SKY_DATA): the scene file's sky is kept";
                if (std::find(c.notes.begin(), c.notes.end(), note) == c.notes.end()) c.notes.push_back(note);
                return sp;
            }
            float height, angle;
            rptr::sun_height_angle_from_dir(file_sky.sun_dir, height, angle);
            float dir[3] = {file_sky.sun_dir[0], file_sky.sun_dir[1], file_sky.sun_dir[2]};
            if (!std::isnan(c.sun_height) || !std::isnan(c.sun_angle)) // scene_state.h:85-90
                rptr::sun_dir_from_height_angle(std::isnan(c.sun_height) ? height : c.sun_height, std::isnan(c.sun_angle) ? angle : c.sun_angle, dir);
            const float turbidity = std::isnan(c.turbidity) ? 3.0f : std::min(10.0f, std::max(1.0f, c.turbidity)); // SceneConfig defaults, render_params.glsl.h:157-162
            const float albedo[3] = {std::isnan(c.albedo[0]) ? 0.2f : c.albedo[0], std::isnan(c.albedo[1]) ? 0.2f : c.albedo[1], std::isnan(c.albedo[2]) ? 0.2f : c.albedo[2]};
            rptr::fit_sky(sky_tables, dir, turbidity, albedo, (int)scene.lights.size(), sp);
            return sp;
        };
        scene.scene_params = sky_of(base);
        for (const rptr::HostConfig *c : {&base})
            for (const std::string &n : c->notes) std::fprintf(stderr, "note: %s\n", n.c_str());
        if (base.target_spp > 0 && !validation) target_spp = base.target_spp;
        if (!got_batch_spp) batch_spp = std::max(1, base.params.batch_spp);
        if (!got_variant && base.variant >= 0) variant = base.variant;
        if (upscale >= 1) base.params.render_upscale_factor = upscale;
        if (base.auto_exposure >= 0) g_auto_exposure = g_auto_exposure || base.auto_exposure != 0; // (.ini "auto exposure": the flag's equal)
        if (const char *why = auto_exposure_refusal(devices.size())) {
            std::fputs(why, stderr);
            return 2;
        }
        g_auto_exposure_params = rptr::RenderHip::auto_exposure_defaults();
        g_auto_exposure_params.source = g_denoise_iterations > 0 || g_denoise_temporal_iterations > 0 ? 1 : 0;
        g_auto_exposure_params.tone_mapping_mode = base.params.early_tone_mapping_mode;
        if (!std::isnan(base.exposure_key)) g_auto_exposure_params.key = base.exposure_key;
        for (int k = 0; k < 3; ++k)
            if (!std::isnan(base.white_balance[k])) g_auto_exposure_params.white_balance[k] = base.white_balance[k];
        g_bloom_params = rptr::RenderHip::bloom_defaults();
        g_bloom_params.source = g_auto_exposure_params.source;
        g_bloom_params.exposure_mode = g_auto_exposure ? 1 : 0;
        g_bloom_params.tone_mapping_mode = g_auto_exposure_params.tone_mapping_mode;
        g_bloom_params.intensity = g_bloom_intensity;
        for (int k = 0; k < 3; ++k) g_bloom_params.white_balance[k] = g_auto_exposure_params.white_balance[k];
        const bool expose_frames = g_auto_exposure && g_denoise_iterations == 0; // (--denoise runs when an image is written: save_image exposes there)
        // --skin <file>: raw RptrSkinVertex records of geometry first_geometry of mesh 0; --bones <file>: two uint32 (frames, bones), then
        // frames x bones x 12 float32. Both are checked against the scene before a device is touched.
        const bool skinned = !skin_path.empty();
        std::vector<RptrSkinVertex> skin_records;
        std::vector<float> bone_frames;
        uint32_t n_bone_frames = 0, n_bones = 0;
        auto slurp = [](const std::string &path, std::vector<char> &out) {
            FILE *f = std::fopen(path.c_str(), "rb");
            if (!f) return false;
            std::fseek(f, 0, SEEK_END);
            const long n = std::ftell(f);
            std::fseek(f, 0, SEEK_SET);
            out.resize(n > 0 ? (size_t)n : 0);
            const bool ok = out.empty() || std::fread(out.data(), 1, out.size(), f) == out.size();
            std::fclose(f);
            return ok;
        };
        if (skinned) {
            if (scene.meshes.empty() || !(scene.meshes[0].dynamic & (RPTR_MESH_DYNAMIC | RPTR_MESH_SUBTLY_DYNAMIC))) {
                std::fprintf(stderr, "--skin needs a scene whose mesh 0 is dynamic\n");
                return 2;
            }
            const size_t n_vertices = (size_t)scene.geometries[scene.meshes[0].first_geometry].num_tris * 3;
            std::vector<char> raw;
            if (!slurp(skin_path, raw) || raw.size() != n_vertices * sizeof(RptrSkinVertex)) {
                std::fprintf(stderr, "--skin %s: %zu bytes, geometry %u has %zu unrolled vertices of %zu bytes each\n", skin_path.c_str(), raw.size(),
                             scene.meshes[0].first_geometry, n_vertices, sizeof(RptrSkinVertex));
                return 2;
            }
            skin_records.resize(n_vertices);
            if (!raw.empty()) std::memcpy(skin_records.data(), raw.data(), raw.size());
            if (slurp(bones_path, raw) && raw.size() >= 8) {
                std::memcpy(&n_bone_frames, raw.data(), 4);
                std::memcpy(&n_bones, raw.data() + 4, 4);
            }
            if (n_bone_frames < 1 || n_bones < 1 || n_bones > RPTR_MAX_BONES || raw.size() != 8 + (size_t)n_bone_frames * n_bones * 48) {
                std::fprintf(stderr, "--bones %s: %zu bytes do not hold a header of two uint32 (frames %u, bones %u of at most %d) and frames x bones x 12 float32\n",
                             bones_path.c_str(), raw.size(), n_bone_frames, n_bones, RPTR_MAX_BONES);
                return 2;
            }
            bone_frames.resize((size_t)n_bone_frames * n_bones * 12);
            std::memcpy(bone_frames.data(), raw.data() + 8, bone_frames.size() * sizeof(float));
        }
        // --morph <file>: uint32 targets, then per target uint32 deltas and that many RptrMorphDelta records, for the same geometry;
        // --morph-weights <file>: two uint32 (frames, targets), then frames x targets float32. Checked like the two above.
        const bool morphed = !morph_path.empty();
        const bool deformed = skinned || morphed; // mesh 0 is posed before every frame
        std::vector<std::vector<RptrMorphDelta>> morph_targets;
        std::vector<float> morph_weight_frames;
        uint32_t n_weight_frames = 0, n_morph_targets = 0;
        if (morphed) {
            if (scene.meshes.empty() || !(scene.meshes[0].dynamic & (RPTR_MESH_DYNAMIC | RPTR_MESH_SUBTLY_DYNAMIC))) {
                std::fprintf(stderr, "--morph needs a scene whose mesh 0 is dynamic\n");
                return 2;
            }
            const size_t n_vertices = (size_t)scene.geometries[scene.meshes[0].first_geometry].num_tris * 3;
            std::vector<char> raw;
            uint32_t file_targets = 0;
            bool ok = slurp(morph_path, raw) && raw.size() >= 4;
            size_t at = 4;
            if (ok) std::memcpy(&file_targets, raw.data(), 4);
            ok = ok && file_targets >= 1 && file_targets <= RPTR_MAX_MORPH_TARGETS;
            for (uint32_t t = 0; ok && t < file_targets; ++t) {
                uint32_t deltas = 0;
                ok = raw.size() - at >= 4;
                if (!ok) break;
                std::memcpy(&deltas, raw.data() + at, 4);
                at += 4;
                ok = (raw.size() - at) / sizeof(RptrMorphDelta) >= deltas;
                if (!ok) break;
                morph_targets.emplace_back(deltas);
                if (deltas) std::memcpy(morph_targets.back().data(), raw.data() + at, (size_t)deltas * sizeof(RptrMorphDelta));
                at += (size_t)deltas * sizeof(RptrMorphDelta);
                for (const RptrMorphDelta &d : morph_targets.back()) ok = ok && d.vertex < n_vertices;
            }
            if (!ok || at != raw.size()) {
                std::fprintf(stderr, "--morph %s: %zu bytes do not hold uint32 targets (%u of at most %d) and per target uint32 deltas and that many %zu-byte records "
                                     "that name the %zu unrolled vertices of geometry %u\n",
                             morph_path.c_str(), raw.size(), file_targets, RPTR_MAX_MORPH_TARGETS, sizeof(RptrMorphDelta), n_vertices, scene.meshes[0].first_geometry);
                return 2;
            }
            if (slurp(morph_weights_path, raw) && raw.size() >= 8) {
                std::memcpy(&n_weight_frames, raw.data(), 4);
                std::memcpy(&n_morph_targets, raw.data() + 4, 4);
            }
            if (n_weight_frames < 1 || n_morph_targets < 1 || n_morph_targets > RPTR_MAX_MORPH_TARGETS || raw.size() != 8 + (size_t)n_weight_frames * n_morph_targets * 4) {
                std::fprintf(stderr, "--morph-weights %s: %zu bytes do not hold a header of two uint32 (frames %u, targets %u of at most %d) and frames x targets float32\n",
                             morph_weights_path.c_str(), raw.size(), n_weight_frames, n_morph_targets, RPTR_MAX_MORPH_TARGETS);
                return 2;
            }
            if (n_morph_targets != file_targets) {
                std::fprintf(stderr, "--morph-weights %s holds weights for %u targets, --morph %s holds %u targets\n", morph_weights_path.c_str(), n_morph_targets,
                             morph_path.c_str(), file_targets);
                return 2;
            }
            morph_weight_frames.resize((size_t)n_weight_frames * n_morph_targets);
            std::memcpy(morph_weight_frames.data(), raw.data() + 8, morph_weight_frames.size() * sizeof(float));
        }
        // --recompute-normals: the written geometry welded at its rest pose (normal_groups.hpp); bound once the scene is set
        std::vector<uint32_t> normal_group_labels;
        if (recompute_normals) {
            if (scene.meshes.empty() || !(scene.meshes[0].dynamic & (RPTR_MESH_DYNAMIC | RPTR_MESH_SUBTLY_DYNAMIC))) {
                std::fprintf(stderr, "--recompute-normals needs a scene whose mesh 0 is dynamic\n");
                return 2;
            }
            const RptrGeometryDesc &g = scene.geometries[scene.meshes[0].first_geometry];
            if (!g.has_normals || !g.qnrm_uv) {
                std::fprintf(stderr, "--recompute-normals needs normals on geometry %u: there are no normal words to recompute\n", scene.meshes[0].first_geometry);
                return 2;
            }
            const size_t n_vertices = (size_t)g.num_tris * 3;
            const std::vector<float> rest_xyz = rest_positions(g);
            std::vector<uint32_t> words(n_vertices);
            for (size_t v = 0; v < n_vertices; ++v) words[v] = uint32_t(g.qnrm_uv[v]);
            normal_group_labels = rptr::normal_groups(rest_xyz.data(), words.data(), n_vertices);
        }
        if (frames_in_flight == 1) synchronous = true; // (one frame context: nothing to overlap)
        // frame contexts: the reference's two swap buffers; what --frames-in-flight asks for; four for a queued --validation accumulation
        // (its launch sequences are independent of the display: the deeper queue is what fills the GPU)
        const int contexts = std::max(frames_in_flight, (validation && !synchronous && !freeze_frame) ? 4 : (int)rptr::RenderHip::MAX_SWAP_BUFFERS);
        rptr::RenderGroup backend(devices, stripe_rows, contexts, RPTR_CREATE_SET_HW_QUEUES); // (this program owns its process: a hardware queue per frame context)
        backend.initialize(width, height);
        backend.set_scene(scene.desc());
        {
            // a scene that animates (instances that move, meshes that deform) registers where its lights came from, so that a refit
            // re-places the lights of emitters that moved (a scene read from a dump carries no provenance: nothing to register)
            bool animates = false;
            for (const RptrMeshDesc &m : scene.meshes) animates = animates || m.dynamic != 0;
            if (animates && !scene.lights.empty() && scene.light_sources.size() == scene.lights.size()) {
                try {
                    backend.set_light_sources(scene.light_sources);
                } catch (const std::exception &e) { // (the scene renders as it did before: lights stay where set_scene got them)
                    std::fprintf(stderr, "rptr_hip: light sources not registered: %s\n", e.what());
                }
            }
        }
        // --generate-mips: the chains of the textures that came without one, made on the device before the first frame
        if (generate_mips)
            for (uint32_t t = 0; t < (uint32_t)scene.textures.size(); ++t) {
                const RptrTextureDesc &td = scene.textures[t];
                if (td.mip_levels > 1u) continue;
                if (backend.update_texture(t, nullptr, 0, true))
                    std::printf("generate-mips: texture %u %u x %u -> %u levels\n", t, td.width, td.height, backend.texture_levels(t));
                else
                    std::printf("generate-mips: texture %u %u x %u skipped (emissive)\n", t, td.width, td.height);
            }
        // --skin / --bones: mesh 0's first geometry is bound at its rest pose; pose(k) stages the bones of the file's frame k mod frames,
        // skins and refits (positions, shading normals and -- with registered sources -- lights follow)
        // --morph / --morph-weights: the same geometry gets its targets; pose(k) stages the weights of the file's frame k mod frames first
        // (the morph stage runs in front of the skin, from the one rest pose the two share)
        if (skinned) backend.set_skin(scene.meshes[0].first_geometry, skin_records);
        if (morphed) backend.set_morph_targets(scene.meshes[0].first_geometry, morph_targets);
        // --recompute-normals: the same geometry's corners in their welded groups; the normals are recomputed in front of every refit
        if (recompute_normals) backend.set_normal_groups(scene.meshes[0].first_geometry, normal_group_labels);
        auto pose = [&](uint64_t k) {
            if (skinned) backend.update_bones(0, n_bones, &bone_frames[(size_t)(k % n_bone_frames) * n_bones * 12]);
            if (morphed) backend.update_morph_weights(scene.meshes[0].first_geometry, 0, n_morph_targets, &morph_weight_frames[(size_t)(k % n_weight_frames) * n_morph_targets]);
            backend.skin();
            if (recompute_normals) backend.recompute_normals();
            backend.refit();
        };
        // --object-motion: the file's transform table stays open; play(k) stages the transforms of the file's frame k mod numFrames that
        // differ from the ones staged last (static instances -- which may be baked into the flattened tree -- are never named) and refits
        rptr::vks::Header anim;
        std::vector<float> anim_xf;
        if (g_object_motion) {
            anim = rptr::vks::read_header(scene_path);
            if (anim.numFrames < 2 || anim.numAnimatedTransforms == 0) {
                std::fprintf(stderr, "--object-motion: %s has no animated transforms (numFrames %llu)\n", scene_path.c_str(), (unsigned long long)anim.numFrames);
                return 2;
            }
            anim_xf = rptr::vks::frame_transforms(anim, g_load.frame, g_load.instance_pruning_probability);
            if (anim_xf.size() != 12 * scene.instances.size()) throw std::runtime_error("--object-motion: the file's instances are not the loaded scene's");
            backend.track_object_motion();
        }
        auto play = [&](uint64_t k) {
            const std::vector<float> xf = rptr::vks::frame_transforms(anim, k % anim.numFrames, g_load.instance_pruning_probability);
            const size_t n = xf.size() / 12;
            for (size_t i = 0; i < n;) {
                if (!std::memcmp(&xf[12 * i], &anim_xf[12 * i], 48)) {
                    ++i;
                    continue;
                }
                size_t j = i + 1;
                while (j < n && std::memcmp(&xf[12 * j], &anim_xf[12 * j], 48)) ++j;
                backend.update_instances((uint32_t)i, (uint32_t)(j - i), &xf[12 * i]);
                i = j;
            }
            anim_xf = xf;
            backend.refit();
        };
        base.params.batch_spp = batch_spp;
        backend.set_params(base.params, base.lighting);
        backend.update_config(scene.scene_params);
        // render backend options: the point set (with the table its render extension uploads) and the BVH policy of dynamic meshes
        if (rng_variant < 0) rng_variant = base.rng_variant;
        if (rng_variant > 0) {
            const std::string matrices = data_dir() + "/sobol_matrices_1024x32.u32";
            if (rng_variant == RPTR_RNG_VARIANT_BN)
                backend.set_rng_variant(rng_variant, bn_table_path.empty() ? rptr::white_noise_bn_table(matrices) : rptr::read_bn_table(bn_table_path));
            else
                backend.set_rng_variant(rng_variant, rptr::sobol_table(matrices));
        }
        if (force_bvh_rebuild >= 0 || rebuild_triangle_budget >= 0 || base.bvh_policy_set) { // (otherwise the library's default: refit only)
            if (force_bvh_rebuild < 0) force_bvh_rebuild = base.force_bvh_rebuild;
            if (rebuild_triangle_budget < 0) rebuild_triangle_budget = base.rebuild_triangle_budget;
            backend.set_bvh_policy(force_bvh_rebuild != 0, rebuild_triangle_budget);
        }
        scene.camera = base.camera;
        rptr::RenderConfiguration cfg{};
        std::memcpy(cfg.camera.pos, scene.camera.pos, 12);
        std::memcpy(cfg.camera.dir, scene.camera.dir, 12);
        std::memcpy(cfg.camera.up, scene.camera.up, 12);
        cfg.camera.fovy = scene.camera.fovy;
        if (got_eye) std::memcpy(cfg.camera.pos, eye, 12);
        if (got_center || got_eye) { // OrientedCamera: the view direction is center - eye, normalised
            float c[3] = {0, 0, 0};
            if (got_center) std::memcpy(c, center, 12);
            else for (int k = 0; k < 3; ++k) c[k] = scene.camera.pos[k] + scene.camera.dir[k];
            float d[3], len = 0;
            for (int k = 0; k < 3; ++k) { d[k] = c[k] - cfg.camera.pos[k]; len += d[k] * d[k]; }
            len = std::sqrt(len);
            if (len > 0) for (int k = 0; k < 3; ++k) cfg.camera.dir[k] = d[k] / len;
        }
        if (got_up) std::memcpy(cfg.camera.up, up, 12);
        if (fov > 0) cfg.camera.fovy = fov;
        cfg.active_variant = variant;
        cfg.freeze_frame = freeze_frame;
        cfg.reset_accumulation = true; // frame 0 of the accumulation (app.cpp: reset on scene load)
        std::vector<float> img((size_t)width * height * 4);

        if (validation) {
            int accumulated = 0;
            double gpu_ms = 0.0, image_ms = 0.0; // (image_ms: read-back + file)
            const auto v0 = std::chrono::steady_clock::now();
            // The frames of an accumulation are independent launch chains that only meet in the running mean: they are queued as launch
            // sequences of up to 16 samples (rptr_hip_render_batch_async, reset_rest = 0: frame k continues the accumulation of frame k - 1;
            // every frame bit-identical to the frame rendered on its own) with four sequences in flight, and collected in order -- the images
            // are written at the same sample counts, with the same bits, as by the loop of synchronous frames below (--synchronous; a frozen
            // frame repeats its samples and cannot share a sequence).
            if (!synchronous && !freeze_frame && !g_taa_upscale && g_denoise_temporal_iterations == 0 && (backend.size() == 1 || !every_frame)) { // (a group's gather assembles the LAST frame of a sequence; the upscaler and the temporal denoiser want every frame as it finishes)
                const int total_frames = (target_spp + batch_spp - 1) / batch_spp;
                // (a launch sequence must fit the sample slots the handle holds: 16 up to ~2.9 Mpixel per rank, fewer above -- 12 at 1440p, 5 at 4K,
                // rptr_hip_get_option "sample_slots"; a frame of more samples than that is split by the library itself, one frame per sequence)
                const int slots = (int)std::max<int64_t>(1, backend.get_option("sample_slots"));
                const int fit = std::max(1, slots / std::max(1, batch_spp));
                const int per_seq = std::min(fit, got_frames_per_launch ? frames_per_launch : std::max(1, std::min(8, 16 / std::max(1, batch_spp))));
                struct Pending {
                    rptr::RenderGroup::Sequence q;
                    int first_frame;
                };
                std::vector<Pending> queue;
                int submitted = 0;
                auto collect_one = [&] {
                    const Pending p = queue.front();
                    queue.erase(queue.begin());
                    for (int k = 0; k < p.q.frames; ++k) {
                        const rptr::RenderStats st = backend.collect_frame(p.q, k);
                        accumulated = st.spp;
                        gpu_ms += st.render_time;
                        if (accumulated >= target_spp || every_frame) {
                            const auto w0 = std::chrono::steady_clock::now();
                            save_image(backend, format, validation_prefix, accumulated, "", width, height, img, true);
                            image_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
                        }
                    }
                };
                while (submitted < total_frames) {
                    const int n = std::min(per_seq, total_frames - submitted);
                    cfg.reset_accumulation = submitted == 0;
                    queue.push_back({backend.submit(cfg, batch_spp, n, /*reset_rest=*/false), submitted});
                    submitted += n;
                    if ((int)queue.size() >= contexts) collect_one();
                }
                while (!queue.empty()) collect_one();
            }
            while (accumulated < target_spp) {
                const rptr::RenderStats st = backend.render(cfg); // params.batch_spp samples
                if (g_taa_upscale) backend.taa_upscale(cfg.reset_accumulation);
                if (g_denoise_temporal_iterations > 0) denoise_temporal(backend, cfg.reset_accumulation);
                cfg.reset_accumulation = false;
                accumulated = freeze_frame ? accumulated + batch_spp : st.spp; // (a frozen frame repeats its samples: the application counts, app_state.cpp)
                gpu_ms += st.render_time;
                if (accumulated >= target_spp || every_frame) {
                    const auto w0 = std::chrono::steady_clock::now();
                    save_image(backend, format, validation_prefix, accumulated, "", width, height, img, true);
                    image_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
                }
            }
            {
                const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - v0).count();
                std::printf("%s: wall %.3f ms rendering + %.3f ms images (read-back and files)\n", backend.name().c_str(), wall - image_ms, image_ms);
            }
            std::printf("%s: %d spp in %.3f ms GPU time -> %s_%04d.%s\n", backend.name().c_str(), accumulated, gpu_ms, validation_prefix.c_str(), accumulated,
                        format == FORMAT_PFM ? "pfm" : format == FORMAT_PNG ? "png" : "exr");
            return 0;
        }
        if (data_capture) {
            // libapp/app_state.cpp:499-531: when a frame is ready (--data-capture-spp samples) the accumulation buffer and the three
            // AOV images
            // of every keyframe (one without --keyframe) are stored as <prefix>_%04d_{rgba,albedo_roughness,normal_depth,motion_jitter}.exr;
            // --data-capture-fps only paces the reference's animation clock between captures (a keyframe here is captured once)
            (void)capture_fps;
            // --object-motion: one capture per frame of the file's animation instead, the motion image rewritten before it is stored
            // --skin / --bones without keyframes: one capture per frame of the bones file, each at its pose
            const size_t n_keys = g_object_motion ? (size_t)anim.numFrames : deformed && frames.empty() ? (size_t)(skinned ? n_bone_frames : n_weight_frames) : std::max<size_t>(1, frames.size());
            for (size_t k = 0; k < n_keys; ++k) {
                if (g_object_motion) {
                    if (k) play(g_load.frame + k);
                    cfg.reset_accumulation = true;
                }
                if (deformed) {
                    pose(k);
                    cfg.reset_accumulation = true;
                }
                if (!frames.empty()) {
                    rptr::HostConfig st = frames[k];
                    st.params.batch_spp = batch_spp;
                    if (upscale >= 1) st.params.render_upscale_factor = upscale;
                    backend.set_params(st.params, st.lighting);
                    if (st.sun_changed || st.bump_scale > 0.f) backend.update_config(sky_of(st));
                    std::memcpy(cfg.camera.pos, st.camera.pos, 12);
                    std::memcpy(cfg.camera.dir, st.camera.dir, 12);
                    std::memcpy(cfg.camera.up, st.camera.up, 12);
                    if (!got_variant && st.variant >= 0) cfg.active_variant = st.variant;
                    cfg.reset_accumulation = true;
                }
                int accumulated = 0;
                while (accumulated < capture_spp) {
                    // (--object-motion: the capture's samples in ONE submission -- the pass compares the last two submissions)
                    const rptr::RenderStats st = g_object_motion ? backend.render(cfg, capture_spp) : backend.render(cfg);
                    cfg.reset_accumulation = false;
                    accumulated = st.spp;
                }
                if (g_object_motion) std::printf("object motion: frame %zu, %lld pixels rewritten\n", k + 1, (long long)backend.object_motion());
                char idx[16];
                std::snprintf(idx, sizeof(idx), "_%04d", (int)k + 1);
                const std::string pf = capture_prefix + idx;
                if (capture_rgba) save_image(backend, FORMAT_EXR, capture_prefix, (int)k + 1, "_rgba", width, height, img);
                if (capture_albedo) save_aov(backend, rptr::RenderHip::AOVAlbedoRoughnessIndex, pf + "_albedo_roughness", width, height);
                if (capture_normal) save_aov(backend, rptr::RenderHip::AOVNormalDepthIndex, pf + "_normal_depth", width, height);
                if (capture_motion) save_aov(backend, rptr::RenderHip::AOVMotionJitterIndex, pf + "_motion_jitter", width, height);
                std::printf("%s: %d spp -> %s_*.exr\n", backend.name().c_str(), accumulated, pf.c_str());
            }
            return 0;
        }

        // ---- profiling mode
        std::vector<float> rest, cur; // --animate-wave: float positions of geometry 0 at rest
        if (wave_amp != 0.f) {
            if (scene.meshes.empty() || !scene.meshes[0].dynamic) throw std::runtime_error("--animate-wave needs a scene whose mesh 0 is dynamic");
            rest = rest_positions(scene.geometries[scene.meshes[0].first_geometry]);
            cur = rest;
        }
        const std::string csv_path = csv_prefix + ".csv";
        FILE *csv = std::fopen(csv_path.c_str(), "w");
        if (!csv) throw std::runtime_error("cannot open " + csv_path);
        std::fprintf(csv, "frames_total,keyframe,frames_accumulated,render_time_ms,app_time_ms\n");
        const float dt = 1.f / profiling_fps;
        double current_time = 0.0, gpu_ms = 0.0;
        // keyframes: each is held for its length on the animation timeline (default one second = profiling_fps frames); without
        // keyframes the run lasts --profiling-frames frames of the base configuration
        std::vector<double> key_end;
        if (!frames.empty()) {
            double t = 0.0;
            for (double hsec : holds) key_end.push_back(t += std::max(hsec, (double)dt));
            profiling_frames = std::max(1, (int)std::floor(key_end.back() * profiling_fps + 0.5));
        }
        auto last = std::chrono::steady_clock::now();
        // ---- the plan: per frame its keyframe, its view, whether it restarts the accumulation and whether its keyframe ends with it
        // (libapp/app_state.cpp:484-493: an image once per keyframe, at its end; without keyframe files a keyframe is one second)
        struct FramePlan {
            int key = -1;            // index into `frames` (-1: the base configuration)
            int keyframe_no = 1;     // the CSV's keyframe column
            int accumulated = 1;     // the CSV's frames_accumulated column
            bool reset = false, key_ends = false;
            double time = 0.0;
            rptr::RenderCameraParams camera;
        };
        // --fly-through: bench.py's camera path (camera_of): frame k looks along the view yawed by 0.002 rad x s about its up axis from 2 cm x s
        // further to the right, s = (k mod 64) - 32 (64 views symmetric around the configuration's own); evaluated in double as numpy does,
        // rounded to float once
        const rptr::RenderCameraParams base_camera = cfg.camera;
        auto fly_camera = [&](int k) {
            rptr::RenderCameraParams c = base_camera;
            const int s = k % 64 - 32;
            const double a = 0.002 * s;
            const double d[3] = {base_camera.dir[0], base_camera.dir[1], base_camera.dir[2]}, u[3] = {base_camera.up[0], base_camera.up[1], base_camera.up[2]};
            double r[3] = {d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]};
            const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            for (double &x : r) x /= rl;
            double nd[3];
            for (int i = 0; i < 3; ++i) nd[i] = std::cos(a) * d[i] + std::sin(a) * r[i];
            const double nl = std::sqrt(nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2]);
            for (int i = 0; i < 3; ++i) {
                c.pos[i] = (float)(double(base_camera.pos[i]) + 0.02 * s * r[i]);
                c.dir[i] = (float)(nd[i] / nl);
            }
            return c;
        };
        std::vector<FramePlan> plan((size_t)profiling_frames);
        {
            int active_key = -1, acc = 0;
            rptr::RenderCameraParams cam = cfg.camera;
            for (int frame = 0; frame < profiling_frames; ++frame) {
                FramePlan &p = plan[(size_t)frame];
                p.reset = frame == 0;
                if (!frames.empty()) { // the keyframe this frame belongs to; a change applies its state and restarts the accumulation
                    int k = 0;
                    while (k + 1 < (int)key_end.size() && current_time >= key_end[(size_t)k] - 1e-9) ++k;
                    if (k != active_key) {
                        active_key = k;
                        const rptr::HostConfig &st = frames[(size_t)k];
                        std::memcpy(cam.pos, st.camera.pos, 12);
                        std::memcpy(cam.dir, st.camera.dir, 12);
                        std::memcpy(cam.up, st.camera.up, 12);
                        p.reset = true;
                    }
                }
                if (!rest.empty() || g_object_motion || deformed) p.reset = true; // the geometry moves: the accumulation starts over
                p.camera = cam;
                if (fly_through) { // a moved camera restarts the accumulation (the application resets when the view changes) ...
                    p.camera = fly_camera(frame);
                    // ... unless the history is reprojected (REPROJECTION_MODE_ACCUMULATE, app.cpp:320-327); moving geometry still resets
                    const int mode = active_key >= 0 ? frames[(size_t)active_key].params.reprojection_mode : base.params.reprojection_mode;
                    if (mode != 2) p.reset = true;
                }
                p.key = active_key;
                p.time = current_time;
                acc = p.reset ? 1 : acc + 1;
                p.accumulated = acc;
                p.keyframe_no = frames.empty() ? (int)std::floor(current_time) + 1 : active_key + 1;
                p.key_ends = frames.empty() ? (current_time + dt) >= std::ceil(current_time + 1e-9) : (current_time + dt) >= key_end[(size_t)active_key] - 1e-9;
                if (!freeze_frame) current_time += dt; // --freeze-frame keeps repeating the same frame (app.cpp:339-345)
                else if (!frames.empty() && frame + 1 >= (int)std::floor(key_end[(size_t)active_key] * profiling_fps + 0.5)) current_time = key_end[(size_t)active_key];
            }
        }
        int applied_key = -1;
        auto apply_key = [&](int k) { // the state of keyframe k: parameters, sky, variant (what is submitted from here on uses it)
            if (k < 0 || k == applied_key) return;
            applied_key = k;
            rptr::HostConfig st = frames[(size_t)k];
            st.params.batch_spp = batch_spp;
            if (upscale >= 1) st.params.render_upscale_factor = upscale;
            backend.set_params(st.params, st.lighting);
            if (st.sun_changed || st.bump_scale > 0.f) backend.update_config(sky_of(st));
            if (!got_variant && st.variant >= 0) cfg.active_variant = st.variant;
        };
        auto config_of = [&](const FramePlan &p) {
            rptr::RenderConfiguration c = cfg;
            c.camera = p.camera;
            c.reset_accumulation = p.reset;
            c.time = p.time;
            return c;
        };
        // ---- queued deeper than the reference's two swap buffers (--frames-in-flight n [--frames-per-launch b]): launch sequences of up to b
        // frames of one keyframe, every frame with its own view (rptr_hip_render_batch_cameras_async), n sequences in flight -- the schedule
        // bench.py times (the library asks the HIP runtime for a hardware queue per frame context itself: csrc/rptr_hip.hip
        // ensure_hw_queues). One CSV row per frame as it is collected; render_time_ms is the frame's share of its sequence.
        if (frames_in_flight > 1 && rest.empty() && !deformed && !freeze_frame && !g_object_motion) {
            frames_per_launch = std::min(frames_per_launch, std::max(1, 16 / std::max(1, batch_spp)));
            // reprojection_mode 2 folds each frame into the one before it: one frame per launch sequence (include/rptr_hip.h)
            bool realtime = base.params.reprojection_mode == 2;
            for (const rptr::HostConfig &st : frames) realtime = realtime || st.params.reprojection_mode == 2;
            if (realtime || g_taa_upscale || g_denoise_temporal_iterations > 0 || expose_frames) frames_per_launch = 1; // (auto-exposure meters the last frame of a sequence only; (the upscaler and the temporal denoiser read the AOV images, which are those of a sequence's last frame)
            struct Pending {
                rptr::RenderGroup::Sequence q;
                int first;
            };
            std::vector<Pending> queue;
            apply_key(plan[0].key);
            for (int w = 0; w < 2; ++w) { // warm-up: every context renders once, the adaptive tail hand-over settles
                std::vector<rptr::RenderGroup::Sequence> warm;
                for (int k = 0; k < frames_in_flight; ++k) {
                    rptr::RenderConfiguration c = config_of(plan[0]);
                    c.reset_accumulation = true;
                    warm.push_back(backend.submit(c, batch_spp, frames_per_launch));
                }
                for (const auto &q : warm) backend.collect(q);
            }
            const auto t0 = std::chrono::steady_clock::now();
            const double rays0 = backend.rays_traced();
            last = t0;
            int submitted = 0, collected = 0;
            auto drain_one = [&] {
                const Pending p = queue.front();
                queue.erase(queue.begin());
                for (int k = 0; k < p.q.frames; ++k) {
                    const FramePlan &fp = plan[(size_t)(p.first + k)];
                    const rptr::RenderStats st = backend.collect_frame(p.q, k);
                    if (g_taa_upscale) backend.taa_upscale(fp.reset);
                    if (g_denoise_temporal_iterations > 0) denoise_temporal(backend, fp.reset);
                    if (expose_frames) auto_exposure(backend, fp.reset, p.first + k ? dt : 0.f, p.first + k + 1);
                    gpu_ms += st.render_time;
                    const auto now = std::chrono::steady_clock::now();
                    std::fprintf(csv, "%d,%d,%d,%g,%g\n", ++collected, fp.keyframe_no, fp.accumulated, st.render_time, std::chrono::duration<double, std::milli>(now - last).count());
                    last = now;
                    // (an image per keyframe: of a one-device group, or of the frame a group's gather assembled last)
                    if (!profiling_img_prefix.empty() && fp.key_ends && (backend.size() == 1 || k == p.q.frames - 1))
                        save_image(backend, format, profiling_img_prefix, fp.keyframe_no, "", width, height, img);
                }
            };
            while (submitted < profiling_frames) {
                // the next sequence: frames of ONE keyframe whose later frames all restart the accumulation or all continue it
                int n = 1;
                const FramePlan &f0 = plan[(size_t)submitted];
                while (n < frames_per_launch && submitted + n < profiling_frames && plan[(size_t)(submitted + n)].key == f0.key &&
                       plan[(size_t)(submitted + n)].reset == plan[(size_t)(submitted + 1)].reset && !(n >= 1 && plan[(size_t)(submitted + n - 1)].key_ends && !profiling_img_prefix.empty() && backend.size() > 1))
                    ++n;
                apply_key(f0.key);
                std::vector<rptr::RenderConfiguration> cs;
                for (int k = 0; k < n; ++k) cs.push_back(config_of(plan[(size_t)(submitted + k)]));
                queue.push_back({backend.submit(cs, batch_spp, n > 1 ? plan[(size_t)(submitted + 1)].reset : true), submitted});
                submitted += n;
                if ((int)queue.size() >= frames_in_flight) drain_one();
            }
            while (!queue.empty()) drain_one();
            const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::fclose(csv);
            std::printf("%s: %d frames, %d in flight x %d per launch sequence%s: %.4f ms per frame (wall), %.1f Mrays/s -> %s\n", backend.name().c_str(), profiling_frames,
                        frames_in_flight, frames_per_launch, fly_through ? ", a camera per frame" : "", wall_ms / profiling_frames, (backend.rays_traced() - rays0) / wall_ms * 1e-3,
                        csv_path.c_str());
            return 0;
        }
        // ---- the reference's loop (app.cpp:453-469): begin_frame / draw_frame / end_frame per frame, with the display's command stream (two
        // frames in flight, statistics two frames late) or, --synchronous, without one
        rptr::CommandStream display_stream;
        // (--object-motion: the pass goes between a frame and its consumer, so the loop below renders one frame at a time and issues both)
        backend.upscale_every_frame(g_taa_upscale && !g_object_motion); // (issued as each frame is collected: render_group.hpp frame)
        backend.denoise_temporal_every_frame(g_denoise_temporal_iterations > 0 && !g_object_motion, denoise_temporal_params());
        backend.auto_exposure_every_frame(expose_frames && !g_object_motion, g_auto_exposure_params); // (dt: the step of RenderConfiguration::time)
        rptr::CommandStream *const cmd_stream = synchronous || g_object_motion ? nullptr : &display_stream;
        if (!rest.empty() || fly_through) { // (a short warm-up when the run is a measurement: the adaptive tail hand-over settles in two frames)
            apply_key(plan[0].key);
            for (int w = 0; w < 4; ++w) {
                rptr::RenderConfiguration c = config_of(plan[0]);
                c.reset_accumulation = true;
                backend.frame(cmd_stream, c);
            }
            backend.flush_pipeline();
        }
        const auto loop_t0 = std::chrono::steady_clock::now();
        const double loop_rays0 = backend.rays_traced();
        last = loop_t0;
        for (int frame = 0; frame < profiling_frames; ++frame) {
            const FramePlan &fp = plan[(size_t)frame];
            apply_key(fp.key);
            if (!rest.empty()) { // the geometry moves: new vertices, refit, and the accumulation starts over
                const float phase = 6.283185307179586f * (float)fp.time;
                for (size_t v = 0; v < rest.size() / 3; ++v) cur[3 * v + 1] = rest[3 * v + 1] + wave_amp * std::sin(wave_k * rest[3 * v] + phase);
                backend.update_vertices(scene.meshes[0].first_geometry, cur.data(), (uint32_t)(cur.size() / 3));
                if (recompute_normals) backend.recompute_normals();
                backend.refit();
            }
            if (deformed) pose((uint64_t)frame); // the bones and morph weights of this frame: skin, refit, and the accumulation starts over
            if (g_object_motion && frame) play(g_load.frame + (uint64_t)frame); // the file's next frame: new transforms, refit
            const rptr::RenderStats st = backend.frame(cmd_stream, config_of(fp));
            if (g_object_motion) {
                backend.object_motion();
                if (g_taa_upscale) backend.taa_upscale(frame == 0);
                if (g_denoise_temporal_iterations > 0) denoise_temporal(backend, frame == 0);
                if (expose_frames) auto_exposure(backend, frame == 0, frame ? dt : 0.f, frame + 1);
            } else if (expose_frames && backend.exposure_state_ready())
                // (a synchronous frame's own call; under the command stream the call of the frame collected last, two frames back, like `st`)
                print_exposure(backend.readback_exposure_state(false), cmd_stream ? std::max(1, frame + 1 - (int)rptr::RenderHip::MAX_SWAP_BUFFERS) : frame + 1);
            gpu_ms += st.render_time;
            const auto now = std::chrono::steady_clock::now();
            const double app_ms = std::chrono::duration<double, std::milli>(now - last).count();
            last = now;
            std::fprintf(csv, "%d,%d,%d,%g,%g\n", frame + 1, fp.keyframe_no, fp.accumulated, st.render_time, app_ms);
            if (!profiling_img_prefix.empty() && fp.key_ends) save_image(backend, format, profiling_img_prefix, fp.keyframe_no, "", width, height, img); // (a read-back finishes what is in flight)
        }
        backend.flush_pipeline();
        {
            const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_t0).count();
            std::printf("%s: frame loop %s: %.4f ms per frame (wall), %.1f Mrays/s\n", backend.name().c_str(),
                        cmd_stream ? "through a command stream (two frames in flight)" : "synchronous", wall_ms / profiling_frames,
                        (backend.rays_traced() - loop_rays0) / wall_ms * 1e-3);
        }
        std::fclose(csv);
        std::printf("%s: %d frames at %.3g fps animation time, %.3f ms GPU time per frame -> %s\n", backend.name().c_str(), profiling_frames, profiling_fps,
                    gpu_ms / profiling_frames, csv_path.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "rptr_hip: %s\n", e.what());
        return 3;
    }
    return 0;
}
