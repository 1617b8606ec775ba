/*
 * rptr_hip.h -- C ABI of the MI355X-native wavefront path-tracing backend.
 *
 * This is the drop-in boundary for the reference's PT_MEGAKERNEL / RQ_CLOSEST /
 * PROCESS_SAMPLES hot path.  Everything a `RenderBackend` implementation
 * (reference: librender/render_backend.h:68-116) needs from the device side is
 * reachable through the entry points below; signatures carry plain pointers and
 * sizes only.  The reference-side adapter (`RenderHip : RenderBackend`) that a
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success or a negative RPTR_E_* code; nothing
 *     throws across the ABI.  rptr_hip_last_error() returns a human-readable
 *     message for the most recent failure on that handle (or the global one
 *     when the handle is NULL).
 *   - all calls for one handle come from one thread (reference:
 *     render_backend.h has no concurrent entry points, SURVEY 8b "Threading").
 *   - host arrays passed to rptr_hip_set_scene are borrowed for the duration
 *     of the call only (reference: Scene is destroyed right after set_scene,
 *     app.cpp:150-175).
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     fails with RPTR_E_NO_DEVICE.
 *
 * POD structs are bit-compatible with the reference's shared C++/GLSL structs;
 * the file:line of each is cited next to it.
 */
#ifndef RPTR_HIP_H
#define RPTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPTR_OK 0
#define RPTR_E_INVALID (-1)    /* bad argument / call order                        */
#define RPTR_E_NO_DEVICE (-2)  /* no HIP device / HIP runtime error                */
#define RPTR_E_NOMEM (-3)
#define RPTR_E_UNSUPPORTED (-4)/* feature of the reference not built yet           */
#define RPTR_E_HIP (-5)        /* a HIP call failed, see rptr_hip_last_error       */

/* ---- compile-time constants of the path (librender/render_params.glsl.h:16-18) */
#define RPTR_MAX_PATH_DEPTH 9
#define RPTR_DEFAULT_RR_PATH_DEPTH 2
#define RPTR_BINNED_LIGHTS_BIN_MAX_SIZE 16
#define RPTR_RAY_EPSILON 0.000005f /* vulkan/gpu_params.glsl:27-29 */

/* material flags, rendering/bsdfs/base_material.h.glsl:7-11. A material WITHOUT NOALPHA is alpha-tested: every hit
 * candidate on it goes through the reference's any-hit test (vulkan/pt_megakernel.glsl:153-212) with the alpha channel of
 * its base colour texture (1 for a literal colour). */
#define RPTR_BASE_MATERIAL_NOALPHA 0x01
#define RPTR_BASE_MATERIAL_ONESIDED 0x02
#define RPTR_BASE_MATERIAL_VOLUME 0x04
#define RPTR_BASE_MATERIAL_EXTENDED 0x08
#define RPTR_BASE_MATERIAL_NEURAL 0x10

/* geometry flags, rendering/rt/geometry.h.glsl:66-70 */
#define RPTR_GEOMETRY_FLAGS_NOALPHA 0x01
#define RPTR_GEOMETRY_FLAGS_IMPLICIT_INDICES 0x02

/* integrator variants of this backend (reference: RenderBackend::variant_names).
 * GLTF   = what PT_MEGAKERNEL ships: glTF metallic-roughness BSDF, 2 lobes
 *          (rendering/bsdfs/gltf_bsdf.glsl, GLTF_SUPPORT_TRANSMISSION off).
 * SIMPLE = Lambert-only material (rendering/bsdfs/simple_bsdf.glsl), the
 *          "diffuse-only BSDF" of BASELINE.json configs[1].                     */
#define RPTR_VARIANT_GLTF 0
#define RPTR_VARIANT_SIMPLE 1
/* GLTF_TRANSMISSION = the same BSDF built with GLTF_SUPPORT_TRANSMISSION + GLTF_SUPPORT_TRANSMISSION_ROUGHNESS (what the reference's
 * MEGAKERNEL_MATERIALS / RT-pipeline hit groups compile, gltf_bsdf.glsl:10-13, vulkan/CMakeLists.txt:35-40): a third lobe for
 * BaseMaterial.specular_transmission -- refraction through BASE_MATERIAL_ONESIDED surfaces, thin "double reflection" through
 * two-sided ones; transmission roughness = roughness, reflection roughness = sqrt(clearcoat_gloss) (gltf_bsdf.glsl:38-62). */
#define RPTR_VARIANT_GLTF_TRANSMISSION 2

/* Point sets: the render backend option rng_variant (librender/render_params.glsl.h:34-37,56,76; rendering/pointsets/selected_rng.glsl).
 * UNIFORM = a per-path LCG (lcg_rng.glsl), the default and what BASELINE.json's configurations use. BN = blue-noise dithered sampling
 * (bn_rng.glsl, BN_OPTIMIZED_SPP 1), SOBOL = the Joe-Kuo Sobol' sequence with a fresh random digital shift per draw (sobol.glsl),
 * Z_SBL = the same sequence with sample indices assigned along a shuffled Z-order curve inside 256 x 256 tiles (Z_ORDER_SHUFFLING). */
#define RPTR_RNG_VARIANT_UNIFORM 0
#define RPTR_RNG_VARIANT_BN 1
#define RPTR_RNG_VARIANT_SOBOL 2
#define RPTR_RNG_VARIANT_Z_SBL 3
/* table sizes in bytes, laid out as the reference uploads them:
 * SobolData (rendering/pointsets/sobol_data.h:13-17): uint32 matrix[1024 * 32], tile_invert_1_0[256 * 256];
 * BNData (bn_data.h:12-27): uint32 sobol_spp_d[256 * 256], tile_scrambling_yx_d_1spp[128 * 128 * 8], then six tables that
 * BN_OPTIMIZED_SPP 1 never reads (they may be left off). */
#define RPTR_SOBOL_TABLE_BYTES ((1024u * 32u + 256u * 256u) * 4u)
#define RPTR_BN_TABLE_MIN_BYTES ((256u * 256u + 128u * 128u * 8u) * 4u)

/* rendering/bsdfs/base_material.h.glsl:13-34 -- 80 bytes */
typedef struct RptrBaseMaterial {
    float base_color[3];
    int32_t normal_map;
    uint32_t flags;
    float roughness;
    float specular;
    float metallic;
    float sheen;
    float sheen_tint;
    float clearcoat;
    float clearcoat_gloss;
    float ior;
    float specular_transmission;
    float anisotropy;
    float specular_tint;
    float transmission_color[3];
    float emission_intensity;
} RptrBaseMaterial;

/* rendering/lights/tri.h.glsl:13-26 -- 48 bytes */
typedef struct RptrTriLightData {
    float v0[3];
    float v1[3];
    float v2[3];
    float radiance[3];
} RptrTriLightData;

/* librender/render_params.glsl.h:165-170 -- 32 bytes */
typedef struct RptrRenderRayQuery {
    float origin[3];
    int32_t mode_or_data;
    float dir[3];
    float t_max;
} RptrRenderRayQuery;

/* librender/render_params.glsl.h:123-128 -- 16 bytes */
typedef struct RptrLightSamplingConfig {
    float light_mis_angle;
    int32_t bin_size;
    float min_perceived_receiver_dist;
    float min_radiance;
} RptrLightSamplingConfig;

/* librender/render_params.glsl.h:130-155 -- 80 bytes
 * reprojection_mode (rendering/postprocess/reprojection.h): 0 REPROJECTION_MODE_NONE -- the running mean over every frame since the last
 * reset; 1 REPROJECTION_MODE_DISCARD_HISTORY -- a frame shows its own samples only; 2 REPROJECTION_MODE_ACCUMULATE -- the real-time
 * resolve of the reference's ENABLE_REALTIME_RESOLVE build (csrc/realtime_resolve.h): each render call of `spp` samples is one frame whose
 * mean is folded into the previous frame's history REPROJECTED along the motion AOV (reprojection.glsl:43-367), so a moving camera keeps
 * its history; the new-sample weight falls to 1 / spp_accumulation_window (>= 1), the accumulation image holds (history.rgb,
 * 1 - new-sample weight), the frame shows history.rgb with its coverage alpha. reset_accumulation starts from this frame's mean. The
 * history is what the previous mode-2 frame left (frames in flight: the frame resolved before it); a frame after one of another mode
 * starts from its mean. Mode 2 returns RPTR_E_UNSUPPORTED with world_size > 1 (a stripe's edge pixels reproject into other ranks' rows),
 * for launch sequences of several frames (rptr_hip_render_batch*_async with n_frames > 1) and with option "aovs" = 0 (no motion or
 * normal + depth); option "taa" = 1 with mode 1, or with render_upscale_factor 2, does too. Modes 0 and 1 launch nothing new.
 * (RPTR_HIP_ABI_VERSION stays: no layout changes, and mode 2 was accepted before -- as mode 0.)
 *
 * Depth of field: aperture_radius (scene units; default 0 = a pinhole, bit-identical to what earlier versions rendered whatever
 * focus_distance holds) and focus_distance (scene units along the pinhole ray, default 2.5). With aperture_radius > 0 a camera ray of a
 * frame starts on a uniformly sampled disc of that radius around the camera position, in the plane of the image axes, and passes through
 * the point focus_distance along the pinhole ray of its pixel sample:
 *     focus  = cam_pos + focus_distance * dir
 *     r2     = the path's sample of dimensions DIM_APERTURE_X, _Y (pathspace.h:16-17: 4, 5; the uniform generator: its next two numbers
 *              after the pixel-filter draw -- its first two with enable_raster_taa != 0, which makes no pixel-filter draw)
 *     lens   = (cos(2 pi r2.x), sin(2 pi r2.x)) * sqrt(r2.y) * aperture_radius        [evaluated as sincospif(2 * r2.x)]
 *     origin = cam_pos + lens.x * normalize(cam_du) + lens.y * normalize(cam_dv);  dir = normalize(focus - origin)
 * with the frame's own camera when a launch sequence carries one per frame. Square root and normalisations are IEEE with option
 * "fast_math" too. This is the rule of the reference's vulkan/raygen.rgen:151-160 and pipeline_pt/perspective.rgen:100-108; the
 * pt_megakernel.glsl this library ports is pinhole only (:322-325), so the lens is a stated extension of that port, not parity with it.
 * Not ported: the transport_footprint term of raygen.rgen:216-222 -- the texture footprint stays that of the pinhole axes
 * (pt_megakernel.glsl:341-351). The AOVs keep their definitions (depth is the distance of the hit from the camera position). Ray and
 * radiance queries carry their own origin and direction and ignore the lens. Lens frames run the general kernel instantiations (as
 * raster TAA and table point sets do). A render call returns RPTR_E_INVALID for an aperture_radius that is negative or not finite, and,
 * with aperture_radius > 0, for a focus_distance that is not finite or not > 0.
 * focal_length is accepted and unread: no shipped GPU program of the reference reads it. */
typedef struct RptrRenderParams {
    int32_t batch_spp;
    int32_t max_path_depth;
    int32_t rr_path_depth;
    int32_t glossy_only_mode;
    float aperture_radius;
    float focus_distance;
    float pixel_radius;
    float variance_radius;
    int32_t output_channel;
    int32_t output_moment;
    float exposure;
    int32_t early_tone_mapping_mode;
    int32_t reprojection_mode;
    int32_t spp_accumulation_window;
    int32_t enable_raster_taa;
    int32_t render_upscale_factor;
    float focal_length;
    int32_t _pad3, _pad4, _pad5;
} RptrRenderParams;

/* rendering/lights/sky_model_arhosek/sky_model.h.glsl:7-10 -- 160 bytes */
typedef struct RptrSkyModelParams {
    float configs[9][4];
    float radiances[4];
} RptrSkyModelParams;

/* the scene-wide constants of vulkan/gpu_params.glsl:120-131 (SceneParams) that
 * the host fills in update_config/update_sky_light (vulkan/render_sky.cpp:25-72).
 * light_count / bin bookkeeping is derived by the backend from set_scene.       */
typedef struct RptrSceneParams {
    RptrSkyModelParams sky_params;
    float sun_dir[3];
    float sun_cos_angle;
    float sun_radiance[4]; /* .w = probability of picking the sun in NEE          */
    float normal_z_scale;
    int32_t _pad[3];
} RptrSceneParams;

/* librender/render_backend.h:26-31 (RenderCameraParams) */
typedef struct RptrCamera {
    float pos[3];
    float dir[3];
    float up[3];
    float fovy; /* degrees */
} RptrCamera;

/* one geometry of a mesh: unrolled, quantized vertex streams
 * (REQUIRE_UNROLLED_VERTICES / QUANTIZED_* of vulkan/gpu_params.glsl:7-9;
 *  stream layout = librender/quantize.h:7-35, librender/dequantize.glsl:8-48). */
typedef struct RptrGeometryDesc {
    const uint64_t *qpos;    /* 3*num_tris, 21 bit/axis                           */
    const uint64_t *qnrm_uv; /* 3*num_tris, lo32 = oct normal, hi32 = uv; or NULL */
    uint32_t num_tris;
    uint32_t has_normals;
    uint32_t has_uvs;
    float quantized_scaling[3];
    float quantized_offset[3];
} RptrGeometryDesc;

/* a mesh = one bottom-level acceleration structure (librender/mesh.h:43-72) */
#define RPTR_MESH_DYNAMIC 1u
#define RPTR_MESH_SUBTLY_DYNAMIC 2u
#define RPTR_MESH_INSTANCES_MOVE 4u /* RptrMeshDesc.dynamic bit 2: instances of this mesh may be moved (rptr_hip_update_instances) */
typedef struct RptrMeshDesc {
    uint32_t first_geometry;
    uint32_t num_geometries;
    uint32_t dynamic; /* Mesh::flags (librender/mesh.h:44-47): 0 static; bit 0 RPTR_MESH_DYNAMIC: vertices may be updated, the tree
                       * is refitted -- or, under rptr_hip_set_bvh_policy, rebuilt on the device; bit 1 RPTR_MESH_SUBTLY_DYNAMIC (small
                       * deformations: SceneLoaderParams::small_deformation): updated and refitted, never rebuilt -- the reference builds
                       * such meshes PREFER_FAST_TRACE | ALLOW_UPDATE instead of PREFER_FAST_BUILD (render_vulkan.cpp:942-952);
                       * bit 2 RPTR_MESH_INSTANCES_MOVE: only read by set_scene -- the mesh's instances keep top-level records of their own
                       * instead of being baked into the flattened world-space tree (as for any non-zero value), and the top level gets
                       * room for device-side rebuilds. With this bit alone the mesh's tree is a static build                           */
} RptrMeshDesc;

/* a mesh with a material assignment (librender/mesh.h:78-108, ParameterizedMesh) */
typedef struct RptrParameterizedMeshDesc {
    uint32_t mesh;
    const int32_t *material_offsets; /* one per geometry of the mesh             */
    const uint8_t *tri_material_ids; /* all triangles of the mesh, or NULL       */
} RptrParameterizedMeshDesc;

/* librender/mesh.h:112-116 (Instance) with the transform already dequantized;
 * row-major 3x4 object-to-world like VkAccelerationStructureInstanceKHR
 * (vulkan/render_vulkan.cpp:1262-1268).                                         */
typedef struct RptrInstanceDesc {
    float transform[12];
    uint32_t parameterized_mesh;
} RptrInstanceDesc;

/* A texture: RGBA8, row 0 first, sampled like the reference's material sampler (render_vulkan.cpp:1657-1670: linear filter, linear
 * mip filter, REPEAT addressing, anisotropy 12) over the footprint the path carries to the hit: textureGrad(uv, duvdxy) for material
 * parameters (rendering/rt/material_textures.glsl:37-75 with USE_MIPMAPPING, librender/render_params.glsl.h:8), textureLod(uv, bounce)
 * for normal maps (pt_megakernel.glsl:642-648), level 0 for the any-hit alpha test (:205).
 * mip_levels: 0 or 1 = level 0 only; n = rgba8 holds levels 0..n-1 back to back, level l being max(1, width >> l) x max(1, height >> l)
 * texels (what a .vkt file holds; set_scene generates none: vulkan/resource_utils.cpp:34-100 uploads the levels of the file. "dynamic textures"
 * below makes the chain on the device).
 * srgb != 0: the colour channels are sRGB-encoded (VK_FORMAT_R8G8B8A8_SRGB), alpha is linear. A float material parameter
 * with its sign bit set is a texture handle (rendering/bsdfs/texture_channel_mask.h): bits 0..28 = index into
 * RptrSceneDesc.textures, bits 29..30 = channel for scalar parameters. */
#define RPTR_TEXTURED_PARAM_MASK 0x80000000u
#define RPTR_TEXTURE_ID(bits) ((bits) & 0x1fffffffu)
#define RPTR_TEXTURE_CHANNEL(bits) (((bits) >> 29) & 0x3u)
typedef struct RptrTextureDesc {
    const uint8_t *rgba8;
    uint32_t width, height;
    uint32_t srgb;
    uint32_t mip_levels;
} RptrTextureDesc;

typedef struct RptrSceneDesc {
    const RptrGeometryDesc *geometries;
    uint32_t num_geometries;
    const RptrMeshDesc *meshes;
    uint32_t num_meshes;
    const RptrParameterizedMeshDesc *parameterized_meshes;
    uint32_t num_parameterized_meshes;
    const RptrInstanceDesc *instances;
    uint32_t num_instances;
    const RptrBaseMaterial *materials;
    uint32_t num_materials;
    /* emitters already collected + bin-equalised on the host
     * (librender/lights.cpp:14-90,220-349) */
    const RptrTriLightData *lights;
    uint32_t num_lights;
    /* textures referenced by textured material parameters and normal_map (may be NULL / 0) */
    const RptrTextureDesc *textures;
    uint32_t num_textures;
} RptrSceneDesc;

/* device selection + multi-GPU tile assignment.  The frame is cut
 * into horizontal stripes of `stripe_rows` rows; stripe s belongs to rank
 * s % world_size.  A rank only allocates and renders its own rows. */
/* Threading: a handle is not thread-safe; calls on ONE handle must come from one thread at a time (different handles are
 * independent). Everything is asynchronous to the host only where said so (rptr_hip_render_async, *_device copies). */
/* Version of this header's struct layouts and field meanings. History: 1 = round 1; 2 = RptrTextureDesc._pad became mip_levels, RptrStats grew
 * the stage split; 3 = RptrCreateInfo._pad became abi_version (checked), rank 0 keeps two assembled frames. rptr_hip_abi_version()
 * returns the library's value. Fields named _pad must be zero. 4 = round 5: rptr_hip_set_option / _get_option; rptr_hip_set_frame_schedule /
 * _get_frame_schedule are gone (the device-driven frame schedules they selected lost to the stage launches and left the product).
 * 5 = round 6: RptrCreateInfo.flags (the library no longer touches GPU_MAX_HW_QUEUES unless RPTR_CREATE_SET_HW_QUEUES asks it to),
 * rptr_hip_build_id, option "fast_math", builder experiments behind the "experimental." key prefix.
 * (Moving lights -- RptrLightSource, rptr_hip_set_light_sources, rptr_hip_readback_lights -- leave it at 5: a new struct and two new
 * entry points, no existing struct changes layout and no existing field changes meaning, which is what the number counts.) */
#define RPTR_HIP_ABI_VERSION 5
/* RptrCreateInfo.flags */
#define RPTR_CREATE_SET_HW_QUEUES 1u /* rptr_hip_create may set the HIP runtime's GPU_MAX_HW_QUEUES for the WHOLE host process (setenv) when the
                                      * variable is unset -- to 2, the most hardware queues the library asks for in one process (a card's queue
                                      * slots are shared by every process on it; frame contexts beyond that share queues) -- effective only when
                                      * the process has made no HIP call yet (the runtime reads the variable once). For hosts that own their
                                      * process (bin/rptr_hip sets it); an embedded plugin leaves it clear and the library never edits its host's
                                      * environment: it then notes on stderr, once, when the variable is below 2 (option "quiet" silences it). */
typedef struct RptrCreateInfo {
    int32_t device_ordinal; /* hipSetDevice                                      */
    int32_t rank;
    int32_t world_size;
    int32_t stripe_rows;    /* 0 -> default 32                                   */
    void *stream;           /* hipStream_t to launch on, NULL -> backend-owned   */
    int32_t frames_in_flight; /* 0/1: frames run one after the other on `stream`; 2..16: that many frame contexts with
                               * their own streams, see rptr_hip_render_async. The HIP runtime maps the streams onto
                               * GPU_MAX_HW_QUEUES hardware queues (default 4; streams that share a queue serialise);
                               * the library asks for no more than 2 per process (RPTR_CREATE_SET_HW_QUEUES).       */
    int32_t abi_version;      /* RPTR_HIP_ABI_VERSION of the header the caller was compiled against: rptr_hip_create refuses any other
                               * value (a caller built against an older header would hand over structs whose former padding
                               * fields have since been given a meaning, e.g. RptrTextureDesc.mip_levels) */
    uint32_t flags;           /* RPTR_CREATE_*; 0: nothing outside the handle is touched */
    uint32_t _pad;            /* 0 */
} RptrCreateInfo;

typedef struct RptrStats {
    float render_time_ms;      /* GPU time of the last render call (hipEvents)   */
    float extend_time_ms;      /* sum over closest-hit traversal launches        */
    float connect_time_ms;     /* sum over shadow traversal launches             */
    float shade_time_ms;       /* raygen+sort+shade+resolve                      */
    uint64_t rays_closest;     /* +1 per closest query (pt_megakernel.glsl:440)  */
    uint64_t rays_shadow;      /* +1 per issued shadow query (:223-227)          */
    uint64_t nodes_visited;    /* only when count_traversal was requested: all   */
    uint64_t tris_tested;      /* queries (closest + shadow)                     */
    uint64_t hits_shaded;
    uint64_t nodes_closest;    /* the closest-hit share of nodes_visited         */
    uint64_t tris_closest;
    int32_t spp;               /* accumulated samples per pixel                  */
    int32_t launches_extend;
    int32_t launches_connect;
    int32_t _pad;
    uint64_t device_bytes_allocated;
    /* the parts of shade_time_ms (stage timing level 2): the shade launches alone, the tail kernel (late bounces: extend + shade +
     * connect of a few thousand paths in one launch), the resolve */
    float shade_only_time_ms;
    float tail_time_ms;
    float resolve_time_ms;
    float _pad2;
} RptrStats;

typedef struct rptr_hip rptr_hip_t;

/* ---- lifetime (≙ create_backend_function, render_backend.h:118-119) */
int rptr_hip_create(const RptrCreateInfo *info, rptr_hip_t **out);
int rptr_hip_abi_version(void);
/* a hash over the sources, headers and compiler flags this library was built from (build.py source_id; "unknown" for a hand-made build):
 * measurements that are kept beside the code -- the counter passes of profiles/pmc_traffic.json -- name the build they belong to */
const char *rptr_hip_build_id(void);
/* the acceleration-structure step of the last rptr_hip_set_scene (the reference builds and compacts its BLAS / TLAS on the GPU inside
 * set_scene: vulkan/render_vulkan.cpp:476-543, vulkan/vulkanrt_utils.h:83-105). Large static triangle sets -- a flattened instanced scene,
 * static meshes of millions of triangles -- are built on the device (csrc/ploc.h: Morton sort, PLOC clustering, a binned-SAH top over the
 * remaining clusters, 4-wide collapse, encoding), everything else by the host's binned-SAH builder (options "bvh_builder",
 * "device_build_min_tris"). out_build_ms: wall time of the whole step;
 * out_device_ms: GPU time of the device builds in it (0 when the host built everything). */
int rptr_hip_bvh_build_info(rptr_hip_t *h, int32_t *out_device_built, float *out_build_ms, float *out_device_ms);
/* the scheduling thresholds the traversal kernels use for the current scene (csrc/dtraverse.h: a wave refills its idle lanes once
 * `refill_min` have finished and leaves a node phase once fewer than `node_min` lanes are at inner nodes; 0 = the compile-time defaults
 * 10 / 48) and the measure they were chosen by at set_scene: the surface-area cost of the largest bottom-level tree times that of the top
 * level (>= 24: the dense preset 16 / 32). They change when lanes take their steps, never what a ray finds. Options "traverse_node_min" /
 * "traverse_refill_min" override. No reference counterpart (the reference's traversal is the driver's). */
int rptr_hip_traversal_preset(rptr_hip_t *h, float *out_area_cost, int32_t *out_node_min, int32_t *out_refill_min);
void rptr_hip_destroy(rptr_hip_t *h);
const char *rptr_hip_last_error(const rptr_hip_t *h);
const char *rptr_hip_name(void); /* RenderBackend::name() */
int rptr_hip_set_stream(rptr_hip_t *h, void *hip_stream);

/* ---- RenderBackend::initialize(fb_w, fb_h) (render_vulkan.cpp:246-370) */
int rptr_hip_initialize(rptr_hip_t *h, int fb_width, int fb_height);

/* ---- RenderBackend::set_scene (render_vulkan.cpp:1554-1644): uploads geometry,
 * builds the bottom/top level acceleration structure (include/rptr_bvh.h), uploads materials + binned lights */
int rptr_hip_set_scene(rptr_hip_t *h, const RptrSceneDesc *scene);

/* ---- dynamic meshes: replace the float positions of one geometry and refit
 * (≙ BLAS update + TLAS refit, render_vulkan.cpp:942-952,1323-1354) */
int rptr_hip_update_vertices(rptr_hip_t *h, uint32_t geometry, const float *xyz, uint32_t num_vertices);
/* same with a DEVICE source (the reference animates with a compute shader that writes the float vertex
 * buffer, render_vulkan.cpp:2834-2840): a device-to-device copy ordered on the backend's stream */
int rptr_hip_update_vertices_device(rptr_hip_t *h, uint32_t geometry, const float *device_xyz, uint32_t num_vertices);
int rptr_hip_refit(rptr_hip_t *h);
/* RenderBackendOptions::force_bvh_rebuild / rebuild_triangle_budget (librender/render_params.glsl.h:61,90-93; the reference ships the
 * options and their UI, libapp/app_state.cpp:65-66, but not the animation extension that consumed them): what rptr_hip_refit does with
 * a dynamic mesh whose vertices changed. force_bvh_rebuild != 0: a new tree every time. Otherwise rebuild_triangle_budget triangles
 * may be rebuilt per rptr_hip_refit call -- the budget is saved up until it covers the next dynamic mesh in turn, so a mesh of n
 * triangles gets a new tree every ceil(n / budget) calls and is refitted in between; 0 (the default here) = refit only.
 * A rebuild runs on the device, asynchronously, on the stream of the refit: Morton codes + radix sort + binary radix tree + 4-wide
 * collapse + the encoder of the host builder (csrc/lbvh.h). Ray-query results are those of any tree (closest hit = smallest t, ties
 * by ids); only the number of node visits differs. rptr_hip_bvh_rebuild_count: device-side rebuilds so far (all scene copies). */
int rptr_hip_set_bvh_policy(rptr_hip_t *h, int force_bvh_rebuild, int rebuild_triangle_budget);
int rptr_hip_bvh_rebuild_count(const rptr_hip_t *h, uint64_t *out_rebuilds);

/* ---- moving instances (the reference rebuilds its TLAS from the instance list every time it changes: default_update_tlas,
 * render_vulkan.cpp:1219-1321; request_tlas_operation(Rebuild | Refit), :1323-1354, picks between a build and an update).
 * rptr_hip_update_instances: transforms12 holds `count` row-major 3x4 object-to-world matrices (the layout of
 * RptrInstanceDesc.transform) for scene instances [first_instance, first_instance + count). Like update_vertices the call only STAGES
 * the change: the next rptr_hip_refit writes it into the instance records of every scene copy, on that copy's stream, together with the
 * vertex updates staged for the same refit -- world_to_object with the arithmetic of set_scene, so the records equal those of a fresh
 * set_scene of the moved scene bit for bit -- re-bounds the records and updates the top level. The _device form reads DEVICE memory,
 * ordered on the backend's stream, no host synchronisation; it cannot report a bad matrix: a matrix that is not finite or singular
 * leaves its instance where it was and is counted: rptr_hip_get_option(h, "instance_updates_rejected") (read-only, since set_scene;
 * reading it waits for the backend's stream).
 * Which instances can move: every instance that has top-level records -- all of them in a two-level scene (option flatten = 0, or the
 * scene was not flattened), and in a flattened scene those of meshes with a non-zero RptrMeshDesc.dynamic (RPTR_MESH_INSTANCES_MOVE is
 * the bit that says nothing else). An instance baked into the flat tree: RPTR_E_INVALID. A bad range, NULL, a matrix that is not
 * finite or whose inverse is not (det == 0): RPTR_E_INVALID, nothing is staged. An instance whose parameterized mesh uses an emissive
 * material: RPTR_E_UNSUPPORTED -- RptrSceneDesc.lights are world-space triangles collected by the host and would go stale -- unless
 * rptr_hip_set_light_sources registered where the lights came from (below).
 * rptr_hip_set_tlas_policy: RPTR_TLAS_REBUILD (default, what default_update_tlas does): a refit that finds moved instances builds a
 * NEW top level on the device (csrc/tlas_build.h: Morton keys of the record boxes + radix sort + binary radix tree + 4-wide collapse,
 * one record per leaf, boxes and encoding through the refit) -- in scenes where set_scene reserved room for one, i.e. where some
 * instanced mesh has RPTR_MESH_INSTANCES_MOVE; elsewhere, and under RPTR_TLAS_REFIT, the topology stays and the boxes follow, which
 * degrades without bound once instances travel. Ray-query results are those of any tree. rptr_hip_tlas_rebuild_count: device-side
 * rebuilds of the top level so far (all scene copies); RPTR_TLAS_REFIT leaves it alone.
 * Traversal stack: a rebuilt top level has another depth than the host-built one. set_scene BOUNDS the need of any tree the device build
 * can make over the scene's records (its keys are 30 Morton bits + the index bits wide: at most 3 entries per 4-wide level, never more
 * than records - 1) and fails with the usual RPTR_E_UNSUPPORTED stack message when that bound plus the bottom-level need exceeds the
 * stack; nothing is checked again per rebuild.
 * Frames in flight: a scene with a RPTR_MESH_INSTANCES_MOVE (or dynamic) mesh gives every frame context its own tree and instance
 * records, so a refit never waits -- per context a copy of the node array (88 bytes per node, top level and bottom-level trees are one
 * array) and of the instance records; triangles and shading records are shared unless a mesh deforms --; in any other scene rptr_hip_refit waits for the frames in flight first, as it always did.
 * Limits: a frame writes its motion AOV with motion_vector = 0 for moved objects, as the reference does; rptr_hip_track_object_motion +
 * rptr_hip_object_motion ("object motion" below) rewrite it after the frame for the consumers that run after it (rptr_hip_denoise_temporal,
 * rptr_hip_taa_upscale). reprojection_mode = 2 and option "taa" resolve inside the frame, before that pass can run: there a moved object
 * still ghosts until its history is rejected. rptr_hip_traversal_preset keeps what set_scene
 * chose. The top level's refit after a rebuild runs in one block up to 8192 records; that break-even was estimated, not measured. */
#define RPTR_TLAS_REBUILD 0
#define RPTR_TLAS_REFIT 1
int rptr_hip_update_instances(rptr_hip_t *h, uint32_t first_instance, uint32_t count, const float *transforms12);
int rptr_hip_update_instances_device(rptr_hip_t *h, uint32_t first_instance, uint32_t count, const float *device_transforms12);
int rptr_hip_set_tlas_policy(rptr_hip_t *h, int mode);
int rptr_hip_tlas_rebuild_count(const rptr_hip_t *h, uint64_t *out_rebuilds);

/* ---- moving lights: where every entry of RptrSceneDesc.lights came from, so that a refit can put it where its triangle is now.
 * RptrSceneDesc.lights are world-space triangles the host collected and bin-equalised (librender/lights.cpp:14-90,220-349); the library
 * does not know their origin, so without this call a moved emissive instance is refused (RPTR_E_UNSUPPORTED) and
 * rptr_hip_update_vertices on an emissive dynamic mesh is accepted but leaves the lights WHERE THEY WERE: paths that hit the deformed
 * emitter see it where it is, next-event estimation samples the old triangles, and the estimate is wrong without an error.
 * rptr_hip_set_light_sources(h, sources, count): after set_scene, count == RptrSceneDesc.num_lights, sources[i] describes lights[i]
 * (clones of one emitter repeat its source). Placement rule: a light's world-space vertex is its instance's object_to_world applied to
 * the object-space vertex -- v0..v2 for a static mesh, the current float positions [9 * triangle ..] of `geometry` for a mesh flagged
 * RPTR_MESH_DYNAMIC / _SUBTLY_DYNAMIC -- per row (m0 * x + m1 * y) + (m2 * z + m3) in float32 without contraction, the order of
 * collect_emitters; radiance is never touched. The call checks the provenance on the host, once: the rule with the transforms set_scene
 * received must reproduce lights[i] to 2^-20 * (|m0 x| + |m1 y| + |m2 z| + |m3|) per coordinate. RPTR_E_INVALID, naming the first
 * offending light, for a mismatch, an instance / geometry / triangle out of range, a geometry that is not one of the instance's mesh,
 * count != num_lights, or a call before set_scene; nothing changes then. (NULL, 0) unregisters: the light buffer is the one set_scene
 * uploaded again. A new set_scene drops the registration. world_size > 1 is fine: every rank holds the whole scene, register on each.
 * With sources registered, rptr_hip_update_instances[_device] accepts movable emissive instances, and the next rptr_hip_refit re-places
 * the lights of every scene copy on that copy's stream (csrc/tlas_build.h rp_k_place_lights) when instances moved or a dynamic mesh
 * that carries lights got new vertices. Every scene copy then owns its light buffer, like its instance records. The call waits for the
 * frames in flight. Without registration nothing changes: the same refusals, the same launches.
 * Bin membership, clone counts and order stay as the host made them. Bins are chosen uniformly and a bin's lights by resampling on
 * their actual contribution, so the estimator stays unbiased under any motion; only how evenly the bins share the power -- the
 * variance -- can drift when emitters change size (non-rigid change). Re-equalise with a new set_scene when that matters.
 * rptr_hip_readback_lights: the master copy's light buffer (count == num_lights) after all pending work, a deferred refit included. */
typedef struct RptrLightSource { /* 48 bytes, one per entry of RptrSceneDesc.lights, same order */
    float v0[3], v1[3], v2[3];   /* object-space vertices as dequantized (dequantize.glsl:8-21) */
    uint32_t instance;           /* scene instance the triangle belongs to */
    uint32_t geometry;           /* global geometry index */
    uint32_t triangle;           /* triangle within that geometry (unrolled order) */
} RptrLightSource;
int rptr_hip_set_light_sources(rptr_hip_t *h, const RptrLightSource *sources, uint32_t count);
int rptr_hip_readback_lights(rptr_hip_t *h, RptrTriLightData *out, uint32_t count);

/* ---- skinned meshes: bones in, float positions and shading normals out on the device. The reference animates "with a compute shader
 * that writes the float vertex buffer" (render_vulkan.cpp:2834-2840) and ships the buffer, not the shader; this is that piece
 * (csrc/skin.h rp_k_skin): linear blend skinning with at most FOUR influences per vertex. The host sends 48 bytes per bone instead of 36
 * bytes per triangle, and the shading normals of the deformed mesh follow, which rptr_hip_update_vertices cannot make them do (it leaves
 * the oct-encoded vertex normals set_scene uploaded where they are; "recomputed normals" below is the remedy on that road).
 * rptr_hip_set_skin(h, geometry, vertices, num_vertices): after set_scene, on a geometry of a mesh flagged RPTR_MESH_DYNAMIC /
 * _SUBTLY_DYNAMIC. One RptrSkinVertex per UNROLLED vertex (three per triangle, the order of rptr_hip_update_vertices: a vertex shared
 * by several triangles is skinned once per corner), num_vertices == 3 * triangles. Binds the geometry: its REST POSE is its float
 * positions at the time of the call (a device copy), its rest normals are the normal halves of its qnrm_uv words as uploaded
 * (dequantize.glsl:23-41). Checked on the host before anything is queued: RPTR_E_INVALID for a NULL handle, a call before set_scene, a
 * geometry that is not dynamic, num_vertices != 3 * triangles, a bone index >= RPTR_MAX_BONES, weights that do not sum to 65535 -- the
 * message names the first offending vertex. (NULL, 0) unbinds: positions and normals stay as last written. A new set_scene drops every
 * binding and resets the bone table to identity. The call waits for the frames in flight.
 * rptr_hip_update_bones[_device](h, first_bone, count, transforms12): `count` row-major 3x4 matrices (the layout of
 * RptrInstanceDesc.transform) that map the mesh's rest object space to its posed object space, staged into rows [first_bone,
 * first_bone + count) of the handle's bone table: RPTR_MAX_BONES rows, identity after set_scene. The host form refuses a bad range, NULL
 * and a matrix that is not finite (RPTR_E_INVALID, nothing staged). The _device form reads DEVICE memory, ordered on the backend's
 * stream, no host synchronisation; it cannot report a bad matrix (see "rejected vertices").
 * rptr_hip_skin(h): for every bound geometry, one kernel on the backend's stream that writes the master copy's float positions and, for
 * a geometry with normals, its skinned normal words; then exactly what rptr_hip_update_vertices_device does per geometry. The host calls
 * rptr_hip_refit afterwards as always: refit or device rebuild, the scene copy of every frame context, registered light sources
 * (rptr_hip_set_light_sources: lights follow ONLY with registered sources, as for update_vertices) and object motion follow without
 * knowing that anything changed; the refit also writes the skinned normal words into the shading records (csrc/skin.h
 * rp_k_refit_normals -- launched only for meshes that have a skinned geometry with normals; the qnrm_uv stream itself, its uv halves and
 * the alpha test that reads them are untouched). No kernel of a frame changes. Nothing bound: RPTR_E_INVALID.
 * Arithmetic: binary32 throughout, every product and sum rounded on its own (no contraction), IEEE division.
 *   w_k     = float(weight[k]) / 65535.0f
 *   B[r][c] = ((w0 M0[r][c] + w1 M1[r][c]) + w2 M2[r][c]) + w3 M3[r][c]                 (a zero weight's bone is still read)
 *   p'[r]   = (B[r][0] x + B[r][1] y) + (B[r][2] z + B[r][3])                           (the placement rule of the moving lights)
 *   n'[r]   = (C[r][0] nx + C[r][1] ny) + C[r][2] nz, C the cofactor matrix of A = the 3x3 part of B: rows cross(A1, A2), cross(A2, A0),
 *             cross(A0, A1); n' is negated when det = A0 . C0 = (x x' + y y') + z z' is negative (a mirroring bone)
 *   word    = quantize_normal(n') (librender/quantize.h:21-35; it divides by the L1 norm: nothing is normalised first)
 * Identity bones reproduce the rest pose ONLY TO ROUNDING: the weights are rounded quotients, and so is their sum.
 * Rejected vertices: a vertex whose skinned position is not finite keeps the position and the normal it had and is counted:
 * rptr_hip_get_option(h, "skin_vertices_rejected") (read-only, since set_scene; reading it waits for the backend's stream). A normal
 * that is not finite or all zero keeps its previous word.
 * rptr_hip_readback_skinned: the master copy's current positions (3 floats per vertex) and normal words (one uint32 per vertex: the
 * normal half of a qnrm_uv word) of a bound geometry, after pending work; either pointer may be NULL. normal_words on a geometry without normals:
 * RPTR_E_INVALID. world_size > 1: every rank holds the whole scene, call on each. */
#define RPTR_MAX_BONES 4096
typedef struct RptrSkinVertex { /* 16 bytes, one per UNROLLED vertex: 3 per triangle, the order of rptr_hip_update_vertices */
    uint16_t bone[4];           /* rows of the handle's bone table, < RPTR_MAX_BONES */
    uint16_t weight[4];         /* unorm16, the four must sum to 65535; a zero weight's bone is still read */
} RptrSkinVertex;
int rptr_hip_set_skin(rptr_hip_t *h, uint32_t geometry, const RptrSkinVertex *vertices, uint32_t num_vertices);
int rptr_hip_update_bones(rptr_hip_t *h, uint32_t first_bone, uint32_t count, const float *transforms12);
int rptr_hip_update_bones_device(rptr_hip_t *h, uint32_t first_bone, uint32_t count, const float *device_transforms12);
int rptr_hip_skin(rptr_hip_t *h);
int rptr_hip_readback_skinned(rptr_hip_t *h, uint32_t geometry, float *xyz, uint32_t *normal_words, uint32_t num_vertices);

/* ---- morph targets (blend shapes): weights in, float positions and shading normals out on the device (csrc/morph.h rp_k_morph). The
 * other half of character animation: faces, corrective shapes, cloth and fluid caches played back as "keyframe minus rest" with a weight,
 * every glTF `targets` / `weights` pair. The morph stage sits IN FRONT of the skinner: it runs alone where a geometry has no skin, and
 * with a skin the morphed rest pose goes through exactly the operations of rp_k_skin. It shares the skinner's rest pose, output arrays,
 * rejection rule and everything downstream; no kernel of a frame or of the refit changes, and a scene that binds nothing launches and
 * allocates what it did.
 * rptr_hip_set_morph_targets(h, geometry, targets, num_targets): after set_scene, on a geometry of a mesh flagged RPTR_MESH_DYNAMIC /
 * _SUBTLY_DYNAMIC. Targets are SPARSE: a target lists only the vertices it moves and may have zero deltas; `vertex` is an UNROLLED
 * vertex (three per triangle, the order of rptr_hip_update_vertices: a vertex shared by several triangles has one delta per corner, the
 * convention of RptrSkinVertex). Checked on the host before anything is queued: RPTR_E_INVALID, nothing changed and a message that names
 * the first offending target and delta, for a NULL handle, a call before set_scene, a geometry that is not dynamic, num_targets >
 * RPTR_MAX_MORPH_TARGETS, a vertex >= 3 * triangles, a vertex that appears twice within one target, a delta component that is not
 * finite, a non-zero _pad, deltas == NULL with num_deltas != 0, and a total number of deltas that does not fit 32 bits. The library
 * transposes the targets once into a per-vertex list sorted by target (csrc/morph.h). (NULL, 0) unbinds: positions and normals stay as
 * last written. A new set_scene drops every binding. The call waits for the frames in flight. The weights of a newly bound geometry are
 * all zero.
 * Rest pose: ONE per geometry, shared by both deformers. A binding call (set_skin or set_morph_targets) captures it -- a device copy of
 * the float positions, and the normal halves of the uploaded qnrm_uv words -- only when the geometry has neither a skin nor morph targets
 * at that moment; on a geometry that already has the other deformer bound it reuses the captured one. (rptr_hip_set_skin on a geometry
 * without morph targets behaves as it always did: it captures.)
 * rptr_hip_update_morph_weights[_device](h, geometry, first_target, count, weights): `count` floats into rows [first_target,
 * first_target + count) of that geometry's weight table, on the backend's stream. The host form refuses a range beyond the geometry's
 * num_targets, NULL with count > 0, a geometry without targets and a weight that is not finite (RPTR_E_INVALID, nothing staged). The
 * _device form reads DEVICE memory, ordered on the backend's stream, and cannot see its values (see "rejected vertices"). Negative
 * weights and weights above 1 are legal.
 * rptr_hip_skin(h) stays the one call that runs the deformers: for every geometry that has a skin, morph targets or both it launches one
 * kernel (a skin without morph targets: rp_k_skin, exactly as before), then does what it always did. "Nothing bound" (RPTR_E_INVALID)
 * means neither deformer. rptr_hip_readback_skinned accepts a geometry bound by either.
 * Arithmetic: binary32, every product and sum rounded on its own. For vertex i, its entries are the deltas of all targets that name it,
 * in ASCENDING TARGET INDEX:
 *   p = rest_pos[i];  n = dequantize_normal(rest_word[i])                          (geometries with normals)
 *   for each entry (t, dpos, dnrm):  w = weight[t];  w == 0.0f: the entry is skipped
 *       p[c] = p[c] + w * dpos[c];   n[c] = n[c] + w * dnrm[c]                     (c = 0, 1, 2)
 *   no skin: p' = p, q = n; when no entry was applied the normal word written is rest_word[i] itself (no re-quantisation)
 *   skin:    B, p' = place(B, p), q = cof(A) n with the sign rule: the operations of "skinned meshes" on the morphed p and n
 *   word = quantize_normal(q) unless q is not finite or all zero (the previous word stays)
 * Without a skin, all-zero weights reproduce the rest pose BIT FOR BIT, positions and words; with a skin and zero weights the result is
 * bit for bit what rp_k_skin writes. The kernel always reads the rest pose, never its own output.
 * Rejected vertices: a vertex whose final position is not finite (a NaN weight from a device table) keeps its position and normal and is
 * counted in the existing read-only option "skin_vertices_rejected".
 * Lights follow only with registered sources, and bins are not re-equalised after non-rigid change (see "moving lights"). */
#define RPTR_MAX_MORPH_TARGETS 1024 /* per geometry */
typedef struct RptrMorphDelta { /* 32 bytes */
    uint32_t vertex;            /* UNROLLED vertex (3 per triangle, the order of rptr_hip_update_vertices) */
    float dpos[3];              /* added to the rest position, object space */
    float dnrm[3];              /* added to the rest normal (ignored for a geometry without normals) */
    uint32_t _pad;              /* zero */
} RptrMorphDelta;
typedef struct RptrMorphTargetDesc {
    const RptrMorphDelta *deltas;
    uint32_t num_deltas;
    uint32_t _pad;
} RptrMorphTargetDesc;
int rptr_hip_set_morph_targets(rptr_hip_t *h, uint32_t geometry, const RptrMorphTargetDesc *targets, uint32_t num_targets);
int rptr_hip_update_morph_weights(rptr_hip_t *h, uint32_t geometry, uint32_t first_target, uint32_t count, const float *weights);
int rptr_hip_update_morph_weights_device(rptr_hip_t *h, uint32_t geometry, uint32_t first_target, uint32_t count, const float *device_weights);

/* ---- recomputed normals: float positions in, shading normals out on the device (csrc/normals.h rp_k_face_normals, rp_k_group_normals).
 * rptr_hip_update_vertices[_device] replaces positions and leaves the normal words set_scene uploaded where they are: a cloth, fluid or
 * soft-body solver that writes the vertex buffer on the device is lit as if it were at rest. Morph targets without normal deltas leave
 * the same hole. This is the remedy: area-weighted smooth normals made from the positions as they are now, written into the array of
 * normal words the deformers write; the refit carries them on as it carries theirs. No kernel of a frame, of the refit, of rp_k_skin or
 * of rp_k_morph changes, and a scene that binds nothing launches and allocates what it did.
 * rptr_hip_set_normal_groups(h, geometry, group, num_vertices, flags): after set_scene, on a geometry of a mesh flagged RPTR_MESH_DYNAMIC
 * / _SUBTLY_DYNAMIC that has normals. Vertices are unrolled, so the library cannot know which corners are one smooth vertex: `group`
 * holds one value per UNROLLED vertex (three per triangle, the order of rptr_hip_update_vertices), num_vertices == 3 * triangles.
 * Corners with the same value share one normal -- a host passes the index buffer of the indexed mesh it unrolled (or welds with
 * host/normal_groups.hpp / scenes.normal_groups); RPTR_NORMAL_GROUP_FLAT gives a corner its own triangle's face normal. Values are
 * arbitrary 32-bit labels: the library renumbers them densely and transposes them once, on the host, into a per-group list of member
 * corners in ASCENDING UNROLLED VERTEX INDEX. The geometry's array of normal words is made if it has none (in the master and in every
 * frame context's scene copy, starting from the uploaded words). RPTR_E_INVALID, nothing changed and a message that names the offender,
 * for a NULL handle, a call before set_scene, a geometry that is not dynamic, a geometry without normals, num_vertices != 3 * triangles
 * and unknown flag bits. (NULL, 0, 0) unbinds: the normals stay as last written. A new set_scene drops every binding. The call waits
 * for the frames in flight.
 * rptr_hip_recompute_normals(h): for every bound geometry, two kernels on the backend's stream that read the master copy's CURRENT
 * float positions -- whatever update_vertices[_device] or rptr_hip_skin last wrote, ordered behind them on the stream -- and write its
 * normal words; then exactly what rptr_hip_update_vertices_device does per geometry, so the next rptr_hip_refit carries the words into
 * the shading records of every scene copy (refit or device rebuild, frames in flight, registered lights, object motion). Host order:
 * update_vertices* and / or rptr_hip_skin, then rptr_hip_recompute_normals, then rptr_hip_refit. On a geometry that also has a skin or
 * morph targets the recomputed words replace what rptr_hip_skin wrote: this is how morph targets without dnrm get correct normals.
 * Nothing bound: RPTR_E_INVALID. rptr_hip_readback_skinned accepts a geometry bound only by normal groups. world_size > 1: every rank
 * holds the whole scene, call on each.
 * Arithmetic: binary32, every product, difference and sum rounded on its own (no contraction), as for "skinned meshes".
 *   triangle t, corners p0 p1 p2 = positions[3t .. 3t+2]:
 *     e1 = p1 - p0,  e2 = p2 - p0
 *     f  = ( e1.y*e2.z - e1.z*e2.y,  e1.z*e2.x - e1.x*e2.z,  e1.x*e2.y - e1.y*e2.x )      (area-weighted, never normalised)
 *   corner i in group g with members c_0 < c_1 < ... :   n = f(c_0 / 3);  n = n + f(c_k / 3) for k = 1, 2, ...     (left to right)
 *   corner i with RPTR_NORMAL_GROUP_FLAT:                n = f(i / 3)
 *   RPTR_NORMALS_FLIP: n = -n
 *   word = quantize_normal(n), unless n is not finite or all zero: the corner keeps its previous word
 * Weighting is by AREA only; angle weighting is out of scope. A triangle that has two corners in one group contributes once per corner
 * (the rule above, not a special case). A zero-area triangle contributes zeros; a group made only of such triangles, a NaN or infinite
 * position and an overflowing product all fall under "keeps its previous word". Nothing is counted. */
#define RPTR_NORMAL_GROUP_FLAT 0xFFFFFFFFu
#define RPTR_NORMALS_FLIP 1u   /* the mesh is wound the other way: negate every recomputed normal */
int rptr_hip_set_normal_groups(rptr_hip_t *h, uint32_t geometry, const uint32_t *group, uint32_t num_vertices, uint32_t flags);
int rptr_hip_recompute_normals(rptr_hip_t *h);

/* ---- dynamic textures: new texels in, mip chain generated on the device (csrc/texture_mips.h rp_k_mip_level).
 * set_scene uploads every RptrTextureDesc once, and the sampler filters the levels the host supplied; until here nothing could write a
 * texel again (a video or procedural texture, a paint tool, a light-map baker needed a fresh set_scene and with it every BVH), and a
 * host with plain RGBA8 images had level 0 only. No frame kernel changes; a scene that never calls these functions allocates and
 * launches what it did. (RPTR_HIP_ABI_VERSION stays 5: new entry points, no layout changes.)
 * rptr_hip_update_texture(h, texture, rgba8, n_bytes, flags): after set_scene. rgba8 is LEVEL 0 ONLY, row 0 first, and n_bytes must be
 * 4 * width * height of the texture as set_scene received it: size and the srgb flag never change. With RPTR_TEXTURE_GENERATE_MIPS the
 * levels 1 .. full - 1 are made on the device from the new level 0 and the texture has the full chain down to 1 x 1; without it the
 * texture becomes level 0 only (rptr_hip_texture_levels says 1): a stale level is never sampled. (NULL, 0, RPTR_TEXTURE_GENERATE_MIPS)
 * keeps level 0 and generates the chain -- the call of a host that has no mip levels. The _device form reads DEVICE memory, ordered on
 * the backend's stream, without a host synchronisation behind the copy.
 * Storage: the first call that needs more room than set_scene allocated gets ONE allocation for the full chain; level 0 is copied
 * across on the device and the old block is released. Later calls reuse it: repeated updates neither allocate nor leak.
 * Ordering: textures are shared by every scene copy, so the call waits for the frames in flight (as rptr_hip_set_skin does), then
 * works on the backend's stream: the copy, one launch per level, and last the texture's record, patched in place. Every frame and every
 * query run submitted afterwards, on any frame context or caller's stream, is queued behind that stream's work and sees the new texels;
 * frames submitted before show the old ones. Double-buffered textures that would avoid the wait are out of scope.
 * RPTR_E_INVALID, nothing changed and a message that names the offender: a NULL handle; a call before set_scene; texture >=
 * num_textures; n_bytes other than 4 * width * height; unknown flag bits; NULL texels without the flag or with n_bytes != 0.
 * RPTR_E_UNSUPPORTED: a texture that any material with emission_intensity > 0 reads, through a textured parameter or its normal map
 * (decided once, in set_scene): RptrSceneDesc.lights carry radiance the host prepared from that texture, and next-event estimation would
 * silently disagree with what paths see -- the precedent of "moving lights". Alpha-tested textures are allowed (the test reads level
 * 0). world_size > 1: every rank holds the whole scene, call on each.
 * rptr_hip_readback_texture(h, texture, level, rgba8, n_bytes): one level as the device holds it, behind whatever was queued on the
 * backend's stream; n_bytes == 4 * that level's texels. A level beyond the current levels: RPTR_E_INVALID. rptr_hip_texture_levels: the
 * levels a sampler may read now. rptr_hip_srgb_decode_table (host only, no handle): the 256-entry table rp_srgb_decode_lut makes and
 * set_scene uploads, so that a host can restate the filter.
 * The filter -- the reference generates no mip levels, so this rule is the definition. Level l + 1 is made from the QUANTISED level l; a
 * source of h x w texels gives max(1, h >> 1) x max(1, w >> 1). Taps per axis of source size n at destination coordinate x, as
 * (source index, integer weight):
 *     n == 1                   (0, 1)                                          total 1
 *     n even                   (2x, 1), (2x + 1, 1)                            total 2
 *     n odd >= 3, m = n >> 1   (2x, m - x), (2x + 1, m), (2x + 2, x + 1)       total n   (the exact-area box: nothing dropped, nothing shifts)
 * Per channel, in binary32, every product, sum and quotient rounded on its own, IEEE division, no contraction (as "skinned meshes"):
 *     f(c) = srgb_decode_table[c] for the colour channels of an sRGB texture; float(c) for alpha and every channel of a linear texture
 *     acc = 0; for ty in row order, tx in column order: acc = acc + float(wx * wy) * f(texel[ty][tx])      (the integer product converted once)
 *     mean = acc / float(totx * toty)                                                                      (the integer product converted once)
 *     linear code: min(255, int(mean + 0.5f))
 *     sRGB code: the number of k in 1..255 with mean >= T[k], T[k] = (table[k - 1] + table[k]) * 0.5f
 * The thresholds are built on the host from the same table; the device evaluates no transcendental function, and the result is bit for
 * bit what tests/texture_mips_ref.py and scenes.generate_mips compute in numpy. On even sizes the linear path is (a + b + c + d + 2) >> 2. */
#define RPTR_TEXTURE_GENERATE_MIPS 1u
int rptr_hip_update_texture(rptr_hip_t *h, uint32_t texture, const uint8_t *rgba8, size_t n_bytes, uint32_t flags);
int rptr_hip_update_texture_device(rptr_hip_t *h, uint32_t texture, const uint8_t *device_rgba8, size_t n_bytes, uint32_t flags);
int rptr_hip_readback_texture(rptr_hip_t *h, uint32_t texture, uint32_t level, uint8_t *rgba8, size_t n_bytes);
int rptr_hip_texture_levels(const rptr_hip_t *h, uint32_t texture, uint32_t *out_levels);
void rptr_hip_srgb_decode_table(float out256[256]); /* host only: the table rp_srgb_decode_lut makes and set_scene uploads */

/* ---- RenderBackend::params / lighting_params / update_config
 * (render_backend.h:69-76, render_vulkan.cpp:2943-2959) */
int rptr_hip_set_params(rptr_hip_t *h, const RptrRenderParams *params,
                        const RptrSceneParams *scene_params,
                        const RptrLightSamplingConfig *lighting_params);

/* ---- begin_frame + draw_frame + end_frame for `spp` samples per pixel
 * (render_vulkan.cpp:1919-2178).  Equivalent to `spp` reference frames with
 * batch_spp = 1: sample_index = frame_id .. frame_id+spp-1, each folded into
 * the accumulation buffer by the running mean of process_samples.comp:116-132.
 * reset_accumulation != 0 -> frame_offset += frame_id; frame_id = 0
 * (render_vulkan.cpp:1937-1941).  count_traversal != 0 additionally counts BVH
 * node visits / triangle tests (slower; for roofline accounting only). */
int rptr_hip_render(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp,
                    int reset_accumulation, int count_traversal, RptrStats *out_stats);

/* Frames in flight (≙ the reference's swap-chain frames, `RenderStats.frame_stats_delay`,
 * librender/render_backend.h:15-24): rptr_hip_render_async queues a frame on the next free frame context and
 * returns; rptr_hip_wait blocks until that frame is done and returns its stats. A wavefront frame ends in a
 * latency-bound tail (late bounces carry few rays); with 2-3 frames in flight the tail of one frame overlaps the
 * head of the next. Resolves run in submission order into the one accumulation buffer; read-backs and
 * rptr_hip_copy_tile_to_device return the image of the frame that was waited for last. With frames_in_flight N,
 * at most N tickets can be outstanding (RPTR_E_INVALID otherwise); rptr_hip_render = async + wait, after waiting
 * for everything still in flight, and so do set_scene / update_vertices / refit / trace. */
int rptr_hip_render_async(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp, int reset_accumulation,
                          int count_traversal, uint64_t *out_ticket);
int rptr_hip_wait(rptr_hip_t *h, uint64_t ticket, RptrStats *out_stats);
/* Several frames in ONE launch sequence. A wavefront frame is a chain of dependent launches that each last at least as long as their
 * slowest ray; a small frame (the stripes of one rank of a multi-GPU split) cannot fill the GPU however many frames are in flight. Paths
 * are independent, so the samples of `n_frames` consecutive frames with the same camera and parameters can share the launches: sample
 * slots [k*spp, (k+1)*spp) belong to frame k, which keeps its own frame_offset / sample indices (reset_first: frame 0 restarts the
 * accumulation, reset_rest: so does every further frame -- begin_frame's rule per frame, render_vulkan.cpp:1937-1941), its own image
 * and its own ticket (out_tickets[0..n_frames)). Every frame is bit-identical to the same frame rendered on its own; the resolve folds
 * the frames into the accumulation in order. n_frames * spp sample slots must fit (options "max_batch_spp" /
 * "path_budget_mb": 16 by default), n_frames <= option "max_batch_frames" (8), frames_in_flight >= 2. rptr_hip_wait on any ticket of the batch waits for the batch;
 * read-backs, AOV read-backs (AOV images: of the batch's last frame) and rptr_hip_gather return / send the image of the ticket waited
 * for last; a frame context is free again when all of its batch's tickets have been waited for. RptrStats of a batched frame: an
 * equal share of the batch's times and counts. No reference counterpart (the reference renders one frame per submission). */
int rptr_hip_render_batch_async(rptr_hip_t *h, const RptrCamera *camera, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                                int count_traversal, uint64_t *out_tickets);
/* The same with a camera PER FRAME: cameras[0 .. n_frames) (n_frames <= 8). The reference's loop may move the camera every frame
 * (app.cpp:350-469, vulkan/render_vulkan.cpp:2880-2941: the view parameters are written per frame); primary rays, the texture footprint
 * and the position view of frame k use cameras[k], the AOV images (those of the last frame of the sequence) its view with the view of
 * frame n_frames - 2 as VP_reference. Every frame is bit-identical to the same frame submitted alone with its camera. (Camera rays of
 * such a sequence are made by the kernels' general instantiation -- the one that also serves table-driven point sets.) */
int rptr_hip_render_batch_cameras_async(rptr_hip_t *h, const RptrCamera *cameras, int variant, int spp, int n_frames, int reset_first, int reset_rest,
                                        int count_traversal, uint64_t *out_tickets);
/* RenderConfiguration::freeze_frame (librender/render_backend.h:39; vulkan/render_vulkan.cpp:1937-1941,2152-2154): while set, a reset
 * does not advance frame_offset and a rendered frame does not advance frame_id -- every frame repeats the same samples (the
 * reference's --freeze-frame, cmdline.cpp:359-360). */
int rptr_hip_set_freeze_frame(rptr_hip_t *h, int freeze_frame);
/* set_backend_options(rng_variant) + the upload of the point set's table (vulkan/pointsets/render_sobol.cpp:84-104, render_bn.cpp:78-126:
 * the buffer bound at RANDOM_NUMBERS_BIND_POINT). `table` = host pointer to SobolData / BNData bytes (sizes above; NULL and 0 for
 * UNIFORM); the library keeps a device copy. Frames in flight are waited for; accumulation is not reset (the caller resets, as
 * the reference does when backend options change). A table that is too short, or a variant outside 0..3, fails with RPTR_E_INVALID. */
int rptr_hip_set_rng_variant(rptr_hip_t *h, int rng_variant, const void *table, size_t table_bytes);
/* hipEvent pairs recorded per frame for RptrStats.*_time_ms: 0 none (render_time_ms only; the default since round 5 -- the reference's
 * RenderStats has nothing else), 1 around the closest-hit traversal launches (extend_time_ms), 2 every stage (~0.06 ms per 1080p frame
 * rendered alone). */
int rptr_hip_set_stage_timing(rptr_hip_t *h, int level);

/* ---- Options: how the library builds and schedules, beyond RptrCreateInfo. The reference expresses such intent per mesh and per backend
 * option (Mesh::Dynamic / SubtlyDynamic -> build flags, vulkan/render_vulkan.cpp:942-952; RenderBackendOptions, librender/render_params.glsl.h:
 * 56-93); here every such switch is a named integer. rptr_hip_set_option(h, key, value) changes one for a handle -- it takes effect at the
 * call named below -- and rptr_hip_set_option(NULL, key, value) changes the process default that new handles (and the handle-less
 * rptr_hip_build_bvh_host) start from. Unknown key or value out of range: RPTR_E_INVALID. rptr_hip_get_option reads the value in force.
 * Every option also has an environment variable (right column): the experimenter's override for A/B runs of an unmodified host. When it is set
 * (read once per handle, in rptr_hip_create) its value is in force and rptr_hip_set_option on that key is accepted and ignored. No other
 * environment variable is read by the library (besides RPTR_FRAMES_IN_FLIGHT, which overrides RptrCreateInfo.frames_in_flight, and the HIP
 * runtime's own GPU_MAX_HW_QUEUES, which it reads -- and writes only under RPTR_CREATE_SET_HW_QUEUES). A host that sets NOTHING gets the
 * configuration bench.py measures.
 *
 *   key                      default   takes effect      meaning                                                                   environment
 *   flatten                  -1        set_scene         -1 / 1: a static scene with >= 2 instances (no RPTR_MESH_DYNAMIC mesh) is   RPTR_FLATTEN
 *                                                        built as ONE world-space tree (~150 bytes per instanced triangle; 1.5 x
 *                                                        faster to trace than instance records; hits are found on the pre-transformed
 *                                                        triangles: t / u / v agree with the instance walk to rounding, not bit for
 *                                                        bit); 0: always two-level
 *   flatten_max_tris         1 << 26   set_scene         ... up to this many instanced triangles                                   RPTR_FLATTEN_MAX_TRIS
 *   bvh_builder              0         set_scene         0 auto, 1 host (binned SAH), 2 device (PLOC) for static trees             RPTR_BVH_BUILDER=auto|host|device
 *   device_build_min_tris    2 << 20   set_scene         auto: triangle sets of at least this size are built on the device        RPTR_DEVICE_BUILD_MIN_TRIS
 *   traverse_node_min /      -1        set_scene         scheduling thresholds of the traversal (rptr_hip_traversal_preset);       RPTR_TRAVERSE_PRESET=n,r
 *   traverse_refill_min                                  -1: chosen from the tree
 *   single_instance          1         set_scene         queries of scenes with one instance record start inside it               RPTR_NO_SINGLE_INSTANCE (set = 0)
 *   max_batch_frames         8         initialize        frames a launch sequence may hold (rptr_hip_render_batch_async)           RPTR_MAX_BATCH_FRAMES
 *   max_batch_spp            0         initialize        sample slots in flight per frame context; 0: min(16, what the budget      RPTR_MAX_BATCH_SPP
 *                                                        holds)
 *   path_budget_mb           6144      initialize        path state per frame context                                              RPTR_PATH_BUDGET_MB
 *   blocks_per_cu            0         initialize        persistent traversal blocks per CU; 0: occupancy for a frame alone on     RPTR_BLOCKS_PER_CU
 *                                                        the GPU, about 12 / n per CU for a frame submitted while n - 1 others
 *                                                        are in flight (n at most the hardware queues, GPU_MAX_HW_QUEUES)
 *   side_connect             -1        initialize        shadow rays of bounce b on a side stream beside the closest-hit rays of   RPTR_SIDE_CONNECT
 *                                                        b + 1; -1: with one frame context, and with two for a frame submitted
 *                                                        while no other is in flight (a synchronous loop); off with more
 *   aovs                     1         initialize        AOV images (rptr_hip_readback_aov)                                        RPTR_AOVS
 *   tail_bounce              -1        next frame        bounce from which ONE launch finishes the frame; -1 adaptive, 0 never     RPTR_TAIL_BOUNCE
 *   tail_threshold           65536     next frame        adaptive: queue length below which a bounce goes to that launch           RPTR_TAIL_THRESHOLD
 *   stage_timing             0         next frame        = rptr_hip_set_stage_timing                                               RPTR_STAGE_TIMING
 *   comm_transport           0         comm init         0 auto (RCCL between devices), 1 rccl, 2 copy, 3 peer writes              RPTR_COMM_TRANSPORT=rccl|copy|peer
 *   comm_priority            1         comm init         the communication stream has the highest stream priority                 RPTR_COMM_PRIORITY
 *   quiet                    0         -                 no notes on stderr                                                        RPTR_QUIET
 *   traverse_fetch           0         set_scene         queue entries a traversal wave takes per pool at most (multiple of 64);   RPTR_TRAVERSE_FETCH
 *                                                        0: chosen with the thresholds above (384, dense trees 256)
 *   fast_math                0         next frame        the shading stages' division / square root / normalize: 0 IEEE, correctly   RPTR_FAST_MATH
 *                                                        rounded -- the CPU oracle's operations, what every parity test runs on;
 *                                                        1 the hardware's 1-ulp v_rcp / v_sqrt / v_rsq (as a GLSL compiler would:
 *                                                        Vulkan asks 2.5 ulp of `/`): the reference's default renderer (glTF BSDF +
 *                                                        binned-RIS lights) 6.5 % faster per frame, whole frames within 2.3e-4 RMSE of
 *                                                        the oracle (IEEE: 1.4e-5; north_star's tolerance 1e-3), coverage and ray
 *                                                        counts unchanged; csrc/dmath.h. Traversal and camera rays are IEEE either way.
 *   taa                      0         next frame        RenderBackendOptions::enable_taa: with reprojection_mode 2, a TAA pass on     RPTR_TAA
 *                                                        the RGBA8 frame after the resolve (vulkan/processing/process_taa.comp:
 *                                                        Lanczos history r = 5, weight 0.15, trimmed neighbourhood box), from the
 *                                                        second frame after a reset on; render_upscale_factor 1 (see "Real-time
 *                                                        resolve" at RptrRenderParams)
 *   rptr_hip_option_count / rptr_hip_option_name enumerate these keys (22). Experiments that were measured and not adopted stay reachable for
 *   A/B runs under the key prefix "experimental." (and their environment variables), are not enumerated and carry no promise:
 *   experimental.rebraid, .tlas_collapse, .collapse, .presplit_density, .presplit_budget_pct, .host_ploc, .ploc_top, .ploc_leaf, .lds_top,
 *   .regroup_materials, .comm_self (profiles/r03_notes.md, r05_notes.md say what each lost by).
 *   Read-only through rptr_hip_get_option: "bvh_rebuild_failures" -- device-side rebuilds of dynamic meshes that could not start (no memory for
 *   their work space); such a mesh is refitted on its old topology, the frame is rendered, the next refit tries again; "sample_slots" -- the
 *   sample slots a frame context holds once rptr_hip_initialize has sized the path state ("max_batch_spp", or what "path_budget_mb" allows:
 *   16 up to ~2.9 Mpixel per rank, 12 at 1440p, 5 at 4K): a launch sequence of n frames of s samples needs n * s <= sample_slots. The
 *   persistent closest-hit grids, in blocks (0 before rptr_hip_initialize): "traversal_resident_blocks" -- the blocks that fit on the device
 *   at once; "traversal_grid_alone" -- the grid of a frame alone on the GPU; "traversal_grid_shared" -- that of a frame beside the most
 *   others that can run at once; "traversal_concurrency" -- that most, min(frame contexts, hardware queues); "traversal_stack_blocks" --
 *   the grid the stack scratch of a frame context holds; "last_traversal_grid" -- the first grid of the last submitted frame. */
int rptr_hip_set_option(rptr_hip_t *h, const char *key, int64_t value);
int rptr_hip_get_option(const rptr_hip_t *h, const char *key, int64_t *out_value);
int rptr_hip_option_count(void);
const char *rptr_hip_option_name(int index);

/* ---- RenderGraphic::get_framebuffer_size / readback_framebuffer
 * (util/display/render_graphic.h:26-37, render_vulkan.cpp:2256-2287).
 * The float read-back returns the RGBA32F accumulation buffer (what
 * --validation writes); rows owned by other ranks are left untouched.
 * Returns the number of floats a full frame needs in *out_count. */
int rptr_hip_get_framebuffer_size(const rptr_hip_t *h, uint32_t out_whc[3]);
int rptr_hip_readback_f32(rptr_hip_t *h, float *rgba, size_t n_floats);
int rptr_hip_readback_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes);
/* RenderGraphic::readback_aov (util/display/render_graphic.h:12-17,40; vulkan/render_vulkan.cpp:2290-2294): the RGBA16F AOV image
 * `aov_index` of the last finished frame, width*height*4 halfs (rows of other ranks stay untouched): 0 albedo.rgb + roughness
 * (1 when ior == 1), 1 shading normal + distance to the camera, 2 screen-space motion.xy + jitter.xy (motion of the hit point
 * between the previous frame's view and this one; no per-vertex motion, jitter 0). Written at bounce 0 by the first sample of a
 * frame (the reference lets every sample of the batch store to the pixel, vulkan/accumulate.glsl:76-103). Option "aovs" = 0 (before
 * rptr_hip_initialize) switches them off. */
#define RPTR_AOV_ALBEDO_ROUGHNESS 0
#define RPTR_AOV_NORMAL_DEPTH 1
#define RPTR_AOV_MOTION_JITTER 2
int rptr_hip_readback_aov(rptr_hip_t *h, int aov_index, uint16_t *rgba16f, size_t n_halfs);

/* ---- the denoiser: a spatial filter for the last finished frame (stands where the reference's hosts link Open Image Denoise:
 * enable_denoising, process_samples.comp's denoise_buffer). An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with the
 * weights and the variance guidance of SVGF's spatial part, run on albedo-demodulated colour and guided by the frame's own normal +
 * depth and albedo AOV images; csrc/denoise.h states every operation, tests/denoise_ref.py restates it in numpy, and the stored images
 * equal that restatement bit for bit. INTEGRATION.md "Denoiser" lists what a host can rely on.
 * The call is explicit and writes images of its own: it never touches the accumulation image, the RGBA8 frame, the AOV images, the
 * reprojection / TAA history, frame_id / frame_offset or the statistics; a frame rendered after it is bit-identical to one rendered without it,
 * and a host that never calls it launches nothing new. The source frame is the one the read-backs return: the frame waited for last (its
 * frame context's images when frames are in flight). The denoise call is asynchronous on the backend's stream; its images (72 bytes per pixel) are
 * allocated by the first call and freed with the handle's other frame-sized buffers. The RGBA8 image shows the denoised colour
 * through the render parameters in force at the call (exposure, early_tone_mapping_mode, sRGB; output_channel != 0: a copy of the
 * frame's RGBA8 image).
 * RPTR_E_INVALID: before a frame has finished; NULL or out-of-range parameters; reserved != 0; the frame's images are being overwritten by a
 * newer frame on the same frame context; the frame waited for last is not the last of its launch sequence (the AOV images are that
 * one's); a denoised read-back before any denoise call, or after a later frame finished or initialize ran (the image is stale).
 * RPTR_E_UNSUPPORTED: option "aovs" = 0; world_size > 1 (a stripe's taps lie in other ranks' rows); render_upscale_factor 2. */
typedef struct RptrDenoiseParams { /* 32 bytes */
    int32_t iterations;        /* 1..5: passes with tap spacing 1, 2, 4, 8, 16; default 5 */
    float sigma_luminance;     /* > 0, default 4 */
    float sigma_depth;         /* > 0, default 1 */
    int32_t normal_power_log2; /* 0..8, default 7: weight = max(0, n_p . n_q) ^ (2 ^ k) */
    int32_t demodulate_albedo; /* 0 / 1, default 1 */
    int32_t reserved[3];       /* must be 0 */
} RptrDenoiseParams;
void rptr_hip_denoise_defaults(RptrDenoiseParams *out);
int rptr_hip_denoise(rptr_hip_t *h, const RptrDenoiseParams *p);
int rptr_hip_readback_denoised_f32(rptr_hip_t *h, float *rgba, size_t n_floats);
int rptr_hip_readback_denoised_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes);

/* ---- the temporal denoiser: the denoiser above with the temporal half of SVGF in front of its passes. A call blends the frame's
 * demodulated colour and the two moments of its luminance with what the previous call left -- the history, fetched along the frame's
 * motion + jitter AOV with four bilinear taps that must agree with the pixel in normal and depth -- counts per pixel how many calls
 * the history is long, and hands the a-trous passes the variance of the blended signal in place of one frame's 3x3 estimate. The passes
 * and the finish are the denoiser's own. csrc/denoise_temporal.h states every operation, tests/denoise_temporal_ref.py restates it in
 * numpy, and the stored images equal that restatement bit for bit. INTEGRATION.md "Temporal denoiser" lists what a host can rely on.
 * The call is explicit, like rptr_hip_denoise, with the same source frame (the frame waited for last) and the same promises: it never
 * touches the accumulation image, the RGBA8 frame, the AOV images, the reprojection / TAA / upscaler histories, frame_id / frame_offset
 * or the statistics, and a host that never calls it launches nothing new. The result goes into the denoiser's output images:
 * rptr_hip_readback_denoised_f32 / _u8 return the result of whichever of the two denoise calls ran last, with their staleness rule.
 * History. The motion AOV describes the step from the previous FRAME's view to this one's, so the contract is one call per frame: a
 * host that skipped a frame sets reset_history. The library does not guess from frame_id. A call has no history -- and its images then
 * equal rptr_hip_denoise's with the same five leading parameters bit for bit -- in exactly these cases: it is the first one since
 * rptr_hip_initialize (which drops and frees the history, whatever the new size); reset_history is 1; demodulate_albedo differs from
 * the call that wrote the history (the stored colour would be in other units). An rptr_hip_denoise call between two temporal calls does
 * not disturb the history, which keeps its own copy of normal + depth.
 * Memory: two sets of history images, 80 bytes per pixel, on top of the denoiser's 72; allocated by the first call, freed with the
 * handle's other frame-sized buffers.
 * rptr_hip_denoise_temporal_defaults fills in the defaults below; rptr_hip_denoise_temporal(h, NULL) uses them.
 * rptr_hip_readback_denoise_history_f32: the history the last temporal call left, W x H x 4 floats, per pixel the blended demodulated
 * colour e' and the history length n' (1 = no history was found for the pixel, at most 255; all zero where the pixel is not surface).
 * RPTR_E_INVALID: NULL handle; before a frame has finished; a parameter out of range or not finite; reserved != 0; the frame's images
 * are being overwritten by a newer frame on the same frame context; the frame waited for last is not the last of its launch sequence;
 * a history read-back before any temporal call since initialize.
 * RPTR_E_UNSUPPORTED: option "aovs" = 0; world_size > 1; render_upscale_factor 2. */
typedef struct RptrDenoiseTemporalParams { /* 64 bytes */
    int32_t iterations;        /* as RptrDenoiseParams: 1..5, default 5 */
    float sigma_luminance;     /* > 0, default 4 */
    float sigma_depth;         /* > 0, default 1 */
    int32_t normal_power_log2; /* 0..8, default 7 */
    int32_t demodulate_albedo; /* 0 / 1, default 1 */
    float alpha_color;         /* (0, 1], default 0.2: least weight of the new frame's colour */
    float alpha_moments;       /* (0, 1], default 0.2: same for the two luminance moments */
    float normal_threshold;    /* [-1, 1], default 0.9: a history tap needs dot(N_p, N_q) >= this */
    float depth_tolerance;     /* >= 0, finite, default 0.1: ... and |z_q - z_p| <= depth_tolerance * z_p + gz_p */
    int32_t reset_history;     /* 0 / 1, default 0 */
    int32_t reserved[6];       /* must be 0 */
} RptrDenoiseTemporalParams;
void rptr_hip_denoise_temporal_defaults(RptrDenoiseTemporalParams *out);
int rptr_hip_denoise_temporal(rptr_hip_t *h, const RptrDenoiseTemporalParams *p /* NULL = defaults */);
int rptr_hip_readback_denoise_history_f32(rptr_hip_t *h, float *rgba, size_t n_floats);

/* ---- temporal upscaling: the TAA pass at twice the render resolution (vulkan/processing/process_taa.comp with render_upscale_factor = 2,
 * the way the reference's application renders at half the display resolution in each axis and lets the history fill in the sub-pixel
 * detail). For a handle initialized at W x H a call makes a 2W x 2H RGBA8 image from the last finished frame's RGBA8 image (every
 * rendered pixel stands for a 2x2 block of display pixels; the block is never stored), its motion + jitter AOV image and the previous
 * call's output, the history: per display pixel a 10 x 10 Lanczos window over the history whose taps lie two display pixels apart, then
 * the blend and the clamp to the 3x3 box of rendered pixels. csrc/taa_upscale.h states every operation, tests/taa_upscale_ref.py restates
 * it in numpy. INTEGRATION.md "Temporal upscaling" lists what a host can rely on.
 * The call is explicit and writes images of its own, like the denoiser: it never touches the accumulation image, the RGBA8 frame, the AOV
 * images, the reprojection / TAA history, frame_id / frame_offset or the statistics; a frame rendered after it is bit-identical to one
 * rendered without it, and a host that never calls it launches nothing new. It works in every reprojection_mode and whatever
 * render_upscale_factor and option "taa" are (the option's own pass stays at the render resolution and still refuses factor 2). The
 * source frame is the one the read-backs return: the frame waited for last. The call is asynchronous on the backend's stream; its two
 * display-size images (32 bytes per rendered pixel) are allocated by the first call and freed with the handle's other frame-sized
 * buffers.
 * History: the output of one call is the history of the next. A call has no history -- and its output is the plain 2x2 replication of
 * the frame, what the reference's history holds after its first frame -- when it is the first one since rptr_hip_initialize, or when
 * reset_history is 1. The library does not guess from frame_id: the host sets reset_history for the frame that restarted its
 * accumulation.
 * RptrTaaUpscaleParams: rptr_hip_taa_upscale_defaults fills in factor 2, reset_history 0, reserved 0; rptr_hip_taa_upscale(h, NULL) uses them.
 * rptr_hip_readback_upscaled_u8: the output of the last call, 2W x 2H x 4 bytes, row 0 at the top; waits for the call.
 * RPTR_E_INVALID: NULL handle; factor != 2; reset_history not 0 / 1; reserved != 0; before initialize or before a frame has finished;
 * the frame's images are being overwritten by a newer frame on the same frame context; the frame waited for last is not the last of its
 * launch sequence; a read-back before any call since initialize, or into fewer than 16 W H bytes.
 * RPTR_E_UNSUPPORTED: option "aovs" = 0; world_size > 1 (a stripe's taps lie in other ranks' rows). */
typedef struct RptrTaaUpscaleParams { /* 16 bytes */
    int32_t factor;        /* 2; anything else RPTR_E_INVALID */
    int32_t reset_history; /* 1: this call has no history: its output is the replicated frame */
    int32_t reserved[2];   /* must be 0 */
} RptrTaaUpscaleParams;
void rptr_hip_taa_upscale_defaults(RptrTaaUpscaleParams *out);
int rptr_hip_taa_upscale(rptr_hip_t *h, const RptrTaaUpscaleParams *p /* NULL = defaults */);
int rptr_hip_readback_upscaled_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes);

/* ---- auto-exposure: a metered display pass, the step from scene-referred radiance to a display image (stands where the reference's
 * application runs its "uber post" step, RenderProcessingStep::UberPost, whose source is not shipped; process_samples.comp exposes and
 * tone-maps only "if we don't have the uber post pass"). A call meters the last finished frame's accumulation image (source 0) or the
 * denoiser's float image (source 1: the result of whichever denoise call ran last) with a log-luminance histogram -- 256 bins, eight
 * per octave from 2^-16 up -- takes the mean log luminance between two percentiles, maps it to `key`, moves an exposure value ev
 * towards that target at speed_up / speed_down per second, and writes an RGBA8 image of its own: colour x 2^(exposure + ev), an optional
 * colour balance in LMS space, the tone map and sRGB of the denoiser's RGBA8 image. The ev lives on the device: no host round trip.
 * csrc/auto_exposure.h states every operation, tests/auto_exposure_ref.py restates it in numpy, and histogram, state and image equal
 * that restatement bit for bit. INTEGRATION.md "Auto-exposure" lists what a host can rely on.
 * The call is explicit and additive, like rptr_hip_denoise, with the same source frame (the frame waited for last): it never touches the
 * accumulation image, the RGBA8 frame, the AOV images, the denoiser's images and history, the upscaler's history, frame_id /
 * frame_offset or the statistics; a frame rendered after it is bit-identical to one rendered without it, and a host that never calls
 * it launches what it always launched. The call is asynchronous on the backend's stream; its buffers (4 bytes per pixel, 2 KB of
 * histogram and state) are allocated by the first call and freed by rptr_hip_initialize / rptr_hip_destroy, which also forget the ev.
 * mode 0 (manual): nothing is metered, the state is untouched, ev counts as 0 -- the image is the source through exposure, balance and
 * tone map. With source 1, gains of 1 and tone_mapping_mode = early_tone_mapping_mode it equals rptr_hip_readback_denoised_u8 byte for
 * byte. With output_channel != 0 the image is a copy of the frame's RGBA8 (an AOV view), nothing is metered and the state is untouched.
 * Defaults: speed_up 1, speed_down 3 per second. A falling EV is a brightening scene, and eyes adapt to brightening within a second or
 * so and to darkening far more slowly: the two rates keep that 3 : 1 order of the common eye-adaptation defaults.
 * rptr_hip_readback_exposed_u8: the image of the last call, W x H x 4 bytes; rptr_hip_readback_exposure_state: what the last mode-1 call
 * left. Both wait for the call.
 * RPTR_E_INVALID: NULL handle; a field outside the range its comment states, or not finite; reserved != 0; before initialize or before a
 * frame has finished, and whatever else rptr_hip_denoise refuses about the finished frame; source 1 when
 * rptr_hip_readback_denoised_f32 would be refused (no denoise call, or stale); a read-back of the image before any call since
 * initialize, after a later frame finished, or into fewer than 4 W H bytes; a state read-back (or NULL out) before any mode-1 call since
 * initialize. RPTR_E_UNSUPPORTED: option "aovs" = 0 with source 1 (source 0 needs no AOV image); world_size > 1;
 * render_upscale_factor 2. */
typedef struct RptrAutoExposureParams { /* 64 bytes */
    int32_t source;            /* 0: the frame's accumulation image; 1: the denoiser's float image (whichever denoise call ran last) */
    int32_t mode;              /* 1: meter and adapt; 0: manual -- nothing is metered, the state is untouched, ev counts as 0 */
    int32_t reset_history;     /* 1: no adaptation, ev jumps to this call's target */
    int32_t tone_mapping_mode; /* -1, 0: none; 1: neutral; 2: fast -- the values of early_tone_mapping_mode */
    float key;                 /* > 0; the luminance the metered mean is mapped to (0.18) */
    float low_percentile;      /* [0, 1) (0.5) */
    float high_percentile;     /* (low, 1] (0.95) */
    float min_ev, max_ev;      /* min <= max, finite (-8, 8) */
    float speed_up, speed_down;/* >= 0, per second: the rate when the target EV is above / below the current one (1, 3) */
    float dt;                  /* >= 0, seconds since the previous call; 0: jump to the target */
    float white_balance[3];    /* > 0, gains on L, M, S (1, 1, 1) */
    int32_t reserved;          /* must be 0 */
} RptrAutoExposureParams;
void rptr_hip_auto_exposure_defaults(RptrAutoExposureParams *out);
int rptr_hip_auto_exposure(rptr_hip_t *h, const RptrAutoExposureParams *p /* NULL = defaults */);
int rptr_hip_readback_exposed_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes);
typedef struct RptrExposureState { /* 32 + 1024 bytes */
    float ev, target_ev, mean_log2, scale; /* scale = what the display kernel multiplied by */
    uint32_t counted, black, ignored, calls;
    uint32_t histogram[256];
} RptrExposureState;
int rptr_hip_readback_exposure_state(rptr_hip_t *h, RptrExposureState *out);

/* ---- bloom: a glare pass between exposure and the display image. After exposure a light can be 10 or 10 000 times display white, and the
 * tone map clips all of them to the same patch; glare around it is the one cue of intensity an 8-bit image has. A call takes the part of
 * the EXPOSED linear image above `threshold` (soft knee, at most `clamp` per source texel: a firefly of 1e6 spreads no wider than an honest
 * highlight), filters it down a pyramid of L levels (each half the size, rounded up), adds the levels back up with `scatter` per step, and
 * writes an RGBA8 image of its own: exposed colour + gain x the upsampled pyramid, then auto-exposure's balance, tone map and sRGB. The
 * exposure scale is auto-exposure's: exposure_mode 1 reads the `scale` the last mode-1 rptr_hip_auto_exposure call left in the device
 * state ON THE DEVICE (call order per frame: rptr_hip_auto_exposure -> rptr_hip_bloom -> present; no host round trip), exposure_mode 0 is
 * its manual rule. csrc/bloom.h states every operation, tests/bloom_ref.py restates it in numpy, and every pyramid level and the image
 * equal that restatement bit for bit. INTEGRATION.md "Bloom" lists what a host can rely on.
 * Source frame, stream and asynchrony, refusals about the finished frame, and the output_channel != 0 rule (the image is a copy of the
 * frame's RGBA8, no pyramid is made, rptr_hip_bloom_levels gives 0) are rptr_hip_auto_exposure's. The call never touches the accumulation
 * image, the RGBA8 frame, the AOV images, the denoisers' images and histories, the upscaler's history, the exposure state, the exposed
 * image, frame_id / frame_offset or the statistics; a frame rendered after it is bit-identical to one rendered without it, and a host that
 * never calls it launches what it always launched. Its buffers (4 bytes per pixel for the image, two pyramids of about 16/3 bytes per
 * pixel each) are allocated by the first call and freed by rptr_hip_initialize / rptr_hip_destroy.
 * With intensity 0 the image equals rptr_hip_readback_exposed_u8 of the auto-exposure call with the corresponding mode and parameters.
 * The defaults are conventional starting values of real-time pipelines, not measurements of anything: tune them per scene.
 * rptr_hip_readback_bloomed_u8: the image of the last call, W x H x 4 bytes. rptr_hip_bloom_levels: L of the last call.
 * rptr_hip_readback_bloom_level_f32: level 1 .. L of the down pyramid d (which 0) or the up pyramid u (which 1) of the last call, w_l x h_l
 * float4 texels with w = 0 (w_0 x h_0 = W x H, w_l = (w_(l-1) + 1) / 2): for tests and for tuning. All three wait for the call.
 * RPTR_E_INVALID: NULL handle; a field outside the range its comment states, or not finite; reserved != 0; exposure_mode 1 when no mode-1
 * rptr_hip_auto_exposure call has run since initialize; whatever rptr_hip_auto_exposure refuses about the finished frame and the
 * denoised image; a read-back before any call since initialize, after a later frame finished, of a level outside 1 .. L, or into a
 * buffer that is too small. RPTR_E_UNSUPPORTED: as rptr_hip_auto_exposure (option "aovs" = 0 with source 1; world_size > 1;
 * render_upscale_factor 2). */
#define RPTR_BLOOM_MAX_LEVELS 12
typedef struct RptrBloomParams { /* 64 bytes */
    int32_t source;            /* 0: the frame's accumulation image; 1: the denoiser's float image -- as RptrAutoExposureParams.source */
    int32_t exposure_mode;     /* 0: scale = float(exp2(double(RptrRenderParams.exposure))), host-evaluated (auto-exposure's manual rule);
                                  1: the `scale` the last mode-1 rptr_hip_auto_exposure call left in the device state, read on the device */
    int32_t tone_mapping_mode; /* as RptrAutoExposureParams (-1) */
    int32_t levels;            /* 0: auto (the largest L <= 8 whose level is at least 2 texels on both axes); 1 .. RPTR_BLOOM_MAX_LEVELS: asked
                                  for, clamped to what the frame size allows */
    float threshold;           /* >= 0, display-linear units: 1 = display white before the tone map (1.0) */
    float knee;                /* >= 0, half-width of the soft threshold (0.5) */
    float clamp;               /* > 0: the most one source texel may contribute, the firefly bound (16) */
    float intensity;           /* >= 0 (0.2); 0: the image is auto-exposure's */
    float scatter;             /* [0, 1]: how much of each coarser level reaches the next finer one (0.7) */
    float white_balance[3];    /* as RptrAutoExposureParams (1, 1, 1) */
    int32_t reserved[4];       /* must be 0 */
} RptrBloomParams;
void rptr_hip_bloom_defaults(RptrBloomParams *out);
int rptr_hip_bloom(rptr_hip_t *h, const RptrBloomParams *p /* NULL = defaults */);
int rptr_hip_readback_bloomed_u8(rptr_hip_t *h, unsigned char *rgba, size_t n_bytes);
int rptr_hip_bloom_levels(const rptr_hip_t *h, uint32_t *out_levels);
int rptr_hip_readback_bloom_level_f32(rptr_hip_t *h, int which /* 0: d, 1: u */, uint32_t level /* 1 .. L */, float *rgba, size_t n_floats);

/* ---- object motion: a pass over a finished frame that rewrites the motion half of its motion + jitter AOV image where objects moved.
 * A frame projects the SAME world point through the previous and the current view (motion_vector = 0, as the reference): the AOV follows
 * the camera, not rptr_hip_update_instances / rptr_hip_update_vertices. rptr_hip_object_motion(h), called after the frame and before
 * its consumers (update_* -> refit -> render -> object_motion -> denoise_temporal / taa_upscale), replaces the .xy half of a texel with
 *   project(view_ref, x_prev) / max(w, 0) - project(view, x_cur) / max(w, 0)        (the frame's own formula when x_prev == x_cur)
 * where x_cur is the hit of the pixel's REPRESENTATIVE RAY and x_prev is where that surface point was in the previous frame: for a rigid
 * instance object_to_world_prev * (world_to_object_cur * x_cur); for a geometry whose positions were updated, the hit's barycentrics on
 * the triangle's previous positions, through the previous object_to_world. The representative ray is the frame's primary ray with the
 * pixel-filter draw replaced by its mean: through ((x + .5) / W, (y + .5) / H), plus half the frame's screen jitter under
 * enable_raster_taa, from the position of the frame's last camera, pinhole even with aperture_radius > 0. Under enable_raster_taa it is
 * exactly the ray whose hit the frame wrote into the AOV images; otherwise a ray through the same pixel. It is traced as ray queries are:
 * opaque geometry (alpha-tested cut-outs count as surfaces), interval (0, inf).
 * Only pixels whose hit lies on an instance whose object_to_world differs bitwise from the previous frame's, or on a geometry whose
 * positions were updated, are written: one 4-byte store of the .xy word. The jitter half, misses and hits on unmoved surfaces keep their
 * bits; the pass computes from the hit, so a second call stores the same bytes. It touches no other image, no frame_id / frame_offset,
 * no statistics; a host that never calls it launches what it always launched.
 * rptr_hip_track_object_motion(h, enable): after set_scene (a new set_scene drops it). Keeps the previous frame's state: 96 bytes per
 * instance and 36 bytes per triangle of the dynamic meshes, copied on the backend's stream by the first update_* call after a frame's
 * submission (transforms) and the first update_vertices* of a geometry in that interval (positions). "The state a frame sees" is what the
 * last rptr_hip_refit before its submission applied; the pass compares the last submitted frame N with frame N-1 (both submitted while
 * the tracking was on). Nothing staged between them, no frame N-1, or a launch sequence of several frames as the last submission
 * (objects cannot move inside one): the call succeeds, launches nothing and writes nothing.
 * The pass waits for the frames in flight, then runs on the backend's stream, asynchronously. rptr_hip_get_option(h,
 * "object_motion_pixels") (read-only; waits for the stream): the pixels the last call rewrote.
 * RPTR_E_INVALID: NULL handle; before set_scene; tracking not switched on; before initialize or before a frame has finished, and whatever
 * else the denoiser refuses about the finished frame; no frame submitted since the tracking was switched on; updates staged and not yet
 * refitted, or staged after frame N's submission (the tables no longer hold what frame N saw: call the pass before the next update_*);
 * frame N or N-1 was submitted while staged updates awaited a refit. RPTR_E_UNSUPPORTED: option "aovs" = 0; world_size > 1.
 * Limits: reprojection_mode = 2 and option "taa" resolve inside the frame and never see the rewritten image; lights' bins do not move. */
int rptr_hip_track_object_motion(rptr_hip_t *h, int enable);
int rptr_hip_object_motion(rptr_hip_t *h);

/* ---- multi-GPU: this rank's rows, packed top-to-bottom, for the RCCL gather.
 * rptr_hip_tile_rows writes up to `cap` (first_row,num_rows) pairs for `rank`
 * and returns the number of stripes; rptr_hip_copy_tile_to_device copies this
 * rank's packed rows (float4 per pixel) into a caller-owned DEVICE buffer on
 * the backend's stream. */
int rptr_hip_tile_rows(const rptr_hip_t *h, int rank, int32_t *first_and_count, int cap);
int rptr_hip_local_pixel_count(const rptr_hip_t *h, uint64_t *out_pixels);
int rptr_hip_copy_tile_to_device(rptr_hip_t *h, void *device_dst, size_t n_bytes);

/* ---- multi-GPU: the path's ONE collective, a gather of tile radiance to rank 0 over RCCL / xGMI (north_star; the
 * reference itself is single-GPU: vulkan/render_vulkan_extensions.cpp:77-82 picks one physical device). One communicator rank per
 * handle (RptrCreateInfo.rank / world_size). RCCL is loaded at run time (librccl.so.1, the copy already in the process if there is
 * one), so the library has no link-time dependency on it and single-GPU hosts never touch it.
 *
 *   one process per GPU:   rank 0: rptr_hip_comm_get_unique_id -> hand the 128 bytes to every rank (file, pipe, MPI, torch.distributed)
 *                          every rank: rptr_hip_comm_init_rank(h, id)            (collective: returns when all ranks have joined)
 *                          per frame:  rptr_hip_wait(h, ticket, ..); rptr_hip_gather(h);
 *   one process, n GPUs:   rptr_hip_comm_init_all(handles, n)                    (handles[i] must have rank i, world_size n)
 *                          per frame:  wait every handle's frame; rptr_hip_gather_all(handles, n);
 *
 * rptr_hip_gather sends the packed rows of the frame that was waited for last (the context's image itself: no staging copy) and, on
 * rank 0, receives every other rank's rows and assembles the full frame with one kernel. It is asynchronous: everything runs on
 * a communication stream of its own, ordered behind the waited frame; the next frame that reuses the sending frame context waits
 * for the send on the device, nothing else does -- with frames in flight the gather of frame i overlaps the rendering of frames
 * i+1.. . The assembled frame (rank 0) is read with rptr_hip_readback_gathered_f32 (which waits for the last gather) or used in
 * place through rptr_hip_gathered_frame (valid once rptr_hip_readback_gathered_f32 / rptr_hip_comm_stats have waited for it, or the device has been synchronised by the
 * caller). Rank 0 keeps TWO receive buffers and TWO assembled frames and uses them in turn: the frame of gather g stays intact while
 * gather g + 1 arrives and is assembled (a reader can hold frame i while i + 1 is in flight), and is rewritten by gather g + 2.
 * Handles that share a device (test rigs) and option "comm_transport" = 2 (copy) use peer-to-peer
 * copies (hipMemcpyPeerAsync) instead of RCCL in the one-process mode. "comm_transport" = 3 (peer; one-process mode, devices with peer
 * access): every rank writes its rows straight into their places in rank 0's frame from a kernel on its own communication stream --
 * rank 0 runs no receive kernels and no assembly pass (csrc/host_comm.h "Peer writes"). rptr_hip_comm_transport names what a handle's
 * communicator uses: "rccl", "copy" or "peer" (NULL without a communicator). */
#define RPTR_COMM_ID_BYTES 128
int rptr_hip_comm_get_unique_id(void *out_id128);
int rptr_hip_comm_init_rank(rptr_hip_t *h, const void *id128);
int rptr_hip_comm_init_all(rptr_hip_t *const *handles, int n);
int rptr_hip_comm_destroy(rptr_hip_t *h);
int rptr_hip_gather(rptr_hip_t *h);
int rptr_hip_gather_all(rptr_hip_t *const *handles, int n);
/* ONE collective for the frames of a launch sequence (rptr_hip_render_batch_async / _batch_cameras_async: they finish together and lie
 * behind each other in the frame context's images): call after waiting for the LAST ticket of the sequence; the last n_frames frames of
 * it (1 <= n_frames <= frames per launch sequence; every rank passes the same number) travel in one transfer per rank and are assembled
 * in one pass -- a quarter of the per-frame cost for sequences of four (csrc/host_comm.h "Batched gathers"). n_frames = 1 is
 * rptr_hip_gather. Rank 0 then holds n_frames assembled images: rptr_hip_gathered_frame / rptr_hip_readback_gathered_f32 show the last
 * one, rptr_hip_readback_gathered_frame_f32(h, k, ..) image k (0 = the oldest) of the last gather. */
int rptr_hip_gather_batch(rptr_hip_t *h, int n_frames);
int rptr_hip_gather_all_batch(rptr_hip_t *const *handles, int n, int n_frames);
int rptr_hip_gathered_frame(rptr_hip_t *h, const void **out_device_rgba32f);
int rptr_hip_readback_gathered_f32(rptr_hip_t *h, float *rgba, size_t n_floats);
int rptr_hip_readback_gathered_frame_f32(rptr_hip_t *h, int index, float *rgba, size_t n_floats);
/* gathers issued so far, and the mean GPU time of the completed ones on this rank's communication stream (send / receive + assembly) */
int rptr_hip_comm_stats(rptr_hip_t *h, uint64_t *out_gathers, float *out_mean_gather_ms);
const char *rptr_hip_comm_transport(rptr_hip_t *h);
/* Peer writes for ONE PROCESS PER GPU (opt-in; csrc/host_comm.h COMM_IPC): rank 0 calls rptr_hip_comm_ipc_export (which makes its
 * communicator and writes RPTR_COMM_IPC_BYTES describing its frame buffers: hipIpcGetMemHandle), the bytes reach every rank through any side
 * channel, every rank calls rptr_hip_comm_ipc_init(h, bytes) (rank 0 too: a check). rptr_hip_gather / _gather_batch then scatter every
 * rank's rows straight into rank 0's frame from a kernel on the rank's own communication stream -- no RCCL, no receive buffer, no
 * assembly pass; the ordering between the processes is carried by counters in a flag block of rank 0 (events do not cross processes).
 * Needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver only supports dmabuf IPC. rptr_hip_comm_transport says "ipc". */
#define RPTR_COMM_IPC_BYTES 256
int rptr_hip_comm_ipc_export(rptr_hip_t *h, void *out_bytes);
int rptr_hip_comm_ipc_init(rptr_hip_t *h, const void *bytes);

/* ---- enable_ray_queries / render_ray_queries with the RQ_CLOSEST kernel
 * (render_backend.h:101-102, vulkan/rt_intersect.comp:31-68): n queries ->
 * n x float4 (bary.x, bary.y, bits(instance_custom_index + geometry_index),
 * bits(primitive_index)); miss = (-1,-1,bits(-1),bits(-1)); mode_or_data < 0
 * leaves the result slot untouched. Host pointers. */
int rptr_hip_trace(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, float *out4);
/* The same over DEVICE buffers, asynchronously on `hip_stream` (NULL: the backend's stream) -- what RenderBackend::render_ray_queries works
 * on (vulkan/render_vulkan.cpp:1867-1876: the queries are in ray_query_buffer, written by other device code, the results go to
 * ray_result_buffer). A caller's stream is ordered behind the scene uploads queued on the backend's stream and the backend's later work
 * behind the queries. */
int rptr_hip_trace_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, float *device_out4, void *hip_stream);
/* RenderBackend::enable_ray_queries(max_queries, max_queries_per_pixel) (render_backend.h:101, render_vulkan.cpp:430-455): the library
 * owns a device buffer of max(max_queries, width x height x max_queries_per_pixel) RptrRenderRayQuery records and one of as many float4
 * results and returns their device addresses (≙ ray_query_buffer / ray_result_buffer; they stay valid until the next call that asks for
 * more, or rptr_hip_destroy). RenderBackend::render_ray_queries(num_queries, ...) with the RQ_CLOSEST program = rptr_hip_render_ray_queries:
 * traces the first num_queries records of that buffer on the backend's stream (with a path-tracing variant: rptr_hip_render_radiance_queries
 * below). */
int rptr_hip_enable_ray_queries(rptr_hip_t *h, int max_queries, int max_queries_per_pixel, void **out_device_queries, void **out_device_results);
int rptr_hip_render_ray_queries(rptr_hip_t *h, int num_queries);
/* ---- render_ray_queries with a path-tracing variant: radiance along the query rays
 * (RenderBackend::render_ray_queries(num_queries, params, variant_idx) with a megakernel variant: pt_megakernel.glsl:276-302, 327-334
 * ENABLE_RAYQUERIES, accumulate.glsl:31-42, render_vulkan.cpp:2961-3059). For query q and sample s < samples_per_query the path tracer's
 * main_spp runs with its first ray replaced by the record's (origin, dir as given, t_min 0, t_max); out4[q] = (radiance.rgb, alpha) is what
 * a frame's pixel is: bounces, next-event estimation, Russian roulette, alpha test, emitters, the sky on a miss (also when t_max ends the
 * first ray before a surface; alpha is then 0). `variant` is an RPTR_VARIANT_* gpu program, `camera` supplies the image-plane axes the
 * texture footprint is made from (pt_megakernel.glsl:341-352 uses the view's for queries too), RenderParams / SceneParams / lights are the
 * handle's. Where the reference leaves things open this ABI pins them:
 *   1. Random numbers: query q is pixel (q mod W, q div W) of a virtual image as wide as the handle's frame (W) and as tall as needed, so
 *      the hashed pixel id px + py * W is q and table point sets get a 2-D pixel; the generator is opened as for that pixel and the
 *      pixel-filter draw is made and dropped, so a query that IS a camera ray sees the stream the pixel's path sees. sample_index =
 *      first_sample + s, frame_offset = the handle's current one (what the next rptr_hip_render without a reset would use), and the
 *      view's frame_id of sample s = its sample_index (a one-sample frame at that point of the accumulation). The reference always
 *      starts at sample 0; first_sample lets a host refine the same probes over several calls.
 *   2. The result is the running mean in sample order, r += (new - r) / (sample_index + 1), a plain store for sample_index 0; for
 *      first_sample > 0 the old mean is read from the result slot. (accumulate_query as written adds the new mean onto the old value
 *      for sample_index > 0 and lets the samples of a dispatch race on the slot.) k calls of one sample == one call of k samples, bit
 *      for bit; so is any split of the queries over calls with the same indices.
 *   3. mode_or_data < 0 leaves the result slot untouched (as rptr_hip_trace; the megakernel does not read the field).
 * A run waits for the frames in flight, writes no AOV image and leaves the accumulation, the frame buffer, frame_id / frame_offset, the
 * reprojection history and rptr_hip_stats alone. n may exceed width x height. world_size > 1: RPTR_E_UNSUPPORTED (queries are not striped
 * over the ranks). Before set_scene / initialize, unknown variant, samples_per_query < 1, first_sample < 0, NULL camera: RPTR_E_INVALID.
 *
 * rptr_hip_trace_radiance: host arrays, synchronous; out4 is read as well as written (slots of skipped queries, old means); out_stats (may
 * be NULL) gets rays_closest / rays_shadow / hits_shaded of the run, spp = first_sample + samples_per_query, times 0.
 * rptr_hip_trace_radiance_device: DEVICE buffers, asynchronously on `hip_stream` (NULL: the backend's stream), ordered as rptr_hip_trace_device.
 * rptr_hip_render_radiance_queries: over the first num_queries records of the buffers of rptr_hip_enable_ray_queries, on the backend's stream
 * (more than the budget: RPTR_E_INVALID). */
int rptr_hip_trace_radiance(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrCamera *camera, int variant, int samples_per_query,
                            int first_sample, float *out4, RptrStats *out_stats);
int rptr_hip_trace_radiance_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, const RptrCamera *camera, int variant,
                                   int samples_per_query, int first_sample, float *device_out4, void *hip_stream);
int rptr_hip_render_radiance_queries(rptr_hip_t *h, int num_queries, const RptrCamera *camera, int variant, int samples_per_query, int first_sample);
/* ---- surface queries: position, normals and material at a query ray's closest hit
 * What lies between rptr_hip_trace (barycentrics and indices) and rptr_hip_trace_radiance (radiance): the surface the ray hit, decoded by
 * the device functions the first shade of a frame uses for its AOV images. The reference's registry declares a GBUFFER computational
 * raytracer beside RQ_CLOSEST (rendering/gpu_programs.cmake:47) and ships no source for it; this is that program for query rays.
 * One record of 96 bytes per query: six rows of 16 bytes. For query (origin, dir, t_max) the direction is used as given, the interval is
 * (0, t_max) as for radiance queries, and w_o = -dir:
 *   t, position      the closest hit and origin + t * dir, geometric. (The megakernel's VOLUME back-face rule, which moves its interaction
 *                    point to the ray origin, does NOT apply here.)
 *   geo_normal, normal   gn and nn of the megakernel's first hit as the normal + depth AOV holds them for a camera ray: hit attributes,
 *                    normalised geometric normal, the flip towards the ray for two-sided materials (pt_megakernel.glsl:624-633), the normal
 *                    map at LOD 0 (:634-654), the w_o correction (:656-668).
 *   instance_geometry, primitive   the two index words of rptr_hip_trace (instance custom index + geometry index; primitive index)
 *   base_color, roughness, ior, metallic, emission   the hit's material unpacked by gpu program `variant` (RPTR_VARIANT_*) at the hit's
 *                    texture coordinate, whose footprint is the camera-derived first-hit footprint of radiance queries (`camera`'s
 *                    image-plane axes, the handle's frame size, RenderParams.pixel_radius; pt_megakernel.glsl:341-352). base_color is 0 on
 *                    emitters, as in the albedo AOV; emission is the emitter's radiance. RPTR_VARIANT_SIMPLE: roughness 1, ior 1, metallic 0.
 *   uv, material_id  the interpolated texture coordinate and the index into RptrSceneDesc.materials the shade would load
 * A miss (also when t_max ends the ray first): t = -1, both indices and material_id -1, roughness 1, ior 1, every other float 0 (the miss
 * texel of the albedo + roughness AOV). mode_or_data < 0 leaves the record untouched. Alpha-tested geometry is opaque to these queries, as
 * it is to rptr_hip_trace. */
typedef struct RptrSurfaceHit {
    float position[3];
    float t;
    float geo_normal[3];
    int32_t instance_geometry;
    float normal[3];
    int32_t primitive;
    float base_color[3];
    float roughness;
    float emission[3];
    float ior;
    float uv[2];
    int32_t material_id;
    float metallic;
} RptrSurfaceHit;
/* rptr_hip_trace_surface: host arrays, synchronous; `out` is read as well as written (the slots of skipped queries are preserved).
 * rptr_hip_trace_surface_device: DEVICE buffers, asynchronously on `hip_stream` (NULL: the backend's stream), ordered as
 * rptr_hip_trace_device; device_queries == NULL: the query buffer of rptr_hip_enable_ray_queries (more than its budget: RPTR_E_INVALID).
 * Both trace the scene copy rptr_hip_trace traces (after update_vertices / update_instances and rptr_hip_refit: the moved geometry), wait
 * for the frames in flight and leave the accumulation and frame buffers, the AOV images, frame_id / frame_offset, the reprojection history,
 * the denoised images and rptr_hip_stats alone. world_size > 1: RPTR_E_UNSUPPORTED. NULL camera, query or output pointer, n < 0, unknown
 * variant, before set_scene / initialize: RPTR_E_INVALID (the argument checks come before the device is touched). */
int rptr_hip_trace_surface(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrCamera *camera, int variant, RptrSurfaceHit *out);
int rptr_hip_trace_surface_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries, int n, const RptrCamera *camera, int variant,
                                  RptrSurfaceHit *device_out, void *hip_stream);
/* ---- occlusion queries: is anything between these two points? One bit per query
 * The any-hit query of line-of-sight, shadow, visibility and ambient-occlusion probes and of light baking: the traversal of a frame's
 * shadow rays (it stops at the first accepted hit) over query records, with the result packed 32 queries to a word. No reference
 * counterpart: the reference's registry has the closest-hit program RQ_CLOSEST only.
 *   Interval   query q is occluded when some triangle of the scene intersects its ray in (t_min, t_max), t_min = RPTR_RAY_EPSILON *
 *              |origin| (the RQ_CLOSEST rule of rptr_hip_trace), `dir` used as given: a point-to-point test from a to b is origin = a,
 *              dir = b - a, t_max = 1.
 *   Result     bit (q & 31) of word (q >> 5) of out_bits, 1 = occluded; the buffer holds ceil(n / 32) words. A query with
 *              mode_or_data < 0 leaves its bit as the caller had it (the convention of every other kind), and so do the bits >= n of
 *              the last word: the host form uploads out_bits as well as downloading it, the device form merges into the words it finds.
 *   Opaque     flags == 0: every triangle occludes, alpha-tested geometry included, as for rptr_hip_trace. The answer equals
 *              out4[4*q] != 0 of rptr_hip_trace_counted with tmin = NULL and any_hit = 1.
 *   Cutout     RPTR_OCCLUSION_ALPHA_CUTOUT: a candidate hit is ignored when its material lacks RPTR_BASE_MATERIAL_NOALPHA and its alpha is
 *              < alpha_cutoff. The alpha is the one a frame's alpha test compares: level 0 of the base-colour texture at the candidate's
 *              interpolated uv, 1 for a literal colour. Deterministic: no random number is drawn (a frame's test is stochastic for
 *              fractional alpha), so the same query gives the same bit in every run, and raising the cutoff never occludes a clear ray.
 * Both forms trace the scene copy rptr_hip_trace traces (after update_vertices / update_instances and rptr_hip_refit: the moved geometry),
 * wait for the frames in flight and leave the accumulation, frame and AOV images, frame_id / frame_offset, the histories, the denoised
 * images and rptr_hip_stats alone. world_size > 1 is allowed, as for rptr_hip_trace: every rank holds the whole scene.
 * rptr_hip_occlusion_defaults: flags 0, alpha_cutoff 0.5, reserved 0.
 * rptr_hip_trace_occlusion: host arrays, synchronous. params NULL = the defaults.
 * rptr_hip_trace_occlusion_device: DEVICE buffers, asynchronously on `hip_stream` (NULL: the backend's stream), ordered as
 * rptr_hip_trace_device; device_queries == NULL: the query buffer of rptr_hip_enable_ray_queries (more than its budget: RPTR_E_INVALID).
 * NULL handle, NULL query or result pointer with n > 0, n < 0, reserved != 0, unknown flag bits, with the cutout flag a cutoff that is not
 * finite or outside (0, 1], before set_scene / initialize: RPTR_E_INVALID (the argument checks come before the device is touched).
 * n == 0 succeeds and touches nothing. */
#define RPTR_OCCLUSION_ALPHA_CUTOUT 1u
typedef struct RptrOcclusionParams { /* 16 bytes */
    uint32_t flags;       /* RPTR_OCCLUSION_*; 0: every triangle is opaque, as for rptr_hip_trace */
    float alpha_cutoff;   /* read with ALPHA_CUTOUT only: 0 < cutoff <= 1, finite; default 0.5 */
    uint32_t reserved[2]; /* must be 0 */
} RptrOcclusionParams;
void rptr_hip_occlusion_defaults(RptrOcclusionParams *out);
int rptr_hip_trace_occlusion(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, const RptrOcclusionParams *params /* NULL = defaults */,
                             uint32_t *out_bits);
int rptr_hip_trace_occlusion_device(rptr_hip_t *h, const RptrRenderRayQuery *device_queries /* NULL: the buffer of rptr_hip_enable_ray_queries */,
                                    int n, const RptrOcclusionParams *params, uint32_t *device_out_bits, void *hip_stream);
/* ---- irradiance probes: positions in, second-order spherical-harmonics coefficients of the incident radiance out
 * The step from rays to a probe (a DDGI-style grid, a light-probe baker, irradiance for particles and volumetrics): a ray-generation
 * kernel, a radiance-query run and a projection kernel, with nothing but 144 bytes per probe leaving the device. No reference counterpart.
 * The arithmetic is binary32, every product and sum rounded on its own (no contraction), IEEE division; tests/probes_ref.py restates it.
 *   Directions  rptr_hip_probe_directions(K, out): the spherical Fibonacci set, on the host in double, each component rounded to float
 *               once: g = (sqrt 5 - 1) / 2, z = 1 - (2k + 1) / K, phi = 2 pi frac(k g), r = sqrt(max(0, 1 - z z)), d_k = (r cos phi,
 *               r sin phi, z). The device evaluates no transcendental function: the table is uploaded once per K and kept in the handle.
 *   Rays        ray q = p K + k of a run: origin = the probe's position, dir[r] = (R[r][0] x + R[r][1] y) + R[r][2] z of d_k = (x, y, z)
 *               with R = `rotation` (row-major), NOT renormalised (queries use dir as given), t_max from the params, mode_or_data = 0.
 *               A probe with a coordinate that is not finite is skipped: its K records get mode_or_data = -1 (origin, dir and t_max are
 *               written as for any probe), its 36 coefficients keep every byte, nothing is traced or counted for it.
 *   Runs        the probes are processed in runs of max(1, floor(R / K)) whole probes, R = max_run_rays or 1 << 22; ray p_local K + k is
 *               query q of the run's radiance queries (rptr_hip_trace_radiance rule 1), so a probe's random numbers depend on its index
 *               within its run, and a call over exactly the probes of one run gives that run's bits.
 *   Samples     the run's samples have random-number indices sample_index ... sample_index + samples_per_ray - 1, and frame_id
 *               likewise, as radiance queries pin it; the fold counts from 0: a ray's value is the running mean (rule 2) of THIS run's
 *               samples alone, whatever sample_index is -- a fresh estimate per call, as per-frame rotated ray sets need.
 *   Values      a ray whose float4 has a component that is not finite contributes (0, 0, 0, 0). clamp > 0 and m = max(r, g, b) > clamp:
 *               rgb = rgb (clamp / m); alpha is never scaled.
 *   Basis       from the rotated float direction (x, y, z), in this order: Y0 = 0.282095f, Y1 = 0.488603f y, Y2 = 0.488603f z,
 *               Y3 = 0.488603f x, Y4 = 1.092548f (x y), Y5 = 1.092548f (y z), Y6 = 0.315392f (3 (z z) - 1), Y7 = 1.092548f (x z),
 *               Y8 = 0.546274f (x x - y y).
 *   Sum         one 64-lane wavefront per probe: lane l starts from +0 and takes k = l, l + 64, ... in ascending order, per step
 *               acc[i][ch] = acc[i][ch] + v[ch] Y_i; then acc = acc + xor-shuffle(acc, off) for off = 32, 16, 8, 4, 2, 1 (IEEE addition
 *               commutes: every lane ends with the same bits); c_new = acc w, w = float(4 pi / K) from double.
 *   Blend       blend == 1: a plain store (garbage or NaN in the buffer never survives); otherwise c = c + (c_new - c) blend.
 *   Layout      coeffs[p][i][ch]: 36 floats, 144 bytes per probe, channels r, g, b, alpha. Alpha is 1 where the first ray hit a surface, so
 *               its coefficients are the SH visibility of geometry against the sky.
 * rptr_hip_probe_defaults: K 128, one sample per ray, sample_index 0, identity rotation, blend 1, clamp 0, t_max 1e20, everything else 0.
 * rptr_hip_probe_directions: host only, no handle; K outside 1 .. RPTR_PROBE_MAX_RAYS or out3K == NULL: RPTR_E_INVALID.
 * The two stages are public on purpose, on DEVICE buffers, asynchronously on `hip_stream` (NULL: the backend's stream; a caller's stream
 * is ordered as for rptr_hip_trace_device). They need a handle and neither a scene nor a frame size, wait for nothing and touch nothing
 * a frame owns:
 *   rptr_hip_probe_rays_device     n_probes K records of 32 bytes (n_probes K < 2^31), for any query kind: closest hits for DDGI
 *                                  visibility, occlusion for AO.
 *   rptr_hip_probe_project_device  any n_probes K float4 -> coefficients. It reads 16 bytes per ray and recomputes the directions from
 *                                  the table, not the records. device_positions3 exists only so that the stage skips the probes the ray
 *                                  stage skipped; NULL: none is skipped.
 * rptr_hip_trace_probes: host arrays, synchronous; coeffs36 is read as well as written (skipped probes, blend < 1); out_stats (may be NULL)
 * gets rays_closest / rays_shadow / hits_shaded of the call, spp = samples_per_ray, times 0.
 * rptr_hip_trace_probes_device: DEVICE buffers, asynchronously on `hip_stream`, ordered as rptr_hip_trace_device.
 * Both are rays -> radiance run -> projection per run, in scratch the handle owns: 48 bytes per ray of a run (record + value), grown to
 * the largest run seen and freed by rptr_hip_destroy; a host that never calls them allocates nothing. `camera` and `variant` mean what
 * they mean for radiance queries (the camera only supplies the texture-footprint axes). Ordering and isolation are those of
 * rptr_hip_trace_radiance: the frames in flight are waited for; the accumulation, frame and AOV images, frame_id / frame_offset, the
 * histories, the denoised images and rptr_hip_stats are left alone; the scene copy is the one rptr_hip_trace traces. world_size > 1:
 * RPTR_E_UNSUPPORTED.
 * rptr_hip_readback_probe_rays (diagnostic, synchronous): the first n_rays ray values of the LAST run of the last rptr_hip_trace_probes
 * [_device], as the radiance run left them (before the sanitising and the clamp); the rays of a skipped probe read 0. More than that
 * run had, or no run yet: RPTR_E_INVALID.
 * RPTR_E_INVALID, checked before the device is touched, with a message that names the offender: NULL handle; NULL position or coefficient
 * (record, value) buffer with n_probes > 0; a whole call before set_scene / initialize; rays_per_probe outside 1 .. RPTR_PROBE_MAX_RAYS;
 * samples_per_ray < 1; sample_index < 0 or sample_index + samples_per_ray > INT32_MAX; flags or reserved != 0; blend outside (0, 1] or
 * not finite; clamp negative or not finite; t_max not > 0; a rotation that is not finite or whose R R^T (in double) differs from the
 * identity by more than 1e-3 in any entry. params NULL = the defaults. n_probes == 0 succeeds and touches nothing. */
#define RPTR_PROBE_MAX_RAYS 4096u
typedef struct RptrProbeParams { /* 80 bytes */
    uint32_t rays_per_probe;  /* K, 1 .. RPTR_PROBE_MAX_RAYS; default 128 */
    uint32_t samples_per_ray; /* m >= 1; default 1 */
    int32_t sample_index;     /* >= 0: random-number sample index of the run's first sample; default 0 */
    uint32_t flags;           /* must be 0 */
    float rotation[9];        /* row-major 3x3 applied to the direction set; default identity */
    float blend;              /* weight of the new coefficients, (0, 1]; default 1 = replace */
    float clamp;              /* 0 = none; > 0, finite: a ray's rgb is scaled so that its largest component is <= clamp */
    float t_max;              /* > 0; default 1e20f */
    uint32_t max_run_rays;    /* 0 = 1 << 22 */
    uint32_t reserved[3];     /* must be 0 */
} RptrProbeParams;
void rptr_hip_probe_defaults(RptrProbeParams *out);
int rptr_hip_probe_directions(uint32_t K, float *out3K);
int rptr_hip_probe_rays_device(rptr_hip_t *h, const float *device_positions3, uint32_t n_probes, const RptrProbeParams *params /* NULL = defaults */,
                               RptrRenderRayQuery *device_queries, void *hip_stream);
int rptr_hip_probe_project_device(rptr_hip_t *h, const float *device_values4, uint32_t n_probes, const float *device_positions3 /* may be NULL */,
                                  const RptrProbeParams *params, float *device_coeffs36, void *hip_stream);
int rptr_hip_trace_probes(rptr_hip_t *h, const float *positions3, uint32_t n_probes, const RptrCamera *camera, int variant,
                          const RptrProbeParams *params, float *coeffs36, RptrStats *out_stats);
int rptr_hip_trace_probes_device(rptr_hip_t *h, const float *device_positions3, uint32_t n_probes, const RptrCamera *camera, int variant,
                                 const RptrProbeParams *params, float *device_coeffs36, void *hip_stream);
int rptr_hip_readback_probe_rays(rptr_hip_t *h, float *out4, size_t n_rays);
/* RenderBackendOptions::light_sampling_variant (rendering/mc/light_sampling.h:11-20, rendering/mc/nee.glsl:12-14): 0 =
 * LIGHT_SAMPLING_VARIANT_NONE disables next-event estimation towards the emissive triangles (every NEE sample goes to the sun; emitters
 * that a path HITS still contribute, at full weight), 1 = LIGHT_SAMPLING_VARIANT_RIS (the default: binned RIS). The image is that of
 * the scene handed over without its light array and with sun_radiance.w = 1 (tested bit for bit); the lights stay uploaded and come back
 * with variant 1. */
int rptr_hip_set_light_sampling_variant(rptr_hip_t *h, int variant);
/* diagnostic twin: also returns, per query, the node and triangle visits of the traversal
 * (visits2[2*i], visits2[2*i+1]; may be NULL) -- the counts behind the roofline's algorithmic bytes,
 * checked ray by ray against the oracle walking the exported tree. tmin (NULL = the RQ_CLOSEST rule
 * eps*|origin|) gives explicit interval starts; any_hit != 0 runs the occlusion traversal of the
 * shadow rays instead (out4[4*i] = 1 if anything is hit in (tmin, t_max)). No reference counterpart. */
int rptr_hip_trace_counted(rptr_hip_t *h, const RptrRenderRayQuery *queries, int n, float *out4, uint32_t *visits2,
                           const float *tmin, int any_hit);

/* ---- test/diagnostic access to the acceleration structure (node format in
 * DESIGN.md): copies out the flattened BVH so the oracle can traverse the very
 * same tree and count the very same node visits. Pass NULL buffers to query
 * sizes. */
int rptr_hip_export_bvh(rptr_hip_t *h, void *nodes, size_t *n_nodes, void *tris, size_t *n_tris,
                        void *instances, size_t *n_instances);

/* ---- the host half of set_scene on its own: builds the same acceleration structure (binned SAH per mesh, top
 * level over the instance bounds, 4-wide collapse, 64-byte encoding) WITHOUT a device or a handle. Two calls like
 * rptr_hip_export_bvh (NULL buffers to query sizes). out_stack_need: worst-case traversal stack entries of the tree.
 * Test/diagnostic entry: the CPU test suite walks this tree with the oracle. */
int rptr_hip_build_bvh_host(const RptrSceneDesc *scene, void *nodes, size_t *n_nodes, void *tris, size_t *n_tris,
                            void *instances, size_t *n_instances, int32_t *out_stack_need);

/* ---- stats() (render_vulkan.cpp:2229-2243) */
int rptr_hip_stats(const rptr_hip_t *h, RptrStats *out);

#ifdef __cplusplus
}
#endif
#endif /* RPTR_HIP_H */
