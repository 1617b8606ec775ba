"""`RenderHip`: Python mirror of the reference's `RenderBackend` plugin surface
(librender/render_backend.h:68-116) over the C ABI of librptr_hip.so.

Same method names, argument meaning and error behaviour as the reference
interface for the hot path: failures raise (the reference throws
`logged_exception`, util/error_io.h:27-29), `configure_for` returns a bool,
read-backs return the element count or 0 when the buffer is too small
(render_vulkan.cpp:2256-2275). No compute happens in Python; without the HIP
library or without a GPU every compute call raises `BackendError`.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import abi
from .build import LIB_PATH


class BackendError(RuntimeError):
    """≙ logged_exception (util/error_io.h:27-29)."""

    def __init__(self, code, msg):
        super().__init__("rptr_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library(path=None):
    """Loads librptr_hip.so and declares every prototype of include/rptr_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("RPTR_HIP_LIB") or LIB_PATH  # RPTR_HIP_LIB: A/B builds of the same ABI (tools/ab.sh)
    if not os.path.exists(path):
        raise BackendError(abi.RPTR_E_NO_DEVICE, "%s is missing: build it with __graft_entry__.build() "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    # PyTorch-ROCm bundles its own HIP runtime under the same soname as /opt/rocm's. Whichever is loaded first serves
    # the whole process, and torch fails with "No HIP GPUs are available" when it finds the system one already loaded.
    # The tile gather (distributed.py) needs torch in the same process, so torch's libraries go first when it is installed.
    if "torch" not in sys.modules and os.environ.get("RPTR_SKIP_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int
    L.rptr_hip_create.argtypes = [C.POINTER(abi.CreateInfo), C.POINTER(vp)]
    L.rptr_hip_destroy.argtypes = [vp]
    L.rptr_hip_destroy.restype = None
    L.rptr_hip_last_error.argtypes = [vp]
    L.rptr_hip_last_error.restype = C.c_char_p
    L.rptr_hip_name.restype = C.c_char_p
    L.rptr_hip_set_stream.argtypes = [vp, vp]
    L.rptr_hip_initialize.argtypes = [vp, i32, i32]
    L.rptr_hip_set_scene.argtypes = [vp, C.POINTER(abi.SceneDesc)]
    L.rptr_hip_update_vertices.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.rptr_hip_update_vertices_device.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.rptr_hip_refit.argtypes = [vp]
    L.rptr_hip_set_params.argtypes = [vp, C.POINTER(abi.RenderParams), C.POINTER(abi.SceneParams), C.POINTER(abi.LightSamplingConfig)]
    L.rptr_hip_render.argtypes = [vp, C.POINTER(abi.Camera), i32, i32, i32, i32, C.POINTER(abi.Stats)]
    L.rptr_hip_render_async.argtypes = [vp, C.POINTER(abi.Camera), i32, i32, i32, i32, C.POINTER(C.c_uint64)]
    L.rptr_hip_wait.argtypes = [vp, C.c_uint64, C.POINTER(abi.Stats)]
    L.rptr_hip_render_batch_async.argtypes = [vp, C.POINTER(abi.Camera), i32, i32, i32, i32, i32, i32, C.POINTER(C.c_uint64)]
    L.rptr_hip_render_batch_cameras_async.argtypes = [vp, C.POINTER(abi.Camera), i32, i32, i32, i32, i32, i32, C.POINTER(C.c_uint64)]
    L.rptr_hip_set_stage_timing.argtypes = [vp, i32]
    L.rptr_hip_trace_device.argtypes = [vp, vp, i32, vp, vp]
    L.rptr_hip_enable_ray_queries.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(vp)]
    L.rptr_hip_render_ray_queries.argtypes = [vp, i32]
    L.rptr_hip_trace_radiance.argtypes = [vp, vp, i32, C.POINTER(abi.Camera), i32, i32, i32, vp, C.POINTER(abi.Stats)]
    L.rptr_hip_trace_radiance_device.argtypes = [vp, vp, i32, C.POINTER(abi.Camera), i32, i32, i32, vp, vp]
    L.rptr_hip_render_radiance_queries.argtypes = [vp, i32, C.POINTER(abi.Camera), i32, i32, i32]
    L.rptr_hip_trace_surface.argtypes = [vp, vp, i32, C.POINTER(abi.Camera), i32, vp]
    L.rptr_hip_trace_surface_device.argtypes = [vp, vp, i32, C.POINTER(abi.Camera), i32, vp, vp]
    L.rptr_hip_occlusion_defaults.argtypes = [C.POINTER(abi.OcclusionParams)]
    L.rptr_hip_occlusion_defaults.restype = None
    L.rptr_hip_trace_occlusion.argtypes = [vp, vp, i32, C.POINTER(abi.OcclusionParams), vp]
    L.rptr_hip_trace_occlusion_device.argtypes = [vp, vp, i32, C.POINTER(abi.OcclusionParams), vp, vp]
    L.rptr_hip_probe_defaults.argtypes = [C.POINTER(abi.ProbeParams)]
    L.rptr_hip_probe_defaults.restype = None
    L.rptr_hip_probe_directions.argtypes = [C.c_uint32, vp]
    L.rptr_hip_probe_rays_device.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.ProbeParams), vp, vp]
    L.rptr_hip_probe_project_device.argtypes = [vp, vp, C.c_uint32, vp, C.POINTER(abi.ProbeParams), vp, vp]
    L.rptr_hip_trace_probes.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.Camera), i32, C.POINTER(abi.ProbeParams), vp, C.POINTER(abi.Stats)]
    L.rptr_hip_trace_probes_device.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.Camera), i32, C.POINTER(abi.ProbeParams), vp, vp]
    L.rptr_hip_readback_probe_rays.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_set_light_sampling_variant.argtypes = [vp, i32]
    L.rptr_hip_set_freeze_frame.argtypes = [vp, i32]
    L.rptr_hip_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.rptr_hip_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.rptr_hip_option_name.argtypes = [i32]
    L.rptr_hip_option_name.restype = C.c_char_p
    L.rptr_hip_set_rng_variant.argtypes = [vp, i32, vp, C.c_size_t]
    L.rptr_hip_set_bvh_policy.argtypes = [vp, i32, i32]
    L.rptr_hip_bvh_rebuild_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rptr_hip_update_instances.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_update_instances_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_set_tlas_policy.argtypes = [vp, i32]
    L.rptr_hip_tlas_rebuild_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rptr_hip_set_light_sources.argtypes = [vp, vp, C.c_uint32]
    L.rptr_hip_readback_lights.argtypes = [vp, vp, C.c_uint32]
    L.rptr_hip_set_skin.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.rptr_hip_update_bones.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_update_bones_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_skin.argtypes = [vp]
    L.rptr_hip_readback_skinned.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32]
    L.rptr_hip_set_morph_targets.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.rptr_hip_update_morph_weights.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_update_morph_weights_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.rptr_hip_set_normal_groups.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32]
    L.rptr_hip_recompute_normals.argtypes = [vp]
    L.rptr_hip_update_texture.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.c_uint32]
    L.rptr_hip_update_texture_device.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.c_uint32]
    L.rptr_hip_readback_texture.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t]
    L.rptr_hip_texture_levels.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rptr_hip_srgb_decode_table.argtypes = [C.POINTER(C.c_float)]
    L.rptr_hip_srgb_decode_table.restype = None
    L.rptr_hip_bvh_build_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rptr_hip_traversal_preset.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rptr_hip_get_framebuffer_size.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rptr_hip_readback_f32.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_readback_u8.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_readback_aov.argtypes = [vp, i32, vp, C.c_size_t]
    L.rptr_hip_denoise_defaults.argtypes = [C.POINTER(abi.DenoiseParams)]
    L.rptr_hip_denoise_defaults.restype = None
    L.rptr_hip_denoise.argtypes = [vp, C.POINTER(abi.DenoiseParams)]
    L.rptr_hip_readback_denoised_f32.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_readback_denoised_u8.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_denoise_temporal_defaults.argtypes = [C.POINTER(abi.DenoiseTemporalParams)]
    L.rptr_hip_denoise_temporal_defaults.restype = None
    L.rptr_hip_denoise_temporal.argtypes = [vp, C.POINTER(abi.DenoiseTemporalParams)]
    L.rptr_hip_readback_denoise_history_f32.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_taa_upscale_defaults.argtypes = [C.POINTER(abi.TaaUpscaleParams)]
    L.rptr_hip_taa_upscale_defaults.restype = None
    L.rptr_hip_taa_upscale.argtypes = [vp, C.POINTER(abi.TaaUpscaleParams)]
    L.rptr_hip_readback_upscaled_u8.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_auto_exposure_defaults.argtypes = [C.POINTER(abi.AutoExposureParams)]
    L.rptr_hip_auto_exposure_defaults.restype = None
    L.rptr_hip_auto_exposure.argtypes = [vp, C.POINTER(abi.AutoExposureParams)]
    L.rptr_hip_readback_exposed_u8.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_readback_exposure_state.argtypes = [vp, C.POINTER(abi.ExposureState)]
    L.rptr_hip_bloom_defaults.argtypes = [C.POINTER(abi.BloomParams)]
    L.rptr_hip_bloom_defaults.restype = None
    L.rptr_hip_bloom.argtypes = [vp, C.POINTER(abi.BloomParams)]
    L.rptr_hip_readback_bloomed_u8.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_bloom_levels.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rptr_hip_readback_bloom_level_f32.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_size_t]
    L.rptr_hip_track_object_motion.argtypes = [vp, i32]
    L.rptr_hip_object_motion.argtypes = [vp]
    L.rptr_hip_tile_rows.argtypes = [vp, i32, vp, i32]
    L.rptr_hip_local_pixel_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rptr_hip_copy_tile_to_device.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_build_bvh_host.argtypes = [C.POINTER(abi.SceneDesc), vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t), vp,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.rptr_hip_trace.argtypes = [vp, vp, i32, vp]
    L.rptr_hip_trace_counted.argtypes = [vp, vp, i32, vp, vp, vp, i32]
    L.rptr_hip_export_bvh.argtypes = [vp, vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_size_t)]
    L.rptr_hip_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.rptr_hip_comm_get_unique_id.argtypes = [vp]
    L.rptr_hip_comm_init_rank.argtypes = [vp, vp]
    L.rptr_hip_comm_init_all.argtypes = [C.POINTER(vp), i32]
    L.rptr_hip_comm_destroy.argtypes = [vp]
    L.rptr_hip_gather.argtypes = [vp]
    L.rptr_hip_gather_all.argtypes = [C.POINTER(vp), i32]
    L.rptr_hip_gather_batch.argtypes = [vp, i32]
    L.rptr_hip_gather_all_batch.argtypes = [C.POINTER(vp), i32, i32]
    L.rptr_hip_readback_gathered_frame_f32.argtypes = [vp, i32, vp, C.c_size_t]
    L.rptr_hip_gathered_frame.argtypes = [vp, C.POINTER(vp)]
    L.rptr_hip_readback_gathered_f32.argtypes = [vp, vp, C.c_size_t]
    L.rptr_hip_comm_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.rptr_hip_comm_transport.argtypes = [vp]
    L.rptr_hip_comm_ipc_export.argtypes = [vp, vp]
    L.rptr_hip_comm_ipc_init.argtypes = [vp, vp]
    L.rptr_hip_comm_transport.restype = C.c_char_p
    for name in abi.EXPORTED_SYMBOLS:
        getattr(L, name)  # AttributeError if the library lacks a declared symbol
    _lib = L
    return L


def srgb_decode_table():
    """(256,) float32: the sRGB decode table set_scene uploads (rptr_hip_srgb_decode_table; no GPU needed). scenes.generate_mips takes it."""
    out = np.zeros(256, dtype=np.float32)
    load_library().rptr_hip_srgb_decode_table(out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def build_bvh_host(scene):
    """The acceleration structure set_scene would build, made on the host alone (no GPU needed): returns
    (nodes, tris, instances, stack_need) as float32 views of RptrBvh4Node / RptrBvhTri / RptrBvhInstance arrays."""
    L = load_library()
    desc = scene.desc()
    nn, nt, ni, need = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    rc = L.rptr_hip_build_bvh_host(C.byref(desc), None, C.byref(nn), None, C.byref(nt), None, C.byref(ni), C.byref(need))
    if rc != 0:
        raise BackendError(rc, L.rptr_hip_last_error(None).decode())
    nodes = np.zeros(max(nn.value, 1) * 16, dtype=np.float32)
    tris = np.zeros(max(nt.value, 1) * 12, dtype=np.float32)
    insts = np.zeros(max(ni.value, 1) * 32, dtype=np.float32)
    rc = L.rptr_hip_build_bvh_host(C.byref(desc), nodes.ctypes.data_as(C.c_void_p), C.byref(nn), tris.ctypes.data_as(C.c_void_p), C.byref(nt),
                                   insts.ctypes.data_as(C.c_void_p), C.byref(ni), C.byref(need))
    if rc != 0:
        raise BackendError(rc, L.rptr_hip_last_error(None).decode())
    return nodes[:nn.value * 16], tris[:nt.value * 12], insts[:ni.value * 32], int(need.value)


class RenderStats:  # librender/render_backend.h:15-24
    def __init__(self, s: abi.Stats = None):
        self.render_time = s.render_time_ms if s else 0.0
        rays = (s.rays_closest + s.rays_shadow) if s else 0
        self.rays_per_second = rays / (self.render_time * 1e-3) if s and self.render_time > 0 else -1.0
        self.spp = s.spp if s else 0
        self.frame_stats_delay = 0
        self.has_valid_frame_stats = bool(s and s.render_time_ms > 0)
        self.total_device_bytes_allocated = s.device_bytes_allocated if s else 0
        self.raw = s


class RenderConfiguration:  # librender/render_backend.h:33-40
    def __init__(self, camera: abi.Camera, active_variant=0, reset_accumulation=False, freeze_frame=False, time=0.0):
        self.camera = camera
        self.time = time
        self.active_variant = active_variant
        self.reset_accumulation = reset_accumulation
        self.freeze_frame = freeze_frame


class RenderHip:
    """Drop-in shaped like `struct RenderBackend` (render_backend.h:68-116)."""

    def __init__(self, device_ordinal=0, rank=0, world_size=1, stripe_rows=32, stream=None, frames_in_flight=1, options=None, create_flags=0):
        """stream: a hipStream_t handle shared with the caller (everything the backend queues is ordered with the caller's
        work on it), or None / 0 for a stream the backend owns. torch's *default* stream has handle 0: to share ordering
        with torch, make a torch.cuda.Stream() current and pass its .cuda_stream (bench.py does)."""
        self._L = load_library()
        info = abi.CreateInfo(device_ordinal, rank, world_size, stripe_rows, stream, frames_in_flight, abi.ABI_VERSION, create_flags, 0)
        self.frames_in_flight = max(1, frames_in_flight)
        h = C.c_void_p()
        rc = self._L.rptr_hip_create(C.byref(info), C.byref(h))
        if rc != 0:
            raise BackendError(rc, self._L.rptr_hip_last_error(None).decode())
        self._h = h
        for k, v in (options or {}).items():  # rptr_hip_set_option right after the create: in force for initialize / set_scene
            self.set_option(k, v)
        # public data members the app mutates directly (render_backend.h:69-76)
        self.params = abi.RenderParams.default()
        # RenderBackendOptions::enable_raytraced_dof (render_params.glsl.h:97, default true): a switch of this class, not a library option.
        # False hands the library aperture_radius = focal_length = 0 (render_vulkan.cpp:2945-2947); self.params stays the caller's.
        self.enable_raytraced_dof = True
        self.lighting_params = abi.LightSamplingConfig.default()
        self.scene_params = None
        self.camera = None
        self.reset_accumulation = False
        self.freeze_frame = False
        self.rank, self.world_size = rank, world_size
        self._variant = abi.VARIANT_GLTF
        self._stats = None
        self._query_stats = None
        self._fb_dims = (0, 0)
        self._spp_per_frame = 1

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.rptr_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise BackendError(rc, self._L.rptr_hip_last_error(self._h).decode())

    # ---- RenderBackend virtuals
    def name(self):
        return self._L.rptr_hip_name().decode()

    def variant_names(self):
        return list(abi.VARIANT_NAMES)

    def variant_index(self, name):
        return abi.VARIANT_NAMES.index(name) if name in abi.VARIANT_NAMES else -1

    def initialize(self, fb_width, fb_height):
        self._check(self._L.rptr_hip_initialize(self._h, fb_width, fb_height))
        self._fb_dims = (fb_width, fb_height)

    def set_scene(self, scene):
        """scene: realtimepathtracingresearchframework_amd.scenes.Scene (≙ const Scene&)."""
        desc = scene.desc()
        self._check(self._L.rptr_hip_set_scene(self._h, C.byref(desc)))
        self._num_lights = int(desc.num_lights)
        self._geometries = [(int(g.num_tris), bool(g.has_normals and g.qnrm_uv is not None)) for g in scene.geometries]  # (readback_skinned)
        self._textures = [tuple(int(v) for v in np.asarray(t.rgba).shape[:2]) for t in scene.textures]  # (height, width): readback_texture
        self.update_config(scene)

    def update_config(self, scene_or_params):
        """≙ update_config(SceneConfig): sky/sun fit + normal_z_scale (render_vulkan.cpp:2954-2959)."""
        sp = scene_or_params if isinstance(scene_or_params, abi.SceneParams) else scene_or_params.scene_params()
        self.scene_params = sp

    def configure_for(self, options=None, variant_idx=0):
        if variant_idx not in (abi.VARIANT_GLTF, abi.VARIANT_SIMPLE, abi.VARIANT_GLTF_TRANSMISSION):
            return False
        self._variant = variant_idx
        return True

    def _push_params(self):
        self._check(self._L.rptr_hip_set_freeze_frame(self._h, 1 if self.freeze_frame else 0))
        params = self.params
        if not self.enable_raytraced_dof:
            params = abi.RenderParams.from_buffer_copy(self.params)
            params.aperture_radius = params.focal_length = 0.0
        self._check(self._L.rptr_hip_set_params(self._h, C.byref(params), C.byref(self.scene_params) if self.scene_params else None,
                                                C.byref(self.lighting_params)))

    def begin_frame(self, cmd_stream, config: RenderConfiguration):
        self.camera = config.camera
        self.reset_accumulation = config.reset_accumulation
        self.freeze_frame = config.freeze_frame
        self.configure_for(None, config.active_variant)

    def draw_frame(self, cmd_stream=None, variant_idx=None, spp=None, count_traversal=False):
        """One reference frame = params.batch_spp samples; `spp` renders that many frames' worth at once."""
        if variant_idx is not None:
            self.configure_for(None, variant_idx)
        self._push_params()
        st = abi.Stats()
        n = spp if spp is not None else max(1, self.params.batch_spp)
        self._check(self._L.rptr_hip_render(self._h, C.byref(self.camera), self._variant, n, 1 if self.reset_accumulation else 0,
                                            1 if count_traversal else 0, C.byref(st)))
        self.reset_accumulation = False
        self._stats = st

    # ---- frames in flight: queue a frame, collect it later (the tail of one frame overlaps the head of the next)
    def render_async(self, config: RenderConfiguration, spp=1, count_traversal=False):
        """begin_frame + an asynchronous draw_frame; returns the ticket to hand to wait()."""
        self.begin_frame(None, config)
        self._push_params()
        ticket = C.c_uint64(0)
        self._check(self._L.rptr_hip_render_async(self._h, C.byref(self.camera), self._variant, spp, 1 if self.reset_accumulation else 0,
                                                  1 if count_traversal else 0, C.byref(ticket)))
        self.reset_accumulation = False
        return int(ticket.value)

    def render_batch_async(self, config: RenderConfiguration, spp=1, n_frames=1, reset_rest=True, count_traversal=False):
        """n_frames consecutive frames of the same view in one launch sequence (include/rptr_hip.h rptr_hip_render_batch_async): frame 0
        resets iff config.reset_accumulation, the others iff reset_rest; returns their tickets"""
        self.begin_frame(None, config)
        self._push_params()
        tickets = (C.c_uint64 * n_frames)()
        self._check(self._L.rptr_hip_render_batch_async(self._h, C.byref(self.camera), self._variant, spp, n_frames, 1 if self.reset_accumulation else 0,
                                                        1 if reset_rest else 0, 1 if count_traversal else 0, tickets))
        self.reset_accumulation = False
        return [int(t) for t in tickets]

    def render_batch_cameras_async(self, config: RenderConfiguration, cameras, spp=1, reset_rest=True, count_traversal=False):
        """len(cameras) consecutive frames in one launch sequence, frame k through cameras[k] (include/rptr_hip.h
        rptr_hip_render_batch_cameras_async; ≙ a host that moves the camera every frame, app.cpp:350-469); returns their tickets"""
        self.begin_frame(None, config)
        self._push_params()
        n = len(cameras)
        arr = (abi.Camera * n)(*cameras)
        tickets = (C.c_uint64 * n)()
        self._check(self._L.rptr_hip_render_batch_cameras_async(self._h, arr, self._variant, spp, n, 1 if self.reset_accumulation else 0,
                                                                1 if reset_rest else 0, 1 if count_traversal else 0, tickets))
        self.camera = cameras[-1]
        self.reset_accumulation = False
        return [int(t) for t in tickets]

    def wait(self, ticket):
        st = abi.Stats()
        self._check(self._L.rptr_hip_wait(self._h, C.c_uint64(ticket), C.byref(st)))
        self._stats = st
        return self.stats()

    def set_stage_timing(self, level):
        """0 (the default): no per-stage events -- RptrStats.render_time_ms is filled, the per-stage *_time_ms stay zero; 1: events around the
        closest-hit traversal launches (extend_time_ms); 2: around every stage (what bench.py's exclusive pass reads: ~0.06 ms per 1080p frame)."""
        self._check(self._L.rptr_hip_set_stage_timing(self._h, int(level)))

    def set_option(self, key, value):
        """rptr_hip_set_option (include/rptr_hip.h "Options"): takes effect at the call the header names for the key
        (initialize / set_scene / the next frame / communicator set-up)."""
        self._check(self._L.rptr_hip_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._check(self._L.rptr_hip_get_option(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def end_frame(self, cmd_stream=None, variant_idx=0):
        pass  # resolve (process_samples) is sequenced inside draw_frame on the same stream

    def render(self, config: RenderConfiguration, spp=1, count_traversal=False):
        """≙ RenderBackend::render(config): begin_frame + draw_frame + end_frame."""
        self.begin_frame(None, config)
        self.draw_frame(None, spp=spp, count_traversal=count_traversal)
        self.end_frame(None)
        return self.stats()

    def stats(self):
        return RenderStats(self._stats)

    def flush_pipeline(self):
        pass

    # ---- RenderGraphic
    def get_framebuffer_size(self):
        whc = (C.c_uint32 * 3)()
        self._check(self._L.rptr_hip_get_framebuffer_size(self._h, whc))
        return tuple(int(x) for x in whc)

    def readback_framebuffer(self, buffer: np.ndarray):
        """float32 buffer -> accumulation buffer (RGBA32F); uint8 buffer -> sRGB RGBA8. Returns #elements or 0."""
        w, hgt, c = self.get_framebuffer_size()
        need = w * hgt * c
        if buffer.size < need:
            return 0
        if buffer.dtype == np.float32:
            self._check(self._L.rptr_hip_readback_f32(self._h, buffer.ctypes.data_as(C.c_void_p), buffer.size))
        elif buffer.dtype == np.uint8:
            self._check(self._L.rptr_hip_readback_u8(self._h, buffer.ctypes.data_as(C.c_void_p), buffer.size))
        else:
            raise TypeError("readback_framebuffer: float32 or uint8 buffer expected")
        return need

    AOVAlbedoRoughnessIndex, AOVNormalDepthIndex, AOVMotionJitterIndex = 0, 1, 2   # RenderGraphic::AOVBufferIndex

    def readback_aov(self, aov_index, buffer: np.ndarray):
        """RenderGraphic::readback_aov (render_graphic.h:40): float16 (or uint16) buffer of width*height*4 -> #elements or 0"""
        w, hgt, c = self.get_framebuffer_size()
        need = w * hgt * c
        if buffer.size < need or buffer.dtype.itemsize != 2:
            return 0
        self._check(self._L.rptr_hip_readback_aov(self._h, int(aov_index), buffer.ctypes.data_as(C.c_void_p), buffer.size))
        return need

    # ---- the denoiser (include/rptr_hip.h rptr_hip_denoise; csrc/denoise.h)
    def denoise(self, params=None, **fields):
        """Denoises the frame the read-backs return (the frame waited for last) into images of its own; asynchronous on the backend's
        stream. params: an abi.DenoiseParams, or None for the library's defaults; keyword arguments override single fields
        (iterations, sigma_luminance, sigma_depth, normal_power_log2, demodulate_albedo). The RGBA8 image goes through the render
        parameters of self.params as they are now. Returns the parameters used."""
        p = abi.DenoiseParams()
        if params is None:
            self._L.rptr_hip_denoise_defaults(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(abi.DenoiseParams._fields_) or k == "reserved":
                raise TypeError("denoise: unknown parameter %r" % k)
            setattr(p, k, v)
        self._push_params()
        self._check(self._L.rptr_hip_denoise(self._h, C.byref(p)))
        return p

    def readback_denoised_f32(self):
        """the denoised RGBA32F image of the last denoise() as an (H, W, 4) float32 array"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((hgt, w, c), np.float32)
        self._check(self._L.rptr_hip_readback_denoised_f32(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def readback_denoised_u8(self):
        """the denoised sRGB RGBA8 image of the last denoise() as an (H, W, 4) uint8 array"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((hgt, w, c), np.uint8)
        self._check(self._L.rptr_hip_readback_denoised_u8(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    # ---- the temporal denoiser (include/rptr_hip.h rptr_hip_denoise_temporal; csrc/denoise_temporal.h)
    def denoise_temporal(self, params=None, **fields):
        """Denoises the frame the read-backs return (the frame waited for last) with the history the previous call left, fetched along
        the frame's motion AOV, and leaves the next call's history; the result is read with readback_denoised_f32 / _u8. One call per
        frame: pass reset_history = 1 for a frame that does not follow the previous call's frame (a skipped frame, a restarted
        accumulation). params: an abi.DenoiseTemporalParams, or None for the library's defaults; keyword arguments override single
        fields. The RGBA8 image goes through the render parameters of self.params as they are now. Returns the parameters used."""
        p = abi.DenoiseTemporalParams()
        if params is None:
            self._L.rptr_hip_denoise_temporal_defaults(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(abi.DenoiseTemporalParams._fields_) or k == "reserved":
                raise TypeError("denoise_temporal: unknown parameter %r" % k)
            setattr(p, k, v)
        self._push_params()
        self._check(self._L.rptr_hip_denoise_temporal(self._h, C.byref(p)))
        return p

    def readback_denoise_history(self):
        """the history the last denoise_temporal() left as an (H, W, 4) float32 array: the blended demodulated colour and, in channel 3,
        the history length (1: none was found for the pixel; 0 where the pixel is not surface)"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((hgt, w, c), np.float32)
        self._check(self._L.rptr_hip_readback_denoise_history_f32(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    # ---- temporal 2x upscaling (include/rptr_hip.h rptr_hip_taa_upscale; csrc/taa_upscale.h)
    def taa_upscale(self, params=None, **fields):
        """Upscales the frame the read-backs return (the frame waited for last) to twice its resolution with the previous call's output
        as history; asynchronous on the backend's stream. params: an abi.TaaUpscaleParams, or None for the library's defaults; keyword
        arguments override single fields (factor, reset_history). Pass reset_history = 1 for the frame that restarted the accumulation
        (RenderConfiguration.reset_accumulation): its output is the replicated frame. Returns the parameters used."""
        p = abi.TaaUpscaleParams()
        if params is None:
            self._L.rptr_hip_taa_upscale_defaults(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(abi.TaaUpscaleParams._fields_) or k == "reserved":
                raise TypeError("taa_upscale: unknown parameter %r" % k)
            setattr(p, k, int(v))
        self._check(self._L.rptr_hip_taa_upscale(self._h, C.byref(p)))
        return p

    def readback_upscaled(self):
        """the RGBA8 image of the last taa_upscale() as a (2H, 2W, 4) uint8 array"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((2 * hgt, 2 * w, c), np.uint8)
        self._check(self._L.rptr_hip_readback_upscaled_u8(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    # ---- auto-exposure (include/rptr_hip.h rptr_hip_auto_exposure; csrc/auto_exposure.h)
    def auto_exposure(self, params=None, **fields):
        """Meters the frame the read-backs return (the frame waited for last; source = 1: the denoised image of that frame), adapts the
        exposure value on the device and writes a display-ready RGBA8 image of its own; asynchronous on the backend's stream. params: an
        abi.AutoExposureParams, or None for the library's defaults; keyword arguments override single fields (white_balance: three
        gains). Pass reset_history = 1 for a frame the adaptation should not carry over to, and dt = the seconds since the previous
        call (0: jump to the target). self.params.exposure, as it is now, is added to the metered value. Returns the parameters used."""
        p = abi.AutoExposureParams()
        if params is None:
            self._L.rptr_hip_auto_exposure_defaults(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(abi.AutoExposureParams._fields_) or k == "reserved":
                raise TypeError("auto_exposure: unknown parameter %r" % k)
            if k == "white_balance":
                p.white_balance[:] = [float(g) for g in v]
            else:
                setattr(p, k, v)
        self._push_params()
        self._check(self._L.rptr_hip_auto_exposure(self._h, C.byref(p)))
        return p

    def readback_exposed(self):
        """the RGBA8 image of the last auto_exposure() as an (H, W, 4) uint8 array"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((hgt, w, c), np.uint8)
        self._check(self._L.rptr_hip_readback_exposed_u8(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def readback_exposure_state(self):
        """what the last metering auto_exposure() (mode = 1) left: an abi.ExposureState"""
        st = abi.ExposureState()
        self._check(self._L.rptr_hip_readback_exposure_state(self._h, C.byref(st)))
        return st

    # ---- bloom (include/rptr_hip.h rptr_hip_bloom; csrc/bloom.h)
    def bloom(self, params=None, **fields):
        """Adds glare to the frame the read-backs return: what the exposed image holds above `threshold` goes down a pyramid, back up,
        and is added in front of the tone map, into an RGBA8 image of its own; asynchronous on the backend's stream. params: an
        abi.BloomParams, or None for the library's defaults; keyword arguments override single fields (white_balance: three gains).
        exposure_mode = 1 uses the scale the last metering auto_exposure() left on the device (call order: auto_exposure -> bloom ->
        present); 0 uses self.params.exposure as it is now. Returns the parameters used."""
        p = abi.BloomParams()
        if params is None:
            self._L.rptr_hip_bloom_defaults(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(abi.BloomParams._fields_) or k == "reserved":
                raise TypeError("bloom: unknown parameter %r" % k)
            if k == "white_balance":
                p.white_balance[:] = [float(g) for g in v]
            else:
                setattr(p, k, v)
        self._push_params()
        self._check(self._L.rptr_hip_bloom(self._h, C.byref(p)))
        return p

    def readback_bloomed(self):
        """the RGBA8 image of the last bloom() as an (H, W, 4) uint8 array"""
        w, hgt, c = self.get_framebuffer_size()
        out = np.zeros((hgt, w, c), np.uint8)
        self._check(self._L.rptr_hip_readback_bloomed_u8(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def bloom_levels(self):
        """L of the last bloom() (0: it copied an AOV view)"""
        n = C.c_uint32(0)
        self._check(self._L.rptr_hip_bloom_levels(self._h, C.byref(n)))
        return int(n.value)

    def bloom_level(self, which, level):
        """level 1 .. L of the last bloom()'s down pyramid d (which = 0) or up pyramid u (which = 1): an (h_l, w_l, 4) float32 array"""
        w, hgt, _ = self.get_framebuffer_size()
        for _ in range(int(level)):
            w, hgt = (w + 1) // 2, (hgt + 1) // 2
        out = np.zeros((max(hgt, 1), max(w, 1), 4), np.float32)
        self._check(self._L.rptr_hip_readback_bloom_level_f32(self._h, int(which), int(level), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    # ---- object motion (include/rptr_hip.h rptr_hip_object_motion; csrc/object_motion.h)
    def track_object_motion(self, enable=True):
        """Keeps the state the previous frame saw (instance transforms, positions of dynamic meshes) so that object_motion() can tell
        what moved. After set_scene; a new set_scene drops it."""
        self._check(self._L.rptr_hip_track_object_motion(self._h, 1 if enable else 0))

    def object_motion(self):
        """Rewrites the .xy half of the last submitted frame's motion + jitter AOV texels where its objects moved since the frame before
        (call order per frame: update_* -> refit -> render -> object_motion -> denoise_temporal / taa_upscale). Returns the number of
        pixels rewritten (waits for the pass)."""
        self._check(self._L.rptr_hip_object_motion(self._h))
        return self.get_option("object_motion_pixels")

    # ---- ray queries (RQ_CLOSEST)
    def enable_ray_queries(self, max_queries=512 * 512, max_queries_per_pixel=0):
        self._max_queries = max_queries

    @staticmethod
    def _query_rows(queries):
        """the contiguous (n, 8) float32 view of RenderRayQuery[n]"""
        return np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 8)

    @staticmethod
    def _result_rows(results, n, dtype, row=(), who="", what=""):
        """`results` when it can hold n rows of shape `row` and type `dtype` (ValueError "<who>: results must be <what>" otherwise), zeros when None"""
        if results is None:
            return np.zeros((n,) + row, dtype=dtype)
        if results.dtype != dtype or not results.flags["C_CONTIGUOUS"] or results.size < n * int(np.prod(row, dtype=np.int64)):
            raise ValueError("%s: results must be %s" % (who, what))
        return results

    def render_ray_queries(self, queries: np.ndarray, results: np.ndarray = None):
        """queries: (n,8) float32 view of RenderRayQuery[n]; returns (n,4) float32 in rt_intersect layout."""
        q = self._query_rows(queries)
        results = self._result_rows(results, len(q), np.float32, (4,), "render_ray_queries", "a C-contiguous float32 array of n x 4")
        self._check(self._L.rptr_hip_trace(self._h, q.ctypes.data_as(C.c_void_p), len(q), results.ctypes.data_as(C.c_void_p)))
        return results

    def enable_ray_queries_device(self, max_queries, max_queries_per_pixel=0):
        """RenderBackend::enable_ray_queries: the backend's device buffers (≙ ray_query_buffer / ray_result_buffer), as addresses"""
        q, r = C.c_void_p(), C.c_void_p()
        self._check(self._L.rptr_hip_enable_ray_queries(self._h, int(max_queries), int(max_queries_per_pixel), C.byref(q), C.byref(r)))
        return q.value, r.value

    def render_ray_queries_device(self, num_queries):
        """RenderBackend::render_ray_queries over the backend's device buffers (asynchronous on the backend's stream)"""
        self._check(self._L.rptr_hip_render_ray_queries(self._h, int(num_queries)))

    def trace_device(self, device_queries, n, device_results, stream=None):
        self._check(self._L.rptr_hip_trace_device(self._h, C.c_void_p(device_queries), int(n), C.c_void_p(device_results), C.c_void_p(stream or 0)))

    # ---- ray queries with a path-tracing variant: radiance along the query rays (include/rptr_hip.h rptr_hip_trace_radiance)
    def render_radiance_queries(self, queries: np.ndarray, camera, variant=abi.VARIANT_GLTF, spp=1, first_sample=0, results: np.ndarray = None):
        """queries: (n,8) float32 view of RenderRayQuery[n]; camera: abi.Camera (its image-plane axes size the texture footprint).
        Returns (n,4) float32 = (radiance.rgb, alpha): the running mean over samples first_sample .. first_sample + spp - 1, folded into
        `results` (read for first_sample > 0 and for the slots of queries with mode_or_data < 0, which stay as they are). The frame in
        progress is left alone; the run's ray counts: radiance_query_stats()."""
        q = self._query_rows(queries)
        results = self._result_rows(results, len(q), np.float32, (4,), "render_radiance_queries", "a C-contiguous float32 array of n x 4")
        self._push_params()
        st = abi.Stats()
        self._check(self._L.rptr_hip_trace_radiance(self._h, q.ctypes.data_as(C.c_void_p), len(q), C.byref(camera), int(variant), int(spp), int(first_sample),
                                                    results.ctypes.data_as(C.c_void_p), C.byref(st)))
        self._query_stats = st
        return results

    def radiance_query_stats(self):
        """RenderStats of the last render_radiance_queries (rays_closest / rays_shadow / hits_shaded; stats() stays the last frame's)"""
        return RenderStats(self._query_stats)

    def render_radiance_queries_device(self, num_queries, camera, variant=abi.VARIANT_GLTF, spp=1, first_sample=0, device_queries=None, device_results=None,
                                       stream=None):
        """the same over DEVICE buffers, asynchronously: the backend's own (enable_ray_queries_device; on the backend's stream) unless
        device_queries / device_results name others (then on `stream`, None = the backend's)"""
        self._push_params()
        if device_queries is None and device_results is None:
            self._check(self._L.rptr_hip_render_radiance_queries(self._h, int(num_queries), C.byref(camera), int(variant), int(spp), int(first_sample)))
        else:
            self._check(self._L.rptr_hip_trace_radiance_device(self._h, C.c_void_p(device_queries), int(num_queries), C.byref(camera), int(variant), int(spp),
                                                               int(first_sample), C.c_void_p(device_results), C.c_void_p(stream or 0)))

    # ---- surface queries: position, normals and material at the closest hit (include/rptr_hip.h rptr_hip_trace_surface)
    def render_surface_queries(self, queries: np.ndarray, camera, variant=abi.VARIANT_GLTF, results: np.ndarray = None):
        """queries: (n,8) float32 view of RenderRayQuery[n]; camera: abi.Camera (its image-plane axes size the texture footprint).
        Returns n records of abi.SURFACE_HIT_DTYPE, written into `results` when given (read too: the slots of queries with
        mode_or_data < 0 stay as they are). A miss has t = -1. The frame in progress is left alone."""
        q = self._query_rows(queries)
        results = self._result_rows(results, len(q), abi.SURFACE_HIT_DTYPE, (), "render_surface_queries", "a C-contiguous array of n abi.SURFACE_HIT_DTYPE records")
        self._push_params()
        self._check(self._L.rptr_hip_trace_surface(self._h, q.ctypes.data_as(C.c_void_p), len(q), C.byref(camera), int(variant), results.ctypes.data_as(C.c_void_p)))
        return results

    def render_surface_queries_device(self, num_queries, camera, variant=abi.VARIANT_GLTF, device_queries=None, device_results=None, stream=None):
        """the same over DEVICE buffers, asynchronously on `stream` (None = the backend's): device_results names num_queries records of
        96 bytes; device_queries None = the query buffer of enable_ray_queries_device"""
        self._push_params()
        self._check(self._L.rptr_hip_trace_surface_device(self._h, C.c_void_p(device_queries or 0), int(num_queries), C.byref(camera), int(variant),
                                                          C.c_void_p(device_results or 0), C.c_void_p(stream or 0)))

    # ---- occlusion queries: one bit per query (include/rptr_hip.h rptr_hip_trace_occlusion)
    @staticmethod
    def pack_occlusion_bits(occluded) -> np.ndarray:
        """n bools -> ceil(n / 32) uint32 words, query q in bit q & 31 of word q >> 5 (little-endian bit order)"""
        b = np.ascontiguousarray(occluded, dtype=bool).reshape(-1)
        return np.packbits(np.concatenate([b, np.zeros(-len(b) % 32, bool)]), bitorder="little").view("<u4").astype(np.uint32)

    @staticmethod
    def unpack_occlusion_bits(words, n) -> np.ndarray:
        """the first n bits of uint32 words as bools"""
        w = np.ascontiguousarray(words, dtype=np.uint32).astype("<u4")
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)

    def _occlusion_params(self, alpha_cutoff):
        p = abi.OcclusionParams()
        self._L.rptr_hip_occlusion_defaults(C.byref(p))
        if alpha_cutoff is not None:
            p.flags = abi.OCCLUSION_ALPHA_CUTOUT
            p.alpha_cutoff = float(alpha_cutoff)
        return p

    def render_occlusion_queries(self, queries: np.ndarray, alpha_cutoff=None, results: np.ndarray = None) -> np.ndarray:
        """queries: (n,8) float32 view of RenderRayQuery[n]. Returns n bools, True = something lies on the ray inside (t_min, t_max).
        alpha_cutoff None: every triangle is opaque; a number in (0, 1]: alpha-tested candidates with alpha below it are ignored.
        `results` (n bools), when given, supplies the answers of queries with mode_or_data < 0 -- they stay as they are -- and receives
        all of them."""
        q = self._query_rows(queries)
        n = len(q)
        if results is not None and (results.dtype != np.bool_ or results.shape != (n,)):
            raise ValueError("render_occlusion_queries: results must be a bool array of shape (n,)")
        words = self.pack_occlusion_bits(np.zeros(n, bool) if results is None else results)
        p = self._occlusion_params(alpha_cutoff)
        self._check(self._L.rptr_hip_trace_occlusion(self._h, q.ctypes.data_as(C.c_void_p), n, C.byref(p), words.ctypes.data_as(C.c_void_p)))
        out = self.unpack_occlusion_bits(words, n)
        if results is None:
            return out
        results[...] = out
        return results

    def render_occlusion_queries_device(self, num_queries, alpha_cutoff=None, device_queries=None, device_bits=None, stream=None):
        """the same over DEVICE buffers, asynchronously on `stream` (None = the backend's): device_bits names ceil(num_queries / 32)
        uint32 words, merged into (skipped queries and the bits behind num_queries keep theirs); device_queries None = the query buffer of
        enable_ray_queries_device"""
        p = self._occlusion_params(alpha_cutoff)
        self._check(self._L.rptr_hip_trace_occlusion_device(self._h, C.c_void_p(device_queries or 0), int(num_queries), C.byref(p), C.c_void_p(device_bits or 0),
                                                            C.c_void_p(stream or 0)))

    # ---- irradiance probes: SH coefficients of the incident radiance at points (include/rptr_hip.h rptr_hip_trace_probes; probes.py)
    @staticmethod
    def probe_params(**fields):
        """abi.ProbeParams: the library's defaults with `fields` set (rays_per_probe, samples_per_ray, sample_index, rotation -- nine
        floats or a 3 x 3 array, row-major --, blend, clamp, t_max, max_run_rays; flags and reserved for the refusal tests)"""
        p = abi.ProbeParams()
        load_library().rptr_hip_probe_defaults(C.byref(p))
        for name, value in fields.items():
            if name not in dict(abi.ProbeParams._fields_):
                raise TypeError("probe_params: unknown field %r" % name)
            if name in ("rotation", "reserved"):
                flat = np.asarray(value).reshape(-1)
                getattr(p, name)[:] = [float(v) if name == "rotation" else int(v) for v in flat]
            else:
                setattr(p, name, value)
        return p

    def trace_probes(self, positions: np.ndarray, camera, variant=abi.VARIANT_GLTF, coeffs: np.ndarray = None, **fields) -> np.ndarray:
        """positions: (n, 3) float32; camera: abi.Camera (its image-plane axes size the texture footprint); fields: probe_params().
        Returns (n, 9, 4) float32: coeffs[p][i][ch], the L2 SH coefficients of the radiance arriving at probe p (channels r, g, b and
        alpha = visibility of geometry), written into `coeffs` when given (read too: probes with a coordinate that is not finite keep
        theirs, and blend < 1 blends into them). The frame in progress is left alone; the call's ray counts: radiance_query_stats()."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        n = len(pos)
        coeffs = self._result_rows(coeffs, n, np.float32, (9, 4), "trace_probes", "a C-contiguous float32 array of n x 9 x 4")
        p = self.probe_params(**fields)
        self._push_params()
        st = abi.Stats()
        self._check(self._L.rptr_hip_trace_probes(self._h, pos.ctypes.data_as(C.c_void_p), n, C.byref(camera), int(variant), C.byref(p),
                                                  coeffs.ctypes.data_as(C.c_void_p), C.byref(st)))
        self._query_stats = st
        return coeffs

    def trace_probes_device(self, device_positions, n_probes, camera, device_coeffs, variant=abi.VARIANT_GLTF, stream=None, **fields):
        """the same over DEVICE buffers (3 floats and 36 floats per probe), asynchronously on `stream` (None = the backend's)"""
        p = self.probe_params(**fields)
        self._push_params()
        self._check(self._L.rptr_hip_trace_probes_device(self._h, C.c_void_p(device_positions or 0), int(n_probes), C.byref(camera), int(variant), C.byref(p),
                                                         C.c_void_p(device_coeffs or 0), C.c_void_p(stream or 0)))

    def probe_rays_device(self, device_positions, n_probes, device_queries, stream=None, **fields):
        """the ray stage alone: n_probes x rays_per_probe RenderRayQuery records into device_queries, for any query kind"""
        p = self.probe_params(**fields)
        self._check(self._L.rptr_hip_probe_rays_device(self._h, C.c_void_p(device_positions or 0), int(n_probes), C.byref(p), C.c_void_p(device_queries or 0),
                                                       C.c_void_p(stream or 0)))

    def probe_project_device(self, device_values, n_probes, device_coeffs, device_positions=None, stream=None, **fields):
        """the projection stage alone: n_probes x rays_per_probe float4 values -> 36 floats per probe; device_positions (optional): the
        probes with a coordinate that is not finite keep their coefficients"""
        p = self.probe_params(**fields)
        self._check(self._L.rptr_hip_probe_project_device(self._h, C.c_void_p(device_values or 0), int(n_probes), C.c_void_p(device_positions or 0), C.byref(p),
                                                          C.c_void_p(device_coeffs or 0), C.c_void_p(stream or 0)))

    def readback_probe_rays(self, n_rays) -> np.ndarray:
        """diagnostic: (n_rays, 4) float32, the ray values of the last run of the last trace_probes[_device] as the radiance run left them"""
        out = np.zeros((int(n_rays), 4), np.float32)
        self._check(self._L.rptr_hip_readback_probe_rays(self._h, out.ctypes.data_as(C.c_void_p), int(n_rays)))
        return out

    def set_light_sampling_variant(self, variant):
        """RenderBackendOptions::light_sampling_variant: 0 = NONE (no NEE towards emissive triangles), 1 = RIS (default)"""
        self._check(self._L.rptr_hip_set_light_sampling_variant(self._h, int(variant)))

    def trace_counted(self, queries: np.ndarray, tmin: np.ndarray = None, any_hit=False):
        """diagnostic: (results (n,4) float32, visits (n,2) uint32 = nodes, triangles per query); tmin: explicit interval
        starts; any_hit: the shadow-ray traversal (results[:,0] = 1 if occluded)."""
        q = self._query_rows(queries)
        results = self._result_rows(None, len(q), np.float32, (4,))
        visits = self._result_rows(None, len(q), np.uint32, (2,))
        tm = None if tmin is None else np.ascontiguousarray(tmin, dtype=np.float32)
        self._check(self._L.rptr_hip_trace_counted(self._h, q.ctypes.data_as(C.c_void_p), len(q), results.ctypes.data_as(C.c_void_p),
                                                   visits.ctypes.data_as(C.c_void_p), None if tm is None else tm.ctypes.data_as(C.c_void_p),
                                                   1 if any_hit else 0))
        return results, visits

    # ---- multi-GPU helpers
    def tile_rows(self, rank=None):
        rank = self.rank if rank is None else rank
        n = self._L.rptr_hip_tile_rows(self._h, rank, None, 0)
        buf = (C.c_int32 * (2 * max(n, 1)))()
        self._L.rptr_hip_tile_rows(self._h, rank, buf, n)
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    def local_pixel_count(self):
        v = C.c_uint64()
        self._check(self._L.rptr_hip_local_pixel_count(self._h, C.byref(v)))
        return int(v.value)

    # ---- dynamic meshes (Mesh::Dynamic vertex buffers + BLAS update / TLAS refit, render_vulkan.cpp:942-952,1323-1354)
    def update_vertices(self, geometry, xyz: np.ndarray):
        """Replace the float positions of one geometry of a dynamic mesh: xyz is (3*num_tris, 3) float32 (unrolled)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._check(self._L.rptr_hip_update_vertices(self._h, int(geometry), xyz.ctypes.data_as(C.c_void_p), xyz.shape[0]))

    def update_vertices_device(self, geometry, device_ptr, num_vertices):
        """same from a device buffer (float32 xyz per unrolled vertex) written on the backend's stream."""
        self._check(self._L.rptr_hip_update_vertices_device(self._h, int(geometry), C.c_void_p(device_ptr), int(num_vertices)))

    def refit(self):
        self._check(self._L.rptr_hip_refit(self._h))

    # ---- moving instances (TLAS rebuild / update from the instance list, render_vulkan.cpp:1219-1354)
    def update_instances(self, first, transforms: np.ndarray):
        """New object-to-world transforms for scene instances [first, first + n): transforms is (n, 12) or (n, 3, 4) float32,
        row-major 3x4. Staged; the next refit() applies them."""
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        self._check(self._L.rptr_hip_update_instances(self._h, int(first), t.shape[0], t.ctypes.data_as(C.c_void_p)))

    def update_instances_device(self, first, device_ptr, count):
        """same from a device buffer (12 float32 per instance) written on the backend's stream."""
        self._check(self._L.rptr_hip_update_instances_device(self._h, int(first), int(count), C.c_void_p(device_ptr)))

    def set_tlas_policy(self, mode):
        """abi.TLAS_REBUILD (default): moved instances get a new top level built on the device; abi.TLAS_REFIT: the topology stays"""
        self._check(self._L.rptr_hip_set_tlas_policy(self._h, int(mode)))

    def tlas_rebuild_count(self):
        n = C.c_uint64()
        self._check(self._L.rptr_hip_tlas_rebuild_count(self._h, C.byref(n)))
        return int(n.value)

    # ---- moving lights (rptr_hip_set_light_sources): where RptrSceneDesc.lights came from, so that a refit can re-place them
    def set_light_sources(self, scene_or_array):
        """Register the provenance of the scene's lights: a scenes.Scene (its `light_sources`, filled by prepare_lights) or an array of
        lights.LIGHT_SOURCE_DTYPE, one record per light in the lights' order; None unregisters. Afterwards emissive instances may move
        and refit() re-places the lights. set_scene never registers on its own, and a new set_scene drops the registration."""
        from . import lights as L
        src = getattr(scene_or_array, "light_sources", scene_or_array)
        if src is None:
            self._check(self._L.rptr_hip_set_light_sources(self._h, None, 0))
            return
        src = np.ascontiguousarray(src, dtype=L.LIGHT_SOURCE_DTYPE).reshape(-1)
        self._check(self._L.rptr_hip_set_light_sources(self._h, src.ctypes.data_as(C.c_void_p) if len(src) else None, len(src)))

    def readback_lights(self, count=None):
        """The master scene copy's light buffer after all pending work: (n, 4, 3) float32 -- v0, v1, v2, radiance -- like Scene.lights.
        count: the scene's number of lights (default: that of the last set_scene)."""
        n = getattr(self, "_num_lights", 0) if count is None else int(count)
        out = np.zeros((n, 4, 3), dtype=np.float32)
        self._check(self._L.rptr_hip_readback_lights(self._h, out.ctypes.data_as(C.c_void_p), n))
        return out

    # ---- skinned meshes (rptr_hip_set_skin / update_bones / skin): bones in, positions and shading normals out on the device
    def set_skin(self, geometry, bones=None, weights=None):
        """Bind one geometry of a dynamic mesh: bones and weights are (n, 4) uint16, one row per UNROLLED vertex (n = 3 * triangles);
        a row's weights are unorm16 and sum to 65535. The rest pose is the geometry's positions now. bones=None unbinds."""
        if bones is None:
            self._check(self._L.rptr_hip_set_skin(self._h, int(geometry), None, 0))
            return
        rec = np.concatenate([np.ascontiguousarray(bones, dtype=np.uint16).reshape(-1, 4), np.ascontiguousarray(weights, dtype=np.uint16).reshape(-1, 4)], axis=1)
        rec = np.ascontiguousarray(rec)  # RptrSkinVertex: bone[4], weight[4]
        self._check(self._L.rptr_hip_set_skin(self._h, int(geometry), rec.ctypes.data_as(C.c_void_p) if len(rec) else None, len(rec)))

    def update_bones(self, first, transforms: np.ndarray):
        """Stage bone matrices [first, first + k): transforms is (k, 3, 4) or (k, 12) float32, row-major 3x4, rest object space to posed
        object space. The next skin() reads them."""
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        self._check(self._L.rptr_hip_update_bones(self._h, int(first), t.shape[0], t.ctypes.data_as(C.c_void_p)))

    def update_bones_device(self, first, device_ptr, count):
        """same from a device buffer (12 float32 per bone) written on the backend's stream."""
        self._check(self._L.rptr_hip_update_bones_device(self._h, int(first), int(count), C.c_void_p(device_ptr)))

    def skin(self):
        """Skin every bound geometry on the device; refit() afterwards, as after update_vertices."""
        self._check(self._L.rptr_hip_skin(self._h))

    def readback_skinned(self, geometry, num_vertices=None):
        """(xyz (n, 3) float32, normal words (n,) uint32 or None for a geometry without normals) of a geometry bound by a skin, morph targets
        or normal groups, after pending work."""
        geoms = getattr(self, "_geometries", [])
        tris, has_normals = geoms[int(geometry)] if 0 <= int(geometry) < len(geoms) else (0, False)
        n = 3 * tris if num_vertices is None else int(num_vertices)
        xyz = np.zeros((n, 3), dtype=np.float32)
        words = np.zeros(n, dtype=np.uint32) if has_normals else None
        self._check(self._L.rptr_hip_readback_skinned(self._h, int(geometry), xyz.ctypes.data_as(C.c_void_p),
                                                      words.ctypes.data_as(C.c_void_p) if has_normals else None, n))
        return xyz, words

    # ---- morph targets (rptr_hip_set_morph_targets / update_morph_weights): the stage in front of the skinner; skin() runs both
    @staticmethod
    def morph_deltas(vertex, dpos, dnrm=None):
        """one target as a numpy array of RptrMorphDelta records (abi.MORPH_DELTA_DTYPE)"""
        vertex = np.ascontiguousarray(vertex, dtype=np.uint32).reshape(-1)
        rec = np.zeros(len(vertex), dtype=abi.MORPH_DELTA_DTYPE)
        rec["vertex"] = vertex
        rec["dpos"] = np.asarray(dpos, dtype=np.float32).reshape(-1, 3)
        if dnrm is not None:
            rec["dnrm"] = np.asarray(dnrm, dtype=np.float32).reshape(-1, 3)
        return rec

    def set_morph_targets(self, geometry, targets=None):
        """Bind one geometry of a dynamic mesh: targets is a list of (vertex uint32[k], dpos float32[k, 3], dnrm float32[k, 3] or None),
        sparse -- a target lists the UNROLLED vertices it moves, each at most once, and may be empty. The weights start at zero. The rest
        pose is the geometry's positions now, or the one its skin captured. targets=None unbinds."""
        if targets is None:
            self._check(self._L.rptr_hip_set_morph_targets(self._h, int(geometry), None, 0))
            return
        recs = [self.morph_deltas(*t) for t in targets]  # (kept alive until the call returns)
        descs = (abi.MorphTargetDesc * max(len(recs), 1))()
        for d, rec in zip(descs, recs):
            d.deltas = C.cast(rec.ctypes.data, C.POINTER(abi.MorphDelta)) if len(rec) else None
            d.num_deltas = len(rec)
        self._check(self._L.rptr_hip_set_morph_targets(self._h, int(geometry), descs if recs else None, len(recs)))

    def update_morph_weights(self, geometry, first_target, weights):
        """Stage the weights of targets [first_target, first_target + k) of one geometry: a numpy array (checked: finite), or a torch
        device tensor of float32 written on the backend's stream (not checked: see "skin_vertices_rejected"). The next skin() reads them."""
        if hasattr(weights, "data_ptr") and getattr(weights, "is_cuda", False):
            assert str(weights.dtype) == "torch.float32" and weights.is_contiguous()
            self.update_morph_weights_device(geometry, first_target, weights.data_ptr(), weights.numel())
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self._check(self._L.rptr_hip_update_morph_weights(self._h, int(geometry), int(first_target), len(w), w.ctypes.data_as(C.c_void_p) if len(w) else None))

    def update_morph_weights_device(self, geometry, first_target, device_ptr, count):
        """same from a device buffer of float32 written on the backend's stream."""
        self._check(self._L.rptr_hip_update_morph_weights_device(self._h, int(geometry), int(first_target), int(count), C.c_void_p(device_ptr)))

    # ---- recomputed normals (rptr_hip_set_normal_groups / recompute_normals): shading normals from the positions as they are now
    def set_normal_groups(self, geometry, groups=None, flip=False):
        """Bind one geometry of a dynamic mesh that has normals: groups is (n,) uint32, one label per UNROLLED vertex (n = 3 * triangles);
        corners with the same label share one normal (the index buffer of the mesh that was unrolled, or scenes.normal_groups),
        abi.NORMAL_GROUP_FLAT gives a corner its triangle's face normal. flip: the mesh is wound the other way. groups=None unbinds."""
        if groups is None:
            self._check(self._L.rptr_hip_set_normal_groups(self._h, int(geometry), None, 0, 0))
            return
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        self._check(self._L.rptr_hip_set_normal_groups(self._h, int(geometry), g.ctypes.data_as(C.c_void_p) if len(g) else None, len(g),
                                                       abi.NORMALS_FLIP if flip else 0))

    def recompute_normals(self):
        """The normal words of every bound geometry from its current positions, on the device: after update_vertices* / skin(), before
        refit()."""
        self._check(self._L.rptr_hip_recompute_normals(self._h))

    # ---- dynamic textures (rptr_hip_update_texture / readback_texture / texture_levels): new texels in, mip chain made on the device
    def update_texture(self, index, rgba=None, generate_mips=True):
        """New level-0 texels for texture `index` of the scene: rgba is (height, width, 4) uint8 of the size set_scene received, as a
        numpy array or a CUDA / HIP torch uint8 tensor written on the backend's stream (the _device form: no host synchronisation).
        generate_mips: the full chain down to 1 x 1 is made on the device (scenes.generate_mips states the filter); without it the
        texture becomes level 0 only. rgba=None keeps level 0 and generates the chain. Waits for the frames in flight; every frame and
        query submitted afterwards sees the new texels. A texture an emissive material reads is refused (BackendError, UNSUPPORTED)."""
        flags = abi.TEXTURE_GENERATE_MIPS if generate_mips else 0
        if rgba is None:
            self._check(self._L.rptr_hip_update_texture(self._h, int(index), None, 0, flags))
        elif hasattr(rgba, "data_ptr") and getattr(rgba, "is_cuda", False):
            assert str(rgba.dtype) == "torch.uint8" and rgba.is_contiguous()
            self._check(self._L.rptr_hip_update_texture_device(self._h, int(index), C.c_void_p(rgba.data_ptr()), rgba.numel(), flags))
        else:
            a = np.ascontiguousarray(rgba, dtype=np.uint8)
            self._check(self._L.rptr_hip_update_texture(self._h, int(index), a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, flags))

    def texture_levels(self, index):
        """the levels of texture `index` a sampler may read now"""
        n = C.c_uint32(0)
        self._check(self._L.rptr_hip_texture_levels(self._h, int(index), C.byref(n)))
        return int(n.value)

    def readback_texture(self, index, level=0):
        """(max(1, height >> level), max(1, width >> level), 4) uint8: one level of texture `index` as the device holds it, after pending work"""
        tex = getattr(self, "_textures", [])
        h, w = tex[int(index)] if 0 <= int(index) < len(tex) else (0, 0)
        out = np.zeros((max(1, h >> int(level)) if h else 0, max(1, w >> int(level)) if w else 0, 4), np.uint8)
        self._check(self._L.rptr_hip_readback_texture(self._h, int(index), int(level), out.ctypes.data_as(C.c_void_p) if out.size else None, out.size))
        return out

    def set_rng_variant(self, rng_variant, table=None):
        """RenderBackendOptions::rng_variant (render_params.glsl.h:34-37,76) + the table upload of the point set's render extension
        (vulkan/pointsets/render_{sobol,bn}.cpp). table: uint32 array laid out as SobolData / BNData; None = `pointsets.default_table`."""
        from . import pointsets
        if table is None:
            table = pointsets.default_table(rng_variant)
        if table is None:
            self._check(self._L.rptr_hip_set_rng_variant(self._h, int(rng_variant), None, 0))
        else:
            t = np.ascontiguousarray(table, dtype=np.uint32)
            self._check(self._L.rptr_hip_set_rng_variant(self._h, int(rng_variant), t.ctypes.data_as(C.c_void_p), t.nbytes))
        self.rng_variant = int(rng_variant)

    def set_bvh_policy(self, force_bvh_rebuild=False, rebuild_triangle_budget=0):
        """RenderBackendOptions::force_bvh_rebuild / rebuild_triangle_budget (render_params.glsl.h:61,90-93): device-side rebuilds of
        dynamic meshes instead of refits (include/rptr_hip.h)"""
        self._check(self._L.rptr_hip_set_bvh_policy(self._h, 1 if force_bvh_rebuild else 0, int(rebuild_triangle_budget)))

    def bvh_build_info(self):
        """(built on the device?, milliseconds of set_scene's acceleration-structure step, GPU milliseconds of its device builds)"""
        dev, ms, dms = C.c_int32(), C.c_float(), C.c_float()
        self._check(self._L.rptr_hip_bvh_build_info(self._h, C.byref(dev), C.byref(ms), C.byref(dms)))
        return bool(dev.value), float(ms.value), float(dms.value)

    def traversal_preset(self):
        """(surface-area cost of the scene's tree, node_min, refill_min): the traversal's scheduling thresholds for this scene (0 = defaults)"""
        cost, nm, rm = C.c_float(), C.c_int32(), C.c_int32()
        self._check(self._L.rptr_hip_traversal_preset(self._h, C.byref(cost), C.byref(nm), C.byref(rm)))
        return float(cost.value), int(nm.value), int(rm.value)

    def bvh_rebuild_count(self):
        n = C.c_uint64()
        self._check(self._L.rptr_hip_bvh_rebuild_count(self._h, C.byref(n)))
        return int(n.value)

    # ---- the RCCL gather of tile radiance (include/rptr_hip.h "multi-GPU"; csrc/host_comm.h)
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128 bytes every rank of a one-process-per-GPU job hands to comm_init_rank (ncclGetUniqueId)"""
        L = load_library()
        buf = C.create_string_buffer(abi.COMM_ID_BYTES)
        rc = L.rptr_hip_comm_get_unique_id(buf)
        if rc != 0:
            raise BackendError(rc, L.rptr_hip_last_error(None).decode())
        return buf.raw

    def comm_init_rank(self, unique_id: bytes):
        """collective over all ranks of the job (one process per GPU): joins the communicator as RptrCreateInfo.rank"""
        assert len(unique_id) == abi.COMM_ID_BYTES
        self._check(self._L.rptr_hip_comm_init_rank(self._h, C.c_char_p(unique_id)))

    def comm_ipc_export(self):
        """rank 0 of a one-process-per-GPU job: makes the peer-write (IPC) communicator and returns the bytes every rank hands to
        comm_ipc_init (hipIpcGetMemHandle of rank 0's frame buffers and flag block)"""
        buf = C.create_string_buffer(abi.COMM_IPC_BYTES)
        self._check(self._L.rptr_hip_comm_ipc_export(self._h, buf))
        return buf.raw

    def comm_ipc_init(self, blob: bytes):
        assert len(blob) == abi.COMM_IPC_BYTES
        self._check(self._L.rptr_hip_comm_ipc_init(self._h, C.c_char_p(blob)))

    @staticmethod
    def _handle_array(renderers):
        arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
        return arr

    @staticmethod
    def comm_init_all(renderers):
        """one process, len(renderers) handles: renderers[i] is rank i of the frame"""
        rc = renderers[0]._L.rptr_hip_comm_init_all(RenderHip._handle_array(renderers), len(renderers))
        if rc != 0:
            msgs = [r._L.rptr_hip_last_error(r._h).decode() for r in renderers]
            raise BackendError(rc, "; ".join(m for m in msgs if m) or renderers[0]._L.rptr_hip_last_error(None).decode())

    def gather(self, n_frames=1):
        """this rank's part of the gather (asynchronous; call right after wait()). n_frames > 1: ONE collective for the last n_frames
        frames of the launch sequence whose last ticket was just waited for"""
        self._check(self._L.rptr_hip_gather_batch(self._h, int(n_frames)))

    @staticmethod
    def gather_all(renderers, n_frames=1):
        rc = renderers[0]._L.rptr_hip_gather_all_batch(RenderHip._handle_array(renderers), len(renderers), int(n_frames))
        if rc != 0:
            msgs = [r._L.rptr_hip_last_error(r._h).decode() for r in renderers]
            raise BackendError(rc, "; ".join(m for m in msgs if m))

    def comm_transport(self):
        """what this handle's communicator moves rows with: "rccl", "copy" or "peer" (None without a communicator)"""
        t = self._L.rptr_hip_comm_transport(self._h)
        return t.decode() if t else None

    def gathered_frame_ptr(self):
        p = C.c_void_p()
        self._check(self._L.rptr_hip_gathered_frame(self._h, C.byref(p)))
        return p.value

    def readback_gathered(self, buffer: np.ndarray, index=None):
        """rank 0: the assembled RGBA32F frame of the last gather (waits for it); index: frame k of a batched gather (default: its
        last). Returns #elements or 0."""
        w, hgt, c = self.get_framebuffer_size()
        if buffer.size < w * hgt * c or buffer.dtype != np.float32:
            return 0
        if index is None:
            self._check(self._L.rptr_hip_readback_gathered_f32(self._h, buffer.ctypes.data_as(C.c_void_p), buffer.size))
        else:
            self._check(self._L.rptr_hip_readback_gathered_frame_f32(self._h, int(index), buffer.ctypes.data_as(C.c_void_p), buffer.size))
        return w * hgt * c

    def comm_stats(self):
        n, ms = C.c_uint64(), C.c_float()
        self._check(self._L.rptr_hip_comm_stats(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def comm_destroy(self):
        self._check(self._L.rptr_hip_comm_destroy(self._h))

    def copy_tile_to_device(self, device_ptr, n_bytes):
        self._check(self._L.rptr_hip_copy_tile_to_device(self._h, C.c_void_p(device_ptr), n_bytes))

    def set_stream(self, hip_stream):
        self._check(self._L.rptr_hip_set_stream(self._h, C.c_void_p(hip_stream)))

    # ---- diagnostics
    def export_bvh(self):
        nn, nt, ni = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.rptr_hip_export_bvh(self._h, None, C.byref(nn), None, C.byref(nt), None, C.byref(ni)))
        nodes = np.zeros(max(nn.value, 1) * 16, dtype=np.float32)
        tris = np.zeros(max(nt.value, 1) * 12, dtype=np.float32)
        insts = np.zeros(max(ni.value, 1) * 32, dtype=np.float32)
        self._check(self._L.rptr_hip_export_bvh(self._h, nodes.ctypes.data_as(C.c_void_p), C.byref(nn), tris.ctypes.data_as(C.c_void_p),
                                                C.byref(nt), insts.ctypes.data_as(C.c_void_p), C.byref(ni)))
        return nodes[:nn.value * 16], tris[:nt.value * 12], insts[:ni.value * 32]
