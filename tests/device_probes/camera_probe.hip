// camera_probe.hip -- TEST INFRASTRUCTURE: the camera ray of csrc/kernels.h on chosen frame constants.
//
// One lane per path id of a launch sequence calls rp_primary_ray_ex<true> -- the function the first extend and the first shade of the
// general kernel instantiations call, nothing of it is restated here -- and stores the ray's origin and direction, the generator state after
// the call and the pixel / sample slot the path belongs to. The frame constants are filled as csrc/host_frame.inl fill_frame_constants and
// rptr_hip_initialize fill them for one rank (world_size 1, stripes of 32 rows); the camera bases come from the caller (tests/dof_ref.py
// camera_basis), so that the model and the device start from the same float bits.
//
// Built by tests/device_probes/camera.py with the product's compiler flags: libcamera_probe.so. Not part of librptr_hip.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "kernels.h"

#define CP_TRY(expr)                                                                                                                   \
    do {                                                                                                                               \
        const hipError_t e_ = (expr);                                                                                                  \
        if (e_ != hipSuccess) {                                                                                                        \
            fprintf(stderr, "camera_probe: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);              \
            rc = 1;                                                                                                                    \
            goto done;                                                                                                                 \
        }                                                                                                                              \
    } while (0)

extern "C" {
struct CpArgs {
    int32_t width, height;
    int32_t frame_spp, n_frames, batch_reset; // sample slots per frame, frames of the launch sequence, frames 1.. restart the accumulation
    uint32_t frame_offset, sample_base, frame_id;
    int32_t rng_variant;        // RPTR_RNG_VARIANT_*
    int32_t enable_raster_taa;
    float aperture_radius, focus_distance;
    int32_t per_frame_cams;     // 0: cams[0] serves every frame
    int32_t _pad;
    float cams[RP_BATCH_CAMS][12]; // pos, du, dv, dir_top_left
};
}

namespace {
__global__ void k_primary_rays(RpFrame f, uint32_t n, float *origin3, float *dir3, uint32_t *state, int32_t *pixel3) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    RpRng rng;
    rng.s = rng.index = rng.pix = 0u;
    V3 dir = v3s(0.0f), origin = v3s(0.0f);
    int lx = 0, ly = 0;
    uint32_t sslot = 0u;
    const bool present = rp_primary_ray_ex<true>(f, p, rng, dir, lx, ly, sslot, origin);
    origin3[3 * p] = origin.x, origin3[3 * p + 1] = origin.y, origin3[3 * p + 2] = origin.z;
    dir3[3 * p] = dir.x, dir3[3 * p + 1] = dir.y, dir3[3 * p + 2] = dir.z;
    state[p] = rng.s;
    pixel3[3 * p] = present ? lx : -1; // (tile padding: no pixel sample)
    pixel3[3 * p + 1] = present ? rp_local_row_to_global(f, ly) : -1;
    pixel3[3 * p + 2] = int32_t(sslot);
}

void fill_frame(const CpArgs &a, const uint32_t *d_table, RpFrame &f) {
    memset(&f, 0, sizeof(f));
    f.rp.aperture_radius = a.aperture_radius;
    f.rp.focus_distance = a.focus_distance;
    f.rp.enable_raster_taa = a.enable_raster_taa;
    f.rp.max_path_depth = 1;
    memcpy(f.cam_pos, a.cams[0], 12);
    memcpy(f.cam_du, a.cams[0] + 3, 12);
    memcpy(f.cam_dv, a.cams[0] + 6, 12);
    memcpy(f.cam_dir_top_left, a.cams[0] + 9, 12);
    f.per_frame_cams = a.per_frame_cams;
    for (int k = 0; k < RP_BATCH_CAMS; ++k) {
        memcpy(f.cams[k].pos, a.cams[k], 12);
        memcpy(f.cams[k].du, a.cams[k] + 3, 12);
        memcpy(f.cams[k].dv, a.cams[k] + 6, 12);
        memcpy(f.cams[k].dir_top_left, a.cams[k] + 9, 12);
    }
    f.frame_offset = a.frame_offset;
    f.sample_base = a.sample_base;
    f.frame_id = a.frame_id;
    f.batch_frames = a.n_frames;
    f.frame_spp = a.frame_spp;
    f.batch_spp = a.n_frames * a.frame_spp;
    f.batch_reset = a.batch_reset;
    f.div_frame_spp = rp_make_div((uint32_t)a.frame_spp);
    f.width = a.width;
    f.height = a.height;
    f.local_rows = a.height;
    f.tiles_x = ((a.width + 7) / 8 + RP_TILE_BLOCK - 1) / RP_TILE_BLOCK * RP_TILE_BLOCK;
    f.tiles_y = ((a.height + 7) / 8 + RP_TILE_BLOCK - 1) / RP_TILE_BLOCK * RP_TILE_BLOCK;
    f.npix_padded = f.tiles_x * f.tiles_y * 64;
    f.rank = 0;
    f.world = 1;
    f.stripe_rows = 32;
    f.div_npix_padded = rp_make_div((uint32_t)f.npix_padded);
    f.div_tiles_x = rp_make_div((uint32_t)(f.tiles_x / RP_TILE_BLOCK));
    f.div_stripe_rows = rp_make_div((uint32_t)f.stripe_rows);
    f.div_width = rp_make_div((uint32_t)f.width);
    f.rng_variant = a.rng_variant;
    f.rng_table = d_table;
}
bool valid(const CpArgs &a) {
    return a.width >= 1 && a.height >= 1 && a.width <= 4096 && a.height <= 4096 && a.frame_spp >= 1 && a.n_frames >= 1 && a.n_frames <= RP_BATCH_CAMS &&
           a.frame_spp * a.n_frames <= 64;
}
} // namespace

extern "C" {
// path ids of the launch sequence: the size (in paths) of every output array of cp_primary_rays
int cp_path_count(const CpArgs *a) {
    if (!a || !valid(*a)) return -1;
    RpFrame f;
    fill_frame(*a, nullptr, f);
    return f.npix_padded * f.batch_spp;
}
// table / table_words: the point set's table as rptr_hip_set_rng_variant takes it (NULL / 0 with the uniform generator).
// origin3, dir3: 3 floats per path; state: the generator's `s` after the call; pixel3: (x, y, sample slot), x = y = -1 for tile padding.
int cp_primary_rays(const CpArgs *a, const uint32_t *table, size_t table_words, float *origin3, float *dir3, uint32_t *state, int32_t *pixel3) {
    if (!a || !valid(*a) || !origin3 || !dir3 || !state || !pixel3) return 2;
    if (a->rng_variant != RPTR_RNG_VARIANT_UNIFORM) { // the whole table of the point set, as the library insists on (every index the draws form lies inside it)
        const size_t need = a->rng_variant == RPTR_RNG_VARIANT_BN ? size_t(RP_BN_SAMPLES) * RP_BN_DIMS + size_t(RP_BN_TILE) * RP_BN_TILE * RP_BN_SCR_DIMS
                                                                  : size_t(RP_SOBOL_DIMS) * RP_SOBOL_BITS + size_t(RP_SOBOL_TILE) * RP_SOBOL_TILE;
        if (!table || table_words < need) return 2;
    }
    int rc = 0;
    uint32_t *d_table = nullptr, *d_state = nullptr;
    float *d_origin = nullptr, *d_dir = nullptr;
    int32_t *d_pixel = nullptr;
    RpFrame f;
    fill_frame(*a, nullptr, f);
    const size_t n = (size_t)f.npix_padded * (size_t)f.batch_spp;
    if (table && table_words) {
        CP_TRY(hipMalloc(&d_table, table_words * sizeof(uint32_t)));
        CP_TRY(hipMemcpy(d_table, table, table_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    f.rng_table = d_table;
    CP_TRY(hipMalloc(&d_origin, n * 3 * sizeof(float)));
    CP_TRY(hipMalloc(&d_dir, n * 3 * sizeof(float)));
    CP_TRY(hipMalloc(&d_state, n * sizeof(uint32_t)));
    CP_TRY(hipMalloc(&d_pixel, n * 3 * sizeof(int32_t)));
    k_primary_rays<<<unsigned((n + 255) / 256), 256>>>(f, (uint32_t)n, d_origin, d_dir, d_state, d_pixel);
    CP_TRY(hipGetLastError());
    CP_TRY(hipDeviceSynchronize());
    CP_TRY(hipMemcpy(origin3, d_origin, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    CP_TRY(hipMemcpy(dir3, d_dir, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    CP_TRY(hipMemcpy(state, d_state, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CP_TRY(hipMemcpy(pixel3, d_pixel, n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
done:
    (void)hipFree(d_table);
    (void)hipFree(d_origin);
    (void)hipFree(d_dir);
    (void)hipFree(d_state);
    (void)hipFree(d_pixel);
    return rc;
}
}
