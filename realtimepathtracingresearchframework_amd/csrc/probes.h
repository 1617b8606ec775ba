// probes.h -- irradiance probes: positions in, second-order spherical-harmonics coefficients of the incident radiance out
// (include/rptr_hip.h "irradiance probes"). Two kernels around a radiance-query run (host_frame.inl radiance_queries_on): rp_k_probe_rays
// writes K query records per probe, rp_k_probe_project folds the K float4 ray values of a probe into 9 x 4 coefficients.
//
// Data: the direction set is a table of K float3 the HOST computes (rptr_hip_probe_directions: spherical Fibonacci in double, rounded
// once); the device evaluates no transcendental function. Both kernels rotate a table entry the same way, so the projection needs the 16
// bytes of a ray's value and not its 32-byte record.
//
// Arithmetic: binary32, every product and sum rounded on its own (-ffp-contract=off), IEEE division; the temporaries keep the association
// explicit. tests/probes_ref.py states the same operations in numpy float32, and the tests compare bit for bit.
//   ray q = p K + k:  origin = pos[p];  dir[r] = (R[r][0] x + R[r][1] y) + R[r][2] z  of d_k = (x, y, z), not renormalised;
//                     mode_or_data = 0, or -1 when a coordinate of pos[p] is not finite (the whole probe is skipped)
//   value:            a component of the float4 not finite -> (0, 0, 0, 0);  clamp > 0 and m = max(r, g, b) > clamp -> rgb = rgb (clamp / m)
//   basis (x, y, z = the rotated direction):  Y0 = 0.282095, Y1 = 0.488603 y, Y2 = 0.488603 z, Y3 = 0.488603 x, Y4 = 1.092548 (x y),
//                     Y5 = 1.092548 (y z), Y6 = 0.315392 (3 (z z) - 1), Y7 = 1.092548 (x z), Y8 = 0.546274 (x x - y y)
//   sum:              one 64-lane wave per probe; lane l starts from +0 and takes k = l, l + 64, ... ascending:
//                     acc[i][ch] = acc[i][ch] + v[ch] Y_i;  then acc = acc + xor-shuffle(acc, off) for off = 32, 16, 8, 4, 2, 1 (IEEE addition
//                     commutes: every lane ends with the same bits);  c_new = acc w,  w = float(4 pi / K)
//   blend:            blend == 1: c = c_new (a plain store);  otherwise c = c + (c_new - c) blend
#pragma once
#include "kernels.h"

static_assert(sizeof(RptrProbeParams) == 80, "RptrProbeParams is 80 bytes");

struct RpProbeConst {
    float rot[9]; // row-major
    float t_max;
    float clamp;
    float blend;
    float weight; // float(4 pi / K)
    uint32_t K;
};

RP_DEV bool rp_probe_usable(const float *pos3, uint32_t p) {
    return isfinite(pos3[3ull * p]) && isfinite(pos3[3ull * p + 1]) && isfinite(pos3[3ull * p + 2]);
}
RP_DEV void rp_probe_direction(const RpProbeConst &c, const float *dirs, uint32_t k, float &x, float &y, float &z) {
    const float dx = dirs[3u * k], dy = dirs[3u * k + 1], dz = dirs[3u * k + 2];
    const float a0 = c.rot[0] * dx, b0 = c.rot[1] * dy, c0 = c.rot[2] * dz;
    const float a1 = c.rot[3] * dx, b1 = c.rot[4] * dy, c1 = c.rot[5] * dz;
    const float a2 = c.rot[6] * dx, b2 = c.rot[7] * dy, c2 = c.rot[8] * dz;
    x = (a0 + b0) + c0;
    y = (a1 + b1) + c1;
    z = (a2 + b2) + c2;
}

// One thread per ray, grid-stride; the record is two 16-byte stores. n_rays = n_probes * K < 2^31 (the host checks).
__global__ __launch_bounds__(256) void rp_k_probe_rays(const float *pos3, uint32_t n_rays, RpProbeConst c, const float *dirs, float4 *records) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_rays; q += gridDim.x * blockDim.x) {
        const uint32_t p = q / c.K, k = q - p * c.K;
        float x, y, z;
        rp_probe_direction(c, dirs, k, x, y, z);
        const int mode = rp_probe_usable(pos3, p) ? 0 : -1;
        records[2ull * q] = make_float4(pos3[3ull * p], pos3[3ull * p + 1], pos3[3ull * p + 2], __int_as_float(mode));
        records[2ull * q + 1] = make_float4(x, y, z, c.t_max);
    }
}

// One wave per probe, the waves grid-stride over the probes. Per lane 36 accumulators, 9 basis values and one float4 in flight: no
// scratch at the default register budget of a 256-thread block. Loads: 16 bytes of value and 12 of table per ray (the table is shared by
// every probe: cache hits), with a blend below 1 the 144 bytes of old coefficients; stores: 144 bytes per probe, nine lanes a float4 each.
// pos3 != NULL: a probe with a coordinate that is not finite keeps its coefficients.
__global__ __launch_bounds__(256) void rp_k_probe_project(const float4 *values, const float *pos3, uint32_t n_probes, RpProbeConst c, const float *dirs, float4 *coeffs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < n_probes; p += waves) {
        if (pos3 && !rp_probe_usable(pos3, p)) continue; // (the same for every lane of the wave)
        float acc[9][4];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
        const float4 *row = values + (size_t)p * c.K;
        for (uint32_t k = lane; k < c.K; k += 64u) {
            const float4 in = row[k];
            float v[4] = {in.x, in.y, in.z, in.w};
            if (!(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]))) v[0] = v[1] = v[2] = v[3] = 0.0f;
            const float m = fmaxf(fmaxf(v[0], v[1]), v[2]);
            if (c.clamp > 0.0f && m > c.clamp) {
                const float s = c.clamp / m;
                v[0] = v[0] * s, v[1] = v[1] * s, v[2] = v[2] * s;
            }
            float x, y, z;
            rp_probe_direction(c, dirs, k, x, y, z);
            const float xy = x * y, yz = y * z, zz = z * z, xz = x * z, xx = x * x, yy = y * y;
            const float zz3 = 3.0f * zz;
            const float Y[9] = {0.282095f,      0.488603f * y,           0.488603f * z,  0.488603f * x,          1.092548f * xy,
                                1.092548f * yz, 0.315392f * (zz3 - 1.0f), 1.092548f * xz, 0.546274f * (xx - yy)};
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const float t = v[ch] * Y[i];
                    acc[i][ch] = acc[i][ch] + t;
                }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) acc[i][ch] = acc[i][ch] + __shfl_xor(acc[i][ch], off, 64);
        float4 *out = coeffs + 9ull * p;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (lane != (uint32_t)i) continue;
            float n[4] = {acc[i][0] * c.weight, acc[i][1] * c.weight, acc[i][2] * c.weight, acc[i][3] * c.weight};
            if (c.blend != 1.0f) {
                const float4 old = out[i];
                const float o[4] = {old.x, old.y, old.z, old.w};
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const float d = n[ch] - o[ch];
                    const float e = d * c.blend;
                    n[ch] = o[ch] + e;
                }
            }
            out[i] = make_float4(n[0], n[1], n[2], n[3]);
        }
    }
}
