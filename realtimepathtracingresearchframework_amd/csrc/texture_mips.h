// texture_mips.h -- dynamic textures: the mip chain of an RGBA8 texture made on the device (include/rptr_hip.h "dynamic textures").
// The sampler (dshade.h rp_texture_grad / rp_texture_lod) filters the levels it is given; nothing made one. rp_k_mip_level makes level
// l + 1 from the QUANTISED level l, one launch per level in stream order, into the storage the sampler reads (levels back to back).
// The reference generates no mip levels, so the rule below is the definition; tests/texture_mips_ref.py and scenes.generate_mips state
// it in numpy float32, and the tests compare bit for bit.
//
// Sizes: a source of h x w texels gives max(1, h >> 1) x max(1, w >> 1).
// Taps per axis of source size n at destination coordinate x (source index, integer weight), and their total:
//   n == 1                  (0, 1)                                            total 1
//   n even                  (2x, 1), (2x + 1, 1)                              total 2
//   n odd >= 3, m = n >> 1  (2x, m - x), (2x + 1, m), (2x + 2, x + 1)         total n    (the exact-area box: nothing dropped or shifted)
// Arithmetic per channel: binary32, every product, sum and quotient rounded on its own (-ffp-contract=off; IEEE division, as in skin.h,
// morph.h and normals.h).
//   f(c)  = srgb_lut[c] for the colour channels of an sRGB texture, float(c) for alpha and every channel of a linear texture
//   acc   = 0;  for ty in row order, tx in column order:  acc = acc + float(wx * wy) * f(texel[ty][tx])      (wx * wy an integer product)
//   mean  = acc / float(totx * toty)                                                                        (an integer product)
//   linear code: min(255, int(mean + 0.5f))
//   sRGB code:   the number of k in 1..255 with mean >= T[k],  T[k] = (lut[k - 1] + lut[k]) * 0.5f
// T is built on the host from the table set_scene uploads (rp_srgb_thresholds) and uploaded beside it: the device evaluates no
// transcendental function, and the encode is an 8-step search over the increasing T.
//
// One lane per destination texel, lanes along x: one uchar4 store and 1-9 uchar4 loads per lane (the two horizontal taps of an even
// row come as ONE 8-byte load where the level's base address allows it: neighbouring lanes then read neighbouring 8 bytes). The table and
// the thresholds (2 KB) are staged in LDS once per block. profiles/texture_mips_notes.md has the measurements.
#pragma once
#include "dshade.h"

// T[0] is never read by the search (it is 0); T[k] as above. `lut` is rp_srgb_decode_lut's table.
static inline void rp_srgb_thresholds(const float lut[256], float T[256]) {
    T[0] = 0.0f;
    for (int k = 1; k < 256; ++k) T[k] = (lut[k - 1] + lut[k]) * 0.5f;
}

#ifdef __HIPCC__
// the taps of one axis: first source index, up to three integer weights, how many of them count
struct RpMipTaps {
    uint32_t first, n, w[3];
};
RP_DEV RpMipTaps rp_mip_taps(uint32_t size, uint32_t x) {
    if (size == 1u) return RpMipTaps{0u, 1u, {1u, 0u, 0u}};
    if ((size & 1u) == 0u) return RpMipTaps{2u * x, 2u, {1u, 1u, 0u}};
    const uint32_t m = size >> 1;
    return RpMipTaps{2u * x, 3u, {m - x, m, x + 1u}};
}
RP_DEV uint32_t rp_mip_total(uint32_t size) { return (size & 1u) ? size : 2u; } // the sum of an axis's weights: 1, 2 or n
RP_DEV uint32_t rp_mip_encode_srgb(const float *T, float mean) { // the number of k in 1..255 with mean >= T[k]
    uint32_t code = 0;
#pragma unroll
    for (uint32_t step = 128u; step; step >>= 1)
        if (mean >= T[code + step]) code += step; // (code + step <= 255)
    return code;
}
RP_DEV uint32_t rp_mip_encode_linear(float mean) { return (uint32_t)min(255, int(mean + 0.5f)); }

// the record of one texture in RpScene::textures, patched in stream order behind the texels it describes
__global__ void rp_k_set_texture_record(RpTexture *record, RpTexture value) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *record = value;
}

// src: sh x sw texels; dst: max(1, sh >> 1) x max(1, sw >> 1). PAIR: sw is even and src is 8-byte aligned.
template <bool PAIR>
__global__ __launch_bounds__(256) void rp_k_mip_level(const uchar4 *src, uchar4 *dst, uint32_t sw, uint32_t sh, uint32_t srgb, const float *srgb_lut,
                                                      const float *srgb_thresholds) {
    __shared__ float s_lut[256], s_thr[256];
    if (srgb) { // (uniform over the launch)
        s_lut[threadIdx.x] = srgb_lut[threadIdx.x];
        s_thr[threadIdx.x] = srgb_thresholds[threadIdx.x];
        __syncthreads();
    }
    const uint32_t dw = max(1u, sw >> 1), dh = max(1u, sh >> 1), n = dw * dh; // (sizes are at most 16384: n <= 2^26)
    const float total = float(rp_mip_total(sw) * rp_mip_total(sh)); // converted once (16383^2 < 2^32)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t y = i / dw, x = i - y * dw;
        const RpMipTaps tx = rp_mip_taps(sw, x), ty = rp_mip_taps(sh, y);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t r = 0; r < ty.n; ++r) {
            const uchar4 *row = src + (size_t)(ty.first + r) * sw + tx.first; // (ty.first + r < sh and tx.first + c < sw by the tap table)
            uchar4 t[3];
            if (PAIR) {
                const uint2 two = *reinterpret_cast<const uint2 *>(row);
                t[0] = *reinterpret_cast<const uchar4 *>(&two.x);
                t[1] = *reinterpret_cast<const uchar4 *>(&two.y);
            } else {
                for (uint32_t c = 0; c < tx.n; ++c) t[c] = row[c];
            }
            for (uint32_t c = 0; c < tx.n; ++c) {
                const float w = float(tx.w[c] * ty.w[r]);
                const float a = float(t[c].w);
                const float f[4] = {srgb ? s_lut[t[c].x] : float(t[c].x), srgb ? s_lut[t[c].y] : float(t[c].y), srgb ? s_lut[t[c].z] : float(t[c].z), a};
                for (int k = 0; k < 4; ++k) {
                    const float p = w * f[k];
                    acc[k] = acc[k] + p;
                }
            }
        }
        const float mean[4] = {acc[0] / total, acc[1] / total, acc[2] / total, acc[3] / total};
        uchar4 out;
        out.x = (unsigned char)(srgb ? rp_mip_encode_srgb(s_thr, mean[0]) : rp_mip_encode_linear(mean[0]));
        out.y = (unsigned char)(srgb ? rp_mip_encode_srgb(s_thr, mean[1]) : rp_mip_encode_linear(mean[1]));
        out.z = (unsigned char)(srgb ? rp_mip_encode_srgb(s_thr, mean[2]) : rp_mip_encode_linear(mean[2]));
        out.w = (unsigned char)rp_mip_encode_linear(mean[3]);
        dst[i] = out;
    }
}
#endif
