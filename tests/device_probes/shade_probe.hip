// shade_probe.hip -- TEST INFRASTRUCTURE: the device shading functions of csrc/dshade.h on chosen inputs.
//
// Every probe calls the very RP_DEV functions the path-tracing kernels call (nothing here restates a function body); one kernel per probe
// group, one lane per input element. The extern "C" entry points take host arrays -- where the CPU oracle has a probe, in its argument
// layout (oracle/oracle.cpp), so that one numpy input set feeds both -- and allocate, copy, launch, synchronise and copy back. Every HIP
// call is checked: an entry point returns non-zero and prints the failing call on stderr.
//
// Built twice by tests/device_probes (-DRP_FAST_MATH=0 / 1, the product's compiler flags): libshade_probe.so, libshade_probe_fast.so.
// Not part of librptr_hip.so.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "dshade.h"

#define SP_TRY(expr)                                                                                                                   \
    do {                                                                                                                               \
        const hipError_t e_ = (expr);                                                                                                  \
        if (e_ != hipSuccess) {                                                                                                        \
            fprintf(stderr, "shade_probe: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);               \
            return 1;                                                                                                                  \
        }                                                                                                                              \
    } while (0)

namespace {

// device buffers of one call, freed when the call returns
struct Buffers {
    std::vector<void *> ptrs;
    ~Buffers() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T>
    int alloc(T *&d, size_t count) {
        d = nullptr;
        void *p = nullptr;
        SP_TRY(hipMalloc(&p, count * sizeof(T) > 0 ? count * sizeof(T) : 4));
        ptrs.push_back(p);
        d = static_cast<T *>(p);
        return 0;
    }
    template <class T>
    int in(const T *&d, const T *h, size_t count) { // device copy of a host array
        T *p = nullptr;
        if (alloc(p, count)) return 1;
        d = p;
        if (count) SP_TRY(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
};
template <class T>
int copy_out(T *h, const T *d, size_t count) {
    if (count) SP_TRY(hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
int launched(const char *what) {
    SP_TRY(hipGetLastError());
    SP_TRY(hipDeviceSynchronize());
    (void)what;
    return 0;
}
constexpr int kBlock = 256;
inline unsigned blocks(int n) { return unsigned((n + kBlock - 1) / kBlock); }

RP_DEV V3 ldv(const float *p, int i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
RP_DEV void stv(float *p, int i, V3 v) { p[3 * i] = v.x, p[3 * i + 1] = v.y, p[3 * i + 2] = v.z; }

// ---- glTF / glTF + transmission: rp_sample_gltf[_t]_brdf with the basis rp_ortho_basis gives (as the shade kernels and
// oracle.cpp gltf_sample_probe), then f and the MIS pdf at the sampled direction when the pdf is positive
template <int VARIANT>
__global__ void k_gltf_sample(RptrBaseMaterial p, const float *n3, const float *wo3, const float *u4, int n, float *wi3, float *weight3,
                              float *pdf, float *mis_pdf, float *f3, float *wpdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RpScene sc{};
    RpMaterial m;
    V3 emit;
    rp_unpack_material<VARIANT, false>(sc, m, emit, p, rp_texcoord(v2(0.0f, 0.0f)));
    const V3 nn = ldv(n3, i), wo = ldv(wo3, i);
    V3 vx, vy;
    rp_ortho_basis(vx, vy, nn);
    V3 wi = v3s(0.0f);
    float pp = 0.0f, mp = 0.0f;
    const V2 ud = v2(u4[4 * i], u4[4 * i + 1]), ul = v2(u4[4 * i + 2], u4[4 * i + 3]);
    const V3 w = VARIANT == RPTR_VARIANT_GLTF_TRANSMISSION ? rp_sample_gltf_t_brdf(m, nn, wo, wi, pp, mp, ud, ul, vx, vy)
                                                           : rp_sample_gltf_brdf(m, nn, wo, wi, pp, mp, ud, ul, vx, vy);
    stv(wi3, i, wi);
    stv(weight3, i, w);
    pdf[i] = pp;
    mis_pdf[i] = mp;
    stv(f3, i, pp > 0.0f ? rp_eval_bsdf<VARIANT>(m, nn, wo, wi) : v3s(0.0f));
    wpdf[i] = pp > 0.0f ? rp_eval_bsdf_wpdf<VARIANT>(m, nn, wo, wi) : 0.0f;
}
template <int VARIANT>
__global__ void k_gltf_eval(RptrBaseMaterial p, const float *n3, const float *wo3, const float *wi3, int n, float *f3, float *wpdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RpScene sc{};
    RpMaterial m;
    V3 emit;
    rp_unpack_material<VARIANT, false>(sc, m, emit, p, rp_texcoord(v2(0.0f, 0.0f)));
    const V3 nn = ldv(n3, i), wo = ldv(wo3, i), wi = ldv(wi3, i);
    stv(f3, i, rp_eval_bsdf<VARIANT>(m, nn, wo, wi));
    wpdf[i] = rp_eval_bsdf_wpdf<VARIANT>(m, nn, wo, wi);
}
template <int VARIANT>
int gltf_sample(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *u4, int n, float *wi3, float *weight3, float *pdf,
                float *mis_pdf, float *f3, float *wpdf) {
    Buffers b;
    const float *dn, *dwo, *du;
    float *dwi, *dw, *dp, *dm, *df, *dq;
    if (b.in(dn, n3, 3 * n) || b.in(dwo, wo3, 3 * n) || b.in(du, u4, 4 * n) || b.alloc(dwi, 3 * n) || b.alloc(dw, 3 * n) || b.alloc(dp, n) ||
        b.alloc(dm, n) || b.alloc(df, 3 * n) || b.alloc(dq, n))
        return 1;
    k_gltf_sample<VARIANT><<<blocks(n), kBlock>>>(*m, dn, dwo, du, n, dwi, dw, dp, dm, df, dq);
    if (launched("k_gltf_sample")) return 1;
    return copy_out(wi3, dwi, 3 * n) || copy_out(weight3, dw, 3 * n) || copy_out(pdf, dp, n) || copy_out(mis_pdf, dm, n) || copy_out(f3, df, 3 * n) ||
           copy_out(wpdf, dq, n);
}
template <int VARIANT>
int gltf_eval(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *wi3, int n, float *f3, float *wpdf) {
    Buffers b;
    const float *dn, *dwo, *dwi;
    float *df, *dq;
    if (b.in(dn, n3, 3 * n) || b.in(dwo, wo3, 3 * n) || b.in(dwi, wi3, 3 * n) || b.alloc(df, 3 * n) || b.alloc(dq, n)) return 1;
    k_gltf_eval<VARIANT><<<blocks(n), kBlock>>>(*m, dn, dwo, dwi, n, df, dq);
    if (launched("k_gltf_eval")) return 1;
    return copy_out(f3, df, 3 * n) || copy_out(wpdf, dq, n);
}

// ---- Lambert: orc_simple_probe per element (sample at u2, evaluate at wi_eval)
__global__ void k_simple(const float *base3, const float *n3, const float *wo3, const float *u2, const float *wie3, int n, float *wi3, float *weight3,
                         float *pdf, float *mis_pdf, float *f3, float *wpdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RpMaterial m{};
    m.base_color = ldv(base3, i);
    m.roughness = 1.0f;
    m.ior = 1.0f;
    const V3 nn = ldv(n3, i), wo = ldv(wo3, i), wie = ldv(wie3, i);
    V3 wi = v3s(0.0f);
    float pp = 0.0f, mp = 0.0f;
    const V3 w = rp_sample_simple_brdf(m, nn, wi, pp, mp, v2(u2[2 * i], u2[2 * i + 1]));
    stv(wi3, i, wi);
    stv(weight3, i, w);
    pdf[i] = pp;
    mis_pdf[i] = mp;
    stv(f3, i, rp_simple_bsdf(m, nn, wo, wie));
    wpdf[i] = rp_simple_pdf(nn, wo, wie);
}

// ---- triangle lights: the solid angle and direction sample of rp_finish_tri_light_sample (orc_tri_light_probe's layout)
__global__ void k_tri_light(const float *v9, const float *u2, int n, float *out9) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *v = v9 + 9 * i;
    const V3 d0 = norm3(v3(v[0], v[1], v[2])), d1 = norm3(v3(v[3], v[4], v[5])), d2 = norm3(v3(v[6], v[7], v[8]));
    V3 tp;
    const float tan_half = rp_half_tri_solid_angle_tan(d0, d1, d2, tp);
    const float omega = 2.0f * rp_fast_positive_atan(tan_half);
    const V3 dir = rp_sample_solid_angle_polygon(d0, d1, d2, omega, tp, v2(u2[2 * i], u2[2 * i + 1]));
    float *o = out9 + 9 * i;
    o[0] = omega, o[1] = tan_half, o[2] = tp.x, o[3] = tp.y, o[4] = tp.z, o[5] = dir.x, o[6] = dir.y, o[7] = dir.z;
    o[8] = rp_frcp(omega);
}
// ---- binned light selection (orc_tri_light_bins' layout): the bin, the straight loop of 16 contributions, the selection among them
__global__ void k_tri_lights(RpScene sc, RpFrame f, const float *p3, const float *n3, const float *u4, int n, float *radiance_over_pdf3, float *dir3,
                             float *dist, float *pdf, float *mis_wpdf, int32_t *bins2, float *contributions16) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 hp = ldv(p3, i), hn = ldv(n3, i);
    const RpLightBin bin = rp_choose_light_bin(sc, f, u4[4 * i + 2]);
    float c[RPTR_BINNED_LIGHTS_BIN_MAX_SIZE];
    for (int k = 0; k < RPTR_BINNED_LIGHTS_BIN_MAX_SIZE; ++k) c[k] = rp_tri_light_contribution(sc, bin.bin_begin + k, bin.bin_end, hp, hn);
    V3 light_dir = v3s(0.0f);
    float light_dist = 0.0f, pp = 0.0f, mw = 0.0f;
    const V3 L = rp_finish_tri_light_sample(sc, f, bin, [&](int k) { return c[k]; }, hp, v2(u4[4 * i], u4[4 * i + 1]), u4[4 * i + 3], light_dir,
                                            light_dist, pp, mw);
    stv(radiance_over_pdf3, i, L);
    stv(dir3, i, light_dir);
    dist[i] = light_dist, pdf[i] = pp, mis_wpdf[i] = mw;
    bins2[2 * i] = bin.bin_begin, bins2[2 * i + 1] = bin.bin_end;
    for (int k = 0; k < RPTR_BINNED_LIGHTS_BIN_MAX_SIZE; ++k) contributions16[16 * i + k] = c[k];
}
// ---- point sets: rp_rng_open<TABLE>, then rp_draw1<TABLE> at the absolute dimensions dims[0..n_single) in order, then rp_draw2<TABLE> at
// dims[n_single], dims[n_single + 2], ... (a pair fills two columns: the host checks that dims[k + 1] == dims[k] + 1 there); 6 words per
// query: width, sample_index, frame_offset, frame_id, px, py
template <bool TABLE>
__global__ void k_pointset(RpFrame f, const uint32_t *q6, int n, const uint32_t *dims, int n_single, int n_dims, float *draws, uint32_t *index) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *q = q6 + 6 * i;
    f.width = int32_t(q[0]);
    RpSlotFrame sf;
    sf.frame = 0u, sf.sample_index = q[1], sf.frame_offset = q[2], sf.frame_id = q[3];
    RpRng r = rp_rng_open<TABLE>(f, sf, q[4], q[5]);
    index[i] = r.index;
    float *out = draws + (size_t)i * n_dims;
    for (int k = 0; k < n_single; ++k) out[k] = rp_draw1<TABLE>(f, r, dims[k]);
    for (int k = n_single; k + 1 < n_dims; k += 2) {
        const V2 v = rp_draw2<TABLE>(f, r, dims[k]);
        out[k] = v.x, out[k + 1] = v.y;
    }
}
// out3: rp_randf, then rp_rand2 from the same state; after2: the state behind each
__global__ void k_randf(const uint32_t *states, int n, float *out3, uint32_t *after2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s = states[i], s2 = states[i];
    out3[3 * i] = rp_randf(s);
    const V2 v = rp_rand2(s2);
    out3[3 * i + 1] = v.x, out3[3 * i + 2] = v.y;
    after2[2 * i] = s, after2[2 * i + 1] = s2;
}
// ---- slot and index arithmetic
__global__ void k_div(const uint32_t *nn, const RpDivU32 *d, int n, uint32_t *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = rp_div(nn[i], d[i]);
}
// local3: (lx, ly, the pixel exists) of every slot; slot_of / global_row: of every pixel (lx, ly) of pix2
__global__ void k_slots(RpFrame f, const uint32_t *slots, int n_slots, int32_t *local3, const int32_t *pix2, int n_pix, uint32_t *slot_of, int32_t *global_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) {
        int lx = 0, ly = 0;
        const bool valid = rp_slot_to_local(f, slots[i], lx, ly);
        local3[3 * i] = lx, local3[3 * i + 1] = ly, local3[3 * i + 2] = valid ? 1 : 0;
    }
    if (i < n_pix) {
        slot_of[i] = rp_local_to_slot(f, pix2[2 * i], pix2[2 * i + 1]);
        global_row[i] = rp_local_row_to_global(f, pix2[2 * i + 1]);
    }
}
__global__ void k_slot_frame(RpFrame f, const uint32_t *sslots, int n, uint32_t *out4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RpSlotFrame sf = rp_slot_frame(f, sslots[i]);
    out4[4 * i] = sf.frame, out4[4 * i + 1] = sf.sample_index, out4[4 * i + 2] = sf.frame_offset, out4[4 * i + 3] = sf.frame_id;
}
// ---- sun and MIS
__global__ void k_sun(V3 sun_dir, float cos_radius, const float *u2, int n, float *dirs3, float *pdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    stv(dirs3, i, rp_sample_sun_dir(sun_dir, cos_radius, v2(u2[2 * i], u2[2 * i + 1])));
    if (i == 0) *pdf = rp_sun_dir_pdf(cos_radius);
}
__global__ void k_sun_pdf(const float *cos_radius, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rp_sun_dir_pdf(cos_radius[i]);
}
__global__ void k_nee_mis(const float *f, const float *g, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rp_nee_mis(f[i], g[i]);
}
// ---- sky
__global__ void k_sky(RptrSkyModelParams sky, V3 sun_dir, const float *dirs3, int n, float *out3) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stv(out3, i, rp_skymodel_radiance(sky, sun_dir, ldv(dirs3, i)));
}
// ---- hit attributes (orc_hit_attributes_probe per element: verts9, nuv3, flags bit 0 normals / bit 1 uvs, n2w9 column by column, t / bu / bv)
__global__ void k_hit(const float *verts9, const uint64_t *nuv3, const int *flags, const float *n2w9, const float *tuv3, const int *mat_in, int n,
                      float *out13, int *mat_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *v = verts9 + 9 * i, *m = n2w9 + 9 * i, *t = tuv3 + 3 * i;
    const M3 n2w{v3(m[0], m[1], m[2]), v3(m[3], m[4], m[5]), v3(m[6], m[7], m[8])};
    const RpHit h = rp_calc_hit_attributes(v3(v[0], v[1], v[2]), v3(v[3], v[4], v[5]), v3(v[6], v[7], v[8]), nuv3[3 * i], nuv3[3 * i + 1], nuv3[3 * i + 2],
                                           (flags[i] & 1) != 0, (flags[i] & 2) != 0, mat_in[i], t[0], t[1], t[2], n2w);
    float *o = out13 + 13 * i;
    o[0] = h.normal.x, o[1] = h.normal.y, o[2] = h.normal.z, o[3] = h.geo_normal.x, o[4] = h.geo_normal.y, o[5] = h.geo_normal.z;
    o[6] = h.tangent.x, o[7] = h.tangent.y, o[8] = h.tangent.z, o[9] = h.dist, o[10] = h.bitangent_l, o[11] = h.uv.x, o[12] = h.uv.y;
    mat_out[i] = h.material_id;
}
__global__ void k_dequantize(const uint64_t *qpos, const uint64_t *qnuv, int n, V3 scaling, V3 offset, float *xyz, float *nrm, float *uv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    stv(xyz, i, rp_dequantize_position(qpos[i], scaling, offset));
    stv(nrm, i, rp_dequantize_normal(uint32_t(qnuv[i])));
    const V2 u = rp_dequantize_uv(uint32_t(qnuv[i] >> 32));
    uv[2 * i] = u.x, uv[2 * i + 1] = u.y;
}
// ---- footprints (orc_footprint_probe per element -> out14)
__global__ void k_footprint(const float *dir3, const float *dpdx3, const float *dpdy3, const float *dst3, int n, float *out14) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 d = ldv(dir3, i);
    const M2 F = rp_dpdxy_to_footprint(d, ldv(dpdx3, i), ldv(dpdy3, i));
    V3 a, b;
    rp_footprint_to_dpdxy(a, b, d, F);
    const M2 R = rp_reflect_footprint(ldv(dst3, i), d, F);
    float *o = out14 + 14 * i;
    o[0] = F.c0.x, o[1] = F.c0.y, o[2] = F.c1.x, o[3] = F.c1.y;
    o[4] = a.x, o[5] = a.y, o[6] = a.z, o[7] = b.x, o[8] = b.y, o[9] = b.z;
    o[10] = R.c0.x, o[11] = R.c0.y, o[12] = R.c1.x, o[13] = R.c1.y;
}
// ---- textures: mode 0 rp_texture_grad(uv, ddx, ddy), 1 rp_texture_lod(uv, q[2]), 2 rp_texture_lod0(uv); 6 floats per sample (orc_texture_probe_ex)
__global__ void k_texture(RpScene sc, int mode, const float *q6, int n, float *out4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *q = q6 + 6 * i;
    const V2 uv = v2(q[0], q[1]);
    float4 c;
    if (mode == 0)
        c = rp_texture_grad(sc, 0, RpTexCoord{uv, v2(q[2], q[3]), v2(q[4], q[5])});
    else if (mode == 1)
        c = rp_texture_lod(sc, 0, uv, q[2]);
    else
        c = rp_texture_lod0(sc, 0, uv);
    out4[4 * i] = c.x, out4[4 * i + 1] = c.y, out4[4 * i + 2] = c.z, out4[4 * i + 3] = c.w;
}
// ---- output conversions
__global__ void k_srgb(const float *x, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rp_linear_to_srgb(x[i]);
}
__global__ void k_half4(const float *x4, int n, uint2 *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rp_half4(x4[4 * i], x4[4 * i + 1], x4[4 * i + 2], x4[4 * i + 3]);
}

} // namespace

extern "C" {
int sp_fast_math(void) { return RP_FAST_MATH; }

int sp_gltf_sample(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *u4, int n, float *wi3, float *weight3, float *pdf,
                   float *mis_pdf, float *f3, float *wpdf) {
    return gltf_sample<RPTR_VARIANT_GLTF>(m, n3, wo3, u4, n, wi3, weight3, pdf, mis_pdf, f3, wpdf);
}
int sp_gltf_eval(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *wi3, int n, float *f3, float *wpdf) {
    return gltf_eval<RPTR_VARIANT_GLTF>(m, n3, wo3, wi3, n, f3, wpdf);
}
int sp_gltf_t_sample(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *u4, int n, float *wi3, float *weight3, float *pdf,
                     float *mis_pdf, float *f3, float *wpdf) {
    return gltf_sample<RPTR_VARIANT_GLTF_TRANSMISSION>(m, n3, wo3, u4, n, wi3, weight3, pdf, mis_pdf, f3, wpdf);
}
int sp_gltf_t_eval(const RptrBaseMaterial *m, const float *n3, const float *wo3, const float *wi3, int n, float *f3, float *wpdf) {
    return gltf_eval<RPTR_VARIANT_GLTF_TRANSMISSION>(m, n3, wo3, wi3, n, f3, wpdf);
}
int sp_simple(const float *base3, const float *n3, const float *wo3, const float *u2, const float *wie3, int n, float *wi3, float *weight3, float *pdf,
              float *mis_pdf, float *f3, float *wpdf) {
    Buffers b;
    const float *db, *dn, *dwo, *du, *dwe;
    float *dwi, *dw, *dp, *dm, *df, *dq;
    if (b.in(db, base3, 3 * n) || b.in(dn, n3, 3 * n) || b.in(dwo, wo3, 3 * n) || b.in(du, u2, 2 * n) || b.in(dwe, wie3, 3 * n) || b.alloc(dwi, 3 * n) ||
        b.alloc(dw, 3 * n) || b.alloc(dp, n) || b.alloc(dm, n) || b.alloc(df, 3 * n) || b.alloc(dq, n))
        return 1;
    k_simple<<<blocks(n), kBlock>>>(db, dn, dwo, du, dwe, n, dwi, dw, dp, dm, df, dq);
    if (launched("k_simple")) return 1;
    return copy_out(wi3, dwi, 3 * n) || copy_out(weight3, dw, 3 * n) || copy_out(pdf, dp, n) || copy_out(mis_pdf, dm, n) || copy_out(f3, df, 3 * n) ||
           copy_out(wpdf, dq, n);
}
int sp_tri_light(const float *v9, const float *u2, int n, float *out9) {
    Buffers b;
    const float *dv, *du;
    float *dout;
    if (b.in(dv, v9, 9 * n) || b.in(du, u2, 2 * n) || b.alloc(dout, 9 * n)) return 1;
    k_tri_light<<<blocks(n), kBlock>>>(dv, du, n, dout);
    if (launched("k_tri_light")) return 1;
    return copy_out(out9, dout, 9 * n);
}
// The light table as the library uploads it (host_scene.inl): num_lights records followed by RPTR_BINNED_LIGHTS_BIN_MAX_SIZE + 1 zeroed ones.
// A selection that falls through its bin reads record bin_end <= num_lights, a bin's contributions records below bin_end: refused are an
// empty table, a bin size outside 1 .. RPTR_BINNED_LIGHTS_BIN_MAX_SIZE and a bin sample u4[2] outside [0, 1] (the bin index would leave the table).
int sp_tri_lights(const RptrTriLightData *lights, int num_lights, const RptrLightSamplingConfig *cfg, const float *p3, const float *n3, const float *u4,
                  int n, float *radiance_over_pdf3, float *dir3, float *dist, float *pdf, float *mis_wpdf, int32_t *bins2, float *contributions16) {
    if (!lights || !cfg || num_lights < 1 || cfg->bin_size < 1 || cfg->bin_size > RPTR_BINNED_LIGHTS_BIN_MAX_SIZE || n < 0) {
        fprintf(stderr, "shade_probe: sp_tri_lights: %d lights in bins of %d\n", num_lights, cfg ? cfg->bin_size : 0);
        return 2;
    }
    for (int i = 0; i < n; ++i)
        if (!(u4[4 * i + 2] >= 0.0f && u4[4 * i + 2] <= 1.0f)) {
            fprintf(stderr, "shade_probe: sp_tri_lights: bin sample %d is %g\n", i, (double)u4[4 * i + 2]);
            return 2;
        }
    const size_t padded = (size_t)num_lights + RPTR_BINNED_LIGHTS_BIN_MAX_SIZE + 1;
    Buffers b;
    RptrTriLightData *dl;
    const float *dp, *dn, *du;
    float *dL, *dd, *dt, *dq, *dm, *dc;
    int32_t *db;
    if (b.alloc(dl, padded) || b.in(dp, p3, 3 * (size_t)n) || b.in(dn, n3, 3 * (size_t)n) || b.in(du, u4, 4 * (size_t)n) || b.alloc(dL, 3 * (size_t)n) ||
        b.alloc(dd, 3 * (size_t)n) || b.alloc(dt, n) || b.alloc(dq, n) || b.alloc(dm, n) || b.alloc(db, 2 * (size_t)n) || b.alloc(dc, 16 * (size_t)n))
        return 1;
    SP_TRY(hipMemset(dl, 0, padded * sizeof(RptrTriLightData)));
    SP_TRY(hipMemcpy(dl, lights, (size_t)num_lights * sizeof(RptrTriLightData), hipMemcpyHostToDevice));
    RpScene sc{};
    sc.lights = dl;
    sc.num_lights = num_lights;
    RpFrame f;
    memset(&f, 0, sizeof f);
    f.lc = *cfg;
    f.num_bins = (num_lights + (cfg->bin_size - 1)) / cfg->bin_size; // host_frame.inl fill_frame_constants
    k_tri_lights<<<blocks(n), kBlock>>>(sc, f, dp, dn, du, n, dL, dd, dt, dq, dm, db, dc);
    if (launched("k_tri_lights")) return 1;
    return copy_out(radiance_over_pdf3, dL, 3 * (size_t)n) || copy_out(dir3, dd, 3 * (size_t)n) || copy_out(dist, dt, n) || copy_out(pdf, dq, n) ||
           copy_out(mis_wpdf, dm, n) || copy_out(bins2, db, 2 * (size_t)n) || copy_out(contributions16, dc, 16 * (size_t)n);
}
// table / table_words: the point set's whole table as rptr_hip_set_rng_variant takes it (every index the draws form lies inside it), NULL / 0
// with the uniform generator; table_code: the rp_rng_open<TABLE> / rp_draw1<TABLE> instantiation (0 serves the uniform generator only)
// dims[0..n_single) are drawn one by one, the rest in pairs (d, d + 1) through rp_draw2
int sp_pointset(int rng_variant, int table_code, const uint32_t *table, size_t table_words, const uint32_t *q6, int n, const uint32_t *dims, int n_single,
                int n_dims, float *draws, uint32_t *index) {
    size_t need = 0;
    if (rng_variant == RPTR_RNG_VARIANT_BN) need = size_t(RP_BN_SAMPLES) * RP_BN_DIMS + size_t(RP_BN_TILE) * RP_BN_TILE * RP_BN_SCR_DIMS;
    else if (rng_variant == RPTR_RNG_VARIANT_SOBOL || rng_variant == RPTR_RNG_VARIANT_Z_SBL) need = size_t(RP_SOBOL_DIMS) * RP_SOBOL_BITS + size_t(RP_SOBOL_TILE) * RP_SOBOL_TILE;
    else if (rng_variant != RPTR_RNG_VARIANT_UNIFORM) return 2;
    bool pairs_ok = n_single >= 0 && n_single <= n_dims && (n_dims - n_single) % 2 == 0;
    for (int k = n_single; pairs_ok && k + 1 < n_dims; k += 2) pairs_ok = dims[k + 1] == dims[k] + 1u;
    if ((need && (!table || table_words < need)) || (need && !table_code) || n < 0 || n_dims < 0 || !pairs_ok) {
        fprintf(stderr, "shade_probe: sp_pointset: point set %d with %zu table words, TABLE = %d\n", rng_variant, table_words, table_code);
        return 2;
    }
    Buffers b;
    const uint32_t *dtab = nullptr, *dq, *ddims;
    float *ddraws;
    uint32_t *dindex;
    if ((need && b.in(dtab, table, need)) || b.in(dq, q6, 6 * (size_t)n) || b.in(ddims, dims, n_dims) || b.alloc(ddraws, (size_t)n * n_dims) || b.alloc(dindex, n))
        return 1;
    RpFrame f;
    memset(&f, 0, sizeof f);
    f.rng_variant = rng_variant;
    f.rng_table = dtab;
    if (table_code)
        k_pointset<true><<<blocks(n), kBlock>>>(f, dq, n, ddims, n_single, n_dims, ddraws, dindex);
    else
        k_pointset<false><<<blocks(n), kBlock>>>(f, dq, n, ddims, n_single, n_dims, ddraws, dindex);
    if (launched("k_pointset")) return 1;
    return copy_out(draws, ddraws, (size_t)n * n_dims) || copy_out(index, dindex, n);
}
int sp_randf(const uint32_t *states, int n, float *out3, uint32_t *after2) {
    Buffers b;
    const uint32_t *ds;
    float *dout;
    uint32_t *da;
    if (b.in(ds, states, n) || b.alloc(dout, 3 * (size_t)n) || b.alloc(da, 2 * (size_t)n)) return 1;
    k_randf<<<blocks(n), kBlock>>>(ds, n, dout, da);
    if (launched("k_randf")) return 1;
    return copy_out(out3, dout, 3 * (size_t)n) || copy_out(after2, da, 2 * (size_t)n);
}
// q[i] = rp_div(n[i], rp_make_div(d[i])), the divisor records made by the header's own host function; d >= 1
int sp_div(const uint32_t *nn, const uint32_t *d, int n, uint32_t *q) {
    std::vector<RpDivU32> divs((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (d[i] < 1u) return 2;
        divs[(size_t)i] = rp_make_div(d[i]);
    }
    Buffers b;
    const uint32_t *dn;
    const RpDivU32 *dd;
    uint32_t *dq;
    if (b.in(dn, nn, n) || b.in(dd, divs.data(), n) || b.alloc(dq, n)) return 1;
    k_div<<<blocks(n), kBlock>>>(dn, dd, n, dq);
    if (launched("k_div")) return 1;
    return copy_out(q, dq, n);
}
namespace {
struct SpGeometry {
    int32_t width, height, rank, world, stripe_rows;
};
// the tile mapping of a frame as rptr_hip_initialize (rptr_hip.hip) and fill_frame_constants (host_frame.inl) set it. A COPY of those
// host lines (local_row_count of host_state.h, tiles_x / tiles_y / npix_padded), made to feed the device functions a frame of the
// product's shape: what sp_slot_geometry hands back, and what the tests compare with their own statement, is this copy, not the product's
// host code (that is exercised by every rendered frame).
bool slot_geometry(const SpGeometry &g, RpFrame &f) {
    memset(&f, 0, sizeof f);
    if (g.width < 1 || g.height < 1 || g.world < 1 || g.rank < 0 || g.rank >= g.world || g.stripe_rows < 1) return false;
    f.width = g.width;
    f.height = g.height;
    f.rank = g.rank;
    f.world = g.world;
    f.stripe_rows = g.stripe_rows;
    const int n_stripes = (g.height + g.stripe_rows - 1) / g.stripe_rows; // host_state.h local_row_count
    for (int s = g.rank; s < n_stripes; s += g.world) f.local_rows += g.stripe_rows < g.height - s * g.stripe_rows ? g.stripe_rows : g.height - s * g.stripe_rows;
    f.tiles_x = ((g.width + 7) / 8 + RP_TILE_BLOCK - 1) / RP_TILE_BLOCK * RP_TILE_BLOCK;
    f.tiles_y = (((f.local_rows > 1 ? f.local_rows : 1) + 7) / 8 + RP_TILE_BLOCK - 1) / RP_TILE_BLOCK * RP_TILE_BLOCK;
    f.npix_padded = f.tiles_x * f.tiles_y * 64;
    f.div_npix_padded = rp_make_div((uint32_t)f.npix_padded);
    f.div_tiles_x = rp_make_div((uint32_t)(f.tiles_x / RP_TILE_BLOCK));
    f.div_stripe_rows = rp_make_div((uint32_t)f.stripe_rows);
    f.div_width = rp_make_div((uint32_t)f.width);
    return true;
}
} // namespace
// out4: local_rows, tiles_x, tiles_y, npix_padded
int sp_slot_geometry(const SpGeometry *g, int32_t *out4) {
    RpFrame f;
    if (!g || !slot_geometry(*g, f)) return 2;
    out4[0] = f.local_rows, out4[1] = f.tiles_x, out4[2] = f.tiles_y, out4[3] = f.npix_padded;
    return 0;
}
int sp_slots(const SpGeometry *g, const uint32_t *slots, int n_slots, int32_t *local3, const int32_t *pix2, int n_pix, uint32_t *slot_of, int32_t *global_row) {
    RpFrame f;
    if (!g || !slot_geometry(*g, f) || n_slots < 0 || n_pix < 0) return 2;
    Buffers b;
    const uint32_t *ds;
    const int32_t *dp;
    int32_t *dl, *dg;
    uint32_t *dso;
    if (b.in(ds, slots, n_slots) || b.in(dp, pix2, 2 * (size_t)n_pix) || b.alloc(dl, 3 * (size_t)n_slots) || b.alloc(dso, n_pix) || b.alloc(dg, n_pix)) return 1;
    const int n = n_slots > n_pix ? n_slots : n_pix;
    if (n == 0) return 0;
    k_slots<<<blocks(n), kBlock>>>(f, ds, n_slots, dl, dp, n_pix, dso, dg);
    if (launched("k_slots")) return 1;
    return copy_out(local3, dl, 3 * (size_t)n_slots) || copy_out(slot_of, dso, n_pix) || copy_out(global_row, dg, n_pix);
}
// out4: (frame, sample_index, frame_offset, frame_id) of every sample slot of a launch sequence of batch_frames frames of frame_spp slots
int sp_slot_frame(int batch_frames, int frame_spp, int batch_reset, uint32_t frame_offset, uint32_t sample_base, uint32_t frame_id, const uint32_t *sslots,
                  int n, uint32_t *out4) {
    if (batch_frames < 1 || frame_spp < 1 || n < 0) return 2;
    RpFrame f;
    memset(&f, 0, sizeof f);
    f.frame_offset = frame_offset; // host_frame.inl fill_frame_constants
    f.sample_base = sample_base;
    f.frame_id = frame_id;
    f.batch_frames = batch_frames;
    f.frame_spp = frame_spp;
    f.batch_spp = batch_frames * frame_spp;
    f.batch_reset = batch_reset ? 1 : 0;
    f.div_frame_spp = rp_make_div((uint32_t)frame_spp);
    Buffers b;
    const uint32_t *ds;
    uint32_t *dout;
    if (b.in(ds, sslots, n) || b.alloc(dout, 4 * (size_t)n)) return 1;
    k_slot_frame<<<blocks(n), kBlock>>>(f, ds, n, dout);
    if (launched("k_slot_frame")) return 1;
    return copy_out(out4, dout, 4 * (size_t)n);
}
int sp_sample_sun(const float sun_dir[3], float cos_radius, const float *u2, int n, float *dirs3, float *pdf) {
    Buffers b;
    const float *du;
    float *dd, *dp;
    if (b.in(du, u2, 2 * n) || b.alloc(dd, 3 * n) || b.alloc(dp, 1)) return 1;
    k_sun<<<blocks(n), kBlock>>>(V3{sun_dir[0], sun_dir[1], sun_dir[2]}, cos_radius, du, n, dd, dp);
    if (launched("k_sun")) return 1;
    return copy_out(dirs3, dd, 3 * n) || copy_out(pdf, dp, 1);
}
int sp_sun_pdf(const float *cos_radius, int n, float *out) {
    Buffers b;
    const float *dc;
    float *dout;
    if (b.in(dc, cos_radius, n) || b.alloc(dout, n)) return 1;
    k_sun_pdf<<<blocks(n), kBlock>>>(dc, n, dout);
    if (launched("k_sun_pdf")) return 1;
    return copy_out(out, dout, n);
}
int sp_nee_mis(const float *pdf_f, const float *pdf_g, int n, float *out) {
    Buffers b;
    const float *df, *dg;
    float *dout;
    if (b.in(df, pdf_f, n) || b.in(dg, pdf_g, n) || b.alloc(dout, n)) return 1;
    k_nee_mis<<<blocks(n), kBlock>>>(df, dg, n, dout);
    if (launched("k_nee_mis")) return 1;
    return copy_out(out, dout, n);
}
int sp_sky_radiance(const RptrSkyModelParams *sky, const float sun_dir[3], const float *dirs3, int n, float *out3) {
    Buffers b;
    const float *dd;
    float *dout;
    if (b.in(dd, dirs3, 3 * n) || b.alloc(dout, 3 * n)) return 1;
    k_sky<<<blocks(n), kBlock>>>(*sky, V3{sun_dir[0], sun_dir[1], sun_dir[2]}, dd, n, dout);
    if (launched("k_sky")) return 1;
    return copy_out(out3, dout, 3 * n);
}
int sp_hit_attributes(const float *verts9, const uint64_t *nuv3, const int *flags, const float *n2w9, const float *tuv3, const int *mat_in, int n,
                      float *out13, int *mat_out) {
    Buffers b;
    const float *dv, *dm, *dt;
    const uint64_t *dq;
    const int *dfl, *dmi;
    float *dout;
    int *dmo;
    if (b.in(dv, verts9, 9 * n) || b.in(dq, nuv3, 3 * n) || b.in(dfl, flags, n) || b.in(dm, n2w9, 9 * n) || b.in(dt, tuv3, 3 * n) || b.in(dmi, mat_in, n) ||
        b.alloc(dout, 13 * n) || b.alloc(dmo, n))
        return 1;
    k_hit<<<blocks(n), kBlock>>>(dv, dq, dfl, dm, dt, dmi, n, dout, dmo);
    if (launched("k_hit")) return 1;
    return copy_out(out13, dout, 13 * n) || copy_out(mat_out, dmo, n);
}
int sp_dequantize(const uint64_t *qpos, const uint64_t *qnuv, int n, const float scaling[3], const float offset[3], float *xyz, float *nrm, float *uv) {
    Buffers b;
    const uint64_t *dqp, *dqn;
    float *dx, *dn, *du;
    if (b.in(dqp, qpos, n) || b.in(dqn, qnuv, n) || b.alloc(dx, 3 * n) || b.alloc(dn, 3 * n) || b.alloc(du, 2 * n)) return 1;
    k_dequantize<<<blocks(n), kBlock>>>(dqp, dqn, n, V3{scaling[0], scaling[1], scaling[2]}, V3{offset[0], offset[1], offset[2]}, dx, dn, du);
    if (launched("k_dequantize")) return 1;
    return copy_out(xyz, dx, 3 * n) || copy_out(nrm, dn, 3 * n) || copy_out(uv, du, 2 * n);
}
int sp_footprint(const float *dir3, const float *dpdx3, const float *dpdy3, const float *dst3, int n, float *out14) {
    Buffers b;
    const float *dd, *dx, *dy, *ds;
    float *dout;
    if (b.in(dd, dir3, 3 * n) || b.in(dx, dpdx3, 3 * n) || b.in(dy, dpdy3, 3 * n) || b.in(ds, dst3, 3 * n) || b.alloc(dout, 14 * n)) return 1;
    k_footprint<<<blocks(n), kBlock>>>(dd, dx, dy, ds, n, dout);
    if (launched("k_footprint")) return 1;
    return copy_out(out14, dout, 14 * n);
}
// one texture: `levels` levels of `width` x `height` RGBA8 stored back to back (RptrTextureDesc.rgba8, `bytes` in all), sampled as texture
// 0 of a scene that holds only it and the sRGB table the library uploads (rp_srgb_decode_lut)
int sp_texture(const uint8_t *texels, size_t bytes, int width, int height, int srgb, int levels, int mode, const float *q6, int n, float *out4) {
    size_t need = 0;
    for (int l = 0, w = width, h = height; l < levels; ++l, w = w > 1 ? w / 2 : 1, h = h > 1 ? h / 2 : 1) need += 4 * (size_t)w * (size_t)h;
    if (width < 1 || height < 1 || levels < 1 || need != bytes) {
        fprintf(stderr, "shade_probe: sp_texture: %zu bytes do not hold %d levels of %d x %d\n", bytes, levels, width, height);
        return 1;
    }
    // The chain lies between two guard bands of one level-0 size each, filled with 0xFF bytes. A wrapped index stays within
    // (-w*h, w*h) texels of its level, so a wrong wrap reads a guard texel (white, opaque: the comparison with the oracle fails)
    // and never leaves the allocation.
    const size_t guard = 4 * (size_t)width * (size_t)height;
    Buffers b;
    uint8_t *dt;
    const float *dq;
    float lut[256], *dout;
    const float *dlut;
    rp_srgb_decode_lut(lut);
    RpTexture *dtex;
    if (b.alloc(dt, guard + bytes + guard) || b.in(dq, q6, 6 * (size_t)n) || b.in(dlut, lut, 256) || b.alloc(dtex, 1) || b.alloc(dout, 4 * (size_t)n))
        return 1;
    SP_TRY(hipMemset(dt, 0xFF, guard + bytes + guard));
    SP_TRY(hipMemcpy(dt + guard, texels, bytes, hipMemcpyHostToDevice));
    const RpTexture tex{reinterpret_cast<const uchar4 *>(dt + guard), width, height, srgb ? 1 : 0, levels};
    SP_TRY(hipMemcpy(dtex, &tex, sizeof tex, hipMemcpyHostToDevice));
    RpScene sc{};
    sc.textures = dtex;
    sc.num_textures = 1;
    sc.srgb_lut = dlut;
    k_texture<<<blocks(n), kBlock>>>(sc, mode, dq, n, dout);
    if (launched("k_texture")) return 1;
    return copy_out(out4, dout, 4 * (size_t)n);
}
int sp_linear_to_srgb(const float *x, int n, float *out) {
    Buffers b;
    const float *dx;
    float *dout;
    if (b.in(dx, x, n) || b.alloc(dout, n)) return 1;
    k_srgb<<<blocks(n), kBlock>>>(dx, n, dout);
    if (launched("k_srgb")) return 1;
    return copy_out(out, dout, n);
}
int sp_half4(const float *x4, int n, uint16_t *out4) {
    Buffers b;
    const float *dx;
    uint2 *dout;
    if (b.in(dx, x4, 4 * (size_t)n) || b.alloc(dout, n)) return 1;
    k_half4<<<blocks(n), kBlock>>>(dx, n, dout);
    if (launched("k_half4")) return 1;
    return copy_out(reinterpret_cast<uint2 *>(out4), dout, n);
}
} // extern "C"
