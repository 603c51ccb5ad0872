// Device functions of the rasterizer's other two argument forms (upstream diff_gaussian_rasterization):
//   colours from spherical harmonics  (shs [P, M, 3], active degree D: (D+1)^2 <= M <= 16 coefficients read)
//   covariances given directly        (cov3D_precomp [P, 6] = xx, xy, xz, yy, yz, zz; scale_modifier not applied)
// used by csrc/raster_forms.hip.  The colours_precomp + scales/rotations form keeps its own kernels (csrc/raster_geom.hip,
// csrc/raster_bwd.hip): factoring their shared tail out of cgs_pre_fwd_one / cgs_pre_bwd_one changed the instructions hipcc
// emits for them, so the tail of the forward and the covariance part of the backward are restated here, statement for
// statement, and the two must be edited together.
#pragma once
#include <hip/hip_fp16.h>
#include "cgs_internal.h"
#include "raster_math.h"
#include "raster_pre.h"

// The two optional forms of one call (include/cgs.h, cgs_raster_preprocess_launch_ex): shs [P, sh_coeffs, 3] of degree
// sh_degree, or NULL; cov3D [P, 6], or NULL.  sh_vec: the SH rows are 16-byte aligned.
struct CgsRasterForms {
    const float *shs;
    int sh_degree, sh_coeffs, sh_vec;
    const float *cov3D;
};
int cgs_launch_preprocess_form(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D,
                               const float *colors, const float *opacities, const float *scales, const float *rotations,
                               CgsGeom &g, int32_t *radii, bool filter_only, hipStream_t stream, bool aa = false);
int cgs_launch_preprocess_bwd_form(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D,
                                   const float *scales, const float *rotations, const int32_t *radii,
                                   const float *dL_dmean2D_px, const float *dL_dconic, const float *dL_dcolors,
                                   float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dshs, float *dL_dscales,
                                   float *dL_drotations, float *dL_dcov3D, hipStream_t stream,
                                   const float *aa_opacities = nullptr, float *aa_dL_dopacities = nullptr,
                                   const float *dL_dabs_px = nullptr);
// aa: antialiasing (raster_math.h); aa_opacities != NULL: its backward, as cgs_launch_preprocess_bwd's; dL_dabs_px likewise

// ---- spherical harmonics (the real SH basis of 3DGS / PlenOctrees, same constants and term order) ----------------------
#define CGS_SH_C0 0.28209479177387814f
#define CGS_SH_C1 0.4886025119029199f
#define CGS_SH_C2_0 1.0925484305920792f
#define CGS_SH_C2_1 (-1.0925484305920792f)
#define CGS_SH_C2_2 0.31539156525252005f
#define CGS_SH_C2_3 (-1.0925484305920792f)
#define CGS_SH_C2_4 0.5462742152960396f
#define CGS_SH_C3_0 (-0.5900435899266435f)
#define CGS_SH_C3_1 2.890611442640554f
#define CGS_SH_C3_2 (-0.4570457994644658f)
#define CGS_SH_C3_3 0.3731763325901154f
#define CGS_SH_C3_4 (-0.4570457994644658f)
#define CGS_SH_C3_5 1.445305721320277f
#define CGS_SH_C3_6 (-0.5900435899266435f)

// N consecutive floats of one row into registers; vec: the row is 16-byte aligned (row stride 3M with M % 4 == 0 and an
// aligned base), read as dwordx4 + a scalar tail.  vec is the same in every lane.
template <int N>
__device__ __forceinline__ void cgs_load_row(const float *__restrict__ src, bool vec, float (&dst)[N]) {
    if (vec) {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            const float4 v = reinterpret_cast<const float4 *>(src)[k];
            dst[4 * k] = v.x; dst[4 * k + 1] = v.y; dst[4 * k + 2] = v.z; dst[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int k = N / 4 * 4; k < N; ++k) dst[k] = src[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) dst[k] = src[k];
    }
}

// dst[0 .. 3M) of one row: value(k) for k < N (a compile-time k), zeros after them (no memset of dL/dshs needed).  vec as
// above; with vec, 3M is a multiple of 4 and >= N rounded up to 4.
template <int N, typename ValueFn>
__device__ __forceinline__ void cgs_store_row(float *__restrict__ dst, bool vec, int M, ValueFn value) {
    const int n = 3 * M;
    if (vec) {
        constexpr int NV = (N + 3) / 4;
#pragma unroll
        for (int k = 0; k < NV; ++k)
            reinterpret_cast<float4 *>(dst)[k] = make_float4(value(4 * k), 4 * k + 1 < N ? value(4 * k + 1) : 0.f,
                                                             4 * k + 2 < N ? value(4 * k + 2) : 0.f,
                                                             4 * k + 3 < N ? value(4 * k + 3) : 0.f);
        for (int k = NV; k < n / 4; ++k) reinterpret_cast<float4 *>(dst)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) dst[k] = value(k);
        for (int k = N; k < n; ++k) dst[k] = 0.f;
    }
}

__device__ __forceinline__ void cgs_zero_row(float *__restrict__ dst, bool vec, int M) {
    const int n = 3 * M;
    if (vec)
        for (int k = 0; k < n / 4; ++k) reinterpret_cast<float4 *>(dst)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    else
        for (int k = 0; k < n; ++k) dst[k] = 0.f;
}

// Colour of degree D before the clamp: sh[3 k + c] = coefficient k of channel c, (x, y, z) the unit view direction.
template <int D>
__device__ __forceinline__ float3 cgs_sh_rgb(const float (&sh)[3 * (D + 1) * (D + 1)], float x, float y, float z) {
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *s = sh + c;
        float v = CGS_SH_C0 * s[0];
        if (D > 0) {
            v = v - CGS_SH_C1 * y * s[3] + CGS_SH_C1 * z * s[6] - CGS_SH_C1 * x * s[9];
            if (D > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                v = v + CGS_SH_C2_0 * xy * s[12] + CGS_SH_C2_1 * yz * s[15] + CGS_SH_C2_2 * (2.f * zz - xx - yy) * s[18] +
                    CGS_SH_C2_3 * xz * s[21] + CGS_SH_C2_4 * (xx - yy) * s[24];
                if (D > 2) {
                    v = v + CGS_SH_C3_0 * y * (3.f * xx - yy) * s[27] + CGS_SH_C3_1 * xy * z * s[30] +
                        CGS_SH_C3_2 * y * (4.f * zz - xx - yy) * s[33] + CGS_SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy) * s[36] +
                        CGS_SH_C3_4 * x * (4.f * zz - xx - yy) * s[39] + CGS_SH_C3_5 * z * (xx - yy) * s[42] +
                        CGS_SH_C3_6 * x * (xx - 3.f * yy) * s[45];
                }
            }
        }
        r[c] = v + 0.5f;
    }
    return make_float3(r[0], r[1], r[2]);
}

// dir = p - campos (not normalised) -> unit direction
__device__ __forceinline__ float3 cgs_sh_dir(const float3 p, const float3 cam, float3 &d) {
    d = make_float3(p.x - cam.x, p.y - cam.y, p.z - cam.z);
    const float inv = 1.f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    return make_float3(d.x * inv, d.y * inv, d.z * inv);
}

// The K = (D+1)^2 basis values of cgs_sh_rgb: colour channel c = sum_k b[k] sh[3 k + c] (+ 0.5), so dL/dsh[3 k + c] = b[k] g[c].
template <int D>
__device__ __forceinline__ void cgs_sh_basis(float x, float y, float z, float (&b)[(D + 1) * (D + 1)]) {
    b[0] = CGS_SH_C0;
    if constexpr (D > 0) {
        b[1] = -CGS_SH_C1 * y;
        b[2] = CGS_SH_C1 * z;
        b[3] = -CGS_SH_C1 * x;
    }
    if constexpr (D > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = CGS_SH_C2_0 * xy;
        b[5] = CGS_SH_C2_1 * yz;
        b[6] = CGS_SH_C2_2 * (2.f * zz - xx - yy);
        b[7] = CGS_SH_C2_3 * xz;
        b[8] = CGS_SH_C2_4 * (xx - yy);
        if constexpr (D > 2) {
            b[9] = CGS_SH_C3_0 * y * (3.f * xx - yy);
            b[10] = CGS_SH_C3_1 * xy * z;
            b[11] = CGS_SH_C3_2 * y * (4.f * zz - xx - yy);
            b[12] = CGS_SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy);
            b[13] = CGS_SH_C3_4 * x * (4.f * zz - xx - yy);
            b[14] = CGS_SH_C3_5 * z * (xx - yy);
            b[15] = CGS_SH_C3_6 * x * (xx - 3.f * yy);
        }
    }
}

// dL/d(unit direction) of cgs_sh_rgb: w[k] = sum_c sh[3 k + c] g[c] with g = dL/dcolor (clamped channels zeroed), the
// derivative of each basis function contracted with it (the terms of the 3DGS backward, per coefficient instead of per channel).
template <int D>
__device__ __forceinline__ float3 cgs_sh_ddir(const float (&w)[(D + 1) * (D + 1)], float x, float y, float z) {
    if constexpr (D == 0) {
        return make_float3(0.f, 0.f, 0.f);
    } else {
        float dx = -CGS_SH_C1 * w[3], dy = -CGS_SH_C1 * w[1], dz = CGS_SH_C1 * w[2];
        if constexpr (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dx += CGS_SH_C2_0 * y * w[4] + CGS_SH_C2_2 * 2.f * -x * w[6] + CGS_SH_C2_3 * z * w[7] + CGS_SH_C2_4 * 2.f * x * w[8];
            dy += CGS_SH_C2_0 * x * w[4] + CGS_SH_C2_1 * z * w[5] + CGS_SH_C2_2 * 2.f * -y * w[6] + CGS_SH_C2_4 * 2.f * -y * w[8];
            dz += CGS_SH_C2_1 * y * w[5] + CGS_SH_C2_2 * 2.f * 2.f * z * w[6] + CGS_SH_C2_3 * x * w[7];
            if constexpr (D > 2) {
                dx += CGS_SH_C3_0 * w[9] * 3.f * 2.f * xy + CGS_SH_C3_1 * w[10] * yz + CGS_SH_C3_2 * w[11] * -2.f * xy +
                      CGS_SH_C3_3 * w[12] * -3.f * 2.f * xz + CGS_SH_C3_4 * w[13] * (-3.f * xx + 4.f * zz - yy) +
                      CGS_SH_C3_5 * w[14] * 2.f * xz + CGS_SH_C3_6 * w[15] * 3.f * (xx - yy);
                dy += CGS_SH_C3_0 * w[9] * 3.f * (xx - yy) + CGS_SH_C3_1 * w[10] * xz +
                      CGS_SH_C3_2 * w[11] * (-3.f * yy + 4.f * zz - xx) + CGS_SH_C3_3 * w[12] * -3.f * 2.f * yz +
                      CGS_SH_C3_4 * w[13] * -2.f * xy + CGS_SH_C3_5 * w[14] * -2.f * yz + CGS_SH_C3_6 * w[15] * -3.f * 2.f * xy;
                dz += CGS_SH_C3_1 * w[10] * xy + CGS_SH_C3_2 * w[11] * 4.f * 2.f * yz +
                      CGS_SH_C3_3 * w[12] * 3.f * (2.f * zz - xx - yy) + CGS_SH_C3_4 * w[13] * 4.f * 2.f * xz +
                      CGS_SH_C3_5 * w[14] * (xx - yy);
            }
        }
        return make_float3(dx, dy, dz);
    }
}

// d(v / |v|)^T dv: the gradient of the unnormalised direction from that of the unit one
__device__ __forceinline__ float3 cgs_dnormvdv(const float3 v, const float3 dv) {
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.f / sqrtf(sum2 * sum2 * sum2);
    return make_float3(((sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32,
                       (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32,
                       (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32);
}

// ---- projection from a given 3-D covariance: cgs_project (csrc/raster_math.h) without its rotation / scale lines -------
template <bool AA = false>
__device__ __forceinline__ bool cgs_project_cov(const float3 p, const CgsCov3 &c3, const float *V, const float *Pm, int W, int H,
                                                float tanfovx, float tanfovy, CgsProj &o) {
    const float3 t = cgs_to_view(p, V);
    if (t.z <= 0.2f) return false;   // near cull: the only frustum test
    const float hx = Pm[0] * p.x + Pm[4] * p.y + Pm[8] * p.z + Pm[12];
    const float hy = Pm[1] * p.x + Pm[5] * p.y + Pm[9] * p.z + Pm[13];
    const float hw = Pm[3] * p.x + Pm[7] * p.y + Pm[11] * p.z + Pm[15];
    const float pw = 1.f / (hw + 0.0000001f);
    const float ndcx = hx * pw, ndcy = hy * pw;
    const CgsJac j = cgs_jacobian(t, V, W, H, tanfovx, tanfovy);
    float a, b, c;
    cgs_cov2d(j.A, c3, a, b, c);
    if constexpr (AA) {
        float d1;
        o.aa_h = cgs_aa_h(cgs_det2_comp(a, b, c), a, c, d1);
    }
    a += 0.3f;
    c += 0.3f;
    const float det = a * c - b * b;
    if (det == 0.f) return false;
    const float inv = 1.f / det;
    o.con_a = c * inv; o.con_b = -b * inv; o.con_c = a * inv;
    o.cov_a = a; o.cov_b = b; o.cov_c = c;
    const float mid = 0.5f * (a + c);
    const float hd = 0.5f * (a - c);                       // mid^2 - det without cancellation (raster_math.h)
    const float disc = sqrtf(fmaxf(0.1f, hd * hd + b * b));
    o.radius = ceilf(3.f * sqrtf(fmaxf(mid + disc, mid - disc)));
    o.px = ((ndcx + 1.f) * (float)W - 1.f) * 0.5f;
    o.py = ((ndcy + 1.f) * (float)H - 1.f) * 0.5f;
    o.depth = t.z;
    return true;
}

// ---- forward: cgs_pre_fwd_one (csrc/raster_pre.h) after its cgs_project call, colour evaluated lazily ------------------
// color() is called only for a Gaussian that touches a tile (radius > 0), the Gaussians whose colour upstream evaluates.
// AA: pr.aa_h is set (cgs_project / cgs_project_cov with AA), the record and the tightening take op_in * pr.aa_h.
template <bool FILTER_ONLY, typename ColorFn, bool AA = false>
__device__ __forceinline__ void cgs_pre_fwd_form(int64_t i, const bool ok, const CgsProj &pr, float op_in, ColorFn color, int W,
                                                 int H, float4 *__restrict__ rec, uint32_t *__restrict__ depth_key,
                                                 uint32_t *__restrict__ tiles, uint2 *__restrict__ rect,
                                                 int32_t *__restrict__ radii) {
    int32_t radius = 0;
    uint32_t ntiles = 0;
    uint2 packed = make_uint2(0u, 0u);
    uint32_t dkey = 0xFFFFFFFFu;
    if (ok) {
        const int gx = (W + CGS_TILE - 1) / CGS_TILE, gy = (H + CGS_TILE - 1) / CGS_TILE;
        const float r = pr.radius;
        int x0 = min(gx, max(0, (int)((pr.px - r) / (float)CGS_TILE)));
        int y0 = min(gy, max(0, (int)((pr.py - r) / (float)CGS_TILE)));
        int x1 = min(gx, max(0, (int)((pr.px + r + (float)(CGS_TILE - 1)) / (float)CGS_TILE)));
        int y1 = min(gy, max(0, (int)((pr.py + r + (float)(CGS_TILE - 1)) / (float)CGS_TILE)));
        if ((x1 - x0) * (y1 - y0) > 0) {
            radius = (int32_t)r;
            if (!FILTER_ONLY) {
                const float op = AA ? op_in * pr.aa_h : op_in;
                // output-invariant tightening to the alpha >= 1/255 ellipse: see cgs_pre_fwd_one
                float hx = -1.f, hy = -1.f;
                uint32_t diag = 0x7C007C00u;
                const float t255 = 255.f * op;
                if (t255 >= 1.f) {
                    const float tau2 = 2.f * logf(t255);
                    hx = sqrtf(tau2 * pr.cov_a) * 1.002f + 0.02f;
                    hy = sqrtf(tau2 * pr.cov_c) * 1.002f + 0.02f;
                    const float su = fmaxf(pr.cov_a + pr.cov_c + 2.f * pr.cov_b, 0.f);
                    const float sv = fmaxf(pr.cov_a + pr.cov_c - 2.f * pr.cov_b, 0.f);
                    const float hu = sqrtf(tau2 * su) * 1.002f + 0.03f, hv = sqrtf(tau2 * sv) * 1.002f + 0.03f;
                    diag = (uint32_t)__half_as_ushort(__float2half_ru(hu)) |
                           ((uint32_t)__half_as_ushort(__float2half_ru(hv)) << 16);
                    const float fx0 = ceilf(pr.px - hx), fx1 = floorf(pr.px + hx);
                    const float fy0 = ceilf(pr.py - hy), fy1 = floorf(pr.py + hy);
                    if (fx1 >= fx0 && fy1 >= fy0 && fx1 >= 0.f && fy1 >= 0.f && fx0 <= (float)(W - 1) &&
                        fy0 <= (float)(H - 1)) {
                        const int tx0 = max(0, (int)fx0) / CGS_TILE;
                        const int ty0 = max(0, (int)fy0) / CGS_TILE;
                        const int tx1 = min(W - 1, (int)fx1) / CGS_TILE + 1;
                        const int ty1 = min(H - 1, (int)fy1) / CGS_TILE + 1;
                        x0 = max(x0, tx0); y0 = max(y0, ty0);
                        x1 = min(x1, tx1); y1 = min(y1, ty1);
                    } else {
                        x1 = x0; y1 = y0;
                    }
                } else {
                    x1 = x0; y1 = y0;
                }
                if (x1 > x0 && y1 > y0) {
                    ntiles = (uint32_t)((x1 - x0) * (y1 - y0));
                    packed = make_uint2((uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16));
                    dkey = __float_as_uint(pr.depth);
                }
                const float3 c = color();
                const float k = 1.4426950408889634f;  // log2(e): blend uses exp2
                rec[3 * i + 0] = make_float4(pr.px, pr.py, -0.5f * k * pr.con_a, -k * pr.con_b);
                rec[3 * i + 1] = make_float4(-0.5f * k * pr.con_c, op, c.x, c.y);
                rec[3 * i + 2] = make_float4(c.z, hx, hy, __uint_as_float(diag));
            }
        }
    }
    radii[i] = radius;
    if (!FILTER_ONLY) {
        tiles[i] = ntiles;
        rect[i] = packed;
        depth_key[i] = dkey;
    }
}

// ---- backward: the first half of cgs_pre_bwd_one (csrc/raster_pre.h) from a given covariance -------------
// Fills o.dp (projection + covariance paths of dL/dmeans3D) and o.dm2; M = dL/dSigma as the full symmetric matrix.
// AA: o.dop and the h terms as in cgs_pre_bwd_one, with d0 from cgs_det2_comp as cgs_project_cov forms it.
template <bool AA = false>
__device__ __forceinline__ void cgs_pre_bwd_cov(const float3 p, const CgsCov3 &c3, float gmean_x, float gmean_y, float gconic_a,
                                                float gconic_b, float gconic_c, const float *V, const float *Pm, int W, int H,
                                                float tanfovx, float tanfovy, CgsPreBwd &o, float M[9], float aa_op = 0.f,
                                                float aa_g = 0.f) {
    const float3 t = cgs_to_view(p, V);
    const CgsJac j = cgs_jacobian(t, V, W, H, tanfovx, tanfovy);
    float x, y, z;   // dilated cov2D = [[x,y],[y,z]]
    cgs_cov2d(j.A, c3, x, y, z);
    float aa_gx = 0.f, aa_gy = 0.f, aa_gz = 0.f;
    if constexpr (AA) {
        float d1;
        const float d0 = cgs_det2_comp(x, y, z);
        const float hh = cgs_aa_h(d0, x, z, d1);
        o.dop = aa_g * hh;
        cgs_aa_bwd(d0, d1, hh, x, y, z, aa_g, aa_op, aa_gx, aa_gy, aa_gz);
    }
    x += 0.3f;
    z += 0.3f;
    const float det = x * z - y * y;
    const float ga = gconic_a, gbb = gconic_b, gc = gconic_c;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (det != 0.f) {
        const float d2 = 1.f / (det * det);
        gx = d2 * (-z * z * ga + y * z * gbb - y * y * gc);
        gy = d2 * (2.f * y * z * ga - (x * z + y * y) * gbb + 2.f * x * y * gc);
        gz = d2 * (-y * y * ga + x * y * gbb - x * x * gc);
    }
    if constexpr (AA) {
        gx += aa_gx;
        gy += aa_gy;
        gz += aa_gz;
    }
    const float h = 0.5f * gy;
    const float *A = j.A;
    float GA0[3], GA1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        GA0[c] = gx * A[c] + h * A[3 + c];
        GA1[c] = h * A[c] + gz * A[3 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = A[r] * GA0[c] + A[3 + r] * GA1[c];
    const float S[9] = {c3.xx, c3.xy, c3.xz, c3.xy, c3.yy, c3.yz, c3.xz, c3.yz, c3.zz};
    float dA[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dA[c] = 2.f * (GA0[0] * S[c] + GA0[1] * S[3 + c] + GA0[2] * S[6 + c]);
        dA[3 + c] = 2.f * (GA1[0] * S[c] + GA1[1] * S[3 + c] + GA1[2] * S[6 + c]);
    }
    const float dJ00 = dA[0] * V[0] + dA[1] * V[4] + dA[2] * V[8];
    const float dJ02 = dA[0] * V[2] + dA[1] * V[6] + dA[2] * V[10];
    const float dJ11 = dA[3] * V[1] + dA[4] * V[5] + dA[5] * V[9];
    const float dJ12 = dA[3] * V[2] + dA[4] * V[6] + dA[5] * V[10];
    const float tz = 1.f / j.tz, tz2 = tz * tz, tz3 = tz2 * tz;
    const float dtx = j.clamp_x ? 0.f : (-j.fx * tz2 * dJ02);
    const float dty = j.clamp_y ? 0.f : (-j.fy * tz2 * dJ12);
    const float dtz = -j.fx * tz2 * dJ00 - j.fy * tz2 * dJ11 + (2.f * j.fx * j.tx) * tz3 * dJ02 +
                      (2.f * j.fy * j.ty) * tz3 * dJ12;
    float dpx = V[0] * dtx + V[1] * dty + V[2] * dtz;
    float dpy = V[4] * dtx + V[5] * dty + V[6] * dtz;
    float dpz = V[8] * dtx + V[9] * dty + V[10] * dtz;
    const float gnx = gmean_x * 0.5f * (float)W;
    const float gny = gmean_y * 0.5f * (float)H;
    const float hx = Pm[0] * p.x + Pm[4] * p.y + Pm[8] * p.z + Pm[12];
    const float hy = Pm[1] * p.x + Pm[5] * p.y + Pm[9] * p.z + Pm[13];
    const float hwv = Pm[3] * p.x + Pm[7] * p.y + Pm[11] * p.z + Pm[15];
    const float mw = 1.f / (hwv + 0.0000001f);
    const float mx = hx * mw * mw, my = hy * mw * mw;
    dpx += (Pm[0] * mw - Pm[3] * mx) * gnx + (Pm[1] * mw - Pm[3] * my) * gny;
    dpy += (Pm[4] * mw - Pm[7] * mx) * gnx + (Pm[5] * mw - Pm[7] * my) * gny;
    dpz += (Pm[8] * mw - Pm[11] * mx) * gnx + (Pm[9] * mw - Pm[11] * my) * gny;
    o.dp[0] = dpx;
    o.dp[1] = dpy;
    o.dp[2] = dpz;
    o.dm2[0] = gnx;
    o.dm2[1] = gny;
    o.dm2[2] = 0.f;
}
