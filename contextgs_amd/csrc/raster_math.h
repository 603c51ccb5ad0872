// Per-Gaussian projection math shared by the forward preprocess, the
// visibility filter and the preprocess backward (which recomputes the forward
// intermediates instead of storing 100+ bytes per Gaussian in HBM).
//
// Conventions: matrices are row-major fp32 in the
// reference's ROW-vector convention, p' = [x y z 1] @ M.  Quaternions are
// (r, x, y, z) and are used as given.
#pragma once
#include <hip/hip_runtime.h>

struct CgsProj {
    float px, py;          // pixel-space centre
    float depth;           // view-space z
    float con_a, con_b, con_c;   // conic = inverse of the dilated 2-D covariance
    float cov_a, cov_b, cov_c;   // dilated 2-D covariance
    float radius;          // ceil(3 sigma_max)
    float aa_h;            // antialiasing only (AA = true): the opacity factor of cgs_aa_h
};

struct CgsCov3 { float xx, xy, xz, yy, yz, zz; };

__device__ __forceinline__ void cgs_quat_to_rot(const float4 q, float R[9]) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - r * z);       R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y);       R[7] = 2.f * (y * z + r * x);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// Sigma = R diag(s^2) R^T
__device__ __forceinline__ CgsCov3 cgs_cov3d(const float3 s, const float R[9]) {
    const float sx = s.x * s.x, sy = s.y * s.y, sz = s.z * s.z;
    CgsCov3 c;
    c.xx = R[0] * R[0] * sx + R[1] * R[1] * sy + R[2] * R[2] * sz;
    c.xy = R[0] * R[3] * sx + R[1] * R[4] * sy + R[2] * R[5] * sz;
    c.xz = R[0] * R[6] * sx + R[1] * R[7] * sy + R[2] * R[8] * sz;
    c.yy = R[3] * R[3] * sx + R[4] * R[4] * sy + R[5] * R[5] * sz;
    c.yz = R[3] * R[6] * sx + R[4] * R[7] * sy + R[5] * R[8] * sz;
    c.zz = R[6] * R[6] * sx + R[7] * R[7] * sy + R[8] * R[8] * sz;
    return c;
}

// View-space position (row-vector convention).
__device__ __forceinline__ float3 cgs_to_view(const float3 p, const float *V) {
    return make_float3(V[0] * p.x + V[4] * p.y + V[8] * p.z + V[12],
                       V[1] * p.x + V[5] * p.y + V[9] * p.z + V[13],
                       V[2] * p.x + V[6] * p.y + V[10] * p.z + V[14]);
}

// A = J * Wv: 2x3 Jacobian of the (clamped) perspective map times the
// world->view rotation.  t is the view-space point, returns clamp flags so the
// backward pass can zero the derivative through a clamped coordinate.
struct CgsJac { float A[6]; float tx, ty, tz; bool clamp_x, clamp_y; float fx, fy; };

__device__ __forceinline__ CgsJac cgs_jacobian(const float3 t, const float *V, int W, int H, float tanfovx,
                                               float tanfovy) {
    CgsJac j;
    const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    j.clamp_x = (txtz < -limx) || (txtz > limx);
    j.clamp_y = (tytz < -limy) || (tytz > limy);
    j.tx = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    j.ty = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    j.tz = t.z;
    j.fx = (float)W / (2.f * tanfovx);
    j.fy = (float)H / (2.f * tanfovy);
    const float j00 = j.fx / j.tz, j02 = -(j.fx * j.tx) / (j.tz * j.tz);
    const float j11 = j.fy / j.tz, j12 = -(j.fy * j.ty) / (j.tz * j.tz);
    // Wv[i][c] = V[4*c + i]
    j.A[0] = j00 * V[0] + j02 * V[2];
    j.A[1] = j00 * V[4] + j02 * V[6];
    j.A[2] = j00 * V[8] + j02 * V[10];
    j.A[3] = j11 * V[1] + j12 * V[2];
    j.A[4] = j11 * V[5] + j12 * V[6];
    j.A[5] = j11 * V[9] + j12 * V[10];
    return j;
}

// cov2D = A Sigma A^T (before dilation)
__device__ __forceinline__ void cgs_cov2d(const float A[6], const CgsCov3 &c, float &a, float &b, float &cc) {
    const float u0 = c.xx * A[0] + c.xy * A[1] + c.xz * A[2];
    const float u1 = c.xy * A[0] + c.yy * A[1] + c.yz * A[2];
    const float u2 = c.xz * A[0] + c.yz * A[1] + c.zz * A[2];
    const float w0 = c.xx * A[3] + c.xy * A[4] + c.xz * A[5];
    const float w1 = c.xy * A[3] + c.yy * A[4] + c.yz * A[5];
    const float w2 = c.xz * A[3] + c.yz * A[4] + c.zz * A[5];
    a = A[0] * u0 + A[1] * u1 + A[2] * u2;
    b = A[3] * u0 + A[4] * u1 + A[5] * u2;
    cc = A[3] * w0 + A[4] * w1 + A[5] * w2;
}

// ---- antialiasing (upstream's `antialiasing`, the 2-D filter of Mip-Splatting) -------------------------------------------
// With [[a, b], [b, c]] the 2-D covariance BEFORE the 0.3 px^2 dilation:
//   d0 = a c - b^2,  d1 = (a + 0.3)(c + 0.3) - b^2 = d0 + 0.3 (a + c) + 0.09,  h = sqrt(max(2.5e-5, d0 / d1))
// and the blend reads opacity * h: the dilation widens the splat, h keeps its integrated alpha.  The conic and the radius
// stay those of the dilated covariance.  d0 is formed without the cancellation of a c - b^2 (thin, oblique Gaussians):
// cgs_det2_rs / cgs_det2_comp below.
#define CGS_AA_R_MIN 2.5e-5f

// d0 from scales / rotations: cov2D = M M^T with M = A R diag(s) (2x3), so by Cauchy-Binet det = the sum of the squared 2x2
// minors of M - a sum of squares.  s = the scales with scale_modifier applied.
__device__ __forceinline__ float cgs_det2_rs(const float A[6], const float R[9], const float3 s) {
    const float sv[3] = {s.x, s.y, s.z};
    float m0[3], m1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m0[k] = sv[k] * (A[0] * R[k] + A[1] * R[3 + k] + A[2] * R[6 + k]);
        m1[k] = sv[k] * (A[3] * R[k] + A[4] * R[3 + k] + A[5] * R[6 + k]);
    }
    const float n01 = m0[0] * m1[1] - m0[1] * m1[0];
    const float n02 = m0[0] * m1[2] - m0[2] * m1[0];
    const float n12 = m0[1] * m1[2] - m0[2] * m1[1];
    return n01 * n01 + n02 * n02 + n12 * n12;
}

// d0 from a given covariance: a c - b^2 with the rounding error of b^2 put back (Kahan's fma-compensated difference; an
// explicit fmaf is fused whatever -ffp-contract says)
__device__ __forceinline__ float cgs_det2_comp(float a, float b, float c) {
    const float bb = b * b;
    const float err = fmaf(b, b, -bb);          // b^2 - bb, exactly
    return fmaf(a, c, -bb) - err;
}

// h of the undilated (a, c) and d0; d1 out (the backward's denominator)
__device__ __forceinline__ float cgs_aa_h(float d0, float a, float c, float &d1) {
    d1 = d0 + 0.3f * (a + c) + 0.09f;
    return sqrtf(fmaxf(CGS_AA_R_MIN, d0 / d1));
}

// dL/d(a, b, c) of h * op with dL/d(op_eff) = g (b as ONE variable, the convention of the conic chain's repeated entry):
// zero where the clamp holds
__device__ __forceinline__ void cgs_aa_bwd(float d0, float d1, float h, float a, float b, float c, float g, float op, float &ga,
                                           float &gb, float &gc) {
    ga = gb = gc = 0.f;
    if (d0 / d1 > CGS_AA_R_MIN) {
        const float k = g * op / (2.f * h * d1 * d1);
        ga = k * (c * d1 - d0 * (c + 0.3f));
        gc = k * (a * d1 - d0 * (a + 0.3f));
        gb = k * (-2.f * b * (d1 - d0));
    }
}

template <typename T /*unused, float only*/, bool AA = false>
__device__ __forceinline__ bool cgs_project(const float3 p, const float3 s, const float4 q, const float *V,
                                            const float *Pm, int W, int H, float tanfovx, float tanfovy,
                                            float scale_modifier, CgsProj &o) {
    const float3 t = cgs_to_view(p, V);
    if (t.z <= 0.2f) return false;   // near cull: the only frustum test
    const float hx = Pm[0] * p.x + Pm[4] * p.y + Pm[8] * p.z + Pm[12];
    const float hy = Pm[1] * p.x + Pm[5] * p.y + Pm[9] * p.z + Pm[13];
    const float hw = Pm[3] * p.x + Pm[7] * p.y + Pm[11] * p.z + Pm[15];
    const float pw = 1.f / (hw + 0.0000001f);
    const float ndcx = hx * pw, ndcy = hy * pw;

    float R[9];
    cgs_quat_to_rot(q, R);
    const float3 sm = make_float3(s.x * scale_modifier, s.y * scale_modifier, s.z * scale_modifier);
    const CgsCov3 c3 = cgs_cov3d(sm, R);
    const CgsJac j = cgs_jacobian(t, V, W, H, tanfovx, tanfovy);
    float a, b, c;
    cgs_cov2d(j.A, c3, a, b, c);
    if constexpr (AA) {
        float d1;
        o.aa_h = cgs_aa_h(cgs_det2_rs(j.A, R, sm), a, c, d1);
    }
    a += 0.3f;
    c += 0.3f;
    const float det = a * c - b * b;
    if (det == 0.f) return false;
    const float inv = 1.f / det;
    o.con_a = c * inv; o.con_b = -b * inv; o.con_c = a * inv;
    o.cov_a = a; o.cov_b = b; o.cov_c = c;
    const float mid = 0.5f * (a + c);
    // mid^2 - det = ((a - c) / 2)^2 + b^2: the sum of squares, not the difference of two near-equal squares (that one lost
    // ~1e-2 absolutely at mid ~ 400 and moved ceil() below on the last ulp - 4K frame: radii off the oracle's)
    const float hd = 0.5f * (a - c);
    const float disc = sqrtf(fmaxf(0.1f, hd * hd + b * b));
    o.radius = ceilf(3.f * sqrtf(fmaxf(mid + disc, mid - disc)));
    o.px = ((ndcx + 1.f) * (float)W - 1.f) * 0.5f;
    o.py = ((ndcy + 1.f) * (float)H - 1.f) * 0.5f;
    o.depth = t.z;
    return true;
}
