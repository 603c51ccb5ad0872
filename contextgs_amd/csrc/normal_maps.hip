// Normal maps and the normal-consistency regulariser (include/cgs.h has the definitions and the gradients):
//   gaussian normals   per Gaussian: the axis of its smallest scale, in view space, turned away from the camera
//   depth normals      per pixel: the normal of the surface a depth map describes (a 4-neighbour stencil, edges replicated)
//   normal consistency per pixel: E = 1 - m <normals, depth normal>, the depth normal computed on the fly
// Everything here streams: one thread per Gaussian or per pixel, rows of 64 pixels per wave so that every plane is read and
// written in whole 256-byte runs, 64 x 4 pixel blocks so that the stencil's halo rows are the block's own rows or a
// neighbouring block's (L1 / L2 hits).  No LDS, and no float atomics anywhere: every backward is a gather in a fixed order,
// so two runs give the same bits.
#include "cgs_internal.h"

#define NM_BX 64
#define NM_BY 4

// 1 / fx, 1 / fy are taken once on the host: the kernels are bound by their arithmetic (up to five stencils per pixel in the
// backwards), and an IEEE division per coordinate of every back-projected point was most of it
struct NmCam {
    int H, W;
    float ifx, ify, cx, cy, eps;
};

static NmCam nm_cam(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps) {
    NmCam c;
    c.H = H;
    c.W = W;
    c.ifx = (2.f * tanfovx) / (float)W;
    c.ify = (2.f * tanfovy) / (float)H;
    c.cx = 0.5f * (float)W;
    c.cy = 0.5f * (float)H;
    c.eps = eps;
    return c;
}

__device__ __forceinline__ float3 nm_sub(const float3 a, const float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 nm_cross(const float3 a, const float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float nm_dot(const float3 a, const float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the view-space point of pixel (v, u): integer pixel coordinates, principal point (W/2, H/2)
__device__ __forceinline__ float3 nm_pos(const float *__restrict__ depth, const NmCam &c, int v, int u) {
    const float d = depth[(size_t)v * c.W + u];
    return make_float3(d * (((float)u - c.cx) * c.ifx), d * (((float)v - c.cy) * c.ify), d);
}

// d0 = p(v+1, u) - p(v-1, u), d1 = p(v, u+1) - p(v, u-1) with replicated edges, n = d0 x d1, len = |n|
struct NmStencil { float3 d0, d1, n; float len; };

__device__ __forceinline__ NmStencil nm_stencil(const float *__restrict__ depth, const NmCam &c, int v, int u) {
    const int vp = min(v + 1, c.H - 1), vm = max(v - 1, 0), up = min(u + 1, c.W - 1), um = max(u - 1, 0);
    NmStencil s;
    s.d0 = nm_sub(nm_pos(depth, c, vp, u), nm_pos(depth, c, vm, u));
    s.d1 = nm_sub(nm_pos(depth, c, v, up), nm_pos(depth, c, v, um));
    s.n = nm_cross(s.d0, s.d1);
    s.len = sqrtf(nm_dot(s.n, s.n));
    return s;
}

// N = -n / (|n| + eps); 0 where the denominator is 0
__device__ __forceinline__ float3 nm_normal(const NmStencil &s, float eps) {
    const float den = s.len + eps;
    if (!(den > 0.f)) return make_float3(0.f, 0.f, 0.f);
    const float inv = -1.f / den;
    return make_float3(s.n.x * inv, s.n.y * inv, s.n.z * inv);
}

// dL/dn from G = dL/dN: -G / den + n (G . n) / (|n| den^2); the second term (the norm's own gradient) is 0 where |n| = 0
__device__ __forceinline__ float3 nm_grad_n(const NmStencil &s, const float3 G, float eps) {
    const float den = s.len + eps;
    if (!(den > 0.f)) return make_float3(0.f, 0.f, 0.f);
    const float inv = 1.f / den;
    float3 g = make_float3(-G.x * inv, -G.y * inv, -G.z * inv);
    if (s.len > 0.f) {
        const float k = nm_dot(G, s.n) * (inv * inv) / s.len;
        g.x += s.n.x * k;
        g.y += s.n.y * k;
        g.z += s.n.z * k;
    }
    return g;
}

// dL/ddepth[v, u] as a gather: the stencils that read pixel (v, u) are those of its (up to four) neighbours and, on an image
// edge, its own replicated copy.  Each one's dL/dd0 = d1 x dL/dn and dL/dd1 = dL/dn x d0 is recomputed and added with the sign
// the stencil read the pixel with (+ as the v+1 / u+1 operand, - as the v-1 / u-1 operand), in a fixed order.  G_at(qv, qu)
// gives dL/dN of stencil q.
template <typename GF>
__device__ __forceinline__ float nm_depth_grad(const float *__restrict__ depth, const NmCam &c, int v, int u, GF G_at) {
    float3 gp = make_float3(0.f, 0.f, 0.f);
    auto add = [&](int qv, int qu, float c0, float c1) {
        const NmStencil s = nm_stencil(depth, c, qv, qu);
        const float3 gn = nm_grad_n(s, G_at(qv, qu), c.eps);
        if (c0 != 0.f) {
            const float3 g0 = nm_cross(s.d1, gn);
            gp.x += c0 * g0.x; gp.y += c0 * g0.y; gp.z += c0 * g0.z;
        }
        if (c1 != 0.f) {
            const float3 g1 = nm_cross(gn, s.d0);
            gp.x += c1 * g1.x; gp.y += c1 * g1.y; gp.z += c1 * g1.z;
        }
    };
    if (v > 0) add(v - 1, u, 1.f, 0.f);
    if (v < c.H - 1) add(v + 1, u, -1.f, 0.f);
    if (u > 0) add(v, u - 1, 0.f, 1.f);
    if (u < c.W - 1) add(v, u + 1, 0.f, -1.f);
    // the pixel's own stencil reads it where an edge is replicated (both copies on a one-pixel axis: they cancel to 0)
    const float e0 = (float)(v == c.H - 1) - (float)(v == 0), e1 = (float)(u == c.W - 1) - (float)(u == 0);
    if (e0 != 0.f || e1 != 0.f) add(v, u, e0, e1);
    return gp.x * (((float)u - c.cx) * c.ifx) + gp.y * (((float)v - c.cy) * c.ify) + gp.z;
}

// ---- depth normals ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NM_BX * NM_BY) depth_normals_fwd_kernel(NmCam c, const float *__restrict__ depth,
                                                                           float *__restrict__ out) {
    const int u = blockIdx.x * NM_BX + threadIdx.x, v = blockIdx.y * NM_BY + threadIdx.y;
    if (u >= c.W || v >= c.H) return;
    const float3 N = nm_normal(nm_stencil(depth, c, v, u), c.eps);
    const size_t plane = (size_t)c.H * c.W, i = (size_t)v * c.W + u;
    out[i] = N.x;
    out[plane + i] = N.y;
    out[2 * plane + i] = N.z;
}

__global__ void __launch_bounds__(NM_BX * NM_BY) depth_normals_bwd_kernel(NmCam c, const float *__restrict__ depth,
                                                                           const float *__restrict__ dL_dout,
                                                                           float *__restrict__ dL_ddepth) {
    const int u = blockIdx.x * NM_BX + threadIdx.x, v = blockIdx.y * NM_BY + threadIdx.y;
    if (u >= c.W || v >= c.H) return;
    const size_t plane = (size_t)c.H * c.W;
    auto G_at = [&](int qv, int qu) {
        const size_t q = (size_t)qv * c.W + qu;
        return make_float3(dL_dout[q], dL_dout[plane + q], dL_dout[2 * plane + q]);
    };
    dL_ddepth[(size_t)v * c.W + u] = nm_depth_grad(depth, c, v, u, G_at);
}

// ---- normal consistency ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NM_BX * NM_BY) normal_consistency_fwd_kernel(NmCam c, const float *__restrict__ normals,
                                                                                const float *__restrict__ depth,
                                                                                const float *__restrict__ weight,
                                                                                float *__restrict__ out) {
    const int u = blockIdx.x * NM_BX + threadIdx.x, v = blockIdx.y * NM_BY + threadIdx.y;
    if (u >= c.W || v >= c.H) return;
    const float3 N = nm_normal(nm_stencil(depth, c, v, u), c.eps);
    const size_t plane = (size_t)c.H * c.W, i = (size_t)v * c.W + u;
    const float m = weight ? weight[i] : 1.f;
    out[i] = 1.f - m * nm_dot(make_float3(normals[i], normals[plane + i], normals[2 * plane + i]), N);
}

__global__ void __launch_bounds__(NM_BX * NM_BY) normal_consistency_bwd_kernel(NmCam c, const float *__restrict__ normals,
                                                                                const float *__restrict__ depth,
                                                                                const float *__restrict__ weight,
                                                                                const float *__restrict__ dL_dE,
                                                                                float *__restrict__ dL_dnormals,
                                                                                float *__restrict__ dL_ddepth) {
    const int u = blockIdx.x * NM_BX + threadIdx.x, v = blockIdx.y * NM_BY + threadIdx.y;
    if (u >= c.W || v >= c.H) return;
    const size_t plane = (size_t)c.H * c.W, i = (size_t)v * c.W + u;
    // dL/d(normals . N) of stencil q = -m[q] dL/dE[q]
    auto k_at = [&](size_t q) { return -(weight ? weight[q] : 1.f) * dL_dE[q]; };
    if (dL_dnormals) {      // (either output may be NULL: an input that asked for no gradient)
        const float3 N = nm_normal(nm_stencil(depth, c, v, u), c.eps);
        const float k = k_at(i);
        dL_dnormals[i] = k * N.x;
        dL_dnormals[plane + i] = k * N.y;
        dL_dnormals[2 * plane + i] = k * N.z;
    }
    if (!dL_ddepth) return;
    auto G_at = [&](int qv, int qu) {
        const size_t q = (size_t)qv * c.W + qu;
        const float kq = k_at(q);
        return make_float3(kq * normals[q], kq * normals[plane + q], kq * normals[2 * plane + q]);
    };
    dL_ddepth[i] = nm_depth_grad(depth, c, v, u, G_at);
}

// ---- per-Gaussian normals ---------------------------------------------------------------------------------------------------
// column k of R(q) for a unit quaternion (r, x, y, z), R as in cgs_quat_to_rot
__device__ __forceinline__ float3 nm_rot_column(int k, float r, float x, float y, float z) {
    if (k == 0) return make_float3(1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y));
    if (k == 1) return make_float3(2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x));
    return make_float3(2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y));
}

// what a Gaussian's normal is made of: the axis index, the unit quaternion and 1 / |q| (0 for the zero quaternion, which
// then reads as the identity rotation), and the sign that turns the view-space axis away from the camera
struct NmAxis { int k; float r, x, y, z, inv_len, sign; float3 n_view; };

__device__ __forceinline__ NmAxis nm_axis(const float *__restrict__ V, const float *__restrict__ means3D,
                                          const float *__restrict__ scales, const float *__restrict__ rotations, int64_t i) {
    NmAxis a;
    const float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    a.k = 0;
    float smin = s0;
    if (s1 < smin) { a.k = 1; smin = s1; }
    if (s2 < smin) a.k = 2;
    // (scalar accesses: a caller's [P, 4] view may start at any float of a larger buffer)
    const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
    const float len = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    a.inv_len = len > 0.f ? 1.f / len : 0.f;
    a.r = q.x * a.inv_len; a.x = q.y * a.inv_len; a.y = q.z * a.inv_len; a.z = q.w * a.inv_len;
    const float3 nw = nm_rot_column(a.k, a.r, a.x, a.y, a.z);
    // n_v = n_w @ V[:3,:3], t = [p, 1] @ V (row vectors, V[4 row + column])
    a.n_view = make_float3(nw.x * V[0] + nw.y * V[4] + nw.z * V[8], nw.x * V[1] + nw.y * V[5] + nw.z * V[9],
                           nw.x * V[2] + nw.y * V[6] + nw.z * V[10]);
    const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
    const float3 t = make_float3(px * V[0] + py * V[4] + pz * V[8] + V[12], px * V[1] + py * V[5] + pz * V[9] + V[13],
                                 px * V[2] + py * V[6] + pz * V[10] + V[14]);
    a.sign = nm_dot(a.n_view, t) >= 0.f ? 1.f : -1.f;
    return a;
}

__global__ void __launch_bounds__(256) gaussian_normals_fwd_kernel(int64_t P, const float *__restrict__ V,
                                                                   const float *__restrict__ means3D,
                                                                   const float *__restrict__ scales,
                                                                   const float *__restrict__ rotations, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const NmAxis a = nm_axis(V, means3D, scales, rotations, i);
    out[3 * i] = a.sign * a.n_view.x;
    out[3 * i + 1] = a.sign * a.n_view.y;
    out[3 * i + 2] = a.sign * a.n_view.z;
}

// one thread owns a row of dL_drotations: no atomics
__global__ void __launch_bounds__(256) gaussian_normals_bwd_kernel(int64_t P, const float *__restrict__ V,
                                                                   const float *__restrict__ means3D,
                                                                   const float *__restrict__ scales,
                                                                   const float *__restrict__ rotations,
                                                                   const float *__restrict__ dL_dout,
                                                                   float *__restrict__ dL_drotations) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const NmAxis a = nm_axis(V, means3D, scales, rotations, i);
    const float gx = a.sign * dL_dout[3 * i], gy = a.sign * dL_dout[3 * i + 1], gz = a.sign * dL_dout[3 * i + 2];
    // dL/dn_w = V[:3,:3] dL/dn_v
    const float g0 = V[0] * gx + V[1] * gy + V[2] * gz, g1 = V[4] * gx + V[5] * gy + V[6] * gz,
                g2 = V[8] * gx + V[9] * gy + V[10] * gz;
    const float r = a.r, x = a.x, y = a.y, z = a.z;
    float dr, dx, dy, dz;       // dL/d(unit quaternion)
    if (a.k == 0) {
        dr = 2.f * (z * g1 - y * g2);
        dx = 2.f * (y * g1 + z * g2);
        dy = -4.f * y * g0 + 2.f * (x * g1 - r * g2);
        dz = -4.f * z * g0 + 2.f * (r * g1 + x * g2);
    } else if (a.k == 1) {
        dr = 2.f * (x * g2 - z * g0);
        dx = -4.f * x * g1 + 2.f * (y * g0 + r * g2);
        dy = 2.f * (x * g0 + z * g2);
        dz = -4.f * z * g1 + 2.f * (y * g2 - r * g0);
    } else {
        dr = 2.f * (y * g0 - x * g1);
        dx = -4.f * x * g2 + 2.f * (z * g0 - r * g1);
        dy = -4.f * y * g2 + 2.f * (r * g0 + z * g1);
        dz = 2.f * (x * g0 + y * g1);
    }
    // through q / |q|: (g - q^ (q^ . g)) / |q|
    const float along = r * dr + x * dx + y * dy + z * dz;
    dL_drotations[4 * i] = (dr - r * along) * a.inv_len;
    dL_drotations[4 * i + 1] = (dx - x * along) * a.inv_len;
    dL_drotations[4 * i + 2] = (dy - y * along) * a.inv_len;
    dL_drotations[4 * i + 3] = (dz - z * along) * a.inv_len;
}

// ---- launchers (csrc/api.hip checks the arguments) ----------------------------------------------------------------------------
static dim3 nm_grid(int32_t H, int32_t W) { return dim3((W + NM_BX - 1) / NM_BX, (H + NM_BY - 1) / NM_BY); }

int cgs_launch_gaussian_normals_fwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                    const float *rotations, float *out, hipStream_t stream) {
    if (P == 0) return CGS_OK;
    hipLaunchKernelGGL(gaussian_normals_fwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, cfg->viewmatrix,
                       means3D, scales, rotations, out);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_gaussian_normals_bwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                    const float *rotations, const float *dL_dout, float *dL_drotations, hipStream_t stream) {
    if (P == 0) return CGS_OK;
    hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, cfg->viewmatrix,
                       means3D, scales, rotations, dL_dout, dL_drotations);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_depth_normals_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth, float *out,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(depth_normals_fwd_kernel, nm_grid(H, W), dim3(NM_BX, NM_BY), 0, stream,
                       nm_cam(H, W, tanfovx, tanfovy, eps), depth, out);
    CGS_CHECK_LAUNCH(stream, 0);
    return CGS_OK;
}

int cgs_launch_depth_normals_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth,
                                 const float *dL_dout, float *dL_ddepth, hipStream_t stream) {
    hipLaunchKernelGGL(depth_normals_bwd_kernel, nm_grid(H, W), dim3(NM_BX, NM_BY), 0, stream,
                       nm_cam(H, W, tanfovx, tanfovy, eps), depth, dL_dout, dL_ddepth);
    CGS_CHECK_LAUNCH(stream, 0);
    return CGS_OK;
}

int cgs_launch_normal_consistency_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                      const float *depth, const float *weight, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(normal_consistency_fwd_kernel, nm_grid(H, W), dim3(NM_BX, NM_BY), 0, stream,
                       nm_cam(H, W, tanfovx, tanfovy, eps), normals, depth, weight, out);
    CGS_CHECK_LAUNCH(stream, 0);
    return CGS_OK;
}

int cgs_launch_normal_consistency_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                      const float *depth, const float *weight, const float *dL_dE, float *dL_dnormals,
                                      float *dL_ddepth, hipStream_t stream) {
    hipLaunchKernelGGL(normal_consistency_bwd_kernel, nm_grid(H, W), dim3(NM_BX, NM_BY), 0, stream,
                       nm_cam(H, W, tanfovx, tanfovy, eps), normals, depth, weight, dL_dE, dL_dnormals, dL_ddepth);
    CGS_CHECK_LAUNCH(stream, 0);
    return CGS_OK;
}
