// Monocular depth priors (contextgs_amd/depth_prior.py; the definition is in include/cgs.h above cgs_depth_prior_fwd).
//
//   moments      dp_moment_kernel: a workgroup walks tiles of 1024 consecutive pixels of the flattened planes (a lane takes four
//                consecutive pixels: one 16-byte access per float plane, one 4-byte access of a byte mask, when the bases are
//                aligned, with the last partial quad of an H*W that is no multiple of 4 taken pixel by pixel; the same four pixels
//                with scalar accesses when a base is not aligned, so the sums do not depend on the alignment).  M, Sx, Sy, Sxx,
//                Syy, Sxy accumulate in fp64 per lane; a product of two fp32 inputs is exact in fp64.  One fixed-order wave + LDS
//                reduction gives the workgroup's record of partials.
//   finish       dp_finish_moments_kernel: one workgroup adds the records in a fixed order and solves in fp64: the least-squares
//                (a, b), the closed-form L2 value, 1 - rho, and the coefficients the backward needs (coef, 8 doubles).
//   residual     dp_resid_kernel / dp_finish_resid_kernel: sum m |r| or sum m r^2 with r formed per pixel in fp64 from the fp64
//                coefficients (L1 after a least-squares fit; both kinds with a given affine map).
//   backward     dp_bwd_kernel: d x per pixel, one launch; dp_dab_kernel + dp_finish_dab_kernel: d (a, b) of a given affine map.
// A pixel of mask 0 is selected out: its x and y are replaced by 0 before any arithmetic, and its gradient is stored as +0.
// No float atomics anywhere; every sum is added in a fixed order, so two calls give the same bytes.
#include "cgs_internal.h"

namespace {

constexpr int DP_THREADS = 256;                 // also the threads of the finishing kernels
constexpr int DP_PX = 4;
constexpr int DP_TILE = DP_THREADS * DP_PX;
constexpr int DP_MAX_BLOCKS = 1024;             // four workgroups per compute unit; beyond it a workgroup walks several tiles
constexpr int DP_REC = 8;                       // doubles per workgroup record of partials (6 moments; 2 residual or d(a, b) sums)
constexpr double DP_DEGENERATE = 1e-12;
// coef: t_p = c2 x_p + c1 y_p + c0 is the residual x - (a y + b) (c2 = 1, c1 = -a, c0 = -b) or the bracket of the Pearson gradient
enum { DPC_C0 = 0, DPC_C1, DPC_C2, DPC_SCALE, DPC_A, DPC_B, DPC_M, DPC_LOSS, DPC_COUNT };
static_assert(DPC_COUNT * sizeof(double) == CGS_DEPTH_PRIOR_COEF_BYTES, "the coefficient record of include/cgs.h");
enum { DP_FIN_LSTSQ_L1 = 0, DP_FIN_LSTSQ_L2, DP_FIN_PEARSON, DP_FIN_SCALE_SHIFT };

// VEC: the plane's base is 16-byte aligned, so a lane's four pixels are one 16-byte access — except the last, partial quad when
// H*W is no multiple of 4, which goes pixel by pixel.  Either way a lane holds the same four pixels.
template <bool VEC> __device__ __forceinline__ void dp_load4(const float *__restrict__ plane, uint32_t p0, uint32_t n, float v[4]) {
    if (VEC && p0 + 3 < n) {
        const float4 t = *reinterpret_cast<const float4 *>(plane + p0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (p0 + k < n) ? plane[p0 + k] : 0.0f;
    }
}

// the weights of four pixels; 0 beyond the last pixel
template <int MASK, bool VEC> __device__ __forceinline__ void dp_mask4(const void *__restrict__ mask, uint32_t p0, uint32_t n, float m[4]) {
    if (MASK == CGS_DP_MASK_NONE) {
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = (p0 + k < n) ? 1.0f : 0.0f;
    } else if (MASK == CGS_DP_MASK_FLOAT) {
        dp_load4<VEC>((const float *)mask, p0, n, m);
    } else {
        const uint8_t *b = (const uint8_t *)mask;
        if (VEC && p0 + 3 < n) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(b + p0);
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = ((w >> (8 * k)) & 255u) ? 1.0f : 0.0f;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = (p0 + k < n && b[p0 + k]) ? 1.0f : 0.0f;
        }
    }
}

// One lane's four pixels as fp64 (w, x, y); a pixel of weight 0 contributes (0, 0, 0) whatever its x and y hold.
template <int MASK, bool VEC>
__device__ __forceinline__ void dp_pixels(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ mask,
                                          uint32_t p0, uint32_t n, double w[4], double xd[4], double yd[4]) {
    float xv[4], yv[4], m[4];
    dp_load4<VEC>(x, p0, n, xv);
    dp_load4<VEC>(y, p0, n, yv);
    dp_mask4<MASK, VEC>(mask, p0, n, m);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool on = m[k] != 0.0f;
        w[k] = on ? (double)m[k] : 0.0;
        xd[k] = on ? (double)xv[k] : 0.0;
        yd[k] = on ? (double)yv[k] : 0.0;
    }
}

__device__ __forceinline__ double dp_t(double xd, double yd, double c0, double c1, double c2) { return fma(c2, xd, fma(c1, yd, c0)); }
// d rho(t) / d t without the 1 / N: sign(t) (sign(0) = 0) for L1, 2 t for L2
__device__ __forceinline__ double dp_w(int kind, double t) {
    if (kind == CGS_DP_L2) return 2.0 * t;
    return t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);
}

// The workgroup's sums of v[0..NQ), in a fixed order, into dst[0..NQ) (global or LDS) by the first NQ threads.
template <int NQ> __device__ __forceinline__ void dp_block_sum(double (&v)[NQ], double *red, double *dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        double t = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if (lane == 0) red[wave * NQ + q] = t;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        double t = red[threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < DP_THREADS / 64; wv++) t += red[wv * NQ + threadIdx.x];
        dst[threadIdx.x] = t;
    }
}

// tot[0..NQ) (LDS) = the records' sums: thread i adds records i, i + 256, ... in index order, then the workgroup's fixed order
template <int NQ> __device__ __forceinline__ void dp_sum_records(const double *__restrict__ part, int nb, double *red, double *tot) {
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = 0.0;
    for (int i = threadIdx.x; i < nb; i += DP_THREADS)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[q] += part[(size_t)i * DP_REC + q];
    dp_block_sum<NQ>(acc, red, tot);
    __syncthreads();
}

template <int MASK, bool VEC>
__global__ void __launch_bounds__(DP_THREADS)
    dp_moment_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ mask, uint32_t n, uint32_t ntiles,
                     double *__restrict__ part) {
    __shared__ double red[(DP_THREADS / 64) * 6];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t p0 = tile * (uint32_t)DP_TILE + threadIdx.x * (uint32_t)DP_PX;
        if (p0 >= n) continue;
        double w[4], xd[4], yd[4];
        dp_pixels<MASK, VEC>(x, y, mask, p0, n, w, xd, yd);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double wx = w[k] * xd[k], wy = w[k] * yd[k];
            acc[0] += w[k];
            acc[1] += wx;
            acc[2] += wy;
            acc[3] += wx * xd[k];
            acc[4] += wy * yd[k];
            acc[5] += wx * yd[k];
        }
    }
    dp_block_sum<6>(acc, red, part + (size_t)blockIdx.x * DP_REC);
}

__global__ void __launch_bounds__(DP_THREADS)
    dp_finish_moments_kernel(const double *__restrict__ part, int nb, double npix, int fin, int mean_over, double *__restrict__ coef,
                             float *__restrict__ out) {
    __shared__ double red[(DP_THREADS / 64) * 6];
    __shared__ double tot[6];
    dp_sum_records<6>(part, nb, red, tot);
    if (threadIdx.x != 0) return;
    const double M = tot[0], Sx = tot[1], Sy = tot[2], Sxx = tot[3], Syy = tot[4], Sxy = tot[5];
    const double Vx = M * Sxx - Sx * Sx, Vy = M * Syy - Sy * Sy, C = M * Sxy - Sx * Sy;
    const bool degx = !(Vx > DP_DEGENERATE * M * Sxx), degy = !(Vy > DP_DEGENERATE * M * Syy);
    const double a = degy ? 0.0 : C / Vy;
    const double b = M > 0.0 ? (Sx - a * Sy) / M : 0.0;
    if (fin == DP_FIN_SCALE_SHIFT) {
        out[0] = (float)a;
        out[1] = (float)b;
        return;
    }
    double c0, c1, c2, scale, loss;
    if (fin == DP_FIN_PEARSON) {
        if (degx || degy) {
            c0 = c1 = c2 = 0.0;
            loss = 1.0;
        } else {
            const double s = sqrt(Vx * Vy), rho = C / s;
            c1 = -M / s;
            c2 = rho * M / Vx;
            c0 = Sy / s - rho * Sx / Vx;
            loss = 1.0 - rho;
        }
        scale = 1.0;
    } else {
        const double N = mean_over == CGS_DP_MEAN_IMAGE ? npix : M;
        scale = N > 0.0 ? 1.0 / N : 0.0;
        c0 = -b; c1 = -a; c2 = 1.0;
        // sum m (x - a y - b)^2 at the least-squares (a, b) = (Vx - a C) / M
        loss = M > 0.0 ? fmax((Vx - a * C) / M, 0.0) * scale : 0.0;
    }
    coef[DPC_C0] = c0; coef[DPC_C1] = c1; coef[DPC_C2] = c2; coef[DPC_SCALE] = scale;
    coef[DPC_A] = a; coef[DPC_B] = b; coef[DPC_M] = M; coef[DPC_LOSS] = loss;
    if (fin != DP_FIN_LSTSQ_L1) out[0] = (float)loss;
}

// Where a kernel finds (c0, c1) of the residual: the coefficients a finishing kernel left, or the caller's (a, b).
struct DpAffine {
    const double *coef;
    double a, b;
    const float *a_dev, *b_dev;
    __device__ __forceinline__ void get(double &c0, double &c1) const {
        if (coef) { c0 = coef[DPC_C0]; c1 = coef[DPC_C1]; return; }
        c1 = -(a_dev ? (double)a_dev[0] : a);
        c0 = -(b_dev ? (double)b_dev[0] : b);
    }
};

// record = (sum m, sum m |t| or sum m t^2)
template <int MASK, bool VEC>
__global__ void __launch_bounds__(DP_THREADS)
    dp_resid_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ mask, uint32_t n, uint32_t ntiles,
                    int kind, DpAffine af, double *__restrict__ part) {
    __shared__ double red[(DP_THREADS / 64) * 2];
    double c0, c1;
    af.get(c0, c1);
    double acc[2] = {0.0, 0.0};
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t p0 = tile * (uint32_t)DP_TILE + threadIdx.x * (uint32_t)DP_PX;
        if (p0 >= n) continue;
        double w[4], xd[4], yd[4];
        dp_pixels<MASK, VEC>(x, y, mask, p0, n, w, xd, yd);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double t = dp_t(xd[k], yd[k], c0, c1, 1.0);
            acc[0] += w[k];
            acc[1] += w[k] * (kind == CGS_DP_L2 ? t * t : fabs(t));
        }
    }
    dp_block_sum<2>(acc, red, part + (size_t)blockIdx.x * DP_REC);
}

__global__ void __launch_bounds__(DP_THREADS)
    dp_finish_resid_kernel(const double *__restrict__ part, int nb, double npix, int mean_over, DpAffine af, double *__restrict__ coef,
                           float *__restrict__ out) {
    __shared__ double red[(DP_THREADS / 64) * 2];
    __shared__ double tot[2];
    dp_sum_records<2>(part, nb, red, tot);
    if (threadIdx.x != 0) return;
    double scale;
    if (af.coef) {                              // after a least-squares fit: the moments' finish left everything but the value
        scale = coef[DPC_SCALE];
    } else {
        double c0, c1;
        af.get(c0, c1);
        const double N = mean_over == CGS_DP_MEAN_IMAGE ? npix : tot[0];
        scale = N > 0.0 ? 1.0 / N : 0.0;
        coef[DPC_C0] = c0; coef[DPC_C1] = c1; coef[DPC_C2] = 1.0; coef[DPC_SCALE] = scale;
        coef[DPC_A] = -c1; coef[DPC_B] = -c0; coef[DPC_M] = tot[0];
    }
    const double loss = tot[0] > 0.0 ? tot[1] * scale : 0.0;
    coef[DPC_LOSS] = loss;
    out[0] = (float)loss;
}

template <int MASK, bool VEC>
__global__ void __launch_bounds__(DP_THREADS)
    dp_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ mask, uint32_t n, int kind,
                  const double *__restrict__ coef, const float *__restrict__ g, float *__restrict__ dx) {
    const uint32_t p0 = blockIdx.x * (uint32_t)DP_TILE + threadIdx.x * (uint32_t)DP_PX;
    if (p0 >= n) return;
    const double c0 = coef[DPC_C0], c1 = coef[DPC_C1], c2 = coef[DPC_C2];
    const double k = (double)g[0] * coef[DPC_SCALE];
    double w[4], xd[4], yd[4];
    dp_pixels<MASK, VEC>(x, y, mask, p0, n, w, xd, yd);
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double t = dp_t(xd[j], yd[j], c0, c1, c2);
        const double v = k * w[j] * (kind == CGS_DP_PEARSON ? t : dp_w(kind, t));
        res[j] = (w[j] != 0.0 && v != 0.0) ? (float)v : 0.0f;          // one rounding; +0 for a pixel selected out
    }
    if (VEC && p0 + 3 < n) {
        *reinterpret_cast<float4 *>(dx + p0) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p0 + j < n) dx[p0 + j] = res[j];
    }
}

// record = (sum m w(r) y, sum m w(r))
template <int MASK, bool VEC>
__global__ void __launch_bounds__(DP_THREADS)
    dp_dab_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ mask, uint32_t n, uint32_t ntiles,
                  int kind, const double *__restrict__ coef, double *__restrict__ part) {
    __shared__ double red[(DP_THREADS / 64) * 2];
    const double c0 = coef[DPC_C0], c1 = coef[DPC_C1], c2 = coef[DPC_C2];
    double acc[2] = {0.0, 0.0};
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t p0 = tile * (uint32_t)DP_TILE + threadIdx.x * (uint32_t)DP_PX;
        if (p0 >= n) continue;
        double w[4], xd[4], yd[4];
        dp_pixels<MASK, VEC>(x, y, mask, p0, n, w, xd, yd);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double mw = w[k] * dp_w(kind, dp_t(xd[k], yd[k], c0, c1, c2));
            acc[0] += mw * yd[k];
            acc[1] += mw;
        }
    }
    dp_block_sum<2>(acc, red, part + (size_t)blockIdx.x * DP_REC);
}

__global__ void __launch_bounds__(DP_THREADS)
    dp_finish_dab_kernel(const double *__restrict__ part, int nb, const double *__restrict__ coef, const float *__restrict__ g,
                         float *__restrict__ dab) {
    __shared__ double red[(DP_THREADS / 64) * 2];
    __shared__ double tot[2];
    dp_sum_records<2>(part, nb, red, tot);
    if (threadIdx.x != 0) return;
    const double k = -(double)g[0] * coef[DPC_SCALE];
    const double da = k * tot[0], db = k * tot[1];
    dab[0] = da != 0.0 ? (float)da : 0.0f;
    dab[1] = db != 0.0 ? (float)db : 0.0f;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct DpShape { uint32_t n, ntiles; int nb; bool vec; };

bool dp_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int dp_blocks(int64_t n) {
    const int64_t t = (n + DP_TILE - 1) / DP_TILE;
    return (int)(t > DP_MAX_BLOCKS ? DP_MAX_BLOCKS : t);
}

// Everything that can be wrong with the planes, decided before anything is enqueued.
int dp_check(const char *who, const float *x, const float *y, const void *mask, int mask_type, int H, int W, DpShape *s) {
    if (H < 1 || W < 1) { cgs_set_error("%s: H and W must be positive (got %d, %d)", who, H, W); return CGS_ERR_ARG; }
    if ((int64_t)H * W > (int64_t)1 << 30) { cgs_set_error("%s: more than 2^30 pixels", who); return CGS_ERR_ARG; }
    if (mask_type != CGS_DP_MASK_NONE && mask_type != CGS_DP_MASK_FLOAT && mask_type != CGS_DP_MASK_BYTE) {
        cgs_set_error("%s: unknown mask type %d", who, mask_type);
        return CGS_ERR_ARG;
    }
    if (!x || !y) { cgs_set_error("%s: NULL x or y", who); return CGS_ERR_ARG; }
    if ((mask_type != CGS_DP_MASK_NONE) != (mask != nullptr)) {
        cgs_set_error("%s: NULL mask with a mask type, or a mask with CGS_DP_MASK_NONE", who);
        return CGS_ERR_ARG;
    }
    const int64_t n = (int64_t)H * W;
    s->n = (uint32_t)n;
    s->ntiles = (uint32_t)((n + DP_TILE - 1) / DP_TILE);
    s->nb = dp_blocks(n);
    s->vec = dp_aligned(x, 16) && dp_aligned(y, 16) &&
             (mask_type == CGS_DP_MASK_NONE || dp_aligned(mask, mask_type == CGS_DP_MASK_FLOAT ? 16 : 4));
    return CGS_OK;
}

int dp_check_scratch(const char *who, const void *scratch, size_t scratch_bytes, int H, int W) {
    const size_t need = cgs_depth_prior_scratch_bytes(H, W);
    if (!scratch || scratch_bytes < need) {
        cgs_set_error("%s: needs %zu bytes of scratch, got %zu", who, need, scratch ? scratch_bytes : (size_t)0);
        return CGS_ERR_WORKSPACE;
    }
    if (!dp_aligned(scratch, 8)) { cgs_set_error("%s: the scratch must be 8-byte aligned", who); return CGS_ERR_ARG; }
    return CGS_OK;
}

int dp_check_coef(const char *who, const void *coef) {
    if (!coef || !dp_aligned(coef, 8)) { cgs_set_error("%s: NULL or misaligned coef (CGS_DEPTH_PRIOR_COEF_BYTES bytes, 8-byte aligned)", who); return CGS_ERR_ARG; }
    return CGS_OK;
}

// KERNEL<mask type, VEC> on `grid` workgroups
#define DP_LAUNCH(KERNEL, mask_type, vec, grid, st, ...)                                                                             \
    do {                                                                                                                              \
        const dim3 g__((unsigned)(grid)), t__(DP_THREADS);                                                                            \
        if (mask_type == CGS_DP_MASK_NONE) {                                                                                          \
            if (vec) hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_NONE, true>), g__, t__, 0, st, __VA_ARGS__);                             \
            else hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_NONE, false>), g__, t__, 0, st, __VA_ARGS__);                                \
        } else if (mask_type == CGS_DP_MASK_FLOAT) {                                                                                  \
            if (vec) hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_FLOAT, true>), g__, t__, 0, st, __VA_ARGS__);                            \
            else hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_FLOAT, false>), g__, t__, 0, st, __VA_ARGS__);                               \
        } else {                                                                                                                      \
            if (vec) hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_BYTE, true>), g__, t__, 0, st, __VA_ARGS__);                             \
            else hipLaunchKernelGGL((KERNEL<CGS_DP_MASK_BYTE, false>), g__, t__, 0, st, __VA_ARGS__);                                \
        }                                                                                                                             \
        CGS_CHECK_LAUNCH(st, false);                                                                                                  \
    } while (0)

int dp_moments(const float *x, const float *y, const void *mask, int mask_type, const DpShape &s, int fin, int mean_over, double *coef,
               float *out, double *part, hipStream_t st) {
    DP_LAUNCH(dp_moment_kernel, mask_type, s.vec, s.nb, st, x, y, mask, s.n, s.ntiles, part);
    hipLaunchKernelGGL(dp_finish_moments_kernel, dim3(1), dim3(DP_THREADS), 0, st, (const double *)part, s.nb, (double)s.n, fin, mean_over,
                       coef, out);
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}

}  // namespace

extern "C" size_t cgs_depth_prior_scratch_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return 0;
    return (size_t)dp_blocks((int64_t)H * W) * DP_REC * sizeof(double);
}

extern "C" int cgs_depth_prior_fwd(const float *x, const float *y, const void *mask, int mask_type, int H, int W, int kind, int align,
                                   int mean_over, double a, double b, const float *a_dev, const float *b_dev, float *out1, void *coef,
                                   void *scratch, size_t scratch_bytes, void *stream) {
    const char *who = "depth_prior_fwd";
    DpShape s;
    if (int rc = dp_check(who, x, y, mask, mask_type, H, W, &s)) return rc;
    if (kind != CGS_DP_L1 && kind != CGS_DP_L2 && kind != CGS_DP_PEARSON) { cgs_set_error("%s: unknown kind %d", who, kind); return CGS_ERR_ARG; }
    if (kind != CGS_DP_PEARSON) {
        if (align != CGS_DP_ALIGN_GIVEN && align != CGS_DP_ALIGN_LSTSQ) { cgs_set_error("%s: unknown align %d", who, align); return CGS_ERR_ARG; }
        if (mean_over != CGS_DP_MEAN_MASK && mean_over != CGS_DP_MEAN_IMAGE) { cgs_set_error("%s: unknown mean_over %d", who, mean_over); return CGS_ERR_ARG; }
    }
    if (!out1) { cgs_set_error("%s: NULL out1", who); return CGS_ERR_ARG; }
    if (int rc = dp_check_coef(who, coef)) return rc;
    if (int rc = dp_check_scratch(who, scratch, scratch_bytes, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)scratch, *cf = (double *)coef;
    if (kind == CGS_DP_PEARSON) return dp_moments(x, y, mask, mask_type, s, DP_FIN_PEARSON, mean_over, cf, out1, part, st);
    DpAffine af = {nullptr, a, b, a_dev, b_dev};
    if (align == CGS_DP_ALIGN_LSTSQ) {
        if (kind == CGS_DP_L2) return dp_moments(x, y, mask, mask_type, s, DP_FIN_LSTSQ_L2, mean_over, cf, out1, part, st);
        if (int rc = dp_moments(x, y, mask, mask_type, s, DP_FIN_LSTSQ_L1, mean_over, cf, out1, part, st)) return rc;
        af.coef = cf;
    }
    DP_LAUNCH(dp_resid_kernel, mask_type, s.vec, s.nb, st, x, y, mask, s.n, s.ntiles, kind, af, part);
    hipLaunchKernelGGL(dp_finish_resid_kernel, dim3(1), dim3(DP_THREADS), 0, st, (const double *)part, s.nb, (double)s.n, mean_over, af, cf, out1);
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}

extern "C" int cgs_depth_prior_scale_shift(const float *x, const float *y, const void *mask, int mask_type, int H, int W, float *ab2,
                                           void *scratch, size_t scratch_bytes, void *stream) {
    const char *who = "depth_prior_scale_shift";
    DpShape s;
    if (int rc = dp_check(who, x, y, mask, mask_type, H, W, &s)) return rc;
    if (!ab2) { cgs_set_error("%s: NULL ab2", who); return CGS_ERR_ARG; }
    if (int rc = dp_check_scratch(who, scratch, scratch_bytes, H, W)) return rc;
    return dp_moments(x, y, mask, mask_type, s, DP_FIN_SCALE_SHIFT, CGS_DP_MEAN_MASK, nullptr, ab2, (double *)scratch, (hipStream_t)stream);
}

extern "C" int cgs_depth_prior_bwd(const float *x, const float *y, const void *mask, int mask_type, int H, int W, int kind,
                                   const void *coef, const float *g, float *dx, void *stream) {
    const char *who = "depth_prior_bwd";
    DpShape s;
    if (int rc = dp_check(who, x, y, mask, mask_type, H, W, &s)) return rc;
    if (kind != CGS_DP_L1 && kind != CGS_DP_L2 && kind != CGS_DP_PEARSON) { cgs_set_error("%s: unknown kind %d", who, kind); return CGS_ERR_ARG; }
    if (int rc = dp_check_coef(who, coef)) return rc;
    if (!g || !dx) { cgs_set_error("%s: NULL g or dx", who); return CGS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = s.vec && dp_aligned(dx, 16);
    DP_LAUNCH(dp_bwd_kernel, mask_type, vec, s.ntiles, st, x, y, mask, s.n, kind, (const double *)coef, g, dx);
    return CGS_OK;
}

extern "C" int cgs_depth_prior_dab(const float *x, const float *y, const void *mask, int mask_type, int H, int W, int kind,
                                   const void *coef, const float *g, float *dab2, void *scratch, size_t scratch_bytes, void *stream) {
    const char *who = "depth_prior_dab";
    DpShape s;
    if (int rc = dp_check(who, x, y, mask, mask_type, H, W, &s)) return rc;
    if (kind != CGS_DP_L1 && kind != CGS_DP_L2) { cgs_set_error("%s: unknown kind %d (an affine map belongs to L1 or L2)", who, kind); return CGS_ERR_ARG; }
    if (int rc = dp_check_coef(who, coef)) return rc;
    if (!g || !dab2) { cgs_set_error("%s: NULL g or dab2", who); return CGS_ERR_ARG; }
    if (int rc = dp_check_scratch(who, scratch, scratch_bytes, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)scratch;
    DP_LAUNCH(dp_dab_kernel, mask_type, s.vec, s.nb, st, x, y, mask, s.n, s.ntiles, kind, (const double *)coef, part);
    hipLaunchKernelGGL(dp_finish_dab_kernel, dim3(1), dim3(DP_THREADS), 0, st, (const double *)part, s.nb, (const double *)coef, g, dab2);
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}
