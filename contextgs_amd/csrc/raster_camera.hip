// Camera gradients of the rasterizer: dL/dviewmatrix [4,4], dL/dprojmatrix [4,4], dL/dcampos [3] (include/cgs.h,
// cgs_raster_camera_backward).  One per-Gaussian kernel behind a backward that has just run: it reads what the blend
// backwards left in the backward's scratch (dL/d(pixel mean), dL/d(conic), with maps dL/dz), recomputes the forward
// intermediates from the inputs the way preprocess_bwd_kernel does (the bodies of raster_math.h; the covariance chain of
// cgs_pre_bwd_one / cgs_pre_bwd_cov restated up to dA and dt, the two must be edited together) and sums the partials of the
// three tensors over all Gaussians.  The rasterizer reads the three tensors independently (row-vector convention, V[4c+i]):
//   viewmatrix V: t = [p,1] V (Jacobian, 1.3 tanfov clamp, depth z = t_z) and W = V[:3,:3] in cov2D = J W Sigma W^T J^T
//   projmatrix PM: the pixel mean, (hx, hy, hw) = [p,1] PM[:, (0,1,3)], ndc = h / (hw + 1e-7)
//   campos: the SH direction means3D - campos
// and each gets the gradient of exactly these uses.  V[:,3] and PM[:,2] are never read: exactly 0.
//
// Reduction, no float atomics (bit-reproducible at fixed inputs): every thread adds its Gaussians (a grid-stride loop, a few
// dozen terms per thread) into CAM_N = 27 registers (12 + 12 live matrix entries + 3), the wave adds up by shuffles, the
// workgroup's four waves through LDS, one CAM_N-float row per workgroup goes to the partials buffer, and the last workgroup
// to arrive (cgs_ticket_last) adds the rows in workgroup order.
#include "cgs_internal.h"
#include "raster_math.h"
#include "raster_pre.h"
#include "raster_forms.h"

#define CAM_THREADS 256
#define CAM_WAVES (CAM_THREADS / CGS_WAVE)
#define CAM_MAX_BLOCKS 1024
#define CAM_N 27            // V[4c+i], i < 3: slots 3c+i (c = 0..3); PM[4c+k], k in {0,1,3}: slots 12 + 3c + {0,1,2}; campos: 24..26
#define CAM_GROUPS (CAM_THREADS / CAM_N)        // the last workgroup's row groups: group g adds rows g, g + CAM_GROUPS, ...

// a float published by a device-scope exchange / read by a device-scope load: cgs_publish / cgs_published (cgs_internal.h) in fp32
__device__ __forceinline__ void cam_publish(float *slot, float v) {
    const unsigned old = atomicExch((unsigned *)slot, __float_as_uint(v));
    asm volatile("" ::"v"(old) : "memory");
}
__device__ __forceinline__ float cam_published(const float *slot) {
    return __uint_as_float(__hip_atomic_load((const unsigned *)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// One Gaussian with radius > 0: adds its partials to acc[0..24).  c3 = its 3-D covariance (scale_modifier applied), g_z =
// dL/dz of the maps (0 without), AA: d0 = the undilated determinant as the forward formed it (cgs_det2_rs / cgs_det2_comp),
// aa_op = its opacity, aa_g = dL/d(opacity * h).
template <bool AA>
__device__ __forceinline__ void cam_bwd_one(const float3 p, const CgsCov3 &c3, float gmean_x, float gmean_y, float gconic_a,
                                            float gconic_b, float gconic_c, float g_z, const float *V, const float *Pm, int W, int H,
                                            float tanfovx, float tanfovy, float d0, float aa_op, float aa_g, float (&acc)[CAM_N]) {
    const float3 t = cgs_to_view(p, V);
    const CgsJac j = cgs_jacobian(t, V, W, H, tanfovx, tanfovy);
    float x, y, z;   // cov2D = [[x,y],[y,z]]
    cgs_cov2d(j.A, c3, x, y, z);
    float aa_gx = 0.f, aa_gy = 0.f, aa_gz = 0.f;
    if constexpr (AA) {
        float d1;
        const float hh = cgs_aa_h(d0, x, z, d1);
        cgs_aa_bwd(d0, d1, hh, x, y, z, aa_g, aa_op, aa_gx, aa_gy, aa_gz);
    }
    x += 0.3f;
    z += 0.3f;
    const float det = x * z - y * y;
    // ---- conic -> cov2D ----------------------------------------------------
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (det != 0.f) {
        const float d2 = 1.f / (det * det);
        gx = d2 * (-z * z * gconic_a + y * z * gconic_b - y * y * gconic_c);
        gy = d2 * (2.f * y * z * gconic_a - (x * z + y * y) * gconic_b + 2.f * x * y * gconic_c);
        gz = d2 * (-y * y * gconic_a + x * y * gconic_b - x * x * gconic_c);
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
    // ---- dL/dA = 2 G2 A Sigma ------------------------------------------------
    const float S[9] = {c3.xx, c3.xy, c3.xz, c3.xy, c3.yy, c3.yz, c3.xz, c3.yz, c3.zz};
    float dA[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dA[c] = 2.f * (GA0[0] * S[c] + GA0[1] * S[3 + c] + GA0[2] * S[6 + c]);
        dA[3 + c] = 2.f * (GA1[0] * S[c] + GA1[1] * S[3 + c] + GA1[2] * S[6 + c]);
    }
    // A = J Wv, Wv[i][c] = V[4c+i]:  dL/dJ[r][i] = sum_c dA[r][c] Wv[i][c], and on to t as cgs_pre_bwd_one does
    const float dJ00 = dA[0] * V[0] + dA[1] * V[4] + dA[2] * V[8];
    const float dJ02 = dA[0] * V[2] + dA[1] * V[6] + dA[2] * V[10];
    const float dJ11 = dA[3] * V[1] + dA[4] * V[5] + dA[5] * V[9];
    const float dJ12 = dA[3] * V[2] + dA[4] * V[6] + dA[5] * V[10];
    const float tz = 1.f / j.tz, tz2 = tz * tz, tz3 = tz2 * tz;
    const float dt[3] = {j.clamp_x ? 0.f : (-j.fx * tz2 * dJ02), j.clamp_y ? 0.f : (-j.fy * tz2 * dJ12),
                         -j.fx * tz2 * dJ00 - j.fy * tz2 * dJ11 + (2.f * j.fx * j.tx) * tz3 * dJ02 +
                             (2.f * j.fy * j.ty) * tz3 * dJ12 + g_z};
    // dL/dWv[i][c] = sum_r J[r][i] dA[r][c] with J = [[j00, 0, j02], [0, j11, j12]] as cgs_jacobian forms it
    const float j00 = j.fx / j.tz, j02 = -(j.fx * j.tx) / (j.tz * j.tz);
    const float j11 = j.fy / j.tz, j12 = -(j.fy * j.ty) / (j.tz * j.tz);
    const float pv[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // t = p Wv^T + V[3,:3]: dL/dV[c][i] += p_c dt_i
        acc[3 * c + 0] += j00 * dA[c] + pv[c] * dt[0];
        acc[3 * c + 1] += j11 * dA[3 + c] + pv[c] * dt[1];
        acc[3 * c + 2] += j02 * dA[c] + j12 * dA[3 + c] + pv[c] * dt[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[9 + i] += dt[i];

    // ---- projection path: pixel = ((ndc+1) W - 1)/2, ndc = h / (hw + 1e-7) ------
    const float gnx = gmean_x * 0.5f * (float)W;   // = dL/d ndc_x
    const float gny = gmean_y * 0.5f * (float)H;
    const float hx = Pm[0] * p.x + Pm[4] * p.y + Pm[8] * p.z + Pm[12];
    const float hy = Pm[1] * p.x + Pm[5] * p.y + Pm[9] * p.z + Pm[13];
    const float hwv = Pm[3] * p.x + Pm[7] * p.y + Pm[11] * p.z + Pm[15];
    const float mw = 1.f / (hwv + 0.0000001f);
    const float mx = hx * mw * mw, my = hy * mw * mw;
    const float dh[3] = {gnx * mw, gny * mw, -(mx * gnx + my * gny)};      // dL/d(hx, hy, hw)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[12 + 3 * c + k] += pv[c] * dh[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[21 + k] += dh[k];
}

// COV6: cov3D_precomp (else scales + rotations); AA: antialiasing; SHD: the SH degree whose direction term goes to dL/dcampos
// (-1: none; degree 0 has none).  d_opacities (AA): dL/d(opacity) as the preprocess backward left it = dL/d(opacity h) h, the
// factor is taken back out with the recomputed h (h >= 0.005 by its clamp).
template <bool COV6, bool AA, int SHD>
__global__ void __launch_bounds__(CAM_THREADS)
    raster_camera_bwd_kernel(int64_t P, int W, int H, float tanfovx, float tanfovy, float scale_modifier,
                             const float *__restrict__ viewmatrix, const float *__restrict__ projmatrix,
                             const float *__restrict__ campos, const float *__restrict__ means3D, const float *__restrict__ shs,
                             int sh_m, int sh_vec, const float *__restrict__ opacities, const float *__restrict__ scales,
                             const float *__restrict__ rotations, const float *__restrict__ cov6,
                             const int32_t *__restrict__ radii, const float *__restrict__ dL_dmean2D_px,
                             const float *__restrict__ dL_dconic, const float *__restrict__ dL_dz,
                             const float *__restrict__ dL_dcolors, const float *__restrict__ d_opacities,
                             float *__restrict__ partial, unsigned int *__restrict__ ticket, float *__restrict__ out_view,
                             float *__restrict__ out_proj, float *__restrict__ out_campos) {
    __shared__ float sh_acc[CAM_GROUPS > CAM_WAVES ? CAM_GROUPS : CAM_WAVES][CAM_N];
    __shared__ bool last;
    float V[16], Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { V[k] = viewmatrix[k]; Pm[k] = projmatrix[k]; }
    float acc[CAM_N];
#pragma unroll
    for (int k = 0; k < CAM_N; ++k) acc[k] = 0.f;

    const int64_t stride = (int64_t)gridDim.x * CAM_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x; i < P; i += stride) {
        if (radii[i] <= 0) continue;         // culled in forward: contributes nothing
        const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
        if constexpr (SHD > 0) {             // SH first: its row is dead before the geometry chain needs its registers
            constexpr int N = 3 * (SHD + 1) * (SHD + 1);
            constexpr int K = (SHD + 1) * (SHD + 1);
            float sh[N];
            cgs_load_row<N>(shs + i * 3 * (int64_t)sh_m, sh_vec != 0, sh);
            float3 d;
            const float3 u = cgs_sh_dir(p, make_float3(campos[0], campos[1], campos[2]), d);
            const float3 c = cgs_sh_rgb<SHD>(sh, u.x, u.y, u.z);         // the forward's colour: its clamp bits
            const float g[3] = {c.x < 0.f ? 0.f : dL_dcolors[3 * i], c.y < 0.f ? 0.f : dL_dcolors[3 * i + 1],
                                c.z < 0.f ? 0.f : dL_dcolors[3 * i + 2]};
            float w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = sh[3 * k] * g[0] + sh[3 * k + 1] * g[1] + sh[3 * k + 2] * g[2];
            const float3 gd = cgs_dnormvdv(d, cgs_sh_ddir<SHD>(w, u.x, u.y, u.z));      // dL/d(means3D - campos)
            acc[24] -= gd.x;
            acc[25] -= gd.y;
            acc[26] -= gd.z;
        }
        CgsCov3 c3;
        float3 s = make_float3(0.f, 0.f, 0.f);
        float R[9];
        if constexpr (COV6) {
            c3 = {cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5]};
        } else {
            s = make_float3(scales[3 * i] * scale_modifier, scales[3 * i + 1] * scale_modifier, scales[3 * i + 2] * scale_modifier);
            const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
            cgs_quat_to_rot(q, R);
            c3 = cgs_cov3d(s, R);
        }
        float d0 = 0.f, aa_op = 0.f, aa_g = 0.f;
        if constexpr (AA) {      // d0 as the forward formed it for this covariance form, and dL/d(opacity h) back from dL/d(opacity)
            const CgsJac j = cgs_jacobian(cgs_to_view(p, V), V, W, H, tanfovx, tanfovy);
            float a, b, c, d1;
            cgs_cov2d(j.A, c3, a, b, c);
            if constexpr (COV6) d0 = cgs_det2_comp(a, b, c);
            else d0 = cgs_det2_rs(j.A, R, s);
            aa_op = opacities[i];
            aa_g = d_opacities[i] / cgs_aa_h(d0, a, c, d1);
        }
        cam_bwd_one<AA>(p, c3, dL_dmean2D_px[2 * i], dL_dmean2D_px[2 * i + 1], dL_dconic[3 * i], dL_dconic[3 * i + 1],
                        dL_dconic[3 * i + 2], dL_dz ? dL_dz[i] : 0.f, V, Pm, W, H, tanfovx, tanfovy, d0, aa_op, aa_g, acc);
    }

    // ---- wave -> workgroup -> one row per workgroup ---------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < CAM_N; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        acc[k] = v;
    }
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < CAM_N; ++k) sh_acc[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < CAM_N) {
        float v = sh_acc[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CAM_WAVES; ++w) v += sh_acc[w][threadIdx.x];
        cam_publish(&partial[(int64_t)blockIdx.x * CAM_N + threadIdx.x], v);
    }
    __syncthreads();         // every exchange of the row has returned before the ticket is taken
    if (threadIdx.x == 0) last = cgs_ticket_last(ticket);
    __syncthreads();
    if (!last) return;

    // ---- the last workgroup: rows in workgroup order, CAM_GROUPS interleaved chains per column ----------------------
    const int grp = threadIdx.x / CAM_N, col = threadIdx.x % CAM_N;
    if (grp < CAM_GROUPS) {
        float v = 0.f;
        const int nb = (int)gridDim.x;
        int r = grp;
        for (; r + 7 * CAM_GROUPS < nb; r += 8 * CAM_GROUPS) {
            float u[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] = cam_published(&partial[(int64_t)(r + k * CAM_GROUPS) * CAM_N + col]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v += u[k];
        }
        for (; r < nb; r += CAM_GROUPS) v += cam_published(&partial[(int64_t)r * CAM_N + col]);
        sh_acc[grp][col] = v;
    }
    __syncthreads();
    if (threadIdx.x < CAM_N) {
        float v = sh_acc[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < CAM_GROUPS; ++g) v += sh_acc[g][threadIdx.x];
        const int k = threadIdx.x;
        if (k < 12) {
            if (out_view) out_view[4 * (k / 3) + k % 3] = v;
        } else if (k < 24) {
            const int c = (k - 12) / 3, m = (k - 12) % 3;
            if (out_proj) out_proj[4 * c + (m == 2 ? 3 : m)] = v;
        } else if (out_campos) {
            out_campos[k - 24] = v;
        }
    }
    if (threadIdx.x < 4) {      // the entries the rasterizer never reads
        if (out_view) out_view[4 * threadIdx.x + 3] = 0.f;
        if (out_proj) out_proj[4 * threadIdx.x + 2] = 0.f;
    }
}

size_t cgs_camera_work_bytes(int64_t P) {
    (void)P;
    return cgs_align_up((size_t)CAM_MAX_BLOCKS * CAM_N * sizeof(float), 256) + CGS_TICKET_BYTES;
}

template <bool COV6, bool AA, int SHD>
static void launch_camera(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D, const float *opacities,
                          const float *scales, const float *rotations, const int32_t *radii, const float *d_mean_px,
                          const float *d_conic, const float *d_z, const float *dL_dcolors, const float *d_opacities, float *partial,
                          unsigned int *ticket, float *out_view, float *out_proj, float *out_campos, hipStream_t stream) {
    const int64_t want = (P + CAM_THREADS - 1) / CAM_THREADS;
    const unsigned blocks = (unsigned)(want < CAM_MAX_BLOCKS ? want : CAM_MAX_BLOCKS);
    hipLaunchKernelGGL((raster_camera_bwd_kernel<COV6, AA, SHD>), dim3(blocks), dim3(CAM_THREADS), 0, stream, P, cfg->image_width,
                       cfg->image_height, cfg->tanfovx, cfg->tanfovy, cfg->scale_modifier, cfg->viewmatrix, cfg->projmatrix,
                       cfg->campos, means3D, f.shs, f.sh_coeffs, f.sh_vec, opacities, scales, rotations, f.cov3D, radii, d_mean_px,
                       d_conic, d_z, dL_dcolors, d_opacities, partial, ticket, out_view, out_proj, out_campos);
}

// f.shs != NULL: the SH direction term (out_campos given); f.cov3D != NULL: covariances as given.  d_z: dL/dz of the maps or
// NULL.  aa: antialiasing, opacities / d_opacities [P] given.  work: cgs_camera_work_bytes(P) bytes, any contents.  P > 0.
int cgs_launch_camera_bwd(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D, const float *opacities,
                          const float *scales, const float *rotations, const int32_t *radii, const float *d_mean_px,
                          const float *d_conic, const float *d_z, const float *dL_dcolors, const float *d_opacities, bool aa,
                          float *out_view, float *out_proj, float *out_campos, void *work, hipStream_t stream) {
    float *partial = (float *)work;
    unsigned int *ticket = (unsigned int *)((char *)work + cgs_align_up((size_t)CAM_MAX_BLOCKS * CAM_N * sizeof(float), 256));
    CGS_CHECK_HIP(hipMemsetAsync(ticket, 0, CGS_TICKET_BYTES, stream));
    const int d = (f.shs && f.sh_degree > 0) ? f.sh_degree : -1;
#define CGS_CAM_ARGS cfg, P, f, means3D, opacities, scales, rotations, radii, d_mean_px, d_conic, d_z, dL_dcolors, d_opacities, partial, \
                     ticket, out_view, out_proj, out_campos, stream
#define CGS_CAM_DEGREE(COV6, AA)                                      \
    switch (d) {                                                      \
        case -1: launch_camera<COV6, AA, -1>(CGS_CAM_ARGS); break;    \
        case 1: launch_camera<COV6, AA, 1>(CGS_CAM_ARGS); break;      \
        case 2: launch_camera<COV6, AA, 2>(CGS_CAM_ARGS); break;      \
        default: launch_camera<COV6, AA, 3>(CGS_CAM_ARGS); break;     \
    }
    if (f.cov3D) {
        if (aa) { CGS_CAM_DEGREE(true, true) } else { CGS_CAM_DEGREE(true, false) }
    } else {
        if (aa) { CGS_CAM_DEGREE(false, true) } else { CGS_CAM_DEGREE(false, false) }
    }
#undef CGS_CAM_DEGREE
#undef CGS_CAM_ARGS
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
