// Preprocess backward (R8, per-Gaussian half): chain dL/d(pixel mean) and
// dL/d(conic) from the blend backward to means3D / scales / rotations, and
// emit the means2D gradient in the NDC-scaled convention the reference's
// densification statistics consume (scene/gaussian_model.py:710,
// arguments/__init__.py:153).  Forward intermediates are recomputed from the
// 40-byte inputs instead of being stored (saves ~100 B/Gaussian of HBM
// traffic each way).
#include "cgs_internal.h"
#include "raster_math.h"
#include "raster_pre.h"

#define PB_THREADS 256

// ABS (cgs_raster_backward_abs): dL_dmeans2D rows are four floats, (gnx, gny, 0.5 W abs_x, 0.5 H abs_y) with abs_x, abs_y
// the blend backward's sums of |dL_p/d(pixel mean)| in dL_dabs_px [P, 2]; the default instance never reads dL_dabs_px.
// AA (antialiasing): also reads opacities[i] and dL_dopacities[i] (dL/d(op_eff), the blend backwards' sum), writes
// dL/d(opacity) = dL/d(op_eff) h over it and adds h's dL/d(cov2D) to the conic chain (raster_pre.h); the other instances
// never touch the two pointers.
template <bool ABS, bool AA>
__global__ void __launch_bounds__(PB_THREADS)
    preprocess_bwd_kernel(int64_t P, int W, int H, float tanfovx, float tanfovy, float scale_modifier,
                          const float *__restrict__ viewmatrix, const float *__restrict__ projmatrix,
                          const float *__restrict__ means3D, const float *__restrict__ scales,
                          const float *__restrict__ rotations, const int32_t *__restrict__ radii,
                          const float *__restrict__ dL_dmean2D_px, const float *__restrict__ dL_dconic,
                          float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D,
                          float *__restrict__ dL_dscales, float *__restrict__ dL_drotations,
                          const float *__restrict__ dL_dabs_px, const float *__restrict__ opacities,
                          float *__restrict__ dL_dopacities) {
    const int64_t i = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x;
    if (i >= P) return;
    if (radii[i] <= 0) {         // culled in forward: all gradients are zero (the arrays arrive uninitialised; no blend list
                                 // holds it, dL_dopacities[i] stays 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = 0.f; if constexpr (!ABS) dL_dmeans2D[3 * i + k] = 0.f; dL_dscales[3 * i + k] = 0.f; }
        if constexpr (ABS) cgs_store_dm2_abs(dL_dmeans2D, i, nullptr, dL_dabs_px, W, H);
#pragma unroll
        for (int k = 0; k < 4; ++k) dL_drotations[4 * i + k] = 0.f;
        return;
    }

    float V[16], Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { V[k] = viewmatrix[k]; Pm[k] = projmatrix[k]; }
    const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    const float3 s_raw = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
    const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2],
                                 rotations[4 * i + 3]);

    const CgsPreBwd o = cgs_pre_bwd_one<AA>(p, s_raw, q, dL_dmean2D_px[2 * i], dL_dmean2D_px[2 * i + 1], dL_dconic[3 * i],
                                            dL_dconic[3 * i + 1], dL_dconic[3 * i + 2], V, Pm, W, H, tanfovx, tanfovy,
                                            scale_modifier, AA ? opacities[i] : 0.f, AA ? dL_dopacities[i] : 0.f);
#pragma unroll
    for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = o.dp[k]; if constexpr (!ABS) dL_dmeans2D[3 * i + k] = o.dm2[k]; dL_dscales[3 * i + k] = o.ds[k]; }
    if constexpr (ABS) cgs_store_dm2_abs(dL_dmeans2D, i, o.dm2, dL_dabs_px, W, H);
#pragma unroll
    for (int k = 0; k < 4; ++k) dL_drotations[4 * i + k] = o.dq[k];
    if constexpr (AA) dL_dopacities[i] = o.dop;
}

int cgs_launch_preprocess_bwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                              const float *rotations, const int32_t *radii, const float *dL_dmean2D_px,
                              const float *dL_dconic, float *dL_dmeans3D, float *dL_dmeans2D,
                              float *dL_dscales, float *dL_drotations, hipStream_t stream, const float *aa_opacities,
                              float *aa_dL_dopacities, const float *dL_dabs_px) {
    if (P == 0) return CGS_OK;
    CgsProfScope prof(CGS_PROF_PREPROCESS_BWD, stream);
    const dim3 grid((unsigned)((P + PB_THREADS - 1) / PB_THREADS)), block(PB_THREADS);
    const bool aa = aa_opacities != nullptr, absg = dL_dabs_px != nullptr;
    hipLaunchKernelGGL((aa ? (absg ? preprocess_bwd_kernel<true, true> : preprocess_bwd_kernel<false, true>)
                           : (absg ? preprocess_bwd_kernel<true, false> : preprocess_bwd_kernel<false, false>)),
                       grid, block, 0, stream, P, cfg->image_width, cfg->image_height, cfg->tanfovx, cfg->tanfovy, cfg->scale_modifier,
                       cfg->viewmatrix, cfg->projmatrix, means3D, scales, rotations, radii, dL_dmean2D_px, dL_dconic, dL_dmeans3D,
                       dL_dmeans2D, dL_dscales, dL_drotations, dL_dabs_px, aa_opacities, aa_dL_dopacities);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
