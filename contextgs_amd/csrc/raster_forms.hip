// The rasterizer's preprocess forward / backward for the argument forms the colours_precomp + scales/rotations kernels
// (csrc/raster_geom.hip, csrc/raster_bwd.hip) do not take: colours from spherical harmonics (shs) and covariances given
// directly (cov3D_precomp), alone or together, and visible_filter with cov3D_precomp.  One lane per Gaussian, the same
// record layout as preprocess_kernel (the colour goes to the slots colors_precomp fills), so the binning and both blend
// kernels are the existing ones and no form adds a launch.
//
// SH rows are [M, 3] fp32 per Gaussian (M <= 16); only the (D+1)^2 active coefficients are read, as dwordx4 when the rows
// are 16-byte aligned (M % 4 == 0).  The backward recomputes the colour and its clamp bits with the forward's device
// function (-ffp-contract=off: the same bits) instead of storing a mask, and writes the whole dL/dshs row, zeros above
// (D+1)^2 and for culled Gaussians included.  It takes dL/d(pixel mean) / dL/d(conic) as the blend backward finishes them
// (not its raw sums).
//
// Two kernel templates, forward and backward.  The form (SHD, COV6) and the options (AA: antialiasing, ABS: absolute
// screen-space gradients) are template flags of the kernels themselves; launch_fwd / launch_bwd pick the instance, and the
// switches at the bottom instantiate only the forms that reach this file.
#include "cgs_internal.h"
#include "raster_forms.h"

#define PF_THREADS 256

// SHD: -1 = colours precomputed, 0..3 = SH of that degree.  COV6: covariance from cov6 instead of scales / rotations.
// AA: antialiasing (raster_math.h, cgs_aa_h), the record's opacity is opacity * h.  Never with FILTER_ONLY.
template <bool FILTER_ONLY, int SHD, bool COV6, bool AA>
__global__ void __launch_bounds__(PF_THREADS)
    preprocess_form_kernel(int64_t P, int W, int H, float tanfovx, float tanfovy, float scale_modifier,
                           const float *__restrict__ viewmatrix, const float *__restrict__ projmatrix,
                           const float *__restrict__ campos, const float *__restrict__ means3D,
                           const float *__restrict__ colors, const float *__restrict__ shs, int sh_m, int sh_vec,
                           const float *__restrict__ opacities, const float *__restrict__ scales,
                           const float *__restrict__ rotations, const float *__restrict__ cov6, float4 *__restrict__ rec,
                           uint32_t *__restrict__ depth_key, uint32_t *__restrict__ tiles, uint2 *__restrict__ rect,
                           int32_t *__restrict__ radii) {
    const int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= P) return;

    float V[16], Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { V[k] = viewmatrix[k]; Pm[k] = projmatrix[k]; }
    const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);

    CgsProj pr;
    bool ok;
    if (COV6) {
        const CgsCov3 c3 = {cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5]};
        ok = cgs_project_cov<AA>(p, c3, V, Pm, W, H, tanfovx, tanfovy, pr);
    } else {
        const float3 s = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
        const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
        ok = cgs_project<float, AA>(p, s, q, V, Pm, W, H, tanfovx, tanfovy, scale_modifier, pr);
    }
    auto color = [&]() -> float3 {
        if constexpr (SHD < 0) {
            return make_float3(colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]);
        } else {
            constexpr int N = 3 * (SHD + 1) * (SHD + 1);
            float sh[N];
            cgs_load_row<N>(shs + i * 3 * (int64_t)sh_m, sh_vec != 0, sh);
            float3 d;
            const float3 u = cgs_sh_dir(p, make_float3(campos[0], campos[1], campos[2]), d);
            const float3 c = cgs_sh_rgb<SHD>(sh, u.x, u.y, u.z);
            return make_float3(fmaxf(c.x, 0.f), fmaxf(c.y, 0.f), fmaxf(c.z, 0.f));
        }
    };
    cgs_pre_fwd_form<FILTER_ONLY, decltype(color), AA>(i, ok, pr, FILTER_ONLY ? 0.f : opacities[i], color, W, H, rec, depth_key, tiles,
                                                       rect, radii);
}

// Per-Gaussian backward of the forms above (the blend backward's dL/d(pixel mean), dL/d(conic) and, for SH, dL/dcolor in,
// as preprocess_bwd_kernel takes them).  Every output row is written, zeros for culled Gaussians.
// AA (antialiasing): also reads opacities[i] and dL_dopacities[i] (dL/d(op_eff), the blend backwards' sum), writes
// dL/d(opacity) = dL/d(op_eff) h over it and adds h's dL/d(cov2D) to the conic chain (raster_pre.h / raster_forms.h); the other
// instances never touch the two pointers.  Culled Gaussians: no blend list holds them, dL_dopacities[i] stays 0.
template <int SHD, bool COV6, bool ABS, bool AA>
__global__ void __launch_bounds__(PF_THREADS)
    preprocess_bwd_form_kernel(int64_t P, int W, int H, float tanfovx, float tanfovy, float scale_modifier,
                               const float *__restrict__ viewmatrix, const float *__restrict__ projmatrix,
                               const float *__restrict__ campos, const float *__restrict__ means3D,
                               const float *__restrict__ shs, int sh_m, int sh_vec, const float *__restrict__ scales,
                               const float *__restrict__ rotations, const float *__restrict__ cov6,
                               const int32_t *__restrict__ radii, const float *__restrict__ dL_dmean2D_px,
                               const float *__restrict__ dL_dconic, const float *__restrict__ dL_dcolors,
                               float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D, float *__restrict__ dL_dshs,
                               float *__restrict__ dL_dscales, float *__restrict__ dL_drotations, float *__restrict__ dL_dcov6,
                               const float *__restrict__ dL_dabs_px, const float *__restrict__ opacities,
                               float *__restrict__ dL_dopacities) {
    const int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= P) return;
    if (radii[i] <= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = 0.f; if constexpr (!ABS) dL_dmeans2D[3 * i + k] = 0.f; }
        if constexpr (ABS) cgs_store_dm2_abs(dL_dmeans2D, i, nullptr, dL_dabs_px, W, H);
        if (COV6) {
#pragma unroll
            for (int k = 0; k < 6; ++k) dL_dcov6[6 * i + k] = 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) dL_dscales[3 * i + k] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) dL_drotations[4 * i + k] = 0.f;
        }
        if (SHD >= 0) cgs_zero_row(dL_dshs + i * 3 * (int64_t)sh_m, sh_vec != 0, sh_m);
        return;
    }

    float V[16], Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { V[k] = viewmatrix[k]; Pm[k] = projmatrix[k]; }
    const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);

    // SH first: its row (up to 48 floats) is dead before the geometry chain needs its registers
    float3 gsh = make_float3(0.f, 0.f, 0.f);      // dL/dmeans3D through the view direction
    if constexpr (SHD >= 0) {
        constexpr int N = 3 * (SHD + 1) * (SHD + 1);
        constexpr int K = (SHD + 1) * (SHD + 1);
        float sh[N];
        cgs_load_row<N>(shs + i * 3 * (int64_t)sh_m, sh_vec != 0, sh);
        float3 d;
        const float3 u = cgs_sh_dir(p, make_float3(campos[0], campos[1], campos[2]), d);
        const float3 c = cgs_sh_rgb<SHD>(sh, u.x, u.y, u.z);         // the forward's colour: its clamp bits
        const float g[3] = {c.x < 0.f ? 0.f : dL_dcolors[3 * i], c.y < 0.f ? 0.f : dL_dcolors[3 * i + 1],
                            c.z < 0.f ? 0.f : dL_dcolors[3 * i + 2]};
        float w[K], b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = sh[3 * k] * g[0] + sh[3 * k + 1] * g[1] + sh[3 * k + 2] * g[2];
        const float3 gdir = cgs_sh_ddir<SHD>(w, u.x, u.y, u.z);
        cgs_sh_basis<SHD>(u.x, u.y, u.z, b);
        cgs_store_row<N>(dL_dshs + i * 3 * (int64_t)sh_m, sh_vec != 0, sh_m, [&](int j) { return b[j / 3] * g[j % 3]; });
        if (SHD > 0) gsh = cgs_dnormvdv(d, gdir);
    }
    CgsPreBwd o;
    if (COV6) {
        const CgsCov3 c3 = {cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5]};
        float M[9];
        cgs_pre_bwd_cov<AA>(p, c3, dL_dmean2D_px[2 * i], dL_dmean2D_px[2 * i + 1], dL_dconic[3 * i], dL_dconic[3 * i + 1],
                            dL_dconic[3 * i + 2], V, Pm, W, H, tanfovx, tanfovy, o, M, AA ? opacities[i] : 0.f,
                            AA ? dL_dopacities[i] : 0.f);
        // an off-diagonal number of the six stands for both symmetric entries
        dL_dcov6[6 * i + 0] = M[0];
        dL_dcov6[6 * i + 1] = M[1] + M[3];
        dL_dcov6[6 * i + 2] = M[2] + M[6];
        dL_dcov6[6 * i + 3] = M[4];
        dL_dcov6[6 * i + 4] = M[5] + M[7];
        dL_dcov6[6 * i + 5] = M[8];
    } else {
        const float3 s_raw = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
        const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
        o = cgs_pre_bwd_one<AA>(p, s_raw, q, dL_dmean2D_px[2 * i], dL_dmean2D_px[2 * i + 1], dL_dconic[3 * i],
                                dL_dconic[3 * i + 1], dL_dconic[3 * i + 2], V, Pm, W, H, tanfovx, tanfovy, scale_modifier,
                                AA ? opacities[i] : 0.f, AA ? dL_dopacities[i] : 0.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) dL_dscales[3 * i + k] = o.ds[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) dL_drotations[4 * i + k] = o.dq[k];
    }

    if (SHD > 0) {
        o.dp[0] += gsh.x;
        o.dp[1] += gsh.y;
        o.dp[2] += gsh.z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = o.dp[k]; if constexpr (!ABS) dL_dmeans2D[3 * i + k] = o.dm2[k]; }
    if constexpr (ABS) cgs_store_dm2_abs(dL_dmeans2D, i, o.dm2, dL_dabs_px, W, H);
    if constexpr (AA) dL_dopacities[i] = o.dop;
}

template <bool FILTER_ONLY, int SHD, bool COV6>
static void launch_fwd(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D, const float *colors,
                       const float *opacities, const float *scales, const float *rotations, CgsGeom &g, int32_t *radii,
                       hipStream_t stream, bool aa) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((P + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, stream, P,
                           cfg->image_width, cfg->image_height, cfg->tanfovx, cfg->tanfovy, cfg->scale_modifier, cfg->viewmatrix,
                           cfg->projmatrix, cfg->campos, means3D, colors, f.shs, f.sh_coeffs, f.sh_vec, opacities, scales, rotations,
                           f.cov3D, g.rec, g.depth_key, g.tiles, g.rect, radii);
    };
    if constexpr (!FILTER_ONLY) {
        if (aa) return go(preprocess_form_kernel<false, SHD, COV6, true>);
    }
    go(preprocess_form_kernel<FILTER_ONLY, SHD, COV6, false>);
}

// dL_dabs_px != NULL: dL_dmeans2D is [P, 4] (cgs_store_dm2_abs); aa_opacities != NULL: antialiasing
template <int SHD, bool COV6>
static void launch_bwd(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D, const float *scales,
                       const float *rotations, const int32_t *radii, const float *dL_dmean2D_px, const float *dL_dconic,
                       const float *dL_dcolors, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dshs, float *dL_dscales,
                       float *dL_drotations, float *dL_dcov3D, hipStream_t stream, const float *aa_opacities,
                       float *aa_dL_dopacities, const float *dL_dabs_px) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((P + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, stream, P,
                           cfg->image_width, cfg->image_height, cfg->tanfovx, cfg->tanfovy, cfg->scale_modifier, cfg->viewmatrix,
                           cfg->projmatrix, cfg->campos, means3D, f.shs, f.sh_coeffs, f.sh_vec, scales, rotations, f.cov3D, radii,
                           dL_dmean2D_px, dL_dconic, dL_dcolors, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dscales, dL_drotations,
                           dL_dcov3D, dL_dabs_px, aa_opacities, aa_dL_dopacities);
    };
    if (aa_opacities && dL_dabs_px) go(preprocess_bwd_form_kernel<SHD, COV6, true, true>);
    else if (aa_opacities) go(preprocess_bwd_form_kernel<SHD, COV6, false, true>);
    else if (dL_dabs_px) go(preprocess_bwd_form_kernel<SHD, COV6, true, false>);
    else go(preprocess_bwd_form_kernel<SHD, COV6, false, false>);
}

// f.shs == NULL: colours precomputed; f.cov3D == NULL: scales / rotations.  Not both NULL (that form is
// cgs_launch_preprocess's).  filter_only: radii only, f.cov3D set.
int cgs_launch_preprocess_form(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D,
                               const float *colors, const float *opacities, const float *scales, const float *rotations,
                               CgsGeom &g, int32_t *radii, bool filter_only, hipStream_t stream, bool aa) {
    if (P == 0) return CGS_OK;
    CgsProfScope prof(filter_only ? CGS_PROF_FILTER : CGS_PROF_PREPROCESS, stream);
    const int d = f.shs ? f.sh_degree : -1;
    if (filter_only) {
        launch_fwd<true, -1, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, false);
    } else if (f.cov3D) {
        switch (d) {
            case -1: launch_fwd<false, -1, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            case 0: launch_fwd<false, 0, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            case 1: launch_fwd<false, 1, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            case 2: launch_fwd<false, 2, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            default: launch_fwd<false, 3, true>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
        }
    } else {
        switch (d) {
            case 0: launch_fwd<false, 0, false>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            case 1: launch_fwd<false, 1, false>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            case 2: launch_fwd<false, 2, false>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
            default: launch_fwd<false, 3, false>(cfg, P, f, means3D, colors, opacities, scales, rotations, g, radii, stream, aa); break;
        }
    }
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_preprocess_bwd_form(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D,
                                   const float *scales, const float *rotations, const int32_t *radii,
                                   const float *dL_dmean2D_px, const float *dL_dconic, const float *dL_dcolors,
                                   float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dshs, float *dL_dscales,
                                   float *dL_drotations, float *dL_dcov3D, hipStream_t stream, const float *aa_opacities,
                                   float *aa_dL_dopacities, const float *dL_dabs_px) {
    if (P == 0) return CGS_OK;
    CgsProfScope prof(CGS_PROF_PREPROCESS_BWD, stream);
    const int d = f.shs ? f.sh_degree : -1;
#define CGS_BWD_ARGS cfg, P, f, means3D, scales, rotations, radii, dL_dmean2D_px, dL_dconic, dL_dcolors, dL_dmeans3D, dL_dmeans2D, \
                     dL_dshs, dL_dscales, dL_drotations, dL_dcov3D, stream, aa_opacities, aa_dL_dopacities, dL_dabs_px
    if (f.cov3D) {
        switch (d) {
            case -1: launch_bwd<-1, true>(CGS_BWD_ARGS); break;
            case 0: launch_bwd<0, true>(CGS_BWD_ARGS); break;
            case 1: launch_bwd<1, true>(CGS_BWD_ARGS); break;
            case 2: launch_bwd<2, true>(CGS_BWD_ARGS); break;
            default: launch_bwd<3, true>(CGS_BWD_ARGS); break;
        }
    } else {
        switch (d) {
            case 0: launch_bwd<0, false>(CGS_BWD_ARGS); break;
            case 1: launch_bwd<1, false>(CGS_BWD_ARGS); break;
            case 2: launch_bwd<2, false>(CGS_BWD_ARGS); break;
            default: launch_bwd<3, false>(CGS_BWD_ARGS); break;
        }
    }
#undef CGS_BWD_ARGS
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
