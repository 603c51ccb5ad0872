// Blend of a caller-supplied per-Gaussian table features [P, C] (1 <= C <= CGS_RASTER_MAX_FEATURES), forward and backward.
//
// For pixel p the contributors i are exactly those of the colour blend (same front-to-back order, same alpha, same skip below
// 1/255, each pixel stopping where the colour pass stopped it) and w_i = alpha_i T_i:
//   features_map[c, p] = sum_i w_i features[i, c],   zero background, values of any sign, nothing clamped.
// The kernels are the walks of raster_aux.hip with the table's row in place of (z, 1/z, 1): the same lane -> pixel map, octagon
// block culling and per-row lists (raster_rows.h), run behind the colour pass of the view on what it left (gid_sorted, ranges,
// tile_order, n_contrib, tile_last, final_T).  The records hold opacity * h under antialiasing, so nothing here knows of it.
//
// Budgets (256 threads = 4 waves per workgroup; a CU has 160 KiB of LDS and 512 VGPRs per lane and SIMD):
//   forward, one pass over all channels, instances of 4 / 8 / 16 / 32 channels (the smallest that holds C): LDS = 8 KiB records
//     + 4.5 KiB lists + 1 KiB per channel = 16.5 .. 44.5 KiB, i.e. 9 .. 3 workgroups per CU; hipcc allocates 72 / 80 / 96 /
//     134 VGPRs (7 / 6 / 5 / 3 waves per SIMD), no scratch: the 32-channel instance runs 3 waves per SIMD by either limit.
//   backward, passes of FT_BWD_NC = 8 channels (blockIdx.y = the pass).  The geometry gradient is linear in the upstream
//     gradient, so every pass is a complete backward of its own channels and adds its share into the same accumulators.
//     6 geometry sums + 8 channel sums are ONE 16-value transposing reduction over the 16 lanes of a row.  LDS = 8 KiB
//     records + 8 KiB feature rows + 16 KiB sums + 4.5 KiB lists = 36.5 KiB and 95 VGPRs: 4 workgroups per CU by both.
// dL_dfeatures, like dL_dcolors, is summed with float atomics (LDS per batch, then global): not bit-reproducible.
#include "raster_rows.h"

#define FT_BWD_NC 8
#define FT_NSUM 16           // gx, gy, gx dx, gx dy, gy dy, dL/dG, 8 x dL/dfeature, 2 unused

// ---- forward --------------------------------------------------------------------------------------------------------------
// One workgroup per tile, walking up to the colour pass's stopping points as aux_fwd_kernel does.  The feature rows of a batch
// are staged next to the records, channel-quad major (sfeat[q][entry]): conflict-free stores, broadcast reads.
template <int NC>
__global__ void __launch_bounds__(AX_THREADS)
    feat_fwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                    const float4 *__restrict__ rec, const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                    const uint32_t *__restrict__ tile_order, const float *__restrict__ features, int C, float *__restrict__ out) {
    constexpr int NQ = NC / 4;
    __shared__ float4 srec[AX_THREADS * 2];
    __shared__ float4 sfeat[NQ * AX_THREADS];
    __shared__ AxLists S;

    const int tile = (int)tile_order[blockIdx.x];
    const uint32_t tlast = tile_last[tile];
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AxLane L = ax_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    float pxf = (float)L.px, pyf = (float)L.py;
    asm volatile("" : "+v"(pxf), "+v"(pyf));
    const size_t pix = (size_t)L.py * W + L.px;
    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    const uint32_t blk_last = ax_row_max(my_last);

    float T = 1.f;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    if (tlast > 0) {      // (uniform over the workgroup)
        const uint2 range = ranges[tile];
        const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
        uint32_t pg = 0;
        if ((uint32_t)tid < tlast) {
            pg = gid_sorted[range.x + tid];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
        }
        for (int bi = 0; bi < nbatch; ++bi) {
            const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
            const uint32_t pos = base_pos + tid;
            uint32_t m16 = 0;
            // the entry's feature row, requested before the barrier: its latency runs while the other waves finish their walk
            float f[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) f[c] = (pos < tlast && c < C) ? features[(size_t)pg * C + c] : 0.f;
            __syncthreads();      // the previous batch's walk is over: LDS may be rewritten
            if (pos < tlast) {
                srec[tid * 2] = p0;
                srec[tid * 2 + 1] = p1;
                m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
            } else {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                srec[tid * 2] = z; srec[tid * 2 + 1] = z;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                sfeat[q * AX_THREADS + tid] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
            {
                const uint32_t nxt = pos + AX_THREADS;
                if (nxt < tlast) {
                    pg = gid_sorted[range.x + nxt];
                    p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
                }
            }
            S.smask[tid] = (uint16_t)m16;
            __syncthreads();
            const uint32_t cnt = ax_list_build(S, L.blk, lane, (int)blk_last - (int)base_pos - 1);
            uint32_t i = 0;
            uint32_t e_next = S.list[L.blk][0];
            while (ax_ballot(i < cnt) != 0ull) {
                const bool has = i < cnt;
                const uint32_t e = e_next;
                i += has ? 1u : 0u;
                e_next = S.list[L.blk][i & (AX_THREADS - 1)];
                const float4 r0 = srec[e * 2], r1 = srec[e * 2 + 1];
                const AxEval ev = ax_eval(r0, r1, pxf, pyf);
                const bool act = has && (base_pos + e + 1u <= my_last) && ev.hit;
                if (ax_ballot(act) == 0ull) continue;
                const float alpha = act ? ev.alpha : 0.f;      // alpha = 0: an exact no-op below (finite features)
                const float w = alpha * T;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const float4 fv = sfeat[q * AX_THREADS + e];
                    acc[4 * q] = fmaf(fv.x, w, acc[4 * q]);
                    acc[4 * q + 1] = fmaf(fv.y, w, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(fv.z, w, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(fv.w, w, acc[4 * q + 3]);
                }
                T = T * (1.f - alpha);
            }
        }
    }
    if (inside) {
        const size_t plane = (size_t)W * H;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < C) out[c * plane + pix] = acc[c];
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------
// Back to front as aux_bwd_kernel, for the channels [c0, c0 + 8) of pass blockIdx.y, with the colour recurrence on the scalar
// c_i(p) = sum_c features[i, c] g[c, p] (zero background), plus dL/dfeatures[i, c] = sum_p w_i(p) g[c, p].  Adds into the
// colour pass's accumulators dL/d(pixel mean), dL/d(conic), dL/dopacity; the per-batch LDS sums and the flush are those of
// aux_bwd_kernel with sixteen sums per entry instead of seven.
__global__ void __launch_bounds__(AX_THREADS)
    feat_bwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                    const float4 *__restrict__ rec, const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                    const uint32_t *__restrict__ tile_last, const uint32_t *__restrict__ tile_order,
                    const float *__restrict__ features, int C, const float *__restrict__ dL_dmap,
                    float *__restrict__ dL_dmean2D_px, float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity,
                    float *__restrict__ dL_dfeatures) {
    __shared__ float4 srec[AX_THREADS * 2];
    __shared__ float4 sfeat[2 * AX_THREADS];
    __shared__ float4 sacc[AX_THREADS][FT_NSUM / 4];
    __shared__ AxLists S;

    const int tile = (int)tile_order[blockIdx.x];
    const uint32_t tlast = tile_last[tile];
    if (tlast == 0) return;
    const int c0 = (int)blockIdx.y * FT_BWD_NC;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AxLane L = ax_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    const float pxf = (float)L.px, pyf = (float)L.py;
    const uint2 range = ranges[tile];
    const size_t pix = (size_t)L.py * W + L.px;
    const size_t plane = (size_t)W * H;

    const float T_final = inside ? final_T[pix] : 0.f;
    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    const uint32_t blk_last = ax_row_max(my_last);
    float T = T_final;
    float gF[FT_BWD_NC];
#pragma unroll
    for (int c = 0; c < FT_BWD_NC; ++c) gF[c] = (inside && c0 + c < C) ? dL_dmap[(size_t)(c0 + c) * plane + pix] : 0.f;
    float acc_dot = 0.f, last_cdot = 0.f, last_alpha = 0.f;

    const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    uint32_t pg = 0;
    {
        const uint32_t pos0 = (uint32_t)(nbatch - 1) * AX_THREADS + tid;
        if (pos0 < tlast) {
            pg = gid_sorted[range.x + pos0];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
        }
    }
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
        const uint32_t pos = base_pos + tid;
        const uint32_t g_cur = pg;
        uint32_t m16 = 0;
        float f[FT_BWD_NC];
#pragma unroll
        for (int c = 0; c < FT_BWD_NC; ++c) f[c] = (pos < tlast && c0 + c < C) ? features[(size_t)pg * C + c0 + c] : 0.f;
        __syncthreads();   // previous batch fully flushed before LDS is reused
        if (pos < tlast) {
            srec[tid * 2] = p0;
            srec[tid * 2 + 1] = p1;
            m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
        } else {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            srec[tid * 2] = z; srec[tid * 2 + 1] = z;
        }
        sfeat[tid] = make_float4(f[0], f[1], f[2], f[3]);
        sfeat[AX_THREADS + tid] = make_float4(f[4], f[5], f[6], f[7]);
        if (bi > 0) {      // every position of an earlier batch is < tlast
            pg = gid_sorted[range.x + pos - AX_THREADS];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
        }
#pragma unroll
        for (int k = 0; k < FT_NSUM / 4; ++k) sacc[tid][k] = make_float4(0.f, 0.f, 0.f, 0.f);
        S.smask[tid] = (uint16_t)m16;
        __syncthreads();

        {
            float *sums = (float *)sacc;
            int i = (int)ax_list_build(S, L.blk, lane, (int)blk_last - (int)base_pos - 1) - 1;
            uint32_t e_next = S.list[L.blk][max(i, 0)];
            while (ax_ballot(i >= 0) != 0ull) {
                const bool has = i >= 0;
                const uint32_t e = e_next;
                i -= has ? 1 : 0;
                e_next = S.list[L.blk][max(i, 0)];
                const uint32_t position = base_pos + e + 1u;         // 1-based
                const float4 r0 = srec[e * 2], r1 = srec[e * 2 + 1];
                const AxEval ev = ax_eval(r0, r1, pxf, pyf);
                const bool act = has && (position <= my_last) && ev.hit;
                if (ax_ballot(act) == 0ull) continue;
                // branch-free as in aux_bwd_kernel: alpha = 0, G = 0 make every update below an exact no-op
                const float alpha = act ? ev.alpha : 0.f, Gm = act ? ev.g : 0.f;
                const float4 f0 = sfeat[e], f1 = sfeat[AX_THREADS + e];
                T = T / (1.f - alpha);
                const float w = alpha * T;
                acc_dot = fmaf(last_alpha, last_cdot, (1.f - last_alpha) * acc_dot);
                last_cdot = fmaf(f0.x, gF[0], fmaf(f0.y, gF[1], fmaf(f0.z, gF[2], fmaf(f0.w, gF[3],
                            fmaf(f1.x, gF[4], fmaf(f1.y, gF[5], fmaf(f1.z, gF[6], f1.w * gF[7])))))));
                const float dL_dalpha = (last_cdot - acc_dot) * T;
                last_alpha = alpha;
                const float gG = Gm * dL_dalpha;
                const float gx = gG * ev.dx, gy = gG * ev.dy;
                float v[FT_NSUM];
                v[0] = gx;
                v[1] = gy;
                v[2] = gx * ev.dx;
                v[3] = gx * ev.dy;
                v[4] = gy * ev.dy;
                v[5] = gG;
#pragma unroll
                for (int c = 0; c < FT_BWD_NC; ++c) v[6 + c] = w * gF[c];
                v[14] = 0.f;
                v[15] = 0.f;
                const int sub = lane & 15;
                const float red = ax_row_transpose_sum(v, lane, sub);
                if (has && sub < 6 + FT_BWD_NC && red != 0.f) atomicAdd(&sums[e * FT_NSUM + sub], red);
            }
        }
        __syncthreads();
        if (pos < tlast) {
            const float4 s0 = sacc[tid][0], s1 = sacc[tid][1], s2 = sacc[tid][2], s3 = sacc[tid][3];
            const float a0 = s0.x, a1 = s0.y, a2 = s0.z, a3 = s0.w, a4 = s1.x, a5 = s1.y;
            const float df[FT_BWD_NC] = {s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y};
            if (a0 != 0.f || a1 != 0.f || a2 != 0.f || a3 != 0.f || a4 != 0.f || a5 != 0.f) {
                ax_flush_geom(g_cur, srec[tid * 2], srec[tid * 2 + 1], a0, a1, a2, a3, a4, a5, dL_dmean2D_px, dL_dconic, dL_dopacity);
            }
#pragma unroll
            for (int c = 0; c < FT_BWD_NC; ++c)
                if (c0 + c < C && df[c] != 0.f) atomicAdd(&dL_dfeatures[(size_t)g_cur * C + c0 + c], df[c]);
        }
    }
}

template <int NC>
static void feat_fwd_launch(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *features, int C, float *out,
                            hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(feat_fwd_kernel<NC>, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, features, C,
                       out);
}

// features [P, C], out [C, H, W]; 1 <= C <= CGS_RASTER_MAX_FEATURES (checked by the caller)
int cgs_launch_feat_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *features, int C, float *out,
                        hipStream_t stream) {
    if (C <= 4) feat_fwd_launch<4>(cfg, g, b, im, features, C, out, stream);
    else if (C <= 8) feat_fwd_launch<8>(cfg, g, b, im, features, C, out, stream);
    else if (C <= 16) feat_fwd_launch<16>(cfg, g, b, im, features, C, out, stream);
    else feat_fwd_launch<32>(cfg, g, b, im, features, C, out, stream);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_feat_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *features, int C,
                        const float *dL_dmap, float *dL_dmean2D_px, float *dL_dconic, float *dL_dopacity, float *dL_dfeatures,
                        hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(feat_bwd_kernel, dim3((unsigned)(tx * ty), (unsigned)((C + FT_BWD_NC - 1) / FT_BWD_NC)), dim3(AX_THREADS),
                       0, stream, cfg->image_width, cfg->image_height, tx, (const uint2 *)im.ranges,
                       (const uint32_t *)b.gid_sorted, (const float4 *)g.rec, (const float *)im.final_T,
                       (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, features, C,
                       dL_dmap, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dfeatures);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
