// Per-pixel geometry regularisers of a rendered view: the depth-distortion map and the median depth, forward and backward.
//
// For pixel p the contributors i = 1..n are exactly those of the colour blend (same front-to-back order, same alpha, same skip
// below 1/255, each pixel stopping at n_contrib; with antialiasing the records hold opacity * h).  With T_1 = 1,
// T_{i+1} = T_i (1 - alpha_i), w_i = alpha_i T_i, z_i the view depth of Gaussian i's centre, A_i = sum_{k<=i} w_k and
// D_i = sum_{k<=i} w_k z_k:
//   distortion[p]   = 2 sum_i w_i (z_i A_{i-1} - D_{i-1})        (= sum_{i,j} w_i w_j |z_i - z_j|: the lists are sorted by z)
//   median_depth[p] = z_m, m = the first contributor with T_m (1 - alpha_m) < 0.5 (0 where none), median_id[p] = its index (-1)
// Both are one more walk of the view's final tile lists, the kernels of raster_aux.hip with other per-pixel state: the same
// lane -> pixel map, block masks, per-row lists and staging (raster_rows.h).
//
// Depths are taken relative to the tile's front-most list entry, zr = z - z_ref with z_ref = z of gid_sorted[range.x]: the
// distortion does not change under a shift of z, and z A - D loses three digits to cancellation at z ~ 3 with a spread of 0.1
// that zr A - Dr does not lose.  The moments buffer the backward reads holds (A_n, Dr_n = D_n - z_ref A_n) accordingly; the
// backward takes the same z_ref from the same list entry.
#include "raster_rows.h"

#define GM_NGRAD 7           // gx, gy, gx dx, gx dy, gy dy, dL/dG, dL/dz

namespace {

// The staged form of an entry: r0 = (px, py, A, B) as in the record, r1 = (C, opacity, z - z_ref, the Gaussian's index as bits).
__device__ __forceinline__ float4 gm_r1(const float4 rec1, uint32_t zbits, float z_ref, uint32_t g) {
    return make_float4(rec1.x, rec1.y, __uint_as_float(zbits) - z_ref, __uint_as_float(g));
}

}  // namespace

// Forward: one workgroup per tile, front to back up to the colour pass's stopping points, as aux_fwd_kernel.  Per pixel it
// carries T, A, Dr and the distortion, and latches the first contributor that takes T below one half.
__global__ void __launch_bounds__(AX_THREADS)
    geom_maps_fwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                         const float4 *__restrict__ rec, const uint32_t *__restrict__ depth_key,
                         const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                         const uint32_t *__restrict__ tile_order, float *__restrict__ out_distortion,
                         float *__restrict__ out_median_depth, int32_t *__restrict__ out_median_id,
                         float *__restrict__ out_moments) {
    __shared__ float4 srec[AX_THREADS * 2];
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

    float T = 1.f, A = 0.f, Dr = 0.f, dist = 0.f, z_ref = 0.f, med_zr = 0.f;
    int32_t med_id = -1;
    if (tlast > 0) {      // (uniform over the workgroup)
        const uint2 range = ranges[tile];
        z_ref = __uint_as_float(depth_key[gid_sorted[range.x]]);
        const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
        uint32_t pz = 0, pg = 0;
        if ((uint32_t)tid < tlast) {
            pg = gid_sorted[range.x + tid];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
            pz = depth_key[pg];
        }
        for (int bi = 0; bi < nbatch; ++bi) {
            const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
            const uint32_t pos = base_pos + tid;
            uint32_t m16 = 0;
            __syncthreads();      // the previous batch's walk is over: LDS may be rewritten
            if (pos < tlast) {
                srec[tid * 2] = p0;
                srec[tid * 2 + 1] = gm_r1(p1, pz, z_ref, pg);
                m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
            } else {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                srec[tid * 2] = z; srec[tid * 2 + 1] = z;
            }
            {
                const uint32_t nxt = pos + AX_THREADS;
                if (nxt < tlast) {
                    pg = gid_sorted[range.x + nxt];
                    p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
                    pz = depth_key[pg];
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
                const float alpha = act ? ev.alpha : 0.f;      // alpha = 0: an exact no-op below (T >= 0.5 stays unlatched)
                const float w = alpha * T;
                dist = fmaf(w, fmaf(r1.z, A, -Dr), dist);
                A += w;
                Dr = fmaf(r1.z, w, Dr);
                T = T * (1.f - alpha);
                const bool cross = act && med_id < 0 && T < 0.5f;
                med_zr = cross ? r1.z : med_zr;
                med_id = cross ? (int32_t)__float_as_uint(r1.w) : med_id;
            }
        }
    }
    if (inside) {
        out_distortion[pix] = 2.f * dist;
        out_median_depth[pix] = med_id >= 0 ? med_zr + z_ref : 0.f;
        out_median_id[pix] = med_id;
        out_moments[pix] = A;
        out_moments[(size_t)W * H + pix] = Dr;
    }
}

// Backward: back to front as aux_bwd_kernel.  The suffix sums SA = sum_{k>i} w_k and SD = sum_{k>i} w_k zr_k run with the walk,
// A_{i-1} = A_n - SA - w_i and Dr_{i-1} = Dr_n - SD - w_i zr_i follow from the saved moments, and
//   e_i = 2 [zr_i A_{i-1} - Dr_{i-1} + SD - zr_i SA]
// is d distortion / d w_i: the colour recurrence runs on the scalar c_i = gd e_i (zero background).  The direct terms:
// dL/dz_i += gd 2 w_i (A_{i-1} - SA), and gm for the Gaussian the forward latched as the pixel's median.  Adds into the colour
// pass's accumulators and dL_dz through the LDS accumulation and the flush of aux_bwd_kernel.
__global__ void __launch_bounds__(AX_THREADS)
    geom_maps_bwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                         const float4 *__restrict__ rec, const uint32_t *__restrict__ depth_key,
                         const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                         const uint32_t *__restrict__ tile_last, const uint32_t *__restrict__ tile_order,
                         const float *__restrict__ moments, const int32_t *__restrict__ median_id,
                         const float *__restrict__ dL_ddistortion, const float *__restrict__ dL_dmedian_depth,
                         float *__restrict__ dL_dmean2D_px, float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity,
                         float *__restrict__ dL_dz) {
    __shared__ float4 srec[AX_THREADS * 2];
    __shared__ float sacc[AX_THREADS][GM_NGRAD];
    __shared__ AxLists S;

    const int tile = (int)tile_order[blockIdx.x];
    const uint32_t tlast = tile_last[tile];
    if (tlast == 0) return;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AxLane L = ax_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    const float pxf = (float)L.px, pyf = (float)L.py;
    const uint2 range = ranges[tile];
    const float z_ref = __uint_as_float(depth_key[gid_sorted[range.x]]);
    const size_t pix = (size_t)L.py * W + L.px;

    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    const uint32_t blk_last = ax_row_max(my_last);
    float T = inside ? final_T[pix] : 0.f;
    const float gd = (inside && dL_ddistortion) ? dL_ddistortion[pix] : 0.f;
    const float gm = (inside && dL_dmedian_depth) ? dL_dmedian_depth[pix] : 0.f;
    // (a pixel without a median, or without a gradient for it, matches no entry: indices are < 2^31)
    const uint32_t mid = (inside && dL_dmedian_depth && gm != 0.f) ? (uint32_t)median_id[pix] : 0xFFFFFFFFu;
    const float An = (inside && dL_ddistortion) ? moments[pix] : 0.f;
    const float Dn = (inside && dL_ddistortion) ? moments[(size_t)W * H + pix] : 0.f;
    float SA = 0.f, SD = 0.f;
    float acc_dot = 0.f, last_cdot = 0.f, last_alpha = 0.f;

    const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    uint32_t pz = 0, pg = 0;
    {
        const uint32_t pos0 = (uint32_t)(nbatch - 1) * AX_THREADS + tid;
        if (pos0 < tlast) {
            pg = gid_sorted[range.x + pos0];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
            pz = depth_key[pg];
        }
    }
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
        const uint32_t pos = base_pos + tid;
        uint32_t m16 = 0;
        __syncthreads();   // previous batch fully flushed before LDS is reused
        if (pos < tlast) {
            srec[tid * 2] = p0;
            srec[tid * 2 + 1] = gm_r1(p1, pz, z_ref, pg);
            m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
        } else {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            srec[tid * 2] = z; srec[tid * 2 + 1] = z;
        }
        if (bi > 0) {      // every position of an earlier batch is < tlast
            pg = gid_sorted[range.x + pos - AX_THREADS];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
            pz = depth_key[pg];
        }
#pragma unroll
        for (int k = 0; k < GM_NGRAD; ++k) sacc[tid][k] = 0.f;
        S.smask[tid] = (uint16_t)m16;
        __syncthreads();

        {
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
                T = T / (1.f - alpha);
                const float w = alpha * T;
                const float zr = r1.z;
                const float Ap = (An - SA) - w;                      // A_{i-1}
                const float Dp = fmaf(-w, zr, Dn - SD);              // Dr_{i-1}
                acc_dot = fmaf(last_alpha, last_cdot, (1.f - last_alpha) * acc_dot);
                last_cdot = 2.f * gd * (fmaf(zr, Ap, -Dp) + fmaf(-zr, SA, SD));
                const float dL_dalpha = (last_cdot - acc_dot) * T;
                last_alpha = alpha;
                const float gG = Gm * dL_dalpha;
                const float gx = gG * ev.dx, gy = gG * ev.dy;
                float v[8];
                v[0] = gx;
                v[1] = gy;
                v[2] = gx * ev.dx;
                v[3] = gx * ev.dy;
                v[4] = gy * ev.dy;
                v[5] = gG;
                v[6] = fmaf(2.f * gd * w, Ap - SA, (act && __float_as_uint(r1.w) == mid) ? gm : 0.f);
                v[7] = 0.f;
                SA += w;
                SD = fmaf(w, zr, SD);
                const int sub = lane & 15;
                const float red = ax_row_transpose_sum(v, lane, sub);
                if (has && sub < GM_NGRAD && red != 0.f) atomicAdd(&sacc[e][sub], red);
            }
        }
        __syncthreads();
        if (pos < tlast) {
            const float a0 = sacc[tid][0], a1 = sacc[tid][1], a2 = sacc[tid][2], a3 = sacc[tid][3],
                        a4 = sacc[tid][4], a5 = sacc[tid][5], a6 = sacc[tid][6];
            if (a0 != 0.f || a1 != 0.f || a2 != 0.f || a3 != 0.f || a4 != 0.f || a5 != 0.f || a6 != 0.f) {
                const uint32_t g = gid_sorted[range.x + pos];
                ax_flush_geom(g, srec[tid * 2], srec[tid * 2 + 1], a0, a1, a2, a3, a4, a5, dL_dmean2D_px, dL_dconic, dL_dopacity);
                atomicAdd(&dL_dz[g], a6);
            }
        }
    }
}

int cgs_launch_geom_maps_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, float *out_distortion,
                             float *out_median_depth, int32_t *out_median_id, float *out_moments, hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(geom_maps_fwd_kernel, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)g.depth_key, (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last,
                       (const uint32_t *)im.tile_order, out_distortion, out_median_depth, out_median_id, out_moments);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_geom_maps_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *moments,
                             const int32_t *median_id, const float *dL_ddistortion, const float *dL_dmedian_depth,
                             float *dL_dmean2D_px, float *dL_dconic, float *dL_dopacity, float *dL_dz, hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(geom_maps_bwd_kernel, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)g.depth_key, (const float *)im.final_T, (const uint32_t *)im.n_contrib,
                       (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, moments, median_id, dL_ddistortion,
                       dL_dmedian_depth, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dz);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
