// Per-pixel geometry maps of a rendered view: depth, inverse depth and alpha, forward and backward.
//
// For pixel p the contributors i are exactly those of the colour blend (same front-to-back order, same alpha, same skip below
// 1/255, same stop at T (1 - alpha) < 1e-4) and w_i = alpha_i T_i, z_i = the view depth of Gaussian i's centre:
//   depth[p] = sum_i w_i z_i,   invdepth[p] = sum_i w_i / z_i,   alpha[p] = 1 - T_final[p] = sum_i w_i.
// Each map is the colour blend of a per-Gaussian scalar (z, 1/z, 1) with a zero background, so the kernels below are the
// row-mapped blend kernels of raster_blend_rows.hip with those scalars in place of the colour: the same lane -> pixel map,
// the same octagon block culling and per-row entry lists, the same staging of the next batch in registers.  They run after
// the colour pass of the view and read what it left: the per-tile lists and their order (gid_sorted, ranges, tile_order),
// where each pixel stopped (n_contrib, tile_last) and its final transmittance (final_T).  z comes from CgsGeom::depth_key
// (the float bits of z of every Gaussian that has a tile; the depth sort reads them and writes elsewhere).
//
// raster_blend_rows.hip stays byte-identical (hipcc's output for it moved when shared code was factored out of it), so the
// few device functions both need are restated under their own names in raster_rows.h, which raster_feat.hip shares.
#include "raster_rows.h"

#define AX_NGRAD 7           // gx, gy, gx dx, gx dy, gy dy, dL/dG, dL/dz
#define AX_PB_THREADS 256

namespace {

// The staged form of an entry: r0 = (px, py, A, B) as in the record, r1 = (C, opacity, z, 1 / z).
__device__ __forceinline__ float4 ax_r1(const float4 rec1, uint32_t zbits) {
    const float z = __uint_as_float(zbits);
    return make_float4(rec1.x, rec1.y, z, 1.f / z);
}

}  // namespace

// Forward: one workgroup per tile (in the colour pass's tile order), walking only up to the colour pass's stopping points.
// Every entry at 1-based position <= n_contrib[p] whose alpha passes the 1/255 test contributed to pixel p in the colour pass,
// so T evolves exactly as there; no termination test is needed.
__global__ void __launch_bounds__(AX_THREADS)
    aux_fwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                   const float4 *__restrict__ rec, const uint32_t *__restrict__ depth_key, const float *__restrict__ final_T,
                   const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                   const uint32_t *__restrict__ tile_order, float *__restrict__ out_depth, float *__restrict__ out_invdepth,
                   float *__restrict__ out_alpha) {
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

    float T = 1.f, dz = 0.f, diz = 0.f;
    if (tlast > 0) {      // (uniform over the workgroup)
        const uint2 range = ranges[tile];
        const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
        uint32_t pz = 0;
        if ((uint32_t)tid < tlast) {
            const uint32_t g = gid_sorted[range.x + tid];
            p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
            pz = depth_key[g];
        }
        for (int bi = 0; bi < nbatch; ++bi) {
            const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
            const uint32_t pos = base_pos + tid;
            uint32_t m16 = 0;
            __syncthreads();      // the previous batch's walk is over: LDS may be rewritten
            if (pos < tlast) {
                srec[tid * 2] = p0;
                srec[tid * 2 + 1] = ax_r1(p1, pz);
                m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
            } else {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                srec[tid * 2] = z; srec[tid * 2 + 1] = z;
            }
            {
                const uint32_t nxt = pos + AX_THREADS;
                if (nxt < tlast) {
                    const uint32_t g = gid_sorted[range.x + nxt];
                    p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
                    pz = depth_key[g];
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
                const float alpha = act ? ev.alpha : 0.f;      // alpha = 0: an exact no-op below
                const float w = alpha * T;
                dz = fmaf(r1.z, w, dz);
                diz = fmaf(r1.w, w, diz);
                T = T * (1.f - alpha);
            }
        }
    }
    if (inside) {
        out_depth[pix] = dz;
        out_invdepth[pix] = diz;
        out_alpha[pix] = 1.f - final_T[pix];
    }
}

// Backward: back to front as blend_bwd_rows_kernel, with the colour recurrence on the scalar c_i = z_i gD + gI / z_i + gA
// (zero background, so no background term), plus dL/dz_i = sum_p w_i (gD - gI / z_i^2).  Adds into the colour pass's
// accumulators dL/d(pixel mean), dL/d(conic), dL/dopacity and into dL_dz; the LDS accumulation and the flush are those of
// blend_bwd_rows_kernel (seven sums instead of nine).
__global__ void __launch_bounds__(AX_THREADS)
    aux_bwd_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                   const float4 *__restrict__ rec, const uint32_t *__restrict__ depth_key, const float *__restrict__ final_T,
                   const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                   const uint32_t *__restrict__ tile_order, const float *__restrict__ dL_ddepth,
                   const float *__restrict__ dL_dinvdepth, const float *__restrict__ dL_dalpha_map,
                   float *__restrict__ dL_dmean2D_px, float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity,
                   float *__restrict__ dL_dz) {
    __shared__ float4 srec[AX_THREADS * 2];
    __shared__ float sacc[AX_THREADS][AX_NGRAD];
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
    const size_t pix = (size_t)L.py * W + L.px;

    const float T_final = inside ? final_T[pix] : 0.f;
    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    const uint32_t blk_last = ax_row_max(my_last);
    float T = T_final;
    const float gD = (inside && dL_ddepth) ? dL_ddepth[pix] : 0.f;
    const float gI = (inside && dL_dinvdepth) ? dL_dinvdepth[pix] : 0.f;
    const float gA = (inside && dL_dalpha_map) ? dL_dalpha_map[pix] : 0.f;
    float acc_dot = 0.f, last_cdot = 0.f, last_alpha = 0.f;

    const int nbatch = (int)((tlast + AX_THREADS - 1) / AX_THREADS);
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    uint32_t pz = 0;
    {
        const uint32_t pos0 = (uint32_t)(nbatch - 1) * AX_THREADS + tid;
        if (pos0 < tlast) {
            const uint32_t g = gid_sorted[range.x + pos0];
            p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
            pz = depth_key[g];
        }
    }
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base_pos = (uint32_t)bi * AX_THREADS;
        const uint32_t pos = base_pos + tid;
        uint32_t m16 = 0;
        __syncthreads();   // previous batch fully flushed before LDS is reused
        if (pos < tlast) {
            srec[tid * 2] = p0;
            srec[tid * 2 + 1] = ax_r1(p1, pz);
            m16 = ax_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
        } else {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            srec[tid * 2] = z; srec[tid * 2 + 1] = z;
        }
        if (bi > 0) {      // every position of an earlier batch is < tlast
            const uint32_t g = gid_sorted[range.x + pos - AX_THREADS];
            p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
            pz = depth_key[g];
        }
#pragma unroll
        for (int k = 0; k < AX_NGRAD; ++k) sacc[tid][k] = 0.f;
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
                // branch-free as in blend_bwd_rows_kernel: alpha = 0, G = 0 make every update below an exact no-op
                const float alpha = act ? ev.alpha : 0.f, Gm = act ? ev.g : 0.f;
                T = T / (1.f - alpha);
                const float w = alpha * T;
                acc_dot = fmaf(last_alpha, last_cdot, (1.f - last_alpha) * acc_dot);
                last_cdot = fmaf(r1.z, gD, fmaf(r1.w, gI, gA));
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
                v[6] = w * fmaf(-gI * r1.w, r1.w, gD);          // w (gD - gI / z^2)
                v[7] = 0.f;
                const int sub = lane & 15;
                const float red = ax_row_transpose_sum(v, lane, sub);
                if (has && sub < AX_NGRAD && red != 0.f) atomicAdd(&sacc[e][sub], red);
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

// dL/dmeans3D += dL/dz * dz/dmeans3D, z = V[2] x + V[6] y + V[10] z + V[14] (column-major view matrix, as cgs_to_view).
// Runs after the preprocess backward, which writes dL_dmeans3D for every Gaussian.
__global__ void __launch_bounds__(AX_PB_THREADS)
    aux_dz_chain_kernel(int64_t P, const float *__restrict__ viewmatrix, const int32_t *__restrict__ radii,
                        const float *__restrict__ dL_dz, float *__restrict__ dL_dmeans3D) {
    const int64_t i = (int64_t)blockIdx.x * AX_PB_THREADS + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;
    const float d = dL_dz[i];
    if (d == 0.f) return;
    dL_dmeans3D[3 * i] += d * viewmatrix[2];
    dL_dmeans3D[3 * i + 1] += d * viewmatrix[6];
    dL_dmeans3D[3 * i + 2] += d * viewmatrix[10];
}

int cgs_launch_aux_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, float *out_depth, float *out_invdepth,
                       float *out_alpha, hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(aux_fwd_kernel, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)g.depth_key, (const float *)im.final_T, (const uint32_t *)im.n_contrib,
                       (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, out_depth, out_invdepth, out_alpha);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_aux_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *dL_ddepth,
                       const float *dL_dinvdepth, const float *dL_dalpha, float *dL_dmean2D_px, float *dL_dconic,
                       float *dL_dopacity, float *dL_dz, hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(aux_bwd_kernel, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)g.depth_key, (const float *)im.final_T, (const uint32_t *)im.n_contrib,
                       (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, dL_ddepth, dL_dinvdepth, dL_dalpha,
                       dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dz);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_aux_dz_chain(const cgs_raster_cfg *cfg, int64_t P, const int32_t *radii, const float *dL_dz, float *dL_dmeans3D,
                            hipStream_t stream) {
    if (P == 0) return CGS_OK;
    hipLaunchKernelGGL(aux_dz_chain_kernel, dim3((unsigned)((P + AX_PB_THREADS - 1) / AX_PB_THREADS)), dim3(AX_PB_THREADS), 0,
                       stream, P, cfg->viewmatrix, radii, dL_dz, dL_dmeans3D);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
