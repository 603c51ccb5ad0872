// Per-Gaussian contribution statistics of a rendered view, and the per-pixel top-contributor maps.  Forward only: nothing
// here is differentiable.
//
// For pixel p the contributors i are exactly those of the colour blend (same front-to-back order, same alpha, same skip below
// 1/255, each pixel stopping where the colour pass stopped it) and w_i(p) = alpha_i T_i > 0 for a contributor, 0 otherwise.
//   per Gaussian i, ACCUMULATED into caller-owned arrays (row slot[i], or i without a slot table):
//     weight     += sum_p w_i(p)                      max_weight  = max(max_weight, max_p w_i(p))
//     pixels     += #{p : w_i(p) > 0}                 top_pixels += #{p : i has the largest w of p's contributors}
//   per pixel p, written for every pixel:
//     top_id = that largest contributor (-1: none; an exact tie goes to the front-most), top_weight = its w, count = the
//     number of contributors.
// The kernel is the walk of aux_fwd_kernel (raster_aux.hip) without the depth: the same lane -> pixel map, octagon block
// culling and per-row lists (raster_rows.h), run behind the colour pass of the view on what it left (gid_sorted, ranges,
// tile_order, n_contrib, tile_last).  The records hold opacity * h under antialiasing, so nothing here knows of it.  In place
// of a per-pixel accumulation, every visited entry is reduced over the 16 lanes (pixels) of its row: the sum and the maximum
// of w with four DPP steps each (ax_row_reduce), the count from the row's 16 bits of the ballot.  Lane 0 of the row adds the three into the
// batch's LDS accumulator [256] x {float sum, uint max = the bit pattern of a float >= 0, uint count} with LDS atomics (up to
// 16 rows meet on one entry); after the batch's walk thread `tid` flushes entry `tid` to global memory with one float
// atomicAdd, one int atomicMax on the bit pattern and one 64-bit atomicAdd, if its count is non-zero.  Each lane also carries
// its pixel's best (w, 1-based position), replaced on strict >, and after the last batch looks the position up in gid_sorted,
// writes the three maps and does one 64-bit atomicAdd to top_pixels: one global atomic per covered pixel.
// `weight` is summed with float atomics: not bit-reproducible.  The other six results are.
//
// Budget (256 threads = 4 waves per workgroup; a CU has 160 KiB of LDS and 512 VGPRs per lane and SIMD), from
// -Rpass-analysis=kernel-resource-usage of the gfx950 build:
//   with the reduction (any of weight / max_weight / pixels asked): LDS = 8 KiB records + 4.5 KiB lists + 3 KiB sums =
//     15872 bytes (10 workgroups per CU by LDS); 72 VGPRs, no scratch: 7 waves per SIMD = 7 workgroups per CU.
//   without it (maps and top_pixels only): LDS = 12800 bytes, 64 VGPRs, no scratch: 8 workgroups per CU.
//   (aux_fwd_kernel, the same walk with three per-pixel sums: 12800 bytes of LDS.)
// The alternative to 16 rows meeting on one LDS accumulator, one accumulator per wave ([4][256] x 3, 12 KiB instead of 3) with a
// 4-way add at the flush, builds with -DCGS_EXPERIMENTS -DCT_PARTS=4 (25088 bytes of LDS, 78 VGPRs, 6 waves per SIMD) and has not
// been timed yet; measured on an MI355X at the bench view the product kernel takes 1.89 x aux_fwd_kernel, the instance without
// the reduction 1.13 x (DESIGN.md sections 7 and 8, profiles/raster_contrib.txt).
// No inline assembly here: aux_fwd_kernel's empty register barrier on (pxf, pyf) changes nothing in this kernel's allocation.
#include "raster_rows.h"

// copies of the batch's LDS accumulator: 1 = all 16 rows of the workgroup meet on one, 4 = one per wave (its 4 rows)
#if defined(CGS_EXPERIMENTS) && defined(CT_PARTS)
#define CT_NPART CT_PARTS
#else
#define CT_NPART 1
#endif

// ACC: the per-entry reduction and its flush (weight, max_weight, pixels); without it the walk only tracks each pixel's best.
template <bool ACC>
__global__ void __launch_bounds__(AX_THREADS)
    contrib_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ gid_sorted,
                   const float4 *__restrict__ rec, const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                   const uint32_t *__restrict__ tile_order, const int32_t *__restrict__ slot, float *__restrict__ acc_weight,
                   int *__restrict__ acc_max_weight, unsigned long long *__restrict__ acc_pixels,
                   unsigned long long *__restrict__ acc_top_pixels, int32_t *__restrict__ out_top_id,
                   float *__restrict__ out_top_weight, int32_t *__restrict__ out_count) {
    __shared__ float4 srec[AX_THREADS * 2];
    __shared__ float ssum[CT_NPART][AX_THREADS];
    __shared__ uint32_t smax[CT_NPART][AX_THREADS];
    __shared__ uint32_t scnt[CT_NPART][AX_THREADS];
    __shared__ AxLists S;

    const int tile = (int)tile_order[blockIdx.x];
    const uint32_t tlast = tile_last[tile];
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AxLane L = ax_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    const float pxf = (float)L.px, pyf = (float)L.py;
    const size_t pix = (size_t)L.py * W + L.px;
    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    const uint32_t blk_last = ax_row_max(my_last);
    const int row_shift = lane & 48;
    const int part = CT_NPART == 4 ? wave : 0;

    float T = 1.f, best_w = 0.f;
    uint32_t best_pos = 0, my_cnt = 0;      // best_pos: 1-based position in the tile's list, 0 = no contributor
    uint2 range = make_uint2(0u, 0u);
    if (tlast > 0) {      // (uniform over the workgroup)
        range = ranges[tile];
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
            const uint32_t g_cur = pg;
            uint32_t m16 = 0;
            __syncthreads();      // the previous batch's walk is over: LDS may be rewritten
            if (pos < tlast) {
                srec[tid * 2] = p0;
                srec[tid * 2 + 1] = p1;
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
                }
            }
            if (ACC) {
#pragma unroll
                for (int k = 0; k < CT_NPART; ++k) { ssum[k][tid] = 0.f; smax[k][tid] = 0u; scnt[k][tid] = 0u; }
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
                const uint64_t hits = ax_ballot(act);
                if (hits == 0ull) continue;
                const float alpha = act ? ev.alpha : 0.f;      // alpha = 0: w = 0 and an exact no-op below
                const float w = alpha * T;
                T = T * (1.f - alpha);
                my_cnt += act ? 1u : 0u;
                if (w > best_w) { best_w = w; best_pos = base_pos + e + 1u; }
                if (ACC) {
                    const uint32_t rc = (uint32_t)__builtin_popcount((uint32_t)(hits >> row_shift) & 0xFFFFu);
                    const float rs = ax_row_reduce(w, [](float a, float b) { return a + b; });
                    const float rm = ax_row_reduce(w, [](float a, float b) { return fmaxf(a, b); });
                    if ((lane & 15) == 0 && rc != 0u) {      // (rc != 0 implies `has`: the row's lanes share i and cnt)
                        atomicAdd(&ssum[part][e], rs);
                        atomicMax(&smax[part][e], __float_as_uint(rm));
                        atomicAdd(&scnt[part][e], rc);
                    }
                }
            }
            if (ACC) {
                __syncthreads();
                uint32_t c = 0u, mx = 0u;
                float sm = 0.f;
#pragma unroll
                for (int k = 0; k < CT_NPART; ++k) { c += scnt[k][tid]; mx = max(mx, smax[k][tid]); sm += ssum[k][tid]; }
                if (c != 0u) {      // (only entries at pos < tlast are ever visited)
                    const size_t r = slot ? (size_t)slot[g_cur] : (size_t)g_cur;
                    if (acc_weight) atomicAdd(&acc_weight[r], sm);
                    if (acc_max_weight) atomicMax(&acc_max_weight[r], (int)mx);
                    if (acc_pixels) atomicAdd(&acc_pixels[r], (unsigned long long)c);
                }
            }
        }
    }
    if (inside) {
        const int32_t g = best_pos ? (int32_t)gid_sorted[range.x + best_pos - 1u] : -1;
        if (out_top_id) out_top_id[pix] = g;
        if (out_top_weight) out_top_weight[pix] = best_w;
        if (out_count) out_count[pix] = (int32_t)my_cnt;
        if (acc_top_pixels && g >= 0) atomicAdd(&acc_top_pixels[slot ? (size_t)slot[g] : (size_t)g], 1ull);
    }
}

// Any of the seven outputs may be NULL (not computed); the caller has checked that one is given.  slot: NULL = identity.
int cgs_launch_contrib(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const int32_t *slot, float *acc_weight,
                       float *acc_max_weight, int64_t *acc_pixels, int64_t *acc_top_pixels, int32_t *out_top_id,
                       float *out_top_weight, int32_t *out_count, hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    const bool acc = acc_weight || acc_max_weight || acc_pixels;
    auto kernel = acc ? contrib_kernel<true> : contrib_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tx * ty)), dim3(AX_THREADS), 0, stream, cfg->image_width, cfg->image_height, tx,
                       (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, (const float4 *)g.rec,
                       (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last, (const uint32_t *)im.tile_order, slot,
                       acc_weight, (int *)acc_max_weight, (unsigned long long *)acc_pixels,
                       (unsigned long long *)acc_top_pixels, out_top_id, out_top_weight, out_count);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
