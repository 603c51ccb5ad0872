// Tile alpha-blend forward / backward, ROW-MAPPED variant: the four 16-lane DPP rows of a wave own one 4x4 pixel
// block each (together the wave's 8x8 quadrant) and walk their OWN Gaussian lists, so one wave iteration processes
// up to four different Gaussians.
//
// Why: the blend kernels are VALU-issue bound (~95 wave instructions per (quadrant, Gaussian)
// visit, all 64 lanes issue them however few pixels contribute).  In the dense-anchor scenes of the headline
// benchmark a Gaussian's alpha >= 1/255 footprint overlaps on average only 2.1 of the four 4x4 blocks of a quadrant
// it touches (tools/blend_occupancy.py: 11.9 M quadrant visits per 1080p view, 7.6 M row-mapped iterations), so
// letting the rows advance independently removes a third of the iterations.  Everything the reduction needs already
// happens inside a 16-lane row (two quad butterflies + two row rotations), and each row adds into the LDS
// accumulator of ITS Gaussian (fewer same-address conflicts than four rows adding into one).
//
// Round 3: a row's Gaussians are a LIST of batch indices (rb_list_build: built by the row itself from the staging threads'
// 16-bit block masks, one DPP scan, no atomics) that the row walks with its own cursor - rows no longer wait for each
// other at 32-entry segment boundaries as with the bit masks of round 2 (-18..20 % wave iterations, tools/rb_iters.py);
// blocks are culled against the octagon (box + diagonals) of the alpha >= 1/255 ellipse (rb_block_mask).
// profiles/r03_blend_lists.txt has the measurements, including what the backward's time is made of now.
//
// Same arithmetic per (pixel, Gaussian) as raster_blend.hip (blend_eval is identical), same list order per pixel, so
// results are bit-identical to the quadrant-mapped kernels for the forward and equal up to the summation order of
// the per-Gaussian partial sums for the backward.
#include <stdlib.h>
#include <hip/hip_fp16.h>
#include "cgs_internal.h"

#define RB_THREADS 256
#define RB_ALPHA_MIN (1.0f / 255.0f)
#define RB_T_EPS 0.0001f
#define RB_INV_LOG2E 0.6931471805599453f
#define RB_NGRAD 9


namespace {

struct RbEval { float dx, dy, g, alpha; bool hit; };

__device__ __forceinline__ RbEval rb_eval(const float4 r0, const float4 r1, float pxf, float pyf) {
    RbEval e;
    e.dx = r0.x - pxf;
    e.dy = r0.y - pyf;
    const float p2 = fmaf(r0.z * e.dx, e.dx, fmaf(r1.x * e.dy, e.dy, (r0.w * e.dx) * e.dy));
    e.g = __builtin_amdgcn_exp2f(p2);
    e.alpha = fminf(0.99f, r1.y * e.g);
    e.hit = (p2 <= 0.f) && (e.alpha >= RB_ALPHA_MIN);
    return e;
}

// 16-bit mask of the 4x4-pixel blocks (row-major 4x4 grid of the 16x16 tile) the alpha >= 1/255 ellipse can reach: its
// bounding box (hx, hy) AND its extents along the two diagonals (`diag` = two fp16 halves: half extent of x + y, of x - y,
// from the preprocess kernel) — an octagon around the ellipse.  Output-invariant: a culled block has no pixel the blend loop
// would not skip anyway; on the bench scene the diagonals drop 10 % of the box test's block visits
// (tools/blend_occupancy.py: 25.4 M -> 22.8 M, 21.8 M have a contributing pixel).
__device__ __forceinline__ uint32_t rb_block_mask(float gx, float gy, float hx, float hy, float diag, int tile_px0,
                                                  int tile_py0) {
    // everything relative to the tile's first pixel: the block bounds are literals (no per-tile registers kept live
    // across the batch loop — 28 of them cost the forward kernel half its occupancy when they were hoisted)
    const float rx = gx - (float)tile_px0, ry = gy - (float)tile_py0;
    const float xl = rx - hx, xh = rx + hx, yl = ry - hy, yh = ry + hy;
    uint32_t xm = 0, ym = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xm |= ((xl <= (float)(4 * k + 3)) && (xh >= (float)(4 * k))) ? (1u << k) : 0u;
        ym |= ((yl <= (float)(4 * k + 3)) && (yh >= (float)(4 * k))) ? (1u << k) : 0u;
    }
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= ((ym >> k) & 1u) ? (xm << (4 * k)) : 0u;
    const uint32_t db = __float_as_uint(diag);
    const float hu = __half2float(__ushort_as_half((unsigned short)(db & 0xFFFFu)));
    const float hv = __half2float(__ushort_as_half((unsigned short)(db >> 16)));
    const float ul = rx + ry - hu, uh = rx + ry + hu, vl = rx - ry - hv, vh = rx - ry + hv;
    // blocks with bx + by = s share the range [4 s, 4 s + 6] of x + y; blocks with bx - by = d the range
    // [4 d - 3, 4 d + 3] of x - y (bit index of a block = 4 by + bx)
    const uint32_t DU[7] = {0x0001u, 0x0012u, 0x0124u, 0x1248u, 0x2480u, 0x4800u, 0x8000u};
    const uint32_t DV[7] = {0x1000u, 0x2100u, 0x4210u, 0x8421u, 0x0842u, 0x0084u, 0x0008u};
    uint32_t um = 0, vm = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        um |= ((ul <= (float)(4 * s + 6)) && (uh >= (float)(4 * s))) ? DU[s] : 0u;
        vm |= ((vl <= (float)(4 * (s - 3) + 3)) && (vh >= (float)(4 * (s - 3) - 3))) ? DV[s] : 0u;
    }
    return m & um & vm;
}

// ballot of a bool (HIP's __ballot takes an int: a v_cndmask + v_cmp_ne pair per call)
__device__ __forceinline__ uint64_t rb_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

template <int CTRL>
__device__ __forceinline__ float rb_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

struct RbLane {
    int px, py, blk;
};

// Workgroup b takes entry b of the tile order.  Runs of 4 / 8 / 16 consecutive entries per XCD (neighbouring tiles read the same
// Gaussians' records, and workgroups go to the eight XCDs' L2s round robin) measured nothing outside the noise
// (profiles/r06_xcd_gathers.txt).

// lane -> pixel: wave = quadrant, row (lane >> 4) = 4x4 block of the quadrant, lane & 15 = pixel of the block
__device__ __forceinline__ RbLane rb_lane(int tx, int ty, int wave, int lane) {
    const int row = lane >> 4, i = lane & 15;
    const int bx = (wave & 1) * 2 + (row & 1), by = (wave >> 1) * 2 + (row >> 1);
    RbLane l;
    l.px = tx * CGS_TILE + bx * 4 + (i & 3);
    l.py = ty * CGS_TILE + by * 4 + (i >> 2);
    l.blk = by * 4 + bx;
    return l;
}

}  // namespace

// Per-block entry lists of one staged batch.  Every staging thread owns one entry of the batch and publishes a 16-bit mask
// of the 4x4 blocks its octagon reaches (smask).  After the staging barrier every ROW builds the list of ITS OWN block: lane
// j of the row takes entries 16 j .. 16 j + 15 (two 16-byte LDS reads), extracts its block's bit from each mask, an
// exclusive scan over the row's sixteen counts (four DPP steps) gives it the slot of its first entry, and it stores the
// batch indices of its entries in ascending order.  The list is written and read by the same wave: no workgroup barrier, no
// atomics.  A row then walks its list with its own cursor — no bit scan, and no waiting for the other rows of the wave at
// 32-entry segment boundaries as the mask walk had (tools/rb_iters.py: 6.45 M -> 5.28 M backward wave iterations per view).
struct RbLists {
    uint8_t list[16][RB_THREADS];       // [block][k] = batch index of the block's k-th entry (ascending)
    uint16_t smask[RB_THREADS];         // block mask of every entry of the batch
};

template <int CTRL>
__device__ __forceinline__ uint32_t rb_dpp_u(uint32_t v) {      // bound_ctrl: lanes shifted in from outside the row read 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// returns the number of entries of the row's block; `lim` = highest admissible batch index for this block (>= 255: all)
__device__ __forceinline__ uint32_t rb_list_build(RbLists &S, int blk, int lane, int lim) {
    const int sub = lane & 15;
    const uint4 w0 = ((const uint4 *)S.smask)[sub * 2], w1 = ((const uint4 *)S.smask)[sub * 2 + 1];
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) bits |= ((w[k >> 1] >> (blk + 16 * (k & 1))) & 1u) << k;
    const int l = lim - 16 * sub;                                 // highest admissible k of this lane
    bits = l < 0 ? 0u : (l >= 15 ? bits : (bits & ((2u << l) - 1u)));
    const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
    uint32_t inc = cnt;
    inc += rb_dpp_u<0x111>(inc);      // row_shr:1
    inc += rb_dpp_u<0x112>(inc);      // row_shr:2
    inc += rb_dpp_u<0x114>(inc);      // row_shr:4
    inc += rb_dpp_u<0x118>(inc);      // row_shr:8
    uint32_t slot = inc - cnt;
    while (bits) {
        const int k = __builtin_ctz(bits);
        bits &= bits - 1u;
        S.list[blk][slot++] = (uint8_t)(16 * sub + k);
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, lane | 15, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the row's own stores are visible to its loads below
    __builtin_amdgcn_wave_barrier();
    return total;
}

__global__ void __launch_bounds__(RB_THREADS)
    blend_fwd_rows_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges,
                          const uint32_t *__restrict__ gid_sorted, const float4 *__restrict__ rec,
                          const float *__restrict__ bg, float *__restrict__ out_color, float *__restrict__ final_T,
                          uint32_t *__restrict__ n_contrib, uint32_t *__restrict__ tile_last,
                          const uint32_t *__restrict__ tile_order) {
    __shared__ float4 srec[RB_THREADS * 3];
    __shared__ RbLists S;
    __shared__ uint32_t wave_last[4];

    const int tile = (int)tile_order[blockIdx.x];        // longest lists first (tile_order_kernel)
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RbLane L = rb_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    float pxf = (float)L.px, pyf = (float)L.py;
    asm volatile("" : "+v"(pxf), "+v"(pyf));      // keep the converted coordinates in registers (the compiler re-converts per iteration)
    const uint2 range = ranges[tile];

    float T = 1.f, cr = 0.f, cg = 0.f, cb = 0.f;
    uint32_t last = 0;
    bool done = !inside;

    // The batch after the one being walked is fetched into registers BEFORE the walk starts (gid -> three dependent
    // 16-byte gathers, ~2 us of latency per batch) and handed to LDS at the top of the next round.
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    bool pvalid = range.x + tid < range.y;
    if (pvalid) {
        const uint32_t g = gid_sorted[range.x + tid];
        p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
    }
    for (uint32_t start = range.x; start < range.y; start += RB_THREADS) {
        if (__syncthreads_count(done) == RB_THREADS) break;      // (also: the previous walk is over, LDS may be rewritten)
        uint32_t m16 = 0;
        if (pvalid) {
            srec[tid * 3] = p0;
            srec[tid * 3 + 1] = p1;
            srec[tid * 3 + 2] = p2;
            m16 = rb_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
        } else {
            // a lane without an entry blends record `e` of a stale list slot with weight 0: the record must be finite
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            srec[tid * 3] = z; srec[tid * 3 + 1] = z; srec[tid * 3 + 2] = z;
        }
        {
            const uint32_t i = start + RB_THREADS + tid;
            pvalid = i < range.y;
            if (pvalid) {
                const uint32_t g = gid_sorted[i];
                p0 = rec[3 * (size_t)g]; p1 = rec[3 * (size_t)g + 1]; p2 = rec[3 * (size_t)g + 2];
            }
        }
        S.smask[tid] = (uint16_t)m16;
        __syncthreads();
        const uint32_t base_pos = start - range.x;
        if (rb_ballot(!done) != 0ull) {
            const uint32_t cnt = rb_list_build(S, L.blk, lane, RB_THREADS);
            uint32_t i = 0, lastb = 0;             // lastb: batch index + 1 of the pixel's last contribution in this batch
            uint32_t e_next = S.list[L.blk][0];
            // every lane of a row advances i together (also the lanes whose pixel is finished); the wave leaves when no
            // unfinished pixel has entries left
            while (rb_ballot(!done && i < cnt) != 0ull) {
                const bool has = i < cnt;
                const uint32_t e = e_next;
                i += has ? 1u : 0u;
                e_next = S.list[L.blk][i & (RB_THREADS - 1)];       // next entry's index: in flight during this iteration
                const float4 r0 = srec[e * 3], r1 = srec[e * 3 + 1];
                const float blue = srec[e * 3 + 2].x;
                const RbEval ev = rb_eval(r0, r1, pxf, pyf);
                // branch-free (as in the backward): a lane that takes no contribution blends weight 0, an exact no-op
                const bool act = has && !done && ev.hit;
                const float alpha = act ? ev.alpha : 0.f;
                const float test_T = T * (1.f - alpha);
                const bool stop = act && test_T < RB_T_EPS;
                const bool upd = act && !stop;
                const float w = upd ? alpha * T : 0.f;
                cr = fmaf(r1.z, w, cr);
                cg = fmaf(r1.w, w, cg);
                cb = fmaf(blue, w, cb);
                T = upd ? test_T : T;
                lastb = upd ? e + 1u : lastb;
                done = done || stop;
            }
            last = lastb ? base_pos + lastb : last;
        }
    }
    if (inside) {
        const size_t pix = (size_t)L.py * W + L.px;
        const size_t hw = (size_t)H * W;
        final_T[pix] = T;
        n_contrib[pix] = last;
        out_color[pix] = fmaf(T, bg[0], cr);
        out_color[hw + pix] = fmaf(T, bg[1], cg);
        out_color[2 * hw + pix] = fmaf(T, bg[2], cb);
    }
    uint32_t wl = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wl = max(wl, (uint32_t)__shfl_xor((int)wl, d, 64));
    if (lane == 0) wave_last[wave] = wl;
    __syncthreads();
    if (tid == 0) tile_last[tile] = max(max(wave_last[0], wave_last[1]), max(wave_last[2], wave_last[3]));
}

// ABS: the opt-in instance of cgs_raster_backward_abs.  Besides everything the default instance sums it accumulates, per
// Gaussian, sum_p |dL_p/d(pixel mean x)| and sum_p |dL_p/d(pixel mean y)| over the same (pixel, Gaussian) visits with the
// same alphas (AbsGS's densification statistic) into dL_dabs_px [P, 2]: two more values per visit in the free places of the
// reduction's third group, two more accumulator columns (11 x 256 floats: 24.6 KB of LDS, six workgroups per CU).  The default
// instance never reads dL_dabs_px.
//
// DET: the opt-in instance of cgs_raster_backward_det (blend_bwd_rows_det_kernel below): the same walk and the same per-visit
// arithmetic, but no sum whose order depends on timing.
//   Inside the tile: one accumulator plane per WAVE, sacc[wave][entry][k] (4 x 256 x NG floats: 36.9 / 45.1 KB; with the records
//   and the lists 50.7 / 58.9 KB of LDS, three / two workgroups per CU).  A wave's iterations run in the order of its rows' lists
//   (a function of the masks, n_contrib and the list alone), and inside an iteration rows 0, 1, 2, 3 add IN TURN with plain LDS
//   read-add-writes, each behind a wave-scope fence + wave_barrier (two rows often hold the same entry: the next row's read must
//   see the previous row's write, and the compiler must not merge the four predicated blocks).  No other wave touches the plane.
//   The flush adds planes 0, 1, 2, 3 in that order.
//   Across tiles: the flush STORES the entry's converted sums (12 floats: mean x, y | conic a, b, c | opacity | r, g, b | abs x,
//   y | spare) into slot(g, tile) = base[g] + (ty - y0_g) (x1_g - x0_g) + (tx - x0_g) of `slots`, exactly one writer per slot;
//   det_sum_kernel adds a Gaussian's slots in an order that depends on tiles[g] alone.  Slots nobody writes (entries behind
//   tile_last, all-zero sums, occluded Gaussians) keep the zeros of the caller's fill.
template <bool ABS>
__global__ void __launch_bounds__(RB_THREADS)
    blend_bwd_rows_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges,
                          const uint32_t *__restrict__ gid_sorted, const float4 *__restrict__ rec,
                          const float *__restrict__ bg, const float *__restrict__ final_T,
                          const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                          const float *__restrict__ dL_dout, float *__restrict__ dL_dmean2D_px,
                          float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity,
                          float *__restrict__ dL_dcolors, const uint32_t *__restrict__ tile_order,
                          float *__restrict__ dL_dabs_px) {
    constexpr bool DET = false;
    const uint2 *const rect = nullptr;             // (the DET instances' arguments: named in discarded statements only)
    const uint32_t *const slot_base = nullptr;
    float4 *const slots = nullptr;
    const uint64_t slot_cap = 0;
#include "raster_blend_rows_bwd.h"
}

// The DET instances (comment above blend_bwd_rows_kernel): nothing is added to global memory, every entry's sums are stored
// to the slot of its (Gaussian, tile) pair.
template <bool ABS>
__global__ void __launch_bounds__(RB_THREADS)
    blend_bwd_rows_det_kernel(int W, int H, int tiles_x, const uint2 *__restrict__ ranges,
                              const uint32_t *__restrict__ gid_sorted, const float4 *__restrict__ rec,
                              const float *__restrict__ bg, const float *__restrict__ final_T,
                              const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ tile_last,
                              const float *__restrict__ dL_dout, const uint32_t *__restrict__ tile_order,
                              const uint2 *__restrict__ rect, const uint32_t *__restrict__ slot_base,
                              float4 *__restrict__ slots, uint64_t slot_cap) {
    constexpr bool DET = true;
    float *const dL_dmean2D_px = nullptr, *const dL_dconic = nullptr, *const dL_dopacity = nullptr, *const dL_dcolors = nullptr,
                 *const dL_dabs_px = nullptr;      // (the default instances' arguments: named in discarded statements only)
#include "raster_blend_rows_bwd.h"
}

// Per-Gaussian sum of the DET instances' slots: Gaussian g owns slots base[g] .. base[g] + tiles[g] - 1 (its rectangle, row-major)
// and every output row is WRITTEN (exact zeros for a Gaussian without tiles; dL/dz of the map blends, which this mode does not
// run, is written zero too so that the camera backward reads a defined scratch).  Order of the additions, a function of tiles[g]
// alone: up to DS_SMALL slots, one thread adds them in ascending order (the headline view: 1.2 slots per Gaussian); above, the
// 64 lanes of the Gaussian's wave add slots lane, lane + 64, ... in ascending order each and the 64 partial sums meet in the xor
// butterfly 32, 16, .., 1 (a + b = b + a bit for bit, so every lane holds the same sum) - a screen-filling Gaussian's thousands
// of slots are read as contiguous 3 KB lines by the wave.
#define DS_SMALL 32u
template <bool ABS>
__global__ void __launch_bounds__(256)
    det_sum_kernel(int64_t P, const uint32_t *__restrict__ tiles, const uint32_t *__restrict__ slot_base,
                   const float4 *__restrict__ slots, uint64_t slot_cap, float *__restrict__ dL_dmean2D_px,
                   float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity, float *__restrict__ dL_dcolors,
                   float *__restrict__ dL_dz, float *__restrict__ dL_dabs_px) {
    constexpr int NV = ABS ? 11 : 9;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t n = 0, b = 0;
    if (g < P) { n = tiles[g]; b = slot_base[g]; }
    // (never with the view's own counts and a capacity >= its pair count: no read past the slot array whatever the inputs)
    if ((uint64_t)b + n > slot_cap) n = (uint64_t)b < slot_cap ? (uint32_t)(slot_cap - b) : 0u;
    float a[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = 0.f;
    const bool big = n > DS_SMALL;
    if (!big)
        for (uint32_t j = 0; j < n; ++j) {
            const float4 *const s = slots + 3 * ((uint64_t)b + j);
            const float4 s0 = s[0], s1 = s[1], s2 = s[2];
            a[0] += s0.x; a[1] += s0.y; a[2] += s0.z; a[3] += s0.w; a[4] += s1.x; a[5] += s1.y; a[6] += s1.z; a[7] += s1.w;
            a[8] += s2.x;
            if constexpr (ABS) { a[9] += s2.y; a[10] += s2.z; }
        }
    uint64_t todo = rb_ballot(big);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint32_t nn = (uint32_t)__shfl((int)n, src, 64), bb = (uint32_t)__shfl((int)b, src, 64);
        float p[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = 0.f;
        for (uint32_t j = (uint32_t)lane; j < nn; j += 64u) {
            const float4 *const s = slots + 3 * ((uint64_t)bb + j);
            const float4 s0 = s[0], s1 = s[1], s2 = s[2];
            p[0] += s0.x; p[1] += s0.y; p[2] += s0.z; p[3] += s0.w; p[4] += s1.x; p[5] += s1.y; p[6] += s1.z; p[7] += s1.w;
            p[8] += s2.x;
            if constexpr (ABS) { p[9] += s2.y; p[10] += s2.z; }
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) p[k] += __shfl_xor(p[k], d, 64);
            a[k] = lane == src ? p[k] : a[k];
        }
    }
    if (g >= P) return;
    dL_dmean2D_px[2 * g] = a[0]; dL_dmean2D_px[2 * g + 1] = a[1];
    dL_dconic[3 * g] = a[2]; dL_dconic[3 * g + 1] = a[3]; dL_dconic[3 * g + 2] = a[4];
    dL_dopacity[g] = a[5];
    dL_dcolors[3 * g] = a[6]; dL_dcolors[3 * g + 1] = a[7]; dL_dcolors[3 * g + 2] = a[8];
    dL_dz[g] = 0.f;
    if constexpr (ABS) { dL_dabs_px[2 * g] = a[9]; dL_dabs_px[2 * g + 1] = a[10]; }
}



// Workgroup -> tile map of the blend kernels: tiles in descending order of their list length CLASS (octaves), raster order
// inside a class.  A view's tiles differ by two orders of magnitude in work and the hardware starts workgroups in index order:
// with tile = workgroup id the last wave of workgroups holds whatever tiles the raster order put last, and the kernel ends when
// the longest of them does; longest first, the tail is made of the shortest lists (LPT scheduling): blend forward 452 -> 401 us,
// backward 958 -> 901 us on the headline scene (same box, profiles/r06_tile_order.txt).  Raster order inside a class keeps
// neighbouring tiles — which read the same Gaussians' records — running together: with an arbitrary order inside
// quarter-octave classes the heavy-pair scene LOST 2 % of its step.  One workgroup: a stable counting sort, thread t owns
// a contiguous run of tiles and one counter per class ([class][thread] in LDS, scanned in that order).  Deterministic.
#define TO_CLASSES 16
#define TO_THREADS 1024
#ifndef TO_DENSE
#define TO_DENSE 4096u      // mean list length above which a view keeps the raster order
#endif
#ifndef TO_TOP
#define TO_TOP 13            // lists of >= 2^(TO_TOP - 1) = 4096 entries share the top class (see below)
#endif
// 0: empty; class c >= 1: [2^(c-1), 2^c) entries; everything from 4096 entries on is ONE class: such lists saturate their pixels
// long before their end, their length says nothing about their work, and sorting them by it only takes neighbouring tiles apart
// (the heavy-pair scene — every list 16 k entries, a few hundred walked — lost 12-18 % of its blend kernels to that).
__device__ __forceinline__ int to_class(uint32_t len) {
    if (len == 0) return 0;
    const int c = 32 - __clz(len);
    return c < TO_TOP ? c : TO_TOP;
}
__global__ void __launch_bounds__(TO_THREADS) tile_order_kernel(int nt, const uint2 *__restrict__ ranges, uint32_t *__restrict__ order) {
    __shared__ uint32_t cnt[TO_CLASSES][TO_THREADS];       // 64 KB
    __shared__ uint32_t wsum[TO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (nt + TO_THREADS - 1) / TO_THREADS;
    const int t0 = tid * per, t1 = min(nt, t0 + per);
#pragma unroll
    for (int c = 0; c < TO_CLASSES; ++c) cnt[c][tid] = 0;
    uint32_t total = 0;
    for (int t = t0; t < t1; ++t) {
        const uint2 r = ranges[t];
        const uint32_t len = r.y > r.x ? r.y - r.x : 0u;
        total += len >> 4;                                        // (in units of 16 entries: no overflow at 2^32 pairs)
        cnt[to_class(len)][tid] += 1;
    }
    // A view of LONG lists (mean above TO_DENSE entries per tile: the heavy-pair scene has 16 k) keeps the raster order: its
    // tiles saturate after a few hundred entries whatever their length, there is no tail to cut, and running the densest tiles
    // together costs the blend kernels 12-18 % (they stream their long lists through the same L2s at the same time, where the
    // raster order mixes them with light tiles) — measured on both scenes, profiles/r06_tile_order.txt.
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) total += __shfl_xor(total, o, 64);
    if (lane == 0) wsum[wave] = total;
    __syncthreads();
    total = 0;
    for (int w = 0; w < TO_THREADS / 64; ++w) total += wsum[w];
    __syncthreads();
    if ((uint64_t)total * 16u > (uint64_t)nt * TO_DENSE) {
        for (int t = t0; t < t1; ++t) order[t] = (uint32_t)t;
        return;
    }
    // exclusive scan of the flat array in (class DESCENDING, thread ascending) order: thread j owns flat entries 16 j .. 16 j + 15
    uint32_t v[TO_CLASSES], mine = 0;
#pragma unroll
    for (int k = 0; k < TO_CLASSES; ++k) {
        const int f = tid * TO_CLASSES + k;                    // flat index: class = 15 - f / 1024, thread = f % 1024
        v[k] = cnt[TO_CLASSES - 1 - f / TO_THREADS][f % TO_THREADS];
        mine += v[k];
    }
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - mine;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TO_CLASSES; ++k) {
        const int f = tid * TO_CLASSES + k;
        cnt[TO_CLASSES - 1 - f / TO_THREADS][f % TO_THREADS] = run;
        run += v[k];
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const uint2 r = ranges[t];
        const int c = to_class(r.y > r.x ? r.y - r.x : 0u);
        order[cnt[c][tid]++] = (uint32_t)t;
    }
}

int cgs_launch_tile_order(const cgs_raster_cfg *cfg, CgsImg &im, hipStream_t stream) {
    const int nt = cgs_tiles_x(cfg) * cgs_tiles_y(cfg);
    hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(TO_THREADS), 0, stream, nt, (const uint2 *)im.ranges, im.tile_order);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

int cgs_launch_blend_fwd_rows(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, float *out_color,
                              hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    hipLaunchKernelGGL(blend_fwd_rows_kernel, dim3((unsigned)(tx * ty)), dim3(RB_THREADS), 0, stream, cfg->image_width,
                       cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted,
                       (const float4 *)g.rec, cfg->bg, out_color, im.final_T, im.n_contrib, im.tile_last,
                       (const uint32_t *)im.tile_order);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

// dL_dabs_px != NULL: the ABS instance, which also adds into dL_dabs_px [P, 2]
int cgs_launch_blend_bwd_rows(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *dL_dout,
                              float *dL_dmean2D_px, float *dL_dconic, float *dL_dopacity, float *dL_dcolors,
                              hipStream_t stream, float *dL_dabs_px) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    const float4 *rec = (const float4 *)g.rec;
    if (dL_dabs_px)
        hipLaunchKernelGGL(blend_bwd_rows_kernel<true>, dim3((unsigned)(tx * ty)), dim3(RB_THREADS), 0, stream, cfg->image_width,
                           cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, rec,
                           cfg->bg, (const float *)im.final_T, (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last,
                           dL_dout, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dcolors, (const uint32_t *)im.tile_order,
                           dL_dabs_px);
    else
        hipLaunchKernelGGL(blend_bwd_rows_kernel<false>, dim3((unsigned)(tx * ty)), dim3(RB_THREADS), 0, stream, cfg->image_width,
                           cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted, rec,
                           cfg->bg, (const float *)im.final_T, (const uint32_t *)im.n_contrib, (const uint32_t *)im.tile_last,
                           dL_dout, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dcolors, (const uint32_t *)im.tile_order,
                           dL_dabs_px);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}

// The blend backward of cgs_raster_backward_det: zero fill of the slot array, the DET instance, the per-Gaussian sum.  slot_base:
// the exclusive scan of g.tiles in id order (the caller's); slot_cap: slots the array holds (>= the view's pair count); R == 0
// or no upstream gradient: only the sum kernel runs, over no slots (every row zero).  dL_dabs_px != NULL: the ABS instances.
int cgs_launch_blend_bwd_rows_det(const cgs_raster_cfg *cfg, int64_t P, int64_t R, CgsGeom &g, CgsBin &b, CgsImg &im,
                                  const float *dL_dout, const uint32_t *slot_base, void *slots, float *dL_dmean2D_px,
                                  float *dL_dconic, float *dL_dopacity, float *dL_dcolors, float *dL_dz, float *dL_dabs_px,
                                  hipStream_t stream) {
    const int tx = cgs_tiles_x(cfg), ty = cgs_tiles_y(cfg);
    const bool blend = R > 0 && dL_dout;
    const uint64_t cap = blend ? (uint64_t)R : 0ull;
    if (blend) {
        CGS_CHECK_HIP(hipMemsetAsync(slots, 0, (size_t)R * 48u, stream));
        if (dL_dabs_px)
            hipLaunchKernelGGL(blend_bwd_rows_det_kernel<true>, dim3((unsigned)(tx * ty)), dim3(RB_THREADS), 0, stream,
                               cfg->image_width, cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted,
                               (const float4 *)g.rec, cfg->bg, (const float *)im.final_T, (const uint32_t *)im.n_contrib,
                               (const uint32_t *)im.tile_last, dL_dout, (const uint32_t *)im.tile_order, (const uint2 *)g.rect,
                               slot_base, (float4 *)slots, cap);
        else
            hipLaunchKernelGGL(blend_bwd_rows_det_kernel<false>, dim3((unsigned)(tx * ty)), dim3(RB_THREADS), 0, stream,
                               cfg->image_width, cfg->image_height, tx, (const uint2 *)im.ranges, (const uint32_t *)b.gid_sorted,
                               (const float4 *)g.rec, cfg->bg, (const float *)im.final_T, (const uint32_t *)im.n_contrib,
                               (const uint32_t *)im.tile_last, dL_dout, (const uint32_t *)im.tile_order, (const uint2 *)g.rect,
                               slot_base, (float4 *)slots, cap);
        CGS_CHECK_LAUNCH(stream, cfg->debug);
    }
    const dim3 grid((unsigned)((P + 255) / 256));
    if (dL_dabs_px)
        hipLaunchKernelGGL(det_sum_kernel<true>, grid, dim3(256), 0, stream, P, (const uint32_t *)g.tiles, slot_base,
                           (const float4 *)slots, cap, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dcolors, dL_dz, dL_dabs_px);
    else
        hipLaunchKernelGGL(det_sum_kernel<false>, grid, dim3(256), 0, stream, P, (const uint32_t *)g.tiles, slot_base,
                           (const float4 *)slots, cap, dL_dmean2D_px, dL_dconic, dL_dopacity, dL_dcolors, dL_dz, dL_dabs_px);
    CGS_CHECK_LAUNCH(stream, cfg->debug);
    return CGS_OK;
}
