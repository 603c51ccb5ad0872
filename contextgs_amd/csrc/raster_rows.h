// Device helpers of the row-mapped tile walks that run behind the colour pass (raster_aux.hip, raster_feat.hip,
// raster_contrib.hip): the colour blend's alpha, the octagon block culling, the per-row entry lists and the lane -> pixel map;
// and, written once for the kernels that use them, the row reductions (ax_row_reduce, ax_row_transpose_sum) and the flush of
// the backward kernels' geometry sums (ax_flush_geom).  raster_blend_rows.hip stays byte-identical (hipcc's output for it moved
// when shared code was factored out of it), so what it defines as rb_* is restated here under ax_* names.
#pragma once
#include <hip/hip_fp16.h>
#include "cgs_internal.h"

#define AX_THREADS 256
#define AX_ALPHA_MIN (1.0f / 255.0f)
#define AX_INV_LOG2E 0.6931471805599453f

namespace {

struct AxEval { float dx, dy, g, alpha; bool hit; };

// = rb_eval (raster_blend_rows.hip): the colour blend's alpha, instruction for instruction
__device__ __forceinline__ AxEval ax_eval(const float4 r0, const float4 r1, float pxf, float pyf) {
    AxEval e;
    e.dx = r0.x - pxf;
    e.dy = r0.y - pyf;
    const float p2 = fmaf(r0.z * e.dx, e.dx, fmaf(r1.x * e.dy, e.dy, (r0.w * e.dx) * e.dy));
    e.g = __builtin_amdgcn_exp2f(p2);
    e.alpha = fminf(0.99f, r1.y * e.g);
    e.hit = (p2 <= 0.f) && (e.alpha >= AX_ALPHA_MIN);
    return e;
}

// = rb_block_mask: the 4x4-pixel blocks of the tile that the alpha >= 1/255 octagon of a record reaches
__device__ __forceinline__ uint32_t ax_block_mask(float gx, float gy, float hx, float hy, float diag, int tile_px0,
                                                  int tile_py0) {
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

__device__ __forceinline__ uint64_t ax_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

template <int CTRL>
__device__ __forceinline__ float ax_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t ax_dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

struct AxLane { int px, py, blk; };

// = rb_lane: wave = 8x8 quadrant of the tile, row (lane >> 4) = 4x4 block of the quadrant, lane & 15 = pixel of the block
__device__ __forceinline__ AxLane ax_lane(int tx, int ty, int wave, int lane) {
    const int row = lane >> 4, i = lane & 15;
    const int bx = (wave & 1) * 2 + (row & 1), by = (wave >> 1) * 2 + (row >> 1);
    AxLane l;
    l.px = tx * CGS_TILE + bx * 4 + (i & 3);
    l.py = ty * CGS_TILE + by * 4 + (i >> 2);
    l.blk = by * 4 + bx;
    return l;
}

struct AxLists {
    uint8_t list[16][AX_THREADS];       // [block][k] = batch index of the block's k-th entry (ascending)
    uint16_t smask[AX_THREADS];         // block mask of every entry of the batch
};

// = rb_list_build: the row's list of the batch entries its block takes, batch index <= lim; returns its length
__device__ __forceinline__ uint32_t ax_list_build(AxLists &S, int blk, int lane, int lim) {
    const int sub = lane & 15;
    const uint4 w0 = ((const uint4 *)S.smask)[sub * 2], w1 = ((const uint4 *)S.smask)[sub * 2 + 1];
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) bits |= ((w[k >> 1] >> (blk + 16 * (k & 1))) & 1u) << k;
    const int l = lim - 16 * sub;
    bits = l < 0 ? 0u : (l >= 15 ? bits : (bits & ((2u << l) - 1u)));
    const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
    uint32_t inc = cnt;
    inc += ax_dpp_u<0x111>(inc);
    inc += ax_dpp_u<0x112>(inc);
    inc += ax_dpp_u<0x114>(inc);
    inc += ax_dpp_u<0x118>(inc);
    uint32_t slot = inc - cnt;
    while (bits) {
        const int k = __builtin_ctz(bits);
        bits &= bits - 1u;
        S.list[blk][slot++] = (uint8_t)(16 * sub + k);
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, lane | 15, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return total;
}

// op over the 16 lanes of a row, in every lane of the row (quad swaps, then row rotations by 4 and 8); V = float or uint32_t
template <int CTRL, class V>
__device__ __forceinline__ V ax_row_move(V v) {
    if constexpr (sizeof(V) == 4 && !__is_same(V, float)) return (V)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
    else return ax_dpp<CTRL>(v);
}
template <class V, class Op>
__device__ __forceinline__ V ax_row_reduce(V v, Op op) {
    v = op(v, ax_row_move<0xB1>(v));
    v = op(v, ax_row_move<0x4E>(v));
    v = op(v, ax_row_move<0x124>(v));
    v = op(v, ax_row_move<0x128>(v));
    return v;
}
__device__ __forceinline__ uint32_t ax_row_max(uint32_t v) {
    return ax_row_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); });
}

// Transposing sum inside each 16-lane row: lane sub = lane & 15 < N of the row returns the row's sum of v[sub] (N = 8 or 16).  Two
// halving exchanges (lane ^ 1, lane ^ 2) leave N / 4 partials per lane, which the two rotations finish.
template <int N>
__device__ __forceinline__ float ax_row_transpose_sum(const float (&v)[N], int lane, int sub) {
    const bool b0 = lane & 1, b1 = lane & 2;
    float a[N / 2], b[N / 4];
#pragma unroll
    for (int q = 0; q < N / 2; ++q) {
        const float keep = b0 ? v[2 * q + 1] : v[2 * q], send = b0 ? v[2 * q] : v[2 * q + 1];
        a[q] = keep + ax_dpp<0xB1>(send);
    }
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
        const float keep = b1 ? a[2 * q + 1] : a[2 * q], send = b1 ? a[2 * q] : a[2 * q + 1];
        b[q] = keep + ax_dpp<0x4E>(send);
    }
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
        b[q] += ax_dpp<0x124>(b[q]);
        b[q] += ax_dpp<0x128>(b[q]);
    }
    if constexpr (N == 8) {
        asm volatile("" : "+v"(b[0]), "+v"(b[1]));
        return sub < 4 ? b[0] : b[1];
    } else {
        asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
        return sub < 8 ? (sub < 4 ? b[0] : b[1]) : (sub < 12 ? b[2] : b[3]);
    }
}

// the flush of an entry's six geometry sums (gx, gy, gx dx, gx dy, gy dy, dL/dG) into the colour pass's accumulators;
// q0, q1 = the entry's staged quads
__device__ __forceinline__ void ax_flush_geom(uint32_t g, const float4 q0, const float4 q1, float a0, float a1, float a2,
                                              float a3, float a4, float a5, float *__restrict__ dL_dmean2D_px,
                                              float *__restrict__ dL_dconic, float *__restrict__ dL_dopacity) {
    const float cC = q1.x, op = q1.y;
    atomicAdd(&dL_dmean2D_px[2 * (size_t)g], op * fmaf(2.f * q0.z, a0, q0.w * a1) * AX_INV_LOG2E);
    atomicAdd(&dL_dmean2D_px[2 * (size_t)g + 1], op * fmaf(2.f * cC, a1, q0.w * a0) * AX_INV_LOG2E);
    atomicAdd(&dL_dconic[3 * (size_t)g], -0.5f * op * a2);
    atomicAdd(&dL_dconic[3 * (size_t)g + 1], -op * a3);
    atomicAdd(&dL_dconic[3 * (size_t)g + 2], -0.5f * op * a4);
    atomicAdd(&dL_dopacity[g], a5);
}

}  // namespace
