// Per-view bilateral grids (contextgs_amd/bilagrid.py; the definition is in include/cgs.h above cgs_bilagrid_slice_fwd).
//
//   slice forward / d image   pixel kernels: a workgroup takes 1024 consecutive pixels of the flattened [H*W] planes (one 16-byte
//                             access per lane, channel and array when H*W is a multiple of 4 and the bases are 16-byte aligned;
//                             a quad may straddle two rows, every pixel has its own (y, x)).  The grid nodes the tile can reach
//                             (all L levels, the y nodes of its rows, the x nodes of its columns) are staged into LDS as
//                             [z][y][x][12], so a corner is three 16-byte LDS reads; a sub-block beyond 48 KiB (grids finer than
//                             the pixels) reads the nodes through the cache instead.
//   d grid                    gx, gy depend on the pixel's position only, so the cell (floor gy, floor gx) owns a pixel rectangle.
//                             One workgroup per (row split, cell, z node): 4 corners x 12 channels in registers per lane, the
//                             z weight of its node per pixel, one fixed-order wave + LDS reduction; a second kernel adds, per
//                             node and in a fixed order, the up-to-four cells around it and the row splits.  No float atomics:
//                             two launches give the same bytes, and every element of dgrid is written.
//   TV                        forward: per-workgroup partial sums, then one workgroup adds them in order; backward: a gather of
//                             each node's up to six neighbours.
#include "cgs_internal.h"

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_PX = 4;                                   // pixels per lane: one 16-byte access per plane
constexpr int BG_TILE = BG_THREADS * BG_PX;
constexpr size_t BG_LDS_MAX = 48 * 1024;
constexpr int BG_TV_MAX_BLOCKS = 1024;

struct BgAxis { int i0, i1; float f; };

__device__ __forceinline__ BgAxis bg_axis(float g, int n) {
    int i0 = (int)floorf(g);
    i0 = min(max(i0, 0), n - 1);
    BgAxis a;
    a.i0 = i0;
    a.i1 = min(i0 + 1, n - 1);
    a.f = g - (float)i0;
    return a;
}
// pixel centre p of n_px pixels on an axis of n_nodes nodes (monotone in p, also after rounding)
__device__ __forceinline__ float bg_coord(int p, int n_px, int n_nodes) {
    return ((float)p + 0.5f) / (float)n_px * (float)(n_nodes - 1);
}
__device__ __forceinline__ float bg_lum(float r, float g, float b) { return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r)); }
__device__ __forceinline__ float bg_gz(float zs, int L) { return fminf(fmaxf(zs, 0.0f), (float)(L - 1)); }

// Where a kernel finds the node (z, y, x): the staged sub-block [z][y - y0][x - x0][12] or the grid itself [12][L][Gh][Gw].
template <bool LDS> struct BgGrid {
    const float *base;
    int L, Gh, Gw, y0, ny, x0, nx;
    size_t plane;
    __device__ __forceinline__ const float *node(int z, int y, int x) const {
        if (LDS) {
            const int yy = min(max(y - y0, 0), ny - 1), xx = min(max(x - x0, 0), nx - 1);
            return base + ((z * ny + yy) * nx + xx) * 12;
        }
        return base + ((size_t)z * Gh + y) * Gw + x;
    }
    __device__ __forceinline__ size_t cs() const { return LDS ? (size_t)1 : plane; }
};

// Stage what the tile [tile0, tile0 + BG_TILE) of flattened pixels can reach.  cap_ny bounds the y nodes the host sized the LDS for.
template <bool LDS>
__device__ __forceinline__ BgGrid<LDS> bg_stage(const float *__restrict__ grid, int L, int Gh, int Gw, int H, int W, uint32_t tile0,
                                                uint32_t npix, int cap_ny, float *lds) {
    BgGrid<LDS> G;
    G.L = L; G.Gh = Gh; G.Gw = Gw;
    G.plane = (size_t)L * Gh * Gw;
    G.y0 = 0; G.ny = Gh; G.x0 = 0; G.nx = Gw;
    if (!LDS) {
        G.base = grid;
        return G;
    }
    const uint32_t last = min(tile0 + (uint32_t)BG_TILE, npix) - 1u;
    const int yf = (int)(tile0 / (uint32_t)W), yl = (int)(last / (uint32_t)W);
    G.y0 = bg_axis(bg_coord(yf, H, Gh), Gh).i0;
    G.ny = min(bg_axis(bg_coord(yl, H, Gh), Gh).i1 - G.y0 + 1, cap_ny);
    if (yf == yl) {
        G.x0 = bg_axis(bg_coord((int)(tile0 - (uint32_t)yf * W), W, Gw), Gw).i0;
        G.nx = bg_axis(bg_coord((int)(last - (uint32_t)yf * W), W, Gw), Gw).i1 - G.x0 + 1;
    }
    const int row = G.nx, slab = G.ny * G.nx, vol = L * slab, total = 12 * vol;
    for (int i = threadIdx.x; i < total; i += BG_THREADS) {          // x fastest: the global reads run along the grid's rows
        const int c = i / vol, r = i - c * vol;
        const int z = r / slab, r2 = r - z * slab;
        const int yy = r2 / row, xx = r2 - yy * row;
        lds[r * 12 + c] = grid[(((size_t)c * L + z) * Gh + (G.y0 + yy)) * Gw + (G.x0 + xx)];
    }
    __syncthreads();
    G.base = lds;
    return G;
}

// A[12] = sum over the 8 corners of wz wy wx G[:, corner]; with DZ also dAdz[12] = sum over the xy corners of wy wx (G[z1] - G[z0]).
template <bool LDS, bool DZ>
__device__ __forceinline__ void bg_affine(const BgGrid<LDS> &G, const BgAxis &ax, const BgAxis &ay, const BgAxis &az, float A[12],
                                          float dAdz[12]) {
#pragma unroll
    for (int c = 0; c < 12; c++) { A[c] = 0.0f; if (DZ) dAdz[c] = 0.0f; }
    const size_t cs = G.cs();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int yc = k >> 1, xc = k & 1;
        const float wxy = (yc ? ay.f : 1.0f - ay.f) * (xc ? ax.f : 1.0f - ax.f);
        const float w0 = (1.0f - az.f) * wxy, w1 = az.f * wxy;
        const int y = yc ? ay.i1 : ay.i0, x = xc ? ax.i1 : ax.i0;
        const float *p0 = G.node(az.i0, y, x), *p1 = G.node(az.i1, y, x);
#pragma unroll
        for (int c = 0; c < 12; c++) {
            const float g0 = p0[c * cs], g1 = p1[c * cs];
            A[c] = fmaf(w1, g1, fmaf(w0, g0, A[c]));
            if (DZ) dAdz[c] = fmaf(wxy, g1 - g0, dAdz[c]);
        }
    }
}

template <bool VEC> __device__ __forceinline__ void bg_load4(const float *__restrict__ plane, uint32_t p0, uint32_t npix, float v[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(plane + p0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (p0 + k < npix) ? plane[p0 + k] : 0.0f;
    }
}
template <bool VEC> __device__ __forceinline__ void bg_store4(float *__restrict__ plane, uint32_t p0, uint32_t npix, const float v[4]) {
    if (VEC) {
        *reinterpret_cast<float4 *>(plane + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (p0 + k < npix) plane[p0 + k] = v[k];
    }
}

// out (DIMG false) or d image (DIMG true, `dout` given) of the tile's pixels
template <bool LDS, bool VEC, bool DIMG>
__global__ void __launch_bounds__(BG_THREADS)             // (asking for four waves per SIMD spills ~400 B per lane and doubles the time)
    bg_pixel_kernel(const float *__restrict__ grid, int L, int Gh, int Gw, const float *__restrict__ img, const float *__restrict__ dout,
                    int H, int W, int cap_ny, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float bg_lds[];
    const uint32_t npix = (uint32_t)H * (uint32_t)W;
    const uint32_t tile0 = blockIdx.x * (uint32_t)BG_TILE;
    const BgGrid<LDS> G = bg_stage<LDS>(grid, L, Gh, Gw, H, W, tile0, npix, cap_ny, bg_lds);
    const uint32_t p0 = tile0 + threadIdx.x * (uint32_t)BG_PX;
    if (p0 >= npix) return;
    float rgb[3][4], go[3][4], res[3][4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        bg_load4<VEC>(img + (size_t)j * npix, p0, npix, rgb[j]);
        if (DIMG) bg_load4<VEC>(dout + (size_t)j * npix, p0, npix, go[j]);
    }
    int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * W);
    const float lm1 = (float)(L - 1);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (p0 + k < npix) {
            const float r = rgb[0][k], g = rgb[1][k], b = rgb[2][k];
            const float zs = bg_lum(r, g, b) * lm1;
            const BgAxis ax = bg_axis(bg_coord(x, W, Gw), Gw), ay = bg_axis(bg_coord(y, H, Gh), Gh), az = bg_axis(bg_gz(zs, L), L);
            float A[12], dAdz[12];
            bg_affine<LDS, DIMG>(G, ax, ay, az, A, dAdz);
            if (!DIMG) {
#pragma unroll
                for (int i = 0; i < 3; i++) res[i][k] = fmaf(A[4 * i + 2], b, fmaf(A[4 * i + 1], g, fmaf(A[4 * i], r, A[4 * i + 3])));
            } else {
                const float g0 = go[0][k], g1 = go[1][k], g2 = go[2][k];
                const float gi[3] = {g0, g1, g2}, px[4] = {r, g, b, 1.0f};
                float s = 0.0f;                                          // sum_c dA_c dAdz_c, dA[4 i + j] = g_i rgb_j
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) s = fmaf(gi[i] * px[j], dAdz[4 * i + j], s);
                const float t = (zs > 0.0f && zs < lm1) ? s * lm1 : 0.0f;   // a clamped guidance passes no gradient
                res[0][k] = fmaf(0.299f, t, fmaf(A[8], g2, fmaf(A[4], g1, A[0] * g0)));
                res[1][k] = fmaf(0.587f, t, fmaf(A[9], g2, fmaf(A[5], g1, A[1] * g0)));
                res[2][k] = fmaf(0.114f, t, fmaf(A[10], g2, fmaf(A[6], g1, A[2] * g0)));
            }
        } else {
            res[0][k] = res[1][k] = res[2][k] = 0.0f;
        }
        if (++x == W) { x = 0; y++; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) bg_store4<VEC>(out + (size_t)j * npix, p0, npix, res[j]);
}

// ---- d grid -----------------------------------------------------------------------------------------------------------------------
// Cells per axis, and a pixel range [lo, hi) that holds every pixel of cell c (the kernel tests each pixel's own cell).
__host__ __device__ inline int bg_cells(int n_nodes) { return n_nodes > 1 ? n_nodes - 1 : 1; }
__device__ __forceinline__ void bg_cell_range(int c, int ncell, int n_px, int n_nodes, int &lo, int &hi) {
    lo = 0; hi = n_px;
    if (n_nodes > 1) {
        if (c > 0) lo = max(0, (int)(((int64_t)c * n_px) / (n_nodes - 1)) - 1);
        if (c < ncell - 1) hi = min(n_px, (int)(((int64_t)(c + 1) * n_px + n_nodes - 2) / (n_nodes - 1)) + 1);
    }
}

// part[((s * ncy + cy) * ncx + cx) * L + l][corner (2 yc + xc)][12]: the sums over the pixels of row split s of cell (cy, cx)
__global__ void __launch_bounds__(BG_THREADS)
    bg_dgrid_cell_kernel(const float *__restrict__ img, const float *__restrict__ dout, int L, int Gh, int Gw, int H, int W, int ncy,
                         int ncx, int S, float *__restrict__ part) {
    __shared__ float red[BG_THREADS / 64][48];
    int b = blockIdx.x;
    const int l = b % L; b /= L;
    const int cx = b % ncx; b /= ncx;
    const int cy = b % ncy;
    const int s = b / ncy;
    int xlo, xhi, ylo, yhi;
    bg_cell_range(cx, ncx, W, Gw, xlo, xhi);
    bg_cell_range(cy, ncy, H, Gh, ylo, yhi);
    const int rs = (yhi - ylo + S - 1) / S;
    const int ya = ylo + s * rs, yb = min(yhi, ya + rs);
    const int nc = xhi - xlo, n = (yb > ya ? yb - ya : 0) * nc;
    const size_t npix = (size_t)H * W;
    const float lm1 = (float)(L - 1);
    float acc[48];
#pragma unroll
    for (int i = 0; i < 48; i++) acc[i] = 0.0f;
    for (int idx = threadIdx.x; idx < n; idx += BG_THREADS) {
        const int ry = idx / nc, y = ya + ry, x = xlo + (idx - ry * nc);
        const BgAxis ax = bg_axis(bg_coord(x, W, Gw), Gw), ay = bg_axis(bg_coord(y, H, Gh), Gh);
        if (min(ax.i0, ncx - 1) != cx || min(ay.i0, ncy - 1) != cy) continue;
        const size_t p = (size_t)y * W + x;
        const float r = img[p], g = img[npix + p], bl = img[2 * npix + p];
        const BgAxis az = bg_axis(bg_gz(bg_lum(r, g, bl) * lm1, L), L);
        const float wz = (az.i0 == l ? 1.0f - az.f : 0.0f) + (az.i1 == l ? az.f : 0.0f);
        if (wz == 0.0f) continue;
        const float gi[3] = {dout[p], dout[npix + p], dout[2 * npix + p]}, px[4] = {r, g, bl, 1.0f};
        float dA[12];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) dA[4 * i + j] = gi[i] * px[j];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float w = wz * ((k >> 1 ? ay.f : 1.0f - ay.f) * (k & 1 ? ax.f : 1.0f - ax.f));
#pragma unroll
            for (int c = 0; c < 12; c++) acc[k * 12 + c] = fmaf(w, dA[c], acc[k * 12 + c]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 48; i++) {
        float v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 48) {
        float v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BG_THREADS / 64; w++) v += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * 48 + threadIdx.x] = v;
    }
}

// dgrid[c, l, y, x] = the cells around node (y, x), their corners that are this node, the row splits: always in this order
__global__ void __launch_bounds__(BG_THREADS)
    bg_dgrid_node_kernel(const float *__restrict__ part, int L, int Gh, int Gw, int ncy, int ncx, int S, float *__restrict__ dgrid) {
    const int total = 12 * L * Gh * Gw;
    const int e = blockIdx.x * BG_THREADS + threadIdx.x;
    if (e >= total) return;
    int r = e;
    const int x = r % Gw; r /= Gw;
    const int y = r % Gh; r /= Gh;
    const int l = r % L;
    const int c = r / L;
    float v = 0.0f;
    for (int cy = max(y - 1, 0); cy <= min(y, ncy - 1); cy++)
        for (int a = 0; a < 2; a++) {
            if ((a ? min(cy + 1, Gh - 1) : cy) != y) continue;
            for (int cx = max(x - 1, 0); cx <= min(x, ncx - 1); cx++)
                for (int bb = 0; bb < 2; bb++) {
                    if ((bb ? min(cx + 1, Gw - 1) : cx) != x) continue;
                    for (int s = 0; s < S; s++)
                        v += part[((((size_t)s * ncy + cy) * ncx + cx) * L + l) * 48 + (a * 2 + bb) * 12 + c];
                }
        }
    dgrid[e] = v;
}

// ---- TV ----------------------------------------------------------------------------------------------------------------------------
struct BgTvScale { float iz, iy, ix; };          // 1 / (differences along the axis in one view); 0 for an axis of length 1
static BgTvScale bg_tv_scale(int L, int Gh, int Gw) {
    BgTvScale s;
    s.iz = L > 1 ? (float)(1.0 / (12.0 * (L - 1) * Gh * Gw)) : 0.0f;
    s.iy = Gh > 1 ? (float)(1.0 / (12.0 * L * (Gh - 1) * Gw)) : 0.0f;
    s.ix = Gw > 1 ? (float)(1.0 / (12.0 * L * Gh * (Gw - 1))) : 0.0f;
    return s;
}

__device__ __forceinline__ float bg_block_sum(float v, float *red) {      // the workgroup's sum, in thread 0, in a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < BG_THREADS / 64; w++) t += red[w];
    return t;
}

__global__ void __launch_bounds__(BG_THREADS)
    bg_tv_fwd_kernel(const float *__restrict__ g, int64_t total, int L, int Gh, int Gw, BgTvScale sc, float *__restrict__ partials) {
    __shared__ float red[BG_THREADS / 64];
    const int64_t sy = Gw, sz = (int64_t)Gh * Gw;
    float acc = 0.0f;
    for (int64_t e = (int64_t)blockIdx.x * BG_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * BG_THREADS) {
        const int x = (int)(e % Gw), y = (int)((e / Gw) % Gh), z = (int)((e / sz) % L);
        const float v = g[e];
        if (x + 1 < Gw) { const float d = g[e + 1] - v; acc = fmaf(d * d, sc.ix, acc); }
        if (y + 1 < Gh) { const float d = g[e + sy] - v; acc = fmaf(d * d, sc.iy, acc); }
        if (z + 1 < L) { const float d = g[e + sz] - v; acc = fmaf(d * d, sc.iz, acc); }
    }
    const float t = bg_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(BG_THREADS) bg_tv_finish_kernel(const float *__restrict__ partials, int nb, float inv_n, float *__restrict__ out1) {
    __shared__ float red[BG_THREADS / 64];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < nb; i += BG_THREADS) acc += partials[i];
    const float t = bg_block_sum(acc, red);
    if (threadIdx.x == 0) out1[0] = t * inv_n;
}

__global__ void __launch_bounds__(BG_THREADS)
    bg_tv_bwd_kernel(const float *__restrict__ g, int64_t total, int L, int Gh, int Gw, BgTvScale sc, float two_over_n,
                     const float *__restrict__ gout, float *__restrict__ dg) {
    const int64_t sy = Gw, sz = (int64_t)Gh * Gw;
    const float k = gout[0] * two_over_n;
    for (int64_t e = (int64_t)blockIdx.x * BG_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * BG_THREADS) {
        const int x = (int)(e % Gw), y = (int)((e / Gw) % Gh), z = (int)((e / sz) % L);
        const float v = g[e];
        float dx = 0.0f, dy = 0.0f, dz = 0.0f;
        if (x > 0) dx += v - g[e - 1];
        if (x + 1 < Gw) dx += v - g[e + 1];
        if (y > 0) dy += v - g[e - sy];
        if (y + 1 < Gh) dy += v - g[e + sy];
        if (z > 0) dz += v - g[e - sz];
        if (z + 1 < L) dz += v - g[e + sz];
        dg[e] = k * fmaf(dz, sc.iz, fmaf(dy, sc.iy, dx * sc.ix));
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
int bg_check_shape(const char *who, int L, int Gh, int Gw, int H, int W) {
    if (L < 1 || Gh < 1 || Gw < 1 || H < 1 || W < 1) {
        cgs_set_error("%s: L, Gh, Gw, H, W must be positive (got %d, %d, %d, %d, %d)", who, L, Gh, Gw, H, W);
        return CGS_ERR_ARG;
    }
    if ((int64_t)H * W > (int64_t)1 << 30 || (int64_t)12 * L * Gh * Gw > (int64_t)1 << 28) {
        cgs_set_error("%s: more than 2^30 pixels or 2^28 grid values", who);
        return CGS_ERR_ARG;
    }
    return CGS_OK;
}

// y nodes a tile of BG_TILE consecutive pixels can reach, and the LDS bytes of its sub-block (all L levels and Gw columns)
size_t bg_stage_bytes(int L, int Gh, int Gw, int H, int W, int *cap_ny) {
    const int64_t rows = (BG_TILE - 1) / W + 2;
    const int64_t ny = (rows - 1) * (Gh - 1) / H + 3;
    *cap_ny = (int)(ny < Gh ? ny : Gh);
    return (size_t)12 * L * (size_t)*cap_ny * Gw * sizeof(float);
}

// row splits of a cell: enough workgroups to fill the chip when the grid is coarse, never less than ~512 pixels each
int bg_splits(int L, int Gh, int Gw, int H, int W) {
    const int64_t ncy = bg_cells(Gh), ncx = bg_cells(Gw);
    const int64_t rows = (H + ncy - 1) / ncy + 2, cols = (W + ncx - 1) / ncx + 2;
    int64_t s = (2048 + ncy * ncx * L - 1) / (ncy * ncx * L);
    const int64_t by_px = rows * cols / 512;
    if (s > by_px) s = by_px;
    if (s > rows) s = rows;
    if (s > 256) s = 256;
    return (int)(s < 1 ? 1 : s);
}

bool bg_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <bool DIMG>
int bg_launch_pixels(const float *grid, int L, int Gh, int Gw, const float *img, const float *dout, int H, int W, float *out, hipStream_t st) {
    int cap_ny = 0;
    const size_t lds = bg_stage_bytes(L, Gh, Gw, H, W, &cap_ny);
    const bool use_lds = lds <= BG_LDS_MAX;
    const int64_t npix = (int64_t)H * W;
    const bool vec = npix % 4 == 0 && bg_aligned16(img) && bg_aligned16(out) && (!DIMG || bg_aligned16(dout));
    const dim3 nb((unsigned)((npix + BG_TILE - 1) / BG_TILE)), th(BG_THREADS);
#define BG_GO(LDSF, VECF) \
    hipLaunchKernelGGL((bg_pixel_kernel<LDSF, VECF, DIMG>), nb, th, (LDSF) ? lds : 0, st, grid, L, Gh, Gw, img, dout, H, W, cap_ny, out)
    if (use_lds) { if (vec) BG_GO(true, true); else BG_GO(true, false); }
    else         { if (vec) BG_GO(false, true); else BG_GO(false, false); }
#undef BG_GO
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}

}  // namespace

extern "C" int cgs_bilagrid_slice_fwd(const float *grid, int L, int Gh, int Gw, const float *img, int H, int W, float *out, void *stream) {
    if (int rc = bg_check_shape("bilagrid_slice_fwd", L, Gh, Gw, H, W)) return rc;
    if (!grid || !img || !out) { cgs_set_error("bilagrid_slice_fwd: NULL grid, img or out"); return CGS_ERR_ARG; }
    return bg_launch_pixels<false>(grid, L, Gh, Gw, img, nullptr, H, W, out, (hipStream_t)stream);
}

extern "C" size_t cgs_bilagrid_bwd_scratch_bytes(int L, int Gh, int Gw, int H, int W) {
    if (L < 1 || Gh < 1 || Gw < 1 || H < 1 || W < 1) return 0;
    return (size_t)bg_splits(L, Gh, Gw, H, W) * bg_cells(Gh) * bg_cells(Gw) * L * 48 * sizeof(float);
}

extern "C" int cgs_bilagrid_slice_bwd(const float *grid, int L, int Gh, int Gw, const float *img, const float *dout, int H, int W,
                                      float *dimg, float *dgrid, void *scratch, size_t scratch_bytes, void *stream) {
    if (int rc = bg_check_shape("bilagrid_slice_bwd", L, Gh, Gw, H, W)) return rc;
    if (!grid || !img || !dout) { cgs_set_error("bilagrid_slice_bwd: NULL grid, img or dout"); return CGS_ERR_ARG; }
    if (!dimg && !dgrid) { cgs_set_error("bilagrid_slice_bwd: neither dimg nor dgrid to write"); return CGS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (dgrid) {
        const size_t need = cgs_bilagrid_bwd_scratch_bytes(L, Gh, Gw, H, W);
        if (!scratch || scratch_bytes < need) {
            cgs_set_error("bilagrid_slice_bwd: dgrid needs %zu bytes of scratch, got %zu", need, scratch ? scratch_bytes : (size_t)0);
            return CGS_ERR_ARG;
        }
    }
    if (dimg)
        if (int rc = bg_launch_pixels<true>(grid, L, Gh, Gw, img, dout, H, W, dimg, st)) return rc;
    if (dgrid) {
        const int ncy = bg_cells(Gh), ncx = bg_cells(Gw), S = bg_splits(L, Gh, Gw, H, W);
        hipLaunchKernelGGL(bg_dgrid_cell_kernel, dim3((unsigned)(S * ncy * ncx * L)), dim3(BG_THREADS), 0, st, img, dout, L, Gh, Gw, H, W,
                           ncy, ncx, S, (float *)scratch);
        CGS_CHECK_LAUNCH(st, false);
        const int total = 12 * L * Gh * Gw;
        hipLaunchKernelGGL(bg_dgrid_node_kernel, dim3((unsigned)((total + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, st,
                           (const float *)scratch, L, Gh, Gw, ncy, ncx, S, dgrid);
        CGS_CHECK_LAUNCH(st, false);
    }
    return CGS_OK;
}

static int bg_tv_blocks(int64_t total) {
    const int64_t nb = (total + 4 * BG_THREADS - 1) / (4 * BG_THREADS);
    return (int)(nb < 1 ? 1 : (nb > BG_TV_MAX_BLOCKS ? BG_TV_MAX_BLOCKS : nb));
}
static int bg_tv_check(const char *who, int N, int L, int Gh, int Gw) {
    if (N < 1 || L < 1 || Gh < 1 || Gw < 1) {
        cgs_set_error("%s: N, L, Gh, Gw must be positive (got %d, %d, %d, %d)", who, N, L, Gh, Gw);
        return CGS_ERR_ARG;
    }
    if ((int64_t)12 * L * Gh * Gw > (int64_t)1 << 28) { cgs_set_error("%s: more than 2^28 grid values per view", who); return CGS_ERR_ARG; }
    return CGS_OK;
}

extern "C" size_t cgs_bilagrid_tv_scratch_bytes(int N, int L, int Gh, int Gw) {
    if (N < 1 || L < 1 || Gh < 1 || Gw < 1) return 0;
    return (size_t)bg_tv_blocks((int64_t)N * 12 * L * Gh * Gw) * sizeof(float);
}

extern "C" int cgs_bilagrid_tv_fwd(const float *grids, int N, int L, int Gh, int Gw, float *out1, void *scratch, void *stream) {
    if (int rc = bg_tv_check("bilagrid_tv_fwd", N, L, Gh, Gw)) return rc;
    if (!grids || !out1 || !scratch) { cgs_set_error("bilagrid_tv_fwd: NULL grids, out1 or scratch"); return CGS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * 12 * L * Gh * Gw;
    const int nb = bg_tv_blocks(total);
    hipLaunchKernelGGL(bg_tv_fwd_kernel, dim3(nb), dim3(BG_THREADS), 0, st, grids, total, L, Gh, Gw, bg_tv_scale(L, Gh, Gw), (float *)scratch);
    CGS_CHECK_LAUNCH(st, false);
    hipLaunchKernelGGL(bg_tv_finish_kernel, dim3(1), dim3(BG_THREADS), 0, st, (const float *)scratch, nb, 1.0f / (float)N, out1);
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}

extern "C" int cgs_bilagrid_tv_bwd(const float *grids, int N, int L, int Gh, int Gw, const float *g, float *dgrids, void *stream) {
    if (int rc = bg_tv_check("bilagrid_tv_bwd", N, L, Gh, Gw)) return rc;
    if (!grids || !g || !dgrids) { cgs_set_error("bilagrid_tv_bwd: NULL grids, g or dgrids"); return CGS_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * 12 * L * Gh * Gw;
    int64_t nb = (total + BG_THREADS - 1) / BG_THREADS;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(bg_tv_bwd_kernel, dim3((unsigned)nb), dim3(BG_THREADS), 0, st, grids, total, L, Gh, Gw, bg_tv_scale(L, Gh, Gw),
                       2.0f / (float)N, g, dgrids);
    CGS_CHECK_LAUNCH(st, false);
    return CGS_OK;
}
