// Anchor position codec (container version 3: anchor.b; format in INTEGRATION.md).
// The quantised grid indices (qx, qy, qz), each in [0, 65535], become 48-bit Morton keys (bit b of qx -> key bit 3b+2,
// qy -> 3b+1, qz -> 3b).  The keys are sorted (stable: two passes of cgs_sort_pairs_u32, low 24 bits then high 24 bits,
// carrying the permutation), cut into blocks of B anchors, and every key but a block's first is sent as the gap d >= 0 to
// its predecessor: the class c = bit length of d (0..48) goes to the lane-parallel table coder (codec.hip), the c - 1 low
// bits of d (the top bit is implied) are bit-packed LSB first, each block's bits starting on a byte boundary.
//   anchor_keys_kernel    q int32 [N,3] -> low / high 24-bit key halves; an index outside [0, 65535] sets *status
//   anchor_pack_kernel    one workgroup per block: gaps, classes (+ histogram), scan of the mantissa lengths, bits
//                         assembled in LDS, flushed with 16-byte stores into the block's worst-case slot
//   anchor_unpack_kernel  one workgroup per block: decoded classes -> scan -> mantissas out of the LDS copy of the block's
//                         bytes -> 64-bit prefix sum of the gaps on the block's first key -> de-interleaved int32 [N,3]
#include "cgs_internal.h"

#define AC_THREADS 256
#define AC_MAX_B 4096                               // anchors per block: 64 .. 4096
#define AC_MAX_CLASS 48
#define AC_PER ((AC_MAX_B + AC_THREADS - 1) / AC_THREADS)
#define AC_LDS_WORDS ((AC_MAX_B * 47 / 8 + 15) / 16 * 4 + 8)   // worst-case block (47 bits per anchor) + a window's overhang

// ---- Morton keys ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ac_spread3(uint32_t v) {          // bit b of a 16-bit value -> bit 3b
    uint64_t x = v & 0xFFFFull;
    x = (x | (x << 16)) & 0x0000FF0000FFull;
    x = (x | (x << 8)) & 0x00F00F00F00Full;
    x = (x | (x << 4)) & 0x0C30C30C30C3ull;
    x = (x | (x << 2)) & 0x249249249249ull;
    return x;
}

__device__ __forceinline__ uint32_t ac_gather3(uint64_t x) {          // inverse of ac_spread3
    x &= 0x249249249249ull;
    x = (x | (x >> 2)) & 0x0C30C30C30C3ull;
    x = (x | (x >> 4)) & 0x00F00F00F00Full;
    x = (x | (x >> 8)) & 0x0000FF0000FFull;
    x = (x | (x >> 16)) & 0xFFFFull;
    return (uint32_t)x;
}

__global__ void __launch_bounds__(AC_THREADS)
    anchor_keys_kernel(const int32_t *__restrict__ q, int64_t n, uint32_t *__restrict__ key_lo, uint32_t *__restrict__ key_hi,
                       int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * AC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    uint64_t key = 0;
    if (((uint32_t)x | (uint32_t)y | (uint32_t)z) > 65535u) atomicMax(status, 1);      // (negative: the sign bit is set)
    else key = (ac_spread3((uint32_t)x) << 2) | (ac_spread3((uint32_t)y) << 1) | ac_spread3((uint32_t)z);
    key_lo[i] = (uint32_t)(key & 0xFFFFFFull);
    key_hi[i] = (uint32_t)(key >> 24);
}

// high halves in the order the first pass left, the operand of the second pass
__global__ void __launch_bounds__(AC_THREADS)
    anchor_gather_hi_kernel(const uint32_t *__restrict__ key_hi, const uint32_t *__restrict__ order, int64_t n,
                            uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * AC_THREADS + threadIdx.x;
    if (i < n) out[i] = key_hi[order[i]];
}

__global__ void __launch_bounds__(AC_THREADS)
    anchor_order_finish_kernel(const uint32_t *__restrict__ key_lo, const uint32_t *__restrict__ hi_sorted,
                               const uint32_t *__restrict__ order, int64_t n, int64_t *__restrict__ order_out,
                               uint64_t *__restrict__ keys_out) {
    const int64_t i = (int64_t)blockIdx.x * AC_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = order[i];
    order_out[i] = (int64_t)o;
    keys_out[i] = ((uint64_t)hi_sorted[i] << 24) | key_lo[o];
}

extern "C" size_t cgs_anchor_order_scratch_bytes(int64_t n) {
    if (n < 1) n = 1;
    // 8 uint32 arrays of n (key halves, gathered high halves, order x2, ping-pong x2, sorted keys) + the sort's scratch
    return (size_t)8 * cgs_align_up((size_t)n * 4, 256) + cgs_sort_scratch_bytes(n) + 1024;
}

extern "C" int cgs_anchor_order(const int32_t *q, int64_t n, int64_t *order, uint64_t *keys_sorted, int32_t *status,
                                void *scratch, size_t scratch_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n >= (1ll << 31)) { cgs_set_error("anchor_order: bad n"); return CGS_ERR_ARG; }
    if (n == 0) return CGS_OK;
    if (!q || !order || !keys_sorted || !status || !scratch) { cgs_set_error("anchor_order: NULL"); return CGS_ERR_ARG; }
    if (scratch_bytes < cgs_anchor_order_scratch_bytes(n)) { cgs_set_error("anchor_order: scratch too small"); return CGS_ERR_WORKSPACE; }
    CgsCarver cv(scratch, scratch_bytes);
    uint32_t *lo = cv.take<uint32_t>(n), *hi = cv.take<uint32_t>(n), *w1 = cv.take<uint32_t>(n), *ord_a = cv.take<uint32_t>(n);
    uint32_t *ord_b = cv.take<uint32_t>(n), *kt = cv.take<uint32_t>(n), *vt = cv.take<uint32_t>(n), *ko = cv.take<uint32_t>(n);
    const size_t sort_bytes = cgs_sort_scratch_bytes(n);
    void *sort_scratch = cv.take<char>(sort_bytes);
    if (!cv.ok) { cgs_set_error("anchor_order: scratch too small"); return CGS_ERR_WORKSPACE; }
    const dim3 grid((unsigned)((n + AC_THREADS - 1) / AC_THREADS)), block(AC_THREADS);
    hipLaunchKernelGGL(anchor_keys_kernel, grid, block, 0, stream, q, n, lo, hi, status);
    CGS_CHECK_HIP(hipGetLastError());
    // stable LSD over the 48-bit key: the low 24 bits (values = positions), then the high 24 bits gathered through that order
    int rc = cgs_sort_pairs_u32(lo, nullptr, ko, ord_b, kt, vt, n, 0, 24, sort_scratch, sort_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(anchor_gather_hi_kernel, grid, block, 0, stream, (const uint32_t *)hi, (const uint32_t *)ord_b, n, w1);
    CGS_CHECK_HIP(hipGetLastError());
    rc = cgs_sort_pairs_u32(w1, ord_b, ko, ord_a, kt, vt, n, 0, 24, sort_scratch, sort_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(anchor_order_finish_kernel, grid, block, 0, stream, (const uint32_t *)lo, (const uint32_t *)ko,
                       (const uint32_t *)ord_a, n, order, keys_sorted);
    CGS_CHECK_HIP(hipGetLastError());
    return CGS_OK;
}

// ---- block-wide exclusive scans (256 threads = 4 waves) ---------------------------------------------------------------
// `part`: 4 LDS slots of the caller; every thread of the workgroup calls.  Returns the exclusive prefix of v, *total = the sum.
template <typename T>
__device__ __forceinline__ T ac_block_scan(T v, T *part, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();                                  // (the slots may still be read by the previous scan)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < AC_THREADS / 64; ++w) {
        const T p = part[w];
        if (w < wave) base += p;
        sum += p;
    }
    *total = sum;
    return base + inc - v;
}

// ---- pack --------------------------------------------------------------------------------------------------------------
extern "C" size_t cgs_anchor_pack_slot_bytes(int block) {
    // (block - 1) mantissas of at most 47 bits, rounded up to the 16-byte stores of the flush
    const size_t bits = (size_t)(block > 1 ? block - 1 : 0) * 47;
    return cgs_align_up((bits + 7) / 8, 16) + 16;
}

__global__ void __launch_bounds__(AC_THREADS)
    anchor_pack_kernel(const uint64_t *__restrict__ keys, int64_t n, int B, int32_t *__restrict__ cls,
                       uint64_t *__restrict__ first_key, uint8_t *__restrict__ slots, int64_t slot_bytes,
                       uint32_t *__restrict__ mant_len, uint32_t *__restrict__ hist) {
    __shared__ __attribute__((aligned(16))) uint32_t buf[AC_LDS_WORDS];
    __shared__ uint32_t h[AC_MAX_CLASS + 1];
    __shared__ uint32_t part[AC_THREADS / 64];
    const int64_t blk = blockIdx.x, i0 = blk * B;
    const int cnt = (int)min((int64_t)B, n - i0), t = threadIdx.x;
    const int per = (B + AC_THREADS - 1) / AC_THREADS;         // consecutive anchors per thread: their bits are consecutive too
    const int used_words = (int)(slot_bytes / 4) + 4;          // (never more than AC_LDS_WORDS: checked by the launcher)
    for (int i = t; i < used_words; i += AC_THREADS) buf[i] = 0u;
    if (t <= AC_MAX_CLASS) h[t] = 0u;
    __syncthreads();
    const int j0 = max(t * per, 1), j1 = min((t + 1) * per, cnt);   // (anchor 0 of the block is its first key: no gap)
    uint32_t bits = 0;
    for (int j = j0; j < j1; ++j) {
        const uint64_t d = keys[i0 + j] - keys[i0 + j - 1];
        const int c = d ? min(64 - __clzll((long long)d), AC_MAX_CLASS) : 0;      // (sorted 48-bit keys: d < 2^48)
        cls[i0 + j - (blk + 1)] = c;
        atomicAdd(&h[c], 1u);
        bits += c > 1 ? (uint32_t)(c - 1) : 0u;
    }
    uint32_t total;
    uint32_t p = ac_block_scan<uint32_t>(bits, part, &total);
    for (int j = j0; j < j1; ++j) {
        const uint64_t d = keys[i0 + j] - keys[i0 + j - 1];
        const int c = d ? min(64 - __clzll((long long)d), AC_MAX_CLASS) : 0;      // (sorted 48-bit keys: d < 2^48)
        if (c > 1) {
            const uint64_t m = d & ((1ull << (c - 1)) - 1ull);
            const uint32_t w = p >> 5, s = p & 31u;
            const uint64_t a = m << s;                         // a 47-bit field shifted by up to 31 spans three words
            const uint32_t top = s ? (uint32_t)(m >> (64u - s)) : 0u;
            if ((uint32_t)a) atomicOr(&buf[w], (uint32_t)a);
            if ((uint32_t)(a >> 32)) atomicOr(&buf[w + 1], (uint32_t)(a >> 32));
            if (top) atomicOr(&buf[w + 2], top);
            p += (uint32_t)(c - 1);
        }
    }
    __syncthreads();
    const uint32_t bytes = (total + 7u) >> 3;
    uint4 *dst = (uint4 *)(slots + blk * slot_bytes);          // slots are 16-byte aligned
    const uint4 *src = (const uint4 *)buf;
    for (uint32_t i = t; i < (bytes + 15u) >> 4; i += AC_THREADS) dst[i] = src[i];
    if (t == 0) {
        mant_len[blk] = bytes;
        first_key[blk] = keys[i0];
    }
    if (t <= AC_MAX_CLASS && h[t]) atomicAdd(&hist[t], h[t]);
}

// keys_sorted uint64 [n] (ascending) -> cls int32 [n - n_blocks] (the gap classes, block after block), first_key uint64
// [n_blocks], the mantissa bytes of block b at slots + b * cgs_anchor_pack_slot_bytes(block) (mant_len[b] of them), and the
// class histogram added to hist uint32 [49] (zeroed by the caller).
extern "C" int cgs_anchor_pack(const uint64_t *keys_sorted, int64_t n, int block, int32_t *cls, uint64_t *first_key,
                               uint8_t *slots, uint32_t *mant_len, uint32_t *hist, void *stream) {
    if (n < 0 || block < 64 || block > AC_MAX_B) { cgs_set_error("anchor_pack: block size outside [64, %d]", AC_MAX_B); return CGS_ERR_ARG; }
    if (n == 0) return CGS_OK;
    if (!keys_sorted || !cls || !first_key || !slots || !mant_len || !hist) { cgs_set_error("anchor_pack: NULL"); return CGS_ERR_ARG; }
    const int64_t nb = (n + block - 1) / block;
    const int64_t slot = (int64_t)cgs_anchor_pack_slot_bytes(block);
    if (nb >= (1ll << 31) || slot / 4 + 4 > AC_LDS_WORDS) { cgs_set_error("anchor_pack: bad sizes"); return CGS_ERR_ARG; }
    hipLaunchKernelGGL(anchor_pack_kernel, dim3((unsigned)nb), dim3(AC_THREADS), 0, (hipStream_t)stream, keys_sorted, n, block,
                       cls, first_key, slots, slot, mant_len, hist);
    CGS_CHECK_HIP(hipGetLastError());
    return CGS_OK;
}

// ---- unpack ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AC_THREADS)
    anchor_unpack_kernel(const float *__restrict__ cls, int64_t n, int B, const uint64_t *__restrict__ first_key,
                         const uint8_t *__restrict__ mant, const int64_t *__restrict__ mant_off, int32_t *__restrict__ q,
                         int32_t *__restrict__ status) {
    __shared__ uint32_t buf[AC_LDS_WORDS];
    __shared__ uint32_t part32[AC_THREADS / 64];
    __shared__ uint64_t part64[AC_THREADS / 64];
    const int64_t blk = blockIdx.x, i0 = blk * B;
    const int cnt = (int)min((int64_t)B, n - i0), t = threadIdx.x;
    const int per = (B + AC_THREADS - 1) / AC_THREADS;
    // the block's bytes -> LDS (dwords assembled from two aligned loads; nothing is read past the dword holding its last byte)
    const int64_t m0 = mant_off[blk];
    const uint32_t len = (uint32_t)max((int64_t)0, min(mant_off[blk + 1] - m0, (int64_t)(AC_LDS_WORDS - 4) * 4));
    const uint32_t words = (len + 3u) >> 2;
    {
        const uint8_t *p = mant + m0;
        const uint32_t sh = (uint32_t)((uintptr_t)p & 3) * 8;
        const uint32_t *pw = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
        const uint32_t last = (uint32_t)((((uintptr_t)p & 3) + len + 3) >> 2);      // aligned dwords that hold the block's bytes
        for (uint32_t i = t; i < words; i += AC_THREADS) {
            const uint32_t a = pw[i];
            const uint32_t b = (sh && i + 1 < last) ? pw[i + 1] : 0u;
            buf[i] = sh ? (a >> sh) | (b << (32 - sh)) : a;
        }
        if (t < 4) buf[words + t] = 0u;                                              // a window's overhang reads zeros
    }
    const int j0 = max(t * per, 1), j1 = min((t + 1) * per, cnt);
    uint32_t bits = 0;
    bool bad = false;
    for (int j = j0; j < j1; ++j) {
        const float cf = cls[i0 + j - (blk + 1)];
        if (!(cf >= 0.0f && cf <= (float)AC_MAX_CLASS)) { bad = true; continue; }
        const int c = (int)cf;
        bits += c > 1 ? (uint32_t)(c - 1) : 0u;
    }
    uint32_t total;
    uint32_t p = ac_block_scan<uint32_t>(bits, part32, &total);         // (its barriers also publish buf)
    uint64_t gaps[AC_PER];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < AC_PER; ++k) {
        const int j = t * per + k;
        uint64_t d = 0;
        if (k < per && j >= j0 && j < j1) {
            const float cf = cls[i0 + j - (blk + 1)];
            if (cf >= 0.0f && cf <= (float)AC_MAX_CLASS) {
                const int c = (int)cf;
                if (c > 1) {
                    const uint32_t nb = (uint32_t)(c - 1);
                    if ((uint64_t)p + nb > (uint64_t)len * 8u) bad = true;           // past the block's end: not read
                    else {
                        const uint32_t w = p >> 5, s = p & 31u;
                        const uint64_t lo = ((uint64_t)buf[w + 1] << 32) | buf[w];
                        const uint64_t win = s ? (lo >> s) | ((uint64_t)buf[w + 2] << (64u - s)) : lo;
                        d = (1ull << nb) | (win & ((1ull << nb) - 1ull));
                    }
                    p += nb;
                } else d = (uint64_t)c;
            }
        }
        gaps[k] = d;
        sum += d;
    }
    if (bad) atomicMax(status, 1 + (int32_t)min(blk, (int64_t)0x7FFFFFF0));
    uint64_t total64;
    uint64_t key = first_key[blk] + ac_block_scan<uint64_t>(sum, part64, &total64);
#pragma unroll
    for (int k = 0; k < AC_PER; ++k) {
        const int j = t * per + k;
        key += gaps[k];
        if (k < per && j < cnt) {
            int32_t *o = q + 3 * (i0 + j);
            o[0] = (int32_t)ac_gather3(key >> 2);
            o[1] = (int32_t)ac_gather3(key >> 1);
            o[2] = (int32_t)ac_gather3(key);
        }
    }
}

// cls float [n - n_blocks]: the decoded classes as cgs_table_ac_decode_lanes leaves them (integer-valued); mant + mant_off[b]
// .. mant_off[b + 1]: block b's mantissa bytes (mant_off int64 [n_blocks + 1], device); -> q int32 [n, 3].  *status (device
// int32, zeroed by the caller) becomes 1 + b when block b holds a class outside 0..48 or a mantissa past its byte length.
extern "C" int cgs_anchor_unpack(const float *cls, int64_t n, int block, const uint64_t *first_key, const uint8_t *mant,
                                 const int64_t *mant_off, int32_t *q, int32_t *status, void *stream) {
    if (n < 0 || block < 64 || block > AC_MAX_B) { cgs_set_error("anchor_unpack: block size outside [64, %d]", AC_MAX_B); return CGS_ERR_ARG; }
    if (n == 0) return CGS_OK;
    if (!cls || !first_key || !mant || !mant_off || !q || !status) { cgs_set_error("anchor_unpack: NULL"); return CGS_ERR_ARG; }
    const int64_t nb = (n + block - 1) / block;
    if (nb >= (1ll << 31)) { cgs_set_error("anchor_unpack: bad sizes"); return CGS_ERR_ARG; }
    hipLaunchKernelGGL(anchor_unpack_kernel, dim3((unsigned)nb), dim3(AC_THREADS), 0, (hipStream_t)stream, cls, n, block, first_key,
                       mant, mant_off, q, status);
    CGS_CHECK_HIP(hipGetLastError());
    return CGS_OK;
}
