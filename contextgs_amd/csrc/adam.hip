// The optimizer step of the training iteration (scene/gaussian_model.py:475 `torch.optim.Adam(l, lr=0.0, eps=1e-15)`,
// train.py:255 `gaussians.optimizer.step()`): torch's default path walks the 13 parameter groups with a handful of
// foreach launches each; here up to CGS_ADAM_MAX tensors are stepped by ONE launch, and a per-anchor tensor may be
// stepped on the rows of a byte mask only (the anchors the view saw), which moves only that fraction of the 28 bytes per
// element (read p, g, m, v; write p, m, v).  HBM-bound: 16-byte accesses over the flat array, four per thread and array.
#include "cgs_internal.h"

#define ADAM_THREADS 256
#define ADAM_VEC_PER_THREAD 4
#define ADAM_CHUNK (ADAM_THREADS * ADAM_VEC_PER_THREAD * 4)      // elements per workgroup

struct AdamArgs {
    cgs_adam_tensor t[CGS_ADAM_MAX];
    uint32_t first_chunk[CGS_ADAM_MAX + 1];      // workgroups [first_chunk[k], first_chunk[k + 1]) walk tensor k
    int nt;
};

struct AdamScalars { float step_size, bias2_sqrt, beta2, omb1, omb2, eps, wd; };

// -ffp-contract=off (build.py): the statements below are what runs, the same on the vector and the scalar path
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars &s) {
    if (s.wd != 0.f) g = g + s.wd * p;
    m = m + (g - m) * s.omb1;
    v = v * s.beta2 + g * g * s.omb2;
    p = p - s.step_size * (m / (sqrtf(v) / s.bias2_sqrt + s.eps));
}

__device__ __forceinline__ void adam_scalar(float *p, const float *g, float *m, float *v, int64_t e, const AdamScalars &s) {
    float pe = p[e], me = m[e], ve = v[e];
    adam_element(pe, g[e], me, ve, s);
    p[e] = pe; m[e] = me; v[e] = ve;
}

__global__ void __launch_bounds__(ADAM_THREADS) adam_step_kernel(AdamArgs a, const uint8_t *__restrict__ rows) {
    int k = 0;
    for (int j = 1; j < a.nt; ++j) k += blockIdx.x >= a.first_chunk[j] ? 1 : 0;
    const cgs_adam_tensor &t = a.t[k];
    float *p = t.p; const float *g = t.g; float *m = t.m; float *v = t.v;
    const int64_t numel = t.numel;
    const uint32_t width = rows ? (uint32_t)t.width : 0u;
    AdamScalars s;
    s.step_size = t.step_size; s.bias2_sqrt = t.bias2_sqrt; s.eps = t.eps; s.wd = t.weight_decay;
    s.beta2 = (float)t.beta2; s.omb1 = (float)(1.0 - t.beta1); s.omb2 = (float)(1.0 - t.beta2);

    const int64_t e0 = (int64_t)(blockIdx.x - a.first_chunk[k]) * ADAM_CHUNK;      // first element of this workgroup's chunk
    const int n = (int)min((int64_t)ADAM_CHUNK, numel - e0);                       // elements of the chunk, >= 1
    // row of the chunk's first element and its column: one 64-bit division per workgroup, 32-bit ones per access below
    const int64_t r0 = width ? e0 / width : 0;
    const uint32_t c0 = width ? (uint32_t)(e0 - r0 * width) : 0u;
    const uint8_t *rw = rows + r0;

    const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15u) == 0;
    if (!aligned) {
        // any 4-byte-aligned pointers: one element per thread and pass, consecutive threads on consecutive elements
        for (int l = threadIdx.x; l < n; l += ADAM_THREADS) {
            if (width && !rw[(c0 + (uint32_t)l) / width]) continue;
            adam_scalar(p, g, m, v, e0 + l, s);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < ADAM_VEC_PER_THREAD; ++i) {
        const int l = 4 * ((int)threadIdx.x + ADAM_THREADS * i);     // e0 is a multiple of 4: e0 + l stays 16-byte aligned
        if (l >= n) break;
        const int cnt = min(4, n - l);                                // < 4 only in the tensor's last float4
        bool on[4] = {true, true, true, true};
        if (width) {
            const uint32_t c = c0 + (uint32_t)l, q = c / width;
            if (c - q * width + 3u < width) {                         // the four components share a row
                on[0] = on[1] = on[2] = on[3] = rw[q] != 0;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) on[j] = j < cnt && rw[(c + (uint32_t)j) / width] != 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) on[j] = on[j] && j < cnt;
        const int64_t e = e0 + l;
        if (on[0] && on[1] && on[2] && on[3]) {
            float4 pp = *(const float4 *)(p + e), mm = *(const float4 *)(m + e), vv = *(const float4 *)(v + e);
            const float4 gg = *(const float4 *)(g + e);
            adam_element(pp.x, gg.x, mm.x, vv.x, s);
            adam_element(pp.y, gg.y, mm.y, vv.y, s);
            adam_element(pp.z, gg.z, mm.z, vv.z, s);
            adam_element(pp.w, gg.w, mm.w, vv.w, s);
            *(float4 *)(p + e) = pp; *(float4 *)(m + e) = mm; *(float4 *)(v + e) = vv;
        } else {
            // a float4 that straddles rows of which some are masked out, or the tensor's tail: visible components one by one
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (on[j]) adam_scalar(p, g, m, v, e + j, s);
        }
    }
}

extern "C" int cgs_adam_step(int nt, const cgs_adam_tensor *tensors, const uint8_t *rows, int64_t n_rows, void *stream) {
    if (nt < 0 || nt > CGS_ADAM_MAX) { cgs_set_error("adam_step: nt = %d outside [0, %d]", nt, CGS_ADAM_MAX); return CGS_ERR_ARG; }
    if (n_rows < 0) { cgs_set_error("adam_step: n_rows < 0"); return CGS_ERR_ARG; }
    if (nt == 0) return CGS_OK;
    if (!tensors) { cgs_set_error("adam_step: NULL descriptor array"); return CGS_ERR_ARG; }
    AdamArgs a;
    uint64_t chunks = 0;
    int used = 0;
    for (int k = 0; k < nt; ++k) {
        const cgs_adam_tensor &t = tensors[k];
        if (t.numel < 0) { cgs_set_error("adam_step: tensor %d: numel < 0", k); return CGS_ERR_ARG; }
        if (t.width < 0) { cgs_set_error("adam_step: tensor %d: width < 0", k); return CGS_ERR_ARG; }
        if (t.width > 0) {
            if (!rows) {
                if (n_rows != 0) { cgs_set_error("adam_step: tensor %d is row-sparse but rows is NULL (n_rows = %lld)", k, (long long)n_rows); return CGS_ERR_ARG; }
            } else if (t.numel / t.width != n_rows || t.numel % t.width != 0) {
                cgs_set_error("adam_step: tensor %d: numel %lld != n_rows %lld * width %d", k, (long long)t.numel,
                              (long long)n_rows, t.width);
                return CGS_ERR_ARG;
            }
        }
        if (t.numel == 0) continue;           // takes no workgroup
        if (!t.p || !t.g || !t.m || !t.v) { cgs_set_error("adam_step: tensor %d: NULL pointer", k); return CGS_ERR_ARG; }
        a.t[used] = t;
        a.first_chunk[used] = (uint32_t)chunks;
        chunks += (uint64_t)((t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
        if (chunks > 0x7fffffffull) { cgs_set_error("adam_step: more than 2^31 workgroups"); return CGS_ERR_ARG; }
        ++used;
    }
    if (used == 0) return CGS_OK;
    for (int k = used; k < CGS_ADAM_MAX; ++k) { a.t[k] = cgs_adam_tensor{}; a.first_chunk[k] = (uint32_t)chunks; }
    a.first_chunk[CGS_ADAM_MAX] = (uint32_t)chunks;
    a.first_chunk[used] = (uint32_t)chunks;
    a.nt = used;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a, rows);
    CGS_CHECK_HIP(hipGetLastError());
    return CGS_OK;
}
