// extern "C" entry points of libcgs_hip.so (see include/cgs.h) for the
// rasterizer, plus error plumbing and workspace carving.
#include <stdarg.h>
#include <string.h>
#include "cgs_internal.h"
#include "raster_forms.h"

static thread_local char g_err[512] = "";

void cgs_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int cgs_num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

extern "C" const char *cgs_last_error(void) { return g_err; }
extern "C" int cgs_version(void) { return CGS_VERSION; }
#ifndef CGS_SOURCE_DIGEST
#define CGS_SOURCE_DIGEST "unknown"
#endif
#ifndef CGS_BUILD_FLAGS
#define CGS_BUILD_FLAGS ""
#endif
extern "C" const char *cgs_build_info(void) { return CGS_SOURCE_DIGEST "|" CGS_BUILD_FLAGS; }

int cgs_scan_exclusive_u32_total(const uint32_t *in, uint32_t *out, int64_t n, void *scratch,
                                 size_t scratch_bytes, uint32_t *grand_total, hipStream_t stream);
int cgs_launch_iota(int64_t n, uint32_t *out, hipStream_t stream);
int cgs_launch_gather_tiles(int64_t P, const uint32_t *order, const uint32_t *tiles, uint32_t *out,
                            hipStream_t stream);
int cgs_launch_stats(const cgs_raster_cfg *cfg, CgsImg &im, int64_t *stats_out, hipStream_t stream);

// ---- workspace carving ---------------------------------------------------------
size_t cgs_geom_carve(CgsGeom *g, void *ws, size_t bytes, int64_t P) {
    CgsCarver c(ws, bytes);
    const size_t n = (size_t)(P > 0 ? P : 1);
    g->rec = c.take<float4>(3 * n);
    g->depth_key = c.take<uint32_t>(n);
    g->tiles = c.take<uint32_t>(n);
    g->rect = c.take<uint2>(n);
    g->order = c.take<uint32_t>(n);
    g->offsets = c.take<uint32_t>(n);
    g->sort_a = c.take<uint32_t>(n);
    g->sort_b = c.take<uint32_t>(n);
    g->sort_c = c.take<uint32_t>(n);
    g->sort_d = c.take<uint32_t>(n);
    g->total = c.take<uint32_t>(4);        // pair count | bucket-pair count | depth-range report of the depth sort | -
    size_t sb = cgs_sort_scratch_bytes((int64_t)n);
    size_t sc = cgs_scan_scratch_bytes((int64_t)n);
    g->scratch_bytes = sb > sc ? sb : sc;
    g->scratch = c.take<char>(g->scratch_bytes);
    return c.ok ? c.used() : 0;
}

size_t cgs_bin_carve(CgsBin *b, void *ws, size_t bytes, int64_t P, int64_t R) {
    (void)P;
    CgsCarver c(ws, bytes);
    const size_t n = (size_t)(R > 0 ? R : 1);
    b->tile_key_a = c.take<uint32_t>(n);
    b->tile_key_b = c.take<uint32_t>(n);
    b->gid_a = c.take<uint32_t>(n);
    b->gid_b = c.take<uint32_t>(n);
    b->tile_key_c = c.take<uint32_t>(n);
    b->gid_sorted = c.take<uint32_t>(n);
    b->scratch_bytes = cgs_sort_scratch_bytes((int64_t)n);
    b->scratch = c.take<char>(b->scratch_bytes);
    const int64_t slots = cgs_bucket_count_slots((int64_t)n);
    b->bk_tab = c.take<uint32_t>(cgs_bucket_tab_words());
    b->bk_counts = c.take<uint32_t>((size_t)slots);
    b->bk_scan = c.take<uint32_t>((size_t)slots);
    b->bk_scan_scratch_bytes = cgs_scan_scratch_bytes(slots);
    b->bk_scan_scratch = c.take<char>(b->bk_scan_scratch_bytes);
    return c.ok ? c.used() : 0;
}

size_t cgs_img_carve(CgsImg *im, void *ws, size_t bytes, int32_t H, int32_t W) {
    CgsCarver c(ws, bytes);
    const size_t tiles = (size_t)((W + CGS_TILE - 1) / CGS_TILE) * ((H + CGS_TILE - 1) / CGS_TILE);
    const size_t hw = (size_t)H * W;
    im->ranges = c.take<uint2>(tiles);
    im->final_T = c.take<float>(hw);
    im->n_contrib = c.take<uint32_t>(hw);
    im->tile_last = c.take<uint32_t>(tiles);
    im->tile_order = c.take<uint32_t>(tiles);
    return c.ok ? c.used() : 0;
}

extern "C" size_t cgs_raster_geom_bytes(int64_t P) {
    CgsGeom g;
    CgsCarver probe(nullptr, 0);
    (void)probe;
    return cgs_geom_carve(&g, nullptr, 0, P);
}
extern "C" size_t cgs_raster_bin_bytes(int64_t P, int64_t R) {
    CgsBin b;
    return cgs_bin_carve(&b, nullptr, 0, P, R);
}
extern "C" size_t cgs_raster_img_bytes(int32_t H, int32_t W) {
    CgsImg im;
    return cgs_img_carve(&im, nullptr, 0, H, W);
}
// The backward's scratch: d_mean_px [P, 2] | d_conic [P, 3] | d_z [P] | d_abs [P, 2], each 256-byte aligned.  Every entry point
// takes a prefix of it: the colour image alone, + dL/dz of the maps, + the absolute sums.  The one place that knows the layout:
// the three size queries, the backward's driver and cgs_raster_camera_backward all carve here.  Returns the prefix's bytes.
enum CgsBwdScratchPart { BWD_SCRATCH_COLOUR = 2, BWD_SCRATCH_MAPS = 3, BWD_SCRATCH_ABS = 4 };
struct CgsBwdScratch { float *d_mean_px, *d_conic, *d_z, *d_abs; };     // (d_z / d_abs: NULL outside the prefix)
static size_t cgs_bwd_scratch_carve(CgsBwdScratch *s, void *ws, int64_t P, CgsBwdScratchPart part) {
    CgsCarver c(ws, (size_t)-1);
    const size_t n = (size_t)(P > 0 ? P : 1);
    s->d_mean_px = c.take<float>(2 * n);
    s->d_conic = c.take<float>(3 * n);
    s->d_z = part >= BWD_SCRATCH_MAPS ? c.take<float>(n) : nullptr;
    s->d_abs = part >= BWD_SCRATCH_ABS ? c.take<float>(2 * n) : nullptr;
    return c.used();
}
extern "C" size_t cgs_raster_bwd_scratch_bytes(int64_t P) {
    CgsBwdScratch s;
    return cgs_bwd_scratch_carve(&s, nullptr, P, BWD_SCRATCH_COLOUR);
}
extern "C" size_t cgs_raster_bwd_aux_scratch_bytes(int64_t P) {
    CgsBwdScratch s;
    return cgs_bwd_scratch_carve(&s, nullptr, P, BWD_SCRATCH_MAPS);
}
// the aux scratch, then the [P, 2] sums of |dL_p/d(pixel mean)| of cgs_raster_backward_abs
extern "C" size_t cgs_raster_bwd_abs_scratch_bytes(int64_t P) {
    CgsBwdScratch s;
    return cgs_bwd_scratch_carve(&s, nullptr, P, BWD_SCRATCH_ABS);
}

static int check_cfg(const cgs_raster_cfg *cfg) {
    if (!cfg) { cgs_set_error("cfg is NULL"); return CGS_ERR_ARG; }
    if (cfg->image_height <= 0 || cfg->image_width <= 0) {
        cgs_set_error("bad image size %dx%d", cfg->image_width, cfg->image_height);
        return CGS_ERR_ARG;
    }
    if (cfg->image_height > 65535 * CGS_TILE / 16 * 16 || cfg->image_width > 65535 * 16) {
        cgs_set_error("image too large for 16-bit tile coordinates");
        return CGS_ERR_ARG;
    }
    if (!cfg->viewmatrix || !cfg->projmatrix) { cgs_set_error("matrices are NULL"); return CGS_ERR_ARG; }
    return CGS_OK;
}

// ---- visible_filter ----------------------------------------------------------------
extern "C" int cgs_filter(const cgs_raster_cfg *cfg, int64_t N, const float *means3D, const float *scales,
                          const float *rotations, int32_t *radii, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (N < 0) { cgs_set_error("N < 0"); return CGS_ERR_ARG; }
    if (N > 0 && (!means3D || !scales || !rotations || !radii)) {
        cgs_set_error("cgs_filter: NULL input");
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    memset(&g, 0, sizeof(g));
    return cgs_launch_preprocess(cfg, N, means3D, nullptr, nullptr, scales, rotations, g, radii, true,
                                 (hipStream_t)stream);
}

// visible_filter(means3D, cov3D_precomp=...): the same projection from the six covariance numbers
extern "C" int cgs_filter_cov(const cgs_raster_cfg *cfg, int64_t N, const float *means3D, const float *cov3D, int32_t *radii,
                              void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (N < 0) { cgs_set_error("N < 0"); return CGS_ERR_ARG; }
    if (N > 0 && (!means3D || !cov3D || !radii)) {
        cgs_set_error("cgs_filter_cov: NULL input");
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    memset(&g, 0, sizeof(g));
    CgsRasterForms f = {nullptr, 0, 0, 0, cov3D};
    return cgs_launch_preprocess_form(cfg, N, f, means3D, nullptr, nullptr, nullptr, nullptr, g, radii, true, (hipStream_t)stream);
}

int cgs_launch_filter_voxel(const cgs_raster_cfg *cfg, int64_t N, const float *means3D, const float *scaling, int64_t ld,
                            int scales_are_log, const float *rot1, uint8_t *visible, hipStream_t stream);

// prefilter_voxel in one launch: scaling [N, ld] raw rows (columns 0..2 used; exp applied when scales_are_log), rot1 [4]
// the normalised rotation shared by every anchor, visible [N] receives (radii > 0) as bool bytes.
extern "C" int cgs_filter_voxel(const cgs_raster_cfg *cfg, int64_t N, const float *means3D, const float *scaling,
                                int64_t ld, int scales_are_log, const float *rot1, uint8_t *visible, void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (N < 0 || ld < 3) { cgs_set_error("cgs_filter_voxel: bad N / ld"); return CGS_ERR_ARG; }
    if (N > 0 && (!means3D || !scaling || !rot1 || !visible)) { cgs_set_error("cgs_filter_voxel: NULL input"); return CGS_ERR_ARG; }
    return cgs_launch_filter_voxel(cfg, N, means3D, scaling, ld, scales_are_log, rot1, visible, (hipStream_t)stream);
}

// ---- forward stage 1 -----------------------------------------------------------------
// cgs_raster_preprocess_launch enqueues projection, the depth sort and the pair-offset scan, and the 4-byte copy of the
// pair count behind them; cgs_raster_preprocess_wait blocks on THAT copy's event only.  What the caller enqueues in between
// (cgs_raster_render_spec) keeps the device busy while the host learns the count.  cgs_raster_preprocess = both.
struct RasterCountSlot {
    uint32_t *pinned; hipEvent_t ev; bool pending; uint64_t ticket;
    // what a second depth sort of the launch needs (see raster_count_tail): valid from _launch to _wait
    int64_t P; void *geom_ws; size_t geom_bytes; hipStream_t stream; uint32_t epoch; bool ranged; bool spec_between; bool resorted;
};
static thread_local RasterCountSlot g_raster_slot = {nullptr, nullptr, false, 0, 0, nullptr, 0, nullptr, 0, false, false, false};
// Depth keys of a view sort on 27 bits (three passes) while every live depth stays below ~13107 (cgs_sort_depth_keys); the first
// view that reports a depth beyond that is sorted again on the full 32 bits (four passes) and so is every later view of the thread.
static thread_local bool g_depth_keys_full = false;
extern "C" int cgs_sort_depth_keys(const uint32_t *keys_in, uint32_t *keys_out, uint32_t *vals_out, uint32_t *keys_tmp,
                                   uint32_t *vals_tmp, int64_t n, void *scratch, size_t scratch_bytes, uint32_t *overflow,
                                   uint32_t epoch, void *stream);
extern "C" int cgs_debug_set_depth_keys_full(int on) { const int was = g_depth_keys_full; g_depth_keys_full = on != 0; return was; }

// Tickets of the *_launch / *_wait pairs: a slot holds ONE count per kind and host thread, so a second launch of the same kind
// overwrites what an earlier launch's wait would have read.  Every launch hands out a ticket (kind in the top byte, a
// per-thread serial below); the wait takes it back and refuses a ticket that is not the slot's current one instead of
// returning another launch's count.
uint64_t cgs_new_ticket(int kind) {
    static thread_local uint64_t serial = 0;
    return ((uint64_t)kind << 56) | (++serial & 0x00FFFFFFFFFFFFFFull);
}
static int raster_count_tail(int64_t P, CgsGeom &g, RasterCountSlot &sl, hipStream_t stream, bool full_keys = false);

// The argument rules of upstream GaussianRasterizer.forward, checked before anything is enqueued: exactly one of colors / shs,
// exactly one of (scales + rotations) / cov3D (both only when P > 0: an empty call may pass NULL everywhere), SH of degree
// 0..3 with (D+1)^2 <= M <= 16 coefficients and a camera position.
static int check_forms(const char *fn, const cgs_raster_cfg *cfg, int64_t P, const float *colors, const float *shs, int32_t sh_degree,
                       int32_t sh_coeffs, const float *scales, const float *rotations, const float *cov3D, CgsRasterForms &f) {
    if (P > 0 && (colors != nullptr) == (shs != nullptr)) {
        cgs_set_error("%s: please provide exactly one of either SHs or precomputed colors", fn);
        return CGS_ERR_ARG;
    }
    if (P > 0 && ((scales != nullptr || rotations != nullptr) == (cov3D != nullptr) || (!cov3D && (!scales || !rotations)))) {
        cgs_set_error("%s: please provide exactly one of either scale/rotation pair or precomputed 3D covariance", fn);
        return CGS_ERR_ARG;
    }
    if (shs) {
        if (sh_degree < 0 || sh_degree > 3) { cgs_set_error("%s: sh_degree %d outside 0..3", fn, sh_degree); return CGS_ERR_ARG; }
        if (sh_coeffs > 16 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) {
            cgs_set_error("%s: %d SH coefficients per Gaussian: degree %d needs %d..16", fn, sh_coeffs, sh_degree,
                          (sh_degree + 1) * (sh_degree + 1));
            return CGS_ERR_ARG;
        }
        if (!cfg->campos) { cgs_set_error("%s: SH colours need cfg->campos", fn); return CGS_ERR_ARG; }
    }
    f.shs = shs;
    f.sh_degree = sh_degree;
    f.sh_coeffs = sh_coeffs;
    f.sh_vec = shs && sh_coeffs % 4 == 0 && ((uintptr_t)shs & 15u) == 0;
    f.cov3D = cov3D;
    return CGS_OK;
}

static int raster_preprocess_launch_impl(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *colors,
                                         const float *opacities, const float *scales, const float *rotations,
                                         const CgsRasterForms *forms, void *geom_ws, size_t geom_bytes, int32_t *radii,
                                         void *stream_, uint64_t *ticket, bool aa = false);

extern "C" int cgs_raster_preprocess_launch(const cgs_raster_cfg *cfg, int64_t P, const float *means3D,
                                            const float *colors, const float *opacities, const float *scales,
                                            const float *rotations, void *geom_ws, size_t geom_bytes, int32_t *radii,
                                            void *stream_, uint64_t *ticket) {
    return raster_preprocess_launch_impl(cfg, P, means3D, colors, opacities, scales, rotations, nullptr, geom_ws, geom_bytes,
                                         radii, stream_, ticket);
}

extern "C" int cgs_raster_preprocess_launch_ex(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *colors,
                                               const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                               const float *scales, const float *rotations, const float *cov3D, void *geom_ws,
                                               size_t geom_bytes, int32_t *radii, void *stream_, uint64_t *ticket) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (ticket) *ticket = 0;
    CgsRasterForms f;
    if ((rc = check_forms("cgs_raster_preprocess_launch_ex", cfg, P, colors, shs, sh_degree, sh_coeffs, scales, rotations, cov3D, f)))
        return rc;
    // the colours_precomp + scales/rotations form is cgs_raster_preprocess_launch itself (same kernel)
    return raster_preprocess_launch_impl(cfg, P, means3D, colors, opacities, scales, rotations, (shs || cov3D) ? &f : nullptr,
                                         geom_ws, geom_bytes, radii, stream_, ticket);
}

// The option bits of the *_opt entry points (include/cgs.h); anything else is refused before anything is enqueued
static int check_opts(const char *fn, uint32_t opts) {
    if (opts & ~(uint32_t)CGS_RASTER_ANTIALIAS) {
        cgs_set_error("%s: unknown option bits 0x%x (known: CGS_RASTER_ANTIALIAS = 0x%x)", fn, opts & ~(uint32_t)CGS_RASTER_ANTIALIAS,
                      (uint32_t)CGS_RASTER_ANTIALIAS);
        return CGS_ERR_ARG;
    }
    return CGS_OK;
}

extern "C" int cgs_raster_preprocess_launch_opt(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *colors,
                                                const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                                const float *scales, const float *rotations, const float *cov3D, void *geom_ws,
                                                size_t geom_bytes, int32_t *radii, void *stream_, uint64_t *ticket, uint32_t opts) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (ticket) *ticket = 0;
    if ((rc = check_opts("cgs_raster_preprocess_launch_opt", opts))) return rc;
    CgsRasterForms f;
    if ((rc = check_forms("cgs_raster_preprocess_launch_opt", cfg, P, colors, shs, sh_degree, sh_coeffs, scales, rotations, cov3D, f)))
        return rc;
    return raster_preprocess_launch_impl(cfg, P, means3D, colors, opacities, scales, rotations, (shs || cov3D) ? &f : nullptr,
                                         geom_ws, geom_bytes, radii, stream_, ticket, (opts & CGS_RASTER_ANTIALIAS) != 0);
}

static int raster_preprocess_launch_impl(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *colors,
                                         const float *opacities, const float *scales, const float *rotations,
                                         const CgsRasterForms *forms, void *geom_ws, size_t geom_bytes, int32_t *radii,
                                         void *stream_, uint64_t *ticket, bool aa) {
    hipStream_t stream = (hipStream_t)stream_;
    RasterCountSlot &sl = g_raster_slot;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!ticket) { cgs_set_error("cgs_raster_preprocess_launch: NULL ticket"); return CGS_ERR_ARG; }
    *ticket = 0;
    if (P < 0 || P >= (1ll << 31)) { cgs_set_error("P out of range"); return CGS_ERR_ARG; }
    if (!sl.pinned) {
        CGS_CHECK_HIP(hipHostMalloc((void **)&sl.pinned, 64, hipHostMallocDefault));
        CGS_CHECK_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    }
    sl.pending = false;
    sl.pinned[0] = 0;
    sl.ranged = sl.spec_between = sl.resorted = false;
    *ticket = sl.ticket = cgs_new_ticket(1);
    if (P == 0) return CGS_OK;
    if (!means3D || !(colors || (forms && forms->shs)) || !opacities || !((scales && rotations) || (forms && forms->cov3D)) ||
        !radii || !geom_ws) {
        cgs_set_error("cgs_raster_preprocess: NULL input");
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    if (!cgs_geom_carve(&g, geom_ws, geom_bytes, P)) {
        cgs_set_error("geometry workspace too small: %zu < %zu", geom_bytes, cgs_raster_geom_bytes(P));
        return CGS_ERR_WORKSPACE;
    }
    if (forms) {
        if ((rc = cgs_launch_preprocess_form(cfg, P, *forms, means3D, colors, opacities, scales, rotations, g, radii, false,
                                             stream, aa)))
            return rc;
    } else if ((rc = cgs_launch_preprocess(cfg, P, means3D, colors, opacities, scales, rotations, g, radii, false,
                                           stream, aa)))
        return rc;
    sl.P = P; sl.geom_ws = geom_ws; sl.geom_bytes = geom_bytes; sl.stream = stream;
    return raster_count_tail(P, g, sl, stream);
}

// depth sort, tile rectangles in depth order, pair-offset scan and the copy of the pair count behind a preprocess launch
static int raster_count_tail(int64_t P, CgsGeom &g, RasterCountSlot &sl, hipStream_t stream, bool full_keys) {
    int rc;
    // depth order (stable: ties keep ascending Gaussian id)
    {
        CgsProfScope prof(CGS_PROF_DEPTH_SORT, stream);
        // (values = positions: the sort's first pass generates them, no iota launch)
        sl.ranged = !(full_keys || g_depth_keys_full);
        if (sl.ranged) {
            // 27-bit keys, three passes; a live depth beyond the range writes this launch's epoch to g.total[2], which travels
            // to the host with the pair count: cgs_raster_preprocess_wait then sorts again on 32 bits
            sl.epoch = (uint32_t)(sl.ticket & 0x7FFFFFFFu) + 1u;
            rc = cgs_sort_depth_keys(g.depth_key, g.sort_a, g.order, g.sort_b, g.sort_d, P, g.scratch, g.scratch_bytes,
                                     g.total + 2, sl.epoch, stream);
        } else {
            rc = cgs_sort_pairs_u32(g.depth_key, nullptr, g.sort_a, g.order, g.sort_b, g.sort_d, P, 0, 32, g.scratch,
                                    g.scratch_bytes, stream);
        }
        if (rc) return rc;
    }
    {
        CgsProfScope prof(CGS_PROF_OFFSETS_SCAN, stream);
        // tile rectangles and tile counts in depth order (sort_b / sort_d / sort_a are free after the sort)
        if ((rc = cgs_launch_gather_rects(P, g, stream))) return rc;
        if ((rc = cgs_scan_exclusive_u32_total(g.sort_a, g.offsets, P, g.scratch, g.scratch_bytes, g.total,
                                               stream)))
            return rc;
    }
    CGS_CHECK_HIP(hipMemcpyAsync(sl.pinned, g.total, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CGS_CHECK_HIP(hipEventRecord(sl.ev, stream));
    sl.pending = true;
    return CGS_OK;
}

// cgs_raster_preprocess_launch with the Gaussians taken straight from the anchor expansion (csrc/expand_raster.hip): slot i
// of the n_anchor * K slots with flags[i] != 0 is Gaussian pos[i] (flags / pos / neural_opacity from cgs_expand_count_launch,
// P = the count it returned); scaling_out [P,3] receives the Gaussians' scales (the one per-Gaussian tensor the training
// loss reads), xyz_out [P,3] / rot_out [P,4] (both or neither) the positions and rotations for a later cgs_raster_backward.
// Everything downstream (cgs_raster_render*, _wait, cgs_raster_backward + cgs_expand_backward) is unchanged.
extern "C" int cgs_raster_preprocess_expand_launch(const cgs_raster_cfg *cfg, int64_t n_anchor, int K, const uint8_t *flags,
                                                   const uint32_t *pos, const float *anchor, const float *gscaling,
                                                   const float *offsets, const float *neural_opacity, const float *color_in,
                                                   const float *cov_in, const int64_t *src_row, int64_t P, float *scaling_out,
                                                   float *xyz_out, float *rot_out, void *geom_ws, size_t geom_bytes,
                                                   int32_t *radii, void *stream_, uint64_t *ticket) {
    hipStream_t stream = (hipStream_t)stream_;
    RasterCountSlot &sl = g_raster_slot;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!ticket) { cgs_set_error("cgs_raster_preprocess_expand_launch: NULL ticket"); return CGS_ERR_ARG; }
    *ticket = 0;
    if (P < 0 || P >= (1ll << 31) || n_anchor < 0 || K < 1 || n_anchor * (int64_t)K >= (1ll << 31) || P > n_anchor * (int64_t)K) {
        cgs_set_error("cgs_raster_preprocess_expand: sizes out of range");
        return CGS_ERR_ARG;
    }
    if (!sl.pinned) {
        CGS_CHECK_HIP(hipHostMalloc((void **)&sl.pinned, 64, hipHostMallocDefault));
        CGS_CHECK_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    }
    sl.pending = false;
    sl.pinned[0] = 0;
    sl.ranged = sl.spec_between = sl.resorted = false;
    *ticket = sl.ticket = cgs_new_ticket(1);
    if (P == 0) return CGS_OK;
    if (!flags || !pos || !anchor || !gscaling || !offsets || !neural_opacity || !color_in || !cov_in || !scaling_out || !radii ||
        !geom_ws) {
        cgs_set_error("cgs_raster_preprocess_expand: NULL input");
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    if (!cgs_geom_carve(&g, geom_ws, geom_bytes, P)) {
        cgs_set_error("geometry workspace too small: %zu < %zu", geom_bytes, cgs_raster_geom_bytes(P));
        return CGS_ERR_WORKSPACE;
    }
    const CgsExpandSrc x{n_anchor, K, flags, pos, anchor, gscaling, offsets, neural_opacity, color_in, cov_in, src_row};
    if ((xyz_out == nullptr) != (rot_out == nullptr)) { cgs_set_error("cgs_raster_preprocess_expand: xyz_out and rot_out go together"); return CGS_ERR_ARG; }
    if ((rc = cgs_launch_expand_preprocess(cfg, x, scaling_out, xyz_out, rot_out, g, radii, stream))) return rc;
    sl.P = P; sl.geom_ws = geom_ws; sl.geom_bytes = geom_bytes; sl.stream = stream;
    return raster_count_tail(P, g, sl, stream);
}

extern "C" int cgs_raster_preprocess_wait2(uint64_t ticket, int64_t *num_rendered_host, int *order_changed) {
    RasterCountSlot &sl = g_raster_slot;
    if (order_changed) *order_changed = 0;
    if (!num_rendered_host) { cgs_set_error("num_rendered_host is NULL"); return CGS_ERR_ARG; }
    *num_rendered_host = 0;
    if (!sl.pinned) { cgs_set_error("cgs_raster_preprocess_wait: no launch on this thread"); return CGS_ERR_ARG; }
    if (ticket == 0 || ticket != sl.ticket) {
        cgs_set_error("cgs_raster_preprocess_wait: stale ticket (another preprocess launch was issued on this thread since)");
        return CGS_ERR_ARG;
    }
    if (sl.pending) {
        CGS_CHECK_HIP(hipEventSynchronize(sl.ev));
        sl.pending = false;
        if (sl.ranged && sl.pinned[2] == sl.epoch) {
            // a live depth beyond the 27-bit key range (~13107): the order in the workspace is not the depth order.  Sort this
            // view again on the full 32 bits — the depth keys are intact — and keep to that for the thread's later views.
            g_depth_keys_full = true;
            CgsGeom g;
            if (!cgs_geom_carve(&g, sl.geom_ws, sl.geom_bytes, sl.P)) { cgs_set_error("geometry workspace too small"); return CGS_ERR_WORKSPACE; }
            int rc = raster_count_tail(sl.P, g, sl, sl.stream, true);
            if (rc) return rc;
            CGS_CHECK_HIP(hipEventSynchronize(sl.ev));
            sl.pending = false;
            sl.resorted = true;
        }
    }
    if (sl.resorted && order_changed) *order_changed = 1;
    *num_rendered_host = (int64_t)sl.pinned[0];
    return CGS_OK;
}

extern "C" int cgs_raster_preprocess_wait(uint64_t ticket, int64_t *num_rendered_host) {
    int changed = 0;
    int rc = cgs_raster_preprocess_wait2(ticket, num_rendered_host, &changed);
    if (rc) return rc;
    if (changed && g_raster_slot.spec_between) {
        cgs_set_error("cgs_raster_preprocess_wait: the view was sorted again on 32-bit depth keys after cgs_raster_render_spec ran on the "
                      "first order; call cgs_raster_render with the returned count (or use cgs_raster_preprocess_wait2)");
        return CGS_ERR_RESPEC;
    }
    return CGS_OK;
}

extern "C" int cgs_raster_preprocess(const cgs_raster_cfg *cfg, int64_t P, const float *means3D,
                                     const float *colors, const float *opacities, const float *scales,
                                     const float *rotations, void *geom_ws, size_t geom_bytes, int32_t *radii,
                                     int64_t *num_rendered_host, void *stream_) {
    if (!num_rendered_host) { cgs_set_error("num_rendered_host is NULL"); return CGS_ERR_ARG; }
    *num_rendered_host = 0;
    uint64_t ticket = 0;
    int rc = cgs_raster_preprocess_launch(cfg, P, means3D, colors, opacities, scales, rotations, geom_ws, geom_bytes, radii,
                                          stream_, &ticket);
    if (rc) return rc;
    return cgs_raster_preprocess_wait(ticket, num_rendered_host);
}

// ---- forward stage 2 -----------------------------------------------------------------
static int tile_bits(const cgs_raster_cfg *cfg) {
    const uint32_t nt = (uint32_t)(cgs_tiles_x(cfg) * cgs_tiles_y(cfg));
    int bits = 0;
    while ((1u << bits) < nt) ++bits;
    return bits;
}

// Which binning: 0 = by the pair count per Gaussian (the two-level path from CGS_BUCKET_MIN_RATIO tiles per Gaussian on),
// 1 = radix passes over (tile, Gaussian) pairs, 2 = two-level wherever the grid allows it.  cgs_debug_set_bin_mode is the
// test / measurement hook (tests/test_raster_gpu.py runs the list comparisons under both).
static int g_bin_mode = 0;
#ifndef CGS_BUCKET_MIN_RATIO
#define CGS_BUCKET_MIN_RATIO 6
#endif
extern "C" int cgs_debug_set_bin_mode(int mode) {
    if (mode < 0 || mode > 2) { cgs_set_error("cgs_debug_set_bin_mode: 0 (auto), 1 (radix) or 2 (buckets)"); return CGS_ERR_ARG; }
    g_bin_mode = mode;
    return CGS_OK;
}
static bool use_buckets(const cgs_raster_cfg *cfg, int64_t P, int64_t R) {
    if (g_bin_mode == 1 || !cgs_tile_bin_buckets_ok(cfg) || !cgs_tile_bin_buckets_fits(R)) return false;
    return g_bin_mode == 2 || R >= (int64_t)CGS_BUCKET_MIN_RATIO * P;
}

static int raster_render_impl(const cgs_raster_cfg *cfg, int64_t P, int64_t R, bool spec, void *geom_ws,
                              size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                              size_t img_bytes, float *out_color, hipStream_t stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!cfg->bg || !out_color || !img_ws) { cgs_set_error("cgs_raster_render: NULL input"); return CGS_ERR_ARG; }
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    memset(&g, 0, sizeof(g));
    memset(&b, 0, sizeof(b));
    const bool bin16 = cgs_tile_bin16_ok(tile_bits(cfg));
    if (spec && (!bin16 || P <= 0 || R <= 0)) {
        cgs_set_error("cgs_raster_render_spec: needs a grid of <= 65536 tiles, P > 0 and a positive capacity");
        return CGS_ERR_ARG;
    }
    if (!cgs_img_carve(&im, img_ws, img_bytes, cfg->image_height, cfg->image_width)) {
        cgs_set_error("image workspace too small");
        return CGS_ERR_WORKSPACE;
    }
    if (P > 0 && (!geom_ws || !cgs_geom_carve(&g, geom_ws, geom_bytes, P))) {
        cgs_set_error("geometry workspace missing or too small");
        return CGS_ERR_WORKSPACE;
    }
    if (R > 0) {
        if (!bin_ws || !cgs_bin_carve(&b, bin_ws, bin_bytes, P, R)) {
            cgs_set_error("binning workspace too small: %zu < %zu", bin_bytes, cgs_raster_bin_bytes(P, R));
            return CGS_ERR_WORKSPACE;
        }
        if (bin16 && use_buckets(cfg, P, R)) {
            // csrc/tile_bin.hip, two-level: bucket lists by one radix pass, tile lists by count + scan + fill
            if ((rc = cgs_launch_tile_bin_buckets(cfg, P, R, g, b, im, stream, spec ? g.total : nullptr))) return rc;
        } else if (bin16) {
            // csrc/tile_bin.hip: the first radix pass generates its pairs, 16-bit tile keys
            if ((rc = cgs_launch_tile_bin16(cfg, P, R, tile_bits(cfg), g, b, im, stream, spec ? g.total : nullptr))) return rc;
        } else {
            if ((rc = cgs_launch_emit_pairs(cfg, P, g, b, stream))) return rc;
            CgsProfScope prof(CGS_PROF_TILE_SORT, stream);
            if ((rc = cgs_sort_pairs_u32(b.tile_key_a, b.gid_a, b.tile_key_c, b.gid_sorted, b.tile_key_b, b.gid_b,
                                         R, 0, tile_bits(cfg), b.scratch, b.scratch_bytes, stream)))
                return rc;
        }
    }
    if (!(bin16 && R > 0) && (rc = cgs_launch_ranges(cfg, R, b, im, stream))) return rc;
    if ((rc = cgs_launch_tile_order(cfg, im, stream))) return rc;
    return cgs_launch_blend_fwd(cfg, g, b, im, out_color, stream);
}

extern "C" int cgs_raster_render(const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws,
                                 size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                 size_t img_bytes, float *out_color, void *stream_) {
    return raster_render_impl(cfg, P, R, false, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, out_color,
                              (hipStream_t)stream_);
}

// Speculative render between cgs_raster_preprocess_launch and _wait: R_cap is the capacity of the binning workspace
// (cgs_raster_bin_bytes(P, R_cap)), the pair count itself stays on the device.  Valid when the count _wait returns is
// <= R_cap (the per-tile lists are then exactly those of cgs_raster_render, and the backward takes R_cap as its R);
// otherwise the caller renders again with cgs_raster_render and the true count.  Grids of more than 65536 tiles: CGS_ERR_ARG.
extern "C" int cgs_raster_render_spec(const cgs_raster_cfg *cfg, int64_t P, int64_t R_cap, void *geom_ws,
                                      size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                      size_t img_bytes, float *out_color, void *stream_) {
    g_raster_slot.spec_between = true;
    return raster_render_impl(cfg, P, R_cap, true, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, out_color,
                              (hipStream_t)stream_);
}

// ---- depth / inverse-depth / alpha maps (csrc/raster_aux.hip) --------------------------------------------------------
int cgs_launch_aux_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, float *out_depth, float *out_invdepth,
                       float *out_alpha, hipStream_t stream);
int cgs_launch_aux_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *dL_ddepth,
                       const float *dL_dinvdepth, const float *dL_dalpha, float *dL_dmean2D_px, float *dL_dconic,
                       float *dL_dopacity, float *dL_dz, hipStream_t stream);
int cgs_launch_aux_dz_chain(const cgs_raster_cfg *cfg, int64_t P, const int32_t *radii, const float *dL_dz, float *dL_dmeans3D,
                            hipStream_t stream);
// ---- N-channel per-Gaussian features (csrc/raster_feat.hip) ---------------------------------------------------------------
int cgs_launch_feat_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *features, int C, float *out,
                        hipStream_t stream);
int cgs_launch_feat_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *features, int C,
                        const float *dL_dmap, float *dL_dmean2D_px, float *dL_dconic, float *dL_dopacity, float *dL_dfeatures,
                        hipStream_t stream);
// ---- per-Gaussian contribution statistics and top-contributor maps (csrc/raster_contrib.hip) ------------------------------
int cgs_launch_contrib(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const int32_t *slot, float *acc_weight,
                       float *acc_max_weight, int64_t *acc_pixels, int64_t *acc_top_pixels, int32_t *out_top_id,
                       float *out_top_weight, int32_t *out_count, hipStream_t stream);

// ---- depth-distortion and median-depth maps (csrc/raster_geom_maps.hip) -----------------------------------------------------
int cgs_launch_geom_maps_fwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, float *out_distortion,
                             float *out_median_depth, int32_t *out_median_id, float *out_moments, hipStream_t stream);
int cgs_launch_geom_maps_bwd(const cgs_raster_cfg *cfg, CgsGeom &g, CgsBin &b, CgsImg &im, const float *moments,
                             const int32_t *median_id, const float *dL_ddistortion, const float *dL_dmedian_depth,
                             float *dL_dmean2D_px, float *dL_dconic, float *dL_dopacity, float *dL_dz, hipStream_t stream);

// The workspaces of a render the caller kept, for the passes enqueued behind it (cgs_raster_render_aux, _render_features,
// cgs_raster_contrib): g and b zeroed, then carved where there is something to carve.  fn: the entry point's name in front of
// the message; NULL for cgs_raster_render_aux, whose messages carry none.
static int carve_kept_render(const char *fn, const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws, size_t geom_bytes,
                             void *bin_ws, size_t bin_bytes, void *img_ws, size_t img_bytes, CgsGeom &g, CgsBin &b, CgsImg &im) {
    const char *sep = fn ? ": " : "";
    if (!fn) fn = "";
    memset(&g, 0, sizeof(g));
    memset(&b, 0, sizeof(b));
    if (!cgs_img_carve(&im, img_ws, img_bytes, cfg->image_height, cfg->image_width)) {
        cgs_set_error("%s%simage workspace too small", fn, sep);
        return CGS_ERR_WORKSPACE;
    }
    if (P > 0 && geom_ws && !cgs_geom_carve(&g, geom_ws, geom_bytes, P)) {
        cgs_set_error("%s%sgeometry workspace too small", fn, sep);
        return CGS_ERR_WORKSPACE;
    }
    if (R > 0 && !cgs_bin_carve(&b, bin_ws, bin_bytes, P, R)) {
        cgs_set_error("%s%sbinning workspace too small: %zu < %zu", fn, sep, bin_bytes, cgs_raster_bin_bytes(P, R));
        return CGS_ERR_WORKSPACE;
    }
    return CGS_OK;
}

// Enqueued after the view's cgs_raster_render / _render_spec that the caller kept (R = the count its binning workspace was
// carved with): reads the lists, n_contrib, tile_last and final_T that render left.
extern "C" int cgs_raster_render_aux(const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws, size_t geom_bytes,
                                     void *bin_ws, size_t bin_bytes, void *img_ws, size_t img_bytes, float *out_depth,
                                     float *out_invdepth, float *out_alpha, void *stream_) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (P < 0 || R < 0) { cgs_set_error("cgs_raster_render_aux: P < 0 or R < 0"); return CGS_ERR_ARG; }
    if (!out_depth || !out_invdepth || !out_alpha || !img_ws || (R > 0 && (!geom_ws || !bin_ws))) {
        cgs_set_error("cgs_raster_render_aux: NULL input");
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    if ((rc = carve_kept_render(nullptr, cfg, P, R, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, g, b, im))) return rc;
    return cgs_launch_aux_fwd(cfg, g, b, im, out_depth, out_invdepth, out_alpha, (hipStream_t)stream_);
}

// The feature map of a view: enqueued after the render the caller kept, exactly as cgs_raster_render_aux.  Every pixel of
// out_features [C, H, W] is written (zeros where nothing was blended, R == 0 included).
extern "C" int cgs_raster_render_features(const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws, size_t geom_bytes,
                                          void *bin_ws, size_t bin_bytes, void *img_ws, size_t img_bytes, const float *features,
                                          int32_t C, float *out_features, void *stream_) {
    const char *fn = "cgs_raster_render_features";
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (P < 0 || R < 0) { cgs_set_error("%s: P < 0 or R < 0", fn); return CGS_ERR_ARG; }
    if (C < 1 || C > CGS_RASTER_MAX_FEATURES) {
        cgs_set_error("%s: %d feature channels outside 1..%d", fn, C, CGS_RASTER_MAX_FEATURES);
        return CGS_ERR_ARG;
    }
    if (!out_features || (P > 0 && !features)) {       // (P == 0: there is no table to point at)
        cgs_set_error("%s: features and out_features go together (one of them is NULL)", fn);
        return CGS_ERR_ARG;
    }
    if (!img_ws || (R > 0 && (!geom_ws || !bin_ws))) { cgs_set_error("%s: NULL workspace", fn); return CGS_ERR_ARG; }
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    if ((rc = carve_kept_render(fn, cfg, P, R, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, g, b, im))) return rc;
    return cgs_launch_feat_fwd(cfg, g, b, im, features, C, out_features, (hipStream_t)stream_);
}

// How much each Gaussian mattered to the view, and which one dominates each pixel: enqueued after the render the caller kept,
// exactly as cgs_raster_render_aux.  The four accumulators are added into (never zeroed here); the three maps are written for
// every pixel (-1 / 0 / 0 where nothing was blended, R == 0 included).  Any of the seven may be NULL: not computed.  The values
// of `slot` are not range-checked on the device: 0 <= slot[i] < n_slots is the caller's contract.
extern "C" int cgs_raster_contrib(const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws, size_t geom_bytes, void *bin_ws,
                                  size_t bin_bytes, void *img_ws, size_t img_bytes, const int32_t *slot, int64_t n_slots,
                                  float *acc_weight, float *acc_max_weight, int64_t *acc_pixels, int64_t *acc_top_pixels,
                                  int32_t *out_top_id, float *out_top_weight, int32_t *out_count, void *stream_) {
    const char *fn = "cgs_raster_contrib";
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (P < 0 || R < 0) { cgs_set_error("%s: P < 0 or R < 0", fn); return CGS_ERR_ARG; }
    if (!acc_weight && !acc_max_weight && !acc_pixels && !acc_top_pixels && !out_top_id && !out_top_weight && !out_count) {
        cgs_set_error("%s: no output given (all four accumulators and all three maps are NULL)", fn);
        return CGS_ERR_ARG;
    }
    if (!img_ws || (R > 0 && (!geom_ws || !bin_ws))) { cgs_set_error("%s: NULL workspace", fn); return CGS_ERR_ARG; }
    if (slot && n_slots <= 0) { cgs_set_error("%s: slot given with n_slots = %lld <= 0", fn, (long long)n_slots); return CGS_ERR_ARG; }
    if (!slot && n_slots != P) {
        cgs_set_error("%s: n_slots = %lld != P = %lld without a slot table", fn, (long long)n_slots, (long long)P);
        return CGS_ERR_ARG;
    }
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    if ((rc = carve_kept_render(fn, cfg, P, R, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, g, b, im))) return rc;
    return cgs_launch_contrib(cfg, g, b, im, slot, acc_weight, acc_max_weight, acc_pixels, acc_top_pixels, out_top_id,
                              out_top_weight, out_count, (hipStream_t)stream_);
}

// The depth-distortion map, the median depth and its Gaussian: enqueued after the render the caller kept, exactly as
// cgs_raster_render_aux.  Every pixel of the three maps and of out_moments [2, H, W] (what the backward needs of the forward's
// sums) is written; zeros / -1 where nothing was blended, R == 0 included.  P == 0: nothing is enqueued.
extern "C" int cgs_raster_render_geom(const cgs_raster_cfg *cfg, int64_t P, int64_t R, void *geom_ws, size_t geom_bytes,
                                      void *bin_ws, size_t bin_bytes, void *img_ws, size_t img_bytes, float *out_distortion,
                                      float *out_median_depth, int32_t *out_median_id, float *out_moments, void *stream_) {
    const char *fn = "cgs_raster_render_geom";
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (P < 0 || R < 0) { cgs_set_error("%s: P < 0 or R < 0", fn); return CGS_ERR_ARG; }
    if (!out_distortion || !out_median_depth || !out_median_id || !out_moments) {
        cgs_set_error("%s: NULL output (distortion, median_depth, median_id and moments are all written)", fn);
        return CGS_ERR_ARG;
    }
    if (!img_ws || (R > 0 && (!geom_ws || !bin_ws))) { cgs_set_error("%s: NULL workspace", fn); return CGS_ERR_ARG; }
    if (P == 0) return CGS_OK;
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    if ((rc = carve_kept_render(fn, cfg, P, R, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, g, b, im))) return rc;
    return cgs_launch_geom_maps_fwd(cfg, g, b, im, out_distortion, out_median_depth, out_median_id, out_moments,
                                    (hipStream_t)stream_);
}

// ---- backward -----------------------------------------------------------------------------
// One driver, raster_backward_run, behind the eight exported cgs_raster_backward* entry points (include/cgs.h): each of them
// fills a RasterBwdCall and calls it.  Nothing is enqueued on a path that returns an error.

// The workspace of the bit-reproducible backward (csrc/raster_blend_rows.hip, the DET instances): base [P] (exclusive scan of
// geom.tiles in id order) | the scan's scratch | the slot array, 48 B per pair
static const size_t DET_SLOT_BYTES = 48;
struct DetLayout { size_t scan_off, scan_bytes, slots_off; };
static DetLayout det_layout(int64_t P) {
    const size_t n = (size_t)(P > 0 ? P : 1);
    DetLayout l;
    l.scan_bytes = cgs_scan_scratch_bytes((int64_t)n);
    l.scan_off = cgs_align_up(n * sizeof(uint32_t), 256);
    l.slots_off = l.scan_off + cgs_align_up(l.scan_bytes, 256);
    return l;
}
extern "C" size_t cgs_raster_bwd_det_bytes(int64_t P, int64_t num_rendered, int32_t means2D_cols) {
    (void)means2D_cols;         // (one slot layout for both widths: columns 9, 10 are the absolute sums)
    return det_layout(P).slots_off + cgs_align_up((size_t)(num_rendered > 0 ? num_rendered : 1) * DET_SLOT_BYTES, 256);
}

int cgs_launch_blend_bwd_det(const cgs_raster_cfg *cfg, int64_t P, int64_t R, CgsGeom &g, CgsBin &b, CgsImg &im,
                             const float *dL_dout, const uint32_t *slot_base, void *slots, float *dL_dmean2D_px, float *dL_dconic,
                             float *dL_dopacity, float *dL_dcolors, float *dL_dz, float *dL_dabs_px, hipStream_t stream);

// What an entry point allows (the first six fields; the table in DESIGN.md), then its arguments in the order of the longest
// signature.  An entry point without an argument leaves it zero: no map gradients, opts == 0, no features, no det_ws, no
// distortion / median-depth gradients.
struct RasterBwdCall {
    const char *fn;         // the entry point's name in front of the messages
    bool oldest;            // cgs_raster_backward / _ex: dL_dout is required, the forms are checked before P and R, and a NULL
                            // workspace is CGS_ERR_WORKSPACE (the later entry points: CGS_ERR_ARG with the other NULL inputs)
    bool any_form;          // check_forms applies; false for cgs_raster_backward, whose signature is the plain form itself
    bool det;               // cgs_raster_backward_det: no map gradients, det_ws, nothing zero-filled (every row is written)
    CgsBwdScratchPart scratch;      // the layout the scratch must hold; zero-filled unless `det`
    int32_t means2D_cols;   // columns of dL_dmeans2D: 3, or 4 with the absolute sums
    const cgs_raster_cfg *cfg;
    int64_t P, R;
    const float *means3D, *colors, *shs;
    int32_t sh_degree, sh_coeffs;
    const float *opacities, *scales, *rotations, *cov3D;
    const int32_t *radii;
    void *geom_ws; size_t geom_bytes;
    void *bin_ws; size_t bin_bytes;
    void *img_ws; size_t img_bytes;
    const float *dL_dout, *dL_ddepth, *dL_dinvdepth, *dL_dalpha;
    float *dL_dmeans3D, *dL_dmeans2D, *dL_dcolors, *dL_dopacities, *dL_dshs, *dL_dscales, *dL_drotations, *dL_dcov3D;
    void *scratch_ws; size_t scratch_bytes;
    void *stream;
    uint32_t opts;
    const float *features; int32_t C; const float *dL_dfeatures_map; float *dL_dfeatures;
    void *det_ws; size_t det_bytes;
    const float *moments; const int32_t *median_id; const float *dL_ddistortion, *dL_dmedian_depth;    // cgs_raster_backward_geom
};

// Checks, carving, [zero fill | scan of geom.tiles], the blend backwards (colour, maps, features) into the scratch's
// dL/d(pixel mean) / dL/d(conic) / dL/dz (and the caller's dL_dcolors / dL_dopacities), the per-Gaussian backward, dL/dz's chain.
static int raster_backward_run(const RasterBwdCall &c) {
    const char *fn = c.fn;
    const cgs_raster_cfg *cfg = c.cfg;
    const int64_t P = c.P, R = c.R;
    hipStream_t stream = (hipStream_t)c.stream;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if ((rc = check_opts(fn, c.opts))) return rc;
    const bool aa = (c.opts & CGS_RASTER_ANTIALIAS) != 0, aux = c.dL_ddepth || c.dL_dinvdepth || c.dL_dalpha;
    const bool plain = !c.shs && !c.cov3D;      // colours + scales / rotations: cgs_launch_preprocess_bwd
    if (!c.oldest && (P < 0 || R < 0)) { cgs_set_error("%s: P < 0 or R < 0", fn); return CGS_ERR_ARG; }
    if (c.means2D_cols != 3 && c.means2D_cols != 4) {
        cgs_set_error("%s: means2D_cols = %d, must be 3 or 4", fn, c.means2D_cols);
        return CGS_ERR_ARG;
    }
    if (c.det && aux) {
        cgs_set_error("%s: dL_ddepth, dL_dinvdepth and dL_dalpha must be NULL (the map blends' backward sums with float atomics "
                      "and is not covered by the deterministic mode)", fn);
        return CGS_ERR_ARG;
    }
    if ((c.features != nullptr) != (c.dL_dfeatures != nullptr)) {
        cgs_set_error("%s: features and dL_dfeatures go together (one of them is NULL)", fn);
        return CGS_ERR_ARG;
    }
    if (c.features && (c.C < 1 || c.C > CGS_RASTER_MAX_FEATURES)) {
        cgs_set_error("%s: %d feature channels outside 1..%d", fn, c.C, CGS_RASTER_MAX_FEATURES);
        return CGS_ERR_ARG;
    }
    const bool geomaps = c.dL_ddistortion || c.dL_dmedian_depth;      // (with both NULL the two saved maps are not looked at)
    if ((c.dL_ddistortion && !c.moments) || (c.dL_dmedian_depth && !c.median_id)) {
        cgs_set_error("%s: dL_ddistortion needs moments and dL_dmedian_depth needs median_id (what cgs_raster_render_geom "
                      "wrote; the one a given gradient needs is NULL)", fn);
        return CGS_ERR_ARG;
    }
    CgsRasterForms f = {nullptr, 0, 0, 0, nullptr};
    if (c.any_form && (rc = check_forms(fn, cfg, P, c.colors, c.shs, c.sh_degree, c.sh_coeffs, c.scales, c.rotations, c.cov3D, f)))
        return rc;
    if (c.oldest) {
        if (plain) fn = "cgs_raster_backward";      // (cgs_raster_backward_ex with the plain form is that entry point)
        if (P < 0 || R < 0) { cgs_set_error("%s: P < 0 or R < 0", fn); return CGS_ERR_ARG; }
    }
    if (P == 0) return CGS_OK;
    if (!c.radii || !c.dL_dmeans3D || !c.dL_dmeans2D || !c.dL_dcolors || !c.dL_dopacities || !c.scratch_ws ||
        (c.shs && !c.dL_dshs) || (c.cov3D && !c.dL_dcov3D) || (!c.cov3D && (!c.dL_dscales || !c.dL_drotations)) ||
        (c.oldest ? !c.dL_dout || (!plain && !c.means3D)
                  : !c.means3D || !c.geom_ws || !c.img_ws || (R > 0 && !c.bin_ws) || (aa && !c.opacities) || (c.det && !c.det_ws))) {
        cgs_set_error("%s: NULL input", fn);
        return CGS_ERR_ARG;
    }
    CgsBwdScratch s;
    const size_t scratch_need = cgs_bwd_scratch_carve(&s, c.scratch_ws, P, c.scratch);
    if (c.scratch_bytes < scratch_need) {
        cgs_set_error("%s: scratch too small: %zu < %zu", fn, c.scratch_bytes, scratch_need);
        return CGS_ERR_WORKSPACE;
    }
    if (c.det && c.det_bytes < cgs_raster_bwd_det_bytes(P, R, c.means2D_cols)) {
        cgs_set_error("%s: det_ws too small: %zu < %zu", fn, c.det_bytes, cgs_raster_bwd_det_bytes(P, R, c.means2D_cols));
        return CGS_ERR_WORKSPACE;
    }
    CgsGeom g;
    CgsBin b;
    CgsImg im;
    memset(&b, 0, sizeof(b));
    if (!c.geom_ws || !c.img_ws || !cgs_geom_carve(&g, c.geom_ws, c.geom_bytes, P) ||
        !cgs_img_carve(&im, c.img_ws, c.img_bytes, cfg->image_height, cfg->image_width) ||
        (R > 0 && (!c.bin_ws || !cgs_bin_carve(&b, c.bin_ws, c.bin_bytes, P, R)))) {
        cgs_set_error("%s: workspace too small", fn);
        return CGS_ERR_WORKSPACE;
    }
    // four columns: dL_dmeans2D is [P, 4] and the blend backward sums the absolute accumulator behind dL/dz
    float *d_abs = c.means2D_cols == 4 ? s.d_abs : nullptr;
    if (c.det) {
        // store-and-sum instead of float atomics (include/cgs.h): base = scan of geom.tiles, [zero fill of the slots, DET blend
        // backward,] per-Gaussian sum INTO the scratch; without a blend the sum kernel reads neither base nor a slot
        const DetLayout dl = det_layout(P);
        uint32_t *base = (uint32_t *)c.det_ws;
        if (R > 0 && c.dL_dout) {
            if ((rc = cgs_scan_exclusive_u32_total(g.tiles, base, P, (char *)c.det_ws + dl.scan_off, dl.scan_bytes, nullptr, stream)))
                return rc;
            if (cfg->debug) CGS_CHECK_HIP(hipStreamSynchronize(stream));
        }
        if ((rc = cgs_launch_blend_bwd_det(cfg, P, R, g, b, im, c.dL_dout, base, (char *)c.det_ws + dl.slots_off, s.d_mean_px,
                                           s.d_conic, c.dL_dopacities, c.dL_dcolors, s.d_z, d_abs, stream)))
            return rc;
    } else {
        CGS_CHECK_HIP(hipMemsetAsync(c.scratch_ws, 0, scratch_need, stream));
        if (R > 0) {
            if (c.dL_dout && (rc = cgs_launch_blend_bwd(cfg, g, b, im, c.dL_dout, s.d_mean_px, s.d_conic, c.dL_dopacities,
                                                        c.dL_dcolors, stream, d_abs)))
                return rc;
            if (aux && (rc = cgs_launch_aux_bwd(cfg, g, b, im, c.dL_ddepth, c.dL_dinvdepth, c.dL_dalpha, s.d_mean_px, s.d_conic,
                                                c.dL_dopacities, s.d_z, stream)))
                return rc;
            if (c.features && c.dL_dfeatures_map &&
                (rc = cgs_launch_feat_bwd(cfg, g, b, im, c.features, c.C, c.dL_dfeatures_map, s.d_mean_px, s.d_conic,
                                          c.dL_dopacities, c.dL_dfeatures, stream)))
                return rc;
            if (geomaps && (rc = cgs_launch_geom_maps_bwd(cfg, g, b, im, c.moments, c.median_id, c.dL_ddistortion,
                                                          c.dL_dmedian_depth, s.d_mean_px, s.d_conic, c.dL_dopacities, s.d_z,
                                                          stream)))
                return rc;
        }
    }
    // antialiasing: the blend backwards have summed dL/d(op_eff) into dL_dopacities by now; the per-Gaussian kernel turns it
    // into dL/d(opacity) in place and chains h's share to the covariance
    const float *aa_op = aa ? c.opacities : nullptr;
    float *aa_dop = aa ? c.dL_dopacities : nullptr;
    if (plain)
        rc = cgs_launch_preprocess_bwd(cfg, P, c.means3D, c.scales, c.rotations, c.radii, s.d_mean_px, s.d_conic, c.dL_dmeans3D,
                                       c.dL_dmeans2D, c.dL_dscales, c.dL_drotations, stream, aa_op, aa_dop, d_abs);
    else
        rc = cgs_launch_preprocess_bwd_form(cfg, P, f, c.means3D, c.scales, c.rotations, c.radii, s.d_mean_px, s.d_conic,
                                            c.dL_dcolors, c.dL_dmeans3D, c.dL_dmeans2D, c.dL_dshs, c.dL_dscales, c.dL_drotations,
                                            c.dL_dcov3D, stream, aa_op, aa_dop, d_abs);
    if (rc) return rc;
    return (aux || geomaps) ? cgs_launch_aux_dz_chain(cfg, P, c.radii, s.d_z, c.dL_dmeans3D, stream) : CGS_OK;
}

extern "C" int cgs_raster_backward(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D,
                                   const float *colors, const float *opacities, const float *scales,
                                   const float *rotations, const int32_t *radii, void *geom_ws,
                                   size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                   size_t img_bytes, const float *dL_dout, float *dL_dmeans3D,
                                   float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacities,
                                   float *dL_dscales, float *dL_drotations, void *scratch,
                                   size_t scratch_bytes, void *stream_) {
    const RasterBwdCall c = {"cgs_raster_backward", true, false, false, BWD_SCRATCH_COLOUR, 3,
                             cfg, P, R, means3D, colors, nullptr, 0, 0, opacities, scales, rotations, nullptr, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, nullptr, nullptr, nullptr,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, nullptr, dL_dscales, dL_drotations, nullptr,
                             scratch, scratch_bytes, stream_};
    return raster_backward_run(c);
}

extern "C" int cgs_raster_backward_ex(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                      const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                      const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                      void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                      size_t img_bytes, const float *dL_dout, float *dL_dmeans3D, float *dL_dmeans2D,
                                      float *dL_dcolors, float *dL_dopacities, float *dL_dshs, float *dL_dscales,
                                      float *dL_drotations, float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_) {
    const RasterBwdCall c = {"cgs_raster_backward_ex", true, true, false, BWD_SCRATCH_COLOUR, 3,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, nullptr, nullptr, nullptr,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_};
    return raster_backward_run(c);
}

// Backward of the colour image and the three maps together, every argument form of cgs_raster_backward_ex.  Each upstream
// gradient may be NULL; without dL_dout no colour blend backward runs (dL_dcolors keeps its zeros).
extern "C" int cgs_raster_backward_aux(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                       const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                       const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                       void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                       size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                       const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                       float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                       float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_) {
    const RasterBwdCall c = {"cgs_raster_backward_aux", false, true, false, BWD_SCRATCH_MAPS, 3,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_};
    return raster_backward_run(c);
}

// cgs_raster_backward_aux with the options word: CGS_RASTER_ANTIALIAS also reads opacities
extern "C" int cgs_raster_backward_opt(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                       const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                       const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                       void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                       size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                       const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                       float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                       float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_, uint32_t opts) {
    const RasterBwdCall c = {"cgs_raster_backward_opt", false, true, false, BWD_SCRATCH_MAPS, 3,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_, opts};
    return raster_backward_run(c);
}

// cgs_raster_backward_opt plus the feature map's gradient: the feature blend backward adds into the same scratch and
// dL_dopacities, behind the other two blends.  features == NULL: cgs_raster_backward_opt's result.
extern "C" int cgs_raster_backward_feat(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                        const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                        const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                        void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                        size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                        const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                        float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                        float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_, uint32_t opts,
                                        const float *features, int32_t C, const float *dL_dfeatures_map, float *dL_dfeatures) {
    const RasterBwdCall c = {"cgs_raster_backward_feat", false, true, false, BWD_SCRATCH_MAPS, 3,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_, opts, features, C, dL_dfeatures_map, dL_dfeatures};
    return raster_backward_run(c);
}

// cgs_raster_backward_feat with dL_dmeans2D [P, 4]: columns 2:4 are the sums over the pixels of |dL_p/d(2-D mean)| of the colour
// image (the ABS instance of the blend backward; include/cgs.h).  Every other result is cgs_raster_backward_feat's.
extern "C" int cgs_raster_backward_abs(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                       const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                       const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                       void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                       size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                       const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                       float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                       float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_, uint32_t opts,
                                       const float *features, int32_t C, const float *dL_dfeatures_map, float *dL_dfeatures) {
    const RasterBwdCall c = {"cgs_raster_backward_abs", false, true, false, BWD_SCRATCH_ABS, 4,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_, opts, features, C, dL_dfeatures_map, dL_dfeatures};
    return raster_backward_run(c);
}

// cgs_raster_backward_abs plus the gradients of the distortion and median-depth maps: their blend backward
// (csrc/raster_geom_maps.hip) adds into the same scratch, dL_dopacities and dL/dz behind the other blends.  With both gradients
// NULL: cgs_raster_backward_abs's result.
extern "C" int cgs_raster_backward_geom(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                        const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                        const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                        void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                        size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                        const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                        float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                        float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_, uint32_t opts,
                                        const float *features, int32_t C, const float *dL_dfeatures_map, float *dL_dfeatures,
                                        const float *moments, const int32_t *median_id, const float *dL_ddistortion,
                                        const float *dL_dmedian_depth) {
    const RasterBwdCall c = {"cgs_raster_backward_geom", false, true, false, BWD_SCRATCH_ABS, 4,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_, opts, features, C, dL_dfeatures_map, dL_dfeatures, nullptr, 0,
                             moments, median_id, dL_ddistortion, dL_dmedian_depth};
    return raster_backward_run(c);
}

// cgs_raster_backward_abs's colour path with every float-atomic sum replaced by the store-and-sum form (include/cgs.h), into the
// scratch layout of cgs_raster_backward_abs for either width of dL_dmeans2D, then the unchanged per-Gaussian backward.
extern "C" int cgs_raster_backward_det(const cgs_raster_cfg *cfg, int64_t P, int64_t R, const float *means3D, const float *colors,
                                       const float *shs, int32_t sh_degree, int32_t sh_coeffs, const float *opacities,
                                       const float *scales, const float *rotations, const float *cov3D, const int32_t *radii,
                                       void *geom_ws, size_t geom_bytes, void *bin_ws, size_t bin_bytes, void *img_ws,
                                       size_t img_bytes, const float *dL_dout, const float *dL_ddepth, const float *dL_dinvdepth,
                                       const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                                       float *dL_dopacities, float *dL_dshs, float *dL_dscales, float *dL_drotations,
                                       float *dL_dcov3D, void *scratch, size_t scratch_bytes, void *stream_, uint32_t opts,
                                       int32_t means2D_cols, void *det_ws, size_t det_bytes) {
    const RasterBwdCall c = {"cgs_raster_backward_det", false, true, true, BWD_SCRATCH_ABS, means2D_cols,
                             cfg, P, R, means3D, colors, shs, sh_degree, sh_coeffs, opacities, scales, rotations, cov3D, radii,
                             geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes, dL_dout, dL_ddepth, dL_dinvdepth, dL_dalpha,
                             dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D,
                             scratch, scratch_bytes, stream_, opts, nullptr, 0, nullptr, nullptr, det_ws, det_bytes};
    return raster_backward_run(c);
}

// ---- camera gradients (csrc/raster_camera.hip) ---------------------------------------------------------------------------
size_t cgs_camera_work_bytes(int64_t P);
int cgs_launch_camera_bwd(const cgs_raster_cfg *cfg, int64_t P, const CgsRasterForms &f, const float *means3D, const float *opacities,
                          const float *scales, const float *rotations, const int32_t *radii, const float *d_mean_px,
                          const float *d_conic, const float *d_z, const float *dL_dcolors, const float *d_opacities, bool aa,
                          float *out_view, float *out_proj, float *out_campos, void *work, hipStream_t stream);

extern "C" size_t cgs_raster_camera_bytes(int64_t P) { return cgs_camera_work_bytes(P); }

extern "C" int cgs_raster_camera_backward(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *shs,
                                          int32_t sh_degree, int32_t sh_coeffs, const float *opacities, const float *scales,
                                          const float *rotations, const float *cov3D, const int32_t *radii, const void *scratch,
                                          size_t scratch_bytes, const float *dL_dcolors, const float *dL_dopacities, uint32_t opts,
                                          float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *work,
                                          size_t work_bytes, void *stream_) {
    const char *fn = "cgs_raster_camera_backward";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (P < 0 || P >= (1ll << 31)) { cgs_set_error("%s: P out of range", fn); return CGS_ERR_ARG; }
    if (opts & ~(uint32_t)(CGS_RASTER_ANTIALIAS | CGS_RASTER_CAMERA_MAPS)) {
        cgs_set_error("%s: unknown option bits 0x%x (known: CGS_RASTER_ANTIALIAS = 0x%x, CGS_RASTER_CAMERA_MAPS = 0x%x)", fn,
                      opts & ~(uint32_t)(CGS_RASTER_ANTIALIAS | CGS_RASTER_CAMERA_MAPS), (uint32_t)CGS_RASTER_ANTIALIAS,
                      (uint32_t)CGS_RASTER_CAMERA_MAPS);
        return CGS_ERR_ARG;
    }
    const bool aa = (opts & CGS_RASTER_ANTIALIAS) != 0, maps = (opts & CGS_RASTER_CAMERA_MAPS) != 0;
    if (!dL_dviewmatrix && !dL_dprojmatrix && !dL_dcampos) { cgs_set_error("%s: no output given", fn); return CGS_ERR_ARG; }
    if (dL_dcampos && ((P > 0 && !shs) || !cfg->campos)) {
        cgs_set_error("%s: dL_dcampos needs shs and cfg->campos (the camera position enters through the SH direction only)", fn);
        return CGS_ERR_ARG;
    }
    if (!work || work_bytes < cgs_camera_work_bytes(P)) {
        cgs_set_error("%s: work missing or too small: %zu < %zu", fn, work ? work_bytes : (size_t)0, cgs_camera_work_bytes(P));
        return CGS_ERR_ARG;
    }
    CgsBwdScratch s;       // (read only; d_z: NULL without the maps)
    const size_t need = cgs_bwd_scratch_carve(&s, const_cast<void *>(scratch), P, maps ? BWD_SCRATCH_MAPS : BWD_SCRATCH_COLOUR);
    CgsRasterForms f = {nullptr, 0, 0, 0, cov3D};
    if (dL_dcampos) {
        if (sh_degree < 0 || sh_degree > 3) { cgs_set_error("%s: sh_degree %d outside 0..3", fn, sh_degree); return CGS_ERR_ARG; }
        if (sh_coeffs > 16 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) {
            cgs_set_error("%s: %d SH coefficients per Gaussian: degree %d needs %d..16", fn, sh_coeffs, sh_degree,
                          (sh_degree + 1) * (sh_degree + 1));
            return CGS_ERR_ARG;
        }
        f.shs = shs;
        f.sh_degree = sh_degree;
        f.sh_coeffs = sh_coeffs;
        f.sh_vec = sh_coeffs % 4 == 0 && ((uintptr_t)shs & 15u) == 0;
    }
    if (P > 0) {
        if ((scales != nullptr || rotations != nullptr) == (cov3D != nullptr) || (!cov3D && (!scales || !rotations))) {
            cgs_set_error("%s: please provide exactly one of either scale/rotation pair or precomputed 3D covariance", fn);
            return CGS_ERR_ARG;
        }
        if (!means3D || !radii || !scratch || (dL_dcampos && !dL_dcolors) || (aa && (!opacities || !dL_dopacities))) {
            cgs_set_error("%s: NULL input", fn);
            return CGS_ERR_ARG;
        }
        if (scratch_bytes < need) { cgs_set_error("%s: scratch too small: %zu < %zu", fn, scratch_bytes, need); return CGS_ERR_ARG; }
    }
    if (P == 0) {       // no Gaussian: zeros
        if (dL_dviewmatrix) CGS_CHECK_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), stream));
        if (dL_dprojmatrix) CGS_CHECK_HIP(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), stream));
        if (dL_dcampos) CGS_CHECK_HIP(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), stream));
        return CGS_OK;
    }
    return cgs_launch_camera_bwd(cfg, P, f, means3D, opacities, scales, rotations, radii, s.d_mean_px, s.d_conic, s.d_z, dL_dcolors,
                                 dL_dopacities, aa, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, work, stream);
}

extern "C" int cgs_raster_stats(const cgs_raster_cfg *cfg, void *img_ws, size_t img_bytes, int64_t *stats_out,
                                void *stream) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    CgsImg im;
    if (!img_ws || !stats_out || !cgs_img_carve(&im, img_ws, img_bytes, cfg->image_height, cfg->image_width)) {
        cgs_set_error("image workspace missing or too small");
        return CGS_ERR_WORKSPACE;
    }
    return cgs_launch_stats(cfg, im, stats_out, (hipStream_t)stream);
}

// ---- normal maps and the normal-consistency regulariser (csrc/normal_maps.hip) ------------------------------------------------
int cgs_launch_gaussian_normals_fwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                    const float *rotations, float *out, hipStream_t stream);
int cgs_launch_gaussian_normals_bwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                    const float *rotations, const float *dL_dout, float *dL_drotations, hipStream_t stream);
int cgs_launch_depth_normals_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth, float *out,
                                 hipStream_t stream);
int cgs_launch_depth_normals_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth,
                                 const float *dL_dout, float *dL_ddepth, hipStream_t stream);
int cgs_launch_normal_consistency_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                      const float *depth, const float *weight, float *out, hipStream_t stream);
int cgs_launch_normal_consistency_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                      const float *depth, const float *weight, const float *dL_dE, float *dL_dnormals,
                                      float *dL_ddepth, hipStream_t stream);

// The per-Gaussian entry points read cfg->viewmatrix only.  P == 0: CGS_OK, nothing enqueued, no pointer looked at.
static int check_gaussian_normals(const char *fn, const cgs_raster_cfg *cfg, int64_t P) {
    if (!cfg) { cgs_set_error("%s: cfg is NULL", fn); return CGS_ERR_ARG; }
    if (P < 0) { cgs_set_error("%s: P < 0", fn); return CGS_ERR_ARG; }
    if (P >= (1ll << 31) * 256) { cgs_set_error("%s: P = %lld is beyond one launch", fn, (long long)P); return CGS_ERR_ARG; }
    if (!cfg->viewmatrix) { cgs_set_error("%s: cfg->viewmatrix is NULL", fn); return CGS_ERR_ARG; }
    return CGS_OK;
}

extern "C" int cgs_gaussian_normals_fwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                        const float *rotations, float *out_normals, void *stream) {
    const char *fn = "cgs_gaussian_normals_fwd";
    int rc = check_gaussian_normals(fn, cfg, P);
    if (rc) return rc;
    if (P > 0 && (!means3D || !scales || !rotations || !out_normals)) { cgs_set_error("%s: NULL input or output", fn); return CGS_ERR_ARG; }
    return cgs_launch_gaussian_normals_fwd(cfg, P, means3D, scales, rotations, out_normals, (hipStream_t)stream);
}

extern "C" int cgs_gaussian_normals_bwd(const cgs_raster_cfg *cfg, int64_t P, const float *means3D, const float *scales,
                                        const float *rotations, const float *dL_dnormals, float *dL_drotations, void *stream) {
    const char *fn = "cgs_gaussian_normals_bwd";
    int rc = check_gaussian_normals(fn, cfg, P);
    if (rc) return rc;
    if (P > 0 && (!means3D || !scales || !rotations || !dL_dnormals || !dL_drotations)) {
        cgs_set_error("%s: NULL input or output", fn);
        return CGS_ERR_ARG;
    }
    return cgs_launch_gaussian_normals_bwd(cfg, P, means3D, scales, rotations, dL_dnormals, dL_drotations, (hipStream_t)stream);
}

// The per-pixel entry points take the five numbers they read instead of a cgs_raster_cfg.
static int check_normal_view(const char *fn, int32_t H, int32_t W, float tanfovx, float tanfovy, float eps) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) { cgs_set_error("%s: image size %dx%d outside 1..65535", fn, W, H); return CGS_ERR_ARG; }
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f) || !(tanfovx < 1e30f) || !(tanfovy < 1e30f)) {
        cgs_set_error("%s: tanfovx, tanfovy = %g, %g must be positive and finite", fn, (double)tanfovx, (double)tanfovy);
        return CGS_ERR_ARG;
    }
    if (!(eps >= 0.f) || !(eps < 1e30f)) { cgs_set_error("%s: eps = %g must be >= 0 and finite", fn, (double)eps); return CGS_ERR_ARG; }
    return CGS_OK;
}

extern "C" int cgs_depth_normals_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth,
                                     float *out_normals, void *stream) {
    const char *fn = "cgs_depth_normals_fwd";
    int rc = check_normal_view(fn, H, W, tanfovx, tanfovy, eps);
    if (rc) return rc;
    if (!depth || !out_normals) { cgs_set_error("%s: NULL input or output", fn); return CGS_ERR_ARG; }
    return cgs_launch_depth_normals_fwd(H, W, tanfovx, tanfovy, eps, depth, out_normals, (hipStream_t)stream);
}

extern "C" int cgs_depth_normals_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *depth,
                                     const float *dL_dnormals, float *dL_ddepth, void *stream) {
    const char *fn = "cgs_depth_normals_bwd";
    int rc = check_normal_view(fn, H, W, tanfovx, tanfovy, eps);
    if (rc) return rc;
    if (!depth || !dL_dnormals || !dL_ddepth) { cgs_set_error("%s: NULL input or output", fn); return CGS_ERR_ARG; }
    return cgs_launch_depth_normals_bwd(H, W, tanfovx, tanfovy, eps, depth, dL_dnormals, dL_ddepth, (hipStream_t)stream);
}

extern "C" int cgs_normal_consistency_fwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                          const float *depth, const float *weight, float *out_error, void *stream) {
    const char *fn = "cgs_normal_consistency_fwd";
    int rc = check_normal_view(fn, H, W, tanfovx, tanfovy, eps);
    if (rc) return rc;
    if (!normals || !depth || !out_error) { cgs_set_error("%s: NULL input or output (only weight may be NULL)", fn); return CGS_ERR_ARG; }
    return cgs_launch_normal_consistency_fwd(H, W, tanfovx, tanfovy, eps, normals, depth, weight, out_error, (hipStream_t)stream);
}

extern "C" int cgs_normal_consistency_bwd(int32_t H, int32_t W, float tanfovx, float tanfovy, float eps, const float *normals,
                                          const float *depth, const float *weight, const float *dL_derror, float *dL_dnormals,
                                          float *dL_ddepth, void *stream) {
    const char *fn = "cgs_normal_consistency_bwd";
    int rc = check_normal_view(fn, H, W, tanfovx, tanfovy, eps);
    if (rc) return rc;
    if (!normals || !depth || !dL_derror) { cgs_set_error("%s: NULL input (only weight may be NULL)", fn); return CGS_ERR_ARG; }
    if (!dL_dnormals && !dL_ddepth) { cgs_set_error("%s: no output given (dL_dnormals and dL_ddepth are both NULL)", fn); return CGS_ERR_ARG; }
    return cgs_launch_normal_consistency_bwd(H, W, tanfovx, tanfovy, eps, normals, depth, weight, dL_derror, dL_dnormals, dL_ddepth,
                                             (hipStream_t)stream);
}
