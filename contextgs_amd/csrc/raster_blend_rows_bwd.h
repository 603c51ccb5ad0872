// The body of the row-mapped blend backward (csrc/raster_blend_rows.hip), shared TEXTUALLY by its kernels: included inside
// blend_bwd_rows_kernel<ABS> (DET = false) and blend_bwd_rows_det_kernel<ABS> (DET = true), which declare ABS, DET and every
// name used below.  A textual include rather than an inlined device function: the default instances compile to exactly the
// device code they had before the DET instances existed.  Not a header in its own right: no include guard, no declarations.
    constexpr int NG = ABS ? RB_NGRAD + 2 : RB_NGRAD;
    constexpr int NPLANE = DET ? 4 : 1;
    // 22.6 KB of LDS per workgroup = seven workgroups per CU: two float4 per record plus its blue component (the third
    // float4 only carries cull extents the staging thread has in registers), no copy of the Gaussian ids (the flush reads
    // gid_sorted again)
    __shared__ float4 srec[RB_THREADS * 2];
    __shared__ float sblue[RB_THREADS];
    __shared__ float sacc[NPLANE][RB_THREADS][NG];
    __shared__ RbLists S;

    const int tile = (int)tile_order[blockIdx.x];        // longest lists first (tile_order_kernel)
    const uint32_t tlast = tile_last[tile];
    if (tlast == 0) return;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RbLane L = rb_lane(tx, ty, wave, lane);
    const bool inside = L.px < W && L.py < H;
    const float pxf = (float)L.px, pyf = (float)L.py;
    const uint2 range = ranges[tile];
    const size_t pix = (size_t)L.py * W + L.px, hw = (size_t)H * W;

    const float T_final = inside ? final_T[pix] : 0.f;
    const uint32_t my_last = inside ? n_contrib[pix] : 0u;
    uint32_t blk_last = my_last;       // maximum over the 16 lanes (pixels) of the row
    blk_last = max(blk_last, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)blk_last, 0xB1, 0xF, 0xF, false));
    blk_last = max(blk_last, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)blk_last, 0x4E, 0xF, 0xF, false));
    blk_last = max(blk_last, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)blk_last, 0x124, 0xF, 0xF, false));
    blk_last = max(blk_last, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)blk_last, 0x128, 0xF, 0xF, false));
    float T = T_final;
    float gr = 0.f, gg = 0.f, gb = 0.f;
    if (inside) { gr = dL_dout[pix]; gg = dL_dout[hw + pix]; gb = dL_dout[2 * hw + pix]; }
    const float bg_dot = bg[0] * gr + bg[1] * gg + bg[2] * gb;
    const float neg_bg_T = -T_final * bg_dot;
    float acc_dot = 0.f, last_cdot = 0.f, last_alpha = 0.f;       // scalar colour recurrence (see raster_blend.hip)

    const int nbatch = (int)((tlast + RB_THREADS - 1) / RB_THREADS);
    // the batch after the one being walked is fetched into registers before the walk starts (see the forward)
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    uint32_t pg = 0;
    {
        const uint32_t pos0 = (uint32_t)(nbatch - 1) * RB_THREADS + tid;
        if (pos0 < tlast) {
            pg = gid_sorted[range.x + pos0];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
        }
    }
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base_pos = (uint32_t)bi * RB_THREADS;
        const uint32_t pos = base_pos + tid;
        uint32_t m16 = 0;
        __syncthreads();   // previous batch fully flushed before LDS is reused
        if (pos < tlast) {
            srec[tid * 2] = p0;
            srec[tid * 2 + 1] = p1;
            sblue[tid] = p2.x;
            m16 = rb_block_mask(p0.x, p0.y, p2.y, p2.z, p2.w, tx * CGS_TILE, ty * CGS_TILE);
        } else {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            srec[tid * 2] = z; srec[tid * 2 + 1] = z; sblue[tid] = 0.f;
        }
        if (bi > 0) {      // every position of an earlier batch is < tlast
            pg = gid_sorted[range.x + pos - RB_THREADS];
            p0 = rec[3 * (size_t)pg]; p1 = rec[3 * (size_t)pg + 1]; p2 = rec[3 * (size_t)pg + 2];
        }
#pragma unroll
        for (int w = 0; w < NPLANE; ++w)
#pragma unroll
            for (int k = 0; k < NG; ++k) sacc[w][tid][k] = 0.f;
        S.smask[tid] = (uint16_t)m16;
        __syncthreads();

        {
            // entries behind the LAST contribution of every pixel of this 4x4 block (n_contrib: where the forward stopped)
            // cannot contribute to it: they never enter the block's list (the tile-wide bound `tlast` is the maximum over
            // 256 pixels, a block's own bound over 16)
            int i = (int)rb_list_build(S, L.blk, lane, (int)blk_last - (int)base_pos - 1) - 1;
            uint32_t e_next = S.list[L.blk][max(i, 0)];
            while (rb_ballot(i >= 0) != 0ull) {
                const bool has = i >= 0;
                const uint32_t e = e_next;
                i -= has ? 1 : 0;
                e_next = S.list[L.blk][max(i, 0)];                   // next entry's index: in flight during this iteration
                const uint32_t position = base_pos + e + 1u;         // 1-based
                const float4 r0 = srec[e * 2], r1 = srec[e * 2 + 1];
                const float blue = sblue[e];
                const RbEval ev = rb_eval(r0, r1, pxf, pyf);
                const bool act = has && (position <= my_last) && ev.hit;
                if (rb_ballot(act) == 0ull) continue;
                // Branch-free: a lane whose pixel takes no contribution runs the same updates on alpha = 0, G = 0, for which
                // every one of them is an exact no-op (T / 1 = T, w = 0, the colour recurrence with alpha = 0 hands on
                // the value the next contributing step would have computed) — two selects instead of a divergent block,
                // nine zero-initialisations and the moves that merge its results (the kernel is VALU-issue bound).
                const float alpha = act ? ev.alpha : 0.f, Gm = act ? ev.g : 0.f;
                const float om = 1.f - alpha;
                // 1/(1 - alpha), alpha <= 0.99: v_rcp_f32 + one Newton step (3 instructions, <= 1 ulp) for the background
                // term; T itself by the IEEE division: T is rebuilt over the whole list, and T * rcp (two roundings per
                // entry) drifted 5-8x further from fp64 than the oracle over 300+ entry lists
                float inv_om = __builtin_amdgcn_rcpf(om);
                inv_om = inv_om * fmaf(-om, inv_om, 2.f);
                T = T / om;
                const float w = alpha * T;
                acc_dot = fmaf(last_alpha, last_cdot, (1.f - last_alpha) * acc_dot);
                last_cdot = fmaf(r1.z, gr, fmaf(r1.w, gg, blue * gb));
                float dL_dalpha = (last_cdot - acc_dot) * T;
                last_alpha = alpha;
                dL_dalpha = fmaf(neg_bg_T, inv_om, dL_dalpha);
                const float gG = Gm * dL_dalpha;
                const float gx = gG * ev.dx, gy = gG * ev.dy;
                float v[RB_NGRAD];
                v[0] = gx;
                v[1] = gy;
                v[2] = gx * ev.dx;
                v[3] = gx * ev.dy;
                v[4] = gy * ev.dy;
                v[5] = gG;
                v[6] = w * gr;
                v[7] = w * gg;
                v[8] = w * gb;
                // transposing reduction inside each 16-lane row (identical to raster_blend.hip); every row then adds
                // into the accumulator of ITS OWN Gaussian
                const bool b0 = lane & 1, b1 = lane & 2;
                float a4[4], b2[2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float keep = b0 ? v[2 * q + 1] : v[2 * q], send = b0 ? v[2 * q] : v[2 * q + 1];
                    a4[q] = keep + rb_dpp<0xB1>(send);
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float keep = b1 ? a4[2 * q + 1] : a4[2 * q], send = b1 ? a4[2 * q] : a4[2 * q + 1];
                    b2[q] = keep + rb_dpp<0x4E>(send);
                }
                float c8;
                if constexpr (ABS) {
                    // third group of the transposing reduction: v[8], |d/d mean x|, |d/d mean y| and a free place end up
                    // in lanes 8..11 of the row (A, B, C = r0.z, r0.w, r1.x: the scaled conic of the record)
                    const float ax = fabsf(fmaf(2.f * r0.z, gx, r0.w * gy)), ay = fabsf(fmaf(2.f * r1.x, gy, r0.w * gx));
                    const float k0 = b0 ? ax : v[8], s0 = b0 ? v[8] : ax;
                    const float k1 = b0 ? 0.f : ay, s1 = b0 ? ay : 0.f;
                    const float t0 = k0 + rb_dpp<0xB1>(s0), t1 = k1 + rb_dpp<0xB1>(s1);
                    c8 = (b1 ? t1 : t0) + rb_dpp<0x4E>(b1 ? t0 : t1);
                } else {
                    c8 = v[8];
                    c8 += rb_dpp<0xB1>(c8);
                    c8 += rb_dpp<0x4E>(c8);
                }
                b2[0] += rb_dpp<0x124>(b2[0]); b2[0] += rb_dpp<0x128>(b2[0]);
                b2[1] += rb_dpp<0x124>(b2[1]); b2[1] += rb_dpp<0x128>(b2[1]);
                c8 += rb_dpp<0x124>(c8); c8 += rb_dpp<0x128>(c8);
                // keep the last three DPP additions in front of the predicated store: sunk into its exec-masked block
                // they split into a full-exec v_mov_dpp plus an add each (and a zero for the mov's `old` operand)
                asm volatile("" : "+v"(b2[0]), "+v"(b2[1]), "+v"(c8));
                const int sub = lane & 15;
                const float red = sub < 4 ? b2[0] : (sub < 8 ? b2[1] : c8);
                // (red != 0: a row whose 16 pixels took nothing from its entry — the wave goes on while ANY row has a contribution —
                //  would add nine zeros through the LDS float-atomic unit, the kernel's second bound: -6 %, same sums bit for bit;
                //  profiles/r05_blend_bwd_ablations.txt)
                if constexpr (DET) {
                    // rows 0..3 in turn into the wave's own plane (header comment): plain read-add-write, ordered by the fence
                    const bool add = has && sub < NG && red != 0.f;
                    float *const dst = &sacc[wave][e][sub < NG ? sub : 0];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (add && (lane >> 4) == r) *dst += red;
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                } else {
                    if (has && sub < NG && red != 0.f) atomicAdd(&sacc[0][e][sub], red);
                }
            }
        }
        __syncthreads();
        if (pos < tlast) {
            float a0, a1, a2, a3, a4, a5, a6, a7, a8;
            float a9 = 0.f, a10 = 0.f;       // the two absolute sums (>= 0)
            if constexpr (DET) {
                float a[NG];
#pragma unroll
                for (int k = 0; k < NG; ++k) a[k] = ((sacc[0][tid][k] + sacc[1][tid][k]) + sacc[2][tid][k]) + sacc[3][tid][k];
                a0 = a[0]; a1 = a[1]; a2 = a[2]; a3 = a[3]; a4 = a[4]; a5 = a[5]; a6 = a[6]; a7 = a[7]; a8 = a[8];
                if constexpr (ABS) { a9 = a[NG - 2]; a10 = a[NG - 1]; }
            } else {
                a0 = sacc[0][tid][0]; a1 = sacc[0][tid][1]; a2 = sacc[0][tid][2]; a3 = sacc[0][tid][3];
                a4 = sacc[0][tid][4]; a5 = sacc[0][tid][5]; a6 = sacc[0][tid][6]; a7 = sacc[0][tid][7];
                a8 = sacc[0][tid][8];
                if constexpr (ABS) { a9 = sacc[0][tid][NG - 2]; a10 = sacc[0][tid][NG - 1]; }
            }
            if (a0 != 0.f || a1 != 0.f || a2 != 0.f || a3 != 0.f || a4 != 0.f || a5 != 0.f || a6 != 0.f ||
                a7 != 0.f || a8 != 0.f || a9 != 0.f || a10 != 0.f) {
                const uint32_t g = gid_sorted[range.x + pos];
                const float4 q0 = srec[tid * 2], q1 = srec[tid * 2 + 1];
                const float cC = q1.x, op = q1.y;
                if constexpr (DET) {
                    const uint2 rc = rect[g];
                    const int x0 = (int)(rc.x & 0xFFFFu), y0 = (int)(rc.x >> 16), x1 = (int)(rc.y & 0xFFFFu);
                    const uint64_t slot = (uint64_t)slot_base[g] + (uint64_t)((ty - y0) * (x1 - x0) + (tx - x0));
                    if (slot < slot_cap) {       // (always, with the view's own rectangles and a capacity >= its pair count)
                        float4 *const dst = slots + 3 * slot;
                        dst[0] = make_float4(op * fmaf(2.f * q0.z, a0, q0.w * a1) * RB_INV_LOG2E,
                                             op * fmaf(2.f * cC, a1, q0.w * a0) * RB_INV_LOG2E, -0.5f * op * a2, -op * a3);
                        dst[1] = make_float4(-0.5f * op * a4, a5, a6, a7);
                        dst[2] = make_float4(a8, op * a9 * RB_INV_LOG2E, op * a10 * RB_INV_LOG2E, 0.f);
                    }
                } else {
                    atomicAdd(&dL_dmean2D_px[2 * (size_t)g], op * fmaf(2.f * q0.z, a0, q0.w * a1) * RB_INV_LOG2E);
                    atomicAdd(&dL_dmean2D_px[2 * (size_t)g + 1], op * fmaf(2.f * cC, a1, q0.w * a0) * RB_INV_LOG2E);
                    atomicAdd(&dL_dconic[3 * (size_t)g], -0.5f * op * a2);
                    atomicAdd(&dL_dconic[3 * (size_t)g + 1], -op * a3);
                    atomicAdd(&dL_dconic[3 * (size_t)g + 2], -0.5f * op * a4);
                    atomicAdd(&dL_dopacity[g], a5);
                    atomicAdd(&dL_dcolors[3 * (size_t)g], a6);
                    atomicAdd(&dL_dcolors[3 * (size_t)g + 1], a7);
                    atomicAdd(&dL_dcolors[3 * (size_t)g + 2], a8);
                    if constexpr (ABS) {
                        if (a9 != 0.f) atomicAdd(&dL_dabs_px[2 * (size_t)g], op * a9 * RB_INV_LOG2E);
                        if (a10 != 0.f) atomicAdd(&dL_dabs_px[2 * (size_t)g + 1], op * a10 * RB_INV_LOG2E);
                    }
                }
            }
        }
    }
