// lit_model_encode_body.h -- the body of lit_model_encode_kernel (lit_kernels.hip), included once per overload of the kernel: inside
// `template <int MM, bool CTXC, bool MIX, int CACHE, bool SEG[, int]> __global__ void lit_model_encode_kernel(const LitBatch b)` behind
// `extern __shared__ uint8_t lds[]` and `constexpr bool WIDE` (the context tables are in the second layout, lit_kernels.h).  Text, not a
// function: as a __device__ function called from both kernels the body compiled to other code than the kernel it was
// (scripts/isa_compare.py), and the instances that exist keep theirs.  No include guard.
#ifndef DIVANS_LIT_KERNEL_BODY
#error "this file is the body of lit_model_encode_kernel: lit_kernels.hip includes it inside that kernel and nothing else may"
#endif
    static_assert(!WIDE || (!CTXC && SEG), "the wide layout: segment lists over a context map that is not constant");
    const LdsView lv = load_config_to_lds<MM, CTXC, WIDE>(lds, b);
    const LitGeometry& g = b.geom;
    const int lane = threadIdx.x & 63, li = lane & 15, rbase = lane & 48;
    const uint32_t gg = blockIdx.x * (LIT_THREADS / 16) + (threadIdx.x >> 4);
    const uint32_t G = gridDim.x * (LIT_THREADS / 16);
    const Table<CACHE> tb = make_table<CACHE>(b, lds, li);
    for (uint32_t s = gg; s < b.n_streams; s += G) {
        const uint8_t* in = b.in + (b.in_offsets ? b.in_offsets[s] : (uint64_t)s * b.stream_len);
        const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
        uint32_t* sf = b.sf + (size_t)s * 2u * b.max_stream_len;
        if (!b.resume) init_table(tb, g.total_rows, li);
        WeightsPair wp; wp.init();
        if (MIX && b.resume) { const int32_t* p = b.wstate + (li < 8 ? 0 : 3); wp.w.w0 = p[0]; wp.w.w1 = p[1]; wp.w.norm = p[2]; }
        int nh = wp.norm_high(), nl = wp.norm_low();     // normalized_weight of model_weights[1] (high nibble) / [0] (low nibble)
        uint64_t last8 = 0;
        uint32_t ctab = WIDE ? LIT_BLOB_CMAP : LIT_BLOB_CTXF;      // context table of the current literal block type
        SegCursor sc;
        if (SEG) sc.start<WIDE>(b, s, last8, ctab);
        uint32_t k1 = CTXC ? 0u : lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];   // lut1 class of prev_prev
        // each lane holds one literal byte of the current and of the next 16-byte window (coalesced reads)
        uint32_t mine = ((uint32_t)li < len) ? in[li] : 0u;
        uint32_t nxt = (16u + li < len) ? in[16u + li] : 0u;
        // Non-mixing path: every symbol is known, so each row is requested one nibble ahead (right after the previous
        // row of the SAME table has been stored) and the model math of one nibble runs under the fetch of the next.
        uint32_t cur = (uint32_t)row_gather((int)mine, rbase, 0);
        uint32_t ctx_cur = context_of<CTXC, WIDE>(g, lv.ctx, ctab, (uint32_t)(last8 >> 56), k1);
        FetchedRow rowH = {}, rowL = {};
        if (!MIX) {
            rowH = fetch_row<true, MM, CACHE>(g, lv, tb, ctx_cur, last8, 0u);
            rowL = fetch_row<false, MM, CACHE>(g, lv, tb, ctx_cur, last8, cur >> 4);
        }
        for (uint32_t base = 0; base < len; base += 16) {
            const uint32_t cnt = len - base < 16u ? len - base : 16u;
            uint32_t pend_a = 0, pend_b = 0;  // lane k keeps the two pairs of byte base+k
            for (uint32_t k = 0; k < cnt; ++k) {
                if (MIX) {
                    const uint32_t byte = (uint32_t)row_gather((int)mine, rbase, (int)k);
                    const uint32_t prev = (uint32_t)(last8 >> 56);
                    const uint32_t ctx = context_of<CTXC, WIDE>(g, lv.ctx, ctab, prev, k1);
                    if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + prev];
                    const uint32_t hi = byte >> 4, lo = byte & 15u;
                    uint32_t fh = 0, fl = 0;
                    const uint32_t ph = model_nibble<true, MM, MIX, CACHE>(g, lv, tb, li, rbase, ctx, last8, 0u, (int)hi, nh, fh);
                    const uint32_t pl = model_nibble<false, MM, MIX, CACHE>(g, lv, tb, li, rbase, ctx, last8, hi, (int)lo, nl, fl);
                    wp.update(li, fh, ph >> 16, fl, pl >> 16);
                    nh = wp.norm_high(); nl = wp.norm_low();
                    last8 = (last8 >> 8) | ((uint64_t)byte << 56);
                    if (SEG) {   // the next Literal command starts from the ring buffer's last 8 bytes and its own block type
                        if (--sc.left == 0u) {
                            sc.advance<WIDE>(g, last8, ctab);
                            if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];
                        }
                    }
                    pend_a = (uint32_t)li == k ? ph : pend_a;
                    pend_b = (uint32_t)li == k ? pl : pend_b;
                } else {
                    const uint32_t byte = cur;
                    const uint32_t nb = (uint32_t)row_gather((int)(k + 1u < 16u ? mine : nxt), rbase, (int)((k + 1u) & 15u));
                    const uint32_t ph = model_finish<CACHE>(g, tb, li, rbase, rowH, (int)(byte >> 4));
                    last8 = (last8 >> 8) | ((uint64_t)byte << 56);
                    if (SEG) { if (--sc.left == 0u) sc.advance<WIDE>(g, last8, ctab); }
                    if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];
                    ctx_cur = context_of<CTXC, WIDE>(g, lv.ctx, ctab, (uint32_t)(last8 >> 56), k1);
                    rowH = fetch_row<true, MM, CACHE>(g, lv, tb, ctx_cur, last8, 0u);           // next byte's high row
                    const uint32_t pl = model_finish<CACHE>(g, tb, li, rbase, rowL, (int)(byte & 15u));
                    rowL = fetch_row<false, MM, CACHE>(g, lv, tb, ctx_cur, last8, nb >> 4);     // next byte's low row
                    cur = nb;
                    pend_a = (uint32_t)li == k ? ph : pend_a;
                    pend_b = (uint32_t)li == k ? pl : pend_b;
                }
            }
            // nibble index of byte (base+li) is 2*(base+li): each lane stores its two pairs (8 B; 128 B coalesced per row)
            if ((uint32_t)li < cnt) {
                u32x2 v = {pend_a, pend_b};   // written once, read once by the rANS kernel: keep it out of the L2's way
                __builtin_nontemporal_store(v, (u32x2*)(sf + 2u * (size_t)(base + li)));
            }
            mine = nxt;
            nxt = (base + 32u + li < len) ? in[base + 32u + li] : 0u;
        }
        if (SEG && li == 0) sc.finish();
        if (MIX && b.wstate && (li & 7) == 0) {   // lanes 0 and 8 of the row hold the two Weights objects
            int32_t* p = b.wstate + (li ? 3 : 0);
            p[0] = wp.w.w0; p[1] = wp.w.w1; p[2] = wp.w.norm;
        }
        if (g.wrap_check) {     // a speed under which a row total can leave i16: say so if one did and was coded with again
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);
            if (wrap_scan<CACHE>(g, tb, li, rbase) && li == 0) {
                if (b.status) atomicOr(b.status, LIT_STATUS_BAD_MODEL);
                if (b.stream_bad) b.stream_bad[s] = 1;
            }
        }
    }
