// lit_decode_body.h -- the body of lit_decode_kernel (lit_kernels.hip), included once per overload of the kernel, as
// lit_model_encode_body.h is: behind `extern __shared__ uint8_t lds[]` and `constexpr bool WIDE`.  No include guard.
#ifndef DIVANS_LIT_KERNEL_BODY
#error "this file is the body of lit_decode_kernel: lit_kernels.hip includes it inside that kernel and nothing else may"
#endif
    static_assert(!WIDE || (!CTXC && SEG), "the wide layout: segment lists over a context map that is not constant");
    const LdsView lv = load_config_to_lds<MM, CTXC, WIDE>(lds, b);
    const LitGeometry& g = b.geom;
    const int lane = threadIdx.x & 63, li = lane & 15, rbase = lane & 48;
    const uint32_t gg = blockIdx.x * (LIT_THREADS / 16) + (threadIdx.x >> 4);
    const uint32_t G = gridDim.x * (LIT_THREADS / 16);
    const Table<CACHE> tb = make_table<CACHE>(b, lds, li);
    for (uint32_t s = gg; s < b.n_streams; s += G) {
        const uint32_t len = b.out_sizes ? b.out_sizes[s] : b.stream_len;
        uint8_t* out = b.out + (b.out_offsets ? b.out_offsets[s] : (uint64_t)s * b.stream_len);
        WordWindow ww;
        ww.in = (const uint32_t*)(b.in + b.in_offsets[s]);
        ww.nwords = b.in_sizes[s] >> 2;
        ww.start(li);
        if (!b.resume) init_table(tb, g.total_rows, li);
        WeightsPair wp; wp.init();
        if (MIX && b.resume) { const int32_t* p = b.wstate + (li < 8 ? 0 : 3); wp.w.w0 = p[0]; wp.w.w1 = p[1]; wp.w.norm = p[2]; }
        int nh = wp.norm_high(), nl = wp.norm_low();     // normalized_weight of model_weights[1] (high nibble) / [0] (low nibble)
        uint64_t last8 = 0;
        uint32_t ctab = WIDE ? LIT_BLOB_CMAP : LIT_BLOB_CTXF;      // context table of the current literal block type
        SegCursor sc;
        if (SEG) sc.start<WIDE>(b, s, last8, ctab);
        uint32_t k1 = CTXC ? 0u : lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];
        uint64_t SA = 0, SB = 0;      // state_a decodes high nibbles, state_b low nibbles (two symbols per byte)
        bool corrupt = false;
        uint32_t ctx_cur = context_of<CTXC, WIDE>(g, lv.ctx, ctab, (uint32_t)(last8 >> 56), k1);
        FetchedRow rowH = {};
        if (!MIX) rowH = fetch_row<true, MM, CACHE>(g, lv, tb, ctx_cur, last8, 0u);
        for (uint32_t cbeg = 0; cbeg < len; cbeg += 32768u) {
            // start of a 65 536-symbol chunk: 16 bytes = state_a, state_b (ans.rs:174-186)
            {
                uint32_t a0 = ww.next(li, rbase), a1 = ww.next(li, rbase), b0 = ww.next(li, rbase), b1 = ww.next(li, rbase);
                SA = ((uint64_t)a1 << 32) | a0;
                SB = ((uint64_t)b1 << 32) | b0;
            }
            const uint32_t cend = cbeg + 32768u < len ? cbeg + 32768u : len;
            for (uint32_t base = cbeg; base < cend; base += 16u) {
                const uint32_t cnt = cend - base < 16u ? cend - base : 16u;
                uint32_t outb = 0;
                for (uint32_t k = 0; k < cnt; ++k) {
                    if (MIX) {
                        const uint32_t prev = (uint32_t)(last8 >> 56);
                        const uint32_t ctx = context_of<CTXC, WIDE>(g, lv.ctx, ctab, prev, k1);
                        if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + prev];
                        // a state that dropped below 2^31 takes 4 more bytes right before it is used again (ans.rs:432-440)
                        if (SA < (1ull << 31)) SA = (SA << 32) | ww.next(li, rbase);
                        uint32_t fh = 0, fl = 0, ph = 0, pl = 0;
                        const uint32_t hi = decode_nibble<true, MM, MIX, CACHE>(g, lv, tb, li, rbase, ctx, last8, 0u, SA, nh, fh, ph);
                        if (SB < (1ull << 31)) SB = (SB << 32) | ww.next(li, rbase);
                        const uint32_t lo = decode_nibble<false, MM, MIX, CACHE>(g, lv, tb, li, rbase, ctx, last8, hi, SB, nl, fl, pl);
                        wp.update(li, fh, ph, fl, pl);
                        nh = wp.norm_high(); nl = wp.norm_low();
                        const uint32_t byte = (hi << 4) | lo;
                        last8 = (last8 >> 8) | ((uint64_t)byte << 56);
                        if (SEG) {
                            if (--sc.left == 0u) {
                                sc.advance<WIDE>(g, last8, ctab);
                                if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];
                            }
                        }
                        outb = (uint32_t)li == k ? byte : outb;
                    } else {
                        // rowH (this byte's high-nibble row) was requested while the previous byte was being finished
                        if (SA < (1ull << 31)) SA = (SA << 32) | ww.next(li, rbase);
                        const int cvh = rowH.is_default ? 4 * (li + 1) : rowH.value;
                        const uint32_t hi = (uint32_t)search_symbol(cvh, (uint32_t)SA & 0x7fffu, rbase);
                        const FetchedRow rowL = fetch_row<false, MM, CACHE>(g, lv, tb, ctx_cur, last8, hi);
                        finish_nibble<CACHE>(g, tb, li, rbase, rowH, cvh, (int)hi, SA);
                        if (SB < (1ull << 31)) SB = (SB << 32) | ww.next(li, rbase);
                        const int cvl = rowL.is_default ? 4 * (li + 1) : rowL.value;
                        const uint32_t lo = (uint32_t)search_symbol(cvl, (uint32_t)SB & 0x7fffu, rbase);
                        const uint32_t byte = (hi << 4) | lo;
                        last8 = (last8 >> 8) | ((uint64_t)byte << 56);
                        if (SEG) { if (--sc.left == 0u) sc.advance<WIDE>(g, last8, ctab); }
                        if (!CTXC) k1 = lv.ctx[LIT_BLOB_LUT1CLASS + (uint32_t)((last8 >> 48) & 0xffu)];
                        ctx_cur = context_of<CTXC, WIDE>(g, lv.ctx, ctab, (uint32_t)(last8 >> 56), k1);
                        rowH = fetch_row<true, MM, CACHE>(g, lv, tb, ctx_cur, last8, 0u);   // next byte's row (harmless past the end)
                        finish_nibble<CACHE>(g, tb, li, rbase, rowL, cvl, (int)lo, SB);
                        outb = (uint32_t)li == k ? byte : outb;
                    }
                }
                if ((uint32_t)li < cnt) __builtin_nontemporal_store((uint8_t)outb, out + base + li);
            }
            // rANS is an exact inverse: a chunk that was coded from the start states 2^31 (ans.rs:135-136,331-378) decodes back
            // to exactly those; anything else means a truncated, corrupt or mismatched stream (the reference would stall on
            // NeedsMoreInput or fail its checksum)
            corrupt |= (SA != (1ull << 31)) | (SB != (1ull << 31));
        }
        if (SEG && li == 0) sc.finish();
        if (b.consumed) { corrupt |= ww.pos > ww.nwords; if (li == 0) b.consumed[s] = ww.pos; }
        else corrupt |= ww.pos != ww.nwords;     // every coded word consumed, none read past the end
        if (MIX && b.wstate && (li & 7) == 0) {   // lanes 0 and 8 of the row hold the two Weights objects
            int32_t* p = b.wstate + (li ? 3 : 0);
            p[0] = wp.w.w0; p[1] = wp.w.w1; p[2] = wp.w.norm;
        }
        if (g.wrap_check) {     // the encoder of this stream coded with a row whose i16 total had wrapped: whatever it wrote, it is not these bytes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);
            corrupt |= wrap_scan<CACHE>(g, tb, li, rbase);
        }
        if (corrupt && li == 0) {
            if (b.status) atomicOr(b.status, LIT_STATUS_BAD_STREAM);
            if (b.stream_bad) b.stream_bad[s] = 1;
        }
    }
